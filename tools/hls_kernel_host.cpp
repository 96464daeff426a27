// Host build of fear_hls_u8's kernel body (feartracker_amd/csrc/fear_train_hls.h) for the sanitizers: one thread per lane, a pthread
// barrier for the workgroup's sync, relaxed atomics for the LDS atomics.  Reads a case file
//   int32 n, H, W, m | crops (n, H, W, 3) uint8 | ops (n) FearHlsOp | segments (m, 4) int16 | qtable (4096) fp32 | exp_table (1025) float64
// and writes the (n, H, W, 3) uint8 result; every buffer is a heap block of exactly its size, so AddressSanitizer sees an access outside.
// tools/hls_kernel_host_check.py builds it with -fsanitize=address,undefined, feeds it the operator cases of tests/test_hls_gpu.py and
// compares with train_data.hls_u8_host.
#include <pthread.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

static pthread_barrier_t g_barrier;
#define FEAR_HL_DEV static inline
#define FEAR_HL_SYNC() pthread_barrier_wait(&g_barrier)
#define FEAR_HL_ATOMIC_ADD(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)
#define FEAR_HL_ATOMIC_OR(p, v) __atomic_fetch_or((p), (v), __ATOMIC_RELAXED)
#include "../feartracker_amd/csrc/fear_train_hls.h"
#include "../include/fear_train.h"

static_assert(sizeof(HlsOp) == sizeof(FearHlsOp), "one layout");

static bool read_all(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s LANES CASE OUT\n", argv[0]); return 2; }
    const int lanes = atoi(argv[1]);
    FILE* f = fopen(argv[2], "rb");
    int32_t hdr[4];
    if (!f || !read_all(f, hdr, sizeof hdr)) return 3;
    const int n = hdr[0], H = hdr[1], W = hdr[2], m = hdr[3];
    if (H > FEAR_HLS_MAX_SIDE || W > FEAR_HLS_MAX_SIDE) return 3;          // (fear_hls_u8's own check)
    const size_t bytes = (size_t)H * W * 3;
    uint8_t* in = (uint8_t*)malloc(n * bytes);
    uint8_t* out = (uint8_t*)malloc(n * bytes);
    HlsOp* ops = (HlsOp*)malloc(n * sizeof(HlsOp));
    int16_t* seg = (int16_t*)malloc((size_t)m * 4 * sizeof(int16_t));
    float* q = (float*)malloc(FEAR_PHOTO_QUANTILES * sizeof(float));
    double* et = (double*)malloc(FEAR_HLS_EXP_ENTRIES * sizeof(double));
    if (!read_all(f, in, n * bytes) || !read_all(f, ops, n * sizeof(HlsOp)) || !read_all(f, seg, (size_t)m * 4 * sizeof(int16_t)) ||
        !read_all(f, q, FEAR_PHOTO_QUANTILES * sizeof(float)) || !read_all(f, et, FEAR_HLS_EXP_ENTRIES * sizeof(double))) return 3;
    fclose(f);
    pthread_barrier_init(&g_barrier, nullptr, lanes);
    for (int crop = 0; crop < n; ++crop) {
        HlsShared* sh = (HlsShared*)malloc(sizeof(HlsShared));               // (uninitialised, as LDS is)
        std::vector<std::thread> pool;
        for (int t = 0; t < lanes; ++t)
            pool.emplace_back([=] { hls_crop(in + crop * bytes, out + crop * bytes, H, W, ops + crop, seg, q, et, *sh, t, lanes); });
        for (auto& th : pool) th.join();
        free(sh);
    }
    f = fopen(argv[3], "wb");
    if (!f || fwrite(out, 1, n * bytes, f) != n * bytes) return 4;
    fclose(f);
    free(in); free(out); free(ops); free(seg); free(q); free(et);
    return 0;
}
