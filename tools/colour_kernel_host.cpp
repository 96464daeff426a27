// Host build of fear_colour_u8's kernel body (feartracker_amd/csrc/fear_train_colour.h) for the sanitizers: one thread per lane, a
// pthread barrier for the workgroup's sync, a relaxed atomic add for the LDS atomics.  Reads a case file
//   int32 n, H, W | crops (n, H, W, 3) uint8 | ops (n) FearColourOp | aux (n, 3, 256) uint8
// and writes the (n, H, W, 3) uint8 result; every buffer is a heap block of exactly its size, so AddressSanitizer sees an access outside.
// tools/colour_kernel_host_check.py builds it with -fsanitize=address,undefined, feeds it the operator cases of tests/test_colour_gpu.py
// and compares with train_data.colour_u8_host.
#include <pthread.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

static pthread_barrier_t g_barrier;
#define FEAR_CL_DEV static inline
#define FEAR_CL_SYNC() pthread_barrier_wait(&g_barrier)
#define FEAR_CL_ATOMIC_ADD(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)
#include "../feartracker_amd/csrc/fear_train_colour.h"
#include "../include/fear_train.h"

static_assert(sizeof(ColourOp) == sizeof(FearColourOp), "one layout");

static bool read_all(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s LANES CASE OUT\n", argv[0]); return 2; }
    const int lanes = atoi(argv[1]);
    FILE* f = fopen(argv[2], "rb");
    int32_t hdr[3];
    if (!f || !read_all(f, hdr, sizeof hdr)) return 3;
    const int n = hdr[0], H = hdr[1], W = hdr[2];
    const size_t bytes = (size_t)H * W * 3;
    uint8_t* in = (uint8_t*)malloc(n * bytes);
    uint8_t* out = (uint8_t*)malloc(n * bytes);
    ColourOp* ops = (ColourOp*)malloc(n * sizeof(ColourOp));
    uint8_t* aux = (uint8_t*)malloc((size_t)n * 768);
    if (!read_all(f, in, n * bytes) || !read_all(f, ops, n * sizeof(ColourOp)) || !read_all(f, aux, (size_t)n * 768)) return 3;
    fclose(f);
    pthread_barrier_init(&g_barrier, nullptr, lanes);
    for (int crop = 0; crop < n; ++crop) {
        ColourShared* sh = (ColourShared*)malloc(sizeof(ColourShared));      // (uninitialised, as LDS is)
        std::vector<std::thread> pool;
        for (int t = 0; t < lanes; ++t)
            pool.emplace_back([=] { colour_crop(in + crop * bytes, out + crop * bytes, H, W, ops + crop, aux + (size_t)crop * 768, *sh, t, lanes); });
        for (auto& th : pool) th.join();
        free(sh);
    }
    f = fopen(argv[3], "wb");
    if (!f || fwrite(out, 1, n * bytes, f) != n * bytes) return 4;
    fclose(f);
    free(in); free(out); free(ops); free(aux);
    return 0;
}
