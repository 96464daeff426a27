// Host build of fear_glass_u8's kernel body (feartracker_amd/csrc/fear_train_glass.h) for the sanitizers: one thread per lane, a pthread
// barrier for the workgroup's sync, one workgroup after the other.  Reads a case file
//   int32 n, H, W | crops (n, H, W, 3) uint8 | ops (n) FearPhotoOp
// and writes the (n, H, W, 3) uint8 result; every buffer is a heap block of exactly its size, so AddressSanitizer sees an access outside.
// tools/glass_kernel_host_check.py builds it with -fsanitize=address,undefined, feeds it the operator cases of tests/test_glass_gpu.py
// and compares with train_data.glass_u8_host.
#include <pthread.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

static pthread_barrier_t g_barrier;
#define FEAR_GL_DEV static inline
#define FEAR_GL_SYNC() pthread_barrier_wait(&g_barrier)
#include "../feartracker_amd/csrc/fear_train_glass.h"
#include "../include/fear_train.h"

static_assert(FEAR_PHOTO_BLUR_GLASS == kGlassBlur, "one kind");

static bool read_all(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s LANES CASE OUT\n", argv[0]); return 2; }
    const int lanes = atoi(argv[1]);
    FILE* f = fopen(argv[2], "rb");
    int32_t hdr[3];
    if (!f || !read_all(f, hdr, sizeof hdr)) return 3;
    const int n = hdr[0], H = hdr[1], W = hdr[2];
    if (H < 4 || W < 4 || (H & 1) || (W & 1) || H > FEAR_HLS_MAX_SIDE || W > FEAR_HLS_MAX_SIDE) return 3;   // (fear_glass_u8's own check)
    const size_t bytes = (size_t)H * W * 3;
    uint8_t* in = (uint8_t*)malloc(n * bytes);
    uint8_t* out = (uint8_t*)malloc(n * bytes);
    FearPhotoOp* ops = (FearPhotoOp*)malloc(n * sizeof(FearPhotoOp));
    if (!read_all(f, in, n * bytes) || !read_all(f, ops, n * sizeof(FearPhotoOp))) return 3;
    fclose(f);
    pthread_barrier_init(&g_barrier, nullptr, lanes);
    for (int crop = 0; crop < n; ++crop)
        for (int ty = 0; ty < H; ty += kGlTile)
            for (int tx = 0; tx < W; tx += kGlTile) {
                GlassShared* sh = (GlassShared*)malloc(sizeof(GlassShared));
                memset(sh, 0xA5, sizeof(GlassShared));        // (what LDS holds is not defined: no offset, and a pixel that shows)
                const GlassTile tile{tx, ty, H, W};
                const FearPhotoOp op = ops[crop];
                std::vector<std::thread> pool;
                for (int t = 0; t < lanes; ++t)
                    pool.emplace_back([=] {
                        glass_tile(in + crop * bytes, out + crop * bytes, tile, op.blur == kGlassBlur, op.key[0], op.key[1], *sh, t, lanes);
                    });
                for (auto& th : pool) th.join();
                free(sh);
            }
    f = fopen(argv[3], "wb");
    if (!f || fwrite(out, 1, n * bytes, f) != n * bytes) return 4;
    fclose(f);
    free(in); free(out); free(ops);
    return 0;
}
