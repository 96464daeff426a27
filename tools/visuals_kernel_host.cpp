// Host build of the kernel bodies of fear_draw_boxes_u8 and fear_miner_update (feartracker_amd/csrc/fear_train_visuals.h) for the
// sanitizers: one thread per lane, a pthread barrier for the workgroup's sync, one workgroup after the other — the drawing workgroups in
// FALLING box order, the worst order there is for "the last box wins".  Three modes:
//   draw LANES CASE OUT     case: int32 n_frames, K, thickness | n_frames x (int32 h, w) | the frames' bytes | boxes (K, 4) int32 |
//                           frame_of (K) int32 | colours (K, 3) uint8.  Writes the frames' bytes after the call.
//   render LANES CASE OUT   case: int32 B, n | template (B,3,128,128) fp32 | search (B,3,256,256) fp32 | pred (n, 4) int32 | gt_box (B, 4)
//                           int32 | visible (B) int32.  Writes the (n 256, 384, 3) sheet.
//   decide LANES CASE OUT   case: int32 mode_max, count | float64 min_delta | float64 scores (count).  Writes the state after every score.
// Every buffer is a heap block of exactly its size, so AddressSanitizer sees an access outside.  tools/visuals_kernel_host_check.py builds
// it with -fsanitize=address,undefined, feeds it the operator cases of the tests and compares with the numpy forms.
#include <pthread.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

static pthread_barrier_t g_barrier;
#define FEAR_VIS_DEV static inline
#define FEAR_VIS_SYNC() pthread_barrier_wait(&g_barrier)
#define FEAR_VIS_HOST 1
#include "../feartracker_amd/csrc/fear_train_visuals.h"
#include "../include/fear_train.h"

static_assert(sizeof(FearMinerState) == sizeof(VisMinerState) && offsetof(FearMinerState, pred) == offsetof(VisMinerState, pred), "one state");
static_assert(sizeof(fear_frame) == sizeof(VisFrame), "one frame record");

static bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

template <typename T>
static T* take(FILE* f, size_t count) {                    // a heap block of exactly count values, read from the case
    T* p = (T*)malloc(count ? count * sizeof(T) : 1);
    if (!read_all(f, p, count * sizeof(T))) { fprintf(stderr, "short case file\n"); exit(3); }
    return p;
}

template <typename F>
static void workgroup(int lanes, F body) {
    std::vector<std::thread> pool;
    for (int t = 0; t < lanes; ++t) pool.emplace_back([=] { body(t); });
    for (auto& th : pool) th.join();
}

static int draw(int lanes, FILE* f, FILE* out) {
    int32_t* hdr = take<int32_t>(f, 3);
    const int n_frames = hdr[0], K = hdr[1], t = hdr[2];
    if (K < 0 || K > 65535 || n_frames < 0 || t < 1 || t > 32) return 3;           // (fear_draw_boxes_u8's own check)
    int32_t* hw = take<int32_t>(f, 2 * (size_t)n_frames);
    VisFrame* frames = (VisFrame*)malloc(n_frames ? n_frames * sizeof(VisFrame) : 1);
    for (int i = 0; i < n_frames; ++i) {
        frames[i].h = hw[2 * i]; frames[i].w = hw[2 * i + 1];
        frames[i].data = take<unsigned char>(f, (size_t)frames[i].h * frames[i].w * 3);
    }
    int32_t* boxes = take<int32_t>(f, 4 * (size_t)K);
    int32_t* frame_of = take<int32_t>(f, K);
    unsigned char* colours = take<unsigned char>(f, 3 * (size_t)K);
    for (int wg = 4 * K - 1; wg >= 0; --wg) {               // the LAST box first: a pixel an earlier box fails to skip stays wrong
        VisShared* sh = (VisShared*)malloc(sizeof(VisShared));
        memset(sh, 0xA5, sizeof(VisShared));                // (what LDS holds is not defined)
        workgroup(lanes, [=](int tid) { vis_draw_side(frames, n_frames, boxes, frame_of, colours, K, t, wg >> 2, wg & 3, *sh, tid, lanes); });
        free(sh);
    }
    for (int i = 0; i < n_frames; ++i) {
        const size_t bytes = (size_t)frames[i].h * frames[i].w * 3;
        if (fwrite(frames[i].data, 1, bytes, out) != bytes) return 4;
        free(frames[i].data);
    }
    free(hdr); free(hw); free(frames); free(boxes); free(frame_of); free(colours);
    return 0;
}

static int render(int lanes, FILE* f, FILE* out) {
    int32_t* hdr = take<int32_t>(f, 2);
    const int B = hdr[0], n = hdr[1];
    if (B < 1 || n < 1 || n > B || n > kVisMaxImages) return 3;
    float* templ = take<float>(f, (size_t)B * 3 * kVisTmpl * kVisTmpl);
    float* search = take<float>(f, (size_t)B * 3 * kVisSearch * kVisSearch);
    int32_t* pred = take<int32_t>(f, 4 * (size_t)n);
    int32_t* gt = take<int32_t>(f, 4 * (size_t)B);
    int32_t* visible = take<int32_t>(f, B);
    const size_t bytes = (size_t)n * kVisItemH * kVisSheetW * 3;
    unsigned char* sheet = (unsigned char*)malloc(bytes);
    memset(sheet, 0x5A, bytes);                             // (every byte of the sheet must be written)
    for (int k = 0; k < n; ++k)
        for (int tile = 0; tile < kVisItemH / kVisTileRows; ++tile)
            workgroup(lanes, [=](int tid) { vis_render_tile(templ, search, pred, gt, visible, k, tile, sheet, tid, lanes); });
    if (fwrite(sheet, 1, bytes, out) != bytes) return 4;
    free(hdr); free(templ); free(search); free(pred); free(gt); free(visible); free(sheet);
    return 0;
}

static int decide(FILE* f, FILE* out) {
    int32_t* hdr = take<int32_t>(f, 2);
    double* min_delta = take<double>(f, 1);
    double* scores = take<double>(f, hdr[1]);
    VisMinerState* st = (VisMinerState*)calloc(1, sizeof(VisMinerState));
    for (int i = 0; i < hdr[1]; ++i) {
        vis_miner_decide(st, scores[i], hdr[0], *min_delta, i);
        if (fwrite(st, 1, sizeof(VisMinerState), out) != sizeof(VisMinerState)) return 4;
    }
    free(hdr); free(min_delta); free(scores); free(st);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: %s draw|render|decide LANES CASE OUT\n", argv[0]); return 2; }
    const int lanes = atoi(argv[2]);
    if (lanes < 8 || lanes > kVisThreads || lanes % 8) { fprintf(stderr, "LANES: a multiple of 8 up to %d\n", kVisThreads); return 2; }
    FILE* f = fopen(argv[3], "rb");
    FILE* out = fopen(argv[4], "wb");
    if (!f || !out) return 3;
    pthread_barrier_init(&g_barrier, nullptr, lanes);
    const int rc = !strcmp(argv[1], "draw") ? draw(lanes, f, out) : !strcmp(argv[1], "render") ? render(lanes, f, out) :
                   !strcmp(argv[1], "decide") ? decide(f, out) : 2;
    fclose(f);
    fclose(out);
    pthread_barrier_destroy(&g_barrier);
    return rc;
}
