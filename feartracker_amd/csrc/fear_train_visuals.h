// fear_train_visuals.h — pictures made on the device: fear_draw_boxes_u8, rectangles drawn into uint8 frames in a
// defined order, and fear_miner_update, the reference's BestWorstMinerCallback (model_training/train/callbacks.py:95-230) with
// FEARLightningModel.get_visuals (train/fear_lightning_model.py:217-258) behind it: the step's score is compared with the best and the
// worst kept so far ON THE DEVICE, and only a step that is a new best or worst renders its batch into that side's sheet.
//
// One band test, vis_in_band, serves both: pixel (px, py) belongs to a box's outline of thickness t iff it lies in the outer rectangle
// [x0 - o, x1 + o] x [y0 - o, y1 + o] and not in the inner one [x0 + i + 1, x1 - i - 1] x [y0 + i + 1, y1 - i - 1], o = t / 2,
// i = (t - 1) / 2.  Several boxes on one frame are drawn in index order, the last one whose band holds a pixel gives it its colour —
// written as a gather (as fear_train_glass.h writes its scatter): the lane that owns a band pixel of box k skips it when a later box of
// the same frame holds it.  No atomics, no order between workgroups, the same bytes on every run.
//
// The bodies name no HIP built-in: with the defaults below they are device code; tools/visuals_kernel_host.cpp defines the macros for a
// host build (one thread per lane, a barrier for the sync) that runs under the sanitizers.  The kernels and entry points at the end are
// the device's alone (FEAR_VIS_HOST leaves them out).  Included by fear_train.hip behind fear_train_metrics.h; the decide kernel needs
// decode_wave (fear_kernels.h).
#ifndef FEAR_VIS_DEV
#define FEAR_VIS_DEV __device__ __forceinline__
#define FEAR_VIS_SYNC() __syncthreads()
#endif

typedef long long vis_i64;

constexpr int kVisThreads = 256;                            // lanes of a drawing workgroup (a multiple of 8: one flag byte per lane)
constexpr int kVisListCap = 512;                            // later boxes a workgroup keeps in LDS; the rest it reads from memory
constexpr int kVisSheetW = 384, kVisItemH = 256, kVisTmpl = 128, kVisSearch = 256;
constexpr int kVisTileRows = 16;                            // sheet rows of one render workgroup
constexpr int kVisMaxImages = 64;                           // FEAR_MINER_MAX_IMAGES
constexpr int kVisBoxLimit = 1 << 20;                       // a decoded coordinate is cut to +-2^20

struct VisFrame {                                           // the layout of fear_frame (include/fear_hip.h)
    unsigned char* data;
    int h, w;
};

struct VisMinerState {                                      // the layout of FearMinerState (include/fear_train.h)
    int has[2], step[2];
    double score[2];
    int take[2], reserved[2];
    int pred[kVisMaxImages][4];
};

struct VisShared {
    vis_i64 list[kVisListCap][4];                           // x0, y0, x1, y1 of the later boxes that meet this workgroup's strip
    unsigned long long flag[kVisThreads / 8];               // one byte per lane: its candidate of the current chunk meets the strip
};

// The shared band test.  (x0, y0) <= (x1, y1) are the box's corners, both inclusive.
FEAR_VIS_DEV bool vis_in_band(vis_i64 x0, vis_i64 y0, vis_i64 x1, vis_i64 y1, int t, vis_i64 px, vis_i64 py) {
    const int o = t / 2, i = (t - 1) / 2;
    if (px < x0 - o || px > x1 + o || py < y0 - o || py > y1 + o) return false;
    return !(px >= x0 + i + 1 && px <= x1 - i - 1 && py >= y0 + i + 1 && py <= y1 - i - 1);
}

// x, y, w, h -> corners: pt2 = (x + w, y + h) is inclusive and may lie on either side of pt1.
FEAR_VIS_DEV void vis_corners(const int* b, vis_i64* c) {
    const vis_i64 xa = b[0], ya = b[1], xb = xa + b[2], yb = ya + b[3];
    c[0] = xa < xb ? xa : xb; c[1] = ya < yb ? ya : yb; c[2] = xa < xb ? xb : xa; c[3] = ya < yb ? yb : ya;
}

FEAR_VIS_DEV vis_i64 vis_max(vis_i64 a, vis_i64 b) { return a > b ? a : b; }
FEAR_VIS_DEV vis_i64 vis_min(vis_i64 a, vis_i64 b) { return a < b ? a : b; }

// One side of box k: 0 the top strip, 1 the bottom strip (both over the outer rectangle's width), 2 the left and 3 the right strip of the
// rows between them.  The four cover the band (a strip runs on to the far side of a box thinner than the band); every pixel is tested
// with vis_in_band all the same.  Every lane of the workgroup takes the same branches up to the pixel loop.
FEAR_VIS_DEV void vis_draw_side(const VisFrame* frames, int n_frames, const int* boxes, const int* frame_of, const unsigned char* colours, int K,
                                int t, int k, int side, VisShared& sh, int tid, int nthr) {
    const int f = frame_of[k];
    if (f < 0 || f >= n_frames) return;
    const VisFrame fr = frames[f];
    if (fr.h <= 0 || fr.w <= 0 || !fr.data) return;
    vis_i64 c[4];
    vis_corners(boxes + 4 * (long)k, c);
    const int o = t / 2, i = (t - 1) / 2;
    vis_i64 sx0 = c[0] - o, sx1 = c[2] + o, sy0 = c[1] - o, sy1 = c[3] + o;
    if (side == 0) sy1 = vis_min(c[1] + i, sy1);
    else if (side == 1) sy0 = vis_max(c[3] - i, sy0);
    else {
        sy0 = c[1] + i + 1; sy1 = c[3] - i - 1;
        if (side == 2) sx1 = vis_min(c[0] + i, sx1);
        else sx0 = vis_max(c[2] - i, sx0);
    }
    sx0 = vis_max(sx0, 0); sy0 = vis_max(sy0, 0); sx1 = vis_min(sx1, fr.w - 1); sy1 = vis_min(sy1, fr.h - 1);
    if (sx0 > sx1 || sy0 > sy1) return;

    // the later boxes of this frame whose outer rectangle meets the strip, nthr candidates at a time: a lane flags its candidate, counts
    // the flags in front of its own and stores the corners there.  When the list cannot take another chunk the boxes from `scan_from` on
    // are read from memory in the pixel loop instead.
    int count = 0, scan_from = K;
    unsigned char* flag = (unsigned char*)sh.flag;
    for (int base = k + 1; base < K; base += nthr) {
        if (count + nthr > kVisListCap) { scan_from = base; break; }
        const int j = base + tid;
        vis_i64 cj[4];
        bool hit = false;
        if (j < K && frame_of[j] == f) {
            vis_corners(boxes + 4 * (long)j, cj);
            hit = cj[0] - o <= sx1 && cj[2] + o >= sx0 && cj[1] - o <= sy1 && cj[3] + o >= sy0;
        }
        flag[tid] = hit ? 1 : 0;
        FEAR_VIS_SYNC();
        int before = 0, total = 0;
        for (int w = 0; w < nthr / 8; ++w) {
            const unsigned long long bits = sh.flag[w];
            total += __builtin_popcountll(bits);
            if (w < tid / 8) before += __builtin_popcountll(bits);
            else if (w == tid / 8) before += __builtin_popcountll(bits & ((1ull << (8 * (tid % 8))) - 1ull));
        }
        if (hit) {
            vis_i64* e = sh.list[count + before];
            e[0] = cj[0]; e[1] = cj[1]; e[2] = cj[2]; e[3] = cj[3];
        }
        count += total;
        FEAR_VIS_SYNC();
    }

    const unsigned char r = colours[3 * (long)k], g = colours[3 * (long)k + 1], b = colours[3 * (long)k + 2];
    const vis_i64 sw = sx1 - sx0 + 1, cnt = sw * (sy1 - sy0 + 1);
    for (vis_i64 p = tid; p < cnt; p += nthr) {
        const vis_i64 py = sy0 + p / sw, px = sx0 + p % sw;
        if (!vis_in_band(c[0], c[1], c[2], c[3], t, px, py)) continue;
        bool later = false;
        for (int e = 0; e < count && !later; ++e) later = vis_in_band(sh.list[e][0], sh.list[e][1], sh.list[e][2], sh.list[e][3], t, px, py);
        for (int j = scan_from; j < K && !later; ++j) {
            if (frame_of[j] != f) continue;
            vis_i64 cj[4];
            vis_corners(boxes + 4 * (long)j, cj);
            later = vis_in_band(cj[0], cj[1], cj[2], cj[3], t, px, py);
        }
        if (later) continue;
        unsigned char* q = fr.data + (py * fr.w + px) * 3;
        q[0] = r; q[1] = g; q[2] = b;
    }
}

// A NaN by its bits (the library is built without NaN semantics for comparisons).
FEAR_VIS_DEV bool vis_is_nan(double v) {
    unsigned long long u;
    __builtin_memcpy(&u, &v, 8);
    return (u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
}

// `_check_score` of the reference for one score: a side that holds nothing takes the batch; otherwise better is s <= best - min_delta
// (mode min) or s >= best + min_delta (mode max) and worse the mirror image.  A NaN on either side of a comparison takes nothing.
FEAR_VIS_DEV int vis_miner_decide(VisMinerState* st, double s, int mode_max, double min_delta, int step_index) {
#pragma clang fp contract(off)
    int any = 0;
    for (int side = 0; side < 2; ++side) {
        bool take = st->has[side] == 0;
        if (!take && !vis_is_nan(s) && !vis_is_nan(st->score[side])) {
            const double kept = st->score[side];
            const bool down = (side == 0) != (mode_max != 0);           // this side wants a smaller score
            take = down ? s <= kept - min_delta : s >= kept + min_delta;
        }
        st->take[side] = take ? 1 : 0;
        if (take) { st->has[side] = 1; st->score[side] = s; st->step[side] = step_index; any = 1; }
    }
    return any;
}

// int(v) of the reference's map(int, ...): toward zero; a NaN is 0, a magnitude above 2^20 is cut to it.
FEAR_VIS_DEV int vis_trunc_box(double v) {
    if (vis_is_nan(v)) return 0;
    if (v > (double)kVisBoxLimit) return kVisBoxLimit;
    if (v < -(double)kVisBoxLimit) return -kVisBoxLimit;
    return (int)v;
}

// rgb_image_from_tensor: 255 (x std + mean) in float64, truncated toward zero; cut to 0..255 where the reference would wrap.
FEAR_VIS_DEV unsigned char vis_denorm(float x, int ch) {
#pragma clang fp contract(off)
    const double sd = ch == 0 ? 0.229 : (ch == 1 ? 0.224 : 0.225), mean = ch == 0 ? 0.485 : (ch == 1 ? 0.456 : 0.406);
    const double scaled = (double)x * sd;
    const double v = 255.0 * (scaled + mean);
    if (vis_is_nan(v)) return 0;
    if (v >= 255.0) return 255;
    if (v <= 0.0) return 0;
    return (unsigned char)(int)v;
}

// One tile of kVisTileRows sheet rows of item k of one side's sheet: the template in columns 0..127 of the top 128 rows and zeros below
// it, the search crop in columns 128..383 with the predicted box (green), then the ground-truth box (red, blue when invisible) on it
// at thickness 2.
FEAR_VIS_DEV void vis_render_tile(const float* templ, const float* search, const int* pred, const int* gt_box, const int* visible, int k,
                                  int tile, unsigned char* sheet, int tid, int nthr) {
    vis_i64 pc[4], gc[4];
    vis_corners(pred + 4 * k, pc);
    vis_corners(gt_box + 4 * (long)k, gc);
    const bool vis = visible[k] != 0;
    const float* tp = templ + (long)k * 3 * kVisTmpl * kVisTmpl;
    const float* sp = search + (long)k * 3 * kVisSearch * kVisSearch;
    for (int p = tid; p < kVisTileRows * kVisSheetW; p += nthr) {
        const int row = tile * kVisTileRows + p / kVisSheetW, col = p % kVisSheetW;
        unsigned char rgb[3] = {0, 0, 0};
        if (col < kVisTmpl) {
            if (row < kVisTmpl)
                for (int ch = 0; ch < 3; ++ch) rgb[ch] = vis_denorm(tp[(ch * kVisTmpl + row) * kVisTmpl + col], ch);
        } else {
            const int x = col - kVisTmpl;
            if (vis_in_band(gc[0], gc[1], gc[2], gc[3], 2, x, row)) {
                rgb[0] = vis ? 250 : 0; rgb[2] = vis ? 0 : 250;
            } else if (vis_in_band(pc[0], pc[1], pc[2], pc[3], 2, x, row)) {
                rgb[1] = 250;
            } else {
                for (int ch = 0; ch < 3; ++ch) rgb[ch] = vis_denorm(sp[(ch * kVisSearch + row) * kVisSearch + x], ch);
            }
        }
        unsigned char* q = sheet + (((long)k * kVisItemH + row) * kVisSheetW + col) * 3;
        q[0] = rgb[0]; q[1] = rgb[1]; q[2] = rgb[2];
    }
}

#ifndef FEAR_VIS_HOST

namespace {

using namespace fear;

struct DrawArgs {
    const VisFrame* frames;
    const int* boxes;
    const int* frame_of;
    const unsigned char* colours;
    int n_frames, K, thickness;
};

// One workgroup per (box, side).
__global__ __launch_bounds__(kVisThreads) void draw_boxes_kernel(DrawArgs a) {
    __shared__ VisShared sh;
    vis_draw_side(a.frames, a.n_frames, a.boxes, a.frame_of, a.colours, a.K, a.thickness, (int)(blockIdx.x >> 2), (int)(blockIdx.x & 3u), sh,
                  (int)threadIdx.x, kVisThreads);
}

struct MinerArgs {
    const float* templ;
    const float* search;
    const float* cls;
    const float* bbox;
    const int* gt_box;
    const int* visible;
    const float* score_a;
    const float* score_b;
    VisMinerState* state;
    unsigned char* sheets;
    double min_delta;
    int n, mode_max, step_index;
};

// One wave.  Lane 0 decides; a step that is taken by either side then has its first n pairs decoded, one after the other, into the
// state's tail — once per item, and not at all on a step that is not taken.
__global__ __launch_bounds__(64) void miner_decide_kernel(MinerArgs a) {
    __shared__ int s_any;
    if (threadIdx.x == 0) {
        float s = a.score_a[0];
        if (a.score_b) s = s + a.score_b[0];
        s_any = vis_miner_decide(a.state, (double)s, a.mode_max, a.min_delta, a.step_index);
    }
    __syncthreads();
    if (!s_any) return;                                     // (uniform)
    for (int k = 0; k < a.n; ++k) {
        const Decoded d = decode_wave(a.cls + (long)k * 256, a.bbox + (long)k * 1024, FEAR_TP_SCORE, FEAR_TP_SEARCH / FEAR_TP_SCORE,
                                      FEAR_TP_SEARCH);
        if (threadIdx.x == 0) {
            int* p = a.state->pred[k];
            p[0] = vis_trunc_box(d.x0); p[1] = vis_trunc_box(d.y0); p[2] = vis_trunc_box(d.w); p[3] = vis_trunc_box(d.h);
        }
    }
}

// Grid (tiles, n, 2).  A workgroup of a side that did not take the step returns after that one load.
__global__ __launch_bounds__(256) void miner_render_kernel(MinerArgs a) {
    const int side = blockIdx.z;
    if (a.state->take[side] == 0) return;                   // (uniform)
    vis_render_tile(a.templ, a.search, &a.state->pred[0][0], a.gt_box, a.visible, (int)blockIdx.y, (int)blockIdx.x,
                    a.sheets + (long)side * a.n * kVisItemH * kVisSheetW * 3, (int)threadIdx.x, 256);
}

}  // namespace

extern "C" {

int fear_draw_boxes_u8(const fear_frame* frames, int n_frames, const int32_t* boxes, const int32_t* frame_of, const uint8_t* colours, int K,
                       int thickness, void* stream) {
    static_assert(sizeof(fear_frame) == sizeof(VisFrame) && offsetof(fear_frame, h) == offsetof(VisFrame, h) &&
                  offsetof(fear_frame, w) == offsetof(VisFrame, w), "fear_frame and VisFrame must share one layout");
    static_assert(kVisThreads % 8 == 0 && kVisListCap >= kVisThreads, "one flag byte per lane, a first chunk always fits");
    if (K < 0 || K > 65535 || n_frames < 0 || thickness < 1 || thickness > 32) return FEAR_TRAIN_ERR_SHAPE;
    if (K == 0 || n_frames == 0) return FEAR_TRAIN_OK;
    if (!frames || !boxes || !frame_of || !colours) return FEAR_TRAIN_ERR_NULL;
    const DrawArgs a{reinterpret_cast<const VisFrame*>(frames), boxes, frame_of, colours, n_frames, K, thickness};
    hipLaunchKernelGGL(draw_boxes_kernel, dim3(4u * (unsigned)K), dim3(kVisThreads), 0, static_cast<hipStream_t>(stream), a);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_miner_update(const float* templ, const float* search, const float* cls, const float* bbox, const int32_t* gt_box,
                      const int32_t* visible, const float* score_a, const float* score_b, int B, int n_images, int mode_max, double min_delta,
                      int step_index, FearMinerState* state, uint8_t* sheets, void* stream) {
    static_assert(sizeof(FearMinerState) == sizeof(VisMinerState) && offsetof(FearMinerState, score) == offsetof(VisMinerState, score) &&
                  offsetof(FearMinerState, take) == offsetof(VisMinerState, take) && offsetof(FearMinerState, pred) == offsetof(VisMinerState, pred) &&
                  FEAR_MINER_MAX_IMAGES == kVisMaxImages, "FearMinerState and VisMinerState must share one layout");
    static_assert(FEAR_TP_SEARCH == kVisSearch && FEAR_TP_TEMPLATE == kVisTmpl && kVisItemH % kVisTileRows == 0, "the crops' sides");
    if (B < 0 || B > 65535 || n_images < 1 || n_images > FEAR_MINER_MAX_IMAGES) return FEAR_TRAIN_ERR_SHAPE;
    if (B == 0) return FEAR_TRAIN_OK;
    if (!templ || !search || !cls || !bbox || !gt_box || !visible || !score_a || !state || !sheets) return FEAR_TRAIN_ERR_NULL;
    const int n = B < n_images ? B : n_images;
    const MinerArgs a{templ, search, cls, bbox, gt_box, visible, score_a, score_b, reinterpret_cast<VisMinerState*>(state), sheets, min_delta,
                      n, mode_max, step_index};
    hipLaunchKernelGGL(miner_decide_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    hipLaunchKernelGGL(miner_render_kernel, dim3(kVisItemH / kVisTileRows, (unsigned)n, 2), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

}  // extern "C"

#endif  // FEAR_VIS_HOST
