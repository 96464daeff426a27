// fear_train_data.h — the training pairs' data stage on gfx950: what the reference's
// SiameseTrackingDataset._transform does per pair on the CPU (model_training/dataset/siam_dataset.py:33-61) for a whole batch,
// straight from the frames:
//   template  get_extended_crop(frame, box, 128, 0.2)                                   utils/utils.py:215-253
//   search    get_extended_crop(frame, box, 512, u) -> BBoxCropWithOffsets' warpAffine   dataset/aug.py:52-143
//   colour    OneOf(ToGray, ToSepia) then one lookup table per channel, shared by the pair's two crops
//   targets   FEARBoxCoder.encode + get_regression_weight_label                          dataset/box_coder.py:58-72, dataset/utils.py:19-31
// The host (feartracker_amd/train_data.py) does every scalar per-pair step — context boxes, the jitter, the moved box, the inverse
// warp, the lookup tables — and restates this file's arithmetic in numpy (`TrainPairBuilder.build_host`); the two agree bit for bit.
// Included by fear_train.hip after the training operators; uses linear_tap and CropFrame of fear_kernels.h.

namespace {

using namespace fear;

// ---- frame mean colours ---------------------------------------------------------------------------------------------------
// One workgroup per frame.  The frame's bytes are summed per channel (the channel of byte k is k % 3) with 16-byte loads between a
// scalar head and tail, in 64-bit integers: exact, so the order of the additions does not matter.  np.mean's float64 pairwise sum of
// uint8 values is exact too, so sum / (h w) in double is its mean bit for bit.
constexpr int kBorderThreads = 1024;

__global__ __launch_bounds__(kBorderThreads) void frame_border_kernel(const CropFrame* frames, uint8_t* out) {
    const CropFrame fr = frames[blockIdx.x];
    unsigned long long s0 = 0ull, s1 = 0ull, s2 = 0ull;      // (scalars, not an array: a dynamically indexed one lands in scratch)
    auto add = [&](int c, unsigned long long v) {
        s0 += c == 0 ? v : 0ull;
        s1 += c == 1 ? v : 0ull;
        s2 += c == 2 ? v : 0ull;
    };
    const bool empty = fr.data == nullptr || fr.H < 1 || fr.W < 1;
    if (!empty) {
        const long nbytes = (long)fr.H * fr.W * 3;
        const uintptr_t base = reinterpret_cast<uintptr_t>(fr.data);
        const long head = min((long)((16 - (base & 15)) & 15), nbytes);
        const long nvec = (nbytes - head) / 16;
        const long body_end = head + nvec * 16;
        for (long k = threadIdx.x; k < head; k += blockDim.x) add((int)(k % 3), fr.data[k]);
        for (long k = body_end + threadIdx.x; k < nbytes; k += blockDim.x) add((int)(k % 3), fr.data[k]);
        const uint4* vec = reinterpret_cast<const uint4*>(fr.data + head);
        const int rot = (int)(head % 3);                 // channel of a vector's byte 0 (16 % 3 == 1: +1 per vector)
        for (long v = threadIdx.x; v < nvec; v += blockDim.x) {
            const uint4 q = vec[v];
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
            uint32_t g0 = 0u, g1 = 0u, g2 = 0u;          // sums of the bytes at positions = 0, 1, 2 (mod 3) of the 16
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const uint32_t byte = (w[b >> 2] >> ((b & 3) * 8)) & 0xffu;
                if (b % 3 == 0) g0 += byte;
                else if (b % 3 == 1) g1 += byte;
                else g2 += byte;
            }
            const int c0 = (int)((rot + v) % 3);
            add(c0, g0);
            add(c0 == 2 ? 0 : c0 + 1, g1);
            add(c0 == 0 ? 2 : c0 - 1, g2);
        }
    }
    __shared__ unsigned long long part[kBorderThreads / 64][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        unsigned long long v = c == 0 ? s0 : (c == 1 ? s1 : s2);
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        unsigned long long tot = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += part[w][c];
        int v = 0;
        if (!empty) {
            const double mean = (double)tot / ((double)fr.H * (double)fr.W);
            v = (int)fmin(fmax(rint(mean), 0.0), 255.0);
        }
        out[blockIdx.x * 3 + c] = (uint8_t)v;
    }
}

// ---- pairs --------------------------------------------------------------------------------------------------------------------
struct PairGeom {            // the layout of FearPairGeom (include/fear_train.h)
    int32_t t_frame, s_frame;
    int32_t t_ctx[4];
    int32_t s_ctx[4];
    int32_t box[4];
    int32_t presence, tone;
    double inv[4];
};

// Out = float: the crops leave normalised, fp32 NCHW (fear_train_pairs).  Out = uint8_t: they leave as the colour stage made them,
// uint8 NHWC, for the photometric stage behind (fear_train_pairs_u8).
struct WindowFrame {         // the layout of fear_frame_window (include/fear_train.h)
    const uint8_t* data;
    int H, W;                // the frame's shape
    int y0, x0, wh, ww;      // the rectangle of it that `data` holds
};

template <typename Out>
struct PairArgs {
    const CropFrame* frames;     // fear_train_pairs, fear_train_pairs_u8
    const WindowFrame* windows;  // fear_train_pairs_windows, fear_train_pairs_windows_u8 (WIN): in place of `frames`
    const uint8_t* border;   // [n_frames][3]
    const PairGeom* geom;    // [n]
    const uint8_t* lut;      // [n][3][256]
    Out* tmpl;               // float [n][3][128][128] | uint8 [n][128][128][3]
    Out* search;             // float [n][3][256][256] | uint8 [n][256][256][3]
    float* gt_reg;           // [n][4][16][16]
    float* gt_cls;           // [n][1][16][16]
    float* gt_weight;        // [n][16][16]
    int n_frames;
    float mean[3], inv_std[3];
};

constexpr int kTpTemplate = FEAR_TP_TEMPLATE, kTpContext = FEAR_TP_CONTEXT, kTpSearch = FEAR_TP_SEARCH, kTpScore = FEAR_TP_SCORE;
constexpr int kSearchBlocks = kTpSearch * kTpSearch / 256;          // one block = one search row
constexpr int kTemplateBlocks = kTpTemplate * kTpTemplate / 256;    // one block = two template rows
constexpr int kPairBlocks = kSearchBlocks + kTemplateBlocks + 1;     // + one block of target cells

// A frame of a pair, with its border colour: an index outside the table reads no pixel and pads with 0.  WIN: the frame-fetch policy
// of the windows form, in which `f` stays the frame's shape and `data` holds the rectangle (y0, x0, wh, ww) of it.
template <bool WIN>
struct PairFrame {
    CropFrame f;
    int pad[3];
};

template <>
struct PairFrame<true> {
    CropFrame f;
    int pad[3];
    int y0, x0, wh, ww;
};

template <bool WIN, typename Out>
__device__ __forceinline__ PairFrame<WIN> pair_frame(const PairArgs<Out>& a, int fi) {
    PairFrame<WIN> p;
    if ((unsigned)fi < (unsigned)a.n_frames) {
        if constexpr (WIN) {
            const WindowFrame w = a.windows[fi];
            p.f = CropFrame{w.data, w.H, w.W};
            p.y0 = w.y0; p.x0 = w.x0; p.wh = w.wh; p.ww = w.ww;
        } else {
            p.f = a.frames[fi];
        }
        for (int c = 0; c < 3; ++c) p.pad[c] = a.border[fi * 3 + c];
    } else {
        p.f = CropFrame{nullptr, 0, 0};
        if constexpr (WIN) p.y0 = p.x0 = p.wh = p.ww = 0;
        for (int c = 0; c < 3; ++c) p.pad[c] = 0;
    }
    return p;
}

template <bool WIN>
__device__ __forceinline__ void frame_rgb(const PairFrame<WIN>& p, int fx, int fy, int* rgb) {
    if (fx < 0 || fx >= p.f.W || fy < 0 || fy >= p.f.H) {
        rgb[0] = p.pad[0]; rgb[1] = p.pad[1]; rgb[2] = p.pad[2];
        return;
    }
    const uint8_t* s;
    if constexpr (WIN) {
        if (!p.f.data || p.wh < 1 || p.ww < 1) {                         // a window without pixels
            rgb[0] = p.pad[0]; rgb[1] = p.pad[1]; rgb[2] = p.pad[2];
            return;
        }
        // clamped to the window: one that is too small gives wrong pixels, never a read outside it
        const int wy = min(max(fy - p.y0, 0), p.wh - 1), wx = min(max(fx - p.x0, 0), p.ww - 1);
        s = p.f.data + ((long)wy * p.ww + wx) * 3;
    } else {
        s = p.f.data + ((long)fy * p.f.W + fx) * 3;
    }
    rgb[0] = s[0]; rgb[1] = s[1]; rgb[2] = s[2];
}

// One axis of a get_extended_crop resize (crop_resize_normalize_kernel's taps) for output coordinate d of S.
struct Taps {
    int i0, i1, w0, w1;
};

template <bool CLAMP>
__device__ __forceinline__ Taps crop_taps(int d, int S, int src) {
    Taps t;
    linear_tap<CLAMP>(d, S, src, t.i0, t.i1, t.w0, t.w1);
    return t;
}

// Pixel (column taps tx, row taps ty) of the S x S resize of context box ctx: crop_resize_normalize_kernel's arithmetic — identity,
// exact 2x decimation (2x2 box mean), or 11-bit bilinear — on all three channels.
template <bool WIN>
__device__ __forceinline__ void crop_rgb(const PairFrame<WIN>& p, const int32_t* ctx, int S, int dx, int dy, const Taps& tx, const Taps& ty,
                                         int* rgb) {
    const int cx = ctx[0], cy = ctx[1], cw = ctx[2], ch = ctx[3];
    if (cw == S && ch == S) {
        frame_rgb(p, cx + dx, cy + dy, rgb);
        return;
    }
    if (cw == 2 * S && ch == 2 * S) {
        int a[3], b[3], c[3], d[3];
        frame_rgb(p, cx + 2 * dx, cy + 2 * dy, a);
        frame_rgb(p, cx + 2 * dx + 1, cy + 2 * dy, b);
        frame_rgb(p, cx + 2 * dx, cy + 2 * dy + 1, c);
        frame_rgb(p, cx + 2 * dx + 1, cy + 2 * dy + 1, d);
        for (int k = 0; k < 3; ++k) rgb[k] = (a[k] + b[k] + c[k] + d[k] + 2) >> 2;
        return;
    }
    int s00[3], s01[3], s10[3], s11[3];
    frame_rgb(p, cx + tx.i0, cy + ty.i0, s00);
    frame_rgb(p, cx + tx.i1, cy + ty.i0, s01);
    frame_rgb(p, cx + tx.i0, cy + ty.i1, s10);
    frame_rgb(p, cx + tx.i1, cy + ty.i1, s11);
    for (int k = 0; k < 3; ++k) {
        const int r0 = s00[k] * tx.w0 + s01[k] * tx.w1;
        const int r1 = s10[k] * tx.w0 + s11[k] * tx.w1;
        const int v = (((ty.w0 * (r0 >> 4)) >> 16) + ((ty.w1 * (r1 >> 4)) >> 16) + 2) >> 2;
        rgb[k] = min(max(v, 0), 255);
    }
}

// Colour stage on a uint8 RGB pixel, then the store policy of Out for pixel `px` of a crop of `plane` pixels: normalisation into the
// three fp32 planes, or the three bytes of the uint8 HWC pixel.
template <typename Out>
__device__ __forceinline__ void colour_store(const PairArgs<Out>& a, int pair, int tone, int* rgb, Out* crop, long px, long plane) {
#pragma clang fp contract(off)      // every product and sum rounded on its own (the pragma covers only the operators written here:
                                    // __fmul_rn / __fadd_rn are plain operators in the HIP headers and would still fuse into fmas)
    if (tone == 1) {                              // cv2 COLOR_RGB2GRAY on 8u: 14-bit fixed point
        const int g = (4899 * rgb[0] + 9617 * rgb[1] + 1868 * rgb[2] + 8192) >> 14;
        rgb[0] = rgb[1] = rgb[2] = g;
    } else if (tone == 2) {                       // albumentations ToSepia: fp32, j = 0, 1, 2, round half to even, saturate
        const float m[3][3] = {{0.393f, 0.769f, 0.189f}, {0.349f, 0.686f, 0.168f}, {0.272f, 0.534f, 0.131f}};
        int o[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            float acc = m[i][0] * (float)rgb[0];
            acc = acc + m[i][1] * (float)rgb[1];
            acc = acc + m[i][2] * (float)rgb[2];
            o[i] = (int)fminf(fmaxf(rintf(acc), 0.f), 255.f);
        }
        rgb[0] = o[0]; rgb[1] = o[1]; rgb[2] = o[2];
    }
    const uint8_t* lut = a.lut + (long)pair * 768;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint8_t v = lut[c * 256 + rgb[c]];
        if constexpr (sizeof(Out) == 1) {
            crop[px * 3 + c] = v;
        } else {
            float f = (float)v;
            f = f - a.mean[c];
            f = f * a.inv_std[c];
            crop[c * plane + px] = f;
        }
    }
}

// cv2.warpAffine's source coordinate of one destination coordinate, in OpenCV 4.x imgwarp.cpp's fixed point: AB_BITS = 10,
// INTER_BITS = 5, round_delta = 16; the row term and the per-column delta are rounded separately (cvRound = half to even), every
// double product and sum on its own (no fma).
// x axis: X = (cvRound(M2 * 1024) + 16 + cvRound(M0 x * 1024)) >> 5   (M1 = 0: the row term is M2 alone)
// y axis: Y = (cvRound((M4 y + M5) * 1024) + 16 + cvRound(M3 x * 1024) = 0) >> 5
__device__ __forceinline__ int warp_x(const double* inv, int x) {
#pragma clang fp contract(off)
    return ((int)rint(inv[1] * 1024.0) + 16 + (int)rint((inv[0] * (double)x) * 1024.0)) >> 5;
}
__device__ __forceinline__ int warp_y(const double* inv, int y) {
#pragma clang fp contract(off)      // M4 y + M5 rounded twice, as OpenCV's host code computes it
    return ((int)rint((inv[2] * (double)y + inv[3]) * 1024.0) + 16) >> 5;
}

template <typename Out, bool WIN>
__global__ __launch_bounds__(256) void train_pairs_kernel(PairArgs<Out> a) {
    const int pair = blockIdx.y;
    const int blk = blockIdx.x;
    const PairGeom& g = a.geom[pair];
    if (blk < kSearchBlocks) {
        // ---- search pixel (dx, dy): warpAffine INTER_LINEAR of the 512 stage-1 crop, BORDER_CONSTANT 0
        const int dy = blk, dx = threadIdx.x;
        const PairFrame<WIN> p = pair_frame<WIN>(a, g.s_frame);
        const int X = warp_x(g.inv, dx), Y = warp_y(g.inv, dy);
        const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
        // initInterTab2D(INTER_LINEAR, fixed point) entry (fy, fx): (vy_k1 vx_k2) * 32768, exact; entry (0, 0) saturates its 32768
        // to 32767 and the sum correction adds the missing 1 to the (1, 1) weight
        int w00 = (32 - fy) * (32 - fx) * 32, w01 = (32 - fy) * fx * 32, w10 = fy * (32 - fx) * 32, w11 = fy * fx * 32;
        if (fx == 0 && fy == 0) { w00 = 32767; w11 = 1; }
        int acc[3] = {0, 0, 0};
        const int ctx_w = g.s_ctx[2], ctx_h = g.s_ctx[3];
        const Taps ty0 = crop_taps<false>(min(max(sy, 0), kTpContext - 1), kTpContext, ctx_h);
        const Taps ty1 = crop_taps<false>(min(max(sy + 1, 0), kTpContext - 1), kTpContext, ctx_h);
        const Taps tx0 = crop_taps<true>(min(max(sx, 0), kTpContext - 1), kTpContext, ctx_w);
        const Taps tx1 = crop_taps<true>(min(max(sx + 1, 0), kTpContext - 1), kTpContext, ctx_w);
        auto tap = [&](int cx, int cy, const Taps& tx, const Taps& ty, int w) {
            if (w == 0 || cx < 0 || cx >= kTpContext || cy < 0 || cy >= kTpContext) return;   // outside the crop: 0
            int rgb[3];
            crop_rgb(p, g.s_ctx, kTpContext, cx, cy, tx, ty, rgb);
            for (int c = 0; c < 3; ++c) acc[c] += rgb[c] * w;
        };
        tap(sx, sy, tx0, ty0, w00);
        tap(sx + 1, sy, tx1, ty0, w01);
        tap(sx, sy + 1, tx0, ty1, w10);
        tap(sx + 1, sy + 1, tx1, ty1, w11);
        int rgb[3];
        for (int c = 0; c < 3; ++c) rgb[c] = (acc[c] + (1 << 14)) >> 15;
        const long plane = (long)kTpSearch * kTpSearch;
        colour_store(a, pair, g.tone, rgb, a.search + (long)pair * 3 * plane, (long)dy * kTpSearch + dx, plane);
    } else if (blk < kSearchBlocks + kTemplateBlocks) {
        // ---- template pixel: crop_resize_normalize_kernel's crop, the colour stage in front of the normalisation
        const int px = (blk - kSearchBlocks) * 256 + threadIdx.x;
        const int dy = px / kTpTemplate, dx = px % kTpTemplate;
        const PairFrame<WIN> p = pair_frame<WIN>(a, g.t_frame);
        const Taps tx = crop_taps<true>(dx, kTpTemplate, g.t_ctx[2]);
        const Taps ty = crop_taps<false>(dy, kTpTemplate, g.t_ctx[3]);
        int rgb[3];
        crop_rgb(p, g.t_ctx, kTpTemplate, dx, dy, tx, ty, rgb);
        const long plane = (long)kTpTemplate * kTpTemplate;
        colour_store(a, pair, g.tone, rgb, a.tmpl + (long)pair * 3 * plane, (long)px, plane);
    } else {
        // ---- target cell (i, j): ltrb against the float64 grid, positive where min(ltrb) > 0, weight 1 within L1 distance 2 of the
        // box centre's cell (r_neg = 0: no 0.5 ring); zeros when the search target is absent
        const int cell = threadIdx.x, i = cell / kTpScore, j = cell % kTpScore;
        const long cells = (long)kTpScore * kTpScore;
        const int bx = g.box[0], by = g.box[1], bw = g.box[2], bh = g.box[3];
        float l = 0.f, t = 0.f, r = 0.f, b = 0.f, cls = 0.f, wgt = 0.f;
        if (g.presence) {
            const double gx = (double)((j - kTpScore / 2) * 16 + kTpSearch / 2), gy = (double)((i - kTpScore / 2) * 16 + kTpSearch / 2);
            const double dl = gx - bx, dt = gy - by, dr = ((double)bx + bw) - gx, db = ((double)by + bh) - gy;
            l = (float)dl; t = (float)dt; r = (float)dr; b = (float)db;
            cls = fminf(fminf(l, t), fminf(r, b)) > 0.f ? 1.f : 0.f;
            const int cxc = bx + bw / 2, cyc = by + bh / 2;       // floor(c / 256 * 16) of a non-negative c
            const int szx = (int)floor((double)cxc / kTpSearch * kTpScore), szy = (int)floor((double)cyc / kTpSearch * kTpScore);
            wgt = (abs(j - szx) + abs(i - szy)) <= 2 ? 1.f : 0.f;
        }
        float* reg = a.gt_reg + (long)pair * 4 * cells + cell;
        reg[0] = l; reg[cells] = t; reg[2 * cells] = r; reg[3 * cells] = b;
        a.gt_cls[(long)pair * cells + cell] = cls;
        a.gt_weight[(long)pair * cells + cell] = wgt;
    }
}

// ---- photometric stage ------------------------------------------------------------------------------------------------------------
// PHOTOMETRIC_AUGMENTATIONS of the reference (dataset/aug.py:8-25) on one uint8 HWC crop, then the normalisation: blur -> noise ->
// Downscale(0.5, INTER_NEAREST), the members and their integer / fp32 forms as DESIGN.md section 11 states them.  One workgroup per
// (32 x 32 output tile, crop); the record is uniform per workgroup, so every member branch is a scalar branch.  A blurred crop stages
// its tile plus a halo of 3 into LDS once, the border rule applied while staging (BORDER_REFLECT_101, BORDER_REPLICATE for the
// median), so the blur loops index LDS without a bounds test.
struct PhotoOp {             // the layout of FearPhotoOp (include/fear_train.h)
    int32_t blur, ksize, noise;
    float scale;
    uint32_t key[2];
    int32_t downscale, tap_row;
};

// Out = float: the crops leave normalised, fp32 NCHW (fear_photometric_u8).  Out = uint8_t: they leave as the chain made them, uint8
// NHWC, for fear_jpeg_u8 behind (fear_photometric_stage_u8).
template <typename Out>
struct PhotoArgs {
    const uint8_t* in;       // [n][H][W][3]
    const PhotoOp* ops;      // [n]
    const float* taps;       // [m][49], may be null
    const float* q;          // [4096]
    Out* out;                // float [n][3][H][W] | uint8 [n][H][W][3]
    int H, W;
    float mean[3], inv_std[3];
};

constexpr int kPhTile = 32, kPhHalo = 3, kPhSide = kPhTile + 2 * kPhHalo, kPhPitch = kPhSide * 3, kPhBytes = kPhSide * kPhPitch;
static_assert(kPhBytes % 4 == 0, "the tile is staged in 4-byte words");

// Source index of coordinate i on an axis of n >= 4 pixels, |overshoot| <= 3 where it matters: one reflection about the edge pixel
// (BORDER_REFLECT_101) or the edge pixel itself (BORDER_REPLICATE).  Columns of a ragged tile further out feed no output pixel; the
// clamp keeps their address inside the crop.
__device__ __forceinline__ int photo_border(int i, int n, bool replicate) {
    if (!replicate) i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
    return min(max(i, 0), n - 1);
}

template <int K>
__device__ __forceinline__ int gauss_weight(int i) {       // OpenCV's small-kernel tables for sigma = 0, as 8-bit weights (sum 256)
    if constexpr (K == 3) return i == 1 ? 128 : 64;
    else if constexpr (K == 5) return i == 2 ? 96 : ((i == 1 || i == 3) ? 64 : 16);
    else return i == 3 ? 72 : ((i == 2 || i == 4) ? 56 : ((i == 1 || i == 5) ? 28 : 8));
}

// One blurred pixel: `win` points at channel 0 of the window's centre in the staged tile.
template <int KIND, int K>
__device__ __forceinline__ void blur_px(const uint8_t* win, int* v) {
    constexpr int R = K / 2;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if constexpr (KIND == 1) {                          // Blur: (sum + k k / 2) / (k k) in integers
            int s = 0;
#pragma unroll
            for (int dy = -R; dy <= R; ++dy)
#pragma unroll
                for (int dx = -R; dx <= R; ++dx) s += win[dy * kPhPitch + dx * 3 + c];
            v[c] = (s + K * K / 2) / (K * K);
        } else if constexpr (KIND == 2) {                   // GaussianBlur, sigma 0: 8-bit weights on both axes, one rounding
            int s = 0;
#pragma unroll
            for (int dy = -R; dy <= R; ++dy) {
                int row = 0;
#pragma unroll
                for (int dx = -R; dx <= R; ++dx) row += gauss_weight<K>(dx + R) * win[dy * kPhPitch + dx * 3 + c];
                s += gauss_weight<K>(dy + R) * row;
            }
            v[c] = (s + 32768) >> 16;
        } else {                                            // MedianBlur: the largest m with #(window >= m) >= (k k + 1) / 2, bit by bit
            int m = 0;
#pragma unroll
            for (int bit = 7; bit >= 0; --bit) {
                const int cand = m | (1 << bit);
                int cnt = 0;
#pragma unroll
                for (int dy = -R; dy <= R; ++dy)
#pragma unroll
                    for (int dx = -R; dx <= R; ++dx) cnt += win[dy * kPhPitch + dx * 3 + c] >= cand ? 1 : 0;
                m = cnt >= (K * K + 1) / 2 ? cand : m;
            }
            v[c] = m;
        }
    }
}

template <int KIND>
__device__ __forceinline__ void blur_px_k(int k, const uint8_t* win, int* v) {
    if (k == 3) blur_px<KIND, 3>(win, v);
    else if (k == 5) blur_px<KIND, 5>(win, v);
    else blur_px<KIND, 7>(win, v);
}

// MotionBlur: cv2.filter2D on uint8 with the crop's 7 x 7 row of the tap table (a k x k kernel sits centred in it): correlation, anchor
// at the centre, fp32 accumulation over the non-zero taps in row-major order, rint half to even, saturate.
__device__ __forceinline__ void motion_px(const float* taps, const uint8_t* win, int* v) {
#pragma clang fp contract(off)
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 49; ++t) {
        const float w = taps[t];                            // uniform: a scalar load and a scalar branch
        if (w != 0.f) {
            const uint8_t* p = win + (t / 7 - 3) * kPhPitch + (t % 7 - 3) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + w * (float)p[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (int)fminf(fmaxf(rintf(acc[c]), 0.f), 255.f);
}

// Philox4x32-10 (Salmon et al., Random123) of counter (c0, c1, 0, 0) and key (k0, k1): words 0, 1, 2.
__device__ __forceinline__ void philox3(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t* out) {
    uint32_t c2 = 0u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2;
}

template <typename Out>
__global__ __launch_bounds__(256) void photometric_kernel(PhotoArgs<Out> a) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[kPhBytes];
    const int crop = blockIdx.z, x0 = blockIdx.x * kPhTile, y0 = blockIdx.y * kPhTile;
    const int H = a.H, W = a.W, tid = threadIdx.x;
    const PhotoOp op = a.ops[crop];
    // a record the host could not have drawn (unknown kind, ksize outside {3, 5, 7}, a motion blur without its taps) means "none"
    int blur = op.blur;
    const int k = op.ksize;
    if (blur < 1 || blur > 4 || !(k == 3 || k == 5 || k == 7) || (blur == 4 && (a.taps == nullptr || op.tap_row < 0))) blur = 0;
    const int noise = (op.noise == 1 || op.noise == 2) ? op.noise : 0;
    const bool down = op.downscale != 0;
    const uint8_t* src = a.in + (long)crop * H * W * 3;
    if (blur != 0) {
        // stage rows y0 - 3 .. y0 + 34, columns x0 - 3 .. x0 + 34: a 4-byte word whose pixels all lie inside the row is one load
        // (the 3-byte pitch leaves it unaligned), a word that touches the border or wraps to the next row goes byte by byte
        const bool rep = blur == 3;
        for (int w = tid; w < kPhBytes / 4; w += 256) {
            const int i = w * 4, r = i / kPhPitch, b = i - r * kPhPitch;
            const int gx0 = x0 - kPhHalo + b / 3, gx1 = x0 - kPhHalo + (b + 3) / 3;
            uint32_t word = 0u;
            if (b + 3 < kPhPitch && gx0 >= 0 && gx1 < W) {
                const int gy = photo_border(y0 - kPhHalo + r, H, rep);
                __builtin_memcpy(&word, src + ((long)gy * W + (x0 - kPhHalo)) * 3 + b, 4);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int rr = (i + j) / kPhPitch, bb = (i + j) - rr * kPhPitch;
                    const int gy = photo_border(y0 - kPhHalo + rr, H, rep), gx = photo_border(x0 - kPhHalo + bb / 3, W, rep);
                    word |= (uint32_t)src[((long)gy * W + gx) * 3 + bb % 3] << (8 * j);
                }
            }
            reinterpret_cast<uint32_t*>(tile)[w] = word;
        }
        __syncthreads();
    }
    const float* taps = blur == 4 ? a.taps + (long)op.tap_row * 49 : nullptr;
#pragma unroll 1
    for (int it = 0; it < kPhTile * kPhTile / 256; ++it) {
        const int ly = it * 8 + (tid >> 5), lx = tid & 31;
        const int x = x0 + lx, y = y0 + ly;
        if (x >= W || y >= H) continue;
        // Downscale(0.5, INTER_NEAREST) and back: the whole chain at the even pixel (H and W are even, tiles start even)
        const int sx = down ? (x & ~1) : x, sy = down ? (y & ~1) : y;
        int v[3];
        if (blur == 0) {
            const uint8_t* p = src + ((long)sy * W + sx) * 3;
            v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
        } else {
            const uint8_t* win = tile + (sy - y0 + kPhHalo) * kPhPitch + (sx - x0 + kPhHalo) * 3;
            if (blur == 1) blur_px_k<1>(k, win, v);
            else if (blur == 2) blur_px_k<2>(k, win, v);
            else if (blur == 3) blur_px_k<3>(k, win, v);
            else motion_px(taps, win, v);
        }
        {
#pragma clang fp contract(off)      // every product and sum rounded on its own, as in colour_store
            if (noise == 1) {                               // MultiplicativeNoise, one multiplier per crop
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = (int)fminf(fmaxf((float)v[c] * op.scale, 0.f), 255.f);
            } else if (noise == 2) {                        // GaussNoise: sigma times a table quantile picked by 12 Philox bits
                uint32_t rnd[3];
                philox3((uint32_t)sx, (uint32_t)sy, op.key[0], op.key[1], rnd);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float f = op.scale * a.q[rnd[c] >> 20];
                    f = (float)v[c] + f;
                    v[c] = (int)fminf(fmaxf(f, 0.f), 255.f);
                }
            }
            if constexpr (sizeof(Out) == 1) {
                Out* o = a.out + ((long)crop * H * W + (long)y * W + x) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c] = (uint8_t)v[c];
            } else {
                Out* o = a.out + (long)crop * 3 * H * W + (long)y * W + x;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float f = (float)v[c];
                    f = f - a.mean[c];
                    f = f * a.inv_std[c];
                    o[(long)c * H * W] = f;
                }
            }
        }
    }
}

// ---- colour stage, the members that are no lookup table ------------------------------------------------------------------------------
// fear_colour_u8: Equalize, HueSaturationValue, ColorJitter and Emboss on uint8 HWC crops (fear_train_colour.h holds the body).  One
// workgroup of 1024 lanes per crop, 3.8 KB of LDS; no global atomics.
#include "fear_train_colour.h"

constexpr int kColourThreads = 1024;

__global__ __launch_bounds__(kColourThreads) void colour_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W,
                                                                const ColourOp* __restrict__ ops, const uint8_t* __restrict__ aux) {
    __shared__ ColourShared sh;
    const long crop = blockIdx.x, bytes = (long)H * W * 3;
    colour_crop(in + crop * bytes, out + crop * bytes, H, W, ops + crop, aux + crop * 768, sh, (int)threadIdx.x, kColourThreads);
}

// ---- the members that work in HLS --------------------------------------------------------------------------------------------------
// fear_hls_u8: ISONoise, RandomRain and RandomShadow on uint8 HWC crops (fear_train_hls.h holds the body).  One workgroup of 1024 lanes
// per crop, 9.3 KB of LDS (the 256 x 256-bit mask, the CDF, two sums); no global atomics.
#include "fear_train_hls.h"

__global__ __launch_bounds__(kColourThreads) void hls_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W,
                                                             const HlsOp* __restrict__ ops, const int16_t* __restrict__ seg,
                                                             const float* __restrict__ q, const double* __restrict__ exp_table) {
    __shared__ HlsShared sh;
    const long crop = blockIdx.x, bytes = (long)H * W * 3;
    hls_crop(in + crop * bytes, out + crop * bytes, H, W, ops + crop, seg, q, exp_table, sh, (int)threadIdx.x, kColourThreads);
}

// ---- GlassBlur -----------------------------------------------------------------------------------------------------------------------
// fear_glass_u8: the blur group's fifth member on uint8 HWC crops (fear_train_glass.h holds the body).  One workgroup of 256 lanes per
// 32 x 32 tile of a crop, 21.4 KB of LDS (two buffers of three 56 x 56 byte planes and the offsets' plane); no atomics.
#include "fear_train_glass.h"

constexpr int kGlassThreads = 256;

__global__ __launch_bounds__(kGlassThreads) void glass_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W,
                                                              const PhotoOp* __restrict__ ops) {
    __shared__ GlassShared sh;
    const long crop = blockIdx.z, bytes = (long)H * W * 3;
    const PhotoOp op = ops[crop];
    const GlassTile t{(int)blockIdx.x * kGlTile, (int)blockIdx.y * kGlTile, H, W};
    glass_tile(in + crop * bytes, out + crop * bytes, t, op.blur == kGlassBlur, op.key[0], op.key[1], sh, (int)threadIdx.x, kGlassThreads);
}

// fear_normalize_u8's constants
template <typename Args>
void set_normalisation(Args& a) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    for (int c = 0; c < 3; ++c) {
        a.mean[c] = mean[c] * 255.0f;
        a.inv_std[c] = 1.0f / (stdv[c] * 255.0f);
    }
}

template <typename Out, bool WIN = false>
int launch_train_pairs(const void* frames, int n_frames, const uint8_t* border_rgb, const FearPairGeom* geom, const uint8_t* lut,
                       int n, Out* template_out, Out* search_out, float* gt_reg, float* gt_cls, float* gt_weight, void* stream) {
    static_assert(sizeof(FearPairGeom) == sizeof(PairGeom) && offsetof(FearPairGeom, inv) == offsetof(PairGeom, inv) &&
                  offsetof(FearPairGeom, presence) == offsetof(PairGeom, presence), "FearPairGeom and PairGeom must share one layout");
    if (n < 0 || n_frames < 0 || n > 65535) return FEAR_TRAIN_ERR_SHAPE;
    if (n == 0) return FEAR_TRAIN_OK;
    if (!geom || !lut || !template_out || !search_out || !gt_reg || !gt_cls || !gt_weight) return FEAR_TRAIN_ERR_NULL;
    if (n_frames > 0 && (!frames || !border_rgb)) return FEAR_TRAIN_ERR_NULL;
    PairArgs<Out> a{};
    static_assert(sizeof(fear_frame_window) == sizeof(WindowFrame) && offsetof(fear_frame_window, h) == offsetof(WindowFrame, H) &&
                  offsetof(fear_frame_window, y0) == offsetof(WindowFrame, y0) && offsetof(fear_frame_window, ww) == offsetof(WindowFrame, ww),
                  "fear_frame_window and WindowFrame must share one layout");
    if constexpr (WIN) a.windows = static_cast<const WindowFrame*>(frames);
    else a.frames = static_cast<const CropFrame*>(frames);
    a.border = border_rgb;
    a.geom = reinterpret_cast<const PairGeom*>(geom);
    a.lut = lut;
    a.tmpl = template_out; a.search = search_out;
    a.gt_reg = gt_reg; a.gt_cls = gt_cls; a.gt_weight = gt_weight;
    a.n_frames = n_frames;
    set_normalisation(a);
    hipLaunchKernelGGL((train_pairs_kernel<Out, WIN>), dim3(kPairBlocks, (unsigned)n), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

template <typename Out>
int launch_photometric(const uint8_t* crops_u8, int n, int H, int W, const FearPhotoOp* ops, const float* taps, const float* qtable,
                       Out* out, void* stream) {
    static_assert(sizeof(FearPhotoOp) == sizeof(PhotoOp) && offsetof(FearPhotoOp, scale) == offsetof(PhotoOp, scale) &&
                  offsetof(FearPhotoOp, key) == offsetof(PhotoOp, key) && offsetof(FearPhotoOp, tap_row) == offsetof(PhotoOp, tap_row),
                  "FearPhotoOp and PhotoOp must share one layout");
    if (n < 0 || n > 65535 || H < 4 || W < 4 || (H & 1) || (W & 1) || (long)H * W > 0x7fffffffL / 3) return FEAR_TRAIN_ERR_SHAPE;
    if (n == 0) return FEAR_TRAIN_OK;
    if (!crops_u8 || !ops || !qtable || !out) return FEAR_TRAIN_ERR_NULL;          // taps may be null: no record may then point at one
    if constexpr (sizeof(Out) == 1) {
        if (crops_u8 == out) return FEAR_TRAIN_ERR_SHAPE;                              // a blur reads its neighbours: not in place
    }
    const unsigned gx = (unsigned)((W + kPhTile - 1) / kPhTile), gy = (unsigned)((H + kPhTile - 1) / kPhTile);
    if (gy > 65535u) return FEAR_TRAIN_ERR_SHAPE;
    PhotoArgs<Out> a{};
    a.in = crops_u8;
    a.ops = reinterpret_cast<const PhotoOp*>(ops);
    a.taps = taps;
    a.q = qtable;
    a.out = out;
    a.H = H; a.W = W;
    set_normalisation(a);
    hipLaunchKernelGGL(photometric_kernel<Out>, dim3(gx, gy, (unsigned)n), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

}  // namespace

extern "C" {

int fear_frame_border_u8(const fear_frame* frames, int n_frames, uint8_t* out_rgb_u8, void* stream) {
    static_assert(sizeof(fear_frame) == sizeof(CropFrame) && offsetof(fear_frame, h) == offsetof(CropFrame, H) &&
                  offsetof(fear_frame, w) == offsetof(CropFrame, W), "fear_frame and CropFrame must share one layout");
    if (n_frames < 0) return FEAR_TRAIN_ERR_SHAPE;
    if (n_frames == 0) return FEAR_TRAIN_OK;
    if (!frames || !out_rgb_u8) return FEAR_TRAIN_ERR_NULL;
    hipLaunchKernelGGL(frame_border_kernel, dim3((unsigned)n_frames), dim3(kBorderThreads), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const CropFrame*>(frames), out_rgb_u8);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_train_pairs(const fear_frame* frames, int n_frames, const uint8_t* border_rgb, const FearPairGeom* geom, const uint8_t* lut,
                     int n, float* template_out, float* search_out, float* gt_reg, float* gt_cls, float* gt_weight, void* stream) {
    return launch_train_pairs<float>(frames, n_frames, border_rgb, geom, lut, n, template_out, search_out, gt_reg, gt_cls, gt_weight,
                                     stream);
}

int fear_train_pairs_u8(const fear_frame* frames, int n_frames, const uint8_t* border_rgb, const FearPairGeom* geom, const uint8_t* lut,
                        int n, uint8_t* template_u8, uint8_t* search_u8, float* gt_reg, float* gt_cls, float* gt_weight, void* stream) {
    return launch_train_pairs<uint8_t>(frames, n_frames, border_rgb, geom, lut, n, template_u8, search_u8, gt_reg, gt_cls, gt_weight,
                                       stream);
}

int fear_train_pairs_windows(const fear_frame_window* windows, int n_frames, const uint8_t* border_rgb, const FearPairGeom* geom,
                             const uint8_t* lut, int n, float* template_out, float* search_out, float* gt_reg, float* gt_cls,
                             float* gt_weight, void* stream) {
    return launch_train_pairs<float, true>(windows, n_frames, border_rgb, geom, lut, n, template_out, search_out, gt_reg, gt_cls,
                                           gt_weight, stream);
}

int fear_train_pairs_windows_u8(const fear_frame_window* windows, int n_frames, const uint8_t* border_rgb, const FearPairGeom* geom,
                                const uint8_t* lut, int n, uint8_t* template_u8, uint8_t* search_u8, float* gt_reg, float* gt_cls,
                                float* gt_weight, void* stream) {
    return launch_train_pairs<uint8_t, true>(windows, n_frames, border_rgb, geom, lut, n, template_u8, search_u8, gt_reg, gt_cls,
                                             gt_weight, stream);
}

int fear_photometric_u8(const uint8_t* crops_u8, int n, int H, int W, const FearPhotoOp* ops, const float* taps, const float* qtable,
                        float* out_f32, void* stream) {
    return launch_photometric<float>(crops_u8, n, H, W, ops, taps, qtable, out_f32, stream);
}

int fear_photometric_stage_u8(const uint8_t* crops_u8, int n, int H, int W, const FearPhotoOp* ops, const float* taps, const float* qtable,
                              uint8_t* out_u8, void* stream) {
    return launch_photometric<uint8_t>(crops_u8, n, H, W, ops, taps, qtable, out_u8, stream);
}

int fear_colour_u8(const uint8_t* crops_in, int n, int H, int W, const FearColourOp* ops, const uint8_t* aux_lut, uint8_t* crops_out,
                   void* stream) {
    static_assert(sizeof(FearColourOp) == sizeof(ColourOp) && offsetof(FearColourOp, order) == offsetof(ColourOp, order) &&
                  offsetof(FearColourOp, contrast) == offsetof(ColourOp, contrast) && offsetof(FearColourOp, alpha) == offsetof(ColourOp, alpha) &&
                  offsetof(FearColourOp, taps) == offsetof(ColourOp, taps), "FearColourOp and ColourOp must share one layout");
    if (n < 0 || n > 65535 || H < 4 || W < 4 || (H & 1) || (W & 1) || (long)H * W > 0x7fffffffL / 3) return FEAR_TRAIN_ERR_SHAPE;
    if (n == 0) return FEAR_TRAIN_OK;
    if (!crops_in || !ops || !aux_lut || !crops_out) return FEAR_TRAIN_ERR_NULL;
    if (crops_in == crops_out) return FEAR_TRAIN_ERR_SHAPE;                          // Emboss reads its neighbours: not in place
    hipLaunchKernelGGL(colour_kernel, dim3((unsigned)n), dim3(kColourThreads), 0, static_cast<hipStream_t>(stream), crops_in, crops_out,
                       H, W, reinterpret_cast<const ColourOp*>(ops), aux_lut);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_hls_u8(const uint8_t* crops_in, int n, int H, int W, const FearHlsOp* ops, const int16_t* segments, const float* qtable,
                const double* exp_table, uint8_t* crops_out, void* stream) {
    static_assert(sizeof(FearHlsOp) == sizeof(HlsOp) && offsetof(FearHlsOp, seg_count) == offsetof(HlsOp, seg_count) &&
                  offsetof(FearHlsOp, hue_scale) == offsetof(HlsOp, hue_scale) && offsetof(FearHlsOp, intensity) == offsetof(HlsOp, intensity) &&
                  offsetof(FearHlsOp, key) == offsetof(HlsOp, key), "FearHlsOp and HlsOp must share one layout");
    static_assert(FEAR_HLS_MAX_SIDE == kHlsMaxSide, "the mask in LDS holds FEAR_HLS_MAX_SIDE squared bits");
    if (n < 0 || n > 65535 || H < 4 || W < 4 || (H & 1) || (W & 1) || H > FEAR_HLS_MAX_SIDE || W > FEAR_HLS_MAX_SIDE) return FEAR_TRAIN_ERR_SHAPE;
    if (n == 0) return FEAR_TRAIN_OK;
    if (!crops_in || !ops || !segments || !qtable || !exp_table || !crops_out) return FEAR_TRAIN_ERR_NULL;
    if (crops_in == crops_out) return FEAR_TRAIN_ERR_SHAPE;                          // rain reads its neighbours: not in place
    hipLaunchKernelGGL(hls_kernel, dim3((unsigned)n), dim3(kColourThreads), 0, static_cast<hipStream_t>(stream), crops_in, crops_out, H, W,
                       reinterpret_cast<const HlsOp*>(ops), segments, qtable, exp_table);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_glass_u8(const uint8_t* crops_u8, int n, int H, int W, const FearPhotoOp* ops, uint8_t* out_u8, void* stream) {
    static_assert(FEAR_PHOTO_BLUR_GLASS == kGlassBlur, "the record's kind of GlassBlur");
    if (n < 0 || n > 65535 || H < 4 || W < 4 || (H & 1) || (W & 1) || H > FEAR_HLS_MAX_SIDE || W > FEAR_HLS_MAX_SIDE) return FEAR_TRAIN_ERR_SHAPE;
    if (n == 0) return FEAR_TRAIN_OK;
    if (!crops_u8 || !ops || !out_u8) return FEAR_TRAIN_ERR_NULL;
    if (crops_u8 == out_u8) return FEAR_TRAIN_ERR_SHAPE;                             // every stage reads its neighbours: not in place
    const unsigned gx = (unsigned)((W + kGlTile - 1) / kGlTile), gy = (unsigned)((H + kGlTile - 1) / kGlTile);
    hipLaunchKernelGGL(glass_kernel, dim3(gx, gy, (unsigned)n), dim3(kGlassThreads), 0, static_cast<hipStream_t>(stream), crops_u8, out_u8,
                       H, W, reinterpret_cast<const PhotoOp*>(ops));
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

}  // extern "C"
