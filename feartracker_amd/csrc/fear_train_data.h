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

struct PairArgs {
    const CropFrame* frames;
    const uint8_t* border;   // [n_frames][3]
    const PairGeom* geom;    // [n]
    const uint8_t* lut;      // [n][3][256]
    float* tmpl;             // [n][3][128][128]
    float* search;           // [n][3][256][256]
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

// A frame of a pair, with its border colour: an index outside the table reads no pixel and pads with 0.
struct PairFrame {
    CropFrame f;
    int pad[3];
};

__device__ __forceinline__ PairFrame pair_frame(const PairArgs& a, int fi) {
    PairFrame p;
    if ((unsigned)fi < (unsigned)a.n_frames) {
        p.f = a.frames[fi];
        for (int c = 0; c < 3; ++c) p.pad[c] = a.border[fi * 3 + c];
    } else {
        p.f = CropFrame{nullptr, 0, 0};
        for (int c = 0; c < 3; ++c) p.pad[c] = 0;
    }
    return p;
}

__device__ __forceinline__ void frame_rgb(const PairFrame& p, int fx, int fy, int* rgb) {
    if (fx < 0 || fx >= p.f.W || fy < 0 || fy >= p.f.H) {
        rgb[0] = p.pad[0]; rgb[1] = p.pad[1]; rgb[2] = p.pad[2];
        return;
    }
    const uint8_t* s = p.f.data + ((long)fy * p.f.W + fx) * 3;
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
__device__ __forceinline__ void crop_rgb(const PairFrame& p, const int32_t* ctx, int S, int dx, int dy, const Taps& tx, const Taps& ty,
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

// Colour stage on a uint8 RGB pixel, then normalisation -> the three fp32 outputs of one pixel (plane stride `plane`).
__device__ __forceinline__ void colour_normalise_store(const PairArgs& a, int pair, int tone, int* rgb, float* out, long plane) {
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
        float f = (float)lut[c * 256 + rgb[c]];
        f = f - a.mean[c];
        f = f * a.inv_std[c];
        out[c * plane] = f;
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

__global__ __launch_bounds__(256) void train_pairs_kernel(PairArgs a) {
    const int pair = blockIdx.y;
    const int blk = blockIdx.x;
    const PairGeom& g = a.geom[pair];
    if (blk < kSearchBlocks) {
        // ---- search pixel (dx, dy): warpAffine INTER_LINEAR of the 512 stage-1 crop, BORDER_CONSTANT 0
        const int dy = blk, dx = threadIdx.x;
        const PairFrame p = pair_frame(a, g.s_frame);
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
        colour_normalise_store(a, pair, g.tone, rgb, a.search + (long)pair * 3 * plane + dy * kTpSearch + dx, plane);
    } else if (blk < kSearchBlocks + kTemplateBlocks) {
        // ---- template pixel: crop_resize_normalize_kernel's crop, the colour stage in front of the normalisation
        const int px = (blk - kSearchBlocks) * 256 + threadIdx.x;
        const int dy = px / kTpTemplate, dx = px % kTpTemplate;
        const PairFrame p = pair_frame(a, g.t_frame);
        const Taps tx = crop_taps<true>(dx, kTpTemplate, g.t_ctx[2]);
        const Taps ty = crop_taps<false>(dy, kTpTemplate, g.t_ctx[3]);
        int rgb[3];
        crop_rgb(p, g.t_ctx, kTpTemplate, dx, dy, tx, ty, rgb);
        const long plane = (long)kTpTemplate * kTpTemplate;
        colour_normalise_store(a, pair, g.tone, rgb, a.tmpl + (long)pair * 3 * plane + px, plane);
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
    static_assert(sizeof(FearPairGeom) == sizeof(PairGeom) && offsetof(FearPairGeom, inv) == offsetof(PairGeom, inv) &&
                  offsetof(FearPairGeom, presence) == offsetof(PairGeom, presence), "FearPairGeom and PairGeom must share one layout");
    if (n < 0 || n_frames < 0 || n > 65535) return FEAR_TRAIN_ERR_SHAPE;
    if (n == 0) return FEAR_TRAIN_OK;
    if (!geom || !lut || !template_out || !search_out || !gt_reg || !gt_cls || !gt_weight) return FEAR_TRAIN_ERR_NULL;
    if (n_frames > 0 && (!frames || !border_rgb)) return FEAR_TRAIN_ERR_NULL;
    PairArgs a{};
    a.frames = reinterpret_cast<const CropFrame*>(frames);
    a.border = border_rgb;
    a.geom = reinterpret_cast<const PairGeom*>(geom);
    a.lut = lut;
    a.tmpl = template_out; a.search = search_out;
    a.gt_reg = gt_reg; a.gt_cls = gt_cls; a.gt_weight = gt_weight;
    a.n_frames = n_frames;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    for (int c = 0; c < 3; ++c) {                 // fear_normalize_u8's constants
        a.mean[c] = mean[c] * 255.0f;
        a.inv_std[c] = 1.0f / (stdv[c] * 255.0f);
    }
    hipLaunchKernelGGL(train_pairs_kernel, dim3(kPairBlocks, (unsigned)n), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

}  // extern "C"
