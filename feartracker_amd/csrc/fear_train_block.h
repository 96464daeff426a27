// fear_train_block.h — block-fused operators of the trunk's TRAINING step (BASELINE.json configs[4]; round 5).
//
// One C-ABI call per inverted-residual block and direction (model_training/model/blocks.py:22-35 over mobile_cv's
// conv-BN-ReLU units: expand 1x1 + BN + ReLU, depthwise kxk + BN + ReLU, project 1x1 + BN [+ input]); the call sequences its
// kernels on the device side of the boundary — the host issues ~70 calls per step instead of ~1 100 launches through ctypes —
// and no BatchNorm'd activation, no BatchNorm input gradient and no ReLU mask is ever written to memory:
//
//   forward    e = W1 x            + column sums of e          (pw_stat_kernel / gemm_lds_kernel)   saved: e
//              d = DW act1(e)      + column sums of d          (dw_fwd_kernel)                      saved: d
//              p = W3 act2(d)      + column sums of p          (pw_stat_kernel / gemm_lds_kernel)   saved: p
//              out = a3 p + b3 [+ x]                           (bn_act_kernel)
//   backward   sums of (dout, p)                               (col_reduce_kernel<1>)      -> d gamma3, d beta3, coef3
//              g2 = (dp W3) * [act2(d) > 0], dp = BN3'(dout, p) formed on load, + sums of (g2, dhat)   (pw_bwd_kernel<MS> / gemm_lds_kernel)
//              dW3 = dp^T act2(d), both operands formed on load                            (weight-gradient stream)
//              dd = BN2'(g2, d) formed on load into an LDS tile; g1 = (DW^T dd) * [act1(e) > 0]; d taps = sum dd (x) act1(e);
//              sums of (g1, ehat) — one pass over g2, d, e                                 (dw_bwd_kernel)
//              dx = de W1 [+ dout], de = BN1'(g1, e) formed on load                        (pw_bwd_kernel / gemm_lds_kernel)
//              dW1 = de^T x                                                                (weight-gradient stream)
// where BNk'(g, x) = gamma rstd (g - mean(g) - xhat mean(g xhat)) (struct BnbIn).  Passes over the expanded tensors of a block,
// forward + backward: e 8 (was 14 layer by layer), d 7 (was 14); launches 19 (was ~36).
//
// On top of that recipe, where the block's input is narrow (second half of round 5):
//   * BN1' without e (cin <= 32): e = x W1^T is linear in the block input, so de folds into the two consumers' own algebra — dx from
//     [A (g1 - s1 + mu Q) | x] [W1 ; -T], dW1 from [A (g1 - ...)]^T x - diag(A Q) W1 (x^T x) — see BnbIn (fear_train.hip), irb_lin_*;
//   * the stride-2 expansions are never written (FEAR_IRB_VIRTUAL_E): the two depthwise kernels form their tile of e on the matrix
//     pipe, BatchNorm1's statistics come from the input's Gram matrix (gram_kernel, irb_virtual_stats_kernel); the 3 x 3 ones also sum
//     the expansion's weight gradient while g1 is on chip (dw_bwd_kernel<.., W1G>);
//   * blocks of 16 / 24 channels throughout sum the projection's weight gradient inside the masked-gradient pass (pw_bwd_kernel<.., W3G>).
// Also here: the head's SepConv + BatchNorm + ReLU layer (fear_sepbn_train_*), the lone conv + BatchNorm units (fear_pwbn_train_*:
// the neck) and the stem on the NCHW image (fear_stem_train_*).
//
// Included at the end of fear_train.hip (same translation unit: it reuses that file's kernels and helpers).  The host side; the kernels
// and their argument structs are in fear_train_block_kernels.h.

#include "fear_train_block_kernels.h"

namespace {

// ------------------------------------------------------------------------------------------------ host side

template <bool MS>
void launch_pw_bwd(const PwBwdArgs& a, dim3 grid, int nt, hipStream_t s) {
    dispatch_nt(nt, [&](auto NT) { hipLaunchKernelGGL((pw_bwd_kernel<NT(), MS>), grid, dim3(256), 0, s, a); });
}

// the workspace of one block call, cut into the regions its kernels use side by side
struct BlockWs {
    double* col;      // column-sum partials of whichever producer runs (stream order: its finalize has read them before the next writes)
    float* wg;        // pointwise weight-gradient row slices
    float* taps;      // depthwise tap-gradient partials
    float* coef;      // 3 x [4][Cmax] BnbIn coefficients (null in a layer's workspace without them: sep_ws)
    size_t col_bytes, wg_bytes, taps_bytes, coef_bytes, total;
};

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// persistent workgroups of the depthwise kernels, all slabs together: the 512 a device holds at two per CU — one round, no tail, and a
// quarter of the partial rows of the 2 048 this started with (15.3 -> 15.0 ms per step; 384 / 768 / 1 024: 15.1)
#ifndef FEAR_DW_WGS
#define FEAR_DW_WGS 512
#endif
int dw_bwd_wgs_per_slab(int n_items, int nslab) {
    int target = FEAR_DW_WGS / nslab;
    if (target < 1) target = 1;
    if (target >= n_items) return n_items;
    const int per = (n_items + target - 1) / target;      // items per workgroup, then as few workgroups as that needs
    return (n_items + per - 1) / per;
}
// 32-channel slabs (128-byte rows per pixel and tensor) from 64 channels up, a ragged last slab included (144 = 4.5 slabs: 11 % of
// the lanes idle, against 64-byte segments for all of them with 16-channel slabs: the 24 -> 144 block's pass ran at 3 TB/s)
int dw_bwd_sq(int C) { return C >= 64 ? 8 : 4; }

// The slab geometry of dw_fwd_kernel / dw_bwd_kernel.  From the channels alone: quads per slab, slabs, and the most workgroups per
// slab dw_bwd_wgs_per_slab hands out (what block_ws and irb_scratch size the per-workgroup partials by: dw_slabs).
// Of one launch over B maps of H x W: the forward tiles its OUTPUT map (side 8 at stride 2, else 16), the backward its INPUT map
// (side 16); either takes 8 x 8 tiles on a small map — 5 x 5, stride 1, 8-quad slabs, at most 8 x 8 (the template branch's last
// stage).  The backward's 8 x 8 kernel exists with BatchNorm1 only, so there the rule asks for an expansion as well.
struct DwGeom {
    int sq, nslab, max_wps;
    bool small_map;
    int ts, tiles_x, tiles_y, n_items, wgs_per_slab;      // (n_items = B * tiles_x * tiles_y)
    // the most tiles one workgroup walks (items slot, slot + wgs_per_slab, ...)
    int items_per_wg() const { return wgs_per_slab ? (n_items + wgs_per_slab - 1) / wgs_per_slab : 0; }
    dim3 grid() const { return dim3((unsigned)(wgs_per_slab * nslab)); }
};
DwGeom dw_geom(int cexp, int k, int stride, bool expand, int B, int H, int W, bool backward) {
    DwGeom g{};
    g.sq = dw_bwd_sq(cexp);
    g.nslab = (cexp / 4 + g.sq - 1) / g.sq;
    g.max_wps = FEAR_DW_WGS / g.nslab > 1 ? FEAR_DW_WGS / g.nslab : 1;
    const int h = backward ? H : H / stride, w = backward ? W : W / stride;
    g.small_map = k == 5 && stride == 1 && g.sq == 8 && h <= 8 && w <= 8 && (expand || !backward);
    g.ts = g.small_map || (!backward && stride == 2) ? 8 : 16;
    g.tiles_x = (w + g.ts - 1) / g.ts; g.tiles_y = (h + g.ts - 1) / g.ts;
    g.n_items = B * g.tiles_x * g.tiles_y;
    g.wgs_per_slab = dw_bwd_wgs_per_slab(g.n_items, g.nslab);
    return g;
}
DwGeom dw_slabs(int cexp) { return dw_geom(cexp, 3, 1, false, 0, 0, 0, false); }      // sq, nslab, max_wps only
DwGeom dw_fwd_geom(const FearIrbBlock* b, int B, int H, int W) { return dw_geom(b->cexp, b->k, b->stride, b->expand != 0, B, H, W, false); }
DwGeom dw_bwd_geom(const FearIrbBlock* b, int B, int H, int W) { return dw_geom(b->cexp, b->k, b->stride, b->expand != 0, B, H, W, true); }

// the two regions every unit's workspace starts with: column-sum partials of `rows` rows of at most cmax channels (dw_sums: those of
// the depthwise kernels as well), and the row slices of a pointwise weight gradient of nk elements
size_t ws_col_bytes(long rows, int cmax, bool dw_sums) {
    size_t col = fear_train_stats_workspace_bytes(rows, cmax);
    const size_t colr = (size_t)col_blocks(rows) * 2 * cmax * sizeof(double);
    if (colr > col) col = colr;
    const size_t lds = rows <= FEAR_GEMM_LDS_MAX_ROWS ? (size_t)((rows + 63) / 64) * 2 * cmax * sizeof(double) : 0;      // gemm_lds_kernel: 64-row blocks
    if (lds > col) col = lds;
    const size_t dwp = dw_sums ? (size_t)2048 * 2 * cmax * sizeof(double) : 0;      // dw_bwd_kernel's sums: <= 2048 workgroups per slab
    if (dwp > col) col = dwp;
    return align256(col);
}
size_t ws_wg_bytes(long rows, size_t nk) {
    size_t wg = (size_t)wgrad_slices(rows) * nk * sizeof(float);
    size_t more = (size_t)1024 * nk * sizeof(float);      // room for wgrad_impl's finer row slicing (up to 1 024 slices of small partials)
    if (more > ((size_t)32 << 20)) more = (size_t)32 << 20;
    if (more > wg) wg = more;
    return align256(wg);
}

// the regions' pointers and the total, once the sizes are set (a size query passes base = nullptr: no arithmetic on it — an offset
// applied to a null pointer is undefined behaviour and traps in the UBSan build, libfear_hip_debug.so)
BlockWs ws_cut(BlockWs w, float* base) {
    w.total = w.col_bytes + w.wg_bytes + w.taps_bytes + w.coef_bytes;
    if (base) {
        char* p = reinterpret_cast<char*>(base);
        w.col = reinterpret_cast<double*>(p); p += w.col_bytes;
        w.wg = reinterpret_cast<float*>(p); p += w.wg_bytes;
        w.taps = reinterpret_cast<float*>(p); p += w.taps_bytes;
        w.coef = w.coef_bytes ? reinterpret_cast<float*>(p) : nullptr;
    }
    return w;
}

BlockWs block_ws(long rows_in, long rows_out, int cin, int cexp, int cout, int k, float* base) {
    BlockWs w{};
    const long rows = rows_in > rows_out ? rows_in : rows_out;
    const int cmax = cexp > cout ? (cexp > cin ? cexp : cin) : (cout > cin ? cout : cin);
    w.col_bytes = ws_col_bytes(rows, cmax, true);
    w.wg_bytes = ws_wg_bytes(rows, (size_t)cexp * (cin > cout ? cin : cout));
    w.taps_bytes = align256((size_t)dw_slabs(cexp).max_wps * k * k * cexp * sizeof(float));
    // (also the Gram matrix | column sums of a virtual expansion's input in the forward: up to 32 * 32 + 32 floats)
    w.coef_bytes = align256((size_t)(3 * 4 * cmax > 1056 ? 3 * 4 * cmax : 1056) * sizeof(float));
    return ws_cut(w, base);
}

// ---- SyncBatchNorm hook (include/fear_train.h, fear_train_sync_bind): streams bound to a FearSync.  A handful of entries, looked up
// once per finalize under a mutex (the host side of a step is one thread per rank; the lock is for whoever drives two devices).
struct SyncSlot { hipStream_t s; FearSync sy; bool used; };
SyncSlot g_sync_slots[16];
std::mutex g_sync_mutex;
bool sync_of(hipStream_t s, FearSync* out) {
    std::lock_guard<std::mutex> lock(g_sync_mutex);
    for (const SyncSlot& e : g_sync_slots)
        if (e.used && e.s == s) { *out = e.sy; return true; }
    return false;
}
// the caller's all-reduce of n elements of the sync buffer; false: the callback failed or the buffer is too small — the caller
// launches nothing that consumes the buffer and its entry point returns FEAR_TRAIN_ERR_SYNC at once
[[nodiscard]] bool sync_all_reduce(const FearSync& sy, long n, int is_f32, hipStream_t s) {
    return (size_t)n * (is_f32 ? 4 : 8) <= sy.buf_bytes && sy.all_reduce(sy.user, sy.buf, n, is_f32, s) == 0;
}

// column-sum partials [blocks][2][C] -> mean | rstd | a | b (vec) + running statistics; false: the all-reduce failed, neither is written
[[nodiscard]] bool finalize_forward(const double* partial, int blocks, int C, double count, const float* gamma, const float* beta, float* vec,
                      float* running_mean, float* running_var, double momentum, double eps, hipStream_t s, const float* mean_shift = nullptr) {
    ColFinArgs f = col_fin(partial, blocks, C, 0, count);
    f.out1 = vec; f.out2 = vec + C; f.out_a = vec + 2 * C; f.out_b = vec + 3 * C; f.gamma = gamma; f.beta = beta;
    f.running_mean = running_mean; f.running_var = running_var; f.mean_shift = mean_shift; f.eps = eps; f.momentum = momentum;
    FearSync sy;
    if (sync_of(s, &sy)) {
        // SyncBatchNorm: this rank's float64 sums -> the ranks' all-reduce -> statistics of all ranks' rows
        finalize_sums(partial, blocks, C, sy.buf, s);
        if (!sync_all_reduce(sy, 2L * C, 0, s)) return false;
        f.partial = sy.buf; f.blocks = 1; f.M = count * sy.world;
    }
    launch_col_finalize(f, s);
    return true;
}

// column-sum partials of (g, g * xhat) -> d beta, d gamma, BnbIn coefficients; false: the all-reduce failed, coef is not written
[[nodiscard]] bool finalize_backward(const double* partial, int blocks, int C, double count, const float* gamma, const float* vec, float* dgamma, float* dbeta,
                       float* coef, hipStream_t s) {
    ColFinArgs f = col_fin(partial, blocks, C, 4, count);
    f.out1 = dbeta; f.out2 = dgamma; f.gamma = gamma; f.mean_in = vec; f.rstd_in = vec + C; f.coef = coef;
    FearSync sy;
    if (sync_of(s, &sy)) {
        // SyncBatchNorm: d beta / d gamma from this rank's sums (they are averaged with every other gradient), the input gradient's
        // coefficients from all ranks' — the split torch.nn.SyncBatchNorm makes
        ColFinArgs r = f;
        r.mode = 6; r.dsum = sy.buf;
        launch_col_finalize(r, s);
        if (!sync_all_reduce(sy, 2L * C, 0, s)) return false;
        f.partial = sy.buf; f.blocks = 1; f.out1 = nullptr; f.out2 = nullptr; f.M = count * sy.world;
    }
    launch_col_finalize(f, s);
    return true;
}

// input-gradient GEMM (reduction over Kred, Nout output columns): when the reduction side is the wide one (an expansion's
// gradient coming back to cin channels) the operand — two tensors with the BatchNorm backward formed on load — is what costs,
// so all output tiles go in ONE pass (NT = n_tiles) instead of train_pw_grid's passes of one tile dealt over gridDim.y, which
// re-read it once per pass (672 -> 112 at 16 x 16: 228 us for a 31 us GEMM)
dim3 dgrad_grid(long M, int Kred, int Nout, int* nt) {
    const int n_tiles = (Nout + 15) / 16;
    if (Kred >= 2 * Nout && n_tiles <= 8 && train_pick_nt(n_tiles) == n_tiles) {
        *nt = n_tiles;
        return dim3((unsigned)((M + 127) / 128), 1);
    }
    return train_pw_grid(M, n_tiles, nt);
}

// Grid of the row-tiled GEMMs with a statistics epilogue: train_pw_grid's, with the row blocks of the large maps fattened to
// `row_tiles` 128-row tiles each so that a launch leaves at most ~2 048 partial rows for its finalize (a 128 x 128 map of 128
// crops has 16 384 tiles: 25 MB of float64 partials at 96 channels, a 130 us finalize)
dim3 stat_grid(long M, int K, int N, int* nt, int* row_tiles) {
    dim3 g = dgrad_grid(M, K, N, nt);      // (a projection 672 -> 112 re-reads its normalised-on-load operand once per pass as well)
    // (three tiles per pass instead of six for the narrow reductions of the large maps — twice the occupancy, the small operand
    //  read once more — measured no better: 395 vs 343 us for 16 -> 96 at 128 x 128)
    int rt = (int)((g.x + 2047) / 2048);
    if (rt < 1) rt = 1;
    *row_tiles = rt;
    g.x = (g.x + rt - 1) / rt;
    return g;
}

// Which kernel a row-tiled pointwise GEMM of the block operators takes, and the first generation's grid: with a statistics epilogue
// (`stats`: the forward producers, the masked gradient) stat_grid's, else dgrad_grid's.  pw_forward_unit and launch_bnb_gemm launch by
// it, the plan queries report it.
struct PwGemmPlan { bool lds; int nt, row_tiles; dim3 grid; };
PwGemmPlan pw_gemm_plan(long M, int K, int N, bool stats) {
    PwGemmPlan p{};
    p.nt = 1; p.row_tiles = 1;
    p.lds = gemm_lds_applies(M, K, N);      // few row blocks: the LDS-staged, pipelined GEMM (fear_train_gemm.h), same epilogue
    if (!p.lds) p.grid = stats ? stat_grid(M, K, N, &p.nt, &p.row_tiles) : dgrad_grid(M, K, N, &p.nt);
    return p;
}

template <int KS, int S>
void launch_dw_fwd_ks(const DwFwdArgs& a, int sq, dim3 grid, hipStream_t s) {
    if (sq == 8) hipLaunchKernelGGL((dw_fwd_kernel<KS, S, 8>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((dw_fwd_kernel<KS, S, 4>), grid, dim3(256), 0, s, a);
}

// Y = act(X) W^T + sums -> vec:  the forward producer of a pointwise unit (false: finalize_forward's)
[[nodiscard]] bool pw_forward_unit(const float* x, int ldx, const float* in_vec, int in_relu, const float* w, float* y, long M, int K, int N, const float* gamma,
                     const float* beta, float* vec, float* rm, float* rv, double momentum, double eps, double* col, hipStream_t s,
                     const float* mean_shift = nullptr) {
    int blocks = 0;
    const PwGemmPlan plan = pw_gemm_plan(M, K, N, true);
    if (plan.lds) {
        GemmArgs g{};
        g.X = x; g.ldx = ldx; g.W = w; g.Y = y; g.ldy = N; g.M = (int)M; g.K = K; g.N = N; g.partial = col;
        if (in_vec) { g.in.a = in_vec + 2 * K; g.in.b = in_vec + 3 * K; g.in.relu = in_relu; }
        launch_gemm_lds<1, 1, false>(g, s, &blocks);
    } else {
        PwStatArgs a{};
        a.X = x; a.ldx = ldx; a.W = w; a.Y = y; a.ldy = N; a.M = (int)M; a.K = K; a.N = N;
        if (in_vec) { a.in.a = in_vec + 2 * K; a.in.b = in_vec + 3 * K; a.in.relu = in_relu; }
        a.partial = col;
        a.row_tiles = plan.row_tiles;
        launch_pw_stat(a, plan.grid, plan.nt, s);
        blocks = (int)plan.grid.x;
    }
    return finalize_forward(col, blocks, N, (double)M, gamma, beta, vec, rm, rv, momentum, eps, s, mean_shift);
}

// sums of (g, g * xhat) over rows of (dy, x_raw) [mask: a ReLU behind the BatchNorm] -> d beta, d gamma, coef (false: finalize_backward's)
[[nodiscard]] bool bn_backward_sums(const float* dy, int lddy, const float* raw, int ldx, const float* vec, int relu, const float* gamma, float* dgamma,
                      float* dbeta, float* coef, long M, int C, double* col, hipStream_t s) {
    ColArgs a{};
    a.A = dy; a.lda = lddy; a.X = raw; a.ldx = ldx; a.mean = vec; a.rstd = vec + C;
    a.act_a = relu ? vec + 2 * C : nullptr; a.act_b = relu ? vec + 3 * C : nullptr;
    return finalize_backward(col, launch_col_reduce<1>(a, col, M, C, s), C, (double)M, gamma, vec, dgamma, dbeta, coef, s);
}

template <int KS, int S>
void launch_dw_bwd_ks(const DwBwdArgs& a, int sq, bool bn1, dim3 grid, hipStream_t s) {
    if (sq == 8) {
        if (bn1) hipLaunchKernelGGL((dw_bwd_kernel<KS, S, 8, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((dw_bwd_kernel<KS, S, 8, false>), grid, dim3(256), 0, s, a);
    } else {
        if (bn1) hipLaunchKernelGGL((dw_bwd_kernel<KS, S, 4, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((dw_bwd_kernel<KS, S, 4, false>), grid, dim3(256), 0, s, a);
    }
}

// Events that order the weight-gradient stream behind the kernels that produce its operands: a ring, created on first use and
// never destroyed (a wait refers to the record that preceded it, so re-recording an event later does not disturb waits already
// enqueued; 512 is far more than a step has in flight)
hipEvent_t ring_event() {
    // one ring per device (an event belongs to the device that was current when it was created), positions handed out atomically:
    // two host threads may drive two networks at once
    static hipEvent_t ring[16][512];
    static std::atomic<unsigned> pos{0};
    static std::mutex create;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
    hipEvent_t& e = ring[dev][pos.fetch_add(1) % 512];
    if (!e) {
        std::lock_guard<std::mutex> lock(create);
        if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    }
    return e;
}
// `to` waits for everything issued on `from` so far
bool stream_follow(hipStream_t to, hipStream_t from) {
    hipEvent_t e = ring_event();
    return e && hipEventRecord(e, from) == hipSuccess && hipStreamWaitEvent(to, e, 0) == hipSuccess;
}

int irb_cmax(const FearIrbBlock* b) {
    return b->cexp > b->cout ? (b->cexp > b->cin ? b->cexp : b->cin) : (b->cout > b->cin ? b->cout : b->cin);
}

bool irb_shape_ok(const FearIrbBlock* b, int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return false;
    if (b->cin < 4 || b->cin % 4 || b->cexp < 4 || b->cexp % 4 || b->cout < 4 || b->cout % 4 || b->cexp > 1024 || b->cout > 1024) return false;
    if (!(b->k == 3 || b->k == 5) || !(b->stride == 1 || b->stride == 2) || H % b->stride || W % b->stride) return false;
    if (!b->expand && b->cexp != b->cin) return false;
    if (b->residual && (b->stride != 1 || b->cin != b->cout)) return false;
    if ((long)B * H * W * b->cexp * 4 >= (1L << 31)) return false;      // 32-bit buffer offsets in the depthwise kernels
    return true;
}

// (FEAR_IRB_FUSE_W3: on request only — with the virtual expansions' in-kernel weight gradient already on the chain of input gradients,
//  this one as well makes that chain the longest of the three streams: 14.65 ms with either, 14.84 with both, 14.75 with neither)
bool irb_w3g(const FearIrbBlock* b) { return (b->flags & FEAR_IRB_FUSE_W3) && b->cexp <= 32 && b->cout <= 32 && (b->cexp + 15) / 16 == (b->cout + 15) / 16; }
bool irb_w1g(const FearIrbBlock* b) { return (b->flags & FEAR_IRB_VIRTUAL_E) && b->k == 3; }

// The scratch of fear_irb_train_backward, in this order, in floats; a region the block does not have is null and takes no room
struct IrbScratch {
    float *g2, *g1;                  // [rows_out][cexp] | (expanding blocks) [rows_in][cexp]
    float *coef1, *coef2, *coef3;    // the three BatchNorms' backward coefficients, [4][cmax] each (they must outlive the call when the
                                     // weight gradients run on their own stream, so they do not live in the shared workspace)
    float *wext, *gram;              // (expanding blocks) the E-free backward's extended weights [cexp + cin][cin] | the input's Gram
                                     // matrix [cin][cin], or gram_kernel's [32][32] | column sums (BnbIn)
    float* taps;                     // dw_bwd_kernel's tap-gradient partials [workgroups per slab][k * k][cexp] (summed on the wgrad stream)
    float* w1g;                      // (virtual 3 x 3 expansions) its partials [workgroups per slab][cexp][cin] of the expansion's weight gradient
    float* w3g;                      // (FEAR_IRB_FUSE_W3) the masked-gradient pass's partials [<= 2048][cout][cexp] of the projection's
    size_t total;
};
IrbScratch irb_scratch(const FearIrbBlock* b, int B, int H, int W, float* base) {
    const size_t rows_in = (size_t)B * H * W, rows_out = rows_in / (b->stride * b->stride);
    const size_t cin = b->cin, cexp = b->cexp, cmax = irb_cmax(b), wps = dw_slabs(b->cexp).max_wps;
    IrbScratch r{};
    // (a size query passes base = nullptr: no arithmetic on it, see block_ws)
    auto cut = [&](size_t n) { float* p = base && n ? base + r.total : nullptr; r.total += n; return p; };
    r.g2 = cut(rows_out * cexp);
    r.g1 = cut(b->expand ? rows_in * cexp : 0);
    r.coef1 = cut(4 * cmax);
    r.coef2 = cut(4 * cmax);
    r.coef3 = cut(4 * cmax);
    r.wext = cut(b->expand ? (cexp + cin) * cin : 0);
    r.gram = cut(b->expand ? (cin * cin > 1056 ? cin * cin : 1056) : 0);
    r.taps = cut(wps * b->k * b->k * cexp);
    r.w1g = cut(irb_w1g(b) ? wps * cexp * cin : 0);
    r.w3g = cut(irb_w3g(b) ? (size_t)2048 * b->cout * cexp : 0);
    return r;
}

// the shapes the virtual expansion is built for: the stride-2 blocks with 16 ... 32 input channels and 32-channel slabs (FEAR-XS:
// 16 -> 96 at 128 x 128, 24 -> 144 at 64 x 64, 32 -> 192 at 32 x 32); the stride-1 depthwise backward has no LDS left for the tile of e
bool irb_virtual_shape(const FearIrbBlock* b) {
    return b->expand && b->cin >= 16 && b->cin <= 32 && b->stride == 2 && b->cexp >= 64 && b->cexp % 16 == 0 && !(b->flags & FEAR_IRB_NO_LINEAR_BN1);
}
bool irb_virtual(const FearIrbBlock* b) { return (b->flags & FEAR_IRB_VIRTUAL_E) != 0; }
// BN1's backward without its input (the E-free form, see fear_irb_train_backward): where it applies and pays, or is asked for
// (cexp % 16: a GEMM stage of 16 reduction columns must not straddle g1 and x.)  Always true for a virtual expansion: irb_virtual_shape.
bool irb_lin(const FearIrbBlock* b) {
    return b->expand && b->cexp % 16 == 0 && b->cin <= 128 && !(b->flags & FEAR_IRB_NO_LINEAR_BN1) && (b->cin <= 32 || (b->flags & FEAR_IRB_LINEAR_BN1));
}

// a virtual expansion's kernels by (kernel size, NC = 1 or 2 chunks of 16 input channels): the {3, 5} x {1, 2} of dispatch_ks's (k, stride)
template <class F>
void dispatch_k_nc(int k, int cin, F&& f) { dispatch_ks(k, cin <= 16 ? 1 : 2, f); }

// rows per gram_kernel workgroup: 512 workgroups (one round), in whole steps of 128 rows
long gram_rows_per_wg(long rows) {
    const long rpw = (rows + 511) / 512;
    return (rpw + 127) / 128 * 128;
}
// G = x^T x and the column sums of x (cin <= 32) in one pass: gram_kernel's per-workgroup partials in `wg`, their fixed-order sum
// in `out` as [KP][KP] | [KP].  Returns the row pitch KP = 16 or 32, or FEAR_TRAIN_ERR_WORKSPACE before anything is launched.
int launch_gram(const float* x, long rows, int cin, float* wg, size_t wg_bytes, float* out, hipStream_t s) {
    const long rpw = gram_rows_per_wg(rows);
    const int wgs = (int)((rows + rpw - 1) / rpw);
    const int nc = cin > 16 ? 2 : 1, kp = 16 * nc, per = kp * kp + kp;
    if ((size_t)wgs * per * sizeof(float) > wg_bytes) return FEAR_TRAIN_ERR_WORKSPACE;
    hipLaunchKernelGGL((nc == 1 ? gram_kernel<1> : gram_kernel<2>), dim3((unsigned)wgs), dim3(256), 0, s, x, rows, cin, rpw, wg);
    launch_slice_sum(wg, out, per, wgs, s);
    return kp;
}

// Y = bnb(X) W [+ R]: the pointwise GEMM with a BatchNorm backward formed on its operand as it is loaded (BnbIn) — LDS-staged where
// gemm_lds_applies, else the first generation (pw_bwd_kernel).  Optional: a second operand for the reduction's rows K1 ... K - 1;
// the epilogue of a masked gradient (D: Y is masked by the ReLU behind D, its column sums for the next BatchNorm backward leave in
// `partial` — the return value is their row count for the caller's finalize, or FEAR_TRAIN_ERR_WORKSPACE before anything is
// launched when they do not fit partial_bytes); with that epilogue, a projection's weight gradient summed in the same pass (p3,
// [<= 2048][K][N]: *p3_rows is the number of partials, 0 where the launch has no room for it).
struct BnbGemm {
    const float* X; int ldx; BnbIn bn;
    const float* W;                        // [K][N]
    const float* X2; int ldx2, K1;
    const float* R; int ldr;
    float* Y; int ldy;
    long M; int K, N;
    const float* D; int ldd; const float* dvec; double* partial; size_t partial_bytes;
    float* p3;
};
// (the masked-gradient pass has room for the projection's weight gradient: every column tile in one pass, at most 2 048 partials)
bool w3g_fits(const PwGemmPlan& p, int N) { return !p.lds && p.grid.y == 1 && p.nt == (N + 15) / 16 && p.grid.x <= 2048; }
int launch_bnb_gemm(const BnbGemm& d, hipStream_t s, int* p3_rows = nullptr) {
    const PwGemmPlan plan = pw_gemm_plan(d.M, d.K, d.N, d.D != nullptr);
    if (plan.lds) {
        GemmArgs g{};
        g.X = d.X; g.ldx = d.ldx; g.bn = d.bn; g.W = d.W; g.X2 = d.X2; g.ldx2 = d.ldx2; g.K1 = d.K1; g.R = d.R; g.ldr = d.ldr; g.Y = d.Y; g.ldy = d.ldy;
        g.D = d.D; g.ldd = d.ldd; g.dvec = d.dvec; g.partial = d.partial; g.M = (int)d.M; g.K = d.K; g.N = d.N;
        int blocks = 0;
        // (checked before the launch that writes them: at most one partial row per 64 output rows)
        if (d.D && (size_t)((d.M + 63) / 64) * 2 * d.N * sizeof(double) > d.partial_bytes) return FEAR_TRAIN_ERR_WORKSPACE;
        if (d.D) launch_gemm_lds<2, 2, true>(g, s, &blocks);
        else if (d.X2) launch_gemm_lds<3, 0, true>(g, s, nullptr);
        else launch_gemm_lds<2, 0, true>(g, s, nullptr);
        return blocks;
    }
    PwBwdArgs a{};
    a.G = d.X; a.ldg = d.ldx; a.bn = d.bn; a.W = d.W; a.X2 = d.X2; a.ldx2 = d.ldx2; a.K1 = d.K1; a.R = d.R; a.ldr = d.ldr; a.Y = d.Y; a.ldy = d.ldy;
    a.D = d.D; a.ldd = d.ldd; a.dvec = d.dvec; a.partial = d.partial; a.M = (int)d.M; a.Kred = d.K; a.Nout = d.N;
    const int nt = plan.nt;
    const dim3 grid = plan.grid;
    if (!d.D) {
        launch_pw_bwd<false>(a, grid, nt, s);
        return 0;
    }
    a.row_tiles = plan.row_tiles;
    if ((size_t)grid.x * 2 * d.N * sizeof(double) > d.partial_bytes) return FEAR_TRAIN_ERR_WORKSPACE;
    // the narrow blocks (16 / 24 channels throughout, the 128 x 128 / 64 x 64 maps): the projection's weight gradient in the same pass
    if (d.p3 && p3_rows && w3g_fits(plan, d.N)) {
        a.p3 = d.p3; *p3_rows = (int)grid.x;
        hipLaunchKernelGGL((nt == 1 ? pw_bwd_kernel<1, true, true> : pw_bwd_kernel<2, true, true>), grid, dim3(256), 0, s, a);
    } else {
        launch_pw_bwd<true>(a, grid, nt, s);
    }
    return (int)grid.x;
}

// out = act(a raw + b) [+ residual], a | b from vec = [mean | rstd | a | b]
void launch_bn_act(const float* raw, const float* residual, float* out, const float* vec, int relu, long M, int C, int ldx, int ldr, int ldy,
                   hipStream_t s) {
    BnActArgs k{};
    k.X = raw; k.R = residual; k.Y = out; k.in.a = vec + 2 * C; k.in.b = vec + 3 * C; k.in.relu = relu;
    k.M = M; k.C = C; k.ldx = ldx; k.ldr = ldr; k.ldy = ldy;
    const long n4 = M * (C / 4);
    hipLaunchKernelGGL(bn_act_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, k);
}

// ---- the plan queries (fear_irb_plan_info, fear_pwbn_plan_info): the helpers above, asked what they would launch
FearGemmPlan gemm_info(long M, int K, int N, bool stats, bool x2) {
    const PwGemmPlan p = pw_gemm_plan(M, K, N, stats);
    FearGemmPlan g{};
    g.present = 1; g.lds = p.lds; g.rows = (int32_t)M; g.k = K; g.n = N; g.x2 = x2;
    if (!p.lds) { g.row_tiles = p.row_tiles; g.grid_x = (int32_t)p.grid.x; g.grid_y = (int32_t)p.grid.y; g.nt = p.nt; }
    return g;
}
FearWgradPlan wgrad_info(long M, int K, int N, bool stem, bool dy_masked, bool dy_lin, size_t ws_bytes) {
    const WgradLaunch w = wgrad_launch_plan(M, K, N, 1, stem, dy_masked, dy_lin, ws_bytes);
    FearWgradPlan g{};
    g.present = 1; g.rows = (int32_t)M; g.k = K; g.n = N; g.swapped = w.swapped; g.lds_tile = w.lds_tile;
    g.rows_per_slice = (int32_t)w.plan.rows_per_slice; g.slices = w.plan.slices;
    return g;
}
FearWgradPlan wgrad_fused_info(long M, int K, int N, int partials) {
    FearWgradPlan g{};
    g.present = 2; g.rows = (int32_t)M; g.k = K; g.n = N; g.slices = partials;
    return g;
}
void dw_info(const DwGeom& geo, FearDwPlan* out) {
    out->tiles_x = geo.tiles_x; out->tiles_y = geo.tiles_y; out->tile_side = geo.ts; out->nslab = geo.nslab; out->wgs_per_slab = geo.wgs_per_slab;
    out->items_per_wg = geo.items_per_wg(); out->small_map = geo.small_map;
}

}  // namespace

extern "C" {

int fear_train_sync_bind(void* stream, const FearSync* sync) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (sync && (!sync->all_reduce || !sync->buf)) return FEAR_TRAIN_ERR_NULL;
    if (sync && (sync->world < 1 || sync->buf_bytes < FEAR_SYNC_BUF_BYTES)) return FEAR_TRAIN_ERR_SHAPE;
    std::lock_guard<std::mutex> lock(g_sync_mutex);
    SyncSlot* slot = nullptr;
    for (SyncSlot& e : g_sync_slots)
        if (e.used && e.s == s) slot = &e;
    if (!sync) {
        if (slot) slot->used = false;
        return FEAR_TRAIN_OK;
    }
    if (!slot)
        for (SyncSlot& e : g_sync_slots)
            if (!e.used) { slot = &e; break; }
    if (!slot) return FEAR_TRAIN_ERR_SHAPE;      // more than 16 streams bound
    slot->s = s; slot->sy = *sync; slot->used = true;
    return FEAR_TRAIN_OK;
}

size_t fear_irb_workspace_bytes(const FearIrbBlock* b, int B, int H, int W) {
    if (!b || !irb_shape_ok(b, B, H, W)) return 0;
    const long rows_in = (long)B * H * W, rows_out = rows_in / (b->stride * b->stride);
    return block_ws(rows_in, rows_out, b->cin, b->cexp, b->cout, b->k, nullptr).total;
}

int fear_irb_virtual_ok(const FearIrbBlock* b) { return b && irb_virtual_shape(b) ? 1 : 0; }

size_t fear_irb_scratch_floats(const FearIrbBlock* b, int B, int H, int W) {
    if (!b || !irb_shape_ok(b, B, H, W)) return 0;
    return irb_scratch(b, B, H, W, nullptr).total;
}

int fear_irb_plan_info(const FearIrbBlock* b, int B, int H, int W, FearIrbPlanInfo* out) {
    if (!b || !out) return FEAR_TRAIN_ERR_NULL;
    if (!irb_shape_ok(b, B, H, W) || (irb_virtual(b) && !irb_virtual_shape(b))) return FEAR_TRAIN_ERR_SHAPE;
    const long rows_in = (long)B * H * W, rows_out = rows_in / (b->stride * b->stride);
    const int cin = b->cin, cexp = b->cexp, cout = b->cout;
    const BlockWs ws = block_ws(rows_in, rows_out, cin, cexp, cout, b->k, nullptr);
    const bool virt = irb_virtual(b), lin = irb_lin(b);
    FearIrbPlanInfo r{};
    r.rows_in = (int32_t)rows_in; r.rows_out = (int32_t)rows_out; r.lin = lin; r.virtual_e = virt;
    // forward: expansion (unless virtual), depthwise, projection
    if (b->expand && !virt) r.expand = gemm_info(rows_in, cin, cexp, true, false);
    dw_info(dw_fwd_geom(b, B, H, W), &r.dw_fwd);
    r.project = gemm_info(rows_out, cexp, cout, true, false);
    // backward: BatchNorm3's sums, masked gradient (+ dW3), depthwise (+ dW1 of a virtual 3 x 3), dW1, dx
    r.col_rows_in = col_rows_per_block(rows_in); r.col_rows_out = col_rows_per_block(rows_out);
    r.wgrad_rows_per_slice = (int32_t)wgrad_rows_per_slice(rows_in);
    const PwGemmPlan g2 = pw_gemm_plan(rows_out, cout, cexp, true);
    r.g2 = gemm_info(rows_out, cout, cexp, true, false);
    r.w3 = irb_w3g(b) && w3g_fits(g2, cexp) ? wgrad_fused_info(rows_out, cexp, cout, (int)g2.grid.x)
                                            : wgrad_info(rows_out, cexp, cout, false, false, false, ws.wg_bytes);
    const DwGeom bwd = dw_bwd_geom(b, B, H, W);
    dw_info(bwd, &r.dw_bwd);
    if (b->expand) {
        r.w1 = irb_w1g(b) ? wgrad_fused_info(rows_in, cin, cexp, bwd.wgs_per_slab) : wgrad_info(rows_in, cin, cexp, false, false, lin, ws.wg_bytes);
        r.dx = gemm_info(rows_in, lin ? cexp + cin : cexp, cin, false, lin);
        if (virt || (lin && cin <= 32)) r.gram_rows_per_wg = (int32_t)gram_rows_per_wg(rows_in);
    }
    *out = r;
    return FEAR_TRAIN_OK;
}

int fear_irb_train_forward(const FearIrbBlock* b, const FearIrbSaved* sv, const float* x, float* out, int B, int H, int W, double momentum,
                           double eps, float* workspace, size_t ws_bytes, void* stream) {
    if (!b || !sv || !x || !out || !workspace || !sv->d || !sv->p || !sv->vec[1] || !sv->vec[2] || !b->w_dw || !b->w_pwl) return FEAR_TRAIN_ERR_NULL;
    if (b->expand && ((!sv->e && !irb_virtual(b)) || !sv->vec[0] || !b->w_pw)) return FEAR_TRAIN_ERR_NULL;
    for (int i = b->expand ? 0 : 1; i < 3; ++i)
        if (!b->gamma[i] || !b->beta[i]) return FEAR_TRAIN_ERR_NULL;
    if (!irb_shape_ok(b, B, H, W) || (irb_virtual(b) && !irb_virtual_shape(b))) return FEAR_TRAIN_ERR_SHAPE;
    const long rows_in = (long)B * H * W, rows_out = rows_in / (b->stride * b->stride);
    const BlockWs ws = block_ws(rows_in, rows_out, b->cin, b->cexp, b->cout, b->k, workspace);
    if (ws_bytes < ws.total) return FEAR_TRAIN_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool virt = irb_virtual(b);
    if (virt) {
        // BatchNorm1's statistics of the expansion that is never written: G = x^T x and the column sums of x in one pass, then W1 on them
        const int kp = b->cin > 16 ? 32 : 16, per = kp * kp + kp;
        if (ws.coef_bytes < per * sizeof(float)) return FEAR_TRAIN_ERR_WORKSPACE;
        const int rc = launch_gram(x, rows_in, b->cin, ws.wg, ws.wg_bytes, ws.coef, s);
        if (rc < 0) return rc;
        double count1 = (double)rows_in;
        FearSync sy;
        if (sync_of(s, &sy)) {
            // SyncBatchNorm: the expansion's statistics are linear in (G, column sums) — those are what the ranks add up
            if (hipMemcpyAsync(sy.buf, ws.coef, per * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) return FEAR_TRAIN_ERR_HIP;
            if (!sync_all_reduce(sy, per, 1, s)) return FEAR_TRAIN_ERR_SYNC;
            if (hipMemcpyAsync(ws.coef, sy.buf, per * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) return FEAR_TRAIN_ERR_HIP;
            count1 *= sy.world;
        }
        hipLaunchKernelGGL((kp == 16 ? irb_virtual_stats_kernel<16> : irb_virtual_stats_kernel<32>), dim3((unsigned)((b->cexp + 63) / 64)), dim3(64), 0, s,
                           ws.coef, b->w_pw, b->gamma[0], b->beta[0], sv->vec[0], b->running_mean[0], b->running_var[0], b->cexp, b->cin, count1, eps,
                           momentum);
    }
    // expand 1x1 (+ statistics)
    if (b->expand && !virt &&
        !pw_forward_unit(x, b->cin, nullptr, 0, b->w_pw, sv->e, rows_in, b->cin, b->cexp, b->gamma[0], b->beta[0], sv->vec[0], b->running_mean[0],
                         b->running_var[0], momentum, eps, ws.col, s))
        return FEAR_TRAIN_ERR_SYNC;
    // depthwise over act1(e) (or over the block input) (+ statistics)
    {
        const DwGeom geo = dw_fwd_geom(b, B, H, W);
        DwFwdArgs a{};
        a.X = b->expand ? sv->e : x; a.ldx = b->cexp; a.Wt = b->w_dw; a.Y = sv->d; a.ldy = b->cexp;
        a.B = B; a.H = H; a.W = W; a.C = b->cexp; a.Ho = H / b->stride; a.Wo = W / b->stride;
        if (b->expand) { a.in.a = sv->vec[0] + 2 * b->cexp; a.in.b = sv->vec[0] + 3 * b->cexp; a.in.relu = 1; }
        a.tiles_x = geo.tiles_x; a.tiles_y = geo.tiles_y; a.nslab = geo.nslab; a.wgs_per_slab = geo.wgs_per_slab;
        a.psums = ws.col;
        const dim3 grid = geo.grid();
        if (virt) {
            a.X = nullptr; a.ve.X = x; a.ve.W1 = b->w_pw; a.ve.cin = b->cin;
            dispatch_k_nc(b->k, b->cin, [&](auto KS, auto NC) { hipLaunchKernelGGL((dw_fwd_kernel<KS(), 2, 8, NC()>), grid, dim3(256), 0, s, a); });
        } else if (geo.small_map) hipLaunchKernelGGL((dw_fwd_kernel<5, 1, 8, 0, 8>), grid, dim3(256), 0, s, a);
        else dispatch_ks(b->k, b->stride, [&](auto KS, auto S) { launch_dw_fwd_ks<KS(), S()>(a, geo.sq, grid, s); });
        if (!finalize_forward(ws.col, geo.wgs_per_slab, b->cexp, (double)rows_out, b->gamma[1], b->beta[1], sv->vec[1], b->running_mean[1],
                              b->running_var[1], momentum, eps, s))
            return FEAR_TRAIN_ERR_SYNC;
    }
    // project 1x1 over act2(d) (+ statistics)
    if (!pw_forward_unit(sv->d, b->cexp, sv->vec[1], 1, b->w_pwl, sv->p, rows_out, b->cexp, b->cout, b->gamma[2], b->beta[2], sv->vec[2],
                         b->running_mean[2], b->running_var[2], momentum, eps, ws.col, s))
        return FEAR_TRAIN_ERR_SYNC;
    // block output = BN3(p) [+ x]
    launch_bn_act(sv->p, b->residual ? x : nullptr, out, sv->vec[2], 0, rows_out, b->cout, b->cout, b->cin, b->cout, s);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_irb_train_backward(const FearIrbBlock* b, const FearIrbSaved* sv, const FearIrbGrads* gr, const float* x, const float* dout, float* dx,
                            float* scratch, int B, int H, int W, float* workspace, size_t ws_bytes, void* stream, void* wgrad_stream) {
    if (!b || !sv || !gr || !x || !dout || !scratch || !workspace || !sv->d || !sv->p || !sv->vec[1] || !sv->vec[2] || !gr->w_dw || !gr->w_pwl)
        return FEAR_TRAIN_ERR_NULL;
    if (b->expand && ((!sv->e && !irb_virtual(b)) || !sv->vec[0] || !gr->w_pw)) return FEAR_TRAIN_ERR_NULL;
    if (!b->expand && !dx) return FEAR_TRAIN_ERR_NULL;
    for (int i = b->expand ? 0 : 1; i < 3; ++i)
        if (!gr->gamma[i] || !gr->beta[i] || !b->gamma[i]) return FEAR_TRAIN_ERR_NULL;
    if (!irb_shape_ok(b, B, H, W) || (irb_virtual(b) && !irb_virtual_shape(b))) return FEAR_TRAIN_ERR_SHAPE;
    const long rows_in = (long)B * H * W, rows_out = rows_in / (b->stride * b->stride);
    const BlockWs ws = block_ws(rows_in, rows_out, b->cin, b->cexp, b->cout, b->k, workspace);
    if (ws_bytes < ws.total) return FEAR_TRAIN_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int cexp = b->cexp, cout = b->cout, cin = b->cin;
    const IrbScratch sc = irb_scratch(b, B, H, W, scratch);
    // the two pointwise weight gradients are off the chain that leads to dx: with a `wgrad_stream` they are issued there, behind
    // an event that follows the kernels producing their operands, and overlap the rest of this block's (and the next blocks')
    // backward — every kernel of a 16 x 16 map is a few hundred workgroups and leaves most of the device idle on its own
    hipStream_t sw = wgrad_stream ? static_cast<hipStream_t>(wgrad_stream) : s;
    // BN3 (no ReLU): sums over (dout, p)
    if (!bn_backward_sums(dout, cout, sv->p, cout, sv->vec[2], 0, b->gamma[2], gr->gamma[2], gr->beta[2], sc.coef3, rows_out, cout, ws.col, s))
        return FEAR_TRAIN_ERR_SYNC;
    BnbIn bn3{};
    bn3.E = sv->p; bn3.coef = sc.coef3; bn3.lde = cout; bn3.C = cout;
    // g2 = (dp W3) masked by act2(d) > 0, + sums of (g2, dhat)
    int w3g_slices = 0;      // > 0: the projection's weight gradient was summed in that pass
    const int blocks = launch_bnb_gemm({.X = dout, .ldx = cout, .bn = bn3, .W = b->w_pwl, .Y = sc.g2, .ldy = cexp, .M = rows_out, .K = cout, .N = cexp,
                                        .D = sv->d, .ldd = cexp, .dvec = sv->vec[1], .partial = ws.col, .partial_bytes = ws.col_bytes, .p3 = sc.w3g},
                                       s, &w3g_slices);
    if (blocks < 0) return blocks;
    if (!finalize_backward(ws.col, blocks, cexp, (double)rows_out, b->gamma[1], sv->vec[1], gr->gamma[1], gr->beta[1], sc.coef2, s))
        return FEAR_TRAIN_ERR_SYNC;
    // dW3 = dp^T act2(d)
    if (sw != s && !stream_follow(sw, s)) return FEAR_TRAIN_ERR_HIP;      // coef3 exists
    if (w3g_slices) {
        launch_slice_sum(sc.w3g, gr->w_pwl, (long)cout * cexp, w3g_slices, sw);
    } else {
        const int rc = wgrad_impl({.dy = dout, .lddy = cout, .x = sv->d, .ldx = cexp, .dw = gr->w_pwl, .workspace = ws.wg, .ws_bytes = ws.wg_bytes,
                                   .M = rows_out, .K = cexp, .N = cout, .s = sw, .act_a = sv->vec[1] + 2 * cexp, .act_b = sv->vec[1] + 3 * cexp,
                                   .act_relu = 1, .bn = &bn3});
        if (rc != FEAR_TRAIN_OK) return rc;
    }
    // depthwise + both BatchNorms around it
    {
        const DwGeom geo = dw_bwd_geom(b, B, H, W);
        DwBwdArgs a{};
        a.G2 = sc.g2; a.D = sv->d; a.ldo = cexp; a.coef2 = sc.coef2; a.Wt = b->w_dw;
        a.E = b->expand ? sv->e : x; a.lde = cexp; a.act1 = b->expand ? sv->vec[0] : nullptr;
        a.R = (!b->expand && b->residual) ? dout : nullptr; a.ldr = cout;
        a.Y = b->expand ? sc.g1 : dx; a.ldy = cexp;
        a.ptaps = sc.taps; a.psums = ws.col;
        a.B = B; a.H = H; a.W = W; a.Ho = H / b->stride; a.Wo = W / b->stride; a.C = cexp;
        a.tiles_x = geo.tiles_x; a.tiles_y = geo.tiles_y; a.nslab = geo.nslab; a.wgs_per_slab = geo.wgs_per_slab;
        const dim3 grid = geo.grid();
        if (irb_virtual(b)) {
            a.E = nullptr; a.ve.X = x; a.ve.W1 = b->w_pw; a.ve.cin = cin;
            a.pw1 = sc.w1g;      // (3 x 3: the expansion's weight gradient in the same pass)
            dispatch_k_nc(b->k, cin, [&](auto KS, auto NC) {
                if constexpr (decltype(KS)::value == 3) {
                    if (a.pw1) {
                        hipLaunchKernelGGL((dw_bwd_kernel<3, 2, 8, true, NC(), 16, true>), grid, dim3(256), 0, s, a);
                        return;
                    }
                }
                hipLaunchKernelGGL((dw_bwd_kernel<KS(), 2, 8, true, NC()>), grid, dim3(256), 0, s, a);
            });
        } else if (geo.small_map) hipLaunchKernelGGL((dw_bwd_kernel<5, 1, 8, true, 0, 8>), grid, dim3(256), 0, s, a);
        else dispatch_ks(b->k, b->stride, [&](auto KS, auto S) { launch_dw_bwd_ks<KS(), S()>(a, geo.sq, b->expand != 0, grid, s); });
        if (b->expand &&
            !finalize_backward(ws.col, a.wgs_per_slab, cexp, (double)rows_in, b->gamma[0], sv->vec[0], gr->gamma[0], gr->beta[0], sc.coef1, s))
            return FEAR_TRAIN_ERR_SYNC;
        // the tap gradients' final sum is a weight gradient too: off the chain (the partials live in the call's private scratch)
        if (sw != s && !stream_follow(sw, s)) return FEAR_TRAIN_ERR_HIP;          // the partials, g1 and coef1 exist
        launch_slice_sum(sc.taps, gr->w_dw, (long)b->k * b->k * cexp, a.wgs_per_slab, sw);
        if (a.pw1) launch_slice_sum(a.pw1, gr->w_pw, (long)cexp * cin, a.wgs_per_slab, sw);      // R[c][k], completed below
    }
    if (b->expand) {
        // BN1's backward without its input: e = x W1^T is linear in the block input, so both consumers read g1 (cexp channels) and x
        // (cin channels) instead of g1 and e — see BnbIn.  G = x^T x and the two small correction kernels are the price.
        // where it pays — 16-32 input channels, the expansions of the 128 x 128 ... 32 x 32 maps: bandwidth-bound launches that read
        // 0.1-0.8 GB less each (16.71 -> 16.49 ms per step).  With 64 / 112 input channels (the 16 x 16 maps) the T kernel on the
        // chain, the Gram matrix and the correction cost more than the lighter loads save: 16.64 / 16.80 ms with those included.
        const bool lin = irb_lin(b);
        BnbIn bn1{};
        bn1.coef = sc.coef1; bn1.C = cexp;
        if (!lin) { bn1.E = sv->e; bn1.lde = cexp; }
        int rc = FEAR_TRAIN_OK, ldg = cin;
        // (cin <= 32: the one-load-per-four-rows Gram kernel of the virtual expansion's forward; its result is [KP][KP] | column sums)
        if (lin && cin <= 32) rc = ldg = launch_gram(x, rows_in, cin, ws.wg, ws.wg_bytes, sc.gram, sw);
        else if (lin)
            rc = wgrad_impl({.dy = x, .lddy = cin, .x = x, .ldx = cin, .dw = sc.gram, .workspace = ws.wg, .ws_bytes = ws.wg_bytes, .M = rows_in,
                             .K = cin, .N = cin, .s = sw});
        if (rc < 0) return rc;
        const bool w1g = irb_w1g(b);      // (then lin and cin <= 32: the Gram kernel's [KP][KP] | column sums above)
        rc = w1g ? FEAR_TRAIN_OK
                 : wgrad_impl({.dy = sc.g1, .lddy = cexp, .x = x, .ldx = cin, .dw = gr->w_pw, .workspace = ws.wg, .ws_bytes = ws.wg_bytes,
                               .M = rows_in, .K = cin, .N = cexp, .s = sw, .bn = &bn1});
        if (rc != FEAR_TRAIN_OK) return rc;
        if (w1g || lin)
            hipLaunchKernelGGL((w1g ? irb_lin_wgrad_fix2_kernel : irb_lin_wgrad_fix_kernel), dim3((unsigned)((cexp * cin + 255) / 256)), dim3(256), 0, sw,
                               sc.coef1, b->w_pw, sc.gram, ldg, gr->w_pw, cexp, cin);
        if (dx) {
            BnbGemm g{.X = sc.g1, .ldx = cexp, .bn = bn1, .W = b->w_pw, .R = b->residual ? dout : nullptr, .ldr = cout, .Y = dx, .ldy = cin,
                      .M = rows_in, .K = cexp, .N = cin};
            if (lin) {
                int kp_log2 = 4;
                while ((1 << kp_log2) < cin) ++kp_log2;
                hipLaunchKernelGGL(irb_lin_weights_kernel, dim3((unsigned)(cin + (cexp * cin + 1023) / 1024)), dim3(1024), 0, s, sc.coef1, b->w_pw,
                                   sc.wext, cexp, cin, kp_log2);
                g.W = sc.wext; g.X2 = x; g.ldx2 = cin; g.K1 = cexp; g.K = cexp + cin;
            }
            launch_bnb_gemm(g, s);
        }
    }
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_bn_running_update(const float* vec, double count, float* running_mean, float* running_var, double momentum, double eps, int C,
                           void* stream) {
    if (!vec || !running_mean || !running_var) return FEAR_TRAIN_ERR_NULL;
    if (C < 1 || !(count >= 1.0)) return FEAR_TRAIN_ERR_SHAPE;
    hipLaunchKernelGGL(bn_running_update_kernel, dim3((C + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), vec, running_mean,
                       running_var, C, count, momentum, eps);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_bn_running_update_multi(const FearBnRunning* items, int n, double momentum, double eps, void* stream) {
    if (!items || n < 0) return FEAR_TRAIN_ERR_NULL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int i = 0; i < n; ++i) {      // every item before the first launch: an error leaves all n BatchNorms as they were
        const FearBnRunning& it = items[i];
        if (!it.vec || !it.running_mean || !it.running_var) return FEAR_TRAIN_ERR_NULL;
        if (it.C < 1 || !(it.count >= 1.0)) return FEAR_TRAIN_ERR_SHAPE;
    }
    for (int i0 = 0; i0 < n; i0 += 64) {
        BnRunMulti t{};
        const int m = n - i0 < 64 ? n - i0 : 64;
        for (int i = 0; i < m; ++i) {
            const FearBnRunning& it = items[i0 + i];
            t.vec[i] = it.vec; t.rm[i] = it.running_mean; t.rv[i] = it.running_var; t.C[i] = it.C; t.count[i] = it.count;
        }
        hipLaunchKernelGGL(bn_running_update_multi_kernel, dim3((unsigned)m), dim3(256), 0, s, t, momentum, eps);
    }
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

size_t fear_pwbn_workspace_bytes(long M, int K, int N) {
    if (M < 1 || K < 4 || N < 4) return 0;
    return block_ws(M, M, K, N, N, 3, nullptr).total;
}

int fear_pwbn_plan_info(long M, int K, int N, int relu, int stem, FearPwbnPlanInfo* out) {
    if (!out) return FEAR_TRAIN_ERR_NULL;
    if (!pw_shape_ok(M, K, N) || N > 1024 || M > 0x7fffffffL || (stem && (K != 28 || N != 16 || !relu))) return FEAR_TRAIN_ERR_SHAPE;
    const BlockWs ws = block_ws(M, M, K, N, N, 3, nullptr);
    FearPwbnPlanInfo r{};
    r.rows = (int32_t)M;
    if (stem) {      // fear_stem_train_forward: pw_stat_kernel on stat_grid whatever the shape, and no input gradient
        int nt = 1, row_tiles = 1;
        const dim3 grid = stat_grid(M, K, N, &nt, &row_tiles);
        r.forward.present = 1; r.forward.rows = (int32_t)M; r.forward.k = K; r.forward.n = N;
        r.forward.row_tiles = row_tiles; r.forward.grid_x = (int32_t)grid.x; r.forward.grid_y = (int32_t)grid.y; r.forward.nt = nt;
    } else {
        r.forward = gemm_info(M, K, N, true, false);
        r.dx = gemm_info(M, N, K, false, false);
    }
    r.col_rows = col_rows_per_block(M);
    r.w = wgrad_info(M, K, N, stem != 0, relu != 0, false, ws.wg_bytes);
    *out = r;
    return FEAR_TRAIN_OK;
}

int fear_pwbn_train_forward(const float* x, int ldx, const float* w, const float* gamma, const float* beta, float* running_mean,
                            float* running_var, float* raw, float* vec, int relu, float* out, long M, int K, int N, double momentum, double eps,
                            float* workspace, size_t ws_bytes, void* stream) {
    if (!x || !w || !gamma || !beta || !raw || !vec || !out || !workspace) return FEAR_TRAIN_ERR_NULL;
    if (!pw_shape_ok(M, K, N) || N > 1024 || M > 0x7fffffffL || !ld_ok(ldx, K)) return FEAR_TRAIN_ERR_SHAPE;
    const BlockWs ws = block_ws(M, M, K, N, N, 3, workspace);
    if (ws_bytes < ws.total) return FEAR_TRAIN_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!pw_forward_unit(x, ldx, nullptr, 0, w, raw, M, K, N, gamma, beta, vec, running_mean, running_var, momentum, eps, ws.col, s))
        return FEAR_TRAIN_ERR_SYNC;
    launch_bn_act(raw, nullptr, out, vec, relu, M, N, N, 0, N, s);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_pwbn_train_backward(const float* dy, const float* raw, const float* vec, int relu, const float* x, int ldx, const float* w,
                             const float* gamma, float* dw, float* dgamma, float* dbeta, float* dx, long M, int K, int N, float* workspace,
                             size_t ws_bytes, void* stream, void* wgrad_stream) {
    if (!dy || !raw || !vec || !x || !w || !gamma || !dw || !dgamma || !dbeta || !workspace) return FEAR_TRAIN_ERR_NULL;
    if (!pw_shape_ok(M, K, N) || N > 1024 || M > 0x7fffffffL || !ld_ok(ldx, K)) return FEAR_TRAIN_ERR_SHAPE;
    const BlockWs ws = block_ws(M, M, K, N, N, 3, workspace);
    if (ws_bytes < ws.total) return FEAR_TRAIN_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipStream_t sw = wgrad_stream ? static_cast<hipStream_t>(wgrad_stream) : s;
    // (this unit's coefficient vectors live in the shared workspace: whatever an earlier call left running on the weight-gradient
    //  stream may still read them — it is waited for first)
    if (sw != s && !stream_follow(s, sw)) return FEAR_TRAIN_ERR_HIP;
    if (!bn_backward_sums(dy, N, raw, N, vec, relu, gamma, dgamma, dbeta, ws.coef, M, N, ws.col, s)) return FEAR_TRAIN_ERR_SYNC;
    BnbIn bn{};
    bn.E = raw; bn.coef = ws.coef; bn.lde = N; bn.C = N;
    if (relu) { bn.mask_a = vec + 2 * N; bn.mask_b = vec + 3 * N; }
    if (dx) launch_bnb_gemm({.X = dy, .ldx = N, .bn = bn, .W = w, .Y = dx, .ldy = K, .M = M, .K = N, .N = K}, s);
    if (sw != s && !stream_follow(sw, s)) return FEAR_TRAIN_ERR_HIP;
    const int rc = wgrad_impl({.dy = dy, .lddy = N, .x = x, .ldx = ldx, .dw = dw, .workspace = ws.wg, .ws_bytes = ws.wg_bytes, .M = M, .K = K, .N = N,
                               .s = sw, .bn = &bn});
    if (rc != FEAR_TRAIN_OK) return rc;
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

// ------------------------------------------------------------------------------------------------
// SepConv (depthwise 3 x 3 + pointwise, both with bias) + BatchNorm + ReLU — the layer the head's towers are made of
// (model_training/model/blocks.py:97-101, 115-119, 151-161) — one call per direction, in the style of the trunk's blocks:
//   forward   d = dw(x) + b_dw;  raw = d W^T (statistics in the GEMM's epilogue; the pointwise bias is left out: it cancels in the
//             normalisation and only shifts the tracked mean);  out = relu(a raw + b)
//   backward  sums over (dy masked, raw) -> coefficients;  dd = bnb(dy) W (the BatchNorm backward formed on load);  dx = DW^T dd;
//             d W = bnb(dy)^T d and the tap gradients on `wgrad_stream`, off the chain of input gradients
// workspace regions: col (stream) | wg, taps (wgrad stream only)
static BlockWs sep_ws(long M, int cin, int cout, float* base) {
    BlockWs w{};
    w.col_bytes = ws_col_bytes(M, cin > cout ? cin : cout, false);
    w.wg_bytes = ws_wg_bytes(M, (size_t)cin * cout);
    w.taps_bytes = align256((size_t)col_blocks(M) * 9 * cin * sizeof(float));
    return ws_cut(w, base);
}

static bool sep_shape_ok(const FearSepLayer* L, int B, int H, int W) {
    return L && B >= 1 && H >= 1 && W >= 1 && L->cin >= 4 && L->cin % 4 == 0 && L->cin <= 1024 && L->cout >= 4 && L->cout % 4 == 0 &&
           L->cout <= 1024 && (long)B * H * W * (L->cin > L->cout ? L->cin : L->cout) * 4 < 0x7fffffffL;
}

size_t fear_sepbn_workspace_bytes(const FearSepLayer* L, int B, int H, int W) {
    if (!sep_shape_ok(L, B, H, W)) return 0;
    return sep_ws((long)B * H * W, L->cin, L->cout, nullptr).total;
}

int fear_sepbn_train_forward(const FearSepLayer* L, const float* x, int ldx, float* d, float* raw, float* vec, float* out, int ldo, int B,
                             int H, int W, double momentum, double eps, float* workspace, size_t ws_bytes, void* stream) {
    if (!L || !x || !d || !raw || !vec || !out || !workspace || !L->w_dw || !L->w_pw || !L->gamma || !L->beta) return FEAR_TRAIN_ERR_NULL;
    if (!sep_shape_ok(L, B, H, W) || !ld_ok(ldx, L->cin) || !ld_ok(ldo, L->cout)) return FEAR_TRAIN_ERR_SHAPE;
    const long M = (long)B * H * W;
    const int K = L->cin, N = L->cout;
    const BlockWs ws = sep_ws(M, K, N, workspace);
    if (ws_bytes < ws.total) return FEAR_TRAIN_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = dw_impl(x, ldx, L->w_dw, L->b_dw, d, K, B, H, W, K, 3, 1, s);
    if (rc != FEAR_TRAIN_OK) return rc;
    if (!pw_forward_unit(d, K, nullptr, 0, L->w_pw, raw, M, K, N, L->gamma, L->beta, vec, L->running_mean, L->running_var, momentum, eps, ws.col, s,
                         L->b_pw))
        return FEAR_TRAIN_ERR_SYNC;
    launch_bn_act(raw, nullptr, out, vec, 1, M, N, N, 0, ldo, s);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_sepbn_train_backward(const FearSepLayer* L, const FearSepGrads* gr, const float* x, int ldx, const float* d, const float* raw,
                              const float* vec, const float* dy, float* dd, float* coef, float* dx, int B, int H, int W, float* workspace,
                              size_t ws_bytes, void* stream, void* wgrad_stream) {
    if (!L || !gr || !x || !d || !raw || !vec || !dy || !dd || !coef || !dx || !workspace || !L->w_dw || !L->w_pw || !L->gamma)
        return FEAR_TRAIN_ERR_NULL;
    if (!gr->w_dw || !gr->w_pw || !gr->gamma || !gr->beta) return FEAR_TRAIN_ERR_NULL;
    if (!sep_shape_ok(L, B, H, W) || !ld_ok(ldx, L->cin)) return FEAR_TRAIN_ERR_SHAPE;
    const long M = (long)B * H * W;
    const int K = L->cin, N = L->cout;
    const BlockWs ws = sep_ws(M, K, N, workspace);
    if (ws_bytes < ws.total) return FEAR_TRAIN_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipStream_t sw = wgrad_stream ? static_cast<hipStream_t>(wgrad_stream) : s;
    if (!bn_backward_sums(dy, N, raw, N, vec, 1, L->gamma, gr->gamma, gr->beta, coef, M, N, ws.col, s)) return FEAR_TRAIN_ERR_SYNC;
    BnbIn bn{};
    bn.E = raw; bn.coef = coef; bn.lde = N; bn.C = N; bn.mask_a = vec + 2 * N; bn.mask_b = vec + 3 * N;
    launch_bnb_gemm({.X = dy, .ldx = N, .bn = bn, .W = L->w_pw, .Y = dd, .ldy = K, .M = M, .K = N, .N = K}, s);
    if (sw != s && !stream_follow(sw, s)) return FEAR_TRAIN_ERR_HIP;
    int rc = wgrad_impl({.dy = dy, .lddy = N, .x = d, .ldx = K, .dw = gr->w_pw, .workspace = ws.wg, .ws_bytes = ws.wg_bytes, .M = M, .K = K, .N = N,
                         .s = sw, .bn = &bn});
    if (rc != FEAR_TRAIN_OK) return rc;
    rc = dw_wgrad_impl(dd, K, x, ldx, gr->w_dw, ws.taps, ws.taps_bytes, B, H, W, K, 3, 1, sw, nullptr, nullptr, 0);
    if (rc != FEAR_TRAIN_OK) return rc;
    rc = dw_dgrad_impl(dd, K, L->w_dw, dx, K, B, H, W, K, 3, 1, s);
    if (rc != FEAR_TRAIN_OK) return rc;
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

// ------------------------------------------------------------------------------------------------
// The stem (3 x 3 stride-2 conv 3 -> 16 + BatchNorm + ReLU, fbnet_c stages[0]) on the NCHW image: fear_pwbn_train_* over
// fear_stem_im2col's rows with the rows never materialised — the forward GEMM and the weight gradient gather them (StemIn).
static bool stem_shape_ok(long n, int H, int W) { return n >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && n * (H / 2) * (W / 2) < 0x7fffffffL / 28; }

size_t fear_stem_workspace_bytes(long n, int H, int W) {
    if (!stem_shape_ok(n, H, W)) return 0;
    const long M = n * (H / 2) * (W / 2);
    return block_ws(M, M, 28, 16, 16, 3, nullptr).total;
}

int fear_stem_train_forward(const float* x_nchw, const float* w, const float* gamma, const float* beta, float* running_mean, float* running_var,
                            float* raw, float* vec, float* out, long n, int H, int W, double momentum, double eps, float* workspace,
                            size_t ws_bytes, void* stream) {
    if (!x_nchw || !w || !gamma || !beta || !raw || !vec || !out || !workspace) return FEAR_TRAIN_ERR_NULL;
    if (!stem_shape_ok(n, H, W)) return FEAR_TRAIN_ERR_SHAPE;
    const long M = n * (H / 2) * (W / 2);
    const BlockWs ws = block_ws(M, M, 28, 16, 16, 3, workspace);
    if (ws_bytes < ws.total) return FEAR_TRAIN_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    PwStatArgs a{};
    a.stem_img = x_nchw; a.stem_H = H; a.stem_W = W; a.W = w; a.Y = raw; a.ldy = 16; a.M = (int)M; a.K = 28; a.N = 16; a.partial = ws.col;
    int nt = 1;
    const dim3 grid = stat_grid(M, 28, 16, &nt, &a.row_tiles);      // (16 output channels: one column tile, nt = 1)
    if (nt != 1 || (size_t)grid.x * 2 * 16 * sizeof(double) > ws.col_bytes) return FEAR_TRAIN_ERR_WORKSPACE;
    hipLaunchKernelGGL((pw_stat_kernel<1, true>), grid, dim3(256), 0, s, a);
    if (!finalize_forward(ws.col, (int)grid.x, 16, (double)M, gamma, beta, vec, running_mean, running_var, momentum, eps, s)) return FEAR_TRAIN_ERR_SYNC;
    launch_bn_act(raw, nullptr, out, vec, 1, M, 16, 16, 0, 16, s);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_stem_train_backward(const float* dy, const float* raw, const float* vec, const float* x_nchw, const float* gamma, float* dw,
                             float* dgamma, float* dbeta, long n, int H, int W, float* workspace, size_t ws_bytes, void* stream,
                             void* wgrad_stream) {
    if (!dy || !raw || !vec || !x_nchw || !gamma || !dw || !dgamma || !dbeta || !workspace) return FEAR_TRAIN_ERR_NULL;
    if (!stem_shape_ok(n, H, W)) return FEAR_TRAIN_ERR_SHAPE;
    const long M = n * (H / 2) * (W / 2);
    const BlockWs ws = block_ws(M, M, 28, 16, 16, 3, workspace);
    if (ws_bytes < ws.total) return FEAR_TRAIN_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipStream_t sw = wgrad_stream ? static_cast<hipStream_t>(wgrad_stream) : s;
    if (sw != s && !stream_follow(s, sw)) return FEAR_TRAIN_ERR_HIP;      // (the coefficient vectors live in the shared workspace, as in fear_pwbn_train_backward)
    if (!bn_backward_sums(dy, 16, raw, 16, vec, 1, gamma, dgamma, dbeta, ws.coef, M, 16, ws.col, s)) return FEAR_TRAIN_ERR_SYNC;
    BnbIn bn{};
    bn.E = raw; bn.coef = ws.coef; bn.lde = 16; bn.C = 16; bn.mask_a = vec + 2 * 16; bn.mask_b = vec + 3 * 16;
    if (sw != s && !stream_follow(sw, s)) return FEAR_TRAIN_ERR_HIP;
    const StemIn st{x_nchw, H, W};
    // (no x: the weight gradient gathers its rows from the image — the pitch 28 is that of the rows it forms)
    const int rc = wgrad_impl({.dy = dy, .lddy = 16, .ldx = 28, .dw = dw, .workspace = ws.wg, .ws_bytes = ws.wg_bytes, .M = M, .K = 28, .N = 16, .s = sw,
                               .bn = &bn, .stem = &st});
    if (rc != FEAR_TRAIN_OK) return rc;
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

}  // extern "C"
