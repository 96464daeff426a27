// fear_train_optim.h — the optimiser family on gfx950: gradient-norm clipping and the SGD / Adam / AdamW
// updates of torch.optim on one flat buffer (the reference's config/optimizer/{adam,adamw,sgd}.yaml and `gradient_clip_val`,
// model_training/train/trainer.py:59).  A clipped step is three launches and no host synchronisation:
//   grad_sumsq_kernel          one workgroup per FEAR_GRAD_SUMSQ_CHUNK floats: squares added in float64, one partial each
//   grad_norm_finalize_kernel  one workgroup: the partials in a fixed order -> norm, coef = min(1, max_norm / (norm + 1e-6))
//   optim_kernel<KIND>         g = grad * coef in registers, then the rule, four elements per lane
// The update does NOT write the gradient buffer: torch.nn.utils.clip_grad_norm_ scales the gradients in place, here the scaled
// gradient lives in a register only (5.5 MB of write-back saved on the whole network) — a caller that reads its gradients after
// the step sees them unclipped.
// Summation order (fixed by n and the base address alone, never by scheduling; no floating-point atomics): lane t of a workgroup
// adds the 16-byte groups t, t + 256, ... of its chunk in that order, then its head / tail scalar; the 64 lanes of a wave meet in
// an xor butterfly (32, 16, ... 1), the four waves as (w0 + w1) + (w2 + w3).  The square of a float is exact in float64.
// Included by fear_train.hip after the training operators.

namespace {

using namespace fear;

constexpr long SUMSQ_CHUNK = FEAR_GRAD_SUMSQ_CHUNK;

// (every lane returns the same value: a + b == b + a at every level of the butterfly)
__device__ __forceinline__ double optim_block_sum(double v, double* s_wave) {
#pragma clang fp contract(off)
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

__device__ __forceinline__ double optim_sq(float x) { return (double)x * (double)x; }

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ grad, long n, double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double s_wave[4];
    const long lo = (long)blockIdx.x * SUMSQ_CHUNK;
    const int len = (int)(n - lo < SUMSQ_CHUNK ? n - lo : SUMSQ_CHUNK);
    const float* p = grad + lo;
    // the chunk is a multiple of four floats: every workgroup sees the same distance to the next 16-byte boundary
    int head = (int)((4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3);
    if (head > len) head = len;
    const int nv = (len - head) >> 2;
    const f32x4* pv = reinterpret_cast<const f32x4*>(p + head);
    double acc = 0.0;
#pragma unroll 4
    for (int i = threadIdx.x; i < nv; i += 256) {
        const f32x4 x = pv[i];
        acc = acc + optim_sq(x.x);
        acc = acc + optim_sq(x.y);
        acc = acc + optim_sq(x.z);
        acc = acc + optim_sq(x.w);
    }
    if ((int)threadIdx.x < head) acc = acc + optim_sq(p[threadIdx.x]);
    const int t = head + nv * 4 + (int)threadIdx.x;
    if (t < len) acc = acc + optim_sq(p[t]);
    const double total = optim_block_sum(acc, s_wave);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const double* __restrict__ partials, long count, int clip, float max_norm,
                                                                 float* __restrict__ out2) {
#pragma clang fp contract(off)
    __shared__ double s_wave[4];
    double acc = 0.0;
    for (long i = threadIdx.x; i < count; i += 256) acc = acc + partials[i];
    const double total = optim_block_sum(acc, s_wave);
    if (threadIdx.x != 0) return;
    const float norm = (float)sqrt(total);
    float coef = 1.f;
    if (clip) {                                       // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1.0) in fp32; a NaN stays a NaN
        const float c = (1.f / (norm + 1e-6f)) * max_norm;      // torch's scalar / tensor is tensor.reciprocal() * scalar: two roundings
        const unsigned u = __float_as_uint(c);        // c >= 0 or NaN: compared as bits, so that a NaN is kept whatever the
        coef = (u > 0x3f800000u && u <= 0x7f800000u) ? 1.f : c;      // compiler may assume about NaNs (the library's build flags)
    }
    out2[0] = norm;
    out2[1] = coef;
}

struct OptimArgs {
    float* p;
    const float* g;
    float* s1;                  // exp_avg | momentum buffer
    float* s2;                  // exp_avg_sq
    const float* coef;          // device scalar, or null
    long n, nvec;               // nvec 16-byte groups, then n - 4 nvec scalar elements
    int nesterov, first, has_buf;
    // Adam / AdamW: the scalars of AdamArgs, computed in double on the host like torch's Python scalars
    float lr_over_bc1, beta1, beta2, eps, weight_decay, bc2_sqrt, one_minus_beta1, one_minus_beta2;
    float decay;                // AdamW: 1 - lr * weight_decay
    float lr, momentum, one_minus_dampening;      // SGD
};

// One element, torch's order of fp32 operations (torch/optim/{adam,adamw,sgd}.py, the single-tensor forms).  Contraction is off
// and every fused multiply-add is written out: left to the compiler, the four-wide body and the scalar tail group their
// multiplies and adds differently (packed instructions), and neither need group them as adam_kernel's one element per lane
// does.  The Adam branch spells the operations adam_kernel compiles to — fma(wd, p, g); m + (g - m) * (1 - beta1) in two
// roundings; fma((1 - beta2) g, g, beta2 v); fma(-step_size, m / denom, p) — so that with clip_coef null it gives
// fear_adam_step's bits (tests/test_optim_family_gpu.py holds the two together).
template <int KIND>
__device__ __forceinline__ void optim_update(const OptimArgs& a, bool clip, float c, float& p_io, float g, float& s1, float& s2) {
#pragma clang fp contract(off)
    float p = p_io;
    if (clip) g = g * c;                              // grad.mul_(clip_coef): rounded on its own, as the in-place product is
    if (KIND == FEAR_OPT_SGD) {
        if (a.weight_decay != 0.f) g = __builtin_fmaf(a.weight_decay, p, g);
        if (a.has_buf) {
            const float buf = a.first ? g : __builtin_fmaf(a.one_minus_dampening, g, s1 * a.momentum);      // buf.mul_(momentum).add_(grad, alpha=1 - dampening)
            s1 = buf;
            g = a.nesterov ? __builtin_fmaf(a.momentum, buf, g) : buf;
        }
        p_io = __builtin_fmaf(-a.lr, g, p);
        return;
    }
    if (KIND == FEAR_OPT_ADAMW) p = p * a.decay;      // param.mul_(1 - lr * weight_decay)
    else if (a.weight_decay != 0.f) g = __builtin_fmaf(a.weight_decay, p, g);
    const float m = s1 + (g - s1) * a.one_minus_beta1;                                // exp_avg.lerp_(grad, 1 - beta1)
    const float v = __builtin_fmaf(a.one_minus_beta2 * g, g, s2 * a.beta2);           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    s1 = m;
    s2 = v;
    p_io = __builtin_fmaf(-a.lr_over_bc1, m / denom, p);
}

template <int KIND>
__global__ __launch_bounds__(256) void optim_kernel(OptimArgs a) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool clip = a.coef != nullptr;
    const float c = clip ? a.coef[0] : 1.f;
    const bool use1 = KIND != FEAR_OPT_SGD || a.has_buf;
    if (i < a.nvec) {
        f32x4 p = reinterpret_cast<f32x4*>(a.p)[i];
        const f32x4 g = reinterpret_cast<const f32x4*>(a.g)[i];
        f32x4 s1 = (f32x4){0.f, 0.f, 0.f, 0.f}, s2 = s1;
        if (use1) s1 = reinterpret_cast<f32x4*>(a.s1)[i];
        if (KIND != FEAR_OPT_SGD) s2 = reinterpret_cast<f32x4*>(a.s2)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = p[j], s1j = s1[j], s2j = s2[j];
            optim_update<KIND>(a, clip, c, pj, g[j], s1j, s2j);
            p[j] = pj; s1[j] = s1j; s2[j] = s2j;
        }
        reinterpret_cast<f32x4*>(a.p)[i] = p;
        if (use1) reinterpret_cast<f32x4*>(a.s1)[i] = s1;
        if (KIND != FEAR_OPT_SGD) reinterpret_cast<f32x4*>(a.s2)[i] = s2;
        return;
    }
    const long e = a.nvec * 4 + (i - a.nvec);         // the scalar tail: n % 4 elements, or all of them behind an unaligned base
    if (e >= a.n) return;
    float p = a.p[e], s1 = use1 ? a.s1[e] : 0.f, s2 = KIND != FEAR_OPT_SGD ? a.s2[e] : 0.f;
    optim_update<KIND>(a, clip, c, p, a.g[e], s1, s2);
    a.p[e] = p;
    if (use1) a.s1[e] = s1;
    if (KIND != FEAR_OPT_SGD) a.s2[e] = s2;
}

inline bool optim_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

long fear_grad_sumsq_partials(long n) { return n <= 0 ? 0 : (n + SUMSQ_CHUNK - 1) / SUMSQ_CHUNK; }

int fear_grad_sumsq(const float* grad, long n, double* partials, void* stream) {
    if (n == 0) return FEAR_TRAIN_OK;
    if (!grad || !partials) return FEAR_TRAIN_ERR_NULL;
    const long blocks = fear_grad_sumsq_partials(n);
    if (n < 0 || blocks > 0x7fffffffL || (reinterpret_cast<uintptr_t>(grad) & 3)) return FEAR_TRAIN_ERR_SHAPE;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), grad, n, partials);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_grad_norm_finalize(const double* partials, long count, double max_norm, float* out2, void* stream) {
    if (!out2 || (count > 0 && !partials)) return FEAR_TRAIN_ERR_NULL;
    if (count < 0) return FEAR_TRAIN_ERR_SHAPE;
    hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), partials, count,
                       max_norm > 0.0 ? 1 : 0, (float)max_norm, out2);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_optim_step(const FearOptim* o, float* param, const float* grad, float* state1, float* state2, long n, int step,
                    const float* clip_coef, void* stream) {
    if (!o) return FEAR_TRAIN_ERR_NULL;
    const int kind = o->kind;
    if (kind != FEAR_OPT_ADAM && kind != FEAR_OPT_ADAMW && kind != FEAR_OPT_SGD) return FEAR_TRAIN_ERR_SHAPE;
    if (n < 0 || step < 1) return FEAR_TRAIN_ERR_SHAPE;
    const bool sgd = kind == FEAR_OPT_SGD;
    if (sgd) {
        if (!(o->momentum >= 0.0)) return FEAR_TRAIN_ERR_SHAPE;
        if (o->nesterov && (o->momentum <= 0.0 || o->dampening != 0.0)) return FEAR_TRAIN_ERR_SHAPE;      // torch's rule
    } else if (!(o->beta1 >= 0.0 && o->beta1 < 1.0) || !(o->beta2 >= 0.0 && o->beta2 < 1.0)) {
        return FEAR_TRAIN_ERR_SHAPE;
    }
    const bool has_buf = sgd && o->momentum != 0.0;
    if (!param || !grad || (!sgd && (!state1 || !state2)) || (has_buf && !state1)) return FEAR_TRAIN_ERR_NULL;
    if (n == 0) return FEAR_TRAIN_OK;
    OptimArgs a{};
    a.p = param; a.g = grad; a.s1 = (sgd && !has_buf) ? nullptr : state1; a.s2 = sgd ? nullptr : state2; a.coef = clip_coef; a.n = n;
    const bool vec = optim_aligned16(param) && optim_aligned16(grad) && optim_aligned16(a.s1) && optim_aligned16(a.s2);
    a.nvec = vec ? n / 4 : 0;
    a.nesterov = o->nesterov != 0; a.first = step == 1; a.has_buf = has_buf;
    a.weight_decay = (float)o->weight_decay;
    if (sgd) {
        a.lr = (float)o->lr; a.momentum = (float)o->momentum; a.one_minus_dampening = (float)(1.0 - o->dampening);
    } else {
        a.beta1 = (float)o->beta1; a.beta2 = (float)o->beta2; a.eps = (float)o->eps;
        a.one_minus_beta1 = (float)(1.0 - o->beta1); a.one_minus_beta2 = (float)(1.0 - o->beta2);
        a.lr_over_bc1 = (float)(o->lr / (1.0 - pow(o->beta1, step)));           // step_size = lr / bias_correction1
        a.bc2_sqrt = (float)sqrt(1.0 - pow(o->beta2, step));
        a.decay = (float)(1.0 - o->lr * o->weight_decay);
    }
    const long threads = a.nvec + (n - 4 * a.nvec);
    const long blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffL) return FEAR_TRAIN_ERR_SHAPE;
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (kind == FEAR_OPT_ADAM) hipLaunchKernelGGL(optim_kernel<FEAR_OPT_ADAM>, grid, block, 0, st, a);
    else if (kind == FEAR_OPT_ADAMW) hipLaunchKernelGGL(optim_kernel<FEAR_OPT_ADAMW>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(optim_kernel<FEAR_OPT_SGD>, grid, block, 0, st, a);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

}  // extern "C"
