// fear_train_block_kernels.h — device code of the block-fused training operators (fear_train_block.h: the recipe, and the host code
// that sequences these kernels; it includes this file).

namespace {

// ------------------------------------------------------------------------------------------------
// Y[m][n] = sum_k X'[m][k] Wt[k][n]  with  X' = BnbIn(X) formed on load and Wt K-major ([Kred][Nout] row-major: the [N][K] matrix
// of the convolution whose INPUT gradient this is).  pw_stat_kernel's tiling (4 waves x 32 rows per workgroup, NT column tiles
// per pass, passes dealt over gridDim.y).  MS = false: + R, store.  MS = true: Y is masked where fma(D, a, b) <= 0 (the ReLU of
// the layer whose raw output D is), stored, and its column sums sum(y) / sum(y * dhat), dhat = (D - mean) * rstd, leave in the
// pass (the next BatchNorm-backward's two reductions): fp32 over a wave's 32 rows, float64 across waves and workgroups.
struct PwBwdArgs {
    const float* G;
    BnbIn bn;
    const float* X2;     // optional: the reduction's rows K1 ... Kred - 1 come from this second tensor [M][ldx2], as loaded (see BnbIn)
    const float* W;      // [Kred][Nout]
    const float* R;      // optional [M][ldr] added to Y (MS = false)
    float* Y;
    const float* D;      // MS: [M][ldd] raw tensor behind the ReLU
    const float* dvec;   // MS: [4][Nout] mean | rstd | a | b of D's BatchNorm
    double* partial;     // MS: [gridDim.x][2][Nout]
    int ldg, ldx2, ldr, ldy, ldd;
    int M, Kred, Nout;
    int K1;              // with X2: a multiple of 16
    int row_tiles;       // 128-row tiles per workgroup (0 = 1)
    float* p3;           // W3G: per-workgroup partials [gridDim.x][Kred][Nout] of the projection's weight gradient, see pw_bwd_kernel
};

// W3G (with MS, NT = all column tiles, Kred and Nout of the same tile count — the blocks without an expansion, 16 / 24 channels on the
// 128 x 128 / 64 x 64 maps): the projection's weight gradient dW3[k][n] = sum_m bnb(G)[m][k] act(D)[m][n] is summed here as well — both
// operands pass through this kernel anyway, a separate weight-gradient launch read three 134 MB tensors again for a 16 x 16 result.
// Lane (k or n index li, row lk) re-reads its elements (L1 hits); one MFMA per four rows and tile; one partial per workgroup.
template <int NT, bool MS, bool W3G = false>
__global__ __launch_bounds__(256) void pw_bwd_kernel(PwBwdArgs a) {
    constexpr int MT = 2;
    static_assert(!W3G || (MS && NT <= 2), "the in-kernel weight gradient: the narrow blocks' masked-gradient pass");
    __shared__ double red[MS ? 4 : 1][2][NT * 16];
    __shared__ f32x4 red3[W3G ? 3 * 64 : 1];
    f32x4 acc3[W3G ? NT : 1][W3G ? NT : 1];
#pragma unroll
    for (int kt = 0; kt < (W3G ? NT : 1); ++kt)
#pragma unroll
        for (int nt = 0; nt < (W3G ? NT : 1); ++nt) acc3[kt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int row_tiles = a.row_tiles > 0 ? a.row_tiles : 1;
    const bool bnb = a.bn.coef != nullptr, bne = a.bn.E != nullptr, bmask = bne && a.bn.mask_a != nullptr;
    const bool two = a.X2 != nullptr;
    const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int n_tiles = (a.Nout + 15) >> 4;
    for (int nc = blockIdx.y * NT; nc < n_tiles; nc += NT * gridDim.y) {
        int ncol[NT];
        bool nvalid[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n = (nc + nt) * 16 + li;
            nvalid[nt] = n < a.Nout;
            ncol[nt] = nvalid[nt] ? n : (a.Nout - 1);
        }
        if (MS && li == 0) {      // float64 column sums of this workgroup's rows (pw_stat_kernel's scheme)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int c = 0; c < 4; ++c) { red[wave][0][nt * 16 + lk * 4 + c] = 0.0; red[wave][1][nt * 16 + lk * 4 + c] = 0.0; }
        }
        for (int rt = 0; rt < row_tiles; ++rt) {
            const int m_wave = ((blockIdx.x * row_tiles + rt) * 4 + wave) * (MT * 16);
            if (m_wave >= a.M) break;      // (wave-uniform; no barrier inside this loop)
            const float* grow[MT];
            const float* erow[MT];
            const float* x2row[MT];
            bool mvalid[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                int m = m_wave + mt * 16 + li;
                mvalid[mt] = m < a.M;
                if (m >= a.M) m = a.M - 1;
                grow[mt] = a.G + (long)m * a.ldg;
                erow[mt] = bne ? a.bn.E + (long)m * a.bn.lde : nullptr;
                x2row[mt] = two ? a.X2 + (long)m * a.ldx2 : nullptr;
            }
            f32x4 acc[MT][NT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = zero;
            for (int kg = 0; kg < a.Kred; kg += 16) {
                const int k = kg + lk * 4;
                const bool kvalid = k < a.Kred;      // Kred is a multiple of 4
                f32x4 xf[MT], wf[NT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) xf[mt] = zero;
                if (kvalid && two && kg >= a.K1) {          // (K1 is a multiple of 16: uniform over the wave)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) xf[mt] = *reinterpret_cast<const f32x4*>(x2row[mt] + (k - a.K1));
                } else if (kvalid) {
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) xf[mt] = *reinterpret_cast<const f32x4*>(grow[mt] + k);
                    if (bnb) {
                        f32x4 ev[MT];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) ev[mt] = bne ? *reinterpret_cast<const f32x4*>(erow[mt] + k) : zero;
                        const f32x4 cA = *reinterpret_cast<const f32x4*>(a.bn.coef + k), cs1 = *reinterpret_cast<const f32x4*>(a.bn.coef + a.bn.C + k);
                        const f32x4 cmu = *reinterpret_cast<const f32x4*>(a.bn.coef + 2 * a.bn.C + k), cQ = *reinterpret_cast<const f32x4*>(a.bn.coef + 3 * a.bn.C + k);
                        if (bmask) {
                            const f32x4 cma = *reinterpret_cast<const f32x4*>(a.bn.mask_a + k), cmb = *reinterpret_cast<const f32x4*>(a.bn.mask_b + k);
#pragma unroll
                            for (int mt = 0; mt < MT; ++mt) xf[mt] = relu_mask4(xf[mt], ev[mt], cma, cmb);
                        }
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) xf[mt] = bnb4(xf[mt], ev[mt], cA, cs1, cmu, cQ);
                    }
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    wf[nt] = zero;
                    if (kvalid && nvalid[nt]) {
                        const float* p = a.W + (long)k * a.Nout + ncol[nt];
                        wf[nt] = (f32x4){p[0], p[a.Nout], p[2 * a.Nout], p[3 * a.Nout]};
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[nt][i], xf[mt][i], acc[mt][nt], 0, 0, 0);
            }
            // epilogue: lane holds columns n0 + 4 lk + {0..3} of rows m_wave + mt * 16 + li
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int n = (nc + nt) * 16 + lk * 4;
                const bool nok = n < a.Nout;      // Nout is a multiple of 4
                if (MS) {
                    f32x4 dmu = zero, drs = zero, da = zero, db = zero;
                    if (nok) {
                        dmu = *reinterpret_cast<const f32x4*>(a.dvec + n); drs = *reinterpret_cast<const f32x4*>(a.dvec + a.Nout + n);
                        da = *reinterpret_cast<const f32x4*>(a.dvec + 2 * a.Nout + n); db = *reinterpret_cast<const f32x4*>(a.dvec + 3 * a.Nout + n);
                    }
                    f32x4 s1 = zero, s2 = zero;
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        if (!mvalid[mt] || !nok) continue;
                        const long m = m_wave + mt * 16 + li;
                        const f32x4 dv = *reinterpret_cast<const f32x4*>(a.D + m * a.ldd + n);
                        const f32x4 v = relu_mask4(acc[mt][nt], dv, da, db);
                        *reinterpret_cast<f32x4*>(a.Y + m * a.ldy + n) = v;
                        s1 += v;
                        s2 += v * ((dv - dmu) * drs);
                    }
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float t1 = row16_sum(s1[c]), t2 = row16_sum(s2[c]);
                        if (li == 0) {
                            red[wave][0][nt * 16 + lk * 4 + c] += (double)t1;
                            red[wave][1][nt * 16 + lk * 4 + c] += (double)t2;
                        }
                    }
                } else {
                    if (!nok) continue;
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        if (!mvalid[mt]) continue;
                        const long m = m_wave + mt * 16 + li;
                        f32x4 v = acc[mt][nt];
                        if (a.R) v += *reinterpret_cast<const f32x4*>(a.R + m * a.ldr + n);
                        *reinterpret_cast<f32x4*>(a.Y + m * a.ldy + n) = v;
                    }
                }
            }
            if constexpr (W3G) {
                // (nc == 0: one pass over all column tiles)  this wave's 32 rows in groups of four
                float cA[NT], cs[NT], cm[NT], cq[NT], da1[NT], db1[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int k = t * 16 + li;
                    const bool kv = k < a.Kred, nv = k < a.Nout;
                    cA[t] = kv ? a.bn.coef[k] : 0.f; cs[t] = kv ? a.bn.coef[a.bn.C + k] : 0.f;
                    cm[t] = kv ? a.bn.coef[2 * a.bn.C + k] : 0.f; cq[t] = kv ? a.bn.coef[3 * a.bn.C + k] : 0.f;
                    da1[t] = nv ? a.dvec[2 * a.Nout + k] : 0.f; db1[t] = nv ? a.dvec[3 * a.Nout + k] : 0.f;
                }
#pragma unroll 2
                for (int g = 0; g < MT * 4; ++g) {
                    const long m = (long)m_wave + g * 4 + lk;
                    const bool mv = m < a.M;
                    float av[NT], bv[NT];
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const int k = t * 16 + li;
                        av[t] = 0.f; bv[t] = 0.f;
                        if (mv && k < a.Kred) av[t] = cA[t] * (a.G[m * a.ldg + k] - cs[t] - (a.bn.E[m * a.bn.lde + k] - cm[t]) * cq[t]);
                        if (mv && k < a.Nout) bv[t] = fmaxf(__builtin_fmaf(a.D[m * a.ldd + k], da1[t], db1[t]), 0.f);
                    }
#pragma unroll
                    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) acc3[kt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kt], bv[nt], acc3[kt][nt], 0, 0, 0);
                }
            }
        }
        if (MS) {
            __syncthreads();
            for (int i = threadIdx.x; i < 2 * NT * 16; i += 256) {
                const int which = i / (NT * 16), col = i % (NT * 16);
                const int n = nc * 16 + col;
                if (n < a.Nout)
                    a.partial[((long)blockIdx.x * 2 + which) * a.Nout + n] =
                        ((red[0][which][col] + red[1][which][col]) + red[2][which][col]) + red[3][which][col];      // fixed order
            }
            __syncthreads();
        }
    }
    if constexpr (W3G) {      // the four waves' shares in wave order, one partial [Kred][Nout] per workgroup
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                __syncthreads();
                if (wave > 0) red3[(wave - 1) * 64 + lane] = acc3[kt][nt];
                __syncthreads();
                if (wave == 0) {
                    f32x4 v = acc3[kt][nt];
#pragma unroll
                    for (int w = 0; w < 3; ++w) v += red3[w * 64 + lane];
                    const int n = nt * 16 + li;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int k = kt * 16 + 4 * lk + r;      // lane (n, q), component r = row 4 q + r of the tile
                        if (k < a.Kred && n < a.Nout) a.p3[((long)blockIdx.x * a.Kred + k) * a.Nout + n] = v[r];
                    }
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------
// The VIRTUAL expansion of a 16 ... 32-channel block input (FEAR_IRB_VIRTUAL_E; the 16 -> 96 expansion of the 128 x 128 map is 0.8 GB per
// 128 crops, written once and read three times): e = x W1^T is never stored.  Its two remaining consumers — the depthwise kernels;
// the expansion's own backward reads g1 and x, see BnbIn — form their tile of it on the matrix pipe as the tile is staged: per 16
// pixels and 16 input channels one 16-byte load per lane (lane (pixel j, k quarter kk) holds x[j][4 kk ..]) and four MFMAs per 16
// channels against the W1 fragments a lane keeps (lane (channel i, kk): W1[i][4 kk ..]); the result lane (pixel j, q) is the float4 of channels 4 q ..
// 4 q + 3 of pixel j — the (pixel, channel quad) unit both kernels work in.  The SAME products in the same order in both
// directions, so the forward's activation and the backward's mask see the same numbers.
// BatchNorm1's batch statistics follow from linearity as well: sum_m e = W1 (sum_m x), sum_m e^2 = diag(W1 G W1^T), G = x^T x.
struct VirtE {
    const float* X;       // [pixels][cin] the block input
    const float* W1;      // [C][cin] the expansion's weights
    int cin;              // 16 ... 32 (a multiple of 4): NC = ceil(cin / 16) chunks of 16 reduction columns, the last one zero-padded
};

// e[16 channels][16 pixels] from the fragments above (NC chunks of 16 input channels): lane (pixel j, q) gets channels 4 q .. 4 q + 3
template <int NC>
__device__ __forceinline__ f32x4 virt_e_tile(const f32x4 (&wa)[NC], const f32x4 (&xb)[NC]) {
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ci = 0; ci < NC; ++ci)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[ci][t], xb[ci][t], acc, 0, 0, 0);
    return acc;
}

// G = x^T x [KP][KP] and s = sum_m x [KP] (KP = 16 NC >= cin, zero-padded) of a narrow tensor in one pass: lane (channel i, row kk)
// loads x[row kk][16 ci + i] — with 16 channels a wave's load is 64 consecutive floats — and that one register is the MFMA fragment of
// four rows for BOTH operands (D[i][j] += sum_kk x[kk][i] x[kk][j]); the column sums are the same product against ones.  Per
// workgroup one partial [KP * KP + KP] = G | s, summed by slice_sum_kernel in a fixed order.
template <int NC>
__global__ __launch_bounds__(256) void gram_kernel(const float* X, long M, int cin, long rows_per_wg, float* P) {
    __shared__ f32x4 red[3][NC * NC + NC][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long m0 = (long)blockIdx.x * rows_per_wg;
    const long m1 = m0 + rows_per_wg < M ? m0 + rows_per_wg : M;
    const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 g[NC][NC], sm[NC];
#pragma unroll
    for (int a_ = 0; a_ < NC; ++a_) {
        sm[a_] = zero;
#pragma unroll
        for (int b_ = 0; b_ < NC; ++b_) g[a_][b_] = zero;
    }
    constexpr int U = NC == 1 ? 8 : 4;
    const long ngroups = m1 > m0 ? (m1 - m0 + 3) / 4 : 0;      // groups of four rows, dealt to the waves U at a time
    bool cok[NC];
#pragma unroll
    for (int ci = 0; ci < NC; ++ci) cok[ci] = ci * 16 + (lane & 15) < cin;
    for (long g0 = (long)wave * U; g0 < ngroups; g0 += 4 * U) {
        float v[U][NC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long r = m0 + (g0 + u) * 4 + (lane >> 4);
            const bool rok = g0 + u < ngroups && r < m1;
#pragma unroll
            for (int ci = 0; ci < NC; ++ci) v[u][ci] = rok && cok[ci] ? X[r * cin + ci * 16 + (lane & 15)] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int a_ = 0; a_ < NC; ++a_) {
#pragma unroll
                for (int b_ = 0; b_ < NC; ++b_) g[a_][b_] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[u][a_], v[u][b_], g[a_][b_], 0, 0, 0);
                sm[a_] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[u][a_], 1.0f, sm[a_], 0, 0, 0);
            }
    }
    if (wave > 0) {
#pragma unroll
        for (int a_ = 0; a_ < NC; ++a_) {
            red[wave - 1][NC * NC + a_][lane] = sm[a_];
#pragma unroll
            for (int b_ = 0; b_ < NC; ++b_) red[wave - 1][a_ * NC + b_][lane] = g[a_][b_];
        }
    }
    __syncthreads();
    if (wave != 0) return;
    constexpr int KP = 16 * NC;
    float* out = P + (long)blockIdx.x * (KP * KP + KP);
    const int j = lane & 15, q = lane >> 4;
#pragma unroll
    for (int a_ = 0; a_ < NC; ++a_) {
#pragma unroll
        for (int w = 0; w < 3; ++w) sm[a_] += red[w][NC * NC + a_][lane];      // fixed order
#pragma unroll
        for (int b_ = 0; b_ < NC; ++b_) {
#pragma unroll
            for (int w = 0; w < 3; ++w) g[a_][b_] += red[w][a_ * NC + b_][lane];
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(a_ * 16 + 4 * q + r) * KP + b_ * 16 + j] = g[a_][b_][r];      // lane (j, q), component r
        }
        if (j == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) out[KP * KP + a_ * 16 + 4 * q + r] = sm[a_][r];
        }
    }
}

// BatchNorm1 of a virtual expansion from (G | s) [KP * KP + KP]: mean, rstd, the affine a | b and the running statistics
// (col_finalize mode 0's arithmetic on float64 sums)
template <int KP>
__global__ __launch_bounds__(256) void irb_virtual_stats_kernel(const float* GS, const float* W1, const float* gamma, const float* beta, float* vec,
                                                              float* running_mean, float* running_var, int C, int cin, double M, double eps,
                                                              double momentum) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double w[KP];                                   // (registers: every index below is a compile-time constant; G's are uniform loads)
#pragma unroll
    for (int k = 0; k < KP; ++k) w[k] = k < cin ? (double)W1[(long)c * cin + k] : 0.0;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        s1 += w[k] * (double)GS[KP * KP + k];
        double t = 0.0;
#pragma unroll
        for (int k2 = 0; k2 < KP; ++k2) t += (double)GS[k * KP + k2] * w[k2];
        s2 += w[k] * t;
    }
    const double mean = s1 / M;
    double var = s2 / M - mean * mean;
    if (var < 0.0) var = 0.0;
    const float mf = (float)mean, rf = (float)(1.0 / sqrt(var + eps));
    vec[c] = mf;
    vec[C + c] = rf;
    const float av = gamma[c] * rf;
    vec[2 * C + c] = av;
    vec[3 * C + c] = __builtin_fmaf(-mf, av, beta[c]);
    if (running_mean) {
        running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
        const double unbiased = M > 1.0 ? var * M / (M - 1.0) : var;
        running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
    }
}

// ------------------------------------------------------------------------------------------------
// Backward through  ReLU o BN2 o depthwise o ReLU o BN1  in one pass (the middle of an inverted-residual block).
//   inputs   G2 [B*Ho*Wo][C]  gradient w.r.t. the depthwise unit's activation, already masked by its ReLU (pw_bwd_kernel<MS>)
//            D  [B*Ho*Wo][C]  raw depthwise output (BN2's input);  coef2 = BN2's BnbIn coefficients
//            E  [B*H*W][C]    raw expansion (BN1's input), act1 = [mean | rstd | a | b] of BN1 — or, BN1 = false (blocks without an
//                             expansion), the block input itself, which is the depthwise conv's operand as it stands
//   outputs  Y = g1 = (DW^T dd) * [act1(e) > 0]      (BN1)      |   Y = DW^T dd [+ R]    (no BN1: the block's input gradient)
//            d taps[t][c] = sum dd[o] * act1(e)[o * S + t - P]   (per-workgroup partials, fixed-order final sum)
//            sum g1, sum g1 * ehat                               (BN1; float64 partials)
//   with dd = A2 (g2 - s1 - (d - mu2) Q2), never written to memory.
// A workgroup owns a slab of 4 SQ channels (SQ channel quads) and walks 16 x 16 tiles of the INPUT map: the tile's dd region
// ((16 + 2P)^2 output pixels at stride 1, (8 + ...)^2 at stride 2; zero outside the map = the convolution's padding) is formed
// once into LDS, then every thread — a fixed channel quad and a fixed pixel lane — gathers its taps from LDS: the input
// gradient, and the products for the tap gradients, which stay in registers across all tiles of the workgroup.  At stride 2 a
// pixel only meets the taps of its parity class (ky = (y + P) mod 2 + 2 j), so a thread keeps ONE class (its pixels are dealt
// that way) and its register slot (j, i) means tap (ky0 + 2 j, kx0 + 2 i): every register index is a compile-time constant.
struct DwBwdArgs {
    const float* G2;
    const float* D;
    const float* coef2;   // [4][C]
    const float* Wt;      // [KS*KS][C]
    const float* E;
    const float* act1;    // BN1: [4][C]
    const float* R;       // no BN1: optional [B*H*W][ldr] added to Y
    float* Y;
    float* ptaps;         // [wgs_per_slab][KS*KS][C]
    double* psums;        // BN1: [wgs_per_slab][2][C]
    int ldo, lde, ldr, ldy;
    int B, H, W, Ho, Wo, C;
    int tiles_x, tiles_y, wgs_per_slab, nslab;
    VirtE ve;             // VE: E is not read, e = ve.X ve.W1^T on the spot
    float* pw1;           // VE, optional: per-workgroup partials [wgs_per_slab][C][cin] of sum_m g1[m][c] x[m][k] — the expansion's weight
                          // gradient before its BatchNorm1 algebra (irb_lin_wgrad_fix2_kernel), formed from the tile while g1 is on chip
};

// TS: the tile side, 16 — or 8 for maps of at most 8 x 8 pixels (the template branch's stride-16 stage: a 16 x 16 tile would be three
// quarters outside the map, dd region and sweeps alike; built for the 5 x 5 stride-1 kernels that stage consists of)
// W1G (with VE): the expansion's weight gradient is accumulated here as well (DwBwdArgs::pw1; built for the 3 x 3 kernels: the 5 x 5
// ones have no registers left for its accumulators)
template <int KS, int S, int SQ, bool BN1, int VE = 0, int TS = 16, bool W1G = false>      // VE = NC chunks of 16 input channels of a virtual expansion (0: E is read)
__global__ __launch_bounds__(256, 2) void dw_bwd_kernel(DwBwdArgs a) {
    static_assert(!VE || (BN1 && S == 2), "the virtual expansion is built for the stride-2 kernels");
    static_assert(TS == 16 || (TS == 8 && S == 1 && KS == 5), "8 x 8 tiles: the 5 x 5 stride-1 kernels only");
    static_assert(!W1G || VE != 0, "the in-kernel weight gradient belongs to the virtual expansion");
    constexpr int P = KS / 2, KK = KS * KS;
    constexpr int LO = P / S;                          // output rows / columns in front of the tile's first own one
    constexpr int OR = (TS - 1 + P) / S + LO + 1;      // side of the dd region a tile reads
    constexpr int PITCH = (OR + 1) * SQ;               // float4s per region row: one pixel of padding turns consecutive rows by half
                                                       // the LDS banks, so the lanes of a ds_read_b128 group (consecutive rows) differ
    constexpr int NT = (KS + S - 1) / S;               // taps per dimension a pixel meets
    constexpr int PL = 256 / SQ;                       // pixel lanes
    constexpr bool WREG = NT * NT <= 9;                // tap weights in registers (else in LDS)
    constexpr int T = KS == 5 ? 2 : 4;                 // stride 1: a thread takes runs of T pixels along x (register window over the taps)
    // 5 x 5 stride 1: TWO lanes share a run — lane half h takes the tap rows ky = KH h ... KH h + KH - 1 (3 + 2) — so that a lane
    // carries 15 tap-gradient accumulators instead of 25 (60 registers instead of 100: 170 instead of 256 per lane, three
    // workgroups per CU instead of two at one wave per SIMD each); the halves of the input gradient meet through one shuffle
    constexpr bool HS = S == 1 && KS == 5;
    constexpr int KH = (KS + 1) / 2;
    constexpr int AJ = HS ? KH : NT;                   // accumulator rows per lane
    constexpr int NCLS = HS ? 2 : S * S;               // lane classes whose accumulator slots mean different taps (halves / parities)
    constexpr int SMEM = OR * PITCH > 512 ? OR * PITCH : 512;
    __shared__ f32x4 tile[SMEM];                        // the dd region; after the last tile, the reduction buffer
    __shared__ f32x4 wl[WREG ? 1 : KK * SQ];
    f32x4* red = tile;
    f64x4* red64 = reinterpret_cast<f64x4*>(tile);
    const int tid = threadIdx.x;
    const int cq_l = tid % SQ, pl = tid / SQ;
    const int slab = blockIdx.x % a.nslab, wslot = blockIdx.x / a.nslab;
    const int c = (slab * SQ + cq_l) * 4;
    const bool cv = c < a.C;
    const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 cA = zero, cs1 = zero, cmu = zero, cQ = zero, mu1 = zero, rs1 = zero, a1 = zero, b1 = zero;
    if (cv) {
        cA = *reinterpret_cast<const f32x4*>(a.coef2 + c); cs1 = *reinterpret_cast<const f32x4*>(a.coef2 + a.C + c);
        cmu = *reinterpret_cast<const f32x4*>(a.coef2 + 2 * a.C + c); cQ = *reinterpret_cast<const f32x4*>(a.coef2 + 3 * a.C + c);
        if (BN1) {
            mu1 = *reinterpret_cast<const f32x4*>(a.act1 + c); rs1 = *reinterpret_cast<const f32x4*>(a.act1 + a.C + c);
            a1 = *reinterpret_cast<const f32x4*>(a.act1 + 2 * a.C + c); b1 = *reinterpret_cast<const f32x4*>(a.act1 + 3 * a.C + c);
        }
    }
    // VE: the tile's raw expansion [256 pixels][SQ quads], formed on the matrix pipe while the dd region is staged
    __shared__ f32x4 es[VE ? TS * TS * SQ : 1];
    f32x4 wa[VE ? SQ / 4 : 1][VE ? VE : 1];
    if (VE) {
#pragma unroll
        for (int ct = 0; ct < SQ / 4; ++ct)
#pragma unroll
            for (int ci = 0; ci < VE; ++ci) {
                const int ch = slab * SQ * 4 + ct * 16 + (tid & 15), k = ci * 16 + 4 * ((tid & 63) >> 4);
                wa[VE ? ct : 0][VE ? ci : 0] = ch < a.C && k < a.ve.cin ? *reinterpret_cast<const f32x4*>(a.ve.W1 + (long)ch * a.ve.cin + k) : zero;
            }
    }
    f32x4 acc1[W1G ? SQ / 4 : 1][W1G ? VE : 1];
#pragma unroll
    for (int ct = 0; ct < (W1G ? SQ / 4 : 1); ++ct)
#pragma unroll
        for (int ci = 0; ci < (W1G ? VE : 1); ++ci) acc1[ct][ci] = zero;
    // this thread's parity class and the first tap it meets in each dimension
    const int cls = S == 1 ? 0 : (pl & 3);
    const int py = S == 1 ? 0 : (cls >> 1), px = S == 1 ? 0 : (cls & 1);
    const int ky0 = (py + P) % S, kx0 = (px + P) % S;
    f32x4 wreg[WREG ? NT : 1][WREG ? NT : 1];
    if (WREG) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int ky = ky0 + S * j, kx = kx0 + S * i;
                wreg[WREG ? j : 0][WREG ? i : 0] = (cv && ky < KS && kx < KS) ? *reinterpret_cast<const f32x4*>(a.Wt + (long)(ky * KS + kx) * a.C + c) : zero;
            }
    } else {
        for (int t = pl; t < KK; t += PL) wl[t * SQ + cq_l] = cv ? *reinterpret_cast<const f32x4*>(a.Wt + (long)t * a.C + c) : zero;
    }
    f32x4 acc[AJ][NT];
#pragma unroll
    for (int j = 0; j < AJ; ++j)
#pragma unroll
        for (int i = 0; i < NT; ++i) acc[j][i] = zero;
    f64x4 S1 = (f64x4){0.0, 0.0, 0.0, 0.0}, S2 = S1;

    const long obytes = (long)a.B * a.Ho * a.Wo * a.ldo * 4;      // < 2^31: checked on the host
    const __amdgpu_buffer_rsrc_t g2r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.G2), 0, (int)obytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.D), 0, (int)obytes, 0x00020000);
    const int n_items = a.B * a.tiles_y * a.tiles_x;
    for (int item = wslot; item < n_items; item += a.wgs_per_slab) {
        const int tx = item % a.tiles_x, ty = (item / a.tiles_x) % a.tiles_y, b = item / (a.tiles_x * a.tiles_y);
        const int iy0 = ty * TS, ix0 = tx * TS;
        const int lo_y = iy0 / S - LO, lo_x = ix0 / S - LO;
        f32x4 s1f = zero, s2f = zero;      // this tile's share of the two sums (at most 16 values per lane), then float64
        int wq = cq_l;                      // index of this thread's weights in LDS, opaque to the compiler: it would otherwise hoist
        asm volatile("" : "+v"(wq));        // all 25 LDS weight reads out of the tile loop into 100 registers
        // ---- phase 1: dd of the tile's output region -> LDS (zero outside the map / beyond the channels)
        // (U loads of each tensor in flight per round: the region is 12.5 float4 per thread and tensor for a 5 x 5 stride-1 tile
        //  with 32-channel slabs — at U = 4 that was four memory round trips per tile on a kernel whose tiles are short)
        constexpr int NIDX = OR * OR * SQ, U = (!HS && (NIDX + 255) / 256 > 8) ? 7 : 4;
        for (int i0 = 0; i0 < NIDX; i0 += 256 * U) {
            f32x4 gv[U], dv[U];
            bool in[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = i0 + u * 256 + tid;
                const int pix = idx / SQ;                 // idx % SQ == cq_l (256 is a multiple of SQ)
                const int r = pix / OR, cc = pix - r * OR;
                const int oy = lo_y + r, ox = lo_x + cc;
                in[u] = idx < NIDX && cv && oy >= 0 && oy < a.Ho && ox >= 0 && ox < a.Wo;
                const int off = in[u] ? (((b * a.Ho + oy) * a.Wo + ox) * a.ldo + c) * 4 : (int)0x80000000;
                gv[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(g2r, off, 0, 0));
                dv[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dr, off, 0, 0));
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = i0 + u * 256 + tid;
                const int pix = idx / SQ;
                const int r = pix / OR, cc = pix - r * OR;
                if (idx < NIDX) tile[r * PITCH + cc * SQ + cq_l] = in[u] ? bnb4(gv[u], dv[u], cA, cs1, cmu, cQ) : zero;
            }
        }
        if constexpr (VE) {
            const int wave = tid >> 6, j = tid & 15, kk = (tid & 63) >> 4;
#pragma unroll 1
            for (int rt = wave; rt < TS * TS / 16; rt += 4) {
                const int p = rt * 16 + j;                       // tile pixel of this lane's column
                const int iy = iy0 + p / TS, ix = ix0 + p % TS;
                const bool inb = iy < a.H && ix < a.W;
                f32x4 xb[VE ? VE : 1];
#pragma unroll
                for (int ci = 0; ci < VE; ++ci)
                    xb[ci] = inb && ci * 16 + 4 * kk < a.ve.cin
                                 ? *reinterpret_cast<const f32x4*>(a.ve.X + (((long)b * a.H + iy) * a.W + ix) * a.ve.cin + ci * 16 + 4 * kk) : zero;
#pragma unroll
                for (int ct = 0; ct < SQ / 4; ++ct) es[p * SQ + ct * 4 + kk] = virt_e_tile<VE ? VE : 1>(wa[ct], xb);
            }
        }
        __syncthreads();
        // ---- phase 2
        if (HS) {
            const int half = pl & 1, prl = pl >> 1;
            constexpr int RPS = (PL / 2) / (TS / T);       // rows per sweep
#pragma unroll 1
            for (int sw = 0; sw < TS / RPS; ++sw) {
                const int iy_l = sw * RPS + prl % RPS, ix_l = (prl / RPS) * T;
                const int iy = iy0 + iy_l;
                const long prow = ((long)b * a.H + iy) * a.W + ix0 + ix_l;
                bool pin[T];
                f32x4 e4[T], av[T], de[T];
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    pin[i] = cv && iy < a.H && ix0 + ix_l + i < a.W;
                    e4[i] = pin[i] ? *reinterpret_cast<const f32x4*>(a.E + (prow + i) * a.lde + c) : zero;
                }
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    av[i] = e4[i];
                    if (BN1) {
                        const f32x4 pre = act4(e4[i], a1, b1, false);
                        av[i] = (f32x4){fmaxf(pre.x, 0.f), fmaxf(pre.y, 0.f), fmaxf(pre.z, 0.f), fmaxf(pre.w, 0.f)};
                    }
                    if (!pin[i]) av[i] = zero;
                    de[i] = zero;
                }
                const int ky_first = half * KH;
                int lb = (iy_l + 2 * P - ky_first) * PITCH + ix_l * SQ + cq_l;
#pragma unroll
                for (int jj = 0; jj < KH; ++jj) {
                    const bool kyv = ky_first + jj < KS;           // (the second half's last row does not exist)
                    const int base = kyv ? lb - jj * PITCH : lb;
                    f32x4 win[T + KS - 1];
#pragma unroll
                    for (int j = 0; j < T + KS - 1; ++j) {
                        win[j] = tile[base + j * SQ];
                        if (!kyv) win[j] = zero;
                    }
                    const int wrow = (kyv ? ky_first + jj : 0) * KS;
#pragma unroll
                    for (int kx = 0; kx < KS; ++kx) {
                        const f32x4 w = wl[(wrow + kx) * SQ + wq];
#pragma unroll
                        for (int i = 0; i < T; ++i) {
                            const f32x4 v = win[i + KS - 1 - kx];
                            de[i] += v * w;
                            acc[jj][kx] += v * av[i];
                        }
                    }
                    asm volatile("" : "+v"(lb), "+v"(wq) : "v"(de[0]), "v"(de[T - 1]), "v"(acc[jj][0]), "v"(acc[jj][1]), "v"(acc[jj][2]), "v"(acc[jj][KS - 2]), "v"(acc[jj][KS - 1]));
                }
#pragma unroll
                for (int i = 0; i < T; ++i) {                      // the other half's tap rows (its lane is SQ lanes away)
                    de[i].x += __shfl_xor(de[i].x, SQ, 64); de[i].y += __shfl_xor(de[i].y, SQ, 64);
                    de[i].z += __shfl_xor(de[i].z, SQ, 64); de[i].w += __shfl_xor(de[i].w, SQ, 64);
                }
                if (half == 0) {
#pragma unroll
                    for (int i = 0; i < T; ++i) {
                        if (!pin[i]) continue;
                        if (BN1) {
                            const f32x4 pre = act4(e4[i], a1, b1, false);
                            const f32x4 g1 = (f32x4){pre.x > 0.f ? de[i].x : 0.f, pre.y > 0.f ? de[i].y : 0.f, pre.z > 0.f ? de[i].z : 0.f, pre.w > 0.f ? de[i].w : 0.f};
                            *reinterpret_cast<f32x4*>(a.Y + (prow + i) * a.ldy + c) = g1;
                            s1f += g1;
                            s2f += g1 * ((e4[i] - mu1) * rs1);
                        } else {
                            f32x4 r4 = zero;
                            if (a.R) r4 = *reinterpret_cast<const f32x4*>(a.R + (prow + i) * a.ldr + c);
                            *reinterpret_cast<f32x4*>(a.Y + (prow + i) * a.ldy + c) = de[i] + r4;
                        }
                    }
                }
            }
        } else if (S == 1) {
            // runs of T pixels along x: per tap row a window of T + KS - 1 region columns is read once and serves all T x KS
            // (pixel, tap) pairs; consecutive pixel lanes are consecutive rows
            constexpr int RPS = PL / (TS / T);             // rows per sweep
#pragma unroll 1
            for (int sw = 0; sw < TS / RPS; ++sw) {
                const int iy_l = sw * RPS + pl % RPS, ix_l = (pl / RPS) * T;
                const int iy = iy0 + iy_l;
                const long prow = ((long)b * a.H + iy) * a.W + ix0 + ix_l;
                bool pin[T];
                f32x4 e4[T], av[T], de[T];
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    pin[i] = cv && iy < a.H && ix0 + ix_l + i < a.W;
                    e4[i] = pin[i] ? *reinterpret_cast<const f32x4*>(a.E + (prow + i) * a.lde + c) : zero;
                }
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    av[i] = e4[i];
                    if (BN1) {
                        const f32x4 pre = act4(e4[i], a1, b1, false);
                        av[i] = (f32x4){fmaxf(pre.x, 0.f), fmaxf(pre.y, 0.f), fmaxf(pre.z, 0.f), fmaxf(pre.w, 0.f)};
                    }
                    if (!pin[i]) av[i] = zero;
                    de[i] = zero;
                }
                int lb = (iy_l + 2 * P) * PITCH + ix_l * SQ + cq_l;
#pragma unroll
                for (int ky = 0; ky < KS; ++ky) {
                    const int base = lb - ky * PITCH;
                    f32x4 win[T + KS - 1];
#pragma unroll
                    for (int j = 0; j < T + KS - 1; ++j) win[j] = tile[base + j * SQ];
#pragma unroll
                    for (int kx = 0; kx < KS; ++kx) {
                        const f32x4 w = WREG ? wreg[WREG ? ky : 0][WREG ? kx : 0] : wl[(ky * KS + kx) * SQ + wq];
#pragma unroll
                        for (int i = 0; i < T; ++i) {
                            const f32x4 v = win[i + KS - 1 - kx];
                            de[i] += v * w;
                            acc[HS ? 0 : ky][kx] += v * av[i];
                        }
                    }
                    // one tap row's window in flight: hipcc hoists all KS of them (100+ registers, spills at two workgroups per
                    // CU) and neither sched_barrier nor the loop structure stops it; a data dependence of the next row's address does
                    if (KS == 5) asm volatile("" : "+v"(lb), "+v"(wq) : "v"(de[0]), "v"(de[T - 1]), "v"(acc[HS ? 0 : ky][0]), "v"(acc[HS ? 0 : ky][1]), "v"(acc[HS ? 0 : ky][2]), "v"(acc[HS ? 0 : ky][KS - 2]), "v"(acc[HS ? 0 : ky][KS - 1]));
                    else asm volatile("" : "+v"(lb), "+v"(wq) : "v"(de[0]), "v"(de[1]), "v"(de[T - 2]), "v"(de[T - 1]), "v"(acc[ky][0]), "v"(acc[ky][1]), "v"(acc[ky][KS - 1]));
                }
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    if (!pin[i]) continue;
                    if (BN1) {
                        const f32x4 pre = act4(e4[i], a1, b1, false);
                        const f32x4 g1 = (f32x4){pre.x > 0.f ? de[i].x : 0.f, pre.y > 0.f ? de[i].y : 0.f, pre.z > 0.f ? de[i].z : 0.f, pre.w > 0.f ? de[i].w : 0.f};
                        *reinterpret_cast<f32x4*>(a.Y + (prow + i) * a.ldy + c) = g1;
                        s1f += g1;
                        s2f += g1 * ((e4[i] - mu1) * rs1);
                    } else {
                        f32x4 r4 = zero;
                        if (a.R) r4 = *reinterpret_cast<const f32x4*>(a.R + (prow + i) * a.ldr + c);
                        *reinterpret_cast<f32x4*>(a.Y + (prow + i) * a.ldy + c) = de[i] + r4;
                    }
                }
            }
        } else {
#pragma unroll 1
            for (int sw = 0; sw < SQ; ++sw) {
                const int id = sw * (PL / 4) + (pl >> 2);      // 2 x 2 pixel group of the tile
                const int iy_l = 2 * (id / (TS / 2)) + py, ix_l = 2 * (id % (TS / 2)) + px;
                const int iy = iy0 + iy_l, ix = ix0 + ix_l;
                const bool pin = cv && iy < a.H && ix < a.W;
                const long prow = ((long)b * a.H + iy) * a.W + ix;
                f32x4 e4 = zero, r4 = zero;
                if (pin) {
                    if constexpr (VE) {
                        e4 = es[(iy_l * TS + ix_l) * SQ + cq_l];
                    } else {
                        e4 = *reinterpret_cast<const f32x4*>(a.E + prow * a.lde + c);
                    }
                    if (!BN1 && a.R) r4 = *reinterpret_cast<const f32x4*>(a.R + prow * a.ldr + c);
                }
                f32x4 av = e4;                                 // the depthwise conv's operand at this pixel
                f32x4 pre = zero;
                if (BN1) {
                    pre = act4(e4, a1, b1, false);
                    av = (f32x4){fmaxf(pre.x, 0.f), fmaxf(pre.y, 0.f), fmaxf(pre.z, 0.f), fmaxf(pre.w, 0.f)};
                }
                if (!pin) av = zero;
                f32x4 de = zero;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const int ky = ky0 + S * j;
                    const bool jv = ky < KS;
                    const int rr = jv ? (iy_l + P - ky) / S + LO : 0;       // (iy_l + P - ky) is a multiple of S for this thread's class
#pragma unroll
                    for (int i = 0; i < NT; ++i) {
                        const int kx = kx0 + S * i;
                        const bool tv = jv && kx < KS;
                        const int cc = tv ? (ix_l + P - kx) / S + LO : 0;
                        f32x4 v = tile[rr * PITCH + cc * SQ + cq_l];
                        if (!tv) v = zero;
                        const f32x4 w = WREG ? wreg[WREG ? j : 0][WREG ? i : 0] : wl[(tv ? ky * KS + kx : 0) * SQ + wq];
                        de += v * w;
                        acc[j][i] += v * av;
                    }
                }
                f32x4 g1 = zero;
                if (pin) {
                    if (BN1) {
                        g1 = (f32x4){pre.x > 0.f ? de.x : 0.f, pre.y > 0.f ? de.y : 0.f, pre.z > 0.f ? de.z : 0.f, pre.w > 0.f ? de.w : 0.f};
                        *reinterpret_cast<f32x4*>(a.Y + prow * a.ldy + c) = g1;
                        s1f += g1;
                        s2f += g1 * ((e4 - mu1) * rs1);
                    } else {
                        *reinterpret_cast<f32x4*>(a.Y + prow * a.ldy + c) = de + r4;
                    }
                }
                if constexpr (W1G) es[(iy_l * TS + ix_l) * SQ + cq_l] = g1;      // (this thread's own slot: e was read from it above)
            }
            if constexpr (W1G) {
                // the expansion's weight gradient while g1 is on chip: sum over the tile's pixels of g1[p][c] x[p][k] — lane (channel i,
                // pixel kk) reads g1 from LDS, lane (input channel j, pixel kk) reads x; four pixels per MFMA, the groups dealt to the waves
                {
                    __syncthreads();
                    const int wave = tid >> 6, lj = tid & 15, kk = (tid & 63) >> 4;
#pragma unroll 1
                    for (int pg = wave; pg < TS * TS / 4; pg += 4) {
                        const int p = pg * 4 + kk;
                        const int iy = iy0 + p / TS, ix = ix0 + p % TS;
                        const bool inb = iy < a.H && ix < a.W;
                        float bx[VE];
#pragma unroll
                        for (int ci = 0; ci < VE; ++ci) {
                            const int k = ci * 16 + lj;
                            bx[ci] = inb && k < a.ve.cin ? a.ve.X[(((long)b * a.H + iy) * a.W + ix) * a.ve.cin + k] : 0.f;
                        }
#pragma unroll
                        for (int ct = 0; ct < SQ / 4; ++ct) {
                            const float gv = reinterpret_cast<const float*>(&es[p * SQ + ct * 4 + (lj >> 2)])[lj & 3];
#pragma unroll
                            for (int ci = 0; ci < VE; ++ci) acc1[ct][ci] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv, bx[ci], acc1[ct][ci], 0, 0, 0);
                        }
                    }
                }
            }
        }
        if (BN1) { S1 += to_f64(s1f); S2 += to_f64(s2f); }
        __syncthreads();      // the next item overwrites the tile
    }
    // ---- the workgroup's partial tap gradients: slot (j, i) of the threads of one class and channel quad, added in lane order
#pragma unroll
    for (int j = 0; j < AJ; ++j)
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            __syncthreads();
            red[tid] = acc[j][i];
            __syncthreads();
            if (tid < NCLS * SQ) {
                const int rc = tid / SQ, q = tid % SQ;
                f32x4 sum = zero;
                for (int g = 0; g < PL / NCLS; ++g) sum += red[(g * NCLS + rc) * SQ + q];
                const int rpy = S == 1 ? 0 : (rc >> 1), rpx = S == 1 ? 0 : (rc & 1);
                const int ky = HS ? rc * KH + j : (rpy + P) % S + S * j, kx = (rpx + P) % S + S * i;
                const int cc = (slab * SQ + q) * 4;
                if (ky < KS && kx < KS && cc < a.C)
                    *reinterpret_cast<f32x4*>(a.ptaps + ((long)wslot * KK + ky * KS + kx) * a.C + cc) = sum;
            }
        }
    if (BN1) {
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            __syncthreads();
            red64[tid] = which == 0 ? S1 : S2;
            __syncthreads();
            if (tid < SQ) {
                f64x4 sum = (f64x4){0.0, 0.0, 0.0, 0.0};
                for (int g = 0; g < PL; ++g) sum += red64[g * SQ + tid];
                const int cc = (slab * SQ + tid) * 4;
                if (cc < a.C) *reinterpret_cast<f64x4*>(a.psums + ((long)wslot * 2 + which) * a.C + cc) = sum;
            }
        }
    }
    if constexpr (W1G) {
        {      // the four waves' shares added in wave order, one partial per workgroup
            const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
            for (int ct = 0; ct < SQ / 4; ++ct)
#pragma unroll
                for (int ci = 0; ci < VE; ++ci) {
                    __syncthreads();
                    if (wave > 0) red[(wave - 1) * 64 + lane] = acc1[ct][ci];
                    __syncthreads();
                    if (wave == 0) {
                        f32x4 v = acc1[ct][ci];
#pragma unroll
                        for (int w = 0; w < 3; ++w) v += red[w * 64 + lane];
                        const int k = ci * 16 + (lane & 15);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ch = slab * SQ * 4 + ct * 16 + 4 * (lane >> 4) + r;      // lane (k, q), component r = channel 4 q + r
                            if (ch < a.C && k < a.ve.cin) a.pw1[((long)wslot * a.C + ch) * a.ve.cin + k] = v[r];
                        }
                    }
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Depthwise conv FORWARD of the block-fused step: Y = DW act(X) with the input activation applied once per input pixel as the
// tile's input region goes to LDS (zero outside the map: the padding pads the ACTIVATION), and the column sums sum(y), sum(y^2)
// of the raw output — float64 per thread over all tiles of a persistent workgroup, ONE partial row per workgroup (the
// thread-per-strip dw_stat_kernel wrote one per 256 threads: 58 MB of partials for a 672-channel 16 x 16 map, and ran at one
// wave per SIMD).  Same slab / tile / lane scheme as dw_bwd_kernel; output tiles of 16 x 16 (stride 1) or 8 x 8 (stride 2).
struct DwFwdArgs {
    const float* X;
    ActIn in;
    const float* Wt;      // [KS*KS][C]
    float* Y;
    double* psums;        // [wgs_per_slab][2][C]
    int ldx, ldy;
    int B, H, W, Ho, Wo, C;
    int tiles_x, tiles_y, wgs_per_slab, nslab;
    VirtE ve;             // VE: X is not read, the operand is act(ve.X ve.W1^T)
};

template <int KS, int S, int SQ, int VE = 0, int TS1 = 16>      // VE = NC chunks of 16 input channels of a virtual expansion (0: X is read)
__global__ __launch_bounds__(256, 2) void dw_fwd_kernel(DwFwdArgs a) {
    constexpr int P = KS / 2, KK = KS * KS;
    constexpr int TO = S == 1 ? TS1 : 8;               // output tile side (TS1 = 8: stride-1 maps of at most 8 x 8 pixels, see dw_bwd_kernel)
    constexpr int IR = (TO - 1) * S + KS;              // input region side
    constexpr int PITCH = (IR + 1) * SQ;
    constexpr int PL = 256 / SQ;
    constexpr int T = S == 1 ? (TO == 8 ? 2 : 4) : 1;  // output pixels per thread and sweep (a run along x)
    constexpr int SMEM = IR * PITCH > 512 ? IR * PITCH : 512;
    __shared__ f32x4 tile[SMEM];
    f64x4* red64 = reinterpret_cast<f64x4*>(tile);
    const int tid = threadIdx.x;
    const int cq_l = tid % SQ, pl = tid / SQ;
    const int slab = blockIdx.x % a.nslab, wslot = blockIdx.x / a.nslab;
    const int c = (slab * SQ + cq_l) * 4;
    const bool cv = c < a.C;
    const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bool affine = a.in.a != nullptr;
    f32x4 ia = zero, ib = zero;
    if (affine && cv) { ia = *reinterpret_cast<const f32x4*>(a.in.a + c); ib = *reinterpret_cast<const f32x4*>(a.in.b + c); }
    constexpr bool WREG = KK <= 9;                      // 3 x 3 taps in registers, 5 x 5 in LDS (100 registers otherwise)
    __shared__ f32x4 wl[WREG ? 1 : KK * SQ];
    f32x4 wr[WREG ? KK : 1];
    if (WREG) {
#pragma unroll
        for (int t = 0; t < KK; ++t) wr[WREG ? t : 0] = cv ? *reinterpret_cast<const f32x4*>(a.Wt + (long)t * a.C + c) : zero;
    } else {
        for (int t = pl; t < KK; t += PL) wl[t * SQ + cq_l] = cv ? *reinterpret_cast<const f32x4*>(a.Wt + (long)t * a.C + c) : zero;
    }
    f64x4 S1 = (f64x4){0.0, 0.0, 0.0, 0.0}, S2 = S1;
    // VE: W1 fragments (lane (channel, k quarter)) and the activation of the two channel quads this lane's results belong to
    f32x4 wa[VE ? SQ / 4 : 1][VE ? VE : 1], va[VE ? SQ / 4 : 1], vb[VE ? SQ / 4 : 1];
    if (VE) {
#pragma unroll
        for (int ct = 0; ct < SQ / 4; ++ct) {
#pragma unroll
            for (int ci = 0; ci < VE; ++ci) {
                const int ch = slab * SQ * 4 + ct * 16 + (tid & 15), k = ci * 16 + 4 * ((tid & 63) >> 4);
                wa[VE ? ct : 0][VE ? ci : 0] = ch < a.C && k < a.ve.cin ? *reinterpret_cast<const f32x4*>(a.ve.W1 + (long)ch * a.ve.cin + k) : zero;
            }
            const int c4 = (slab * SQ + ct * 4 + ((tid & 63) >> 4)) * 4;
            va[VE ? ct : 0] = c4 < a.C ? *reinterpret_cast<const f32x4*>(a.in.a + c4) : zero;
            vb[VE ? ct : 0] = c4 < a.C ? *reinterpret_cast<const f32x4*>(a.in.b + c4) : zero;
        }
    }
    const long xbytes = (long)a.B * a.H * a.W * (VE ? a.ve.cin : a.ldx) * 4;      // < 2^31: checked on the host
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(VE ? a.ve.X : a.X), 0, (int)xbytes, 0x00020000);
    const int n_items = a.B * a.tiles_y * a.tiles_x;
    for (int item = wslot; item < n_items; item += a.wgs_per_slab) {
        const int tx = item % a.tiles_x, ty = (item / a.tiles_x) % a.tiles_y, b = item / (a.tiles_x * a.tiles_y);
        const int oy0 = ty * TO, ox0 = tx * TO;
        const int iy0 = oy0 * S - P, ix0 = ox0 * S - P;
        f32x4 s1f = zero, s2f = zero;      // this tile's share of the sums (at most 16 values per lane), then float64
        int wq = cq_l;
        asm volatile("" : "+v"(wq));        // (LDS weight index, opaque: see dw_bwd_kernel)
        constexpr int NIDX = IR * IR * SQ, U = 4;
        if constexpr (VE) {
            const int wave = tid >> 6, j = tid & 15, kk = (tid & 63) >> 4;
#pragma unroll 1
            for (int rt = wave; rt < (IR * IR + 15) / 16; rt += 4) {
                const int pix = rt * 16 + j;                     // region pixel of this lane's column
                const int r = pix / IR, cc = pix - r * IR;
                const int y = iy0 + r, x = ix0 + cc;
                const bool inb = pix < IR * IR && y >= 0 && y < a.H && x >= 0 && x < a.W;
                f32x4 xb[VE ? VE : 1];
#pragma unroll
                for (int ci = 0; ci < VE; ++ci) {
                    const int off = inb && ci * 16 + 4 * kk < a.ve.cin ? (((b * a.H + y) * a.W + x) * a.ve.cin + ci * 16 + 4 * kk) * 4 : (int)0x80000000;
                    xb[ci] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
                }
#pragma unroll
                for (int ct = 0; ct < SQ / 4; ++ct) {
                    const f32x4 v = act4(virt_e_tile<VE ? VE : 1>(wa[ct], xb), va[ct], vb[ct], a.in.relu != 0);
                    const bool cok = (slab * SQ + ct * 4 + kk) * 4 < a.C;
                    if (pix < IR * IR) tile[r * PITCH + cc * SQ + ct * 4 + kk] = inb && cok ? v : zero;
                }
            }
        } else
        for (int i0 = 0; i0 < NIDX; i0 += 256 * U) {
            f32x4 xv[U];
            bool in[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = i0 + u * 256 + tid;
                const int pix = idx / SQ;
                const int r = pix / IR, cc = pix - r * IR;
                const int y = iy0 + r, x = ix0 + cc;
                in[u] = idx < NIDX && cv && y >= 0 && y < a.H && x >= 0 && x < a.W;
                const int off = in[u] ? (((b * a.H + y) * a.W + x) * a.ldx + c) * 4 : (int)0x80000000;
                xv[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = i0 + u * 256 + tid;
                const int pix = idx / SQ;
                const int r = pix / IR, cc = pix - r * IR;
                f32x4 v = xv[u];
                if (affine) v = act4(v, ia, ib, a.in.relu != 0);
                if (idx < NIDX) tile[r * PITCH + cc * SQ + cq_l] = in[u] ? v : zero;
            }
        }
        __syncthreads();
        if (S == 1) {
            constexpr int RPS = PL / (TO / T);             // output rows per sweep; consecutive pixel lanes are consecutive rows
#pragma unroll 1
            for (int sw = 0; sw < TO / RPS; ++sw) {
                const int oy_l = sw * RPS + pl % RPS, ox_l = (pl / RPS) * T;
                f32x4 out[T];
#pragma unroll
                for (int i = 0; i < T; ++i) out[i] = zero;
                int lb = oy_l * PITCH + ox_l * SQ + cq_l;
#pragma unroll
                for (int ky = 0; ky < KS; ++ky) {
                    const int base = lb + ky * PITCH;
                    f32x4 win[T + KS - 1];
#pragma unroll
                    for (int j = 0; j < T + KS - 1; ++j) win[j] = tile[base + j * SQ];
#pragma unroll
                    for (int kx = 0; kx < KS; ++kx) {
                        const f32x4 w = WREG ? wr[WREG ? ky * KS + kx : 0] : wl[(ky * KS + kx) * SQ + wq];
#pragma unroll
                        for (int i = 0; i < T; ++i) out[i] += win[i + kx] * w;
                    }
                    asm volatile("" : "+v"(lb), "+v"(wq) : "v"(out[0]), "v"(out[1]), "v"(out[T - 2]), "v"(out[T - 1]));      // (see dw_bwd_kernel)
                }
                const int oy = oy0 + oy_l;
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    const int ox = ox0 + ox_l + i;
                    if (cv && oy < a.Ho && ox < a.Wo) {
                        *reinterpret_cast<f32x4*>(a.Y + (((long)b * a.Ho + oy) * a.Wo + ox) * a.ldy + c) = out[i];
                        s1f += out[i];
                        s2f += out[i] * out[i];
                    }
                }
            }
        } else {
#pragma unroll 1
            for (int sw = 0; sw < TO * TO / PL; ++sw) {
                const int id = sw * PL + pl;
                const int oy_l = id / TO, ox_l = id % TO;
                f32x4 out = zero;
#pragma unroll
                for (int ky = 0; ky < KS; ++ky)
#pragma unroll
                    for (int kx = 0; kx < KS; ++kx)
                        out += tile[(oy_l * S + ky) * PITCH + (ox_l * S + kx) * SQ + cq_l] * (WREG ? wr[WREG ? ky * KS + kx : 0] : wl[(ky * KS + kx) * SQ + wq]);
                const int oy = oy0 + oy_l, ox = ox0 + ox_l;
                if (cv && oy < a.Ho && ox < a.Wo) {
                    *reinterpret_cast<f32x4*>(a.Y + (((long)b * a.Ho + oy) * a.Wo + ox) * a.ldy + c) = out;
                    s1f += out;
                    s2f += out * out;
                }
            }
        }
        S1 += to_f64(s1f);
        S2 += to_f64(s2f);
        __syncthreads();
    }
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        __syncthreads();
        red64[tid] = which == 0 ? S1 : S2;
        __syncthreads();
        if (tid < SQ) {
            f64x4 sum = (f64x4){0.0, 0.0, 0.0, 0.0};
            for (int g = 0; g < PL; ++g) sum += red64[g * SQ + tid];
            const int cc = (slab * SQ + tid) * 4;
            if (cc < a.C) *reinterpret_cast<f64x4*>(a.psums + ((long)wslot * 2 + which) * a.C + cc) = sum;
        }
    }
}

// The E-free form of an expansion's backward (BnbIn, fear_train.hip): from BN1's coefficients [A | s1 | mu | Q] and the expansion
// weights W1 [cexp][cin], the extended K-major weight matrix of the input-gradient GEMM
//     Wext [cexp + cin][cin] = [ W1 ; -T ],   T = W1^T diag(A Q) W1
// so that  dx = [A (g1 - s1 + mu Q) | x] Wext  (the GEMM's operand is g1 with BnbIn::E = nullptr, then the block input as loaded).
// (one workgroup per row of T, the reduction over cexp dealt to 1024 / kp lanes per element, kp = cin rounded up to a power of two —
// the kernel sits between BN1's coefficients and the input-gradient GEMM on the chain of input gradients; further workgroups copy W1)
__global__ __launch_bounds__(1024) void irb_lin_weights_kernel(const float* coef, const float* W1, float* Wext, int cexp, int cin, int kp_log2) {
    __shared__ double part[1024];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= cin) {
        const int idx = ((int)blockIdx.x - cin) * 1024 + tid;
        if (idx < cexp * cin) Wext[idx] = W1[idx];
        return;
    }
    const int kp = 1 << kp_log2, J = 1024 >> kp_log2;
    const int k1 = blockIdx.x, k = tid & (kp - 1), j = tid >> kp_log2;
    double t = 0.0;
    if (k < cin)
        for (int c = j; c < cexp; c += J)
            t += (double)W1[(long)c * cin + k1] * ((double)coef[c] * (double)coef[3 * cexp + c]) * (double)W1[(long)c * cin + k];
    part[tid] = t;
    __syncthreads();
    if (j != 0 || k >= cin) return;
    for (int l = 1; l < J; ++l) t += part[l * kp + k];      // fixed order
    Wext[(long)(cexp + k1) * cin + k] = (float)-t;
}

// ... and of its weight gradient: dW1 [cexp][cin] (holding [A (g1 - s1 + mu Q)]^T x) -= diag(A Q) W1 G, G = x^T x [cin][cin]
__global__ __launch_bounds__(256) void irb_lin_wgrad_fix_kernel(const float* coef, const float* W1, const float* G, int ldg, float* dW1, int cexp, int cin) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= cexp * cin) return;
    const int c = idx / cin, k = idx - c * cin;
    double t = 0.0;
    for (int k1 = 0; k1 < cin; ++k1) t += (double)W1[(long)c * cin + k1] * (double)G[(long)k1 * ldg + k];
    dW1[idx] = (float)((double)dW1[idx] - (double)coef[c] * (double)coef[3 * cexp + c] * t);
}

// ... and where dw_bwd_kernel<.., W1G> has already summed R[c][k] = sum_m g1[m][c] x[m][k] (dW1 holds it): the whole of BatchNorm1's algebra
//     dW1 = A (R - (s1 - mu Q) Sx) - (A Q) W1 G,   Sx = column sums of x (gram_kernel's tail: G | Sx with row pitch ldg)
__global__ __launch_bounds__(256) void irb_lin_wgrad_fix2_kernel(const float* coef, const float* W1, const float* G, int ldg, float* dW1, int cexp, int cin) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= cexp * cin) return;
    const int c = idx / cin, k = idx - c * cin;
    double t = 0.0;
    for (int k1 = 0; k1 < cin; ++k1) t += (double)W1[(long)c * cin + k1] * (double)G[(long)k1 * ldg + k];
    const double A = coef[c], s1 = coef[cexp + c], mu = coef[2 * cexp + c], Q = coef[3 * cexp + c];
    dW1[idx] = (float)(A * ((double)dW1[idx] - (s1 - mu * Q) * (double)G[(long)ldg * ldg + k]) - A * Q * t);
}

// running statistics of a BatchNorm from its saved vec = [mean | rstd | a | b] (the forward ran with running_mean = NULL so that
// two passes of the shared trunk can overlap on two streams; torch's order — template pass first — is restored by applying the
// search pass's update afterwards): biased variance = 1 / rstd^2 - eps, tracked unbiased
__device__ __forceinline__ void bn_running_update_one(const float* vec, float* rm, float* rv, int C, int c, double count, double momentum, double eps) {
    const double mean = (double)vec[c], rs = (double)vec[C + c];
    double var = 1.0 / (rs * rs) - eps;
    if (var < 0.0) var = 0.0;
    rm[c] = (float)((1.0 - momentum) * (double)rm[c] + momentum * mean);
    const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
    rv[c] = (float)((1.0 - momentum) * (double)rv[c] + momentum * unbiased);
}
__global__ __launch_bounds__(256) void bn_running_update_kernel(const float* vec, float* rm, float* rv, int C, double count, double momentum, double eps) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) bn_running_update_one(vec, rm, rv, C, c, count, momentum, eps);
}

// the same update for up to 64 BatchNorms in one launch (block = one BatchNorm): the deferred updates of a trunk pass were 47 launches
struct BnRunMulti { const float* vec[64]; float* rm[64]; float* rv[64]; int C[64]; double count[64]; };
__global__ __launch_bounds__(256) void bn_running_update_multi_kernel(BnRunMulti t, double momentum, double eps) {
    const int e = blockIdx.x, C = t.C[e];
    const float* vec = t.vec[e];
    const double count = t.count[e];
    for (int c = threadIdx.x; c < C; c += blockDim.x) bn_running_update_one(vec, t.rm[e], t.rv[e], C, c, count, momentum, eps);
}

}  // namespace
