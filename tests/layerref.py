"""Float64 references of the layer family of training operators (include/fear_train.h: fear_pw_forward / _backward_data /
_backward_weight[_act], fear_col_sum, the BatchNorm forwards and backwards in all their forms, fear_pw_forward_stats,
fear_dw_forward[_stats] / _backward_data / _backward_weight[_act], fear_stem_im2col) with an element-wise error bound each, the seeded
inputs and the case tables of their tests, and an fp32 numpy restatement of every formula that can be broken on purpose.  A helper
module (not collected), shared by tests/test_train_layer_ops_gpu.py (the kernels against reference and bound, and the plan query
that proves which branch a case reaches) and tests/test_layer_ops_reference_cpu.py (the restatement fits every bound, every mutant
leaves one).

Conventions of tests/headref.py: a reference returns (reference, bound) pairs, `got` passes where |got - reference| <= bound
element-wise, u = 2^-24.  Bounds come from the arithmetic the kernels are written in (cited next to each), never from what they
return.  Two kinds of input per GEMM- or sum-shaped output:
  "gauss"  standard normal operands against the derived bound;
  "int"    small integers (x, dy, w in {-2..2}, a in {1, 2}, b in {-1, 0, 1}) with sum |a||b| < 2^24 for every output element
           (`int_headroom` returns that sum; the CPU test asserts it for every case): every partial sum in any order is then an
           exact fp32 integer, the bound is ZERO and the kernel must equal the float64 reference bit for bit — what catches a
           dropped, doubled or foreign row in a 100 000-row reduction, where no rounding bound can.
ReLU masks: fma(x, a, b) > 0 in fp32 has the sign of x a + b in float64 (the product of two fp32 numbers is exact in 53 bits and
rounding cannot change a non-zero sign; the inputs hold no value near the underflow range), so the reference forms the operator's own
mask from the operator's inputs and no element is excused from any comparison."""
import numpy as np

from headref import U, _gemm_bound, excess  # noqa: F401  (excess is re-exported to the two test files)

f32, f64 = np.float32, np.float64
EPS, MOMENTUM = 1e-5, 0.1
D = 2.0 ** -53            # unit roundoff of float64

# ---------------------------------------------------------------------------------------------------------------------------
# case tables; the `claim` of a case is what fear_layer_plan_info must report for it (tests/test_train_layer_ops_gpu.py::
# test_cases_reach_the_branches_they_claim)

# pointwise forward (rows x contraction x outputs); fear_pw_backward_data runs the same table with the roles swapped (M, K = outputs,
# N = contraction), so the claim is about `forward` there and about `dx` of (M, N, K) here
GEMM_CASES = [
    ((768, 256, 256), dict(lds=1, row_tile=64, ntw=8, col_blocks=2)),                 # the product's call (ldx = 320)
    ((10945, 32, 672), dict(lds=1, row_tile=128, ntw=7, col_blocks=6)),               # 86 x 6 = 516 workgroups; last row tile 65 rows
    ((10880, 32, 672), dict(lds=1, row_tile=64, ntw=7, col_blocks=6)),                # 85 x 6 = 510: the other side
    ((200, 48, 80), dict(lds=1, row_tile=64, ntw=8, col_blocks=1)),                   # 5 tiles of 8, three k-groups, ragged rows
    ((65, 36, 36), dict(lds=1, row_tile=64, ntw=4, col_blocks=1)),                    # 3 tiles of 4, last 4 wide, k tail of 4
    ((131072, 32, 16), dict(lds=1, row_tile=128, ntw=4, col_blocks=1)),               # the last LDS row count
    ((131200, 32, 16), dict(lds=0, grid_x=1025, grid_y=1, nt=1)),                     # pw_mfma_kernel at K >= 32
    ((76795, 16, 112), dict(lds=0, grid_x=600, grid_y=2, nt=1)),                      # 7 passes dealt over gridDim.y = 2: 4 and 3
    ((2304, 256, 4), dict(lds=0, grid_y=1, nt=1)),                                    # fewer than 16 outputs
    ((9, 4, 8), dict(lds=0, grid_x=1, nt=1)),                                         # the smallest legal shape
]
# weight gradient (M, K = width of x, N = width of dy)
WGRAD_CASES = [
    ((3001, 12, 100), dict(swapped=0, lds_tile=0, small_k=1)),
    ((2050, 28, 16), dict(swapped=0, lds_tile=0, small_k=2)),
    ((2050, 20, 72), dict(swapped=0, lds_tile=0, small_k=2, n_tiles=2)),
    ((2304, 256, 4), dict(swapped=1, small_k=1, n_tiles=4)),
    ((2304, 100, 12), dict(swapped=1, small_k=1, n_tiles=2)),                         # the wide tile ragged
    ((3000, 96, 24), dict(swapped=1, small_k=2)),
    ((777, 72, 40), dict(swapped=0, lds_tile=0, small_k=0, n_tiles=1, k_tiles=2)),    # 64 x 64 tiles, both ragged
    # (N = 36, not the issue's 32: with N <= 32 and K > 32 wgrad_launch_plan trades the operands and never stages through LDS)
    ((16383, 48, 36), dict(swapped=0, lds_tile=0, small_k=0)),
    ((16384, 48, 36), dict(swapped=0, lds_tile=1, small_k=0, n_tiles=1, k_tiles=1)),  # one of the four waves live
    ((16400, 136, 72), dict(swapped=0, lds_tile=1, n_tiles=1, k_tiles=2)),            # second k tile 8 wide, ragged last stage
]
# column reductions (M, C): rows per workgroup, workgroups
COL_CASES = [
    ((127, 96), dict(col_rows=128, col_blocks=1)),         # 24 quads: 10 row lanes, 16 idle threads
    ((129, 96), dict(col_rows=128, col_blocks=2)),         # a second workgroup of one row
    ((300, 4), dict(col_rows=128, col_blocks=3)),          # 256 row lanes
    ((141, 1024), dict(col_rows=128, col_blocks=2)),       # one row lane; a workgroup of 13 rows = 8 + 4 + 1 unrolled
    ((777, 672), dict(col_rows=128, col_blocks=7)),
    ((131073, 4), dict(col_rows=256, col_blocks=513)),     # 256 rows per workgroup, > 64 partials in the finalize
]
# depthwise (B, H, W, C); k in {3, 5}, stride in {1, 2} (H = 1: stride 1 only)
DW_CASES = [(3, 12, 6, 8), (2, 2, 2, 4), (2, 1, 8, 12), (1, 8, 8, 1024)]
DW_WGRAD_ONLY = (3, 256, 256, 4)                          # > 131072 output pixels: 256 per workgroup
DW_SPAN_LD = (8388604, 8388608)                           # B = 1, H = W = 8, C = 8: 64 rows of this pitch just below / at 2^31 bytes
STEM_CASES = [(2, 2, 2), (1, 6, 10), (2, 64, 48)]         # (n, H, W)


WGRAD_FORMS = ["plain", "act_relu0", "act_relu1", "act_null"]      # fear_pw_backward_weight | _act with relu 0 / 1 | _act with in_a = NULL


def wgrad_act(d, form):
    """(a, b, relu) of a weight-gradient form from the inputs d"""
    return (d["a"], d["b"], int(form[-1])) if form.startswith("act_relu") else (None, None, 0)


def layer_plan(M, K, N, ws_bytes=1 << 40, dw=None):
    """fear_layer_plan_info (host only) -> FearLayerPlanInfo; dw = (B, H, W, C, k, stride, ld)"""
    import ctypes
    from feartracker_amd import train_abi
    info = train_abi.FearLayerPlanInfo()
    shape = train_abi.FearLayerDwShape(*dw) if dw else None
    rc = train_abi.load_train_library().fear_layer_plan_info(M, K, N, ws_bytes, ctypes.byref(shape) if dw else None, ctypes.byref(info))
    assert rc == 0, (rc, M, K, N, dw)
    return info


def wgrad_ws(M, K, N):
    """room for the 1 024 partials wgrad_plan cuts at the most: the slicing is then the shape's own, not the workspace's (the training
    step shares one workspace sized by its largest layer; test_pw_backward_weight_workspace covers a plan the workspace caps)"""
    return 1024 * N * K * 4


def wgrad_plan(M, K, N, ws_bytes=None):
    w = layer_plan(M, K, N, wgrad_ws(M, K, N) if ws_bytes is None else ws_bytes).w
    return (w.rows_per_slice, w.slices, w.lds_tile)


def dw_wgrad_plan(B, H, W, C, k, stride):
    d = layer_plan(16, 4, 4, dw=(B, H, W, C, k, stride, C)).dw
    return (d.wgrad_rows, d.wgrad_workgroups)


def dw_variants(case):
    return [(k, s) for k in (3, 5) for s in (1, 2) if case[1] % s == 0 and case[2] % s == 0 and not (case[1] == 1 and s == 2)]


# ---------------------------------------------------------------------------------------------------------------------------
# inputs


def _draw(rng, shape, kind, lo=-2, hi=2):
    if kind == "int":
        return rng.integers(lo, hi + 1, shape).astype(f32)
    return rng.standard_normal(shape).astype(f32)


def gemm_inputs(M, K, N, kind="gauss", seed=0):
    """x (M, K), w (N, K), bias (N), dy (M, N), add (M, K)"""
    rng = np.random.default_rng(4000 + seed + M + 7 * K + 13 * N)
    return {"x": _draw(rng, (M, K), kind), "w": _draw(rng, (N, K), kind), "bias": _draw(rng, (N,), kind),
            "dy": _draw(rng, (M, N), kind), "add": _draw(rng, (M, K), kind),
            "a": rng.integers(1, 3, K).astype(f32) if kind == "int" else rng.uniform(0.5, 1.5, K).astype(f32),
            "b": rng.integers(-1, 2, K).astype(f32) if kind == "int" else (0.5 * rng.standard_normal(K)).astype(f32)}


def bn_inputs(M, C, kind="gauss", seed=0):
    """x with per-column scale and offset — column 1 has mean 300 and standard deviation 0.01 (fp32 sums would lose its variance) —
    dy, gamma, beta, residual, running statistics; y_act = an activation tensor of its OWN draw with exact zeros (the unfused
    backward takes it as an input); int: x, dy in {-2..2}"""
    rng = np.random.default_rng(5000 + seed + M + 3 * C)
    if kind == "int":
        x = _draw(rng, (M, C), "int")
    else:
        x = rng.standard_normal((M, C)) * rng.uniform(0.2, 3.0, C) + rng.uniform(-2.0, 2.0, C)
        x[:, 1] = 300.0 + 0.01 * rng.standard_normal(M)
        x = x.astype(f32)
    y_act = np.maximum(rng.standard_normal((M, C)), 0).astype(f32)
    return {"x": x, "dy": _draw(rng, (M, C), kind), "gamma": rng.uniform(0.5, 1.5, C).astype(f32),
            "beta": (0.5 * rng.standard_normal(C)).astype(f32), "residual": rng.standard_normal((M, C)).astype(f32), "y_act": y_act,
            "running_mean": rng.standard_normal(C).astype(f32), "running_var": rng.uniform(0.5, 2.0, C).astype(f32)}


def dw_inputs(B, H, W, C, k, stride, kind="gauss", seed=0):
    """x (B, H, W, C), w_taps (k k, C), bias (C), dy (B, H / s, W / s, C), a / b (C)"""
    rng = np.random.default_rng(6000 + seed + B + 3 * H + 5 * W + 7 * C + 11 * k + 13 * stride)
    return {"x": _draw(rng, (B, H, W, C), kind), "w": _draw(rng, (k * k, C), kind), "bias": _draw(rng, (C,), kind),
            "dy": _draw(rng, (B, H // stride, W // stride, C), kind),
            "a": rng.integers(1, 3, C).astype(f32) if kind == "int" else rng.uniform(0.5, 1.5, C).astype(f32),
            "b": rng.integers(-1, 2, C).astype(f32) if kind == "int" else (0.5 * rng.standard_normal(C)).astype(f32)}


def strided(flat, rows, cols, ld, off=0, pitch_is_width=False):
    """rows x cols view of a flat buffer at pitch ld from element off; pitch_is_width: the mutant that multiplies the row by the width"""
    p = cols if pitch_is_width else ld
    return np.lib.stride_tricks.as_strided(flat[off:], (rows, cols), (4 * p, 4), writeable=False)


def act64(x, a, b, relu):
    """fma(x, a, b) [max 0] in float64 of the fp32 inputs; a = None: x as it is"""
    if a is None:
        return x.astype(f64)
    t = x.astype(f64) * a.astype(f64) + b.astype(f64)
    return np.maximum(t, 0) if relu else t


def act32(x, a, b, relu):
    """the same in fp32 with ONE rounding, as the fma of act4 (csrc/fear_train.hip) gives it"""
    if a is None:
        return x
    return act64(x, a, b, relu).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------------
# pointwise forward and input gradient: headref's GEMM bound (2 K + 4) u (|A| |B| + |add|), contraction <= 672; gemm_lds_kernel and
# pw_mfma_kernel add the products of one output with v_mfma_f32_16x16x4_f32 alone, k ascending, then the bias / residual once


def pw_forward(x, w, bias=None):
    x, w = x.astype(f64), w.astype(f64)
    b = np.zeros(w.shape[0]) if bias is None else bias.astype(f64)
    return x @ w.T + b, _gemm_bound(x.shape[1], np.abs(x) @ np.abs(w).T, np.abs(b))


def pw_backward_data(dy, w, add=None):
    dy, w = dy.astype(f64), w.astype(f64)
    a = np.zeros((dy.shape[0], w.shape[1])) if add is None else add.astype(f64)
    return a + dy @ w, _gemm_bound(dy.shape[1], np.abs(dy) @ np.abs(w), np.abs(a))


def _drop(out, mutant):
    if mutant == "last_row":
        out[-1] = 0
    if mutant == "last_quad":
        out[..., -4:] = 0
    return out


def pw_forward_fp32(x, w, bias=None, mutant=None):
    """mutants: "last_row" / "last_quad" (never written), "no_bias" """
    y = x @ w.T
    if bias is not None and mutant != "no_bias":
        y = y + bias
    return _drop(y, mutant)


def pw_backward_data_fp32(dy, w, add=None, mutant=None):
    """mutants: "last_row", "last_quad", "no_add" """
    dx = dy @ w
    if add is not None and mutant != "no_add":
        dx = dx + add
    return _drop(dx, mutant)


# ---------------------------------------------------------------------------------------------------------------------------
# pointwise weight gradient dw[n][k] = sum_m dy[m][n] x'[m][k], x' = act(x)
#
# 2 M u sum |ab| is larger than the result from ~16 000 rows up, so the bound follows the kernels' summation TREE; an fp32 sum whose
# every term passes through at most d rounded additions errs by at most gamma_d sum |terms| (Higham 4.2), and d is short here:
#   a slice of `rows_per_slice` rows (wgrad_plan; the plan query reports it) is one workgroup;
#   pw_wgrad_kernel / pw_wgrad_smallk_kernel: wave w takes the 16-row groups w, w + 4, ... of the slice and adds its rows four per MFMA:
#       n_w = 16 ceil(rows_per_slice / 64) rows in one chain; the MFMA does not say how it rounds inside its four terms, so a row
#       counts twice (headref's factor 2): 2 n_w; then (w0 + w2) + (w1 + w3): 2 more additions;
#   wgrad_lds_kernel: the four waves split the TILE and each adds ALL rows of the slice: n_w = rows_per_slice, no wave sum;
#   slice_sum_kernel: with fewer than 64 slices one lane adds them in order (slices - 1 additions); from 64 up 16 lanes add every
#       16th slice (ceil(slices / 16) - 1), then the lane sums in order (15);
#   + 1 for the rounding of act() on x' (the reference forms it in float64), + 3 spare for the 1 / (1 - d u) of gamma_d (d u < 2e-4).
# A single missing row is an error of ~ |dy x|, the bound at 16 384 rows ~ 530 u sum |dy x| ~ 0.3: the Gaussian form sees a lost row
# only where its term happens to be large — the integer form sees every one.


def wgrad_depth(rows_per_slice, slices, lds_tile):
    n_w = rows_per_slice if lds_tile else 16 * -(-rows_per_slice // 64)
    chain = (-(-slices // 16) - 1 + 15) if slices >= 64 else slices - 1
    return 2 * n_w + (0 if lds_tile else 2) + chain + 1 + 3


def pw_backward_weight(dy, x, a=None, b=None, relu=0, plan=None, kind="gauss"):
    """plan = (rows_per_slice, slices, lds_tile) of fear_layer_plan_info for this call's workspace; int: bound 0"""
    dy64, xa = dy.astype(f64), act64(x, a, b, relu)
    ref = dy64.T @ xa
    if kind == "int":
        return ref, np.zeros_like(ref)
    return ref, wgrad_depth(*plan) * U * (np.abs(dy64).T @ np.abs(xa))


def pw_backward_weight_fp32(dy, x, a=None, b=None, relu=0, plan=None, mutant=None):
    """the same tree in fp32: per slice and wave an fp32 product of that wave's rows (BLAS: some fp32 order of the same chain length),
    the waves (w0 + w2) + (w1 + w3), the slices in slice_sum_kernel's order.  mutants: "last_row" (missing from the sum),
    "last_quad" (the last four columns of dw never written), "mask_from_x" (ReLU taken from x > 0 where it is fma(x, a, b) > 0),
    "no_act" (x used raw)"""
    rps, slices, lds_tile = plan
    M = x.shape[0]
    if mutant == "no_act":
        xa = x
    elif mutant == "mask_from_x" and a is not None and relu:
        xa = np.where(x > 0, act32(x, a, b, 0), f32(0))
    else:
        xa = act32(x, a, b, relu)
    if mutant == "last_row":
        xa = xa.copy()
        xa[-1] = 0
    parts = []
    for s in range(slices):
        m0, m1 = s * rps, min((s + 1) * rps, M)
        if lds_tile:
            parts.append(dy[m0:m1].T @ xa[m0:m1])
            continue
        idx = np.arange(m0, m1)
        w = [dy[idx[((idx - m0) // 16) % 4 == q]].T @ xa[idx[((idx - m0) // 16) % 4 == q]] for q in range(4)]
        parts.append((w[0] + w[2]) + (w[1] + w[3]))
    return _drop(slice_sum_fp32(parts), "last_quad" if mutant == "last_quad" else None)


def slice_sum_fp32(parts):
    """slice_sum_kernel: lanes = 16 from 64 slices up, else 1; lane l adds slices l, l + lanes, ... in order, then the lanes in order"""
    lanes = 16 if len(parts) >= 64 else 1
    lane_sums = []
    for lane in range(lanes):
        s = np.zeros_like(parts[0])
        for j in range(lane, len(parts), lanes):
            s = s + parts[j]
        lane_sums.append(s)
    out = lane_sums[0]
    for s in lane_sums[1:]:
        out = out + s
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# column sums: col_reduce_kernel widens every fp32 term to float64 (`s1 += to_f64(v)`), adds lanes, partials and the finalize's 64
# lane sums in float64, and rounds ONCE on the way out (`a.out1[c] = (float)s1`).  Bound: u |ref| for that rounding + M 2^-53 sum |terms|
# for the float64 additions in any order.  An fp32 accumulation (the mutant) errs by ~ sqrt(M) u |partial sums| and leaves it.


def _sum_bound(ref, absterms, M, roundings=1):
    return roundings * U * np.abs(ref) + M * D * absterms


def col_sum(dy, kind="gauss"):
    d = dy.astype(f64)
    ref = d.sum(0)
    return ref, (np.zeros_like(ref) if kind == "int" else _sum_bound(ref, np.abs(d).sum(0), d.shape[0]))


def col_sum_fp32(dy, mutant=None):
    """mutants: "fp32_accumulate" (one serial fp32 chain per column), "last_row" """
    d = dy[:-1] if mutant == "last_row" else dy
    if mutant == "fp32_accumulate":
        return np.cumsum(d, axis=0, dtype=f32)[-1]
    return d.astype(f64).sum(0).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------------
# BatchNorm forward statistics (col_finalize_kernel mode 0 / bn_finalize_kernel), float64 from float64 sums:
#   mean = s1 / M, var = max((s2 - s1 mean) / M, 0), rstd = 1 / sqrt(var + eps), each rounded to fp32 once;
#   running = (1 - momentum) running + momentum stat in float64, rounded once (unbiased variance var M / (M - 1); M = 1 keeps var,
#   where torch has NaN — the kernel's choice, pinned here).
# Bounds: mean u |mean| + e1, e1 = M 2^-53 sum |x| / M (the float64 sum).  var carries the cancellation of s2 - s1 mean:
# dv = (M + 4) 2^-53 (s2 + |s1 mean|) / M absolute (M float64 additions of non-negative terms, the product, the difference, the
# quotient), so rstd errs by u rstd + rstd dv / (2 (var + eps)); running statistics u |ref| + momentum (e1 | dv M / (M - 1)).


def bn_stats(x, running_mean=None, running_var=None, sums=None, count=None):
    """{"mean", "rstd", "running_mean", "running_var"}: (ref, bound) each (running: None when not given).  `sums` = float64 [2][C]
    and `count` instead of x: fear_bn_finalize's inputs."""
    if sums is None:
        x = x.astype(f64)
        M = x.shape[0]
        s1, s2, sabs = x.sum(0), (x * x).sum(0), np.abs(x).sum(0)
        e1, nadd = M * D * sabs / M, M
    else:
        s1, s2, M = sums[0].astype(f64), sums[1].astype(f64), count
        e1, nadd = np.zeros_like(s1), 0
    mean = s1 / M
    var = np.maximum((s2 - s1 * mean) / M, 0)
    rstd = 1 / np.sqrt(var + EPS)
    dv = (nadd + 4) * D * (s2 + np.abs(s1 * mean)) / M
    out = {"mean": (mean, U * np.abs(mean) + e1), "rstd": (rstd, rstd * (U + 0.5 * dv / (var + EPS))), "running_mean": None, "running_var": None}
    if running_mean is not None:
        rm = (1 - MOMENTUM) * running_mean.astype(f64) + MOMENTUM * mean
        unb = var * M / (M - 1) if M > 1 else var
        rv = (1 - MOMENTUM) * running_var.astype(f64) + MOMENTUM * unb
        out["running_mean"] = (rm, U * np.abs(rm) + MOMENTUM * e1)
        out["running_var"] = (rv, U * np.abs(rv) + MOMENTUM * dv * (M / (M - 1) if M > 1 else 1))
    return out


def bn_stats_fp32(x, running_mean=None, running_var=None, mutant=None, sums=None, count=None):
    """mutants: "fp32_accumulate" (sum x and sum x^2 in serial fp32 chains), "last_row", "biased_running_var"; with `sums` and `count`
    instead of x (fear_bn_finalize): "fp32_variance" (the sums rounded to fp32 and mean, variance formed in fp32), "biased_running_var" """
    if sums is not None:
        M, s1, s2 = count, sums[0].astype(f64), sums[1].astype(f64)
        if mutant == "fp32_variance":
            t1, t2 = s1.astype(f32), s2.astype(f32)
            m32 = t1 / f32(M)
            return {"mean": m32, "rstd": (1 / np.sqrt(np.maximum((t2 - t1 * m32) / f32(M), 0).astype(f64) + EPS)).astype(f32)}
    else:
        xs = x[:-1] if mutant == "last_row" else x
        M = x.shape[0]
        if mutant == "fp32_accumulate":
            s1, s2 = np.cumsum(xs, axis=0, dtype=f32)[-1].astype(f64), np.cumsum(xs * xs, axis=0, dtype=f32)[-1].astype(f64)
        else:
            s1, s2 = xs.astype(f64).sum(0), (xs.astype(f64) ** 2).sum(0)
    mean = s1 / M
    var = np.maximum((s2 - s1 * mean) / M, 0)
    out = {"mean": mean.astype(f32), "rstd": (1 / np.sqrt(var + EPS)).astype(f32)}
    if running_mean is not None:
        unb = var * M / (M - 1) if M > 1 and mutant != "biased_running_var" else var
        out["running_mean"] = ((1 - MOMENTUM) * running_mean.astype(f64) + MOMENTUM * mean).astype(f32)
        out["running_var"] = ((1 - MOMENTUM) * running_var.astype(f64) + MOMENTUM * unb).astype(f32)
    return out


# The element-wise halves take the per-channel vectors THE OPERATOR RETURNED (after those passed their own bounds above) as inputs:
# the kernel reads exactly those fp32 numbers, and the check on the apply kernel is then as sharp as its own arithmetic — a mean of
# 300 rounded to fp32 moves y by 300 u rstd, which is the statistics' error and no business of the apply pass.
#   bn_apply_kernel   y = (x - mean) * rstd * gamma + beta [max 0]: four roundings -> 4 u (|xhat gamma| + |beta|) (+ u |x - mean| rstd
#                     gamma for the first difference, inside 4 u |xhat gamma| because it is relative to (x - mean) itself)
#   a = gamma * rstd (u |a|), b = fma(-mean, a, beta) (u |b|, with the returned a); y = fma(x, a, b) [max 0] [+ residual]: 2 u (|t| + |r|)


def bn_apply(x, mean, rstd, gamma, beta, relu):
    x, mean, rstd, gamma, beta = (v.astype(f64) for v in (x, mean, rstd, gamma, beta))
    t = (x - mean) * rstd * gamma
    y = t + beta
    return (np.maximum(y, 0) if relu else y), 4 * U * (np.abs(t) + np.abs(beta))


def bn_affine(mean, rstd, gamma, beta, a_got):
    """a from the returned rstd, b from the returned mean and the returned a"""
    a = gamma.astype(f64) * rstd.astype(f64)
    b = beta.astype(f64) - mean.astype(f64) * a_got.astype(f64)
    return (a, U * np.abs(a)), (b, U * np.abs(b))


def bn_act(x, a, b, relu, residual=None):
    t = x.astype(f64) * a.astype(f64) + b.astype(f64)
    r = np.zeros_like(t) if residual is None else residual.astype(f64)
    return (np.maximum(t, 0) if relu else t) + r, 2 * U * (np.abs(t) + np.abs(r))


def bn_apply_fp32(x, mean, rstd, gamma, beta, relu, mutant=None):
    y = (x - mean) * rstd * gamma + beta
    return _drop(np.maximum(y, f32(0)) if relu else y, mutant)


def bn_act_fp32(x, a, b, relu, residual=None, mutant=None):
    """mutants: "no_residual", "last_row", "last_quad" """
    y = act32(x, a, b, relu)
    if residual is not None and mutant != "no_residual":
        y = y + residual
    return _drop(y, mutant)


# BatchNorm backward.  g = dy masked (y_act > 0, or fma(x, a, b) > 0 for the _x forms, or unmasked).
#   col_reduce_kernel<1>: xhat = (x - mean) * rstd in fp32 (two roundings), the products g xhat and both sums in float64, each
#       rounded once: d beta = sum g: u |ref| (+ float64 term); d gamma = sum g xhat: 2 u sum |g xhat| + u |ref| <= 3 u sum |g xhat|.
#       The float64 sums of fear_bn_backward_reduce_x are not rounded: 2 u sum |g xhat| and the float64 term alone.
#   bn_bwd_apply_kernel: dx = gamma * rstd * (g - sg - xhat * sgx), sg = sum_g * inv_m, sgx = sum_gx * inv_m with inv_m = (float)(1 / M),
#       from the RETURNED fp32 sums: sg, sgx 2 u each, xhat 2 u, the product 1: p = xhat sgx 5 u; the two differences u (|g| + |sg|)
#       and u (|g| + |sg| + |p|); gamma * rstd and the last product 2 u: in all <= 8 u |gamma rstd| (|g| + |sg| + |p|).


def bn_mask(dy, y_act=None, x=None, a=None, b=None):
    if y_act is not None:
        return y_act > 0
    if a is not None:
        return x.astype(f64) * a.astype(f64) + b.astype(f64) > 0
    return np.ones(dy.shape, bool)


def bn_backward_sums(dy, x, mean, rstd, mask, kind="gauss", rounded=True):
    """{"dbeta", "dgamma"}: the two column sums; mean / rstd as the operator is handed them (fp32).  int: d beta exact."""
    g = np.where(mask, dy.astype(f64), 0.0)
    xh = (x.astype(f64) - mean.astype(f64)) * rstd.astype(f64)
    M = dy.shape[0]
    s1, s2 = g.sum(0), (g * xh).sum(0)
    r = 1 if rounded else 0
    b1 = np.zeros_like(s1) if kind == "int" else _sum_bound(s1, np.abs(g).sum(0), M, r)
    return {"dbeta": (s1, b1), "dgamma": (s2, (2 + r) * U * np.abs(g * xh).sum(0) + M * D * np.abs(g * xh).sum(0))}


def bn_backward_dx(dy, x, mean, rstd, gamma, mask, sum_g, sum_gx, count):
    g = np.where(mask, dy.astype(f64), 0.0)
    x, mean, rstd, gamma = (v.astype(f64) for v in (x, mean, rstd, gamma))
    xh = (x - mean) * rstd
    sg, p = sum_g.astype(f64) / count, xh * (sum_gx.astype(f64) / count)
    return gamma * rstd * (g - sg - p), 8 * U * np.abs(gamma * rstd) * (np.abs(g) + np.abs(sg) + np.abs(p))


def bn_backward_fp32(dy, x, mean, rstd, gamma, y_act=None, a=None, b=None, mutant=None, y_out=None):
    """{"dbeta", "dgamma", "dx"} as the kernels form them.  mutants: "mask_from_y" (the mask of the _x forms taken from the forward's
    output y_out = act(x) + residual where it is fma(x, a, b) > 0), "mask_from_x" (x > 0), "no_mask", "fp32_accumulate", "last_row"
    (missing from both sums, dx's last row not written)"""
    if mutant == "no_mask":
        mask = np.ones(dy.shape, bool)
    elif mutant == "mask_from_y":
        mask = y_out > 0
    elif mutant == "mask_from_x" and a is not None:
        mask = x > 0
    elif y_act is not None:
        mask = y_act > 0
    else:
        mask = act32(x, a, b, 0) > 0 if a is not None else np.ones(dy.shape, bool)
    g = np.where(mask, dy, f32(0))
    xh = (x - mean) * rstd
    gs, ps = (g[:-1], (g.astype(f64) * xh.astype(f64))[:-1]) if mutant == "last_row" else (g, g.astype(f64) * xh.astype(f64))
    if mutant == "fp32_accumulate":
        s1, s2 = np.cumsum(gs, axis=0, dtype=f32)[-1], np.cumsum(ps.astype(f32), axis=0, dtype=f32)[-1]
    else:
        s1, s2 = gs.astype(f64).sum(0).astype(f32), ps.sum(0).astype(f32)
    inv_m = f32(1.0 / dy.shape[0])
    dx = gamma * rstd * (g - s1 * inv_m - xh * (s2 * inv_m))
    return {"dbeta": s1, "dgamma": s2, "dx": _drop(dx, "last_row" if mutant == "last_row" else None)}


# ---------------------------------------------------------------------------------------------------------------------------
# pointwise forward with statistics: y = act(x) w^T by pw_stat_kernel (the GEMM bound, + 1 rounding of act: |x'| carries u, inside the
# + 4), sums = [sum y | sum y^2] in float64 FROM THE RETURNED y: per pass a lane adds its two rows' values, a 16-lane butterfly the
# wave's 32 rows, all in fp32 (depth 5), the rest in float64: sum y 6 u sum |y|; the squares round once more: 7 u sum y^2.
# dw_stat_kernel: a thread adds its strip's <= 4 rows in fp32 (depth 3): 4 u sum |y|, 5 u sum y^2.


def pw_forward_stats(x, w, a=None, b=None, relu=0):
    xa, w = act64(x, a, b, relu), w.astype(f64)
    return xa @ w.T, _gemm_bound(x.shape[1], np.abs(xa) @ np.abs(w).T)


def stats_sums(y_got, depth, kind="gauss"):
    y = y_got.astype(f64)
    M = y.shape[0]
    s1, s2 = y.sum(0), (y * y).sum(0)
    b1 = np.zeros_like(s1) if kind == "int" else (depth + 1) * U * np.abs(y).sum(0) + M * D * np.abs(y).sum(0)
    return np.stack([s1, s2]), np.stack([b1, (depth + 2) * U * s2 + M * D * s2])


def stats_groups(y, rows):
    """y's rows in the groups one fp32 partial adds, zero-padded: (groups, rows, C).  pw_stat_kernel: a wave's 32 consecutive rows of y
    (M, N); dw_stat_kernel: the <= 4 output rows of a thread's strip of y (B, Ho, Wo, C)"""
    if y.ndim == 2:
        pad = -y.shape[0] % rows
        return np.pad(y, ((0, pad), (0, 0))).reshape(-1, rows, y.shape[1])
    B, Ho, Wo, C = y.shape
    yp = np.pad(y, ((0, 0), (0, -Ho % rows), (0, 0), (0, 0)))
    return np.ascontiguousarray(yp.reshape(B, -1, rows, Wo, C).transpose(0, 1, 3, 2, 4)).reshape(-1, rows, C)


def stats_sums_fp32(groups, mutant=None):
    """[sum y | sum y^2] as the producers form them: per group in fp32 — 32 rows: rows r and r + 16 first (a lane's two values), then the
    16-lane butterfly; 4 rows: in order — the groups in float64.  mutant "fp32_accumulate": every group sum added in ONE fp32 chain"""
    def partial(v):
        if v.shape[1] == 32:
            v = v[:, :16] + v[:, 16:]
            for step in (8, 4, 2, 1):
                v = v[:, :step] + v[:, step:2 * step]
            return v[:, 0]
        out = v[:, 0]
        for r in range(1, v.shape[1]):
            out = out + v[:, r]
        return out
    p1, p2 = partial(groups), partial(groups * groups)
    if mutant == "fp32_accumulate":
        return np.stack([np.cumsum(p1, axis=0, dtype=f32)[-1], np.cumsum(p2, axis=0, dtype=f32)[-1]]).astype(f64)
    return np.stack([p1.astype(f64).sum(0), p2.astype(f64).sum(0)])


# ---------------------------------------------------------------------------------------------------------------------------
# depthwise k x k, stride s, zero padding k / 2 of the ACTIVATION; taps [k k][C], tap t = ky k + kx.
#   forward (dw_conv_kernel, dw_stat_kernel): acc = bias, then one fma per tap, in order: k k + 1 terms in one chain:
#       (k k + 2) u (sum |x'| |w| + |bias|) (+ 1 for act's rounding, + 1 spare);
#   input gradient (dw_dgrad_kernel): at most k k products in one chain: (k k + 2) u sum |dy| |w|;
#   weight gradient (dw_wgrad_kernel): a workgroup takes `rows` output pixels (col_rows_per_block), R = 256 / (C / 4) pixel lanes; a lane
#       adds its pixels (or its runs of T pixels) in one fp32 chain of at most ceil(rows / R) + T terms, the R lanes are added in order
#       (R - 1), the workgroups by slice_sum_kernel as above; + 1 for act, + 3 spare.


def _taps(k):
    return [(ky, kx) for ky in range(k) for kx in range(k)]


def _pad(x, k):
    p = k // 2
    return np.pad(x, ((0, 0), (p, p), (p, p), (0, 0)))


def dw_forward(x, w, bias, k, stride, a=None, b=None, relu=0, kind="gauss", wrap=False):
    """x (B, H, W, C) -> (B, Ho, Wo, C).  wrap: the mutant whose taps above / below an image read the neighbouring image's rows"""
    B, H, W, C = x.shape
    Ho, Wo = H // stride, W // stride
    xa = act64(x, a, b, relu)
    w = w.astype(f64)
    if wrap:
        tall = _pad(xa.reshape(1, B * H, W, C), k)
        xp = np.stack([tall[0, i * H:i * H + H + 2 * (k // 2)] for i in range(B)])
    else:
        xp = _pad(xa, k)
    bias64 = np.zeros(C) if bias is None else bias.astype(f64)
    y, absy = np.zeros((B, Ho, Wo, C)) + bias64, np.zeros((B, Ho, Wo, C)) + np.abs(bias64)
    for t, (ky, kx) in enumerate(_taps(k)):
        v = xp[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride]
        y += v * w[t]
        absy += np.abs(v * w[t])
    return y, (np.zeros_like(y) if kind == "int" else (k * k + 4) * U * absy)


def dw_backward_data(dy, w, H, W, k, stride, kind="gauss"):
    B, Ho, Wo, C = dy.shape
    p = k // 2
    dy64, w = dy.astype(f64), w.astype(f64)
    dxp, absp = np.zeros((B, H + 2 * p, W + 2 * p, C)), np.zeros((B, H + 2 * p, W + 2 * p, C))
    for t, (ky, kx) in enumerate(_taps(k)):
        dxp[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride] += dy64 * w[t]
        absp[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride] += np.abs(dy64 * w[t])
    dx, ab = dxp[:, p:p + H, p:p + W], absp[:, p:p + H, p:p + W]
    return dx, (np.zeros_like(dx) if kind == "int" else (k * k + 2) * U * ab)


def dw_wgrad_depth(rows, workgroups, C, stride):
    R = 256 // (C // 4)
    T = 8 if stride == 1 else 4
    chain = (-(-workgroups // 16) - 1 + 15) if workgroups >= 64 else workgroups - 1
    return -(-rows // R) + T + (R - 1) + chain + 1 + 3


def dw_backward_weight(dy, x, k, stride, a=None, b=None, relu=0, plan=None, kind="gauss"):
    """plan = (wgrad_rows, wgrad_workgroups) of fear_layer_plan_info"""
    B, Ho, Wo, C = dy.shape
    xp, dy64 = _pad(act64(x, a, b, relu), k), dy.astype(f64)
    ref, ab = np.zeros((k * k, C)), np.zeros((k * k, C))
    for t, (ky, kx) in enumerate(_taps(k)):
        v = xp[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride] * dy64
        ref[t], ab[t] = v.sum((0, 1, 2)), np.abs(v).sum((0, 1, 2))
    return ref, (np.zeros_like(ref) if kind == "int" else dw_wgrad_depth(plan[0], plan[1], C, stride) * U * ab)


def dw_forward_fp32(x, w, bias, k, stride, a=None, b=None, relu=0, mutant=None):
    """mutants: "tap_wraps", "ho_wo_swapped" (the output indexed (ox, oy)), "no_bias", "pad_is_act_of_zero" (the padding is act(0) = max(b, 0),
    not zero), "last_row", "last_quad" """
    B, H, W, C = x.shape
    Ho, Wo = H // stride, W // stride
    xa = act32(x, a, b, relu)
    if mutant == "tap_wraps":
        tall = _pad(xa.reshape(1, B * H, W, C), k)
        xp = np.stack([tall[0, i * H:i * H + H + 2 * (k // 2)] for i in range(B)])
    elif mutant == "pad_is_act_of_zero" and a is not None:
        xp = _pad(xa - act32(np.zeros_like(x), a, b, relu), k) + act32(np.zeros((1, 1, 1, C), f32), a, b, relu)
    else:
        xp = _pad(xa, k)
    y = np.zeros((B, Ho, Wo, C), f32)
    if bias is not None and mutant != "no_bias":
        y = y + bias
    for t, (ky, kx) in enumerate(_taps(k)):
        y = y + xp[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride] * w[t]
    if mutant == "ho_wo_swapped":
        y = np.ascontiguousarray(y.transpose(0, 2, 1, 3)).reshape(B, Ho, Wo, C)
    return _drop(y.reshape(B * Ho * Wo, C), mutant).reshape(B, Ho, Wo, C)


def dw_backward_data_fp32(dy, w, H, W, k, stride, mutant=None):
    """mutants: "tap_wraps" (a gradient row of the neighbouring image is gathered), "last_row", "last_quad" """
    B, Ho, Wo, C = dy.shape
    p = k // 2
    if mutant == "tap_wraps":
        tall = dw_backward_data_fp32(dy.reshape(1, B * Ho, Wo, C), w, B * H, W, k, stride)
        return tall.reshape(B, H, W, C)
    dxp = np.zeros((B, H + 2 * p, W + 2 * p, C), f32)
    for t, (ky, kx) in enumerate(_taps(k)):
        dxp[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride] += dy * w[t]
    dx = np.ascontiguousarray(dxp[:, p:p + H, p:p + W])
    return _drop(dx.reshape(B * H * W, C), mutant).reshape(B, H, W, C)


def dw_backward_weight_fp32(dy, x, k, stride, a=None, b=None, relu=0, plan=None, mutant=None):
    """per workgroup of plan[0] output pixels an fp32 sum (numpy's pairwise order: no longer a chain than the kernel's), the workgroups in
    slice_sum_kernel's order.  mutants: "tap_wraps", "last_row" (the last output pixel missing), "mask_from_x", "last_quad" """
    B, Ho, Wo, C = dy.shape
    H, W = x.shape[1:3]
    if mutant == "mask_from_x" and a is not None and relu:
        xa = np.where(x > 0, act32(x, a, b, 0), f32(0))
    else:
        xa = act32(x, a, b, relu)
    if mutant == "tap_wraps":
        tall = _pad(xa.reshape(1, B * H, W, C), k)
        xp = np.stack([tall[0, i * H:i * H + H + 2 * (k // 2)] for i in range(B)])
    else:
        xp = _pad(xa, k)
    g = dy.copy()
    if mutant == "last_row":
        g[-1, -1, -1] = 0
    rows = plan[0]
    parts = [np.zeros((k * k, C), f32) for _ in range(plan[1])]
    for t, (ky, kx) in enumerate(_taps(k)):
        v = (xp[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride] * g).reshape(-1, C)
        for i in range(plan[1]):
            parts[i][t] = v[i * rows:(i + 1) * rows].sum(0, dtype=f32)
    return _drop(slice_sum_fp32(parts), "last_quad" if mutant == "last_quad" else None)


# ---------------------------------------------------------------------------------------------------------------------------
# fear_stem_im2col: a gather, exact.  rows of 28: k = (ci 3 + ky) 3 + kx of the 3 x 3 stride-2 pad-1 window, column 27 zero


def stem_im2col(x_nchw, mutant=None):
    """mutants: "ho_wo_swapped" (the pixel index decoded with H / 2 and W / 2 traded), "no_zero_column" (column 27 left as it was: -1)"""
    n, _, H, W = x_nchw.shape
    Ho, Wo = H // 2, W // 2
    xp = np.pad(x_nchw, ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = np.full((n, Ho, Wo, 28), -1.0 if mutant == "no_zero_column" else 0.0, x_nchw.dtype)
    for ci in range(3):
        for ky in range(3):
            for kx in range(3):
                out[..., (ci * 3 + ky) * 3 + kx] = xp[:, ci, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]
    if mutant == "ho_wo_swapped":
        out = np.ascontiguousarray(out.transpose(0, 2, 1, 3))
    return out.reshape(n * Ho * Wo, 28)


def int_headroom(*abs_products):
    """the largest sum |a||b| over the output elements of the given |A| |B| arrays: must stay below 2^24 for the integer form"""
    return max(float(np.max(p)) for p in abs_products)
