"""Float64 references of the head-side training operators (include/fear_train.h: fear_xcorr_forward / _backward,
fear_exp_head_forward / _backward, fear_head_loss) with an element-wise error bound each, the seeded inputs of their tests, and an
fp32 numpy evaluation of the same formulas that can be broken on purpose.  A helper module (not collected), shared by
tests/test_train_head_ops_gpu.py (the kernels against reference and bound) and tests/test_head_ops_reference_cpu.py (the fp32
evaluation fits the bound, every `mutant` leaves it).

Every reference function returns (reference, bound) pairs; a result `got` passes where |got - reference| <= bound element-wise.
The bounds are derived from the arithmetic the kernels are written in, never from what they return.  u = 2^-24 is the unit
roundoff of fp32 (half an ulp): one correctly rounded operation errs by at most u relative."""
import numpy as np
import torch

U = 2.0 ** -24

XCORR_FWD_CASES = [(3, 256, 256, 64), (5, 32, 64, 16), (3, 96, 8, 4), (2, 160, 256, 36), (1, 32, 4, 4)]      # (B, P, C, J)
XCORR_BWD_CASES = [(3, 256, 256, 64), (2, 128, 64, 16), (1, 384, 8, 4)]
EXP_M = [1, 255, 257, 1000]
EXP_ADJUST = [1.0, 0.37]
LOSS_M = [1, 255, 257, 1000, 70001]
LOSS_COEFS = [(1.0, 1.0), (0.7, 2.5)]
LOSS_VARIANTS = ["npos0", "npos1", "npos2", "nneg0", "nneg1", "nreg0"]      # selections of no / one / two cells, run at M = 1000

f32, f64 = np.float32, np.float64


def excess(got, ref, bound):
    """max over the elements of |got - ref| / bound (0 / 0 counts as 0: an exact result under a zero bound)"""
    err = np.abs(np.asarray(got, f64) - np.asarray(ref, f64))
    bound = np.broadcast_to(np.asarray(bound, f64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(np.max(q)) if q.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# MobileCorrelation: s[b][p][j] = sum_c x[b][p][c] z[b][c][j] and its two gradients
#
# Bound of a GEMM-shaped output: (2 K + 4) u (|A| @ |B| + |add|), K = the contraction length.  ANY order of adding K rounded fp32
# products obeys gamma_K = K u / (1 - K u) times sum |a_k b_k| (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5), fused
# multiply-adds included; the factor 2 is there because v_mfma_f32_16x16x4_f32 does not specify how it rounds inside its group of 4
# terms (the kernels use that instruction alone, and the build has no fast-math flag); + 4 covers the addition of `add`, the sum of
# the four waves' partial tiles (weight gradient) and the 1 / (1 - K u) of gamma_K for every K here (K <= 384).  A single missing
# or foreign term is ~ 1 / (K u) times larger than this, so the bound tells a wrong tile from a right one.


def xcorr_inputs(B, P, C, J, seed=0):
    """x (B, P, C), z (B, C, J): every crop its own z; ds (B, P, J), add (B, P, C) for the backward"""
    rng = np.random.default_rng(1000 + seed)
    return {"x": rng.standard_normal((B, P, C)).astype(f32), "z": rng.standard_normal((B, C, J)).astype(f32),
            "ds": rng.standard_normal((B, P, J)).astype(f32), "add": rng.standard_normal((B, P, C)).astype(f32)}


def _gemm_bound(K, absprod, absadd=0.0):
    return (2 * K + 4) * U * (absprod + absadd)


def xcorr_forward(x, z):
    x, z = x.astype(f64), z.astype(f64)
    return np.matmul(x, z), _gemm_bound(x.shape[2], np.matmul(np.abs(x), np.abs(z)))


def xcorr_backward(ds, x, z, add=None):
    """{"dx": (ref, bound), "dz": (ref, bound)}: dx = add + ds z^T (contraction J), dz = x^T ds (contraction P)"""
    ds, x, z = ds.astype(f64), x.astype(f64), z.astype(f64)
    a = np.zeros_like(x) if add is None else add.astype(f64)
    zt, xt = z.transpose(0, 2, 1), x.transpose(0, 2, 1)
    return {"dx": (a + np.matmul(ds, zt), _gemm_bound(ds.shape[2], np.matmul(np.abs(ds), np.abs(zt)), np.abs(a))),
            "dz": (np.matmul(xt, ds), _gemm_bound(x.shape[1], np.matmul(np.abs(xt), np.abs(ds))))}


def _straddled_second_groups(B, P):
    """rows of the second 32-row group of every 128-row tile that holds rows of more than one crop"""
    rows = []
    for t0 in range(0, B * P, 128):
        t1 = min(t0 + 128, B * P)
        if t0 // P != (t1 - 1) // P and t0 + 32 < t1:
            rows.append((t0 + 32, min(t0 + 64, t1)))
    return rows


def xcorr_forward_fp32(x, z, mutant=None):
    """the forward in fp32 numpy.  mutants: "crop_stride" (the second 32-row group of a tile that straddles crops reads the NEXT
    crop's z), "last_row" (the last row is never written), "z_transposed" (z[b] read as (J, C))"""
    B, P, C = x.shape
    J = z.shape[2]
    if mutant == "z_transposed":
        z = np.ascontiguousarray(z.reshape(B, J, C).transpose(0, 2, 1))
    s = np.matmul(x, z).reshape(B * P, J)
    if mutant == "crop_stride":
        xr = x.reshape(B * P, C)
        for r0, r1 in _straddled_second_groups(B, P):
            s[r0:r1] = xr[r0:r1] @ z[(r0 // P + 1) % B]
    if mutant == "last_row":
        s[-1] = 0
    return s.reshape(B, P, J)


def xcorr_backward_fp32(ds, x, z, add=None, mutant=None):
    """mutants: "no_add" (dx_add not added), "last_row" (dx's last row never written, the last row missing from dz's sum)
    and "z_transposed".  Returns {"dx", "dz"}."""
    B, P, C = x.shape
    J = z.shape[2]
    zz = np.ascontiguousarray(z.reshape(B, J, C).transpose(0, 2, 1)) if mutant == "z_transposed" else z
    dx = np.matmul(ds, zz.transpose(0, 2, 1))
    if add is not None and mutant != "no_add":
        dx = dx + add
    xs, dss = x, ds
    if mutant == "last_row":
        dx[-1, -1] = 0
        xs = x.copy()
        xs[-1, -1] = 0
    return {"dx": dx, "dz": np.matmul(xs.transpose(0, 2, 1), dss)}


# ---------------------------------------------------------------------------------------------------------------------------
# Box head: bbox = exp(adjust * p + bias[c]); dp = dbbox * bbox * adjust, d bias[c] = sum_m dbbox * bbox, d adjust = sum dbbox * bbox * p

BIAS4 = np.array([0.5, -1.0, 2.0, -0.25], f32)


def exp_inputs(M, adjust, seed=0):
    """p such that adjust * p + bias covers [-20, 12] (the first cell sits at -20 and, where M > 1, one at 12);
    an fp32 bbox drawn independently of p (the backward takes bbox as an input); a signed dbbox whose four column sums of
    dbbox * bbox * p have the signs + - + - (so that d adjust, their sum, cancels)"""
    rng = np.random.default_rng(2000 + seed + M)
    a = rng.uniform(-20.0, 12.0, (M, 4))
    a.reshape(-1)[0] = -20.0
    if M > 1:
        a.reshape(-1)[5] = 12.0
    s = f32(adjust)
    p = ((a - BIAS4.astype(f64)) / f64(s)).astype(f32)
    bbox = np.exp(rng.uniform(-3.0, 3.0, (M, 4))).astype(f32)
    flip = rng.random((M, 4)) < 0.2
    flip[0] = False
    sign = np.sign(p.astype(f64)) * np.array([1.0, -1.0, 1.0, -1.0]) * np.where(flip, -1.0, 1.0)
    dbbox = (np.abs(rng.standard_normal((M, 4))) + 0.1) * sign
    return {"p": p, "adjust": np.array([s], f32), "bias4": BIAS4.copy(), "bbox": bbox, "dbbox": dbbox.astype(f32)}


def exp_forward(p, adjust, bias4):
    """Relative bound u (|s p| + |s p + b|) + 4 u.  The argument is fl(fl(s p) + b) or one fused multiply-add: its absolute error is at
    most u |s p| + u |s p + b| (first order), which is the relative error it leaves in exp(.); expf itself is documented at 1 ulp = 2 u
    in HIP's math API table (no ROCm document installed with the toolchain states another figure), taken twice: 4 u.  |s p + b| <= 20
    here, so the second-order term of the argument's error (4e-12) is far inside that margin."""
    sp = f64(adjust[0]) * p.astype(f64)
    arg = sp + bias4.astype(f64)
    ref = np.exp(arg)
    return ref, ref * (U * (np.abs(sp) + np.abs(arg)) + 4 * U)


def exp_backward(p, adjust, bbox, dbbox):
    """{"dp", "dbias4", "dadjust"}: (ref, bound) each, float64 of the fp32 inputs.
    dp = (dbbox * bbox) * adjust: two rounded products, (1 + u)^2 - 1 < 3 u relative.
    The two sums: bound (n + 3) u sum |terms|, n = the longest chain of fp32 additions an output passes through.
      d bias4: n = 0.  exp_head_bwd_kernel stores T = fl(dbbox * bbox) (one rounding per term); col_reduce_kernel<2> adds the rows in
               float64 (`s1 += to_f64(v)`, the lane sums `s1 += red[0][...]` and the partial rows are double), col_finalize_kernel
               adds the partials in double (`s1 += a.partial[...]`, `s1 += red[0][l][cl]`) and rounds once, `a.out1[c] = (float)s1`:
               2 u in all, inside 3 u.
      d adjust: n = 2.  U = fl(fl(dbbox * bbox) * p) (two roundings per term), the same float64 column sums rounded to fp32 once per
               column, then sum4_kernel's `(in[0] + in[1]) + (in[2] + in[3])`: every column sum passes through two fp32 additions.
               (2 + 1 + 2) u = (n + 3) u.
    The bound is on sum |terms|, not on the result: d adjust cancels by construction of the inputs."""
    p, bbox, dbbox, s = p.astype(f64), bbox.astype(f64), dbbox.astype(f64), f64(adjust[0])
    t = dbbox * bbox
    dp = t * s
    return {"dp": (dp, 3 * U * np.abs(dp)),
            "dbias4": (t.sum(0), (0 + 3) * U * np.abs(t).sum(0)),
            "dadjust": (np.array([(t * p).sum()]), np.array([(2 + 3) * U * np.abs(t * p).sum()]))}


def _exp32(x):
    """an fp32 exp of at most 1/2 ulp error: float64 exp, rounded (numpy's own float32 exp is looser than HIP's 1 ulp)"""
    with np.errstate(over="ignore"):
        return np.exp(x.astype(f64)).astype(f32)


def exp_forward_fp32(p, adjust, bias4, mutant=None):
    """mutant "last_row": the last row is never written"""
    out = _exp32(adjust[0] * p + bias4)
    if mutant == "last_row":
        out[-1] = 0
    return out


def exp_backward_fp32(p, adjust, bbox, dbbox, mutant=None):
    """the kernels' arithmetic: fp32 products, float64 column sums rounded once, sum4 in fp32.  mutants: "no_adjust" (dp without
    the factor adjust), "three_columns" (d adjust from three of the four column sums), "last_row" (the last row missing from
    both sums)"""
    t = dbbox * bbox
    u = t * p
    dp = t if mutant == "no_adjust" else t * adjust[0]
    ts, us = (t[:-1], u[:-1]) if mutant == "last_row" else (t, u)
    dbias4 = ts.astype(f64).sum(0).astype(f32)
    u4 = us.astype(f64).sum(0).astype(f32)
    dadjust = (u4[0] + u4[1]) + u4[2] if mutant == "three_columns" else (u4[0] + u4[1]) + (u4[2] + u4[3])
    return {"dp": dp, "dbias4": dbias4, "dadjust": np.array([dadjust], f32)}


# ---------------------------------------------------------------------------------------------------------------------------
# FEARLoss


def loss_inputs(M, variant=None, seed=0):
    """bbox / gt_reg rows of 4, cls / gt_cls / gt_weight per cell.  Labels from {1, 0, -1} (-1: ignored); weights zero on cells
    [256, 600) where M >= 1000 and on [0, 256) at M = 257 (a whole 256-cell block without a weighted cell); three weighted cells
    with bbox == gt_reg exactly in one, two and four coordinates (fewer cells: as many as there are); logits +-30 and +-100 under
    both labels.  `variant` thins a selection: "npos0/1/2", "nneg0/1", "nreg0"."""
    rng = np.random.default_rng(3000 + seed + M)
    bbox = np.exp(rng.uniform(-1.0, 4.0, (M, 4))).astype(f32)
    gt_reg = rng.uniform(1.0, 60.0, (M, 4)).astype(f32)
    cls = (3.0 * rng.standard_normal(M)).astype(f32)
    gt_cls = rng.choice(np.array([1.0, 0.0, -1.0], f32), M, p=[0.3, 0.4, 0.3]).astype(f32)
    gt_w = np.where(rng.random(M) > 0.6, rng.choice(np.array([1.0, 0.25], f32), M), 0.0).astype(f32)
    if M >= 16:
        cls[:8] = [30.0, -30.0, 100.0, -100.0, 30.0, -30.0, 100.0, -100.0]
        gt_cls[:8] = [1, 1, 1, 1, 0, 0, 0, 0]
    if M >= 1000:
        gt_w[256:600] = 0
    elif M > 256:
        gt_w[:256] = 0
    gt_w[M - 1] = 1.0                                    # the tail block always has a weighted cell
    if M > 2:
        gt_cls[M - 1], gt_cls[M - 2] = 1.0, 0.0          # ... a positive and a negative one
    if variant and variant.startswith("npos"):
        pos = np.flatnonzero(gt_cls == 1)
        gt_cls[pos[:len(pos) - int(variant[4:])]] = -1.0            # the LAST cells stay: ordinary logits, not the saturated ones
    if variant and variant.startswith("nneg"):
        neg = np.flatnonzero(gt_cls == 0)
        gt_cls[neg[:len(neg) - int(variant[4:])]] = -1.0
    if variant == "nreg0":
        gt_w[:] = 0
    weighted = np.flatnonzero(gt_w > 0)
    for cell, coords in zip(weighted[:3], ([1, 3], [2], [0, 1, 2, 3]) if len(weighted) < 3 else ([2], [1, 3], [0, 1, 2, 3])):
        bbox[cell, coords] = gt_reg[cell, coords]
    return {"bbox": bbox, "cls": cls, "gt_reg": gt_reg, "gt_cls": gt_cls, "gt_weight": gt_w}


def loss_reference(bbox, cls, gt_reg, gt_cls, gt_weight, coef_cls, coef_reg):
    """oracle.fear_train_oracle.fear_loss (pinned to the reference's FEARLoss fixtures) in float64 under autograd, the coefficients at
    their fp32 values (the ABI takes floats).  Returns {"losses", "dcls", "dbbox"}: (ref, bound) each, plus "ignored" (cells whose
    label is neither 0 nor 1: their dcls must be exactly 0) and "unweighted" (dbbox exactly 0).

    An EMPTY selection is NaN in torch; the operator's stated deviation (include/fear_train.h) is 0 for that half.  The oracle is
    still the reference: two padding cells that are exactly right are appended for an empty selection — label 1 with logit +1000,
    label 0 with logit -1000 (BCE = 0 and sigmoid - label = 0 exactly in float64), weight 1 with bbox == gt_reg (IoU term 0) — so the
    half is the mean of zeros = the deviation's 0, and no real cell belongs to it.

    Bounds.  Losses: relative (256 + 16) u — the terms are non-negative, each block adds its 256 in one serial fp32 chain
    (loss_partial_kernel: gamma_255), the block sums are added in float64 (loss_finalize_kernel); 16 u for the terms' own arithmetic
    (expf, log1pf, the IoU quotient) and the final rounding.
    dcls: ABSOLUTE 4 u * 0.5 coef_cls / n_sel (sigma(x) - 1 cancels near sigma = 1, so no relative bound exists): sigma in [0, 1] carries
    at most 2 u absolute, the product and the quotient one rounding each of a value <= 0.5 coef_cls / n_sel.
    dbbox: R u * sc * (|dI| (U+1) + (I+1) (|dPa| + |dI|)) / (U+1)^2 with sc = coef_reg / n_reg and R = 21, the fp32 operations that round on
    the way to one output in loss_grad_kernel as written: pw, ph (2); ta (3); pa (1); wi, hi (2); inter (1); uni (2); uni + 1 (1);
    den (1); sc (1); dI * (uni + 1) (1); inter + 1 (1); dPa - dI (1); their product (1); the difference (1); -sc * (1); / den (1).
    (min and the tie factor 1 / 0.5 / 0 are exact.)"""
    from oracle.fear_train_oracle import fear_loss
    M = cls.shape[0]
    cc, cr = f64(f32(coef_cls)), f64(f32(coef_reg))
    lab, w = gt_cls.astype(f64), gt_weight.astype(f64)
    n_pos, n_neg, n_reg = int((lab == 1).sum()), int((lab == 0).sum()), int((w > 0).sum())
    pads = []           # (bbox row, logit, gt_reg row, label, weight)
    one = [1.0, 1.0, 1.0, 1.0]
    if n_pos == 0:
        pads += [(one, 1000.0, [2.0] * 4, 1.0, 0.0)] * 2
    if n_neg == 0:
        pads += [(one, -1000.0, [2.0] * 4, 0.0, 0.0)] * 2
    if n_reg == 0:
        pads += [(one, 0.0, one, -1.0, 1.0)]
    cat = lambda a, col: np.concatenate([a.astype(f64), np.array([p[col] for p in pads], f64).reshape((len(pads),) + a.shape[1:])]) if pads else a.astype(f64)
    b = torch.from_numpy(cat(bbox, 0)).requires_grad_(True)
    c = torch.from_numpy(cat(cls, 1)).requires_grad_(True)
    n = M + len(pads)
    nchw = lambda t: t.t().reshape(1, 4, n, 1)
    lc, lr = fear_loss(nchw(b), c.reshape(1, 1, n, 1), nchw(torch.from_numpy(cat(gt_reg, 2))), torch.from_numpy(cat(gt_cls, 3)).reshape(1, 1, n, 1),
                       torch.from_numpy(cat(gt_weight, 4)).reshape(1, n, 1), float(cc), float(cr))
    (lc + lr).backward()
    losses = np.array([float(lc.detach()), float(lr.detach())])
    assert np.isfinite(losses).all()
    dcls = np.zeros(M) if c.grad is None else c.grad.numpy()[:M]        # (both halves single cells: constants, no gradient)
    dbbox = b.grad.numpy()[:M]
    n_sel = np.where(lab == 1, max(n_pos, 1), max(n_neg, 1)).astype(f64)
    p, t = bbox.astype(f64), gt_reg.astype(f64)
    pw, ph = p[:, 0] + p[:, 2], p[:, 1] + p[:, 3]
    wi = np.minimum(p[:, 0], t[:, 0]) + np.minimum(p[:, 2], t[:, 2])
    hi = np.minimum(p[:, 3], t[:, 3]) + np.minimum(p[:, 1], t[:, 1])
    I = wi * hi
    Un = (t[:, 0] + t[:, 2]) * (t[:, 1] + t[:, 3]) + pw * ph - I
    dmin = np.where(p < t, 1.0, np.where(p == t, 0.5, 0.0))
    dI = dmin * np.stack([hi, wi, hi, wi], 1)
    dPa = np.stack([ph, pw, ph, pw], 1)
    sc = cr / max(n_reg, 1)
    bb = 21 * U * sc * (np.abs(dI) * (Un + 1)[:, None] + (I + 1)[:, None] * (np.abs(dPa) + np.abs(dI))) / ((Un + 1) ** 2)[:, None]
    return {"losses": (losses, (256 + 16) * U * np.abs(losses)),
            "dcls": (dcls, 4 * U * 0.5 * cc / n_sel),
            "dbbox": (dbbox, np.where((w > 0)[:, None], bb, 0.0)),
            "ignored": (lab != 1) & (lab != 0), "unweighted": ~(w > 0), "counts": (n_pos, n_neg, n_reg)}


def loss_fp32(bbox, cls, gt_reg, gt_cls, gt_weight, coef_cls, coef_reg, mutant=None):
    """The three kernels of fear_head_loss restated in fp32 numpy: per-cell terms in fp32, 256 cells per block added serially in fp32,
    block sums in float64, gradients in fp32.  mutants: "ignored_negative" (a label that is neither 0 nor 1 counts as 0),
    "single_cell" (a selection of exactly one cell is not dropped: n > 0 where the reference has n > 1), "tie_one" / "tie_zero" (the
    gradient of min at p == t), "no_coef_reg", "tail_block" (the cells of a ragged last block are not summed)."""
    M = cls.shape[0]
    cc, cr = f32(coef_cls), f32(coef_reg)
    one, half = f32(1), f32(0.5)
    x, y = cls, gt_cls.copy()
    if mutant == "ignored_negative":
        y[y != 1] = 0
    pos, neg, wsel = y == 1, y == 0, gt_weight > 0
    bce = np.maximum(x, f32(0)) - x * y + np.log1p(_exp32(-np.abs(x)).astype(f64)).astype(f32)
    p, t = bbox, gt_reg
    pw, ph = p[:, 0] + p[:, 2], p[:, 1] + p[:, 3]
    ta, pa = (t[:, 0] + t[:, 2]) * (t[:, 1] + t[:, 3]), pw * ph
    wi = np.minimum(p[:, 0], t[:, 0]) + np.minimum(p[:, 2], t[:, 2])
    hi = np.minimum(p[:, 3], t[:, 3]) + np.minimum(p[:, 1], t[:, 1])
    inter = wi * hi
    uni = ta + pa - inter
    terms = np.stack([pos.astype(f32), neg.astype(f32), wsel.astype(f32), np.where(pos, bce, f32(0)), np.where(neg, bce, f32(0)),
                      np.where(wsel, one - (inter + one) / (uni + one), f32(0))], 1)
    blocks = (M + 255) // 256
    pad = np.zeros((blocks * 256, 6), f32)
    pad[:M] = terms
    if mutant == "tail_block" and M % 256:
        pad[(blocks - 1) * 256:] = 0
    s = np.cumsum(pad.reshape(blocks, 256, 6), axis=1, dtype=f32)[:, -1].astype(f64).sum(0)
    lone = 0 if mutant == "single_cell" else 1
    lp = s[3] / s[0] if s[0] > lone else 0.0
    ln = s[4] / s[1] if s[1] > lone else 0.0
    lr = s[5] / s[2] if s[2] > 0 else 0.0
    creg = one if mutant == "no_coef_reg" else cr
    losses = np.array([f32((0.5 * lp + 0.5 * ln) * f64(cc)), f32(lr * f64(creg))])
    n_pos, n_neg, n_reg = f32(s[0]), f32(s[1]), f32(s[2])
    sg = one / (one + _exp32(-x))
    with np.errstate(divide="ignore", invalid="ignore"):
        dpos = half * cc * (sg - one) / n_pos if n_pos > lone else np.zeros(M, f32)
        dneg = half * cc * sg / n_neg if n_neg > lone else np.zeros(M, f32)
        dcls = np.where(pos, dpos, np.where(neg, dneg, f32(0))).astype(f32)
        tie = {"tie_one": one, "tie_zero": f32(0)}.get(mutant, half)
        dmin = np.where(p < t, one, np.where(p == t, tie, f32(0))).astype(f32)
        dI = dmin * np.stack([hi, wi, hi, wi], 1)
        dPa = np.stack([ph, pw, ph, pw], 1)
        u1 = (uni + one)[:, None]
        den = u1 * u1
        sc = creg / n_reg
        o = -sc * (dI * u1 - (inter + one)[:, None] * (dPa - dI)) / den
    dbbox = np.where(wsel[:, None], o, f32(0)).astype(f32)
    return {"losses": losses, "dcls": dcls, "dbbox": dbbox}


# ---------------------------------------------------------------------------------------------------------------------------
# layout kernels, fear_scale_column, fear_add: copies or one fp32 operation — exact

LAYOUT_CASES = [(2, 256, 64, 256, 0), (3, 4, 256, 4, 0), (2, 4, 5, 12, 8), (1, 3, 7, 8, 4)]      # (n, C, HW, ld, ch_off)
ADD_N = [1, 3, 4, 5, 1023, 1025]
