"""Float64 references of the block-fused training operators with a BatchNorm inside (include/fear_train.h: fear_pwbn_train_*,
fear_stem_train_*, fear_sepbn_train_*), shared by tests/test_train_block.py (one rank), tests/test_train_syncbn.py (two played ranks
through the all-reduce hook) and tests/test_syncbn_reference_cpu.py:

  * `*_autograd`: torch autograd on the WHOLE batch — the reference every kernel test compares with;
  * `*_sync_inputs`: the inputs of the two-rank tests (rank 1's half is 1.5 x + 1.0 of its draw, so that the statistics of a half
    are far from the statistics of the batch);
  * `played_ranks`: SyncBatchNorm over ranks written out by hand — local float64 sums, their total, the finalize and the backward
    split torch.nn.SyncBatchNorm makes — with a `variant` argument that breaks it in one of the ways a wrong kernel finalize could:
    the CPU test shows that each of them leaves the whole-batch reference by far more than the kernel tests' tolerance.

Layout of every result: activations as rows [B * H * W][C] (NHWC), the keys `compare` understands."""
import torch
import torch.nn.functional as F

TOL = 2e-4          # the project's bound against float64 (tests/test_train_block.py)
MOMENTUM, EPS = 0.1, 1e-5


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rows(t):
    """(B, C, H, W) -> [B * H * W][C]"""
    return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def compare(ranks, ref):
    """Per-rank results against the whole-batch reference: `out` / `dx` of the ranks concatenated, parameter gradients (`d ...`)
    added up — what the gradient all-reduce of data-parallel training does, up to the division by the world size —, and the running
    statistics of EVERY rank against the whole batch's.  Keys a rank does not have (dx of an operator without one) are skipped."""
    errs = {}
    for k, v in ref.items():
        if v is None or ranks[0].get(k) is None:
            continue
        if k.startswith("running_"):
            for r, res in enumerate(ranks):
                errs[f"rank {r} {k}"] = rel(res[k], v)
        elif k.startswith("d "):
            errs[k] = rel(sum(res[k].detach().double().cpu() for res in ranks), v)
        else:
            errs[k] = rel(torch.cat([res[k].detach().double().cpu() for res in ranks]), v)
    return errs


def _leaf(t):
    return None if t is None else t.detach().clone().requires_grad_(True)


# ---------------------------------------------------------------------------------------------------------------------------
# whole-batch autograd


def pwbn_autograd(x, w, gamma, beta, relu, dy):
    """conv 1x1 as rows (M, K) @ (N, K)^T + BatchNorm [+ ReLU]"""
    x, w, gamma, beta = _leaf(x), _leaf(w), _leaf(gamma), _leaf(beta)
    M, N = x.shape[0], w.shape[0]
    rm, rv = torch.zeros(N, dtype=torch.float64), torch.ones(N, dtype=torch.float64)
    y = F.batch_norm((x @ w.t()).t().reshape(1, N, M, 1), rm, rv, gamma, beta, True, MOMENTUM, EPS).reshape(N, M).t()
    y = F.relu(y) if relu else y
    y.backward(dy)
    return {"out": y.detach(), "dx": x.grad, "d w": w.grad, "d gamma": gamma.grad, "d beta": beta.grad, "running_mean": rm, "running_var": rv}


def stem_autograd(x, w, gamma, beta, dy):
    """3x3 stride-2 conv 3 -> 16 on the NCHW image + BatchNorm + ReLU; dy as rows"""
    w, gamma, beta = _leaf(w), _leaf(gamma), _leaf(beta)
    rm, rv = torch.zeros(16, dtype=torch.float64), torch.ones(16, dtype=torch.float64)
    y = F.relu(F.batch_norm(F.conv2d(x, w, stride=2, padding=1), rm, rv, gamma, beta, True, MOMENTUM, EPS))
    n, _, Ho, Wo = y.shape
    y.backward(dy.reshape(n, Ho, Wo, 16).permute(0, 3, 1, 2))
    return {"out": rows(y), "d w": w.grad, "d gamma": gamma.grad, "d beta": beta.grad, "running_mean": rm, "running_var": rv}


def sepbn_autograd(x, taps, w, b_dw, b_pw, gamma, beta, dy):
    """SepConv (depthwise 3x3 taps [9][cin] + pointwise [cout][cin], biases or None) + BatchNorm + ReLU on NCHW x; dy as rows"""
    x, taps, w, b_dw, b_pw, gamma, beta = (_leaf(t) for t in (x, taps, w, b_dw, b_pw, gamma, beta))
    cin, cout = w.shape[1], w.shape[0]
    B, _, H, W = x.shape
    rm, rv = torch.zeros(cout, dtype=torch.float64), torch.ones(cout, dtype=torch.float64)
    d = F.conv2d(x, taps.t().reshape(cin, 1, 3, 3), b_dw, padding=1, groups=cin)
    y = F.relu(F.batch_norm(F.conv2d(d, w.view(cout, cin, 1, 1), b_pw), rm, rv, gamma, beta, True, MOMENTUM, EPS))
    y.backward(dy.reshape(B, H, W, cout).permute(0, 3, 1, 2))
    return {"out": rows(y), "d": rows(d), "dx": rows(x.grad), "d taps": taps.grad, "d w": w.grad, "d gamma": gamma.grad, "d beta": beta.grad,
            "running_mean": rm, "running_var": rv, "bias grads": None if b_pw is None else (b_dw.grad, b_pw.grad)}


# ---------------------------------------------------------------------------------------------------------------------------
# the two-rank cases and their inputs

# M (all ranks), K, N, relu, need_dx.  Forward GEMM per rank: 384 x 112 x 256 takes launch_gemm_lds (K >= 32, N >= 16:
# gemm_lds_applies), 1000 x 28 x 16 and 333 x 24 x 40 take pw_stat_kernel (K < 32); 333 rows are no multiple of the 128-row tile.
PWBN_SYNC_CASES = [(768, 112, 256, 0, True), (2000, 28, 16, 1, False), (666, 24, 40, 1, True)]
# n (all ranks), H, W: pw_stat_kernel<1, true> gathering its rows from the image
STEM_SYNC_CASES = [(4, 32, 32), (2, 24, 40)]
# B (all ranks), H, W, cin, cout, bias, ldx_pad, ldo_pad: cin >= 32 everywhere, so all three forwards take launch_gemm_lds
SEPBN_SYNC_CASES = [(4, 8, 8, 64, 48, False, 16, 0), (2, 16, 16, 320, 256, True, 0, 64), (2, 8, 24, 256, 256, True, 0, 0)]


def _skew_rank1(x):
    """rank 1's half of the leading dimension becomes 1.5 x + 1.0: local and global statistics far apart"""
    h = x.shape[0] // 2
    x = x.clone()
    x[h:] = 1.5 * x[h:] + 1.0
    return x


def _dy(g, *shape):
    # (a gradient with a mean: sum(g) / count is then no small term of the BatchNorm backward, and a wrong count shows)
    return torch.randn(*shape, generator=g, dtype=torch.float64) + 0.5


def pwbn_sync_inputs(M, K, N, relu, need_dx):
    g = torch.Generator().manual_seed(700 + K + N)
    R = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return {"x": _skew_rank1(R(M, K)), "w": R(N, K) * 0.3, "gamma": torch.rand(N, generator=g, dtype=torch.float64) + 0.5, "beta": R(N) * 0.3,
            "dy": _dy(g, M, N)}


def stem_sync_inputs(n, H, W):
    g = torch.Generator().manual_seed(720 + n + H + W)
    R = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return {"x": _skew_rank1(R(n, 3, H, W)), "w": R(16, 3, 3, 3) * 0.3, "gamma": torch.rand(16, generator=g, dtype=torch.float64) + 0.5,
            "beta": R(16) * 0.3, "dy": _dy(g, n * (H // 2) * (W // 2), 16)}


def sepbn_sync_inputs(B, H, W, cin, cout, bias, ldx_pad=0, ldo_pad=0):
    g = torch.Generator().manual_seed(740 + cin + cout + B + W)
    R = lambda *s, scale=1.0: torch.randn(*s, generator=g, dtype=torch.float64) * scale
    return {"x": _skew_rank1(R(B, cin, H, W)), "taps": R(9, cin, scale=0.4), "w": R(cout, cin, scale=(2.0 / cin) ** 0.5),
            "b_dw": R(cin, scale=0.3) if bias else None, "b_pw": R(cout, scale=0.3) if bias else None,
            "gamma": torch.rand(cout, generator=g, dtype=torch.float64) + 0.5, "beta": R(cout, scale=0.3), "dy": _dy(g, B * H * W, cout)}


def pwbn_sync_reference(inp, relu):
    return pwbn_autograd(inp["x"], inp["w"], inp["gamma"], inp["beta"], relu, inp["dy"])


def stem_sync_reference(inp):
    return stem_autograd(inp["x"], inp["w"], inp["gamma"], inp["beta"], inp["dy"])


def sepbn_sync_reference(inp):
    ref = sepbn_autograd(inp["x"], inp["taps"], inp["w"], inp["b_dw"], inp["b_pw"], inp["gamma"], inp["beta"], inp["dy"])
    return {k: v for k, v in ref.items() if k not in ("d", "bias grads")}


# ---------------------------------------------------------------------------------------------------------------------------
# SyncBatchNorm over played ranks by hand, right or wrong in a chosen way

VARIANTS = ("local_stats", "count_without_world", "dx_local_sums", "dgamma_dbeta_global", "no_bias_shift")


def played_ranks(pre_fn, x, params, gamma, beta, dy, relu, variant="correct", mean_shift=None, world=2):
    """`pre_fn(x_r, params_r)` -> the BatchNorm's input of one rank as rows (differentiable).  Returns one result dict per rank.
    variant: "correct", or
      local_stats          mean / variance from the rank's own rows
      count_without_world  the all-reduced sums with the LOCAL row count in the unbiased running variance and the backward's 1 / count
      dx_local_sums        the input gradient's coefficients from the rank's own (sum g, sum g xhat)
      dgamma_dbeta_global  d gamma / d beta from the all-reduced sums (the ranks' sum is then `world` times the truth)
      no_bias_shift        the running mean without `mean_shift` (the SepConv pointwise bias, which the kernels keep out of `raw`)"""
    assert variant == "correct" or variant in VARIANTS
    h = x.shape[0] // world
    xs = [_leaf(x[r * h:(r + 1) * h]) for r in range(world)]
    ps = [{k: _leaf(v) for k, v in params.items()} for _ in range(world)]
    pre = [pre_fn(xs[r], ps[r]) for r in range(world)]
    n = [float(p.shape[0]) for p in pre]
    dys = dy.reshape(world, -1, dy.shape[-1])
    loc = [torch.stack([p.detach().sum(0), (p.detach() ** 2).sum(0)]) for p in pre]
    tot, N = sum(loc), sum(n)
    fw = []
    for r in range(world):
        s, cnt = (loc[r], n[r]) if variant == "local_stats" else (tot, N)
        mean = s[0] / cnt
        var = s[1] / cnt - mean * mean
        rstd = (var + EPS) ** -0.5
        cnt_u = n[r] if variant == "count_without_world" else cnt
        tracked = mean - mean_shift if variant == "no_bias_shift" else mean
        xhat = (pre[r].detach() - mean) * rstd
        y = gamma * xhat + beta
        g = dys[r] * (y > 0) if relu else dys[r]
        fw.append({"xhat": xhat, "rstd": rstd, "g": g, "out": F.relu(y) if relu else y,
                   "running_mean": MOMENTUM * tracked, "running_var": (1 - MOMENTUM) + MOMENTUM * var * cnt_u / (cnt_u - 1),
                   "sums": torch.stack([g.sum(0), (g * xhat).sum(0)])})
    gtot = sum(f["sums"] for f in fw)
    out = []
    for r, f in enumerate(fw):
        s, cnt = (f["sums"], n[r]) if variant == "dx_local_sums" else (gtot, N)
        if variant == "count_without_world":
            cnt = n[r]
        pre[r].backward(gamma * f["rstd"] * (f["g"] - s[0] / cnt - f["xhat"] * s[1] / cnt))
        ps_sums = gtot if variant == "dgamma_dbeta_global" else f["sums"]
        res = {"out": f["out"], "dx": xs[r].grad, "d gamma": ps_sums[1], "d beta": ps_sums[0], "running_mean": f["running_mean"],
               "running_var": f["running_var"]}
        res.update({f"d {k}": v.grad for k, v in ps[r].items()})
        out.append(res)
    return out


def pwbn_played(inp, relu, need_dx, variant="correct"):
    ranks = played_ranks(lambda x, p: x @ p["w"].t(), inp["x"], {"w": inp["w"]}, inp["gamma"], inp["beta"], inp["dy"], relu, variant)
    for res in ranks:
        res["dx"] = res["dx"] if need_dx else None
    return ranks


def stem_played(inp, variant="correct"):
    ranks = played_ranks(lambda x, p: _rows_grad(F.conv2d(x, p["w"], stride=2, padding=1)), inp["x"], {"w": inp["w"]}, inp["gamma"], inp["beta"],
                         inp["dy"], 1, variant)
    for res in ranks:
        res["dx"] = None          # (the stem has no input gradient)
    return ranks


def sepbn_played(inp, variant="correct"):
    cin, cout = inp["w"].shape[1], inp["w"].shape[0]
    bias = inp["b_pw"] is not None

    def pre_fn(x, p):
        d = F.conv2d(x, p["taps"].t().reshape(cin, 1, 3, 3), inp["b_dw"], padding=1, groups=cin)
        return _rows_grad(F.conv2d(d, p["w"].view(cout, cin, 1, 1), inp["b_pw"]))
    ranks = played_ranks(pre_fn, inp["x"], {"taps": inp["taps"], "w": inp["w"]}, inp["gamma"], inp["beta"], inp["dy"], 1, variant,
                         mean_shift=inp["b_pw"] if bias else torch.zeros(cout, dtype=torch.float64))
    for res in ranks:
        res["dx"] = rows(res["dx"])
    return ranks


def _rows_grad(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
