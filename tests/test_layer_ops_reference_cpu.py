"""The bounds of tests/layerref.py are neither vacuous nor too tight (no GPU): at every case of tests/test_train_layer_ops_gpu.py an
fp32 numpy restatement of the operator — in the kernels' summation tree where the bound depends on it — stays inside its bound around
the float64 reference, each way a kernel could be subtly wrong leaves the bound on at least one element, and every exact-integer case
keeps sum |a||b| below 2^24."""
import numpy as np

import layerref as lr

f32 = np.float32


def _note(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), value)
    assert value <= 1.0, (key, value)


def _strided_copy(a, ld, off, fill=-7777.0):
    """`a` (rows, cols) laid into a flat buffer at pitch ld from element off, sentinel elsewhere"""
    rows, cols = a.shape
    flat = np.full(off + rows * ld + 8, fill, f32)
    np.lib.stride_tricks.as_strided(flat[off:], (rows, cols), (4 * ld, 4))[:] = a
    return flat


def test_fp32_restatement_stays_within_every_bound():
    """Largest error / bound of the fp32 restatement over all cases (Gaussian inputs): pw y 0.17, dx 0.26, dw 0.011; col_sum 0.96;
    mean 0.99, rstd 0.98, running_mean 0.99, running_var 0.98 (one rounding against u |ref|: a ratio near 1 is a value just above a
    power of two); a 0.99, b 0.98, bn y 0.81, act y 0.97; dbeta 0.98, dgamma 0.20, bn dx 0.57; depthwise y 0.26, dx 0.29, dw 0.036;
    the producers' statistics sum y 0.25, sum y^2 0.38; fear_bn_finalize from sums as mean / rstd / running above; every integer form is
    exact (0)."""
    worst = {}
    for (M, K, N), _ in lr.GEMM_CASES:
        for kind in ("gauss", "int"):
            d = lr.gemm_inputs(M, K, N, kind)
            for bias in (d["bias"], None):
                _note(worst, "pw y " + kind, lr.excess(lr.pw_forward_fp32(d["x"], d["w"], bias), *lr.pw_forward(d["x"], d["w"], bias)))
            for add in (d["add"], None):
                _note(worst, "pw dx " + kind, lr.excess(lr.pw_backward_data_fp32(d["dy"], d["w"], add), *lr.pw_backward_data(d["dy"], d["w"], add)))
    for (M, K, N), _ in lr.WGRAD_CASES:
        plan = lr.wgrad_plan(M, K, N)
        for kind in ("gauss", "int"):
            d = lr.gemm_inputs(M, K, N, kind)
            for form in lr.WGRAD_FORMS[:3]:
                a, b, relu = lr.wgrad_act(d, form)
                ref = lr.pw_backward_weight(d["dy"], d["x"], a, b, relu, plan, kind)
                got = lr.pw_backward_weight_fp32(d["dy"], d["x"], a, b, relu, plan)
                if kind == "int":
                    assert np.array_equal(got.astype(np.float64), ref[0]), (M, K, N, form)
                else:
                    _note(worst, "pw dw", lr.excess(got, *ref))
    for M, K, N in ((768, 256, 256), (200, 48, 80), (65, 36, 36), (76795, 16, 112), (2304, 256, 4), (9, 4, 8)):      # STATS_CASES of the GPU file
        for kind in ("gauss", "int"):
            d = lr.gemm_inputs(M, K, N, kind)
            y = lr.pw_forward_fp32(lr.act32(d["x"], d["a"], d["b"], 1), d["w"])
            ref, bound = lr.stats_sums(y, 5, kind)
            got = lr.stats_sums_fp32(lr.stats_groups(y, 32))
            _note(worst, "pw sum y " + kind, lr.excess(got[0], ref[0], bound[0]))
            _note(worst, "pw sum y^2", lr.excess(got[1], ref[1], bound[1]))
    for (M, C), _ in lr.COL_CASES:
        d = lr.bn_inputs(M, C)
        x64 = d["x"].astype(np.float64)
        sums = np.stack([x64.sum(0), (x64 * x64).sum(0)])
        st, got = lr.bn_stats(None, d["running_mean"], d["running_var"], sums=sums, count=M), lr.bn_stats_fp32(None, d["running_mean"], d["running_var"], sums=sums, count=M)
        for key in st:
            _note(worst, "finalize " + key, lr.excess(got[key], *st[key]))
        _note(worst, "col_sum", lr.excess(lr.col_sum_fp32(d["dy"]), *lr.col_sum(d["dy"])))
        di = lr.bn_inputs(M, C, "int")
        assert np.array_equal(lr.col_sum_fp32(di["dy"]).astype(np.float64), lr.col_sum(di["dy"], "int")[0])
        st, got = lr.bn_stats(d["x"], d["running_mean"], d["running_var"]), lr.bn_stats_fp32(d["x"], d["running_mean"], d["running_var"])
        for key in st:
            _note(worst, key, lr.excess(got[key], *st[key]))
        mean, rstd = got["mean"], got["rstd"]
        for relu in (0, 1):
            _note(worst, "bn y", lr.excess(lr.bn_apply_fp32(d["x"], mean, rstd, d["gamma"], d["beta"], relu), *lr.bn_apply(d["x"], mean, rstd, d["gamma"], d["beta"], relu)))
            a32 = d["gamma"] * rstd
            b32 = (d["beta"].astype(np.float64) - mean.astype(np.float64) * a32).astype(f32)
            ra, rb = lr.bn_affine(mean, rstd, d["gamma"], d["beta"], a32)
            _note(worst, "a", lr.excess(a32, *ra))
            _note(worst, "b", lr.excess(b32, *rb))
            for res in (d["residual"], None):
                _note(worst, "act y", lr.excess(lr.bn_act_fp32(d["x"], a32, b32, relu, res), *lr.bn_act(d["x"], a32, b32, relu, res)))
            for y_act, a, b in ((d["y_act"] if relu else None, None, None), (None, a32 if relu else None, b32 if relu else None)):
                got_b = lr.bn_backward_fp32(d["dy"], d["x"], mean, rstd, d["gamma"], y_act, a, b)
                mask = lr.bn_mask(d["dy"], y_act, d["x"], a, b)
                sums = lr.bn_backward_sums(d["dy"], d["x"], mean, rstd, mask)
                _note(worst, "dbeta", lr.excess(got_b["dbeta"], *sums["dbeta"]))
                _note(worst, "dgamma", lr.excess(got_b["dgamma"], *sums["dgamma"]))
                _note(worst, "bn dx", lr.excess(got_b["dx"], *lr.bn_backward_dx(d["dy"], d["x"], mean, rstd, d["gamma"], mask, got_b["dbeta"], got_b["dgamma"], M)))
    for case in lr.DW_CASES + [lr.DW_WGRAD_ONLY]:
        for k, s in lr.dw_variants(case):
            plan = lr.dw_wgrad_plan(*case, k, s)
            for kind in ("gauss", "int"):
                d = lr.dw_inputs(*case, k, s, kind)
                for a, b, relu in ((None, None, 0), (d["a"], d["b"], 1)):
                    ref = lr.dw_backward_weight(d["dy"], d["x"], k, s, a, b, relu, plan, kind)
                    _note(worst, "dw dw " + kind, lr.excess(lr.dw_backward_weight_fp32(d["dy"], d["x"], k, s, a, b, relu, plan), *ref))
                if case == lr.DW_WGRAD_ONLY:
                    continue
                y = lr.dw_forward_fp32(d["x"], d["w"], None, k, s, d["a"], d["b"], 1)
                ref, bound = lr.stats_sums(y.reshape(-1, case[3]), 3, kind)
                got = lr.stats_sums_fp32(lr.stats_groups(y, 4))
                _note(worst, "dw sum y " + kind, lr.excess(got[0], ref[0], bound[0]))
                _note(worst, "dw sum y^2", lr.excess(got[1], ref[1], bound[1]))
                for bias, a, b, relu in ((d["bias"], None, None, 0), (None, None, None, 0), (None, d["a"], d["b"], 1)):
                    _note(worst, "dw y " + kind, lr.excess(lr.dw_forward_fp32(d["x"], d["w"], bias, k, s, a, b, relu), *lr.dw_forward(d["x"], d["w"], bias, k, s, a, b, relu, kind)))
                _note(worst, "dw dx " + kind, lr.excess(lr.dw_backward_data_fp32(d["dy"], d["w"], case[1], case[2], k, s), *lr.dw_backward_data(d["dy"], d["w"], case[1], case[2], k, s, kind)))
    print("fp32 restatement, largest error / bound:", {k: round(v, 3) for k, v in sorted(worst.items())})
    assert all(v == 0.0 for k, v in worst.items() if k.endswith(" int"))


def test_integer_cases_keep_every_partial_sum_exact():
    """sum |a||b| < 2^24 over every output element of every integer case: any partial sum in any order is an fp32 integer"""
    lim = 2.0 ** 24
    for (M, K, N), _ in lr.GEMM_CASES:
        d = lr.gemm_inputs(M, K, N, "int")
        ax, aw, ady = (np.abs(d[k]).astype(np.float64) for k in ("x", "w", "dy"))
        assert lr.int_headroom(ax @ aw.T + np.abs(d["bias"]), ady @ aw + np.abs(d["add"])) < lim
    for (M, K, N), _ in lr.WGRAD_CASES:
        d = lr.gemm_inputs(M, K, N, "int")
        xa = np.abs(d["x"]).astype(np.float64) * d["a"] + np.abs(d["b"])
        assert lr.int_headroom(np.abs(d["dy"]).astype(np.float64).T @ xa) < lim
    for (M, C), _ in lr.COL_CASES:
        d = lr.bn_inputs(M, C, "int")
        assert lr.int_headroom(np.abs(d["dy"]).astype(np.float64).sum(0)) < lim
    for case in lr.DW_CASES + [lr.DW_WGRAD_ONLY]:
        for k, s in lr.dw_variants(case):
            d = lr.dw_inputs(*case, k, s, "int")
            xa = np.abs(d["x"]).astype(np.float64) * d["a"] + np.abs(d["b"])
            assert lr.int_headroom(np.array(k * k * xa.max() * 2.0 + 2), np.array(k * k * 4.0)) < lim                       # forward, input gradient
            assert lr.int_headroom(np.array(xa.max() * 2.0 * d["dy"][..., 0].size)) < lim                                   # weight gradient


def _rejected(got, ref_bound):
    return lr.excess(got, *ref_bound) > 1.0


def test_every_mutant_leaves_its_bound():
    """pitch taken as the width; last row / last float4 column dropped; add, bias or residual ignored; a tap across an image boundary;
    Ho and Wo swapped; the mask taken from y (or from x) where it is fma(x, a, b); fp32 accumulation in the column sums — each on Gaussian and,
    where the output is GEMM- or sum-shaped, on the integer inputs (where "leaves the bound" is "differs at all")."""
    # pointwise forward / input gradient (a case with ragged everything) and the pitch
    M, K, N = 65, 36, 36
    for kind in ("gauss", "int"):
        d = lr.gemm_inputs(M, K, N, kind)
        fwd, bwd = lr.pw_forward(d["x"], d["w"], d["bias"]), lr.pw_backward_data(d["dy"], d["w"], d["add"])
        if kind == "int":
            fwd, bwd = (fwd[0], 0 * fwd[1]), (bwd[0], 0 * bwd[1])
        for m in ("last_row", "last_quad", "no_bias"):
            assert _rejected(lr.pw_forward_fp32(d["x"], d["w"], d["bias"], m), fwd), m
        for m in ("last_row", "last_quad", "no_add"):
            assert _rejected(lr.pw_backward_data_fp32(d["dy"], d["w"], d["add"], m), bwd), m
        flat = _strided_copy(d["x"], 44, 4)
        assert not _rejected(lr.pw_forward_fp32(lr.strided(flat, M, K, 44, 4), d["w"], d["bias"]), fwd)
        assert _rejected(lr.pw_forward_fp32(lr.strided(flat, M, K, 44, 4, pitch_is_width=True), d["w"], d["bias"]), fwd)
    # weight gradient: a staged case of 16 384 rows — the Gaussian bound (0.3) is the size of one row's term there, the integer form is exact
    M, K, N = 16384, 48, 36
    plan = lr.wgrad_plan(M, K, N)
    dg, di = lr.gemm_inputs(M, K, N), lr.gemm_inputs(M, K, N, "int")
    for d, kind in ((dg, "gauss"), (di, "int")):
        ref = lr.pw_backward_weight(d["dy"], d["x"], d["a"], d["b"], 1, plan, kind)
        for m in ("last_quad", "mask_from_x", "no_act", "last_row"):
            assert _rejected(lr.pw_backward_weight_fp32(d["dy"], d["x"], d["a"], d["b"], 1, plan, m), ref), (kind, m)
    ref, bound = lr.pw_backward_weight(dg["dy"], dg["x"], None, None, 0, plan)
    lost = np.abs(np.outer(dg["dy"][-1], dg["x"][-1]))
    assert ((lost > 0) & (lost < bound)).any()      # a row whose terms are inside the rounding bound: only the exact form sees it go
    M, K, N = 777, 72, 40
    d = lr.gemm_inputs(M, K, N)
    ref = lr.pw_backward_weight(d["dy"], d["x"], None, None, 0, lr.wgrad_plan(M, K, N))
    assert _rejected(lr.pw_backward_weight_fp32(d["dy"], d["x"], None, None, 0, lr.wgrad_plan(M, K, N), "last_row"), ref)
    # the producers' statistics: a lost row, and the group sums added in one fp32 chain (sum y^2, all terms positive, shows it)
    d = lr.gemm_inputs(76795, 16, 112)
    y = lr.pw_forward_fp32(d["x"], d["w"])
    ref, bound = lr.stats_sums(y, 5)
    cut = y.copy()
    cut[-1] = 0
    got = lr.stats_sums_fp32(lr.stats_groups(cut, 32))
    assert _rejected(got[0], (ref[0], bound[0])) and _rejected(got[1], (ref[1], bound[1]))
    assert _rejected(lr.stats_sums_fp32(lr.stats_groups(y, 32), "fp32_accumulate")[1], (ref[1], bound[1]))
    yi = lr.pw_forward_fp32(*(lr.gemm_inputs(200, 48, 80, "int")[k] for k in ("x", "w")))
    cut = yi.copy()
    cut[-1] = 0
    assert yi[-1].any() and _rejected(lr.stats_sums_fp32(lr.stats_groups(cut, 32))[0], tuple(v[0] for v in lr.stats_sums(yi, 5, "int")))
    d = lr.dw_inputs(3, 12, 6, 8, 3, 2)
    y = lr.dw_forward_fp32(d["x"], d["w"], None, 3, 2)
    ref, bound = lr.stats_sums(y.reshape(-1, 8), 3)
    cut = y.copy()
    cut[-1, -1, -1] = 0
    got = lr.stats_sums_fp32(lr.stats_groups(cut, 4))
    assert _rejected(got[0], (ref[0], bound[0])) and _rejected(got[1], (ref[1], bound[1]))
    # fear_bn_finalize from sums handed in
    d = lr.bn_inputs(777, 672)
    x64 = d["x"].astype(np.float64)
    sums = np.stack([x64.sum(0), (x64 * x64).sum(0)])
    st = lr.bn_stats(None, d["running_mean"], d["running_var"], sums=sums, count=777)
    assert _rejected(lr.bn_stats_fp32(None, sums=sums, count=777, mutant="fp32_variance")["rstd"], st["rstd"])
    assert _rejected(lr.bn_stats_fp32(None, d["running_mean"], d["running_var"], "biased_running_var", sums=sums, count=777)["running_var"], st["running_var"])
    # column sums and BatchNorm
    for M, C in ((777, 672), (131073, 4)):
        d, di = lr.bn_inputs(M, C), lr.bn_inputs(M, C, "int")
        for m in ("fp32_accumulate", "last_row"):
            assert _rejected(lr.col_sum_fp32(d["x"], m), lr.col_sum(d["x"])), (M, C, m)
        dyi = di["dy"].copy()
        dyi[-1] = 1                                  # (a last row that cannot be all zero)
        assert _rejected(lr.col_sum_fp32(dyi, "last_row"), lr.col_sum(dyi, "int"))
        st = lr.bn_stats(d["x"], d["running_mean"], d["running_var"])
        for m, keys in (("fp32_accumulate", ("rstd",)), ("last_row", ("mean",)), ("biased_running_var", ("running_var",))):
            got = lr.bn_stats_fp32(d["x"], d["running_mean"], d["running_var"], m)
            assert any(_rejected(got[k], st[k]) for k in keys), (M, C, m)
    M, C = 129, 96
    d = lr.bn_inputs(M, C)
    ok = lr.bn_stats_fp32(d["x"])
    mean, rstd = ok["mean"], ok["rstd"]
    a32 = d["gamma"] * rstd
    b32 = (d["beta"].astype(np.float64) - mean.astype(np.float64) * a32).astype(f32)
    for m in ("last_row", "last_quad"):
        assert _rejected(lr.bn_apply_fp32(d["x"], mean, rstd, d["gamma"], d["beta"], 1, m), lr.bn_apply(d["x"], mean, rstd, d["gamma"], d["beta"], 1)), m
    for m in ("no_residual", "last_row", "last_quad"):
        assert _rejected(lr.bn_act_fp32(d["x"], a32, b32, 1, d["residual"], m), lr.bn_act(d["x"], a32, b32, 1, d["residual"])), m
    flat = _strided_copy(d["x"], 104, 4)
    assert _rejected(lr.bn_act_fp32(lr.strided(flat, M, C, 104, 4, pitch_is_width=True), a32, b32, 1), lr.bn_act(d["x"], a32, b32, 1))
    mask = lr.bn_mask(d["dy"], None, d["x"], a32, b32)
    sums = lr.bn_backward_sums(d["dy"], d["x"], mean, rstd, mask)
    y_out = lr.bn_act_fp32(d["x"], a32, b32, 1, d["residual"])
    for m, keys in (("mask_from_y", ("dbeta", "dgamma", "dx")), ("mask_from_x", ("dbeta", "dgamma", "dx")), ("no_mask", ("dbeta", "dgamma", "dx")),
                    ("last_row", ("dbeta", "dgamma", "dx"))):
        got = lr.bn_backward_fp32(d["dy"], d["x"], mean, rstd, d["gamma"], None, a32, b32, m, y_out)
        refs = dict(sums, dx=lr.bn_backward_dx(d["dy"], d["x"], mean, rstd, d["gamma"], mask, got["dbeta"], got["dgamma"], M))
        for key in keys:
            assert _rejected(got[key], refs[key]), (m, key)
    M, C = 131073, 4
    d = lr.bn_inputs(M, C)
    ok = lr.bn_stats_fp32(d["x"])
    mask = lr.bn_mask(d["dy"], d["y_act"])
    sums = lr.bn_backward_sums(d["dy"], d["x"], ok["mean"], ok["rstd"], mask)
    got = lr.bn_backward_fp32(d["dy"], d["x"], ok["mean"], ok["rstd"], d["gamma"], d["y_act"], mutant="fp32_accumulate")
    assert _rejected(got["dbeta"], sums["dbeta"])      # (d gamma's terms carry xhat's two roundings each: its bound is no tighter than an fp32 sum)
    # depthwise: (3, 12, 6, 8) has Ho != Wo, three images in one workgroup and a ragged strip
    case = (3, 12, 6, 8)
    for k, s in lr.dw_variants(case):
        plan = lr.dw_wgrad_plan(*case, k, s)
        for kind in ("gauss", "int"):
            d = lr.dw_inputs(*case, k, s, kind)
            ref = lr.dw_forward(d["x"], d["w"], d["bias"], k, s, kind=kind)
            for m in ("tap_wraps", "ho_wo_swapped", "no_bias", "last_row", "last_quad"):
                assert _rejected(lr.dw_forward_fp32(d["x"], d["w"], d["bias"], k, s, mutant=m), ref), (k, s, kind, m)
            ref = lr.dw_forward(d["x"], d["w"], None, k, s, d["a"], d["b"], 1, kind)
            assert _rejected(lr.dw_forward_fp32(d["x"], d["w"], None, k, s, d["a"], d["b"], 1, "pad_is_act_of_zero"), ref), (k, s, kind)
            rows = d["x"].reshape(-1, 8)
            flat = _strided_copy(rows, 12, 4)
            bad = np.ascontiguousarray(lr.strided(flat, rows.shape[0], 8, 12, 4, pitch_is_width=True)).reshape(d["x"].shape)
            assert _rejected(lr.dw_forward_fp32(bad, d["w"], d["bias"], k, s), lr.dw_forward(d["x"], d["w"], d["bias"], k, s, kind=kind))
            ref = lr.dw_backward_data(d["dy"], d["w"], case[1], case[2], k, s, kind)
            for m in ("tap_wraps", "last_row", "last_quad"):
                assert _rejected(lr.dw_backward_data_fp32(d["dy"], d["w"], case[1], case[2], k, s, m), ref), (k, s, kind, m)
            dyl, xl = d["dy"].copy(), d["x"].copy()
            dyl[-1, -1, -1], xl[-1, -2:, -2:] = 1, 2     # (the last output pixel and the inputs under its taps: never zero)
            ref = lr.dw_backward_weight(dyl, xl, k, s, d["a"], d["b"], 1, plan, kind)
            for m in ("tap_wraps", "mask_from_x", "last_quad") + (("last_row",) if kind == "int" else ()):
                assert _rejected(lr.dw_backward_weight_fp32(dyl, xl, k, s, d["a"], d["b"], 1, plan, m), ref), (k, s, kind, m)
    # the stem's gather
    x = np.random.default_rng(9).standard_normal((1, 3, 6, 10)).astype(f32)
    ref = lr.stem_im2col(x.astype(np.float64))
    assert np.array_equal(lr.stem_im2col(x), ref) and not ref[:, 27].any()
    for m in ("ho_wo_swapped", "no_zero_column"):
        assert not np.array_equal(lr.stem_im2col(x, m), ref), m
