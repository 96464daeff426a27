"""The head-side training operators of include/fear_train.h one by one through the C ABI — fear_xcorr_forward / _backward,
fear_exp_head_forward / _backward, fear_head_loss, fear_nchw_to_nhwc / fear_nhwc_to_nchw, fear_scale_column, fear_add — against the
float64 references and the derived element-wise bounds of tests/headref.py, at the strides the product calls them with (the
correlation written in place into columns of its own input buffer) and at the edges of their tilings.  Every output buffer is
pre-filled with a sentinel and has spare cells behind (and, strided, between) what the operator owns: they must come back untouched.
tests/test_head_ops_reference_cpu.py shows that the bounds admit an fp32 evaluation and reject the ways a kernel could be wrong."""
import functools

import numpy as np
import pytest
import torch

import headref as hr

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
GUARD = 8            # spare rows behind every output
OK, ERR_SHAPE, ERR_WORKSPACE = 0, -2, -7


@functools.lru_cache(maxsize=None)
def _lib():
    from feartracker_amd.train_head import load_train_library
    return load_train_library()


def _p(t, offset=0):
    from feartracker_amd.train_head import _p as p
    return p(t, offset)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


def _sent(*shape):
    return torch.full(shape, SENTINEL, device="cuda:0")


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _untouched(a):
    return bool((np.asarray(a) == np.float32(SENTINEL)).all())


def _within(got, ref_bound, what):
    ref, bound = ref_bound
    q = hr.excess(got.reshape(ref.shape), ref, bound)
    print(f"{what}: error / bound {q:.3f}")
    assert np.isfinite(got).all() and q <= 1.0, f"{what}: error / bound = {q:.3f}"


@functools.lru_cache(maxsize=None)
def _xcorr(case):
    d = hr.xcorr_inputs(*case)
    return d, hr.xcorr_forward(d["x"], d["z"]), hr.xcorr_backward(d["ds"], d["x"], d["z"], d["add"]), hr.xcorr_backward(d["ds"], d["x"], d["z"])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. / 2. MobileCorrelation


@pytest.mark.parametrize("form", ["dense", "in_place"])
@pytest.mark.parametrize("case", hr.XCORR_FWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_xcorr_forward(case, form):
    """(3,256,256,64): the product's shape, in_place = its call (ld 320, s into columns 256..319 of x's buffer); (5,32,64,16) and
    (2,160,256,36): 128-row workgroups that hold rows of two to four crops, J % 16 != 0; (3,96,8,4): a ragged last workgroup of three
    waves, J < 16; (1,32,4,4): one wave, one k group of four."""
    lib = _lib()
    B, P, C, J = case
    d, ref, _, _ = _xcorr(case)
    M = B * P
    z = _dev(d["z"])
    if form == "dense":
        x, s = _dev(d["x"].reshape(M, C)), _sent(M + GUARD, J)
        assert lib.fear_xcorr_forward(_p(x), C, _p(z), _p(s), J, B, P, C, J, None) == OK
        out = _np(s)
        assert _untouched(out[M:])
        got = out[:M]
    else:
        ld = (C + J + 3) // 4 * 4
        buf = _sent(M + GUARD, ld)
        buf[:M, :C] = _dev(d["x"].reshape(M, C))
        assert lib.fear_xcorr_forward(_p(buf), ld, _p(z), _p(buf, C), ld, B, P, C, J, None) == OK
        out = _np(buf)
        assert _untouched(out[M:]) and _untouched(out[:M, C + J:]) and np.array_equal(out[:M, :C], d["x"].reshape(M, C))
        got = out[:M, C:C + J]
    _within(got, ref, f"xcorr forward {case} {form}")


@pytest.mark.parametrize("with_add", [True, False], ids=["add", "no_add"])
@pytest.mark.parametrize("form", ["dense", "product"])
@pytest.mark.parametrize("case", hr.XCORR_BWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_xcorr_backward(case, form, with_add):
    """dx = dx_add + ds z^T and dz = x^T ds.  `product`: ds in columns C.. of an ld = C + J buffer whose columns 0..C-1 are dx_add, x in
    an ld = C + J buffer of its own, dx dense — the call of the head's backward (320 / 320 / 256).  (1,384,8,4): three 128-row tiles in
    one crop and the narrow weight-gradient kernel; (2,128,64,16): one tile per crop."""
    lib = _lib()
    B, P, C, J = case
    d, _, ref_add, ref_none = _xcorr(case)
    ref = ref_add if with_add else ref_none
    M = B * P
    z = _dev(d["z"])
    dx, dz = _sent(M + GUARD, C), _sent(B * C * J + 64)
    if form == "dense":
        ds, x, add = _dev(d["ds"].reshape(M, J)), _dev(d["x"].reshape(M, C)), _dev(d["add"].reshape(M, C))
        assert lib.fear_xcorr_backward(_p(ds), J, _p(x), C, _p(z), _p(add) if with_add else None, C, _p(dx), C, _p(dz), B, P, C, J, None) == OK
    else:
        ld = C + J
        dcat, cat = _sent(M, ld), _sent(M, ld)
        dcat[:, :C], dcat[:, C:] = _dev(d["add"].reshape(M, C)), _dev(d["ds"].reshape(M, J))
        cat[:, :C] = _dev(d["x"].reshape(M, C))
        before = _np(dcat).copy()
        assert lib.fear_xcorr_backward(_p(dcat, C), ld, _p(cat), ld, _p(z), _p(dcat) if with_add else None, ld, _p(dx), C, _p(dz),
                                       B, P, C, J, None) == OK
        assert np.array_equal(_np(dcat), before) and _untouched(_np(cat)[:, C:])
    out_dx, out_dz = _np(dx), _np(dz)
    assert _untouched(out_dx[M:]) and _untouched(out_dz[B * C * J:])
    _within(out_dx[:M], ref["dx"], f"xcorr dx {case} {form} add={with_add}")
    _within(out_dz[:B * C * J], ref["dz"], f"xcorr dz {case} {form} add={with_add}")


# 3. argument checks: every buffer is far larger than any of these calls could reach if it were NOT rejected — a missing check
# fails this test, it does not fault
_BIG = 1 << 20
_FWD_OK = dict(ldx=8, lds=8, B=2, P=128, C=8, J=8)
_FWD_BAD = [dict(B=-1), dict(P=0), dict(P=48), dict(C=2), dict(C=6), dict(J=2), dict(J=6), dict(ldx=6), dict(ldx=10), dict(ldx=4),
            dict(lds=6), dict(lds=10), dict(lds=4)]
_BWD_OK = dict(ldds=8, ldx=8, ldadd=8, lddx=8, B=2, P=128, C=8, J=8)
_BWD_BAD = [dict(B=-1), dict(P=0), dict(P=64), dict(P=96), dict(C=2), dict(C=6), dict(J=2), dict(J=6), dict(ldds=10), dict(ldds=4),
            dict(ldx=10), dict(ldx=4), dict(ldadd=10), dict(ldadd=4), dict(lddx=10), dict(lddx=4)]


def test_xcorr_argument_checks():
    """Both directions reject, with FEAR_TRAIN_ERR_SHAPE and before anything is launched, C or J below 4 or no multiple of 4, a
    leading dimension that is no multiple of 4 floats or shorter than its row, and a P that lets a tile straddle crops."""
    lib = _lib()
    x, z, add = (torch.ones(_BIG, device="cuda:0") for _ in range(3))
    s, dx, dz = _sent(_BIG), _sent(_BIG), _sent(_BIG)

    def fwd(a):
        return lib.fear_xcorr_forward(_p(x), a["ldx"], _p(z), _p(s), a["lds"], a["B"], a["P"], a["C"], a["J"], None)

    def bwd(a):
        return lib.fear_xcorr_backward(_p(x), a["ldds"], _p(x), a["ldx"], _p(z), _p(add), a["ldadd"], _p(dx), a["lddx"], _p(dz),
                                       a["B"], a["P"], a["C"], a["J"], None)

    for bad in _FWD_BAD:
        assert fwd(dict(_FWD_OK, **bad)) == ERR_SHAPE, ("forward", bad)
    for bad in _BWD_BAD:
        assert bwd(dict(_BWD_OK, **bad)) == ERR_SHAPE, ("backward", bad)
    assert _untouched(_np(s)) and _untouched(_np(dx)) and _untouched(_np(dz))
    # the same arguments without the defect are accepted (the rejections above are not the buffers' or the base shape's)
    assert fwd(_FWD_OK) == OK and bwd(_BWD_OK) == OK
    assert not _untouched(_np(s)[:2 * 128 * 8]) and not _untouched(_np(dx)[:2 * 128 * 8]) and not _untouched(_np(dz)[:2 * 8 * 8])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. box head


def _exp_ws_floats(M):
    blocks = (M + 127) // 128                  # col_blocks(M) for M <= 128 * 1024 rows
    return 2 * 4 * M + blocks * 16 + 8


@pytest.mark.parametrize("adjust", hr.EXP_ADJUST)
@pytest.mark.parametrize("M", hr.EXP_M)
def test_exp_head(M, adjust):
    """bbox = exp(adjust p + bias) over arguments in [-20, 12], and the backward from an fp32 bbox of its own and a signed dbbox whose
    four column sums behind d adjust have mixed signs; one workgroup with a ragged tail, two workgroups, eight column-sum partials."""
    lib = _lib()
    d = hr.exp_inputs(M, adjust)
    fwd = hr.exp_forward(d["p"], d["adjust"], d["bias4"])
    bwd = hr.exp_backward(d["p"], d["adjust"], d["bbox"], d["dbbox"])
    p, adj, bias = _dev(d["p"]), _dev(d["adjust"]), _dev(d["bias4"])
    out = _sent(M + GUARD, 4)
    assert lib.fear_exp_head_forward(_p(p), _p(adj), _p(bias), _p(out), M, None) == OK
    got = _np(out)
    assert _untouched(got[M:])
    _within(got[:M], fwd, f"exp head bbox M={M} adjust={adjust}")

    bbox, dbbox = _dev(d["bbox"]), _dev(d["dbbox"])
    dp, small = _sent(M + GUARD, 4), _sent(16)            # d adjust -> small[1], d bias4 -> small[4:8]
    need = _exp_ws_floats(M)
    ws = _sent(need + 64)
    args = (_p(p), _p(adj), _p(bbox), _p(dbbox), _p(dp), _p(small, 1), _p(small, 4), _p(ws))
    assert lib.fear_exp_head_backward(*args, (need - 1) * 4, M, None) == ERR_WORKSPACE
    assert _untouched(_np(dp)) and _untouched(_np(small)) and _untouched(_np(ws))
    assert lib.fear_exp_head_backward(*args, need * 4, M, None) == OK
    got_dp, got_small = _np(dp), _np(small)
    assert _untouched(got_dp[M:]) and _untouched(got_small[[0, 2, 3]]) and _untouched(got_small[8:]) and _untouched(_np(ws)[need:])
    _within(got_dp[:M], bwd["dp"], f"exp head dp M={M} adjust={adjust}")
    _within(got_small[4:8], bwd["dbias4"], f"exp head dbias4 M={M} adjust={adjust}")
    _within(got_small[1:2], bwd["dadjust"], f"exp head dadjust M={M} adjust={adjust}")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. FEARLoss

LOSS_CASES = [(M, coef, None) for M in hr.LOSS_M for coef in hr.LOSS_COEFS] + [(1000, hr.LOSS_COEFS[1], v) for v in hr.LOSS_VARIANTS]


@pytest.mark.parametrize("case", LOSS_CASES, ids=lambda c: f"M{c[0]}-coef{c[1][0]}_{c[1][1]}-{c[2] or 'mixed'}")
def test_head_loss(case):
    """Both losses, dcls and dbbox element-wise; labels 1 / 0 / ignored, a whole block without a weighted cell, exact p == t ties in
    one, two and four coordinates, logits +-30 and +-100, one block / a ragged tail block / 274 blocks through the finalize loop,
    selections of no, one and two cells; ignored and unweighted cells get exactly 0; a second call is bit-identical."""
    lib = _lib()
    M, (coef_cls, coef_reg), variant = case
    d = hr.loss_inputs(M, variant)
    ref = hr.loss_reference(**d, coef_cls=coef_cls, coef_reg=coef_reg)
    ins = [_dev(d[k]) for k in ("bbox", "cls", "gt_reg", "gt_cls", "gt_weight")]
    blocks = (M + 255) // 256
    need = blocks * 8 + 8

    def run():
        losses, dbbox, dcls, ws = _sent(4), _sent(M + GUARD, 4), _sent(M + GUARD), _sent(need + 64)
        assert lib.fear_head_loss(*[_p(t) for t in ins], coef_cls, coef_reg, _p(losses, 1), _p(dbbox), _p(dcls), _p(ws), need * 4, M, None) == OK
        out = _np(losses), _np(dbbox), _np(dcls)
        assert _untouched(out[0][[0, 3]]) and _untouched(out[1][M:]) and _untouched(out[2][M:]) and _untouched(_np(ws)[need:])
        return out[0][1:3], out[1][:M], out[2][:M]

    losses, dbbox, dcls = run()
    what = f"head loss M={M} coef=({coef_cls}, {coef_reg}) {variant or 'mixed'}"
    _within(losses, ref["losses"], what + " losses")
    _within(dcls, ref["dcls"], what + " dcls")
    _within(dbbox, ref["dbbox"], what + " dbbox")
    assert not dcls[ref["ignored"]].any() and not dbbox[ref["unweighted"]].any()
    n_pos, n_neg, n_reg = ref["counts"]
    if n_pos <= 1:
        assert not dcls[d["gt_cls"] == 1].any()
    if n_neg <= 1:
        assert not dcls[d["gt_cls"] == 0].any()
    if n_reg == 0:
        assert losses[1] == 0.0 and not dbbox.any()
    again = run()
    assert all(np.array_equal(a, b) for a, b in zip((losses, dbbox, dcls), again))


# ---------------------------------------------------------------------------------------------------------------------------
# 6. layout kernels, fear_scale_column, fear_add: exact


@pytest.mark.parametrize("case", hr.LAYOUT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_layout_kernels(case):
    """NCHW -> rows [n * HW][ld] at column ch_off and back, bit for bit; C = 3 (no multiple of 4), ch_off != 0, ld > C."""
    lib = _lib()
    n, C, HW, ld, off = case
    rng = np.random.default_rng(5)
    src = rng.standard_normal((n, C, HW)).astype(np.float32)
    rows, srcd = _sent(n * HW + GUARD, ld), _dev(src)
    assert lib.fear_nchw_to_nhwc(_p(srcd), _p(rows), n, C, HW, ld, off, None) == OK
    want = np.full((n * HW + GUARD, ld), SENTINEL, np.float32)
    want[:n * HW, off:off + C] = src.transpose(0, 2, 1).reshape(n * HW, C)
    assert np.array_equal(_np(rows), want)
    wide = rng.standard_normal((n * HW, ld)).astype(np.float32)
    back, wided = _sent(n * C * HW + GUARD), _dev(wide)
    assert lib.fear_nhwc_to_nchw(_p(wided), _p(back), n, C, HW, ld, off, None) == OK
    got = _np(back)
    assert _untouched(got[n * C * HW:])
    assert np.array_equal(got[:n * C * HW].reshape(n, C, HW), wide[:, off:off + C].reshape(n, HW, C).transpose(0, 2, 1))
    # no crops: nothing is written
    assert lib.fear_nchw_to_nhwc(_p(srcd), _p(back), 0, C, HW, ld, off, None) == OK
    assert lib.fear_nhwc_to_nchw(_p(wided), _p(back), 0, C, HW, ld, off, None) == OK
    assert np.array_equal(_np(back), got)


@pytest.mark.parametrize("M", [1, 257])
@pytest.mark.parametrize("shape", [(4, 3, 1, 0), (1, 0, 4, 2), (8, 5, 4, 3)], ids=["4to1", "1to4", "8to4"])
def test_scale_column(shape, M):
    """out[m * ld_out + col_out] = scale * in[m * ld_in + col_in]: one fp32 product, the other columns untouched"""
    lib = _lib()
    ld_in, col_in, ld_out, col_out = shape
    src = np.random.default_rng(6).standard_normal((M, ld_in)).astype(np.float32)
    out, srcd = _sent(M + GUARD, ld_out), _dev(src)
    assert lib.fear_scale_column(_p(srcd), ld_in, col_in, 0.1, _p(out), ld_out, col_out, M, None) == OK
    want = np.full((M + GUARD, ld_out), SENTINEL, np.float32)
    want[:M, col_out] = np.float32(0.1) * src[:, col_in]
    assert np.array_equal(_np(out), want)
    assert lib.fear_scale_column(_p(srcd), ld_in, col_in, 0.1, _p(out), ld_out, col_out, 0, None) == OK
    assert np.array_equal(_np(out), want)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n", hr.ADD_N)
def test_add(n, in_place):
    """out = a + b: the float4 body and the scalar tail (n % 4 != 0, n < 4, one element past a workgroup), out == a"""
    lib = _lib()
    rng = np.random.default_rng(7)
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    buf = _sent(n + GUARD)
    ad, bd = _dev(a), _dev(b)
    if in_place:
        buf[:n] = ad
        assert lib.fear_add(_p(buf), _p(bd), _p(buf), n, None) == OK
    else:
        assert lib.fear_add(_p(ad), _p(bd), _p(buf), n, None) == OK
    got = _np(buf)
    assert _untouched(got[n:]) and np.array_equal(got[:n], a + b)
    assert lib.fear_add(_p(bd), _p(bd), _p(buf), 0, None) == OK
    assert np.array_equal(_np(buf), got)
