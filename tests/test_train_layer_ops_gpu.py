"""The layer family of training operators of include/fear_train.h one by one through the C ABI — fear_pw_forward / _backward_data /
_backward_weight[_act] / _forward_stats, fear_col_sum, fear_bn_train_forward[_ab] / _backward[_x], fear_bn_backward_reduce_x / _apply_x,
fear_bn_finalize, fear_bn_act, fear_dw_forward[_stats] / _backward_data / _backward_weight[_act], fear_stem_im2col — against the float64
references and derived element-wise bounds of tests/layerref.py, on Gaussian inputs (error / bound <= 1) and on exact integer inputs
(bit-for-bit equality), dense and with every pitch different from its width (a pointer 4 floats into a wider buffer), at the shapes
where a launch changes kernel, tile or grid.  Every output is pre-filled with a sentinel and has GUARD spare rows behind it and, in the
strided form, spare columns around what the operator owns: all must come back untouched, and so must every input.
test_cases_reach_the_branches_they_claim (no GPU) holds each case to fear_layer_plan_info, which asks the launch code's own helpers.
tests/test_layer_ops_reference_cpu.py shows that the bounds admit an fp32 evaluation and reject the ways a kernel could be wrong."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import layerref as lr

gpu = pytest.mark.gpu

SENTINEL = -7777.0
GUARD = 8
OK, ERR_SHAPE, ERR_WORKSPACE = 0, -2, -7
MOM, EPS = lr.MOMENTUM, lr.EPS
f64 = np.float64


@functools.lru_cache(maxsize=None)
def _lib():
    from feartracker_amd.train_abi import load_train_library
    return load_train_library()


def _p(t, offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + t.element_size() * offset)


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _sent(*shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL, device="cuda:0", dtype=dtype)


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _ld(C, form):
    """dense: the width; strided: 320 for 256 channels (the product's buffers), else the width + 12"""
    return C if form == "dense" else (320 if C == 256 else C + 12)


class Mat:
    """A rows x cols matrix in device memory: dense, or at pitch ld inside a sentinel-filled (rows + GUARD) x ld buffer from column 4 on.
    As an input it holds `a`; as an output it is all sentinel.  `check()` returns the owned block and asserts the rest untouched."""

    def __init__(self, rows, cols, form, a=None):
        self.rows, self.cols, self.ld = rows, cols, _ld(cols, form)
        self.off = 0 if form == "dense" else 4
        self.t = _sent(rows + GUARD, self.ld)
        self.a = None if a is None else np.asarray(a, np.float32).reshape(rows, cols)
        if a is not None:
            self.t[:rows, self.off:self.off + cols] = _dev(self.a)
        self.before = _np(self.t).copy() if a is not None else None

    @property
    def p(self):
        return _p(self.t, self.off)

    def check(self, what=""):
        out = _np(self.t)
        if self.before is not None:
            assert np.array_equal(out, self.before), f"{what}: an input was modified"
            return self.a
        own = out[:self.rows, self.off:self.off + self.cols]
        rest = out.copy()
        rest[:self.rows, self.off:self.off + self.cols] = SENTINEL
        assert (rest == np.float32(SENTINEL)).all(), f"{what}: written outside the output"
        return own.copy()


_VECS = []


def _vec(a):
    """a per-channel input vector (weights, bias, gamma, beta, a, b, mean, rstd): must come back as it went in"""
    t = _dev(a)
    _VECS.append((t, np.array(a, np.float32)))
    return t


@pytest.fixture(autouse=True)
def _vectors_unchanged():
    _VECS.clear()
    yield
    for t, a in _VECS:
        assert np.array_equal(_np(t), a), "an input vector was modified"
    _VECS.clear()


def _untouched(t):
    return bool((_np(t) == SENTINEL).all())


def _within(got, ref_bound, what):
    ref, bound = ref_bound
    q = lr.excess(np.asarray(got).reshape(ref.shape), ref, bound)
    print(f"{what}: error / bound {q:.3f}")
    assert np.isfinite(got).all() and q <= 1.0, f"{what}: error / bound = {q:.3f}"


def _exact(got, ref, what):
    got = np.asarray(got, f64).reshape(ref.shape)
    assert np.array_equal(got, ref), f"{what}: {int((got != ref).sum())} of {ref.size} elements differ from the exact integer result"


def _twice(run):
    """run() allocates fresh outputs, calls the operator and returns its outputs as arrays: twice, bit-identical; the first is returned"""
    first, second = run(), run()
    assert len(first) == len(second) and all(np.array_equal(a, b) for a, b in zip(first, second)), "the second call differs from the first"
    return first


def _check(got, ref_bound, kind, what):
    if kind == "int":
        _exact(got, ref_bound[0], what)
    else:
        _within(got, ref_bound, what)


_cid = lambda c: "x".join(map(str, c[0] if isinstance(c[0], tuple) else c))


# ---------------------------------------------------------------------------------------------------------------------------
# the plan (host only)


def _fields(s):
    return {n: getattr(s, n) for n, _ in s._fields_}


def test_cases_reach_the_branches_they_claim():
    """Every case of this file against fear_layer_plan_info: kernel generation, row tile, column tiles and blocks or the first
    generation's grid; the weight gradient's variant and tiles; rows per column-reduction workgroup; the depthwise strips, the row-run
    path and the plain-load switch.  Move a threshold and this fails until the cases move with it."""
    for (M, K, N), claim in lr.GEMM_CASES:
        fwd = _fields(lr.layer_plan(M, K, N).forward)                    # fear_pw_forward(M, K, N)
        dx = _fields(lr.layer_plan(M, N, K).dx)                           # fear_pw_backward_data(M, K = outputs, N = contraction)
        assert {k: fwd[k] for k in claim} == claim, ((M, K, N), fwd)
        assert {k: dx[k] for k in claim} == claim, ((M, K, N), dx)
    assert lr.layer_plan(10945, 32, 672).forward.row_tile == 128 and -(-10945 // 128) * 6 == 516 and 10945 % 128 == 65
    assert -(-10880 // 128) * 6 == 510
    for (M, K, N), claim in lr.WGRAD_CASES:
        p = lr.layer_plan(M, K, N, lr.wgrad_ws(M, K, N))
        w = _fields(p.w)
        assert {k: w[k] for k in claim} == claim and _fields(p.w_act) == w, ((M, K, N), w)
        assert w["slices"] > 1 and w["rows_per_slice"] * (w["slices"] - 1) < M <= w["rows_per_slice"] * w["slices"]
    assert lr.layer_plan(16400, 136, 72, lr.wgrad_ws(16400, 136, 72)).w.slices >= 64          # slice_sum_kernel with 16 lanes
    M, K, N = WS_CAPPED
    capped, free = lr.layer_plan(M, K, N, 20 * N * K * 4).w, lr.layer_plan(M, K, N, lr.wgrad_ws(M, K, N)).w
    assert capped.slices == 20 < free.slices and capped.rows_per_slice > free.rows_per_slice
    for (M, C), claim in lr.COL_CASES:
        p = _fields(lr.layer_plan(M, 4, 4))
        assert {k: p[k] for k in claim} == claim, ((M, C), p)
    assert 141 - 128 == 13 and 256 // (96 // 4) == 10 and 256 // (1024 // 4) == 1
    run, strips = set(), set()
    for case in lr.DW_CASES + [lr.DW_WGRAD_ONLY]:
        for k, s in lr.dw_variants(case):
            d = lr.layer_plan(16, 4, 4, dw=(*case, k, s, case[3])).dw
            run.add(d.wgrad_row_run)
            strips.add((case[1] // s) % 4 != 0)
            assert not d.fwd_plain and not d.dgrad_plain
            if case == lr.DW_WGRAD_ONLY and s == 1:
                assert d.wgrad_rows == 256 and d.wgrad_workgroups >= 64
    assert run == {0, 1} and strips == {True, False}
    below, at = (lr.layer_plan(16, 4, 4, dw=(1, 8, 8, 8, 3, 1, ld)).dw for ld in lr.DW_SPAN_LD)
    assert (below.fwd_plain, below.dgrad_plain, at.fwd_plain, at.dgrad_plain) == (0, 0, 1, 1)


WS_CAPPED = (16400, 136, 72)


# ---------------------------------------------------------------------------------------------------------------------------
# pointwise forward and input gradient


@functools.lru_cache(maxsize=4)
def _gemm(M, K, N, kind):
    return lr.gemm_inputs(M, K, N, kind)


@gpu
@pytest.mark.parametrize("form", ["dense", "strided"])
@pytest.mark.parametrize("case", lr.GEMM_CASES, ids=_cid)
def test_pw_forward(case, form):
    """y = x w^T (+ bias), Gaussian and integer, with and without bias; the dense Gaussian call twice, bit-identical.  Largest error /
    bound measured on the MI355X: 0.21 (fear_pw_backward_data 0.17, fear_pw_forward_stats y 0.21, its sums 0.25)."""
    lib = _lib()
    (M, K, N), _ = case
    for kind in ("gauss", "int"):
        d = _gemm(M, K, N, kind)
        x, w, bias = Mat(M, K, form, d["x"]), _vec(d["w"]), _vec(d["bias"])
        first = None
        for b, bh in ((bias, d["bias"]), (None, None)) + (((bias, d["bias"]),) if form == "dense" and kind == "gauss" else ()):
            y = Mat(M, N, form)
            assert lib.fear_pw_forward(x.p, x.ld, _p(w), _p(b), y.p, y.ld, M, K, N, None) == OK
            what = f"pw_forward {M}x{K}x{N} {form} {kind} bias={b is not None}"
            got = y.check(what)
            _check(got, lr.pw_forward(d["x"], d["w"], bh), kind, what)
            if b is not None and first is not None:
                assert np.array_equal(got, first), what + ": the second call differs"
            if b is not None:
                first = got
        x.check("pw_forward x")


@gpu
@pytest.mark.parametrize("form", ["dense", "strided"])
@pytest.mark.parametrize("case", lr.GEMM_CASES, ids=_cid)
def test_pw_backward_data(case, form):
    """dx = (add) + dy w over the same table with the roles swapped: rows x contraction (dy's width N) x outputs (K); `add` at a pitch of
    its own, and absent."""
    lib = _lib()
    (M, N, K), _ = case
    for kind in ("gauss", "int"):
        d = _gemm(M, K, N, kind)
        dy, w = Mat(M, N, form, d["dy"]), _vec(d["w"])
        add = Mat(M, K, "strided" if form == "dense" else "dense", d["add"])      # never dx's pitch
        first = None
        for a in (add, None) + ((add,) if form == "dense" and kind == "gauss" else ()):
            dx = Mat(M, K, form)
            assert lib.fear_pw_backward_data(dy.p, dy.ld, _p(w), a.p if a else None, a.ld if a else 0, dx.p, dx.ld, M, K, N, None) == OK
            what = f"pw_backward_data {M}x{N}x{K} {form} {kind} add={a is not None}"
            got = dx.check(what)
            _check(got, lr.pw_backward_data(d["dy"], d["w"], d["add"] if a else None), kind, what)
            if a is not None and first is not None:
                assert np.array_equal(got, first), what + ": the second call differs"
            if a is not None:
                first = got
        dy.check("dy"), add.check("add")


def _stats_sums_check(s, y_got, depth, kind, what):
    """[sum y | sum y^2] from the returned y; integer y: sum y exactly (sum y^2 may pass 2^24 inside an fp32 partial: its bound stays)"""
    ref, bound = lr.stats_sums(y_got, depth, kind)
    C = ref.shape[1]
    _check(s[:C], (ref[0], bound[0]), kind, what + " sum y")
    _within(s[C:], (ref[1], bound[1]), what + " sum y^2")


STATS_CASES = [(768, 256, 256), (200, 48, 80), (65, 36, 36), (76795, 16, 112), (2304, 256, 4), (9, 4, 8)]


@gpu
@pytest.mark.parametrize("form", ["dense", "strided"])
@pytest.mark.parametrize("case", STATS_CASES, ids=_cid)
def test_pw_forward_stats(case, form):
    """y = act(x) w^T with the float64 column sums of the returned y; in_a = NULL, relu 0 and 1; exactly
    fear_train_stats_workspace_bytes of workspace with a guard behind it."""
    lib = _lib()
    M, K, N = case
    need = lib.fear_train_stats_workspace_bytes(M, N)
    assert need >= lr.layer_plan(M, K, N).stats_blocks * 2 * N * 8
    for kind in ("gauss", "int"):
        d = _gemm(M, K, N, kind)
        x, w, a, b = Mat(M, K, form, d["x"]), _vec(d["w"]), _vec(d["a"]), _vec(d["b"])
        for ah, bh, relu in ((None, None, 0), (d["a"], d["b"], 0), (d["a"], d["b"], 1)):
            what = f"pw_forward_stats {case} {form} {kind} act={ah is not None} relu={relu}"

            def run():
                y, sums, ws = Mat(M, N, form), _sent(2 * N + GUARD, dtype=torch.float64), _sent(need // 4 + 64)
                assert lib.fear_pw_forward_stats(x.p, x.ld, _p(a) if ah is not None else None, _p(b) if ah is not None else None, relu, _p(w),
                                                 y.p, y.ld, M, K, N, _p(sums), _p(ws), need, None) == OK
                s = _np(sums)
                assert (s[2 * N:] == SENTINEL).all() and _untouched(ws[need // 4:])
                return y.check(what), s[:2 * N]

            got, s = _twice(run)
            _check(got, lr.pw_forward_stats(d["x"], d["w"], ah, bh, relu), kind, what)
            _stats_sums_check(s, got, 5, kind, what)
        x.check("x")


# ---------------------------------------------------------------------------------------------------------------------------
# pointwise weight gradient


def _wgrad_call(lib, form_w, dy, x, a, b, relu, dw, ws, ws_bytes, M, K, N):
    if form_w == "plain":
        return lib.fear_pw_backward_weight(dy.p, dy.ld, x.p, x.ld, _p(dw), _p(ws), ws_bytes, M, K, N, None)
    return lib.fear_pw_backward_weight_act(dy.p, dy.ld, x.p, x.ld, _p(a), _p(b), relu, _p(dw), _p(ws), ws_bytes, M, K, N, None)


@gpu
@pytest.mark.parametrize("form", ["dense", "strided"])
@pytest.mark.parametrize("case", lr.WGRAD_CASES, ids=_cid)
def test_pw_backward_weight(case, form):
    """dw = dy^T act(x): plain, _act with relu 0 / 1 and with in_a = NULL, Gaussian against the bound of the launch's own summation
    tree (rows per slice and slices from the plan query) and integer against equality; a workspace with room for any slicing, a guard
    behind it.  Largest error / bound measured: 0.011 (the chain bound is a worst case; rounding errors add like a random walk)."""
    lib = _lib()
    (M, K, N), _ = case
    ws_bytes = lr.wgrad_ws(M, K, N)
    plan = lr.wgrad_plan(M, K, N, ws_bytes)
    assert plan[1] * N * K * 4 <= ws_bytes
    for kind in ("gauss", "int"):
        d = _gemm(M, K, N, kind)
        dy, x, a, b = Mat(M, N, form, d["dy"]), Mat(M, K, form, d["x"]), _vec(d["a"]), _vec(d["b"])
        ws = _sent(ws_bytes // 4 + 64)
        for form_w in lr.WGRAD_FORMS:
            ah, bh, relu = lr.wgrad_act(d, form_w)
            dw = _sent(N * K + 64)
            assert _wgrad_call(lib, form_w, dy, x, a if ah is not None else None, b if ah is not None else None, relu, dw, ws, ws_bytes, M, K, N) == OK
            got = _np(dw)
            what = f"pw_backward_weight {M}x{K}x{N} {form} {kind} {form_w}"
            assert (got[N * K:] == SENTINEL).all(), what
            _check(got[:N * K], lr.pw_backward_weight(d["dy"], d["x"], ah, bh, relu, plan, kind), kind, what)
        again = _sent(N * K + 64)
        assert _wgrad_call(lib, lr.WGRAD_FORMS[-1], dy, x, None, None, 0, again, ws, ws_bytes, M, K, N) == OK
        assert np.array_equal(_np(again), got), "the second call differs"
        assert _untouched(ws[ws_bytes // 4:])
        dy.check("dy"), x.check("x")


@gpu
def test_pw_backward_weight_workspace():
    """A workspace that holds 20 partials caps wgrad_plan at 20 slices (65 with room): same result within the bound of THAT tree, exact
    on integers.  One byte less than 17 partials — the fewest slices of 1 024 rows — is FEAR_TRAIN_ERR_WORKSPACE with dw untouched;
    so is no workspace at all."""
    lib = _lib()
    M, K, N = WS_CAPPED
    ws_bytes = 20 * N * K * 4
    plan = lr.wgrad_plan(M, K, N, ws_bytes)
    assert plan[:2] == (832, 20)
    ws = _sent(ws_bytes // 4 + 64)
    for kind in ("gauss", "int"):
        d = _gemm(M, K, N, kind)
        dy, x, dw = Mat(M, N, "dense", d["dy"]), Mat(M, K, "dense", d["x"]), _sent(N * K + 64)
        assert lib.fear_pw_backward_weight(dy.p, dy.ld, x.p, x.ld, _p(dw), _p(ws), ws_bytes, M, K, N, None) == OK
        got = _np(dw)
        assert (got[N * K:] == SENTINEL).all() and _untouched(ws[ws_bytes // 4:])
        _check(got[:N * K], lr.pw_backward_weight(d["dy"], d["x"], plan=plan, kind=kind), kind, f"capped weight gradient {kind}")
    dw, ws = _sent(N * K + 64), _sent(17 * N * K + 64)
    assert lr.wgrad_plan(M, K, N, 17 * N * K * 4)[:2] == (1024, 17) == lr.wgrad_plan(M, K, N, 17 * N * K * 4 - 1)[:2]
    assert lib.fear_pw_backward_weight(dy.p, dy.ld, x.p, x.ld, _p(dw), _p(ws), 17 * N * K * 4 - 1, M, K, N, None) == ERR_WORKSPACE
    assert lib.fear_pw_backward_weight(dy.p, dy.ld, x.p, x.ld, _p(dw), None, 0, M, K, N, None) == ERR_WORKSPACE
    assert lib.fear_pw_backward_weight_act(dy.p, dy.ld, x.p, x.ld, None, None, 0, _p(dw), _p(ws), 17 * N * K * 4 - 1, M, K, N, None) == ERR_WORKSPACE
    assert _untouched(dw) and _untouched(ws)
    # ... and exactly the 17 partials are enough (dy, x: the integer inputs of the loop above)
    assert lib.fear_pw_backward_weight(dy.p, dy.ld, x.p, x.ld, _p(dw), _p(ws), 17 * N * K * 4, M, K, N, None) == OK
    got = _np(dw)
    assert (got[N * K:] == SENTINEL).all() and _untouched(ws[17 * N * K:])
    _exact(got[:N * K], lr.pw_backward_weight(d["dy"], d["x"], kind="int")[0], "weight gradient with exactly 17 partials")


# ---------------------------------------------------------------------------------------------------------------------------
# column reductions and BatchNorm


@functools.lru_cache(maxsize=4)
def _bn(M, C, kind):
    return lr.bn_inputs(M, C, kind)


def _col_ws(M, C):
    """exactly the partials of col_blocks workgroups, [blocks][2][C] float64, and a guard behind them"""
    need = lr.layer_plan(M, 4, 4).col_blocks * 2 * C * 8
    return _sent(need // 4 + 64), need


def _ws_ok(ws, need):
    return _untouched(ws[need // 4:])


@gpu
@pytest.mark.parametrize("form", ["dense", "strided"])
@pytest.mark.parametrize("case", lr.COL_CASES, ids=_cid)
def test_col_sum(case, form):
    """out[c] = sum_m dy[m][c]: float64 end to end (a column of mean 300, deviation 0.01 among them), integers exactly; one byte of
    workspace less is FEAR_TRAIN_ERR_WORKSPACE"""
    lib = _lib()
    (M, C), _ = case
    for kind, key in (("gauss", "x"), ("int", "dy")):
        d = _bn(M, C, kind)
        dy, (ws, need) = Mat(M, C, form, d[key]), _col_ws(M, C)
        out = _sent(C + GUARD)
        assert lib.fear_col_sum(dy.p, dy.ld, _p(out), _p(ws), need - 1, M, C, None) == ERR_WORKSPACE and _untouched(out) and _untouched(ws)
        assert lib.fear_col_sum(dy.p, dy.ld, _p(out), _p(ws), need, M, C, None) == OK
        got = _np(out)
        assert (got[C:] == SENTINEL).all() and _ws_ok(ws, need)
        _check(got[:C], lr.col_sum(d[key], kind), kind, f"col_sum {M}x{C} {form} {kind}")
        again = _sent(C + GUARD)
        assert lib.fear_col_sum(dy.p, dy.ld, _p(again), _p(ws), need, M, C, None) == OK and np.array_equal(_np(again), got)
        dy.check("dy")


def _stats_check(got, st, what, running):
    for key in ("mean", "rstd") + (("running_mean", "running_var") if running else ()):
        _within(got[key], st[key], f"{what} {key}")


@gpu
@pytest.mark.parametrize("form", ["dense", "strided"])
@pytest.mark.parametrize("case", lr.COL_CASES, ids=_cid)
def test_bn_train_forward_and_backward(case, form):
    """fear_bn_train_forward (relu 0 / 1, running statistics tracked or NULL) and fear_bn_train_backward (y_act of its own pitch, or NULL):
    mean, rstd and the running statistics against float64; y, d beta, d gamma against references that take the vectors the operator
    returned; dx from the returned sums.  Largest error / bound measured (the same figures for _forward_ab and fear_bn_finalize): mean
    0.99, rstd 0.98, running_mean 0.99, running_var 0.98, a 0.99, b 0.98 (a single rounding against u |ref|), y 0.63 (0.97 in the
    affine form), d beta 0.98, d gamma 0.20, dx 0.57; fear_col_sum 0.99; the float64 sums of _reduce_x 0 and 0.26."""
    lib = _lib()
    (M, C), _ = case
    d = _bn(M, C, "gauss")
    st = lr.bn_stats(d["x"], d["running_mean"], d["running_var"])
    x, dy, gamma, beta = Mat(M, C, form, d["x"]), Mat(M, C, form, d["dy"]), _vec(d["gamma"]), _vec(d["beta"])
    yact = Mat(M, C, "strided" if form == "dense" else "dense", d["y_act"])
    for relu, running in ((1, True), (0, False)):
        what = f"bn_train_forward {M}x{C} {form} relu={relu}"

        def run_forward():
            y, vec, (ws, need) = Mat(M, C, form), _sent(2 * C + GUARD), _col_ws(M, C)
            rm, rv = _dev(d["running_mean"]), _dev(d["running_var"])
            args = lambda nbytes: (x.p, x.ld, _p(gamma), _p(beta), y.p, y.ld, _p(vec), _p(vec, C), _p(rm) if running else None,
                                   _p(rv) if running else None, MOM, EPS, M, C, relu, _p(ws), nbytes, None)
            assert lib.fear_bn_train_forward(*args(need - 1)) == ERR_WORKSPACE and _untouched(vec)
            assert lib.fear_bn_train_forward(*args(need)) == OK
            v = _np(vec)
            assert (v[2 * C:] == SENTINEL).all() and _ws_ok(ws, need)
            return v[:2 * C], _np(rm), _np(rv), y.check(what)

        v, rm_got, rv_got, y_got = _twice(run_forward)
        got = {"mean": v[:C], "rstd": v[C:2 * C], "running_mean": rm_got, "running_var": rv_got}
        _stats_check(got, st, what, running)
        if not running:
            assert np.array_equal(got["running_mean"], d["running_mean"]) and np.array_equal(got["running_var"], d["running_var"])
        _within(y_got, lr.bn_apply(d["x"], got["mean"], got["rstd"], d["gamma"], d["beta"], relu), what + " y")
        # backward, from the mean / rstd just returned
        mean, rstd = _vec(got["mean"]), _vec(got["rstd"])
        ya = yact if relu else None
        what = f"bn_train_backward {M}x{C} {form} y_act={ya is not None}"

        def run_backward():
            dx, grads, (ws, need) = Mat(M, C, form), _sent(2 * C + GUARD), _col_ws(M, C)
            assert lib.fear_bn_train_backward(dy.p, dy.ld, ya.p if ya else None, ya.ld if ya else 0, x.p, x.ld, _p(mean), _p(rstd), _p(gamma),
                                              dx.p, dx.ld, _p(grads), _p(grads, C), M, C, _p(ws), need, None) == OK
            g = _np(grads)
            assert (g[2 * C:] == SENTINEL).all() and _ws_ok(ws, need)
            return g[:2 * C], dx.check(what)

        g, dx_got = _twice(run_backward)
        mask = lr.bn_mask(d["dy"], d["y_act"] if relu else None)
        sums = lr.bn_backward_sums(d["dy"], d["x"], got["mean"], got["rstd"], mask)
        _within(g[C:2 * C], sums["dbeta"], what + " dbeta")
        _within(g[:C], sums["dgamma"], what + " dgamma")
        _within(dx_got, lr.bn_backward_dx(d["dy"], d["x"], got["mean"], got["rstd"], d["gamma"], mask, g[C:2 * C], g[:C], M), what + " dx")
    x.check("x"), dy.check("dy"), yact.check("y_act")


@gpu
@pytest.mark.parametrize("form", ["dense", "strided"])
@pytest.mark.parametrize("case", lr.COL_CASES, ids=_cid)
def test_bn_forward_ab_and_backward_x(case, form):
    """fear_bn_train_forward_ab (relu 0 / 1; a residual of its own pitch, or none; running statistics or NULL) -> the a, b it returned pass
    their bounds -> fear_bn_train_backward_x and the pair fear_bn_backward_reduce_x / _apply_x with those a, b as inputs: the mask is
    fma(x, a, b) > 0 in float64, no element excused.  Integer dy: d beta exact."""
    lib = _lib()
    (M, C), _ = case
    d, di = _bn(M, C, "gauss"), _bn(M, C, "int")
    st = lr.bn_stats(d["x"], d["running_mean"], d["running_var"])
    x, gamma, beta = Mat(M, C, form, d["x"]), _vec(d["gamma"]), _vec(d["beta"])
    res = Mat(M, C, "strided" if form == "dense" else "dense", d["residual"])
    for relu, running, r in ((1, True, None), (0, False, res), (1, False, res)):
        what = f"bn_train_forward_ab {M}x{C} {form} relu={relu} residual={r is not None}"

        def run_forward():
            y, vec, (ws, need) = Mat(M, C, form), _sent(4 * C + GUARD), _col_ws(M, C)
            rm, rv = _dev(d["running_mean"]), _dev(d["running_var"])
            assert lib.fear_bn_train_forward_ab(x.p, x.ld, _p(gamma), _p(beta), relu, r.p if r else None, r.ld if r else 0, y.p, y.ld, _p(vec),
                                                _p(vec, C), _p(vec, 2 * C), _p(vec, 3 * C), _p(rm) if running else None, _p(rv) if running else None,
                                                MOM, EPS, M, C, _p(ws), need, None) == OK
            v = _np(vec)
            assert (v[4 * C:] == SENTINEL).all() and _ws_ok(ws, need)
            return v[:4 * C], _np(rm), _np(rv), y.check(what)

        v, rm_got, rv_got, y_got = _twice(run_forward)
        got = {"mean": v[:C], "rstd": v[C:2 * C], "running_mean": rm_got, "running_var": rv_got}
        a, b = v[2 * C:3 * C], v[3 * C:4 * C]
        _stats_check(got, st, what, running)
        ra, rb = lr.bn_affine(got["mean"], got["rstd"], d["gamma"], d["beta"], a)
        _within(a, ra, what + " a")
        _within(b, rb, what + " b")
        _within(y_got, lr.bn_act(d["x"], a, b, relu, d["residual"] if r else None), what + " y")
        # backward with the returned a, b
        mean, rstd, av, bv = _vec(got["mean"]), _vec(got["rstd"]), _vec(a), _vec(b)
        mask = lr.bn_mask(d["dy"], None, d["x"], a if relu else None, b if relu else None)
        for kind, dyh in (("gauss", d["dy"]), ("int", di["dy"])):
            dy = Mat(M, C, form, dyh)
            sums = lr.bn_backward_sums(dyh, d["x"], got["mean"], got["rstd"], mask, kind)
            what = f"bn_train_backward_x {M}x{C} {form} relu={relu} {kind}"

            def run_backward():
                dx, grads, (ws, need) = Mat(M, C, form), _sent(2 * C + GUARD), _col_ws(M, C)
                assert lib.fear_bn_train_backward_x(dy.p, dy.ld, x.p, x.ld, _p(av) if relu else None, _p(bv) if relu else None, relu, _p(mean),
                                                    _p(rstd), _p(gamma), dx.p, dx.ld, _p(grads), _p(grads, C), M, C, _p(ws), need, None) == OK
                g = _np(grads)
                assert (g[2 * C:] == SENTINEL).all() and _ws_ok(ws, need)
                return g[:2 * C], dx.check(what)

            g, got_dx = _twice(run_backward)
            _check(g[C:2 * C], sums["dbeta"], kind, what + " dbeta")
            _within(g[:C], sums["dgamma"], what + " dgamma")
            _within(got_dx, lr.bn_backward_dx(dyh, d["x"], got["mean"], got["rstd"], d["gamma"], mask, g[C:2 * C], g[:C], M), what + " dx")
            # the SyncBatchNorm pair: float64 sums, then dx / d gamma / d beta from them (one rank: the same numbers, bit for bit)
            def run_reduce():
                s64, (ws, need) = _sent(2 * C + GUARD, dtype=torch.float64), _col_ws(M, C)
                assert lib.fear_bn_backward_reduce_x(dy.p, dy.ld, x.p, x.ld, _p(av) if relu else None, _p(bv) if relu else None, relu, _p(mean),
                                                     _p(rstd), _p(s64), M, C, _p(ws), need, None) == OK
                s = _np(s64)
                assert (s[2 * C:] == SENTINEL).all() and _ws_ok(ws, need)
                return (s[:2 * C],)

            s, = _twice(run_reduce)
            s64 = _dev(s, f64)
            raw = lr.bn_backward_sums(dyh, d["x"], got["mean"], got["rstd"], mask, kind, rounded=False)
            _check(s[:C], raw["dbeta"], kind, what + " reduce_x sum g")
            _within(s[C:2 * C], raw["dgamma"], what + " reduce_x sum g xhat")
            dx2, grads2, ws2 = Mat(M, C, form), _sent(2 * C + GUARD), _sent(2 * C + GUARD)
            assert lib.fear_bn_backward_apply_x(dy.p, dy.ld, x.p, x.ld, _p(av) if relu else None, _p(bv) if relu else None, relu, _p(mean), _p(rstd),
                                                _p(gamma), _p(s64), float(M), _p(s64), dx2.p, dx2.ld, _p(grads2), _p(grads2, C), _p(ws2), 2 * C * 4,
                                                M, C, None) == OK
            assert np.array_equal(_np(grads2)[:2 * C], g) and np.array_equal(dx2.check(what), got_dx) and (_np(ws2)[2 * C:] == SENTINEL).all()
            assert (_np(grads2)[2 * C:] == SENTINEL).all()
            dy.check("dy")
    x.check("x"), res.check("residual")


@gpu
@pytest.mark.parametrize("case", lr.COL_CASES, ids=_cid)
def test_bn_finalize_and_act(case):
    """fear_bn_finalize from float64 sums handed in (count = M; running statistics or NULL) and fear_bn_act (relu 0 / 1, a residual of its
    own pitch or none, dense and strided) with vectors handed in."""
    lib = _lib()
    (M, C), _ = case
    d = _bn(M, C, "gauss")
    x64 = d["x"].astype(f64)
    sums_h = np.stack([x64.sum(0), (x64 * x64).sum(0)])
    st = lr.bn_stats(None, d["running_mean"], d["running_var"], sums=sums_h, count=M)
    sums, gamma, beta = _dev(sums_h, f64), _vec(d["gamma"]), _vec(d["beta"])
    for running in (True, False):
        def run_finalize():
            vec, rm, rv = _sent(4 * C + GUARD), _dev(d["running_mean"]), _dev(d["running_var"])
            assert lib.fear_bn_finalize(_p(sums), float(M), _p(gamma), _p(beta), _p(vec), _p(vec, C), _p(vec, 2 * C), _p(vec, 3 * C),
                                        _p(rm) if running else None, _p(rv) if running else None, MOM, EPS, C, None) == OK
            v = _np(vec)
            assert (v[4 * C:] == SENTINEL).all()
            return v[:4 * C], _np(rm), _np(rv)

        v, rm_got, rv_got = _twice(run_finalize)
        got = {"mean": v[:C], "rstd": v[C:2 * C], "running_mean": rm_got, "running_var": rv_got}
        _stats_check(got, st, f"bn_finalize {M}x{C}", running)
        ra, rb = lr.bn_affine(got["mean"], got["rstd"], d["gamma"], d["beta"], v[2 * C:3 * C])
        _within(v[2 * C:3 * C], ra, "bn_finalize a")
        _within(v[3 * C:4 * C], rb, "bn_finalize b")
    a, b = v[2 * C:3 * C].copy(), v[3 * C:4 * C].copy()
    av, bv = _vec(a), _vec(b)
    for form in ("dense", "strided"):
        x, res = Mat(M, C, form, d["x"]), Mat(M, C, "strided" if form == "dense" else "dense", d["residual"])
        for relu, r in ((0, None), (1, res), (0, res)):
            what = f"bn_act {M}x{C} {form} relu={relu} residual={r is not None}"

            def run_act():
                y = Mat(M, C, form)
                assert lib.fear_bn_act(x.p, x.ld, _p(av), _p(bv), relu, r.p if r else None, r.ld if r else 0, y.p, y.ld, M, C, None) == OK
                return (y.check(what),)

            _within(_twice(run_act)[0], lr.bn_act(d["x"], a, b, relu, d["residual"] if r else None), what)
        x.check("x"), res.check("residual")


@gpu
@pytest.mark.parametrize("M", [1, 2])
def test_bn_running_variance_of_one_and_two_rows(M):
    """M = 2: the unbiased variance is twice the biased one; M = 1: the kernel tracks the biased variance 0 (torch has NaN there)"""
    lib = _lib()
    C = 8
    d = lr.bn_inputs(M, C)
    st = lr.bn_stats(d["x"], d["running_mean"], d["running_var"])
    x, gamma, beta, y = Mat(M, C, "dense", d["x"]), _vec(d["gamma"]), _vec(d["beta"]), Mat(M, C, "dense")
    vec, rm, rv, (ws, need) = _sent(2 * C + GUARD), _dev(d["running_mean"]), _dev(d["running_var"]), _col_ws(M, C)
    assert lib.fear_bn_train_forward(x.p, x.ld, _p(gamma), _p(beta), y.p, y.ld, _p(vec), _p(vec, C), _p(rm), _p(rv), MOM, EPS, M, C, 0, _p(ws), need, None) == OK
    v = _np(vec)
    _stats_check({"mean": v[:C], "rstd": v[C:2 * C], "running_mean": _np(rm), "running_var": _np(rv)}, st, f"bn M={M}", True)
    if M == 1:
        assert np.array_equal(_np(rv), (0.9 * d["running_var"].astype(f64)).astype(np.float32))
    _within(y.check("y"), lr.bn_apply(d["x"], v[:C], v[C:2 * C], d["gamma"], d["beta"], 0), f"bn M={M} y")


# ---------------------------------------------------------------------------------------------------------------------------
# depthwise


@functools.lru_cache(maxsize=4)
def _dw(case, k, s, kind):
    return lr.dw_inputs(*case, k, s, kind)


DW_PARAMS = [(c, k, s) for c in lr.DW_CASES for k, s in lr.dw_variants(c)]
_dwid = lambda p: "x".join(map(str, p[0])) + f"-k{p[1]}s{p[2]}"


@gpu
@pytest.mark.parametrize("form", ["dense", "strided"])
@pytest.mark.parametrize("param", DW_PARAMS, ids=_dwid)
def test_dw_forward_and_stats(param, form):
    """fear_dw_forward with and without bias, and fear_dw_forward_stats (in_a NULL, relu 0 / 1; zero padding of the ACTIVATION) with
    exactly fear_train_stats_workspace_bytes(rows, C) of workspace and the float64 sums of the returned y.  Largest error / bound
    measured: y 0.27 (0.28 with statistics), sums 0.30; fear_dw_backward_data 0.27; fear_dw_backward_weight 0.026."""
    lib = _lib()
    case, k, s = param
    B, H, W, C = case
    Ho, Wo = H // s, W // s
    rows = B * Ho * Wo
    need = lib.fear_train_stats_workspace_bytes(rows, C)
    assert need >= lr.layer_plan(16, 4, 4, dw=(*case, k, s, C)).dw.workgroups * 2 * C * 8
    for kind in ("gauss", "int"):
        d = _dw(case, k, s, kind)
        x, w, bias, a, b = Mat(B * H * W, C, form, d["x"]), _vec(d["w"]), _vec(d["bias"]), _vec(d["a"]), _vec(d["b"])
        first = None
        for bv, bh in ((bias, d["bias"]), (None, None), (bias, d["bias"])):
            y = Mat(rows, C, form)
            assert lib.fear_dw_forward(x.p, x.ld, _p(w), _p(bv), y.p, y.ld, B, H, W, C, k, s, None) == OK
            what = f"dw_forward {case} k{k} s{s} {form} {kind} bias={bv is not None}"
            got = y.check(what)
            _check(got, lr.dw_forward(d["x"], d["w"], bh, k, s, kind=kind), kind, what)
            if bv is not None and first is not None:
                assert np.array_equal(got, first), what + ": the second call differs"
            if bv is not None:
                first = got
        for ah, bh, relu in ((None, None, 0), (d["a"], d["b"], 0), (d["a"], d["b"], 1)):
            what = f"dw_forward_stats {case} k{k} s{s} {form} {kind} act={ah is not None} relu={relu}"

            def run():
                y, sums, ws = Mat(rows, C, form), _sent(2 * C + GUARD, dtype=torch.float64), _sent(need // 4 + 64)
                assert lib.fear_dw_forward_stats(x.p, x.ld, _p(a) if ah is not None else None, _p(b) if ah is not None else None, relu, _p(w),
                                                 y.p, y.ld, B, H, W, C, k, s, _p(sums), _p(ws), need, None) == OK
                sm = _np(sums)
                assert (sm[2 * C:] == SENTINEL).all() and _untouched(ws[need // 4:])
                return y.check(what), sm[:2 * C]

            got, sm = _twice(run)
            _check(got, lr.dw_forward(d["x"], d["w"], None, k, s, ah, bh, relu, kind), kind, what)
            _stats_sums_check(sm, got, 3, kind, what)
        x.check("x")


@gpu
def test_dw_forward_stats_workspace_of_a_flat_map():
    """One output row of 256 x 1024 channels: a thread's strip of four rows holds one, so the launch is 256 workgroups where
    fear_train_stats_workspace_bytes allows for 192 — FEAR_TRAIN_ERR_WORKSPACE before anything is launched (the header says so); with
    the 256 partial rows the launch needs, the result is right."""
    lib = _lib()
    case, k, s = (1, 1, 256, 1024), 3, 1
    B, H, W, C = case
    plan = lr.layer_plan(16, 4, 4, dw=(*case, k, s, C)).dw
    helper, need = lib.fear_train_stats_workspace_bytes(B * H * W, C), plan.workgroups * 2 * C * 8
    assert plan.workgroups == 256 and helper == 192 * 2 * C * 8 < need
    d = lr.dw_inputs(*case, k, s)
    x, w, y = Mat(B * H * W, C, "dense", d["x"]), _vec(d["w"]), Mat(B * H * W, C, "dense")
    sums, ws = _sent(2 * C + GUARD, dtype=torch.float64), _sent(need // 4 + 64)
    call = lambda n: lib.fear_dw_forward_stats(x.p, x.ld, None, None, 0, _p(w), y.p, y.ld, B, H, W, C, k, s, _p(sums), _p(ws), n, None)
    assert call(helper) == ERR_WORKSPACE and call(need - 1) == ERR_WORKSPACE
    assert _untouched(sums) and _untouched(ws) and _untouched(y.t)
    assert call(need) == OK
    got = y.check("y")
    _within(got, lr.dw_forward(d["x"], d["w"], None, k, s), "dw_forward_stats flat map")
    _stats_sums_check(_np(sums)[:2 * C], got, 3, "gauss", "dw_forward_stats flat map")
    assert _untouched(ws[need // 4:])


@gpu
@pytest.mark.parametrize("form", ["dense", "strided"])
@pytest.mark.parametrize("param", DW_PARAMS, ids=_dwid)
def test_dw_backward_data(param, form):
    """dx = the gather of dy over the taps whose parity matches the stride; images side by side in one workgroup, a 5 x 5 halo wider than
    a 2 x 2 map, twice (bit-identical)"""
    lib = _lib()
    case, k, s = param
    B, H, W, C = case
    rows = B * (H // s) * (W // s)
    for kind in ("gauss", "int"):
        d = _dw(case, k, s, kind)
        dy, w = Mat(rows, C, form, d["dy"]), _vec(d["w"])
        ref, first = lr.dw_backward_data(d["dy"], d["w"], H, W, k, s, kind), None
        for _ in range(2):
            dx = Mat(B * H * W, C, form)
            assert lib.fear_dw_backward_data(dy.p, dy.ld, _p(w), dx.p, dx.ld, B, H, W, C, k, s, None) == OK
            what = f"dw_backward_data {case} k{k} s{s} {form} {kind}"
            got = dx.check(what)
            _check(got, ref, kind, what)
            assert first is None or np.array_equal(got, first)
            first = got
        dy.check("dy")


@gpu
@pytest.mark.parametrize("form", ["dense", "strided"])
@pytest.mark.parametrize("param", DW_PARAMS + [(lr.DW_WGRAD_ONLY, k, s) for k, s in lr.dw_variants(lr.DW_WGRAD_ONLY)], ids=_dwid)
def test_dw_backward_weight(param, form):
    """dw_taps = sum over the output pixels of dy x act(x): plain, _act with relu 0 / 1 and in_a = NULL; the row-run path and the pixel
    path; exactly the partials of the plan's workgroups as workspace (one byte less: FEAR_TRAIN_ERR_WORKSPACE)"""
    lib = _lib()
    case, k, s = param
    B, H, W, C = case
    rows = B * (H // s) * (W // s)
    plan = lr.dw_wgrad_plan(*case, k, s)
    need = plan[1] * k * k * C * 4
    for kind in ("gauss", "int"):
        d = _dw(case, k, s, kind)
        dy, x, a, b = Mat(rows, C, form, d["dy"]), Mat(B * H * W, C, form, d["x"]), _vec(d["a"]), _vec(d["b"])
        ws, got = _sent(need // 4 + 64), None
        for form_w in lr.WGRAD_FORMS + ["act_null"]:
            ah, bh, relu = lr.wgrad_act(d, form_w)
            dw = _sent(k * k * C + 64)
            if form_w == "plain":
                call = lambda n: lib.fear_dw_backward_weight(dy.p, dy.ld, x.p, x.ld, _p(dw), _p(ws), n, B, H, W, C, k, s, None)
            else:
                call = lambda n: lib.fear_dw_backward_weight_act(dy.p, dy.ld, x.p, x.ld, _p(a) if ah is not None else None, _p(b) if ah is not None else None,
                                                                 relu, _p(dw), _p(ws), n, B, H, W, C, k, s, None)
            assert call(need - 1) == ERR_WORKSPACE and _untouched(dw)
            assert call(need) == OK
            what = f"dw_backward_weight {case} k{k} s{s} {form} {kind} {form_w}"
            prev, got = got, _np(dw)
            assert (got[k * k * C:] == SENTINEL).all() and _untouched(ws[need // 4:]), what
            _check(got[:k * k * C], lr.dw_backward_weight(d["dy"], d["x"], k, s, ah, bh, relu, plan, kind), kind, what)
        assert np.array_equal(prev, got), "the second call differs"
        dy.check("dy"), x.check("x")


@gpu
def test_dw_span_boundary():
    """B = 1, H = W = 8, C = 8 with the 64 rows at a pitch of 8388604 floats (the tensor spans 2^31 - 1024 bytes: buffer loads) and of
    8388608 floats (2^31 bytes: plain loads): fear_dw_forward, fear_dw_forward_stats (x at that pitch) and fear_dw_backward_data (dy at
    that pitch).  One 2 GiB allocation, of which only the 64 rows are written; the outputs are dense."""
    lib = _lib()
    B, H, W, C = 1, 8, 8, 8
    big = torch.empty(63 * max(lr.DW_SPAN_LD) + 64, device="cuda:0")
    need = lib.fear_train_stats_workspace_bytes(64, C)
    for ld in lr.DW_SPAN_LD:
        for k, s in ((3, 1), (5, 1), (5, 2)):
            d = lr.dw_inputs(B, H, W, C, k, s, "gauss")
            rows_view = torch.as_strided(big, (64, C), (ld, 1))
            rows_view.copy_(_dev(d["x"].reshape(64, C)))
            w, bias = _vec(d["w"]), _vec(d["bias"])
            rows = (H // s) * (W // s)
            y = Mat(rows, C, "dense")
            assert lib.fear_dw_forward(_p(big), ld, _p(w), _p(bias), y.p, y.ld, B, H, W, C, k, s, None) == OK
            _within(y.check("y"), lr.dw_forward(d["x"], d["w"], d["bias"], k, s), f"dw_forward ld={ld} k{k} s{s}")
            y, sums, ws = Mat(rows, C, "dense"), _sent(2 * C + GUARD, dtype=torch.float64), _sent(need // 4 + 64)
            a, b = _vec(d["a"]), _vec(d["b"])
            assert lib.fear_dw_forward_stats(_p(big), ld, _p(a), _p(b), 1, _p(w), y.p, y.ld, B, H, W, C, k, s, _p(sums), _p(ws), need, None) == OK
            got = y.check("y")
            _within(got, lr.dw_forward(d["x"], d["w"], None, k, s, d["a"], d["b"], 1), f"dw_forward_stats ld={ld} k{k} s{s}")
            _stats_sums_check(_np(sums)[:2 * C], got, 3, "gauss", f"dw_forward_stats ld={ld}")
            assert np.array_equal(_np(rows_view), d["x"].reshape(64, C))
            if s == 1:
                rows_view.copy_(_dev(d["dy"].reshape(64, C)))
                dx = Mat(64, C, "dense")
                assert lib.fear_dw_backward_data(_p(big), ld, _p(w), dx.p, dx.ld, B, H, W, C, k, s, None) == OK
                _within(dx.check("dx"), lr.dw_backward_data(d["dy"], d["w"], H, W, k, s), f"dw_backward_data ld={ld} k{k}")


# ---------------------------------------------------------------------------------------------------------------------------
# the stem's im2col


@gpu
@pytest.mark.parametrize("case", lr.STEM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_stem_im2col(case):
    """rows of 28 = the float64 gather exactly, column 27 zero, nothing behind the last row; odd H or W: FEAR_TRAIN_ERR_SHAPE"""
    lib = _lib()
    n, H, W = case
    img = np.random.default_rng(7000 + H).standard_normal((n, 3, H, W)).astype(np.float32)
    rows = n * (H // 2) * (W // 2)
    out, x = _sent(rows + GUARD, 28), _dev(img)
    assert lib.fear_stem_im2col(_p(x), _p(out), n, H, W, None) == OK
    got = _np(out)
    assert (got[rows:] == SENTINEL).all() and np.array_equal(got[:rows].astype(f64), lr.stem_im2col(img.astype(f64))) and not got[:rows, 27].any()
    again = _sent(rows + GUARD, 28)
    assert lib.fear_stem_im2col(_p(x), _p(again), n, H, W, None) == OK and np.array_equal(_np(again), got)
    fresh = _sent(rows + GUARD, 28)
    for h, w in ((H + 1, W), (H, W + 1), (1, W)):
        assert lib.fear_stem_im2col(_p(x), _p(fresh), n, h, w, None) == ERR_SHAPE
    assert lib.fear_stem_im2col(_p(x), _p(fresh), 0, H, W, None) == OK and _untouched(fresh)


# ---------------------------------------------------------------------------------------------------------------------------
# argument checks: every buffer is far larger than any of these calls could reach if it were NOT rejected


@gpu
def test_argument_checks_and_empty_calls():
    """Every leading dimension of every operator ON ITS OWN below its width and no multiple of 4 floats, and C = 1028 for the column
    reductions: FEAR_TRAIN_ERR_SHAPE before anything is launched.  No rows (M = 0; B = 0 for the depthwise operators): FEAR_TRAIN_OK from
    every operator, nothing launched and nothing written (include/fear_train.h states it).  Every output stays untouched throughout."""
    lib = _lib()
    n = 1 << 21
    src, vec = torch.ones(n, device="cuda:0"), torch.ones(4096, device="cuda:0")
    out, out2, ws, d64 = _sent(n), _sent(8192), _sent(n), _sent(8192, dtype=torch.float64)
    S, V, O, O2, WS, D = _p(src), _p(vec), _p(out), _p(out2), _p(ws), _p(d64)
    nb = n * 4
    # name -> (the width each pitch must cover, in the order the lambda takes them: k, n or c; the call)
    ops = {
        "pw_forward": ("kn", lambda L, M, B, K, N, C: lib.fear_pw_forward(S, L[0], V, V, O, L[1], M, K, N, None)),
        "pw_backward_data": ("nkk", lambda L, M, B, K, N, C: lib.fear_pw_backward_data(S, L[0], V, S, L[1], O, L[2], M, K, N, None)),
        "pw_backward_weight": ("nk", lambda L, M, B, K, N, C: lib.fear_pw_backward_weight(S, L[0], S, L[1], O, WS, nb, M, K, N, None)),
        "pw_backward_weight_act": ("nk", lambda L, M, B, K, N, C: lib.fear_pw_backward_weight_act(S, L[0], S, L[1], V, V, 1, O, WS, nb, M, K, N, None)),
        "pw_forward_stats": ("kn", lambda L, M, B, K, N, C: lib.fear_pw_forward_stats(S, L[0], V, V, 1, V, O, L[1], M, K, N, D, WS, nb, None)),
        "col_sum": ("c", lambda L, M, B, K, N, C: lib.fear_col_sum(S, L[0], O2, WS, nb, M, C, None)),
        "bn_train_forward": ("cc", lambda L, M, B, K, N, C: lib.fear_bn_train_forward(S, L[0], V, V, O, L[1], O2, O2, None, None, MOM, EPS, M, C, 1, WS, nb, None)),
        "bn_train_backward": ("cccc", lambda L, M, B, K, N, C: lib.fear_bn_train_backward(S, L[0], S, L[1], S, L[2], V, V, V, O, L[3], O2, O2, M, C, WS, nb, None)),
        "bn_train_forward_ab": ("ccc", lambda L, M, B, K, N, C: lib.fear_bn_train_forward_ab(S, L[0], V, V, 1, S, L[1], O, L[2], O2, O2, O2, O2, None, None, MOM, EPS,
                                                                                             M, C, WS, nb, None)),
        "bn_train_backward_x": ("ccc", lambda L, M, B, K, N, C: lib.fear_bn_train_backward_x(S, L[0], S, L[1], V, V, 1, V, V, V, O, L[2], O2, O2, M, C, WS, nb, None)),
        "bn_backward_reduce_x": ("cc", lambda L, M, B, K, N, C: lib.fear_bn_backward_reduce_x(S, L[0], S, L[1], V, V, 1, V, V, D, M, C, WS, nb, None)),
        "bn_backward_apply_x": ("ccc", lambda L, M, B, K, N, C: lib.fear_bn_backward_apply_x(S, L[0], S, L[1], V, V, 1, V, V, V, D, float(max(M, 1)), D, O, L[2], O2, O2,
                                                                                             WS, nb, M, C, None)),
        "bn_act": ("ccc", lambda L, M, B, K, N, C: lib.fear_bn_act(S, L[0], V, V, 1, S, L[1], O, L[2], M, C, None)),
        "dw_forward": ("cc", lambda L, M, B, K, N, C: lib.fear_dw_forward(S, L[0], V, V, O, L[1], B, 8, 8, C, 3, 1, None)),
        "dw_forward_stats": ("cc", lambda L, M, B, K, N, C: lib.fear_dw_forward_stats(S, L[0], V, V, 1, V, O, L[1], B, 8, 8, C, 3, 1, D, WS, nb, None)),
        "dw_backward_data": ("cc", lambda L, M, B, K, N, C: lib.fear_dw_backward_data(S, L[0], V, O, L[1], B, 8, 8, C, 3, 1, None)),
        "dw_backward_weight": ("cc", lambda L, M, B, K, N, C: lib.fear_dw_backward_weight(S, L[0], S, L[1], O2, WS, nb, B, 8, 8, C, 3, 1, None)),
        "dw_backward_weight_act": ("cc", lambda L, M, B, K, N, C: lib.fear_dw_backward_weight_act(S, L[0], S, L[1], V, V, 1, O2, WS, nb, B, 8, 8, C, 3, 1, None)),
    }
    good = dict(M=64, B=1, K=8, N=8, C=8)

    def pitches(kinds, shape):
        return [shape[k.upper()] for k in kinds]

    for name, (kinds, call) in ops.items():
        for slot in range(len(kinds)):
            for delta in (-4, 2):                            # shorter than its row; no multiple of 4 floats
                L = pitches(kinds, good)
                L[slot] += delta
                assert call(L, **good) == ERR_SHAPE, (name, "pitch", slot, L)
        if name.startswith(("col_", "bn_")) and name != "bn_act":
            wide = dict(good, C=1028)
            assert call(pitches(kinds, wide), **wide) == ERR_SHAPE, (name, "C = 1028")
        empty = dict(good, M=0, B=0)
        assert call(pitches(kinds, empty), **empty) == OK, (name, "no rows")
    assert _untouched(out) and _untouched(out2) and _untouched(ws) and _untouched(d64)
    assert bool((src == 1).all()) and bool((vec == 1).all())
    # the same arguments without the defect are accepted: the rejections above are not the buffers' or the base shape's
    for name, (kinds, call) in ops.items():
        assert call(pitches(kinds, good), **good) == OK, name
    torch.cuda.synchronize()
    assert not _untouched(out[:64])
