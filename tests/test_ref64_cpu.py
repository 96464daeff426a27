"""The float64 reference (oracle/fear_ref64.py) on the CPU: its rounding helpers on their edges, its mode 0 against the fp32 oracle
and the golden fixtures, and the mutation argument: on the inputs the GPU tests use, every block and head mutant (a kernel defect
the reference can model) lies at least 3x the GPU tests' bound away from the faithful reference, in the metric that bound is
stated in, so a kernel with that defect would be at least 2x its tolerance off and fail.  The storage mutant does not reach
that separation (test_storage_mutant_against_the_measured_kernel_distance).  For modes 0 and 1: what fp32 accumulation of
the neck + head costs against float64 when torch does it, and the mode-0 / mode-1 mutants against the GPU test's median bounds."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from blocktaps import edge_crops, trunk_length, write_truncated
from oracle.fear_oracle import (ACT_EXP, ROLE_BBOX_PRED, ROLE_BBOX_TOWER, ROLE_CLS_CORR, ROLE_CLS_ENCODE, ROLE_CLS_PRED,
                                ROLE_CLS_TOWER, ROLE_REG_CORR, ROLE_REG_ENCODE)
from oracle.fear_ref64 import (MUTANTS, Ref64Net, max_rel, round_bf16, round_fp16, split_fp16, to_fp32,
                               trunc_bf16)
from test_ref64_gpu import (FRAC_BLOCK2, PASS_SIZES, STORAGE_MEASURED, STORAGE_RATIO, TOL_HEAD01, TOL_HEAD01_MEDIAN, TOL_HEAD2,
                            TOL_HEAD2_MEDIAN, checked_crops, deviation, head01_arith, median_deviation, stored_bf16_units)

F32 = np.float32


def bf16_rne_bits(x: np.ndarray) -> np.ndarray:
    """fear_engine.hip `float_to_bf16`, restated on uint32 (NaN kept quiet NaN, inf stays inf)."""
    u = x.astype(F32).view(np.uint32).astype(np.uint64)
    nan_or_inf = (u & 0x7F800000) == 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    special = (u >> 16) | np.where((u & 0xFFFF) != 0, np.uint64(0x40), np.uint64(0))
    return np.where(nan_or_inf, special, r).astype(np.uint16)


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.to(torch.float32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def f32(bits: int) -> float:
    return float(np.array([bits], dtype=np.uint32).view(F32)[0])


# ------------------------------------------------------------------------------------------------------ rounding helpers
def test_bf16_rounding_matches_the_engines_rne_on_edges_and_random_values():
    edges = [
        f32(0x3F808000),            # tie, even neighbour below (1.0): stays
        f32(0x3F818000),            # tie, odd neighbour below: rounds up to even
        f32(0x3F808001), f32(0x3F807FFF),   # just above / below a tie
        0.0, -0.0,
        f32(0x00000001), f32(0x00008000), f32(0x00018000), f32(0x007FFFFF),   # subnormals, ties among them
        f32(0x7F7FFFFF),            # largest finite fp32: overflows to inf
        f32(0x7F7F7FFF),            # just below the overflow tie: largest finite bf16
        float("inf"), -float("inf"), float("nan"),
    ]
    x = np.array(edges, dtype=F32)
    x = np.concatenate([x, -x])
    got = bf16_bits(torch.from_numpy(x))
    want = bf16_rne_bits(x)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.all((got[nan] & 0x7F80) == 0x7F80) and np.all(got[nan] & 0x7F)      # NaN stays NaN
    r = np.random.RandomState(0)
    bits = r.randint(0, 2 ** 32, size=2 ** 20, dtype=np.uint64).astype(np.uint32)
    bits = bits[(bits & 0x7F800000) != 0x7F800000]
    v = bits.view(F32)
    assert np.array_equal(bf16_bits(torch.from_numpy(v)), bf16_rne_bits(v))
    # the helper itself: fp32 first, then bf16, values back in float64
    assert round_bf16(torch.tensor([1.0 + 2 ** -8], dtype=torch.float64)).item() == 1.0            # tie to even (down)
    assert round_bf16(torch.tensor([1.0 + 3 * 2 ** -8], dtype=torch.float64)).item() == 1.0 + 2 ** -6   # tie to even (up)
    # double rounding through fp32: 1 + 2^-8 + 2^-40 is 1 + 2^-8 in fp32, a tie, rounded to even -> 1.0
    assert round_bf16(torch.tensor([1.0 + 2 ** -8 + 2 ** -40], dtype=torch.float64)).item() == 1.0
    assert trunc_bf16(torch.tensor([1.0 + 255 * 2 ** -15], dtype=torch.float64)).item() == 1.0
    assert trunc_bf16(torch.tensor([-(1.0 + 255 * 2 ** -15)], dtype=torch.float64)).item() == -1.0


def test_fp16_rounding_and_split_on_edges():
    h = lambda v: round_fp16(torch.tensor([v], dtype=torch.float64)).item()
    assert h(1.0 + 2 ** -11) == 1.0 and h(1.0 + 3 * 2 ** -11) == 1.0 + 2 ** -9        # ties to even
    assert h(1.0 + 2 ** -11 + 2 ** -20) == 1.0 + 2 ** -10                             # just above a tie
    assert h(1.0 + 2 ** -11 - 2 ** -20) == 1.0                                        # just below
    assert h(65504.0) == 65504.0 and h(65519.0) == 65504.0 and h(65520.0) == float("inf")    # largest finite, overflow tie
    assert h(2 ** -24) == 2 ** -24 and h(2 ** -25) == 0.0 and h(3 * 2 ** -25) == 2 ** -23   # subnormal ties to even
    assert np.signbit(h(-0.0)) and h(0.0) == 0.0 and not np.signbit(h(0.0))
    assert h(float("inf")) == float("inf") and np.isnan(h(float("nan")))
    # hi + lo of split_half8: 11 + 11 significant bits (lo may be subnormal in fp16 for small x)
    r = np.random.RandomState(1)
    x = torch.from_numpy(r.uniform(-100, 100, 4096)).to(torch.float32).to(torch.float64)
    hi, lo = split_fp16(x)
    assert torch.equal(hi, round_fp16(x))
    assert float(((hi + lo - x).abs() / x.abs()).max()) <= 2.0 ** -16   # lo keeps 11 of the remaining 13 bits
    assert torch.equal(to_fp32(torch.tensor([1.0 + 2 ** -30], dtype=torch.float64)), torch.tensor([1.0], dtype=torch.float64))


# ------------------------------------------------------------------------------------------------ mode 0 against the oracle
def _norm(u8):
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1) * 255.0
    inv = 1.0 / (torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1) * 255.0)
    return (u8.float() - mean) * inv


def test_mode0_reference_matches_the_fp32_oracle_and_the_golden_fixtures(golden_dir, oracle_net):
    """Mode 0 (no rounding) is the network itself: the trunk taps and maps of the fixtures at the fixtures' fp32 accuracy, and
    the fp32 oracle block by block at fp32 summation-order distance."""
    from conftest import WEIGHTS
    ref = Ref64Net(WEIGHTS)
    d = np.load(os.path.join(golden_dir, "trunk_taps.npz"))
    img = torch.from_numpy(d["image"])
    x = ref.conv(ref.trunk[0]["conv"][0], img.double())
    close = lambda a, b: max_rel(torch.as_tensor(a), torch.as_tensor(b)) < 2e-5      # fp32 accuracy, in the tensor's scale
    assert close(x, d["block00"])
    ora = []
    oracle_net.feature_extractor(img, ora)
    for k in range(1, len(ref.trunk)):
        x = ref.ir_block(k, x, 0)
        assert close(x, d[f"block{k:02d}"]), k
        assert max_rel(ora[k], x) < 1e-5, k
    m = np.load(os.path.join(golden_dir, "track_maps.npz"))
    s = _norm(torch.from_numpy(m["search_u8"][:2]))
    z = torch.from_numpy(m["template_features"][:2])
    feat = ref.neck_out(ref.trunk_out(s), 0)
    bbox, cls = ref.head_maps(feat, z, None, 0, 0)
    assert close(bbox, m["bbox"][:2]) and close(cls, m["cls"][:2])
    zt = ref.neck_out(ref.trunk_out(_norm(torch.from_numpy(m["template_u8"][:2]))), 0)
    assert close(zt, m["template_features"][:2])


def test_truncated_model_is_the_trunk_up_to_its_cut(tmp_path, oracle_net):
    """The identity-neck cut of tests/blocktaps.py computes block k's output (fp32 oracle on the written file)."""
    from conftest import WEIGHTS
    from oracle.fear_oracle import OracleNet
    x = edge_crops(3, 128)
    taps = []
    oracle_net.feature_extractor(x, taps)
    for k in (1, 5, trunk_length(WEIGHTS) - 1):
        p = str(tmp_path / f"cut{k}.fearw")
        c = write_truncated(WEIGHTS, k, p)
        out = OracleNet(p).get_features(x)
        assert out.shape[1] == c and torch.equal(out, taps[k])


# ----------------------------------------------------------------------------------------------------------------- mutants
MUTANT_FACTOR = 3.0


def _mode2_taps(ref, x):
    """The reference's own mode-2 trunk (every block with expansion on the matrix pipe): the inputs of the blocks."""
    ariths = [0, 0] + [2 if ref.expands(k) else 0 for k in range(2, len(ref.trunk))]
    taps = []
    ref.trunk_out(x, ariths, taps=taps)
    return taps


@pytest.mark.parametrize("model", ("fear_xs", "fear_m"))
def test_block_mutants_are_far_outside_the_block_tolerance(model):
    """For every block the GPU test runs on the bf16 matrix pipe, on the GPU test's crops (tests/blocktaps.edge_crops, 128-pixel
    and 256-pixel): each block-level mutant moves at least MUTANT_FACTOR x FRAC_BLOCK2 of the output elements past the mode-0
    bound — a kernel with that defect fails the GPU test.  Measured: at least 0.80 (residual added after rounding, FEAR-XS),
    0.95 .. 0.98 for the others.  (The residual mutant applies to residual blocks only.)"""
    from test_ref64_gpu import _models
    ref = Ref64Net(_models()[model])
    names = ("dw_truncated", "dw_not_rounded", "weights_not_rounded", "expanded_rounded", "residual_after_rounding")
    nearest = {m: float("inf") for m in names}
    for hw in (128, 256):
        x = edge_crops(3, hw, seed=hw)
        taps = _mode2_taps(ref, x)
        seen = set()
        for k in range(2, len(ref.trunk)):
            if not ref.expands(k):
                continue
            key = (tuple(taps[k - 2].shape), tuple(ref.convs[ref.trunk[k]["conv"][1]]["w"].shape))
            if model == "fear_m" and key in seen:
                continue
            seen.add(key)
            want = ref.ir_block(k, taps[k - 2], 2)
            for m in names:
                if m == "residual_after_rounding" and not ref.trunk[k]["residual"]:
                    continue
                _, frac = deviation(ref.ir_block(k, taps[k - 2], 2, MUTANTS[m]), want)
                nearest[m] = min(nearest[m], frac)
    print("REF64 block mutants " + model + ": " + " ".join(f"{m} {v:.3e}" for m, v in nearest.items()))
    for m, v in nearest.items():
        assert v >= MUTANT_FACTOR * FRAC_BLOCK2, (m, v, FRAC_BLOCK2)


@pytest.mark.parametrize("plan", ("small", "throughput"))
def test_head_mutants_are_far_outside_the_head_tolerance(plan):
    """FEAR-XS neck + head in mode 2 on the GPU head test's crops, with each plan's roundings (small-batch plans: neck and
    correlation fp32; throughput plan: both bf16).  Every head mutant's MEDIAN deviation is at least MUTANT_FACTOR x the plan's
    TOL_HEAD2_MEDIAN: measured 2.4e-4 and above in the throughput plan (bound 1e-6), 2.8e-4 and above in the small-batch plans
    (bound 8.5e-5).  The template operand of the correlation is rounded only in the throughput plan.  Their MAX deviations are
    printed as well: only truncation exceeds TOL_HEAD2, the max bound alone would miss the others."""
    from conftest import WEIGHTS
    ref = Ref64Net(WEIGHTS)
    n = 17 if plan == "small" else 6
    sel = checked_crops(n)
    x = edge_crops(n, 256, seed=7)[sel]
    t = edge_crops(n, 128, seed=8)[sel]
    ar = 2 if plan == "throughput" else 0
    z = ref.neck_out(ref.trunk_out(t), 0)
    trunk = ref.trunk_out(x)
    want = ref.head_maps(ref.neck_out(trunk, ar), z, None, 2, ar)
    medians, maxes = {}, {}
    names = ("dw_truncated", "dw_not_rounded", "weights_not_rounded") + (("corr_template_not_rounded",) if ar else ())
    for m in names:
        rnd = MUTANTS[m]
        got = ref.head_maps(ref.neck_out(trunk, ar, rnd), z, None, 2, ar, rnd)
        # the larger of the two maps': a kernel with the defect fails the GPU test when either map is past the bound
        medians[m] = max(median_deviation(got[0], want[0]), median_deviation(got[1], want[1]))
        maxes[m] = max(deviation(got[0], want[0])[0], deviation(got[1], want[1])[0])
    print(f"REF64 head mutants {plan} median: " + " ".join(f"{m} {v:.3e}" for m, v in medians.items()))
    print(f"REF64 head mutants {plan} max: " + " ".join(f"{m} {v:.3e}" for m, v in maxes.items()))
    for m, v in medians.items():
        assert v >= MUTANT_FACTOR * TOL_HEAD2_MEDIAN[plan], (m, v, TOL_HEAD2_MEDIAN[plan])
    assert maxes["dw_truncated"] >= TOL_HEAD2


# ------------------------------------------------------------------------------------- modes 0 and 1: the neck and the head
HEAD01_N = {"tiny": 3, "small": 17, "throughput": 6, "throughput_fused": 6}      # one pass size of the GPU test per plan kind


@functools.lru_cache(maxsize=None)
def _head01_all():
    """FEAR-XS: the reference, and the float64 trunk output / template features of every crop the GPU head test checks at the
    pass sizes of HEAD01_N (its crops: the first n of edge_crops(97, hw, seed=hw))."""
    from conftest import WEIGHTS
    ref = Ref64Net(WEIGHTS)
    rows = sorted({i for n in HEAD01_N.values() for i in checked_crops(n)})
    x = edge_crops(max(PASS_SIZES), 256, seed=256)[rows]
    t = edge_crops(max(PASS_SIZES), 128, seed=128)[rows]
    return ref, rows, ref.trunk_out(x), ref.neck_out(ref.trunk_out(t), 0)


def _head01_inputs(kind):
    ref, rows, trunk, z = _head01_all()
    pick = [rows.index(i) for i in checked_crops(HEAD01_N[kind])]
    return ref, trunk[pick], z[pick]


def _head32(ref, trunk, z, mode, neck_arith, corr_arith):
    """Ref64Net's own neck + head formula (`neck_out`, `head_maps` with the default roundings) evaluated in fp32 by torch:
    what fp32 accumulation of this head costs against float64, measured without a kernel."""
    f32 = lambda v: None if v is None else v.to(torch.float32)

    def opnd(v, arith):
        if arith == 1:
            hi = v.to(torch.float16).to(torch.float32)
            return hi + (v - hi).to(torch.float16).to(torch.float32)
        return v

    def pw(idx, v, arith):
        c = ref.convs[idx]
        y = F.conv2d(opnd(v, arith), f32(c["w"]), f32(c["b"]))
        return F.relu(y) if c["relu"] else y

    def sep(b, v):
        c = ref.convs[b["conv"][0]]
        d = F.conv2d(v, f32(c["w"]), f32(c["b"]), stride=c["stride"], padding=c["pad"], groups=c["groups"])
        y = pw(b["conv"][1], F.relu(d) if c["relu"] else d, mode)
        return torch.exp(y) if b["act"] == ACT_EXP else y

    def corr(zz, v):
        b, c, hh, ww = v.shape
        zf = lambda q: q.reshape(q.size(0), q.size(1), -1).permute(0, 2, 1)
        xf = lambda q: q.reshape(b, c, -1)
        if corr_arith == 1:
            zh, xh = zz.to(torch.float16).to(torch.float32), v.to(torch.float16).to(torch.float32)
            zl, xl = (zz - zh).to(torch.float16).to(torch.float32), (v - xh).to(torch.float16).to(torch.float32)
            s = zf(zh) @ xf(xh) + zf(zh) @ xf(xl) + zf(zl) @ xf(xh)
        else:
            s = zf(zz) @ xf(v)
        return s.view(b, -1, hh, ww)

    feat = pw(ref.neck["conv"][0], f32(trunk), neck_arith)
    zz = f32(z)
    out = []
    for enc, cr, tower, pred in ((ROLE_REG_ENCODE, ROLE_REG_CORR, ROLE_BBOX_TOWER, ROLE_BBOX_PRED),
                                 (ROLE_CLS_ENCODE, ROLE_CLS_CORR, ROLE_CLS_TOWER, ROLE_CLS_PRED)):
        v = sep(ref.head[enc][0], feat)
        y = sep(ref.head[cr][0], torch.cat([v, corr(zz, v)], dim=1))
        for tb in ref.head.get(tower, []):
            y = sep(tb, y)
        out.append(sep(ref.head[pred][0], y))
    return out[0], out[1]


def test_fp32_evaluations_of_the_head_lie_at_fp32_distance_from_float64(oracle_net):
    """The size of "fp32 accumulation against float64" for the FEAR-XS neck + head, measured without the code under test, on
    the GPU head test's crops (small plan, 5 crops; throughput plan, 5 crops): the fp32 `OracleNet`, and torch's fp32
    evaluation of Ref64Net's own formula in modes 0 and 1 at each plan's arithmetic, against Ref64Net in float64 (in map
    scale, the larger of the two maps').  Measured: oracle 1.16e-6 max / 4.4e-8 median; formula, mode 0: the same (it is the
    same arithmetic), mode 1 small-batch: 1.18e-6 / 4.6e-8, mode 1 throughput: 1.15e-6 / 4.5e-8.  A kernel 50x and more above
    these is a finding, not something to set a bound around (the kernels: at most 2.4e-6 / 1.6e-7 on these weights).
    Asserted: every one below 1e-5 max and 1e-6 median."""
    rows = []
    for kind, mode in (("small", 0), ("small", 1), ("throughput", 1)):
        ref, trunk, z = _head01_inputs(kind)
        neck_arith, corr_arith = head01_arith(mode, kind, 16)
        want = ref.head_maps(ref.neck_out(trunk, neck_arith), z, None, mode, corr_arith)
        got = _head32(ref, trunk, z, mode, neck_arith, corr_arith)
        rows.append((f"formula mode {mode} {kind}", got, want))
        if mode == 0:
            feat = oracle_net._conv(oracle_net.neck[0]["conv"][0], trunk.float())
            rows.append(("oracle", oracle_net.connector(z.float(), feat, return_all=True)[:2], want))
    for name, got, want in rows:
        mx = max(deviation(got[0], want[0])[0], deviation(got[1], want[1])[0])
        med = max(median_deviation(got[0], want[0]), median_deviation(got[1], want[1]))
        print(f"REF64 head fp32 evaluation, {name}: max {mx:.3e} median {med:.3e}")
        assert mx < 1e-5 and med < 1e-6, (name, mx, med)


HEAD01_MUTANTS = {0: ("operand_fp16", "operand_bf16"), 1: ("split_lo_dropped", "corr_cross_dropped", "corr_lolo_kept")}


@pytest.mark.parametrize("mode,kind", [(0, "tiny"), (0, "small"), (0, "throughput"), (0, "throughput_fused"),
                                       (1, "tiny"), (1, "small"), (1, "throughput")])
def test_mode01_head_mutants_against_the_head_tolerance(mode, kind):
    """FEAR-XS neck + head in modes 0 and 1 on the GPU head test's crops, at each plan's arithmetic (`head01_arith`).  Mode 0: a
    neck / pointwise operand rounded to fp16 or bf16 (a reduced-precision kernel launched in fp32 mode).  Mode 1: the lo half
    of the split dropped from every GEMM activation operand; in the throughput plan, where the correlation is a split GEMM
    (the small-batch plans run it in fp32), also the correlation without its hi x lo cross terms.  Every such mutant's
    MEDIAN deviation from the faithful reference is at least MUTANT_FACTOR x TOL_HEAD01_MEDIAN of its mode and plan kind
    (3): measured medians 3.2e-5 .. 3.5e-5 (fp16 operand), 2.7e-4 (bf16 operand), 3.3e-5 .. 3.6e-5 (lo dropped), 1.2e-5 (cross
    terms dropped) against bounds of 6e-7 .. 1e-6, factors of 17 and more; their max deviations (2.7e-4 .. 5.2e-3, printed)
    are past the max bounds as well.
    `corr_lolo_kept` (the correlation adds lo x lo, 2^-22 of a product) is out of reach by construction: it is asserted to
    lie BELOW both bounds, so that nobody reads the test as claiming it."""
    ref, trunk, z = _head01_inputs(kind)
    neck_arith, corr_arith = head01_arith(mode, "throughput" if kind == "throughput_fused" else kind, 16)
    want = ref.head_maps(ref.neck_out(trunk, neck_arith), z, None, mode, corr_arith)
    medians, maxes = {}, {}
    for m in HEAD01_MUTANTS[mode]:
        if m.startswith("corr_") and corr_arith != 1:
            continue
        rnd = MUTANTS[m]
        got = ref.head_maps(ref.neck_out(trunk, neck_arith, rnd), z, None, mode, corr_arith, rnd)
        medians[m] = max(median_deviation(got[0], want[0]), median_deviation(got[1], want[1]))
        maxes[m] = max(deviation(got[0], want[0])[0], deviation(got[1], want[1])[0])
    print(f"REF64 head mutants mode {mode} {kind} median: " + " ".join(f"{m} {v:.3e}" for m, v in medians.items()))
    print(f"REF64 head mutants mode {mode} {kind} max: " + " ".join(f"{m} {v:.3e}" for m, v in maxes.items()))
    bound = TOL_HEAD01_MEDIAN[mode][kind]
    for m, v in medians.items():
        if m == "corr_lolo_kept":
            assert v < bound and maxes[m] < TOL_HEAD01[mode][kind], (m, v, maxes[m])
        else:
            assert v >= MUTANT_FACTOR * bound, (m, v, bound)


def test_storage_mutant_against_the_measured_kernel_distance():
    """The mutant "no storage rounding" on the storage test's FEAR-M crops and metric (mean over the crops of the per-crop max
    deviation of the maps): 2.4e-2 from the faithful whole-network reference.  The kernels sit 1.74e-2 from it
    (STORAGE_MEASURED), so the mutant is only 1.4x away, not 3x: through 28 blocks the kernels' own bf16 boundary crossings
    grow to the size of the storage roundings.  Asserted: the storage rule gives the seven tensors, and the mutant lies farther
    from the faithful reference than STORAGE_MEASURED / STORAGE_RATIO (2.2e-2)."""
    from feartracker_amd.hip_backend import WEIGHTS_FEAR_M
    from oracle.fear_ref64 import EXACT
    ref = Ref64Net(WEIGHTS_FEAR_M)
    n = 8
    x = edge_crops(n, 256, seed=11)
    t = edge_crops(n, 128, seed=12)
    ariths = [0, 0] + [2 if ref.expands(k) else 0 for k in range(2, len(ref.trunk))]
    ops = ["stem_irt"] + ["irt_" if k <= 15 else "ir16_" for k in range(2, len(ref.trunk))]     # FEAR-M: tiles up to block 15
    stored = stored_bf16_units(ops, ref)
    assert stored == [1, 2, 3, 4, 5, 6, 7], stored
    z = ref.neck_out(ref.trunk_out(t, ariths), 0)
    maps = {}
    for key, rnd in (("with", EXACT), ("without", MUTANTS["no_storage_rounding"])):
        tr = ref.trunk_out(x, ariths, rnd, stored_bf16=stored)
        maps[key] = ref.head_maps(ref.neck_out(tr, 2, rnd), z, None, 2, 2, rnd)
    per_crop = [max(deviation(maps["without"][0][i:i + 1], maps["with"][0][i:i + 1])[0],
                    deviation(maps["without"][1][i:i + 1], maps["with"][1][i:i + 1])[0]) for i in range(n)]
    d = float(np.mean(per_crop))
    print(f"REF64 storage mutant: {d:.3e} (kernels at {STORAGE_MEASURED:.3e})")
    assert d >= STORAGE_MEASURED / STORAGE_RATIO, d
