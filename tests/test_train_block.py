"""Block-fused operators of the trunk's training step (include/fear_train.h `fear_irb_*`, `fear_pwbn_*`; csrc/fear_train_block.h)
against torch autograd on one inverted-residual block (model_training/model/blocks.py:22-35 over mobile_cv's conv-BN-ReLU units:
expand 1x1 + BN + ReLU, depthwise + BN + ReLU, project 1x1 + BN [+ input]) — every shape class of the FEAR-XS trunk (SURVEY.md
Appendix A): with / without expansion, 3x3 / 5x5, stride 1 / 2, residual or not, maps of 8 ... 64 pixels, ragged channel slabs.
The whole network in this mode is pinned by tests/test_train_head.py::test_whole_network_training_step_matches_autograd.
The launch code picks kernels and grids from the row count: LARGE_CASES are the smallest shapes above each of its thresholds, and
test_cases_reach_the_paths_they_claim holds them to the plan the library reports.  Every buffer a call writes sits between guard regions."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from syncref import pwbn_autograd, sepbn_autograd, stem_autograd


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# Guard regions: every buffer a call may write (workspace, scratch, saved tensors, outputs, gradients) is cut out of an allocation
# with GUARD floats of a fixed finite sentinel on either side, at exactly the size the library reports or the shape implies — a write
# one element past the end lands in the guard instead of the allocator's padding, and _Guarded.check finds it.
GUARD = 256
SENTINEL = 12345.678
_SENTINEL_BITS = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()


class _Guarded:
    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def alloc(self, name, *shape, fill=None):
        n = math.prod(shape)
        buf = torch.full((n + 2 * GUARD,), SENTINEL, device=self.dev)
        view = buf[GUARD:GUARD + n].view(*shape)
        if fill is not None:
            view.fill_(fill)
        self.bufs.append((name, buf, n))
        return view

    def check(self, when):
        """Every guard is bit-unchanged (the caller has synchronised)."""
        touched = []
        for name, buf, n in self.bufs:
            bits = buf.view(torch.int32)
            if not bool(((bits[:GUARD] == _SENTINEL_BITS).all() & (bits[GUARD + n:] == _SENTINEL_BITS).all()).item()):
                bad = torch.nonzero(bits != _SENTINEL_BITS).flatten()
                bad = bad[(bad < GUARD) | (bad >= GUARD + n)] - GUARD
                touched.append((name, n, bad[:4].tolist(), int(bad.numel())))
        assert not touched, f"guard regions written {when}: (buffer, its floats, first offsets, count) {touched}"


# The kinks of the two ReLUs.  Where a BatchNorm's output z is within fp32 rounding of zero, float64 and fp32 arithmetic may see
# different signs; relu(z) is the same to that rounding either way, but the derivative is 0 or 1, and ONE such element moves the
# input gradient at its pixel by percents of the tensor's max-norm and every parameter gradient by ~1 / sqrt(rows).  Among the 5 * 10^7
# activations of a large case a handful sit that close (expected: elements x density at zero x 2^-23; the small cases have none), so
# there, and only there, the derivative is undefined to the precision of the operator under test, and the reference takes the side the
# operator took — read from the masked gradients the backward leaves in its scratch, exact zeros where masked (g2 | g1, csrc/
# fear_train_block.h IrbScratch).  The band: z ends a chain of at most 2^8 fp32 roundings (a 1 x 1 conv of up to 192 terms or 25 taps,
# the statistics, the affine), so |fp32 z - float64 z| <= 2^8 * 2^-24 = 2^-16 of the largest |z|; a sign the operator gets wrong
# outside the band still fails the test.
KINK_BAND = 2.0 ** -16


class _ReluTakingSides(torch.autograd.Function):
    """relu(z) with the derivative taken the other way at the flat indices `flip`."""
    @staticmethod
    def forward(ctx, z, flip):
        mask = z > 0
        mask.view(-1)[flip] ^= True
        ctx.save_for_backward(mask)
        return z.clamp_min(0)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None


def _torch_block(x, p, cfg, train_stats, flips=None, pre=None):
    """`pre` (a dict) receives the inputs of the two ReLUs; `flips`: per ReLU the flat indices whose derivative goes the other way."""
    cin, cexp, cout, k, stride, expand, residual = cfg

    def relu(z, name):
        if pre is not None:
            pre[name] = z.detach()
        return _ReluTakingSides.apply(z, flips[name]) if flips and name in flips else F.relu(z)
    y = x
    if expand:
        y = F.conv2d(y, p["w_pw"].view(cexp, cin, 1, 1))
        y = relu(F.batch_norm(y, train_stats["rm0"], train_stats["rv0"], p["g0"], p["b0"], True, 0.1, 1e-5), "act1")
    y = F.conv2d(y, p["w_dw"].t().reshape(cexp, 1, k, k), stride=stride, padding=k // 2, groups=cexp)
    y = relu(F.batch_norm(y, train_stats["rm1"], train_stats["rv1"], p["g1"], p["b1"], True, 0.1, 1e-5), "act2")
    y = F.conv2d(y, p["w_pwl"].view(cout, cexp, 1, 1))
    y = F.batch_norm(y, train_stats["rm2"], train_stats["rv2"], p["g2"], p["b2"], True, 0.1, 1e-5)
    return y + x if residual else y


CASES = [
    # cin, cexp, cout, k, stride, expand, residual,   B, H
    ((16, 16, 16, 3, 1, 0, 1), 2, 64),       # stage 1: no expansion, 16 channels = one ragged slab
    ((16, 96, 24, 3, 2, 1, 0), 3, 32),       # stage 2: the widest expansion of the large maps, stride 2
    ((24, 24, 24, 3, 1, 0, 1), 2, 32),       # e1 blocks: 24 channels = 1.5 slabs
    ((24, 144, 32, 5, 2, 1, 0), 2, 32),      # 5x5 stride 2, 144 = 9 slabs of 16
    ((32, 192, 32, 5, 1, 1, 1), 2, 16),      # 5x5 stride 1, residual, 32-channel slabs
    ((32, 192, 32, 3, 1, 1, 1), 3, 32),
    ((32, 192, 64, 5, 2, 1, 0), 2, 32),
    ((64, 384, 112, 5, 1, 1, 0), 3, 16),
    ((112, 672, 112, 5, 1, 1, 1), 2, 8),     # the template branch's last stage: the 16 x 16 tile overhangs the 8 x 8 map
    ((112, 336, 112, 5, 1, 1, 1), 5, 16),    # 336 = 21 slabs of 16, odd crop count
]


# ... and the expansions of the large maps once more in the E-free form of BatchNorm1's backward (FEAR_IRB_LINEAR_BN1: the call
# chooses it by itself for up to 32 input channels).  The 81 920-row case runs the first-generation GEMMs only where the reduction is
# shorter than 32 channels (the expansion, the masked gradient); its projection and input gradient take the LDS-staged kernel, as every
# reduction of 32 channels or more does up to FEAR_GEMM_LDS_MAX_ROWS = 131 072 rows: the first generation at such reductions is
# LARGE_CASES' (C, D, E), and test_cases_reach_the_paths_they_claim holds every such claim to the library's own plan
LIN_CASES = [(c, b, h, 1) for c, b, h in CASES if c[5]] + [((16, 96, 24, 3, 2, 1, 0), 5, 128, 1), ((32, 192, 32, 5, 1, 1, 1), 2, 16, 2)]
# ... and the 16 -> 96 expansion never written (FEAR_IRB_VIRTUAL_E): FearIrbSaved.e = NULL, BatchNorm1's statistics from the Gram matrix
LIN_CASES += [((16, 96, 24, 3, 2, 1, 0), 3, 32, 4), ((16, 96, 24, 3, 2, 1, 0), 5, 128, 4), ((16, 64, 16, 3, 2, 1, 0), 2, 24, 4),
              ((24, 144, 32, 5, 2, 1, 0), 2, 32, 4), ((32, 192, 64, 5, 2, 1, 0), 2, 32, 4), ((32, 128, 48, 3, 2, 1, 0), 3, 16, 4),
              ((20, 80, 24, 5, 2, 1, 0), 2, 24, 4)]
# ... and the narrow blocks' projection weight gradient summed inside the masked-gradient pass (FEAR_IRB_FUSE_W3)
LIN_CASES += [((16, 16, 16, 3, 1, 0, 1), 2, 64, 8), ((24, 24, 24, 3, 1, 0, 1), 2, 32, 8), ((24, 24, 24, 3, 1, 0, 1), 40, 64, 8)]
ALL_CASES = [(c, b, h, 0) for c, b, h in CASES] + LIN_CASES

# The smallest shapes above every row-count threshold of the launch code (csrc/fear_train_block.h stat_grid, fear_train_gemm.h
# gemm_lds_applies, fear_train.hip col_rows_per_block / wgrad_rows_per_slice, launch_gram), with ragged tails: no row count is a
# multiple of 256, no tile count a multiple of row_tiles.  The 128-pair step runs at 2 097 152 ... 32 768 rows per stage, above all of
# them; what each case reaches is LARGE_PLANS below, asserted by test_cases_reach_the_paths_they_claim.  Cases that share a float64
# reference are neighbours (_irb_reference keeps the last one).
#   id: (cfg, B, H, flags, biased)
LARGE_CASES = {
    "A": ((16, 16, 16, 3, 1, 0, 1), 5, 232, 0, False),       # 269 120 rows: 2 103 tiles -> row_tiles 2, 1 052 workgroups, one overhang tile
    "A8": ((16, 16, 16, 3, 1, 0, 1), 5, 232, 8, False),      # ... FEAR_IRB_FUSE_W3 partials summed over two row tiles per workgroup
    "B": ((24, 24, 24, 3, 1, 0, 1), 5, 232, 0, False),       # ... on 1.5 column tiles and two slabs
    "C": ((16, 96, 24, 3, 2, 1, 0), 9, 244, 0, False),       # 535 824 / 133 956 rows: row_tiles 3; first generation at K = 96 and 96 + 16
    "C4": ((16, 96, 24, 3, 2, 1, 0), 9, 244, 4, False),      # ... the virtual expansion: the form the step uses for this block
    "C4b": ((16, 96, 24, 3, 2, 1, 0), 9, 244, 4, True),      # ... on biased, correlated inputs: the Gram-matrix variance at 535 824 rows
    "D": ((24, 144, 32, 5, 2, 1, 0), 9, 172, 0, False),      # 266 256 / 66 564 rows: K = 24 with row_tiles 2; dx first generation, 144 + 24
    "D4": ((24, 144, 32, 5, 2, 1, 0), 9, 172, 4, False),     # ... virtual, two input-channel chunks
    "E0": ((32, 192, 32, 5, 1, 1, 1), 8, 128, 0, False),     # 131 072 rows: the most the LDS GEMMs take (the step's own count for this stage)
    "E": ((32, 192, 32, 5, 1, 1, 1), 9, 122, 0, False),      # 133 956 rows: the first shape above it, every GEMM first generation
}
LARGE_STEM = (5, 464)                                        # "F": 269 120 rows, fear_stem_train_* (and fear_pwbn_train_*) with row_tiles 2


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(LARGE_CASES))
def test_irb_block_above_the_row_count_thresholds(case):
    cfg, B, H, flags, biased = LARGE_CASES[case]
    _irb_case(cfg, B, H, H, flags, biased=biased)


# What the table above claims, in the fields of FearIrbPlanInfo ("gemm.field": value).  `lds` 0 is the first-generation kernel.
_FIRST_GEN_1047 = {"lds": 0, "row_tiles": 1, "grid_x": 1047, "grid_y": 1}      # 133 956 rows = 1 046 tiles of 128 and a ragged one
LARGE_PLANS = {
    "A": {"rows_in": 269120, "rows_out": 269120, "expand.present": 0, "dx.present": 0,
          "project": {"lds": 0, "row_tiles": 2, "grid_x": 1052, "grid_y": 1, "nt": 1}, "g2": {"lds": 0, "row_tiles": 2, "grid_x": 1052, "grid_y": 1, "nt": 1},
          "col_rows_out": 512, "wgrad_rows_per_slice": 2048, "w3.present": 1, "w1.present": 0,
          "dw_fwd": {"tiles_x": 15, "tiles_y": 15, "tile_side": 16, "nslab": 1, "items_per_wg": 3, "small_map": 0},
          "dw_bwd": {"tiles_x": 15, "tiles_y": 15, "tile_side": 16, "nslab": 1, "items_per_wg": 3, "small_map": 0}, "gram_rows_per_wg": 0},
    "A8": {"g2": {"lds": 0, "row_tiles": 2, "grid_x": 1052, "nt": 1}, "w3": {"present": 2, "slices": 1052}},
    "B": {"rows_in": 269120, "project": {"lds": 0, "row_tiles": 2, "grid_x": 1052, "grid_y": 1, "nt": 2},
          "g2": {"lds": 0, "row_tiles": 2, "grid_x": 1052, "grid_y": 1, "nt": 2}, "col_rows_out": 512, "wgrad_rows_per_slice": 2048,
          "dw_fwd.nslab": 2, "dw_bwd.nslab": 2, "dw_bwd.items_per_wg": 5},
    "C": {"rows_in": 535824, "rows_out": 133956, "lin": 1, "virtual_e": 0,
          "expand": {"present": 1, "lds": 0, "k": 16, "row_tiles": 3, "grid_x": 1396, "grid_y": 1, "nt": 6},
          "project": {"k": 96, "nt": 2, **_FIRST_GEN_1047}, "g2": {"k": 24, "nt": 6, **_FIRST_GEN_1047},
          "dx": {"present": 1, "lds": 0, "x2": 1, "k": 96 + 16, "n": 16, "grid_x": 4187, "grid_y": 1, "nt": 1},
          "col_rows_in": 1024, "col_rows_out": 256, "wgrad_rows_per_slice": 4096, "gram_rows_per_wg": 1152,
          "w3": {"present": 1, "swapped": 1}, "w1": {"present": 1, "rows_per_slice": 1408, "slices": 381},
          "dw_fwd": {"tiles_x": 16, "tile_side": 8, "nslab": 3}, "dw_bwd": {"tiles_x": 16, "tile_side": 16, "nslab": 3, "items_per_wg": 14}},
    "C4": {"virtual_e": 1, "lin": 1, "expand.present": 0, "project": {"k": 96, **_FIRST_GEN_1047}, "g2": {"k": 24, **_FIRST_GEN_1047},
           "dx": {"lds": 0, "x2": 1, "k": 112, "grid_x": 4187}, "gram_rows_per_wg": 1152, "w1": {"present": 2, "slices": 165}},
    "C4b": {"virtual_e": 1, "rows_in": 535824, "gram_rows_per_wg": 1152, "project.lds": 0, "dx.lds": 0},
    "D": {"rows_in": 266256, "rows_out": 66564, "lin": 1,
          "expand": {"present": 1, "lds": 0, "k": 24, "row_tiles": 2, "grid_x": 1041, "grid_y": 1, "nt": 3}, "project.lds": 1, "g2.lds": 1,
          "dx": {"lds": 0, "x2": 1, "k": 144 + 24, "n": 24, "grid_x": 2081, "grid_y": 1, "nt": 2},
          "col_rows_in": 512, "col_rows_out": 128, "wgrad_rows_per_slice": 2048, "gram_rows_per_wg": 640,
          "w1": {"present": 1, "rows_per_slice": 1088, "slices": 245}, "w3": {"present": 1, "swapped": 1}},
    "D4": {"virtual_e": 1, "expand.present": 0, "dx": {"lds": 0, "x2": 1, "k": 168, "nt": 2}, "w1.present": 1, "gram_rows_per_wg": 640},
    "E0": {"rows_in": 131072, "expand": {"present": 1, "lds": 1}, "project.lds": 1, "g2.lds": 1, "dx": {"present": 1, "lds": 1, "x2": 1, "k": 224},
           "col_rows_out": 128, "wgrad_rows_per_slice": 1024},
    "E": {"rows_in": 133956, "expand": {"present": 1, "k": 32, "nt": 6, **_FIRST_GEN_1047}, "project": {"k": 192, "nt": 2, **_FIRST_GEN_1047},
          "g2": {"k": 32, "nt": 6, **_FIRST_GEN_1047}, "dx": {"present": 1, "lds": 0, "x2": 1, "k": 192 + 32, "grid_x": 1047, "nt": 2},
          "col_rows_out": 256, "wgrad_rows_per_slice": 1024},
}


def _plan_mismatches(info, want, prefix=""):
    bad = []
    for key, value in want.items():
        obj = info
        for part in key.split("."):
            obj = getattr(obj, part)
        if isinstance(value, dict):
            bad += _plan_mismatches(obj, value, prefix + key + ".")
        elif obj != value:
            bad.append(f"{prefix}{key} = {obj}, the case claims {value}")
    return bad


def test_cases_reach_the_paths_they_claim():
    """The kernels and grids of the block operators are chosen from the row count; a case pins a path only as long as the thresholds
    stay where they were when it was written (FEAR_GEMM_LDS_MAX_ROWS went from 65 536 to 131 072 and the 81 920-row case left the
    first-generation GEMMs unnoticed).  Here every large case, and that one, is held to the plan the library itself reports
    (fear_irb_plan_info / fear_pwbn_plan_info: host only, the launch code's own helpers): move a threshold and this fails until the
    cases are moved with it.  The figures are the arithmetic of the table in LARGE_CASES, not a recording of the library's answers."""
    from feartracker_amd.train_abi import FearIrbBlock, FearIrbPlanInfo, FearPwbnPlanInfo, load_train_library
    lib = load_train_library()
    assert lib.fear_irb_plan_info(None, 1, 16, 16, None) == -1
    bad = []
    cases = {k: v[:4] for k, v in LARGE_CASES.items()}
    plans = dict(LARGE_PLANS)
    # the existing 81 920 / 20 480-row E-free case: first generation where the reduction is shorter than 32 channels, LDS-staged elsewhere
    cases["lin81920"] = ((16, 96, 24, 3, 2, 1, 0), 5, 128, 1)
    plans["lin81920"] = {"rows_in": 81920, "rows_out": 20480, "lin": 1, "expand": {"lds": 0, "k": 16, "row_tiles": 1, "grid_x": 640}, "project.lds": 1,
                         "g2": {"lds": 0, "k": 24}, "dx": {"lds": 1, "x2": 1, "k": 112}, "col_rows_in": 128, "wgrad_rows_per_slice": 1024}
    assert cases["lin81920"] in LIN_CASES and set(plans) == set(cases)
    for name, (cfg, B, H, flags) in cases.items():
        blk = FearIrbBlock()
        blk.cin, blk.cexp, blk.cout, blk.k, blk.stride, blk.expand, blk.residual = cfg
        blk.flags = flags
        info = FearIrbPlanInfo()
        assert lib.fear_irb_plan_info(ctypes.byref(blk), B, H, H, ctypes.byref(info)) == 0, name
        assert B * H * H * cfg[1] * 4 < 2 ** 31 and lib.fear_irb_workspace_bytes(ctypes.byref(blk), B, H, H) > 0
        bad += [f"{name}: {m}" for m in _plan_mismatches(info, plans[name])]
        # the ragged tails: no large case's row counts are whole tiles, and a fattened grid has an overhang tile to skip
        if name in LARGE_CASES and name != "E0":
            assert info.rows_in % 128 and info.rows_out % 128, name
            for gemm in (info.expand, info.project, info.g2):
                if gemm.present and gemm.row_tiles > 1:
                    assert gemm.grid_x * gemm.row_tiles == -(-gemm.rows // 128) + 1, (name, "no overhang tile")
    # F: the stem and the pointwise unit it is held to, 269 120 rows
    n, H = LARGE_STEM
    M = n * (H // 2) ** 2
    for stem in (1, 0):
        info = FearPwbnPlanInfo()
        assert lib.fear_pwbn_plan_info(M, 28, 16, 1, stem, ctypes.byref(info)) == 0
        bad += [f"F (stem = {stem}): {m}" for m in _plan_mismatches(info, {"rows": 269120, "forward": {"present": 1, "lds": 0, "row_tiles": 2, "grid_x": 1052,
                                                                                                       "grid_y": 1, "nt": 1}, "col_rows": 512})]
    assert lib.fear_pwbn_plan_info(M, 24, 16, 1, 1, ctypes.byref(info)) == -2      # the stem is 28 -> 16
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,B,H,flags", ALL_CASES,
                         ids=[f"{c[0]}x{c[1]}x{c[2]}k{c[3]}s{c[4]}_b{b}h{h}" + {0: "", 1: "_lin", 2: "_nolin", 4: "_virtual", 8: "_fusew3"}[f] for c, b, h, f in ALL_CASES])
def test_irb_block_forward_backward_vs_autograd(cfg, B, H, flags):
    _irb_case(cfg, B, H, H, flags, biased=False)


BIASED_CASES = [((16, 96, 24, 3, 2, 1, 0), 3, 32, 4), ((24, 144, 32, 5, 2, 1, 0), 2, 32, 4), ((32, 192, 64, 5, 2, 1, 0), 2, 32, 4),
                ((32, 192, 32, 5, 1, 1, 1), 2, 16, 0), ((16, 96, 24, 3, 2, 1, 0), 3, 32, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,B,H,flags", BIASED_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}k{c[3]}s{c[4]}_flags{f}" for c, b, h, f in BIASED_CASES])
def test_irb_block_on_biased_correlated_inputs(cfg, B, H, flags):
    """a virtual expansion's BatchNorm1 variance is w^T G w / M - mean^2 with G = x^T x accumulated in fp32; the cases
    above feed zero-mean uncorrelated inputs, the benign case.  Real block inputs are post-ReLU / residual: here every channel is
    relu(noise) + 3 plus a component shared by all channels (mean ~ 4 x the spread, channels correlated at 0.5), on the virtual
    blocks, an E-free one and a plain one — the same 2e-4 against float64 autograd, running statistics included."""
    _irb_case(cfg, B, H, H, flags, biased=True)


# Rectangular maps (the ABI takes H and W separately and irb_shape_ok accepts any pair): wide and tall, a stride-2 virtual expansion,
# the 8-row small-map kernel with a 16-wide map, the fused projection weight gradient — a swapped H / W in a tile count, a halo index
# or Ho / Wo shows in none of the square cases above
RECT_CASES = [((16, 96, 24, 3, 2, 1, 0), 2, 16, 48, 0), ((16, 96, 24, 3, 2, 1, 0), 2, 16, 48, 4), ((32, 192, 32, 5, 1, 1, 1), 2, 24, 8, 0),
              ((112, 672, 112, 5, 1, 1, 1), 2, 8, 16, 0), ((16, 16, 16, 3, 1, 0, 1), 2, 40, 24, 0), ((16, 16, 16, 3, 1, 0, 1), 2, 40, 24, 8),
              ((24, 144, 32, 5, 2, 1, 0), 2, 32, 16, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,B,H,W,flags", RECT_CASES,
                         ids=[f"{c[0]}x{c[1]}x{c[2]}k{c[3]}s{c[4]}_b{b}h{h}w{w}" + {0: "", 4: "_virtual", 8: "_fusew3"}[f] for c, b, h, w, f in RECT_CASES])
def test_irb_block_on_rectangular_maps(cfg, B, H, W, flags):
    _irb_case(cfg, B, H, W, flags, biased=False)


@functools.lru_cache(maxsize=1)
def _irb_reference(cfg, B, H, W, biased):
    """Inputs, parameters and float64 autograd of one block (the reference): computed once for the cases that differ in `flags` alone
    (neighbours in the case lists), and read only.  Last: per ReLU, (shape, flat indices, reference sides) of the activations in the
    kink band."""
    pre = {}
    x, p, stats, ref, dout = _irb_autograd(cfg, B, H, W, biased, None, pre)
    kinks = {}
    for name, z in pre.items():
        near = torch.nonzero(z.abs().flatten() < KINK_BAND * z.abs().max()).flatten()
        kinks[name] = (tuple(z.shape), near, z.flatten()[near] > 0)
    return x, p, stats, ref, dout, kinks


def _irb_autograd(cfg, B, H, W, biased, flips, pre=None):
    cin, cexp, cout, k, stride, expand, residual = cfg
    g = torch.Generator().manual_seed(100 + cin + cexp + k + stride + H)
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64)
    if biased:
        shared = torch.randn(B, 1, H, W, generator=g, dtype=torch.float64)
        x = (torch.relu(x) * 0.7 + shared * 0.7 + 3.0)
    x.requires_grad_(True)
    p = {"w_dw": torch.randn(k * k, cexp, generator=g, dtype=torch.float64) * (2.0 / (k * k)) ** 0.5,
         "w_pwl": torch.randn(cout, cexp, generator=g, dtype=torch.float64) * (2.0 / cexp) ** 0.5}
    if expand:
        p["w_pw"] = torch.randn(cexp, cin, generator=g, dtype=torch.float64) * (2.0 / cin) ** 0.5
    chans = (cexp, cexp, cout)
    for i in range(3):
        p[f"g{i}"] = torch.rand(chans[i], generator=g, dtype=torch.float64) + 0.5
        p[f"b{i}"] = torch.randn(chans[i], generator=g, dtype=torch.float64) * 0.3
    for v in p.values():
        v.requires_grad_(True)
    stats = {}
    for i in range(3):
        stats[f"rm{i}"] = torch.zeros(chans[i], dtype=torch.float64)
        stats[f"rv{i}"] = torch.ones(chans[i], dtype=torch.float64)
    ref = _torch_block(x, p, cfg, stats, flips, pre)
    dout = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    ref.backward(dout)
    return x, p, stats, ref.detach(), dout


def _sides_taken(kinks, masked, dev):
    """Per ReLU the flat (NCHW) indices in the kink band where the operator's derivative — `masked[name]`: its masked gradient as rows,
    zero where the ReLU is shut — is on the other side than the reference's."""
    flips = {}
    for name, (shape, near, ref_open) in kinks.items():
        _, C, Hh, Ww = shape
        b, c, yx = near // (C * Hh * Ww), (near // (Hh * Ww)) % C, near % (Hh * Ww)
        dev_open = masked[name].flatten()[((b * Hh * Ww + yx) * C + c).to(dev)].cpu() != 0
        flips[name] = near[dev_open != ref_open]
    return flips


def _irb_case(cfg, B, H, W, flags, biased):
    from feartracker_amd.train_head import FearIrbBlock, FearIrbGrads, FearIrbSaved, _p, load_train_library
    lib = load_train_library()
    dev = torch.device("cuda:0")
    cin, cexp, cout, k, stride, expand, residual = cfg
    Ho, Wo = H // stride, W // stride
    chans = (cexp, cexp, cout)
    x, p, stats, ref, dout, kinks = _irb_reference(cfg, B, H, W, biased)

    keep = []

    def D(t):
        keep.append(t.detach().to(dev, torch.float32).contiguous())
        return keep[-1]

    G = _Guarded(dev)
    nan = float("nan")
    rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    blk = FearIrbBlock()
    blk.cin, blk.cexp, blk.cout, blk.k, blk.stride, blk.expand, blk.residual = cin, cexp, cout, k, stride, expand, residual
    blk.flags = flags
    w_pw = D(p["w_pw"]) if expand else None
    w_dw, w_pwl = D(p["w_dw"]), D(p["w_pwl"])
    blk.w_pw, blk.w_dw, blk.w_pwl = (w_pw.data_ptr() if expand else None), w_dw.data_ptr(), w_pwl.data_ptr()
    gam, bet, rm, rv = [], [], [], []
    for i in range(3):
        gam.append(D(p[f"g{i}"])); bet.append(D(p[f"b{i}"]))
        rm.append(G.alloc(f"running_mean{i}", chans[i], fill=0.0)); rv.append(G.alloc(f"running_var{i}", chans[i], fill=1.0))
        blk.gamma[i], blk.beta[i], blk.running_mean[i], blk.running_var[i] = gam[i].data_ptr(), bet[i].data_ptr(), rm[i].data_ptr(), rv[i].data_ptr()
    # workspace and scratch at exactly the sizes the library reports: that size, not the allocation's, is what the calls are told
    wsb = int(lib.fear_irb_workspace_bytes(ctypes.byref(blk), B, H, W))
    assert wsb > 0 and wsb % 4 == 0
    ws = G.alloc("workspace", wsb // 4)
    scratch = G.alloc("scratch", int(lib.fear_irb_scratch_floats(ctypes.byref(blk), B, H, W)))
    sv = FearIrbSaved()
    e = G.alloc("e", B * H * W, cexp) if expand and not flags & 4 else None
    assert not flags & 4 or lib.fear_irb_virtual_ok(ctypes.byref(blk)) == 1
    d, pp = G.alloc("d", B * Ho * Wo, cexp), G.alloc("p", B * Ho * Wo, cout)
    vec = [G.alloc(f"vec{i}", 4 * c) for i, c in enumerate(chans)]
    sv.e, sv.d, sv.p = (e.data_ptr() if e is not None else None), d.data_ptr(), pp.data_ptr()
    for i in range(3):
        sv.vec[i] = vec[i].data_ptr()
    xd = D(rows(x))
    out = G.alloc("out", B * Ho * Wo, cout)
    assert lib.fear_irb_train_forward(ctypes.byref(blk), ctypes.byref(sv), _p(xd), _p(out), B, H, W, 0.1, 1e-5, _p(ws), wsb, None) == 0
    torch.cuda.synchronize()
    G.check("by the forward")
    errs = {"out": _rel(out, rows(ref))}
    for i in range(0 if expand else 1, 3):
        errs[f"running_mean{i}"] = _rel(rm[i], stats[f"rm{i}"])
        errs[f"running_var{i}"] = _rel(rv[i], stats[f"rv{i}"])
    gr = FearIrbGrads()
    gw_pw = G.alloc("d w_pw", cexp, cin, fill=nan) if expand else None
    gw_dw, gw_pwl = G.alloc("d w_dw", k * k, cexp, fill=nan), G.alloc("d w_pwl", cout, cexp, fill=nan)
    gr.w_pw, gr.w_dw, gr.w_pwl = (gw_pw.data_ptr() if expand else None), gw_dw.data_ptr(), gw_pwl.data_ptr()
    gg, gb = [], []
    for i in range(3):
        gg.append(G.alloc(f"d gamma{i}", chans[i], fill=nan)); gb.append(G.alloc(f"d beta{i}", chans[i], fill=nan))
        gr.gamma[i], gr.beta[i] = gg[i].data_ptr(), gb[i].data_ptr()
    dx = G.alloc("dx", B * H * W, cin, fill=nan)
    doutd = D(rows(dout))
    assert lib.fear_irb_train_backward(ctypes.byref(blk), ctypes.byref(sv), ctypes.byref(gr), _p(xd), _p(doutd), _p(dx), _p(scratch),
                                       B, H, W, _p(ws), wsb, None, None) == 0
    torch.cuda.synchronize()
    G.check("by the backward")
    first_gb = [t.clone() for t in gg + gb]
    # (KINK_BAND) the gradients' reference with the ReLU derivatives in the kink band on the operator's side
    n_out, n_in = B * Ho * Wo * cexp, B * H * W * cexp
    masked = {"act2": scratch[:n_out]}
    if expand:
        masked["act1"] = scratch[n_out:n_out + n_in]
    flips = _sides_taken(kinks, masked, dev)
    print("activations in the kink band:", {n_: int(v[1].numel()) for n_, v in kinks.items()}, "taken from the operator:", {n_: int(v.numel()) for n_, v in flips.items()})
    if any(v.numel() for v in flips.values()):
        x, p = _irb_autograd(cfg, B, H, W, biased, flips)[:2]
    errs["dx"] = _rel(dx, rows(x.grad))
    errs["d w_dw"] = _rel(gw_dw, p["w_dw"].grad)
    errs["d w_pwl"] = _rel(gw_pwl, p["w_pwl"].grad)
    if expand:
        errs["d w_pw"] = _rel(gw_pw, p["w_pw"].grad)
    for i in range(0 if expand else 1, 3):
        errs[f"d gamma{i}"] = _rel(gg[i], p[f"g{i}"].grad)
        errs[f"d beta{i}"] = _rel(gb[i], p[f"b{i}"].grad)
    print({k_: f"{v:.1e}" for k_, v in errs.items()})
    bad = {k_: v for k_, v in errs.items() if not v < 2e-4}
    assert not bad, bad
    # the same call again: bit-identical (fixed-order reductions), and without the input gradient where the block allows it
    dx2 = G.alloc("dx (second call)", B * H * W, cin)
    gw2 = G.alloc("d w_dw (second call)", k * k, cexp)
    gr.w_dw = gw2.data_ptr()
    # ... with the two pointwise weight gradients on a second stream (`wgrad_stream`): same numbers
    gw_pwl2 = G.alloc("d w_pwl (second call)", cout, cexp, fill=nan)
    gr.w_pwl = gw_pwl2.data_ptr()
    gw_pw2 = G.alloc("d w_pw (second call)", cexp, cin, fill=nan) if expand else None
    if expand:
        gr.w_pw = gw_pw2.data_ptr()
    aux = torch.cuda.Stream()
    assert lib.fear_irb_train_backward(ctypes.byref(blk), ctypes.byref(sv), ctypes.byref(gr), _p(xd), _p(doutd), _p(dx2), _p(scratch),
                                       B, H, W, _p(ws), wsb, None, ctypes.c_void_p(aux.cuda_stream)) == 0
    torch.cuda.synchronize()
    G.check("by the backward with a weight-gradient stream")
    assert torch.equal(dx2, dx) and torch.equal(gw2, gw_dw) and torch.equal(gw_pwl2, gw_pwl)
    assert not expand or torch.equal(gw_pw2, gw_pw)
    if not expand:
        return      # (without an expansion dx is the depthwise pass's own output: dx = NULL is FEAR_TRAIN_ERR_NULL by design)
    # ... and without the input gradient (dx = NULL): every weight, gamma and beta gradient as in the first call
    first = [gw_dw, gw_pwl, gw_pw] + first_gb
    third = [G.alloc(f"gradient {i} (third call)", *t.shape, fill=nan) for i, t in enumerate(first)]
    gr.w_dw, gr.w_pwl, gr.w_pw = (t.data_ptr() for t in third[:3])
    for i in range(3):
        gr.gamma[i], gr.beta[i] = third[3 + i].data_ptr(), third[6 + i].data_ptr()
    assert lib.fear_irb_train_backward(ctypes.byref(blk), ctypes.byref(sv), ctypes.byref(gr), _p(xd), _p(doutd), None, _p(scratch),
                                       B, H, W, _p(ws), wsb, None, None) == 0
    torch.cuda.synchronize()
    G.check("by the backward without dx")
    assert all(torch.equal(a, b) for a, b in zip(third, first))


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,N,relu,need_dx", [(2 * 64 * 64, 28, 16, 1, False), (3 * 16 * 16, 112, 256, 0, True), (1000, 24, 40, 1, True)])
def test_pwbn_unit_forward_backward_vs_autograd(M, K, N, relu, need_dx):
    """The stem (im2col rows, K = 28) and the AdjustLayer neck (blocks.py:75-88) as lone conv + BatchNorm [+ ReLU] units."""
    from feartracker_amd.train_head import _p, load_train_library
    lib = load_train_library()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5 + K + N)
    x = torch.randn(M, K, generator=g, dtype=torch.float64)
    w = torch.randn(N, K, generator=g, dtype=torch.float64) * 0.3
    gamma = torch.rand(N, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(N, generator=g, dtype=torch.float64) * 0.3
    dy = torch.randn(M, N, generator=g, dtype=torch.float64)
    ref = pwbn_autograd(x, w, gamma, beta, relu, dy)      # (tests/syncref.py: the two-rank tests compare with the same reference)
    D = lambda t: t.detach().to(dev, torch.float32).contiguous()
    xd, wd, gd, bd, dyd = D(x), D(w), D(gamma), D(beta), D(dy)
    G = _Guarded(dev)
    rm, rv = G.alloc("running_mean", N, fill=0.0), G.alloc("running_var", N, fill=1.0)
    raw, vec, out = G.alloc("raw", M, N), G.alloc("vec", 4 * N), G.alloc("out", M, N)
    wsb = int(lib.fear_pwbn_workspace_bytes(M, K, N))      # the calls are told the reported size, and get exactly that
    ws = G.alloc("workspace", wsb // 4)
    assert lib.fear_pwbn_train_forward(_p(xd), K, _p(wd), _p(gd), _p(bd), _p(rm), _p(rv), _p(raw), _p(vec), relu, _p(out), M, K, N, 0.1, 1e-5,
                                       _p(ws), wsb, None) == 0
    torch.cuda.synchronize()
    G.check("by the forward")
    dw, dg, db = G.alloc("dw", N, K), G.alloc("dgamma", N), G.alloc("dbeta", N)
    dx = G.alloc("dx", M, K) if need_dx else None
    assert lib.fear_pwbn_train_backward(_p(dyd), _p(raw), _p(vec), relu, _p(xd), K, _p(wd), _p(gd), _p(dw), _p(dg), _p(db), _p(dx), M, K, N,
                                        _p(ws), wsb, None, None) == 0
    torch.cuda.synchronize()
    G.check("by the backward")
    errs = {"out": _rel(out, ref["out"]), "running_mean": _rel(rm, ref["running_mean"]), "running_var": _rel(rv, ref["running_var"]),
            "dw": _rel(dw, ref["d w"]), "dgamma": _rel(dg, ref["d gamma"]), "dbeta": _rel(db, ref["d beta"])}
    if need_dx:
        errs["dx"] = _rel(dx, ref["dx"])
    print({k_: f"{v:.1e}" for k_, v in errs.items()})
    bad = {k_: v for k_, v in errs.items() if not v < 2e-4}
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,cin,cout,bias,ldx_pad,ldo_pad", [(3, 16, 256, 256, True, 0, 0), (2, 16, 320, 256, True, 0, 64), (2, 8, 64, 48, False, 16, 0),
                                                            (40, 16, 256, 256, True, 0, 0)])
def test_sepbn_layer_forward_backward_vs_autograd(B, H, cin, cout, bias, ldx_pad, ldo_pad):
    _sepbn_case(B, H, H, cin, cout, bias, ldx_pad, ldo_pad)


@pytest.mark.gpu
def test_sepbn_layer_on_a_rectangular_map():
    _sepbn_case(2, 8, 24, 64, 48, False, 16, 0)


def _sepbn_case(B, H, W, cin, cout, bias, ldx_pad, ldo_pad):
    """The head's layer — SepConv (3x3 depthwise + pointwise, with or without biases) + BatchNorm + ReLU, model_training/model/
    blocks.py:97-101 / 115-119 / 151-161 — as one call per direction; input / output rows with a pitch (the [encode | correlation]
    concatenation); the weight gradients on a second stream are bit-identical to the in-line ones.  The last case's 10 240 rows reach
    the row-sliced weight-gradient kernels of the full batch."""
    from feartracker_amd.train_head import FearSepGrads, FearSepLayer, _p, load_train_library
    lib = load_train_library()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11 + cin + cout + B)
    M = B * H * W
    R = lambda *s, scale=1.0: (torch.randn(*s, generator=g, dtype=torch.float64) * scale)
    x = R(B, cin, H, W)
    taps = R(9, cin, scale=0.4)
    w = R(cout, cin, scale=(2.0 / cin) ** 0.5)
    b_dw = R(cin, scale=0.3) if bias else None
    b_pw = R(cout, scale=0.3) if bias else None
    gamma = torch.rand(cout, generator=g, dtype=torch.float64) + 0.5
    beta = R(cout, scale=0.3)
    dy = R(B, cout, H, W)
    rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(M, -1)
    ref = sepbn_autograd(x, taps, w, b_dw, b_pw, gamma, beta, rows(dy))      # (tests/syncref.py, shared with the two-rank tests)
    D = lambda t: None if t is None else t.detach().to(dev, torch.float32).contiguous()
    ldx, ldo = cin + ldx_pad, cout + ldo_pad
    xd = torch.zeros(M, ldx, device=dev)
    xd[:, :cin] = D(rows(x))
    td, wd, bdw, bpw, gd, bd, dyd = D(taps), D(w), D(b_dw), D(b_pw), D(gamma), D(beta), D(rows(dy))
    rm, rv = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    L = FearSepLayer(cin, cout, ptr(td), ptr(bdw), ptr(wd), ptr(bpw), ptr(gd), ptr(bd), ptr(rm), ptr(rv))
    ws = torch.empty(int(lib.fear_sepbn_workspace_bytes(ctypes.byref(L), B, H, W)) // 4 + 64, device=dev)
    d, raw, vec = torch.empty(M, cin, device=dev), torch.empty(M, cout, device=dev), torch.empty(4 * cout, device=dev)
    out = torch.full((M, ldo), 7.0, device=dev)
    assert lib.fear_sepbn_train_forward(ctypes.byref(L), _p(xd), ldx, _p(d), _p(raw), _p(vec), _p(out), ldo, B, H, W, 0.1, 1e-5, _p(ws),
                                        ws.numel() * 4, None) == 0

    def backward(aux):
        gt, gw, gg, gb = torch.empty(9, cin, device=dev), torch.empty(cout, cin, device=dev), torch.empty(cout, device=dev), torch.empty(cout, device=dev)
        dd, coef, dx = torch.empty(M, cin, device=dev), torch.empty(4 * cout, device=dev), torch.empty(M, cin, device=dev)
        G = FearSepGrads(gt.data_ptr(), gw.data_ptr(), gg.data_ptr(), gb.data_ptr())
        assert lib.fear_sepbn_train_backward(ctypes.byref(L), ctypes.byref(G), _p(xd), ldx, _p(d), _p(raw), _p(vec), _p(dyd), _p(dd), _p(coef),
                                             _p(dx), B, H, W, _p(ws), ws.numel() * 4, None,
                                             ctypes.c_void_p(aux.cuda_stream) if aux is not None else None) == 0
        torch.cuda.synchronize()
        return gt, gw, gg, gb, dx
    gt, gw, gg, gb, dx = backward(None)
    errs = {"out": _rel(out[:, :cout], ref["out"]), "running_mean": _rel(rm, ref["running_mean"]), "running_var": _rel(rv, ref["running_var"]),
            "d": _rel(d, ref["d"]), "dtaps": _rel(gt, ref["d taps"]), "dw": _rel(gw, ref["d w"]), "dgamma": _rel(gg, ref["d gamma"]),
            "dbeta": _rel(gb, ref["d beta"]), "dx": _rel(dx, ref["dx"])}
    print({k_: f"{v:.1e}" for k_, v in errs.items()})
    bad = {k_: v for k_, v in errs.items() if not v < 2e-4}
    assert not bad, bad
    assert ldo_pad == 0 or bool((out[:, cout:] == 7.0).all())        # nothing written beyond the layer's own columns
    if bias:                                                          # the biases' gradients vanish in front of the BatchNorm
        assert all(float(t.abs().max()) < 1e-9 for t in ref["bias grads"])
    torch.cuda.synchronize()
    again = backward(torch.cuda.Stream(device=dev))
    for a, b in zip((gt, gw, gg, gb, dx), again):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("n,H", [(3, 64), (2, 256), (5, 30)])
def test_stem_on_the_image_forward_backward_vs_autograd(n, H):
    _stem_case(n, H, H)


@pytest.mark.gpu
def test_stem_above_the_row_count_thresholds():
    """LARGE_CASES' "F": 269 120 rows — two row tiles per workgroup of the stem's GEMM and of the pointwise unit it is held to bit for
    bit, 512-row column blocks, a ragged last tile of 64 rows and an overhang tile."""
    _stem_case(*LARGE_STEM, LARGE_STEM[1])


@pytest.mark.gpu
@pytest.mark.parametrize("n,H,W", [(2, 24, 40), (3, 52, 30)])
def test_stem_on_a_rectangular_image(n, H, W):
    _stem_case(n, H, W)


def _stem_case(n, H, W):
    """The stem — 3x3 stride-2 conv 3 -> 16 + BatchNorm + ReLU — with its im2col rows gathered from the NCHW image by the GEMM and by the
    weight gradient (fear_stem_train_*): same numbers as the materialised rows (fear_stem_im2col + fear_pwbn_train_*), bit for bit
    in the forward, and autograd's gradients."""
    from feartracker_amd.train_head import _p, load_train_library
    lib = load_train_library()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(21 + n + H)
    x = torch.randn(n, 3, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(16, 3, 3, 3, generator=g, dtype=torch.float64) * 0.3
    gamma = torch.rand(16, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(16, generator=g, dtype=torch.float64) * 0.3
    Ho, Wo = H // 2, W // 2
    M = n * Ho * Wo
    dy = torch.randn(n, 16, Ho, Wo, generator=g, dtype=torch.float64)
    rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(M, -1)
    ref = stem_autograd(x, w, gamma, beta, rows(dy))      # (tests/syncref.py, shared with the two-rank tests)
    D = lambda t: t.detach().to(dev, torch.float32).contiguous()
    xd, gd, bd, dyd = D(x), D(gamma), D(beta), D(rows(dy))
    w28 = torch.zeros(16, 28, device=dev)
    w28[:, :27] = D(w).reshape(16, 27)
    G = _Guarded(dev)
    wsb = int(lib.fear_stem_workspace_bytes(n, H, W))      # the calls are told the reported size, and get exactly that
    assert wsb > 0 and wsb == int(lib.fear_pwbn_workspace_bytes(M, 28, 16))
    ws = G.alloc("workspace", wsb // 4)
    rm, rv = G.alloc("running_mean", 16, fill=0.0), G.alloc("running_var", 16, fill=1.0)
    raw, vec, out = G.alloc("raw", M, 16), G.alloc("vec", 64), G.alloc("out", M, 16)
    assert lib.fear_stem_train_forward(_p(xd), _p(w28), _p(gd), _p(bd), _p(rm), _p(rv), _p(raw), _p(vec), _p(out), n, H, W, 0.1, 1e-5,
                                       _p(ws), wsb, None) == 0
    torch.cuda.synchronize()
    G.check("by the stem's forward")
    # the materialised form
    col = G.alloc("im2col rows", M, 28)
    assert lib.fear_stem_im2col(_p(xd), _p(col), n, H, W, None) == 0
    rm2, rv2 = G.alloc("running_mean (pwbn)", 16, fill=0.0), G.alloc("running_var (pwbn)", 16, fill=1.0)
    raw2, vec2, out2 = G.alloc("raw (pwbn)", M, 16), G.alloc("vec (pwbn)", 64), G.alloc("out (pwbn)", M, 16)
    assert lib.fear_pwbn_train_forward(_p(col), 28, _p(w28), _p(gd), _p(bd), _p(rm2), _p(rv2), _p(raw2), _p(vec2), 1, _p(out2), M, 28, 16,
                                       0.1, 1e-5, _p(ws), wsb, None) == 0
    torch.cuda.synchronize()
    G.check("by the materialised forward")
    assert torch.equal(raw, raw2) and torch.equal(out, out2) and torch.equal(vec, vec2)
    dw, dg, db = G.alloc("dw", 16, 28), G.alloc("dgamma", 16), G.alloc("dbeta", 16)
    assert lib.fear_stem_train_backward(_p(dyd), _p(raw), _p(vec), _p(xd), _p(gd), _p(dw), _p(dg), _p(db), n, H, W, _p(ws), wsb,
                                        None, None) == 0
    torch.cuda.synchronize()
    G.check("by the stem's backward")
    dw2, dg2, db2 = G.alloc("dw (pwbn)", 16, 28), G.alloc("dgamma (pwbn)", 16), G.alloc("dbeta (pwbn)", 16)
    assert lib.fear_pwbn_train_backward(_p(dyd), _p(raw2), _p(vec2), 1, _p(col), 28, _p(w28), _p(gd), _p(dw2), _p(dg2), _p(db2), None, M, 28, 16,
                                        _p(ws), wsb, None, None) == 0
    torch.cuda.synchronize()
    G.check("by the materialised backward")
    assert torch.equal(dw, dw2) and torch.equal(dg, dg2) and torch.equal(db, db2)
    errs = {"out": _rel(out, ref["out"]), "running_mean": _rel(rm, ref["running_mean"]), "running_var": _rel(rv, ref["running_var"]),
            "dw": _rel(dw[:, :27].reshape(16, 3, 3, 3), ref["d w"]), "dgamma": _rel(dg, ref["d gamma"]), "dbeta": _rel(db, ref["d beta"])}
    print({k_: f"{v:.1e}" for k_, v in errs.items()})
    bad = {k_: v for k_, v in errs.items() if not v < 2e-4}
    assert not bad, bad
    assert float(dw[:, 27].abs().max()) == 0.0
