"""float64 evaluator of the FEAR network that rounds where the HIP kernels round.  TEST INFRASTRUCTURE ONLY.

Same import rule as `fear_oracle.py`: only `tests/`, `__graft_entry__.smoke()` and `bench.py` may import it.

`fear_oracle.OracleNet` restates the network in fp32; its error against the kernels (1e-6 of scale in fp32) says nothing about
the bf16 mode, whose kernels deviate from fp32 by ~1e-2 by construction.  This module evaluates in float64 and applies the
kernels' own roundings at the points where the code makes them, so a kernel can be held to the summation-order difference
that is left (fp32 accumulators against float64), one block or one head at a time.

Arithmetic modes (`FEAR_OPT_MATH`, fear_kernels.h `MatOps`):
  0  exact fp32 MFMA: no rounding but fp32 accumulation -> the float64 value.
  1  fp16 hi + lo split of the activation operand of every matrix-pipe GEMM (`split_half8`: hi = fp16(x), lo = fp16(x - hi),
     computed from the fp32 value); weights are fp16 numbers, exact.  In the correlation both operands are split and the
     lo x lo product is dropped (`MatOps<1>::mma2`).
  2  both GEMM operands rounded to bf16 with ties to even (`MatOps<2>::split` = `__builtin_convertvector(..., bf16)`; weights
     on the host by `float_to_bf16`, fear_engine.hip:85).  Bias, ReLU, the depthwise conv and the residual stay fp32.

Rounding points of an inverted-residual block on the matrix pipe (ir16h_fused_kernel, ir_tile_h_kernel in fear_kernels.h):
  * the expansion operand x (`MX::split(v0, v1, xhi, xlo)` at the activation-fragment loads of both kernels; under IO_X_BF16 the
    stored activations are the operands as they stand),
  * the expansion / projection weights (`pack_fused_h(..., bf16)`: rounded from their fp16 values),
  * the depthwise output after its ReLU (`MX::split(q0, q1, dhi, dlo)` / `MX::split(d[0], d[1], ...)` ahead of phase C).
  The expanded map is written to the LDS tile as fp32 (`*reinterpret_cast<f32x4*>(E + ...) = v` after bias + ReLU), so it is
  NOT a rounding point; the projection epilogue adds bias and residual to the fp32 accumulator.
Which kernel a block runs is the plan's choice, read from its op names (`block_arith`): blocks without expansion on the tile
kernels (e1) stay on the fp32 kernel in every mode (fear_engine.hip `add_fused_tile`: `math = ce >= 0 ? h->math : 0`), the stem
+ first block unit (`stem_irt_*`) is fp32, and the layer-wise fall-back launches of the template branch (`pw_*`, `dw*`) are the
fp32 kernels (`run_plan`, OP_PW: `launch_pw_h` only `if (h->math && p.with_head)`).

Head in mode 2 (sep16 `*_h` launches = ir16h_fused_kernel<..., EXPAND=false, 2>, headchain_b_kernel): every SepConv rounds its
depthwise output (no activation there) and its pointwise weights; the prediction SepConv likewise; the pixel-wise correlation
rounds both operands (the encode output and the caller's template features; fear_headchain_b.h `hcb_cvt(za, zb)`, pw_h_kernel
`WKN`), while the encode output enters the concatenation (the correlation SepConv's depthwise input) as fp32.  The correlation
is a bf16 GEMM only in the throughput plan: the small-batch plans run it on the split-column fp32 kernel (`run_plan`, OP_CORR
with `pw_split`: `pw_mfma_kernel` before the `h->math` branch).  So is the neck there when its 16-channel tile count is even
(OP_PW: `op.pw_split && n_tiles % 2 == 0`; 16 tiles for the shipped 256-channel necks); with an odd count it takes
`launch_pw_h`, bf16 in mode 2.

Head in modes 0 and 1: the same launches with `MatOps<0>` / `MatOps<1>` (mode 0 in the throughput plan: headchain_kernel, or the
sep16 launches with the correlation / prediction epilogues); the neck and the correlation follow the same plan rules with the
fp16 split in place of bf16.  The `Rounding` settings for these modes are MUTANTS only (an operand that keeps just its hi half,
a correlation without its cross terms, an fp32-mode operand rounded to fp16 / bf16): the defaults are the exact kernels.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

from .fear_oracle import (ACT_EXP, K_IR, K_NECK, K_SEP, K_STEM, ROLE_BBOX_PRED, ROLE_BBOX_TOWER, ROLE_CLS_CORR,
                          ROLE_CLS_ENCODE, ROLE_CLS_PRED, ROLE_CLS_TOWER, ROLE_REG_CORR, ROLE_REG_ENCODE, load_fearw)


# ---------------------------------------------------------------------------------------------------------- rounding helpers
def to_fp32(x: torch.Tensor) -> torch.Tensor:
    """float64 -> fp32 (round to nearest even) -> float64: the fp32 accumulator a kernel rounds from."""
    return x.to(torch.float32).to(torch.float64)


def round_bf16(x: torch.Tensor) -> torch.Tensor:
    """fp32(x) rounded to bf16, ties to even, back to float64 (fear_engine.hip `float_to_bf16`, `v_cvt_pk_bf16_f32`).
    torch's CPU float32 -> bfloat16 conversion is RNE with NaN kept NaN and overflow to inf; tests/test_ref64_cpu.py checks it
    against the bit-twiddled form on edges and random values."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def trunc_bf16(x: torch.Tensor) -> torch.Tensor:
    """fp32(x) with the low 16 bits cleared (round toward zero): a MUTANT of `round_bf16`, never a kernel's rounding."""
    b = x.to(torch.float32).contiguous().view(torch.int32) & ~0xFFFF
    return b.view(torch.float32).to(torch.float64)


def round_fp16(x: torch.Tensor) -> torch.Tensor:
    """fp32(x) rounded to fp16, ties to even, overflow to inf, subnormals kept (`__builtin_convertvector(x, h8)`)."""
    return x.to(torch.float32).to(torch.float16).to(torch.float64)


def split_fp16(x: torch.Tensor):
    """(hi, lo) of `split_half8`: hi = fp16(x32), lo = fp16(x32 - fp32(hi)); the subtraction is exact in fp32."""
    x32 = x.to(torch.float32)
    hi = x32.to(torch.float16)
    lo = (x32 - hi.to(torch.float32)).to(torch.float16)
    return hi.to(torch.float64), lo.to(torch.float64)


# ------------------------------------------------------------------------------------------------------------ rounding plan
@dataclass(frozen=True)
class Rounding:
    """Where an evaluation rounds.  The defaults are the kernels' rounding points; every other setting is a MUTANT (a
    defect a kernel could have), used to show that the GPU tests' tolerances would catch it (tests/test_ref64_cpu.py).
    The first eight settings act in arithmetic 2, the split settings in arithmetic 1, `fp32_operand` in arithmetic 0."""
    op: str = "rne"               # "rne" | "trunc": how the depthwise output is rounded
    dw_out: bool = True           # round the depthwise output (the projection / pointwise operand)
    weights: bool = True          # round the GEMM weights
    gemm_in: bool = True          # round the expansion / neck operand x
    expanded: bool = False        # MUTANT: round the expanded map (it stays fp32 in LDS)
    residual_after: bool = False  # MUTANT: round the block output before the residual is added
    corr_tmpl: bool = True        # round the template operand of the correlation
    storage: bool = True          # round the tensors the plan stores as bf16 (FEAR_OPT_BF16_STORE)
    split_lo: bool = True         # arithmetic 1: a GEMM activation operand is hi + lo (False, MUTANT: hi only)
    corr_cross: bool = True       # arithmetic 1: the correlation keeps its hi x lo and lo x hi products (False, MUTANT: hi x hi only)
    corr_lolo: bool = False       # MUTANT, arithmetic 1: the correlation adds lo x lo (~2^-22: not separable, not claimed)
    fp32_operand: str = ""        # MUTANT, arithmetic 0: "fp16" | "bf16": the neck / pointwise operand rounded to that format

    def dw(self, x: torch.Tensor) -> torch.Tensor:
        if not self.dw_out:
            return x
        return trunc_bf16(x) if self.op == "trunc" else round_bf16(x)


EXACT = Rounding()

# name -> the defect it stands for
MUTANTS: Dict[str, Rounding] = {
    "dw_truncated": Rounding(op="trunc"),
    "dw_not_rounded": Rounding(dw_out=False),
    "weights_not_rounded": Rounding(weights=False),
    "expanded_rounded": Rounding(expanded=True),
    "residual_after_rounding": Rounding(residual_after=True),
    "corr_template_not_rounded": Rounding(corr_tmpl=False),
    "no_storage_rounding": Rounding(storage=False),
    # arithmetic 1 (fp16 hi + lo split)
    "split_lo_dropped": Rounding(split_lo=False),
    "corr_cross_dropped": Rounding(corr_cross=False),
    "corr_lolo_kept": Rounding(corr_lolo=True),
    # arithmetic 0 (exact fp32): a reduced-precision kernel launched in fp32 mode
    "operand_fp16": Rounding(fp32_operand="fp16"),
    "operand_bf16": Rounding(fp32_operand="bf16"),
}


def _fp32_operand(x: torch.Tensor, rnd: Rounding) -> torch.Tensor:
    """An arithmetic-0 GEMM operand: the fp32 value itself; rounded only by the `fp32_operand` MUTANTS."""
    if rnd.fp32_operand:
        return {"fp16": round_fp16, "bf16": round_bf16}[rnd.fp32_operand](x)
    return x


def operand(x: torch.Tensor, arith: int, rnd: Rounding = EXACT) -> torch.Tensor:
    """The activation operand of a matrix-pipe GEMM in arithmetic mode `arith`, as the kernel multiplies it."""
    if arith == 1:
        hi, lo = split_fp16(x)
        return hi + lo if rnd.split_lo else hi
    if arith == 2:
        return round_bf16(x) if rnd.gemm_in else x
    return _fp32_operand(x, rnd)


# --------------------------------------------------------------------------------------------------------- op-name parsing
def block_arith(op_names: Sequence[str], math: int, expand: bool) -> int:
    """Arithmetic of the kernel(s) that ran one trunk block, from its op names in the TEMPLATE-branch plan (`plan(hw, False)`):
    ir16_* (fused 16x16: ir16h on the matrix pipe in modes 1 / 2, with or without expansion) and irt_* with expansion
    (ir_tile_h) -> `math`; irt_* without expansion (e1), stem_irt_* and the layer-wise pw_* / dw* launches -> 0."""
    assert op_names, "a block ran no op"
    for n in op_names:
        if n.startswith(("stem_irt", "pw_", "dw")):
            continue
        if n.startswith("ir16_"):
            return math
        if n.startswith("irt_"):
            return math if expand else 0
        raise AssertionError(f"unexpected trunk op {n!r} in the template-branch plan")
    return 0


# --------------------------------------------------------------------------------------------------------------- evaluator
class Ref64Net:
    """The network of a `.fearw` file in float64; weights = the file's fp16 values (exact in float64)."""

    def __init__(self, fearw_path: str):
        m = load_fearw(fearw_path)
        self.convs: List[Dict] = []
        for c in m["convs"]:
            c = dict(c)
            c["w"] = c["w"].double()
            c["b"] = None if c["b"] is None else c["b"].double()
            self.convs.append(c)
        self.blocks = m["blocks"]
        self.trunk = [b for b in self.blocks if b["kind"] in (K_STEM, K_IR)]
        self.neck = [b for b in self.blocks if b["kind"] == K_NECK][0]
        self.head: Dict[int, list] = {}
        for b in self.blocks:
            if b["kind"] == K_SEP:
                self.head.setdefault(b["role"], []).append(b)

    # -- primitives
    def _w(self, idx: int, arith: int, rnd: Rounding) -> torch.Tensor:
        w = self.convs[idx]["w"]
        return round_bf16(w) if arith == 2 and rnd.weights else w

    def conv(self, idx: int, x: torch.Tensor, relu: Optional[bool] = None, w: Optional[torch.Tensor] = None) -> torch.Tensor:
        c = self.convs[idx]
        y = F.conv2d(x, c["w"] if w is None else w, c["b"], stride=c["stride"], padding=c["pad"], groups=c["groups"])
        if c["relu"] if relu is None else relu:
            y = F.relu(y)
        return y

    def pw(self, idx: int, x: torch.Tensor, arith: int, rnd: Rounding = EXACT) -> torch.Tensor:
        """A pointwise conv on the matrix pipe: operand x (rounded / split per mode), weights (rounded in mode 2)."""
        return self.conv(idx, operand(x, arith, rnd), w=self._w(idx, arith, rnd))

    def _pw_operand(self, d: torch.Tensor, arith: int, rnd: Rounding) -> torch.Tensor:
        """A depthwise output as the following pointwise GEMM takes it."""
        if arith == 1:
            hi, lo = split_fp16(d)
            return hi + lo if rnd.split_lo else hi
        return rnd.dw(d) if arith == 2 else _fp32_operand(d, rnd)

    # -- trunk
    def stem_block1(self, img: torch.Tensor) -> torch.Tensor:
        """stem 3x3 s2 + ReLU, then block 1 (e1): the `stem_irt` unit, an fp32 kernel in every mode."""
        x = self.conv(self.trunk[0]["conv"][0], img.double())
        return self.ir_block(1, x, 0)

    def ir_block(self, k: int, x: torch.Tensor, arith: int, rnd: Rounding = EXACT) -> torch.Tensor:
        """Trunk block k (k >= 1: `self.trunk[k]`) on input x in arithmetic mode `arith`."""
        b = self.trunk[k]
        assert b["kind"] == K_IR
        ce, cd, cp = b["conv"]
        x = x.double()
        e = x
        if ce >= 0:
            e = self.pw(ce, x, arith, rnd)
            if arith == 2 and rnd.expanded:
                e = round_bf16(e)
        d = self._pw_operand(self.conv(cd, e), arith, rnd)
        c = self.convs[cp]
        y = F.conv2d(d, self._w(cp, arith, rnd), c["b"])
        if arith == 2 and rnd.residual_after:
            y = round_bf16(y)
        if b["residual"]:
            y = y + x
        if c["relu"]:
            y = F.relu(y)
        return y

    def expands(self, k: int) -> bool:
        return self.trunk[k]["conv"][0] >= 0

    def trunk_out(self, img: torch.Tensor, ariths: Optional[Sequence[int]] = None, rnd: Rounding = EXACT,
                  stored_bf16: Sequence[int] = (), taps: Optional[List[torch.Tensor]] = None) -> torch.Tensor:
        """Stem .. last block.  ariths[k]: arithmetic of block k (k >= 2; default 0).  stored_bf16: trunk units (1 = the stem +
        block 1 unit, k = block k) whose output the plan stores as bf16 (rounded when rnd.storage)."""
        x = self.stem_block1(img)
        if 1 in stored_bf16 and rnd.storage:
            x = round_bf16(x)
        if taps is not None:
            taps.append(x)
        for k in range(2, len(self.trunk)):
            x = self.ir_block(k, x, ariths[k] if ariths is not None else 0, rnd)
            if k in stored_bf16 and rnd.storage:
                x = round_bf16(x)
            if taps is not None:
                taps.append(x)
        return x

    def neck_out(self, trunk: torch.Tensor, arith: int, rnd: Rounding = EXACT) -> torch.Tensor:
        return self.pw(self.neck["conv"][0], trunk.double(), arith, rnd)

    # -- head
    def sep(self, b: Dict, x: torch.Tensor, arith: int, rnd: Rounding = EXACT) -> torch.Tensor:
        """SepConv (+folded BN) + activation: depthwise (no ReLU), its output rounded as the pointwise operand."""
        d = self._pw_operand(self.conv(b["conv"][0], x), arith, rnd)
        c = self.convs[b["conv"][1]]
        y = F.conv2d(d, self._w(b["conv"][1], arith, rnd), c["b"])
        if c["relu"]:
            y = F.relu(y)
        if b["act"] == ACT_EXP:
            y = torch.exp(y)
        return y

    @staticmethod
    def corr(z: torch.Tensor, x: torch.Tensor, arith: int, rnd: Rounding = EXACT) -> torch.Tensor:
        """MobileCorrelation's z^T x (blocks.py:121-126) with the kernels' operands: (B, 64, H, W)."""
        b, c, hh, ww = x.shape
        z = z.double()
        zf = lambda t: t.reshape(t.size(0), t.size(1), -1).permute(0, 2, 1)
        xf = lambda t: t.reshape(b, c, -1)
        if arith == 1:
            zh, zl = split_fp16(z)
            xh, xl = split_fp16(x)
            s = zf(zh) @ xf(xh)
            if rnd.split_lo and rnd.corr_cross:
                s = s + zf(zh) @ xf(xl) + zf(zl) @ xf(xh)                    # lo x lo dropped (MatOps<1>::mma2)
            if rnd.corr_lolo:
                s = s + zf(zl) @ xf(xl)
        else:
            if arith == 2:
                x = round_bf16(x)
                if rnd.corr_tmpl:
                    z = round_bf16(z)
            s = zf(z) @ xf(x)
        return s.view(b, -1, hh, ww)

    def head_maps(self, feat: torch.Tensor, z: torch.Tensor, zu: Optional[torch.Tensor], arith: int, corr_arith: int,
                  rnd: Rounding = EXACT):
        """BoxTower.forward (blocks.py:174-194) on the neck output `feat`: (bbox, cls).  corr_arith: arithmetic of the
        correlation GEMM (the plan's choice: bf16 in the throughput plan, fp32 in the small-batch plans)."""
        h = self.head
        feat = feat.double()
        out = []
        for enc, cr, tower, pred, zz in ((ROLE_REG_ENCODE, ROLE_REG_CORR, ROLE_BBOX_TOWER, ROLE_BBOX_PRED, z),
                                         (ROLE_CLS_ENCODE, ROLE_CLS_CORR, ROLE_CLS_TOWER, ROLE_CLS_PRED, z if zu is None else zu)):
            x = self.sep(h[enc][0], feat, arith, rnd)
            y = self.sep(h[cr][0], torch.cat([x, self.corr(zz, x, corr_arith, rnd)], dim=1), arith, rnd)
            for tb in h.get(tower, []):
                y = self.sep(tb, y, arith, rnd)
            out.append(self.sep(h[pred][0], y, arith, rnd))
        return out[0], out[1]


def max_rel(a: torch.Tensor, b: torch.Tensor) -> float:
    """max |a - b| / max |b|: the deviation in units of the tensor's own scale."""
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
