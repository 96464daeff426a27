"""N3: one training step of the correlation head on the HIP operators of include/fear_train.h against the
fixture produced by the REFERENCE's own BoxTower (train mode) + FEARLoss + torch autograd (tools/make_golden.py section 11):
outputs, both losses, the gradient of every parameter and of both inputs, BatchNorm running statistics."""
import copy
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fear_[a-z0-9_]+)\s*\(", text)))


def test_struct_mirrors_have_the_headers_layout(tmp_path):
    """The ctypes mirrors of the structs in include/fear_train.h (block / layer descriptors handed across the C ABI by pointer) have the
    size and field offsets the C compiler gives the header's own definitions, and the flag values agree; null / shape errors of the
    struct-taking entry points need no GPU."""
    import ctypes
    import subprocess
    from feartracker_amd import train_abi, train_head as th
    from feartracker_amd.train_net import FEAR_IRB_VIRTUAL_E
    structs = {"FearIrbBlock": th.FearIrbBlock, "FearIrbSaved": th.FearIrbSaved, "FearIrbGrads": th.FearIrbGrads,
               "FearSepLayer": th.FearSepLayer, "FearSepGrads": th.FearSepGrads,
               # the plan queries' records (fear_irb_plan_info, fear_pwbn_plan_info)
               "FearGemmPlan": train_abi.FearGemmPlan, "FearWgradPlan": train_abi.FearWgradPlan, "FearDwPlan": train_abi.FearDwPlan,
               "FearIrbPlanInfo": train_abi.FearIrbPlanInfo, "FearPwbnPlanInfo": train_abi.FearPwbnPlanInfo,
               # ... and the layer operators' (fear_layer_plan_info)
               "FearLayerGemmPlan": train_abi.FearLayerGemmPlan, "FearLayerWgradPlan": train_abi.FearLayerWgradPlan,
               "FearLayerDwShape": train_abi.FearLayerDwShape, "FearLayerDwPlan": train_abi.FearLayerDwPlan,
               "FearLayerPlanInfo": train_abi.FearLayerPlanInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/fear_train.h"', 'int main(void) {']
    for name, cls in structs.items():
        lines.append(f'  printf("{name} size %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    lines += ['  printf("FLAGS %d %d %d\\n", FEAR_IRB_LINEAR_BN1, FEAR_IRB_NO_LINEAR_BN1, FEAR_IRB_VIRTUAL_E);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = 0
    for line in out:
        parts = line.split()
        if len(parts) == 3 and parts[0] in structs:
            cls = structs[parts[0]]
            want = ctypes.sizeof(cls) if parts[1] == "size" else getattr(cls, parts[1]).offset
            assert int(parts[2]) == want, line
            seen += 1
        elif parts[:1] == ["FLAGS"]:
            assert [int(v) for v in parts[1:]] == [1, 2, FEAR_IRB_VIRTUAL_E]
            seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in structs.values()) + 1
    lib = th.load_train_library()
    blk = th.FearIrbBlock()
    assert lib.fear_irb_workspace_bytes(ctypes.byref(blk), 1, 16, 16) == 0            # all-zero descriptor: unsupported shape
    assert lib.fear_irb_virtual_ok(ctypes.byref(blk)) == 0 and lib.fear_irb_virtual_ok(None) == 0
    blk.cin, blk.cexp, blk.cout, blk.k, blk.stride, blk.expand = 16, 96, 24, 3, 2, 1
    assert lib.fear_irb_virtual_ok(ctypes.byref(blk)) == 1 and lib.fear_irb_workspace_bytes(ctypes.byref(blk), 2, 32, 32) > 0
    blk.stride = 1
    assert lib.fear_irb_virtual_ok(ctypes.byref(blk)) == 0                             # (the stride-1 kernels keep their saved expansion)
    assert lib.fear_irb_train_forward(ctypes.byref(blk), None, None, None, 2, 32, 32, 0.1, 1e-5, None, 0, None) == -1
    # the plan query: host only; null and shape errors like the calls it describes (a virtual expansion at stride 1 is no shape)
    info = train_abi.FearIrbPlanInfo()
    assert lib.fear_irb_plan_info(ctypes.byref(blk), 2, 32, 32, None) == -1 and lib.fear_irb_plan_info(None, 2, 32, 32, ctypes.byref(info)) == -1
    assert lib.fear_irb_plan_info(ctypes.byref(blk), 2, 32, 32, ctypes.byref(info)) == 0 and (info.rows_in, info.rows_out, info.expand.present) == (2048, 2048, 1)
    assert lib.fear_irb_plan_info(ctypes.byref(blk), 2, 33, 32, ctypes.byref(info)) == 0 and lib.fear_irb_plan_info(ctypes.byref(blk), 0, 32, 32, ctypes.byref(info)) == -2
    blk.flags = FEAR_IRB_VIRTUAL_E
    assert lib.fear_irb_plan_info(ctypes.byref(blk), 2, 32, 32, ctypes.byref(info)) == -2
    blk.flags = 0
    pw = train_abi.FearPwbnPlanInfo()
    assert lib.fear_pwbn_plan_info(1024, 28, 16, 1, 0, None) == -1 and lib.fear_pwbn_plan_info(1024, 27, 16, 1, 0, ctypes.byref(pw)) == -2
    assert lib.fear_pwbn_plan_info(1024, 28, 16, 1, 1, ctypes.byref(pw)) == 0 and (pw.rows, pw.forward.present, pw.dx.present, pw.w.present) == (1024, 1, 0, 1)
    lay, shape = train_abi.FearLayerPlanInfo(), train_abi.FearLayerDwShape(1, 8, 8, 8, 3, 1, 8)
    assert lib.fear_layer_plan_info(1024, 32, 16, 0, None, None) == -1 and lib.fear_layer_plan_info(1024, 30, 16, 0, None, ctypes.byref(lay)) == -2
    assert lib.fear_layer_plan_info(1024, 32, 16, 0, None, ctypes.byref(lay)) == 0 and (lay.forward.lds, lay.forward.row_tile, lay.dw.workgroups) == (1, 64, 0)
    assert lib.fear_layer_plan_info(1024, 32, 16, 0, ctypes.byref(shape), ctypes.byref(lay)) == 0 and (lay.dw.strips, lay.dw.workgroups) == (2, 1)
    shape.ld = 6
    assert lib.fear_layer_plan_info(1024, 32, 16, 0, ctypes.byref(shape), ctypes.byref(lay)) == -2
    sep = th.FearSepLayer()
    assert lib.fear_sepbn_workspace_bytes(ctypes.byref(sep), 2, 16, 16) == 0
    sep.cin, sep.cout = 320, 256
    assert lib.fear_sepbn_workspace_bytes(ctypes.byref(sep), 2, 16, 16) > 0
    assert lib.fear_sepbn_train_forward(ctypes.byref(sep), None, 320, None, None, None, None, 256, 2, 16, 16, 0.1, 1e-5, None, 0, None) == -1
    assert lib.fear_stem_workspace_bytes(2, 255, 256) == 0 and lib.fear_stem_workspace_bytes(2, 256, 256) > 0
    assert lib.fear_stem_train_forward(None, None, None, None, None, None, None, None, None, 2, 256, 256, 0.1, 1e-5, None, 0, None) == -1


def test_training_operators_are_exported():
    """The C-ABI library exports every symbol include/fear_train.h declares, and the Python binding declares them all."""
    from feartracker_amd.train_head import TRAIN_SYMBOLS, load_train_library
    lib = load_train_library()
    declared = _declared("fear_train.h")
    assert len(declared) >= 18 and set(declared) == set(TRAIN_SYMBOLS)
    for sym in declared:
        assert hasattr(lib, sym)
    assert lib.fear_train_workspace_bytes(1024, 320) >= 320 * 320 * 4
    # null / shape errors need no GPU
    assert lib.fear_pw_forward(None, 0, None, None, None, 0, 16, 8, 8, None) == -1
    assert lib.fear_pw_backward_weight(None, 0, None, 0, None, None, 0, 16, 8, 8, None) == -1
    assert lib.fear_bn_train_forward(None, 0, None, None, None, 0, None, None, None, None, 0.1, 1e-5, 16, 8, 1, None, 0, None) == -1
    # layout rules are checked before anything touches the device: leading dimensions are multiples of 4 floats and cover the row
    import ctypes
    fake = ctypes.c_void_p(4096)
    assert lib.fear_pw_forward(fake, 10, fake, None, fake, 8, 16, 8, 8, None) == -2            # ldx % 4
    assert lib.fear_pw_forward(fake, 4, fake, None, fake, 8, 16, 8, 8, None) == -2             # ldx < K
    assert lib.fear_pw_backward_weight(fake, 8, fake, 6, fake, fake, 1 << 20, 16, 8, 8, None) == -2
    assert lib.fear_bn_train_forward(fake, 8, fake, fake, fake, 6, fake, fake, None, None, 0.1, 1e-5, 16, 8, 1, fake, 1 << 20, None) == -2
    assert lib.fear_dw_forward(fake, 8, fake, None, fake, 7, 1, 4, 4, 8, 3, 1, None) == -2
    assert lib.fear_bn_reduce(fake, 9, fake, 16, 8, fake, 1 << 20, None) == -2


def test_fixture_is_self_consistent(golden_dir):
    """The reference-generated fixture itself: FEARLoss recomputed from its stored outputs/targets with plain numpy."""
    d = np.load(f"{golden_dir}/head_train_step.npz")
    cls, lab = d["out_cls"].reshape(-1).astype(np.float64), d["gt_cls"].reshape(-1)
    bce = np.maximum(cls, 0) - cls * lab + np.log1p(np.exp(-np.abs(cls)))
    np.testing.assert_allclose(0.5 * bce[lab == 1].mean() + 0.5 * bce[lab == 0].mean(), d["loss_cls"], rtol=1e-6)
    p = d["out_bbox"].transpose(0, 2, 3, 1).reshape(-1, 4).astype(np.float64)
    t = d["gt_reg"].transpose(0, 2, 3, 1).reshape(-1, 4).astype(np.float64)
    sel = d["gt_weight"].reshape(-1) > 0
    p, t = p[sel], t[sel]
    inter = (np.minimum(p[:, 0], t[:, 0]) + np.minimum(p[:, 2], t[:, 2])) * (np.minimum(p[:, 3], t[:, 3]) + np.minimum(p[:, 1], t[:, 1]))
    union = (t[:, 0] + t[:, 2]) * (t[:, 1] + t[:, 3]) + (p[:, 0] + p[:, 2]) * (p[:, 1] + p[:, 3]) - inter
    np.testing.assert_allclose((1 - (inter + 1) / (union + 1)).mean(), d["loss_reg"], rtol=1e-6)
    assert sel.sum() == 3 * 13 and (d["gt_cls"][3] == 0).all()


def _close(got, ref, what, rel=1e-3):
    """|got - ref| <= rel * max|ref| + 1e-9 element-wise (gradient tensors span many magnitudes; the tensor's own scale is
    the yardstick, and biases in front of a BatchNorm have an exactly-zero true gradient)."""
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    ref = torch.as_tensor(ref).double().reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    tol = rel * float(ref.abs().max()) + 1e-9
    err = float((got - ref).abs().max())
    assert err <= tol, f"{what}: max abs err {err:.3e} > {tol:.3e} (max |ref| {float(ref.abs().max()):.3e})"
    return err / max(float(ref.abs().max()), 1e-30)


@pytest.mark.gpu
def test_head_training_step_matches_reference_autograd(golden_dir):
    from feartracker_amd.train_head import BoxTowerTrainHIP
    d = np.load(f"{golden_dir}/head_train_step.npz")
    sd = {k[len("param."):]: d[k] for k in d.files if k.startswith("param.")}
    net = BoxTowerTrainHIP(sd, device=0)
    out = net.step(torch.from_numpy(d["in_search"]), torch.from_numpy(d["in_template"]), torch.from_numpy(d["gt_reg"]),
                   torch.from_numpy(d["gt_cls"]), torch.from_numpy(d["gt_weight"]))
    torch.cuda.synchronize()
    # forward in train mode (BatchNorm on batch statistics)
    _close(out["bbox"], d["out_bbox"], "bbox")
    _close(out["cls"], d["out_cls"], "cls")
    assert abs(float(out["loss_cls"]) - float(d["loss_cls"])) <= 1e-5 * abs(float(d["loss_cls"]))
    assert abs(float(out["loss_reg"]) - float(d["loss_reg"])) <= 1e-5 * abs(float(d["loss_reg"]))
    # every parameter gradient, by reference name
    names = [k[len("grad."):] for k in d.files if k.startswith("grad.")]
    assert set(names) == set(out["grads"]) and len(names) == 54
    worst = {}
    for n in names:
        pre_bn_bias = n.endswith(".bias") and ("depthwise" in n or "pointwise" in n) and "pred" not in n
        ref = d["grad." + n]
        if pre_bn_bias:
            # a bias that feeds a BatchNorm has zero gradient; autograd returns rounding noise (1e-10), so do we
            assert float(np.abs(ref).max()) < 1e-8 and float(out["grads"][n].abs().max()) < 1e-7
            continue
        worst[n] = _close(out["grads"][n], ref, "grad " + n)
    # gradients w.r.t. the inputs (what the trunk's backward would receive)
    _close(out["grad_search"], d["grad_in_search"], "grad search features")
    _close(out["grad_template"], d["grad_in_template"], "grad template features")
    # BatchNorm running statistics after the step
    for k, v in net.running_stats().items():
        _close(v, d["after." + k], "running stat " + k, rel=1e-5)
    print("worst relative gradient errors:", sorted(worst.items(), key=lambda kv: -kv[1])[:3])
    # deterministic: the same step again gives bit-identical gradients (fixed-order reductions, no atomics)
    net2 = BoxTowerTrainHIP(sd, device=0)
    out2 = net2.step(torch.from_numpy(d["in_search"]), torch.from_numpy(d["in_template"]), torch.from_numpy(d["gt_reg"]),
                     torch.from_numpy(d["gt_cls"]), torch.from_numpy(d["gt_weight"]))
    for n in names:
        assert torch.equal(out["grads"][n], out2["grads"][n]), n


RECT_DW_CASES = ((2, 8, 20, 64, 5, 1), (2, 12, 32, 96, 3, 2), (1, 40, 6, 144, 5, 2))       # B, H, W, C, k, stride


@pytest.mark.gpu
def test_training_operators_individually_vs_torch():
    """Each heavy operator against the same operator written with torch ops on the GPU tensors' CPU copies (fp32 reference
    of the same op): pointwise forward / dgrad / wgrad, depthwise dgrad / wgrad, BatchNorm train forward / backward, the
    correlation's two gradients — at sizes that are not the fixture's (ragged row counts, 320 channels, 5x5 taps)."""
    import torch.nn.functional as F
    from feartracker_amd.train_head import _p, load_train_library
    lib = load_train_library()
    dev = torch.device("cuda:0")
    st = None
    keep = []                     # device tensors handed to the C ABI by pointer must outlive the (asynchronous) calls

    def D(t):
        keep.append(t.detach().to(dev).contiguous())
        return keep[-1]

    g = torch.Generator().manual_seed(3)
    ws = torch.empty(lib.fear_train_workspace_bytes(4096, 320) // 4 + 1024, device=dev)
    wsb = ws.numel() * 4
    # (K <= 32 takes pw_wgrad_smallk_kernel: 16 / 28 / 24 / 32 input channels, ragged row counts, several row slices)
    for M, K, N in ((1000, 320, 256), (2304, 256, 4), (130, 64, 112), (5000, 16, 96), (3001, 28, 16), (70000, 16, 16), (2050, 24, 144),
                    (1111, 32, 192), (9, 4, 8)):
        x, w, dy = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.1, torch.randn(M, N, generator=g)
        b = torch.randn(N, generator=g)
        xd, wd, dyd, bd = x.to(dev), w.to(dev), dy.to(dev), b.to(dev)
        y = torch.empty(M, N, device=dev)
        assert lib.fear_pw_forward(_p(xd), K, _p(wd), _p(bd), _p(y), N, M, K, N, st) == 0
        _close(y, x @ w.t() + b, "pw forward", 1e-5)
        dx = torch.empty(M, K, device=dev)
        assert lib.fear_pw_backward_data(_p(dyd), N, _p(wd), None, 0, _p(dx), K, M, K, N, st) == 0
        _close(dx, dy @ w, "pw dgrad", 1e-5)
        dw = torch.empty(N, K, device=dev)
        assert lib.fear_pw_backward_weight(_p(dyd), N, _p(xd), K, _p(dw), _p(ws), wsb, M, K, N, st) == 0
        _close(dw, dy.t() @ x, "pw wgrad", 1e-5)
        db = torch.empty(N, device=dev)
        assert lib.fear_col_sum(_p(dyd), N, _p(db), _p(ws), wsb, M, N, st) == 0
        _close(db, dy.sum(0), "bias grad", 1e-5)
    def dw_case(B, H, W, C, k, st_, g):
        x = torch.randn(B, C, H, W, generator=g, requires_grad=True)
        w = torch.randn(C, 1, k, k, generator=g, requires_grad=True)
        y = F.conv2d(x, w, None, stride=st_, padding=k // 2, groups=C)
        Ho, Wo = H // st_, W // st_
        dy = torch.randn(y.shape, generator=g)
        y.backward(dy)
        rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1, C).contiguous()
        taps = D(w.detach().reshape(C, k * k).t())
        yd = torch.empty(B * Ho * Wo, C, device=dev)
        assert lib.fear_dw_forward(_p(D(rows(x))), C, _p(taps), None, _p(yd), C, B, H, W, C, k, st_, st) == 0
        _close(yd, rows(y), f"dw forward {H}x{W}", 1e-5)
        dxd = torch.empty(B * H * W, C, device=dev)
        assert lib.fear_dw_backward_data(_p(D(rows(dy))), C, _p(taps), _p(dxd), C, B, H, W, C, k, st_, st) == 0
        _close(dxd, rows(x.grad), f"dw dgrad {H}x{W}", 1e-5)
        dtaps = torch.empty(k * k, C, device=dev)
        assert lib.fear_dw_backward_weight(_p(D(rows(dy))), C, _p(D(rows(x))), C, _p(dtaps), _p(ws), wsb, B, H, W, C, k, st_, st) == 0
        _close(dtaps, w.grad.reshape(C, k * k).t(), f"dw wgrad {H}x{W}", 1e-5)

    for B, H, C, k, st_ in ((3, 16, 320, 3, 1), (2, 8, 64, 5, 1), (2, 32, 96, 3, 2), (2, 16, 144, 5, 2)):
        dw_case(B, H, H, C, k, st_, g)
    # ... and on rectangular maps (H != W: tile counts, halo indices and Ho / Wo must not be swapped anywhere) — from a generator of
    # their own, so that the draws of the sections below stay what they were
    g_rect = torch.Generator().manual_seed(33)
    for B, H, W, C, k, st_ in RECT_DW_CASES:
        dw_case(B, H, W, C, k, st_, g_rect)
    for M, C, relu in ((1024, 256, 1), (777, 112, 0)):
        x = (torch.randn(M, C, generator=g) * 2 + 0.5).requires_grad_(True)
        gamma, beta = (torch.rand(C, generator=g) + 0.5).requires_grad_(True), torch.randn(C, generator=g).requires_grad_(True)
        rm, rv = torch.zeros(C), torch.ones(C)
        y = F.batch_norm(x, rm, rv, gamma, beta, training=True, momentum=0.1, eps=1e-5)
        y = F.relu(y) if relu else y
        dy = torch.randn(M, C, generator=g)
        y.backward(dy)
        xd, yd = x.detach().to(dev), torch.empty(M, C, device=dev)
        mean, rstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
        rmd, rvd = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        assert lib.fear_bn_train_forward(_p(xd), C, _p(D(gamma)), _p(D(beta)), _p(yd), C, _p(mean), _p(rstd),
                                         _p(rmd), _p(rvd), 0.1, 1e-5, M, C, relu, _p(ws), wsb, st) == 0
        _close(yd, y.detach(), "bn forward", 1e-5)
        _close(rmd, rm, "running mean", 1e-5)
        _close(rvd, rv, "running var", 1e-5)
        dxd, dg, db = torch.empty(M, C, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
        assert lib.fear_bn_train_backward(_p(D(dy)), C, _p(yd) if relu else None, C, _p(xd), C, _p(mean), _p(rstd),
                                          _p(D(gamma)), _p(dxd), C, _p(dg), _p(db), M, C, _p(ws), wsb, st) == 0
        _close(dxd, x.grad, "bn dx", 1e-4)
        _close(dg, gamma.grad, "bn dgamma", 1e-4)
        _close(db, beta.grad, "bn dbeta", 1e-4)
    # stem conv 3x3 s2 (3 -> 16) as im2col + GEMM: forward and weight gradient
    img = torch.randn(2, 3, 64, 64, generator=g)
    ws_ = torch.randn(16, 3, 3, 3, generator=g, requires_grad=True)
    ys = F.conv2d(img, ws_, None, stride=2, padding=1)
    dys = torch.randn(ys.shape, generator=g)
    ys.backward(dys)
    Ms = 2 * 32 * 32
    col = torch.empty(Ms, 28, device=dev)
    assert lib.fear_stem_im2col(_p(D(img)), _p(col), 2, 64, 64, st) == 0
    w28 = torch.zeros(16, 28)
    w28[:, :27] = ws_.detach().reshape(16, 27)
    yd = torch.empty(Ms, 16, device=dev)
    assert lib.fear_pw_forward(_p(col), 28, _p(D(w28)), None, _p(yd), 16, Ms, 28, 16, st) == 0
    _close(yd, ys.detach().permute(0, 2, 3, 1).reshape(Ms, 16), "stem forward", 1e-5)
    dw28 = torch.empty(16, 28, device=dev)
    assert lib.fear_pw_backward_weight(_p(D(dys.permute(0, 2, 3, 1).reshape(Ms, 16))), 16, _p(col), 28, _p(dw28), _p(ws),
                                       wsb, Ms, 28, 16, st) == 0
    _close(dw28[:, :27], ws_.grad.reshape(16, 27), "stem wgrad", 1e-5)
    B, P, C, J = 3, 256, 256, 64
    x = torch.randn(B, P, C, generator=g, requires_grad=True)
    z = torch.randn(B, C, J, generator=g, requires_grad=True)
    s = torch.matmul(x, z)
    ds = torch.randn(s.shape, generator=g)
    s.backward(ds)
    xd, zd = x.detach().reshape(B * P, C).to(dev), z.detach().to(dev)
    sd_ = torch.empty(B * P, J, device=dev)
    assert lib.fear_xcorr_forward(_p(xd), C, _p(zd), _p(sd_), J, B, P, C, J, st) == 0
    _close(sd_, s.detach().reshape(B * P, J), "xcorr forward", 1e-5)
    dxd, dzd = torch.empty(B * P, C, device=dev), torch.empty(B, C, J, device=dev)
    add = torch.randn(B * P, C, generator=g)
    assert lib.fear_xcorr_backward(_p(D(ds.reshape(B * P, J))), J, _p(xd), C, _p(zd), _p(D(add)), C, _p(dxd), C, _p(dzd),
                                   B, P, C, J, st) == 0
    torch.cuda.synchronize()
    _close(dxd, x.grad.reshape(B * P, C) + add, "xcorr dx", 1e-5)
    _close(dzd, z.grad, "xcorr dz", 1e-5)


def test_training_oracle_head_matches_reference_fixture(golden_dir):
    """Pins oracle/fear_train_oracle.py's head + loss restatement against the REFERENCE's BoxTower + FEARLoss + autograd
    (fixture of tools/make_golden.py section 11): same outputs, losses and gradients on CPU."""
    from oracle.fear_train_oracle import BoxTowerOracle, fear_loss
    d = np.load(f"{golden_dir}/head_train_step.npz")
    net = BoxTowerOracle().train()
    sd = {k[len("param."):]: torch.from_numpy(d[k]) for k in d.files if k.startswith("param.")}
    missing = net.load_state_dict(sd, strict=True)
    xs = torch.from_numpy(d["in_search"]).requires_grad_(True)
    zs = torch.from_numpy(d["in_template"]).requires_grad_(True)
    bbox, cls = net(xs, zs)
    lc, lr = fear_loss(bbox, cls, torch.from_numpy(d["gt_reg"]), torch.from_numpy(d["gt_cls"]), torch.from_numpy(d["gt_weight"]))
    (lc + lr).backward()
    np.testing.assert_allclose(bbox.detach().numpy(), d["out_bbox"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(cls.detach().numpy(), d["out_cls"], rtol=1e-5, atol=1e-7)
    assert abs(float(lc) - float(d["loss_cls"])) < 1e-6 and abs(float(lr) - float(d["loss_reg"])) < 1e-6
    for n, p in net.named_parameters():
        _close(p.grad, d["grad." + n], "oracle grad " + n, 1e-4)
    _close(xs.grad, d["grad_in_search"], "oracle grad search", 1e-4)
    _close(zs.grad, d["grad_in_template"], "oracle grad template", 1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("fused,B", [(False, 2), (True, 2), ("block", 2), (False, 16), (True, 16), ("block", 16)],
                         ids=["layerwise_b2", "fused_conv_bn_b2", "block_b2", "layerwise_b16", "fused_conv_bn_b16", "block_b16"])
def test_whole_network_training_step_matches_autograd(fused, B):
    """BASELINE configs[4] "backbone + xcorr fwd/bwd, random-init": FEARNet.forward((template, search)) in train mode +
    FEARLoss + backward to all 195 parameter tensors on the HIP operators vs torch autograd on the restated graph
    (oracle/fear_train_oracle.py: head pinned by the reference fixture, trunk = FBNet-C blocks with a BatchNorm after every
    conv — the reference's own trunk code is the absent mobile_cv package).  Tolerance 1e-3 of each tensor's max-norm."""
    from feartracker_amd.train_net import FEARNetTrainHIP
    from oracle.fear_train_oracle import FEARNetTrainOracle, fear_loss, random_init_state
    sd = random_init_state(5)
    ora = FEARNetTrainOracle().train()
    ora.load_state_dict(sd, strict=False)
    # B = 16: train-mode BatchNorm couples the crops of a batch, so gradient parity at a batch size is only
    # shown by running the oracle at THAT size — 16 pairs is what CPU autograd does in seconds; a sample of a larger batch has no
    # oracle of its own (its statistics are the whole batch's), which is why the 128-pair test below stays a property test
    g = torch.Generator().manual_seed(9 + B)
    tmpl = torch.randn(B, 3, 128, 128, generator=g)
    srch = torch.randn(B, 3, 256, 256, generator=g)
    gt_reg = torch.rand(B, 4, 16, 16, generator=g) * 60 + 1
    gt_cls = (torch.rand(B, 1, 16, 16, generator=g) > 0.8).float()
    gt_w = (torch.rand(B, 16, 16, generator=g) > 0.85).float()
    # all three implementations of the trunk's conv + BatchNorm units ("block": one call per inverted-residual block, the default)
    net = FEARNetTrainHIP(sd, device=0, mode="block") if fused == "block" else FEARNetTrainHIP(sd, device=0, fused=fused)
    assert net.mode == {False: "layerwise", True: "fused", "block": "block"}[fused]
    out = net.step(tmpl, srch, gt_reg, gt_cls, gt_w)
    torch.cuda.synchronize()
    # the oracle's backward runs on the HIP forward's ReLU activity pattern (oracle/fear_train_oracle.py::MaskableReLU: the
    # derivative at a pre-activation within rounding of 0 is a tie-break, not arithmetic); the two forwards must agree first
    with torch.no_grad():
        bbox0, cls0 = copy.deepcopy(ora)(tmpl, srch)
    _close(out["bbox"], bbox0, "bbox (plain forward)", 1e-4)
    _close(out["cls"], cls0, "cls (plain forward)", 1e-4)
    pats = net.relu_patterns()
    n_relu = 0

    def resolve(root, dotted):
        for part in dotted.split("."):
            root = root[int(part)] if part.isdigit() else getattr(root, part)
        return root

    for name, masks in pats.items():
        if name == "stem" or name.startswith("trunk."):
            target = resolve(ora, name).act                      # ConvBN of the trunk
        else:                                                    # head: name = the BatchNorm inside BoxTower, its ReLU is the next module
            parent, idx = name.rsplit(".", 1)
            target = resolve(ora.connect_model, parent)[int(idx) + 1]
        target.masks = list(masks)
        n_relu += len(masks)
    assert n_relu == 2 * 30 + 8                    # stem + 13 expand + 16 depthwise ReLUs per trunk pass, 8 in the head
    bbox, cls = ora(tmpl, srch)
    lc, lr = fear_loss(bbox, cls, gt_reg, gt_cls, gt_w)
    (lc + lr).backward()
    _close(out["bbox"], bbox.detach(), "bbox")
    _close(out["cls"], cls.detach(), "cls")
    assert abs(float(out["loss_cls"]) - float(lc.detach())) <= 1e-4 * abs(float(lc.detach()))
    assert abs(float(out["loss_reg"]) - float(lr.detach())) <= 1e-4 * abs(float(lr.detach()))
    ref = {n: p.grad for n, p in ora.named_parameters()}
    assert set(ref) == set(out["grads"]) and len(ref) == 195, set(ref) ^ set(out["grads"])
    worst = {}
    for n, gr in ref.items():
        if float(gr.abs().max()) < 1e-7:                     # biases in front of a BatchNorm: exactly-zero true gradient (both sides hold rounding noise, 1e-8)
            assert float(out["grads"][n].abs().max()) < 1e-6
            continue
        worst[n] = _close(out["grads"][n], gr, "grad " + n)
    print("worst relative gradient errors:", sorted(worst.items(), key=lambda kv: -kv[1])[:4])


def _loss_edge_cases(golden_dir):
    d = np.load(f"{golden_dir}/loss_edge.npz")
    for tag in ("one_pos", "two_pos", "one_neg"):
        yield tag, {k[len(tag) + 1:]: d[k] for k in d.files if k.startswith(tag + "_")}


def test_training_oracle_loss_on_single_cell_selections(golden_dir):
    """The reference's FEARLoss indexes with `.nonzero().squeeze()` (loss.py:77-78): exactly one positive (or negative) cell
    makes that half of the classification loss a constant 0.  Fixture = the reference's own FEARLoss + autograd
    (tools/make_golden.py section 11b); the oracle restatement must reproduce value and gradient."""
    from oracle.fear_train_oracle import fear_loss
    for tag, c in _loss_edge_cases(golden_dir):
        bbox = torch.from_numpy(c["bbox"]).requires_grad_(True)
        cls = torch.from_numpy(c["cls"]).requires_grad_(True)
        lc, lr = fear_loss(bbox, cls, torch.from_numpy(c["gt_reg"]), torch.from_numpy(c["gt_cls"]), torch.from_numpy(c["gt_weight"]))
        (lc + lr).backward()
        assert abs(float(lc) - float(c["loss_cls"])) < 1e-6 and abs(float(lr) - float(c["loss_reg"])) < 1e-6, tag
        np.testing.assert_allclose(cls.grad.numpy(), c["dcls"], rtol=1e-5, atol=1e-8, err_msg=tag)
        np.testing.assert_allclose(bbox.grad.numpy(), c["dbbox"], rtol=1e-5, atol=1e-8, err_msg=tag)
    one = dict(_loss_edge_cases(golden_dir))["one_pos"]
    assert np.count_nonzero(one["dcls"].reshape(-1)[one["gt_cls"].reshape(-1) == 1]) == 0      # the lone positive gets no gradient


@pytest.mark.gpu
def test_head_loss_operator_on_single_cell_selections(golden_dir):
    """fear_head_loss through the C ABI on the same fixture: one positive / two positives / one negative cell, values and both
    gradients; and the stated deviation — no positive cell at all gives 0 for that half (torch: NaN), finite gradients."""
    from feartracker_amd.train_head import _p, load_train_library
    lib = load_train_library()
    dev = torch.device("cuda:0")
    ws = torch.empty(lib.fear_train_workspace_bytes(4096, 320) // 4 + 1024, device=dev)

    def run(bbox, cls, gt_reg, gt_cls, gt_w):
        M = 256
        rows = lambda a, c: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).reshape(c, M).T)).to(dev).contiguous()
        b, c_, gr = rows(bbox, 4), rows(cls, 1).reshape(M), rows(gt_reg, 4)
        gc = torch.from_numpy(np.asarray(gt_cls, np.float32).reshape(M)).to(dev)
        gw = torch.from_numpy(np.asarray(gt_w, np.float32).reshape(M)).to(dev)
        losses, db, dc = torch.zeros(2, device=dev), torch.empty(M, 4, device=dev), torch.empty(M, device=dev)
        assert lib.fear_head_loss(_p(b), _p(c_), _p(gr), _p(gc), _p(gw), 1.0, 1.0, _p(losses), _p(db), _p(dc), _p(ws),
                                  ws.numel() * 4, M, None) == 0
        torch.cuda.synchronize()
        return losses.cpu().numpy(), db.cpu().numpy().T.reshape(1, 4, 16, 16), dc.cpu().numpy().reshape(1, 1, 16, 16)

    for tag, c in _loss_edge_cases(golden_dir):
        losses, db, dc = run(c["bbox"], c["cls"], c["gt_reg"], c["gt_cls"], c["gt_weight"])
        np.testing.assert_allclose(losses, [c["loss_cls"], c["loss_reg"]], rtol=2e-6, err_msg=tag)
        np.testing.assert_allclose(dc, c["dcls"], rtol=2e-5, atol=1e-8, err_msg=tag)
        np.testing.assert_allclose(db, c["dbbox"], rtol=2e-5, atol=1e-8, err_msg=tag)
    c = dict(_loss_edge_cases(golden_dir))["two_pos"]
    losses, db, dc = run(c["bbox"], c["cls"], c["gt_reg"], np.zeros_like(c["gt_cls"]), np.zeros_like(c["gt_weight"]))
    assert np.isfinite(losses).all() and np.isfinite(dc).all() and np.isfinite(db).all() and losses[1] == 0.0
    x = c["cls"].reshape(-1).astype(np.float64)
    np.testing.assert_allclose(losses[0], 0.5 * np.mean(np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))), rtol=2e-6)


@pytest.mark.gpu
def test_fused_conv_bn_operators_individually_vs_torch():
    """The fused trunk operators (include/fear_train.h, "fused conv + BatchNorm"): producers with the activation applied on load
    and the column sums from the same pass, fear_bn_finalize, fear_bn_act, the backward pair with the mask recomputed from the
    raw tensor, and the two weight gradients with act-on-load — each against torch ops on CPU copies, ragged sizes."""
    import torch.nn.functional as F
    from feartracker_amd.train_head import _p, load_train_library
    lib = load_train_library()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11)
    keep = []

    def D(t, dtype=torch.float32):
        keep.append(t.detach().to(dev, dtype).contiguous())
        return keep[-1]

    ws = torch.empty(max(lib.fear_train_workspace_bytes(8192, 320), lib.fear_train_stats_workspace_bytes(8192, 320)) // 4 + 1024, device=dev)
    wsb = ws.numel() * 4

    def act(x, a, b, relu):
        y = x * a + b                      # (the kernel's fma differs from mul+add by one rounding: compared at 1e-6)
        return y.clamp_min(0) if relu else y

    # ---- pointwise producer: Y = act(X) W^T, sums of Y
    for M, K, N, relu in ((1000, 96, 24, 1), (130, 16, 96, 0), (4096, 28, 16, None), (333, 672, 112, 1)):
        x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.2
        a, b = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.3
        y, sums = torch.empty(M, N, device=dev), torch.empty(2 * N, dtype=torch.float64, device=dev)
        ia, ib = (None, None) if relu is None else (_p(D(a)), _p(D(b)))
        assert lib.fear_pw_forward_stats(_p(D(x)), K, ia, ib, int(bool(relu)), _p(D(w)), _p(y), N, M, K, N, _p(sums), _p(ws), wsb, None) == 0
        ref = (x if relu is None else act(x, a, b, relu)) @ w.t()
        _close(y, ref, f"pw producer {M}x{K}x{N}", 2e-5)
        yd = y.cpu().double()
        np.testing.assert_allclose(sums.cpu().numpy(), torch.cat([yd.sum(0), (yd * yd).sum(0)]).numpy(), rtol=2e-6, atol=1e-6)
    # ---- depthwise producer
    def dw_producer_case(B, H, W, C, k, st_, relu, g):
        x = torch.randn(B, C, H, W, generator=g)
        wt = torch.randn(C, 1, k, k, generator=g) * 0.3
        a, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
        xr = D(x.permute(0, 2, 3, 1).reshape(-1, C))
        taps = D(wt.reshape(C, k * k).t())
        Ho, Wo = H // st_, W // st_
        y, sums = torch.empty(B * Ho * Wo, C, device=dev), torch.empty(2 * C, dtype=torch.float64, device=dev)
        ia, ib = (None, None) if relu is None else (_p(D(a)), _p(D(b)))
        assert lib.fear_dw_forward_stats(_p(xr), C, ia, ib, int(bool(relu)), _p(taps), _p(y), C, B, H, W, C, k, st_, _p(sums), _p(ws), wsb, None) == 0
        xin = x if relu is None else act(x, a.view(1, C, 1, 1), b.view(1, C, 1, 1), relu)
        ref = F.conv2d(xin, wt, stride=st_, padding=k // 2, groups=C).permute(0, 2, 3, 1).reshape(-1, C)
        _close(y, ref, f"dw producer {B}x{C}x{H}x{W} k{k}s{st_}", 2e-5)
        yd = y.cpu().double()
        np.testing.assert_allclose(sums.cpu().numpy(), torch.cat([yd.sum(0), (yd * yd).sum(0)]).numpy(), rtol=2e-6, atol=1e-6)

    for B, H, C, k, st_, relu in ((3, 16, 96, 3, 2, 1), (2, 8, 64, 5, 1, 1), (2, 32, 16, 3, 1, None), (1, 16, 144, 5, 2, 0), (2, 16, 672, 5, 1, 1)):
        dw_producer_case(B, H, H, C, k, st_, relu, g)
    # ---- finalize + act + backward pair on one BatchNorm (+ReLU), vs autograd
    for M, C, relu in ((777, 96, 1), (1024, 24, 0)):
        x = torch.randn(M, C, generator=g) * 2 + 0.5
        gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
        res = torch.randn(M, C, generator=g)
        dy = torch.randn(M, C, generator=g)
        xd = x.double()
        sums = D(torch.cat([xd.sum(0), (xd * xd).sum(0)]), torch.float64)
        mean, rstd, a, b = (torch.empty(C, device=dev) for _ in range(4))
        rm, rv = D(torch.zeros(C)), D(torch.ones(C))
        assert lib.fear_bn_finalize(_p(sums), float(M), _p(D(gamma)), _p(D(beta)), _p(mean), _p(rstd), _p(a), _p(b), _p(rm), _p(rv), 0.1, 1e-5, C, None) == 0
        xt = x.clone().requires_grad_(True)
        bn = torch.nn.BatchNorm2d(C).train()
        with torch.no_grad():
            bn.weight.copy_(gamma); bn.bias.copy_(beta)
        yt = bn(xt.t().reshape(1, C, M, 1))
        yt = (F.relu(yt) if relu else yt).reshape(C, M).t()
        yt.backward(dy)
        _close(mean, x.mean(0), "mean", 1e-5)
        _close(rm, bn.running_mean, "running_mean", 1e-5)
        _close(rv, bn.running_var, "running_var", 1e-5)
        out = torch.empty(M, C, device=dev)
        assert lib.fear_bn_act(_p(D(x)), C, _p(a), _p(b), relu, _p(D(res)), C, _p(out), C, M, C, None) == 0
        _close(out, yt.detach() + res, "bn_act + residual", 2e-5)
        s2 = torch.empty(2 * C, dtype=torch.float64, device=dev)
        assert lib.fear_bn_backward_reduce_x(_p(D(dy)), C, _p(D(x)), C, _p(a), _p(b), relu, _p(mean), _p(rstd), _p(s2), M, C, _p(ws), wsb, None) == 0
        dx, dg, db = torch.empty(M, C, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
        assert lib.fear_bn_backward_apply_x(_p(D(dy)), C, _p(D(x)), C, _p(a), _p(b), relu, _p(mean), _p(rstd), _p(D(gamma)), _p(s2), float(M),
                                            _p(s2), _p(dx), C, _p(dg), _p(db), _p(ws), wsb, M, C, None) == 0
        _close(dx, xt.grad, "bn backward dx", 2e-4)
        _close(dg, bn.weight.grad, "bn backward dgamma", 2e-4)
        _close(db, bn.bias.grad, "bn backward dbeta", 2e-4)
    # ---- weight gradients with the activation applied to their x operand on load
    M, K, N = 3000, 96, 24
    x, dy = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g)
    a, b = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.3
    dw = torch.empty(N, K, device=dev)
    assert lib.fear_pw_backward_weight_act(_p(D(dy)), N, _p(D(x)), K, _p(D(a)), _p(D(b)), 1, _p(dw), _p(ws), wsb, M, K, N, None) == 0
    _close(dw, dy.t() @ act(x, a, b, 1), "pw wgrad act", 2e-5)
    for M, K, N, relu in ((4100, 16, 96, 1), (3000, 24, 144, 0), (2500, 32, 64, 1)):      # the K <= 32 kernel applies it per scalar
        x, dy = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g)
        a, b = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.3
        dw = torch.empty(N, K, device=dev)
        assert lib.fear_pw_backward_weight_act(_p(D(dy)), N, _p(D(x)), K, _p(D(a)), _p(D(b)), relu, _p(dw), _p(ws), wsb, M, K, N, None) == 0
        _close(dw, dy.t() @ act(x, a, b, relu), f"pw wgrad act K={K}", 2e-5)
    def dw_wgrad_act_case(B, H, W, C, k, st_, g):
        x = torch.randn(B, C, H, W, generator=g)
        a, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
        wt = torch.zeros(C, 1, k, k, requires_grad=True)
        dyt = torch.randn(B, C, H // st_, W // st_, generator=g)
        F.conv2d(act(x, a.view(1, C, 1, 1), b.view(1, C, 1, 1), 1), wt, stride=st_, padding=k // 2, groups=C).backward(dyt)
        dtaps = torch.empty(k * k, C, device=dev)
        assert lib.fear_dw_backward_weight_act(_p(D(dyt.permute(0, 2, 3, 1).reshape(-1, C))), C, _p(D(x.permute(0, 2, 3, 1).reshape(-1, C))), C,
                                               _p(D(a)), _p(D(b)), 1, _p(dtaps), _p(ws), wsb, B, H, W, C, k, st_, None) == 0
        _close(dtaps, wt.grad.reshape(C, k * k).t(), f"dw wgrad act {H}x{W} k{k}s{st_}", 2e-5)

    for B, H, C, k, st_ in ((2, 16, 96, 3, 2), (2, 8, 64, 5, 1), (3, 12, 32, 3, 1)):
        dw_wgrad_act_case(B, H, H, C, k, st_, g)
    # ---- the `_stats` / `_act` depthwise forms on rectangular maps (a generator of their own: the draws above stay what they were)
    g_rect = torch.Generator().manual_seed(34)
    for B, H, W, C, k, st_ in RECT_DW_CASES:
        dw_producer_case(B, H, W, C, k, st_, 1, g_rect)
        dw_wgrad_act_case(B, H, W, C, k, st_, g_rect)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_fused_training_step_equals_the_layerwise_one():
    """FEARNetTrainHIP(fused=True) — activations applied on load, statistics from the producers — against fused=False (one
    kernel per layer and direction, the implementation the autograd / reference fixtures pinned first): same losses, every
    one of the 195 gradients equal to the layer-wise step's — median difference under 1e-2, no tensor more than a quarter off (per-channel cancelling sums behind a flipped ReLU move by percents; the two
    differ by fma-vs-mul+add roundings of the BatchNorm affine, which can flip a ReLU at a pre-activation of ~1e-7), same running statistics; and the fused step keeps half as many saved floats."""
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    B = 4
    g = torch.Generator().manual_seed(21)
    tmpl, srch = torch.randn(B, 3, 128, 128, generator=g), torch.randn(B, 3, 256, 256, generator=g)
    gt_reg = torch.rand(B, 4, 16, 16, generator=g) * 60 + 1
    gt_cls = (torch.rand(B, 1, 16, 16, generator=g) > 0.8).float()
    gt_w = (torch.rand(B, 16, 16, generator=g) > 0.9).float()
    sd = random_init_state(9)
    outs, stats = {}, {}
    for fused in (False, True, "block"):
        net = FEARNetTrainHIP(sd, device=0, mode="block") if fused == "block" else FEARNetTrainHIP(sd, device=0, fused=fused)
        outs[fused] = net.step(tmpl, srch, gt_reg, gt_cls, gt_w)
        stats[fused] = {k: v.cpu() for k, v in net.running_stats().items()}
        torch.cuda.synchronize()
    for other in (True, "block"):
        _compare_steps(outs[False], outs[other], stats[False], stats[other], str(other))


def _compare_steps(out_ref, out_got, stats_ref, stats_got, tag):
    outs, stats = {False: out_ref, True: out_got}, {False: stats_ref, True: stats_got}
    for k in ("loss_cls", "loss_reg"):
        assert abs(float(outs[True][k]) - float(outs[False][k])) <= 1e-5 * abs(float(outs[False][k])), k
    assert set(outs[True]["grads"]) == set(outs[False]["grads"]) and len(outs[True]["grads"]) == 195
    worst, errs = 0.0, []
    for k, ref in outs[False]["grads"].items():
        got = outs[True]["grads"][k]
        # a bias in front of a BatchNorm has an exactly-zero true gradient and both sides hold rounding noise: recognised by its
        # size against the gradient of the weight it belongs to
        sib = outs[False]["grads"].get(k[: -len("bias")] + "weight") if k.endswith("bias") else None
        if sib is not None and float(ref.abs().max()) < 1e-4 * float(sib.abs().max()):
            assert float(got.abs().max()) < 1e-3 * float(sib.abs().max()), k
            continue
        err = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12))
        worst = max(worst, err)
        # per-channel gradients (BatchNorm affine, conv biases) are cancelling sums over the batch: one pre-activation within
        # 1e-7 of zero that the two forwards resolve differently moves them by up to a percent (the reason the
        # autograd test pins the ReLU pattern); the weight tensors are not sensitive to that
        errs.append(err)
        assert err < 0.25, (k, err)            # (each implementation's gradients are pinned one by one against autograd, with the ReLU
                                               #  pattern held fixed, in test_whole_network_training_step_matches_autograd)
    for k, ref in stats[False].items():
        assert float((stats[True][k] - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max())), k
    # the two forwards differ by roundings that flip a few ReLUs at pre-activations of ~1e-7; everything behind them moves by 1e-3
    assert float(np.median(errs)) < 1e-2, float(np.median(errs))
    print(f"{tag} vs layer-wise: median relative gradient difference {np.median(errs):.2e}, worst {worst:.2e}")


@pytest.mark.gpu
def test_training_step_at_the_config_size_is_finite_and_reproducible():
    """BASELINE configs[4]'s per-rank workload, 128 pairs (the size bench.py times), layer-wise and fused: finite losses and
    gradients, bit-identical across two runs of the same step (every reduction is fixed-order), and BatchNorm of two 64-pair halves with added sums =
    the 128-pair statistics (what SyncBatchNorm over two ranks computes) on the widest producer of the trunk."""
    from feartracker_amd.train_head import _p, load_train_library
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    B = 128
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(31)
    tmpl, srch = torch.randn(B, 3, 128, 128, generator=g).to(dev), torch.randn(B, 3, 256, 256, generator=g).to(dev)
    gt_reg = (torch.rand(B, 4, 16, 16, generator=g) * 60 + 1).to(dev)
    gt_cls = (torch.rand(B, 1, 16, 16, generator=g) > 0.8).float().to(dev)
    gt_w = (torch.rand(B, 16, 16, generator=g) > 0.9).float().to(dev)
    sd = random_init_state(3)
    runs = []
    for fused in (False, False, True, True, "block", "block"):
        net = FEARNetTrainHIP(sd, device=0, mode="block") if fused == "block" else FEARNetTrainHIP(sd, device=0, fused=fused)
        out = net.step(tmpl, srch, gt_reg, gt_cls, gt_w)
        torch.cuda.synchronize()
        runs.append({k: v.clone() for k, v in out["grads"].items()} | {"loss": torch.tensor([float(out["loss_cls"]), float(out["loss_reg"])])})
        del net, out
        torch.cuda.empty_cache()
    for i in (0, 2, 4):                                       # the layer-wise step, the fused one, the block-fused one
        assert torch.isfinite(runs[i]["loss"]).all()
        for k, v in runs[i].items():
            assert torch.isfinite(v).all(), k
            assert torch.equal(v, runs[i + 1][k]), f"{k} differs between two runs of the same step (fused={i > 0})"
    assert float((runs[0]["loss"] - runs[2]["loss"]).abs().max()) < 1e-4 and float((runs[0]["loss"] - runs[4]["loss"]).abs().max()) < 1e-4
    # two half batches, sums added = the full batch (16 -> 96 channels at 128x128: 2.1 M rows)
    lib = load_train_library()
    M, K, N = B * 128 * 128, 16, 96
    x = torch.randn(M, K, generator=g).to(dev)
    w = (torch.randn(N, K, generator=g) * 0.3).to(dev)
    ws = torch.empty(max(lib.fear_train_workspace_bytes(M, 96), lib.fear_train_stats_workspace_bytes(M, 96)) // 4 + 1024, device=dev)
    y = torch.empty(M, N, device=dev)
    full, h0, h1 = (torch.empty(2 * N, dtype=torch.float64, device=dev) for _ in range(3))
    assert lib.fear_pw_forward_stats(_p(x), K, None, None, 0, _p(w), _p(y), N, M, K, N, _p(full), _p(ws), ws.numel() * 4, None) == 0
    assert lib.fear_pw_forward_stats(_p(x), K, None, None, 0, _p(w), _p(y), N, M // 2, K, N, _p(h0), _p(ws), ws.numel() * 4, None) == 0
    assert lib.fear_pw_forward_stats(_p(x[M // 2:]), K, None, None, 0, _p(w), _p(y[M // 2:]), N, M // 2, K, N, _p(h1), _p(ws), ws.numel() * 4, None) == 0
    torch.cuda.synchronize()
    np.testing.assert_allclose((h0 + h1).cpu().numpy(), full.cpu().numpy(), rtol=1e-12)
    yd = y[: 1 << 16].double()
    assert torch.isfinite(full).all() and float(full[N:].min()) > 0 and abs(float(yd.sum())) < 1e12



@pytest.mark.gpu
def test_deferred_running_statistics_in_one_launch_equal_the_per_batchnorm_updates():
    """fear_bn_running_update_multi (the search pass's 47 deferred running-statistics updates as one launch) against
    fear_bn_running_update item by item."""
    import ctypes
    from feartracker_amd.train_head import FearBnRunning, _p, load_train_library
    lib = load_train_library()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(12)
    Cs = [16, 96, 24, 672, 256, 112, 4] * 11          # 77 items: more than one launch's table of 64
    vecs = [torch.cat([torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5, torch.zeros(2 * C)]).to(dev) for C in Cs]
    rm = [torch.randn(C, generator=g).to(dev) for C in Cs]
    rv = [(torch.rand(C, generator=g) + 0.5).to(dev) for C in Cs]
    rm2, rv2 = [t.clone() for t in rm], [t.clone() for t in rv]
    counts = [float(100 + 7 * i) for i in range(len(Cs))]
    items = (FearBnRunning * len(Cs))()
    for it, v, a, b, C, n in zip(items, vecs, rm, rv, Cs, counts):
        it.vec, it.running_mean, it.running_var, it.C, it.count = v.data_ptr(), a.data_ptr(), b.data_ptr(), C, n
    assert lib.fear_bn_running_update_multi(items, len(Cs), 0.1, 1e-5, None) == 0
    for v, a, b, C, n in zip(vecs, rm2, rv2, Cs, counts):
        assert lib.fear_bn_running_update(_p(v), n, _p(a), _p(b), 0.1, 1e-5, C, None) == 0
    torch.cuda.synchronize()
    for a, a2, b, b2 in zip(rm, rm2, rv, rv2):
        assert torch.equal(a, a2) and torch.equal(b, b2)
    items[3].count = 0.0
    assert lib.fear_bn_running_update_multi(items, len(Cs), 0.1, 1e-5, None) == -2


@pytest.mark.gpu
def test_deferred_running_statistics_with_an_invalid_late_item_update_nothing():
    """fear_bn_running_update_multi launches one kernel per 64 items: every item is validated before the first launch, so an invalid
    item in the SECOND chunk (item 66 of 70 with C = 0) returns FEAR_TRAIN_ERR_SHAPE with all 70 BatchNorms bit-equal to before —
    and with the item repaired the call equals 70 single fear_bn_running_update calls bit for bit."""
    import ctypes
    from feartracker_amd.train_head import FearBnRunning, _p, load_train_library
    lib = load_train_library()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(13)
    n, C = 70, 8
    vecs = [torch.cat([torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5, torch.zeros(2 * C)]).to(dev) for _ in range(n)]
    rm = [torch.randn(C, generator=g).to(dev) for _ in range(n)]
    rv = [(torch.rand(C, generator=g) + 0.5).to(dev) for _ in range(n)]
    rm0, rv0 = [t.clone() for t in rm], [t.clone() for t in rv]
    counts = [float(50 + 3 * i) for i in range(n)]
    items = (FearBnRunning * n)()
    for it, v, a, b, cnt in zip(items, vecs, rm, rv, counts):
        it.vec, it.running_mean, it.running_var, it.C, it.count = v.data_ptr(), a.data_ptr(), b.data_ptr(), C, cnt
    items[66].C = 0
    assert lib.fear_bn_running_update_multi(items, n, 0.1, 1e-5, None) == -2
    torch.cuda.synchronize()
    changed = [i for i in range(n) if not (torch.equal(rm[i], rm0[i]) and torch.equal(rv[i], rv0[i]))]
    assert not changed, changed
    items[66].C = C
    assert lib.fear_bn_running_update_multi(items, n, 0.1, 1e-5, None) == 0
    for v, a, b, cnt in zip(vecs, rm0, rv0, counts):
        assert lib.fear_bn_running_update(_p(v), cnt, _p(a), _p(b), 0.1, 1e-5, C, None) == 0
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(rm[i], rm0[i]) and torch.equal(rv[i], rv0[i]), i
