"""The optimiser family of include/fear_train.h (fear_grad_sumsq, fear_grad_norm_finalize, fear_optim_step) and its Python side
(optim.AdamHIP / AdamWHIP / SGDHIP with `max_grad_norm`, state_dict, schedule.save_training_checkpoint): bit identities, the norm
operator against float64, the three rules against torch.optim in fp32, the whole network against clip_grad_norm_ + torch.optim,
and resuming a run."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import optimref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
KIND = {"adam": 0, "adamw": 1, "sgd": 2}


def test_optimiser_struct_mirror_has_the_headers_layout(tmp_path):
    """The ctypes mirror of FearOptim has the size and field offsets the C compiler gives the header's definition, the constants
    agree, and the argument errors that need no device come back as documented."""
    from feartracker_amd import train_abi as ta
    fields = [f for f, _ in ta.FearOptim._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/fear_train.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(FearOptim));']
    lines += [f'  printf("{f} %zu\\n", offsetof(FearOptim, {f}));' for f in fields]
    lines += ['  printf("consts %d %d %d %d\\n", FEAR_OPT_ADAM, FEAR_OPT_ADAMW, FEAR_OPT_SGD, FEAR_GRAD_SUMSQ_CHUNK);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = dict(line.split(None, 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n"))
    assert int(out.pop("size")) == ctypes.sizeof(ta.FearOptim)
    assert [int(v) for v in out.pop("consts").split()] == [ta.FEAR_OPT_ADAM, ta.FEAR_OPT_ADAMW, ta.FEAR_OPT_SGD, ta.FEAR_GRAD_SUMSQ_CHUNK]
    assert sorted(out) == sorted(fields)
    for f in fields:
        assert int(out[f]) == getattr(ta.FearOptim, f).offset, f
    lib = ta.load_train_library()
    chunk = ta.FEAR_GRAD_SUMSQ_CHUNK
    assert [lib.fear_grad_sumsq_partials(n) for n in (-1, 0, 1, chunk, chunk + 1, 2 * chunk + 5)] == [0, 0, 1, 1, 2, 3]
    fake = ctypes.c_void_p(4096)
    assert lib.fear_grad_sumsq(None, 8, fake, None) == -1 and lib.fear_grad_sumsq(fake, -1, fake, None) == -2
    assert lib.fear_grad_sumsq(ctypes.c_void_p(4098), 8, fake, None) == -2                  # not a float's address
    assert lib.fear_grad_norm_finalize(None, 3, 1.0, fake, None) == -1 and lib.fear_grad_norm_finalize(fake, 3, 1.0, None, None) == -1
    assert lib.fear_optim_step(None, fake, fake, fake, fake, 8, 1, None, None) == -1


def _desc(name, kwargs):
    from feartracker_amd.train_abi import FearOptim
    kw = dict(kwargs)
    betas = kw.pop("betas", (0.9, 0.999))
    torch_defaults = {"adam": dict(lr=1e-3, eps=1e-8, weight_decay=0.0), "adamw": dict(lr=1e-3, eps=1e-8, weight_decay=1e-2),
                      "sgd": dict(momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False)}[name]
    kw = dict(torch_defaults, **kw)
    kw["nesterov"] = int(kw.get("nesterov", False))
    if name != "sgd":
        kw.update(beta1=betas[0], beta2=betas[1])
    return FearOptim(kind=KIND[name], **kw)


class _Op:
    """The C ABI on flat device tensors."""

    def __init__(self):
        from feartracker_amd.train_abi import _p, load_train_library
        self.lib, self.p = load_train_library(), _p
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def norm(self, grad, max_norm, partials=None, out2=None):
        count = self.lib.fear_grad_sumsq_partials(grad.numel())
        partials = torch.full((count + 1,), -7.0, dtype=torch.float64, device="cuda") if partials is None else partials
        out2 = torch.full((3,), -7.0, device="cuda") if out2 is None else out2
        assert self.lib.fear_grad_sumsq(self.p(grad), grad.numel(), self.p(partials), self.st) == 0
        assert self.lib.fear_grad_norm_finalize(self.p(partials), count, max_norm, self.p(out2), self.st) == 0
        return partials, out2

    def step(self, desc, p, g, s1, s2, step, coef=None):
        n = (p if p is not None else g).numel()
        return self.lib.fear_optim_step(ctypes.byref(desc), self.p(p), self.p(g), self.p(s1), self.p(s2), n, step,
                                        None if coef is None else self.p(coef, 1), self.st)


# ---------------------------------------------------------------------------------------------------------- 1. bit identities
@gpu
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_kind_without_clipping_gives_fear_adam_steps_bits(wd):
    op = _Op()
    p0, grads = optimref.gradient_schedule(10007)
    desc = _desc("adam", dict(lr=1e-3, weight_decay=wd))
    a = [p0.clone().cuda(), torch.zeros(10007, device="cuda"), torch.zeros(10007, device="cuda")]
    b = [t.clone() for t in a]
    for step, g in enumerate(grads, 1):
        gd = g.cuda()
        assert op.lib.fear_adam_step(op.p(a[0]), op.p(gd), op.p(a[1]), op.p(a[2]), 10007, 1e-3, 0.9, 0.999, 1e-8, wd, step, op.st) == 0
        assert op.step(desc, b[0], gd, b[1], b[2], step) == 0
        torch.cuda.synchronize()
        for x, y, what in zip(a, b, ("param", "exp_avg", "exp_avg_sq")):
            assert torch.equal(x, y), (step, what, int((x != y).sum()))
        assert torch.equal(gd.cpu(), g)                              # the gradient is read only


@gpu
@pytest.mark.parametrize("case", ["adam_yaml", "adamw_yaml", "sgd_yaml", "adam_l2"])
def test_a_coefficient_of_one_changes_nothing_and_runs_repeat_bit_for_bit(case):
    op = _Op()
    name, kwargs = optimref.CASES[case]
    desc = _desc(name, kwargs)
    p0, grads = optimref.gradient_schedule(10007)
    runs = []
    for clipped in (False, True, True):
        p, s1, s2 = p0.clone().cuda(), torch.zeros(10007, device="cuda"), torch.zeros(10007, device="cuda")
        seen = []
        for step, g in enumerate(grads, 1):
            gd = g.cuda()
            coef = None
            if clipped:
                partials, coef = op.norm(gd, 10.0 * float(g.double().norm()))
                seen += [partials.clone(), coef.clone()]
            assert op.step(desc, p, gd, s1, s2, step, coef) == 0
        torch.cuda.synchronize()
        if clipped:
            assert all(float(c[1]) == 1.0 for c in seen[1::2])
        runs.append(([p, s1, s2], seen))
    for x, y, z in zip(*(r[0] for r in runs)):
        assert torch.equal(x, y) and torch.equal(y, z)
    for x, y in zip(runs[1][1], runs[2][1]):                         # the same inputs twice: partial sums, norm, coefficient
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------ 2. norm operator
@gpu
@pytest.mark.parametrize("offset", [0, 1])
def test_norm_operator_matches_float64(offset):
    """norm = (float) sqrt(float64 sum): the float64 sum of up to 10^4 exact squares is good to ~1e-15, so the only rounding that
    shows is the one to fp32 (2^-24 relative); 2^-23 leaves room for a last-place difference of the float64 square root.  The
    coefficient is the fp32 expression of clip_grad_norm_ on that fp32 norm, exactly."""
    from feartracker_amd.train_abi import FEAR_GRAD_SUMSQ_CHUNK as chunk
    op = _Op()
    gen = torch.Generator().manual_seed(3)
    for n in (1, 3, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 5, 10007):
        for k in range(1, 6):
            g = torch.randn(n, generator=gen) * (10.0 ** (k - 3))
            buf = torch.full((n + offset + 4,), 1e30, device="cuda")          # anything read outside [offset, offset + n) would show
            gd = buf[offset: offset + n]
            gd.copy_(g)
            assert gd.data_ptr() % 16 == 4 * offset
            exact = math.sqrt(float((g.double() ** 2).sum()))
            for max_norm in (0.5 * exact, 2.0 * exact, 0.0):
                partials, out2 = op.norm(gd, max_norm)
                torch.cuda.synchronize()
                count = op.lib.fear_grad_sumsq_partials(n)
                assert count == (n + chunk - 1) // chunk
                assert float(partials[count]) == -7.0 and float(out2[2]) == -7.0        # nothing written past the documented outputs
                norm = out2[0].cpu()
                assert abs(float(norm) - exact) <= 2.0 ** -23 * exact, (n, k, float(norm), exact)
                want = torch.clamp(max_norm / (norm + 1e-6), max=1.0) if max_norm > 0 else torch.tensor(1.0)
                assert float(out2[1]) == float(want), (n, k, max_norm, float(out2[1]), float(want))
                assert max_norm != 0.5 * exact or float(out2[1]) < 1.0                   # (half the norm does clip)


@gpu
def test_finalize_adds_the_partials_of_several_calls():
    """The per-tensor path: consecutive ranges of `partials` written by one call per tensor, one finalize over all of them."""
    op = _Op()
    gen = torch.Generator().manual_seed(4)
    pieces = [torch.randn(n, generator=gen) for n in (5, 4097, 300, 9000)]
    counts = [op.lib.fear_grad_sumsq_partials(t.numel()) for t in pieces]
    partials = torch.zeros(sum(counts), dtype=torch.float64, device="cuda")
    off = 0
    for t, c in zip(pieces, counts):
        assert op.lib.fear_grad_sumsq(op.p(t.cuda()), t.numel(), ctypes.c_void_p(partials.data_ptr() + 8 * off), op.st) == 0
        off += c
    out2 = torch.zeros(2, device="cuda")
    assert op.lib.fear_grad_norm_finalize(op.p(partials), sum(counts), 1.0, op.p(out2), op.st) == 0
    exact = math.sqrt(sum(float((t.double() ** 2).sum()) for t in pieces))
    assert abs(float(out2[0]) - exact) <= 2.0 ** -23 * exact


# -------------------------------------------------------------------------------------------- 3. the rules against torch.optim
# What does not fit the project's 2e-7 * max|x| (tests/test_train_optim.py:40) is held to 2 E + 1 ulp of max|x| instead, E being
# torch-fp32's own distance from the float64 result of tests/optimref.py for that tensor (two fp32 evaluations of one formula may
# each be E away from the exact value).  These are the state tensors of the clipped cases: torch adds its squares up in fp32, so
# its coefficient — and with it every clipped gradient — is already a few 1e-7 (relative) away from the exact one, while the
# operator's float64 norm is not; the parameters move too little per step to show it.
# {(case, what): E as measured over the five steps, with max|x|} — the test recomputes E at every step and uses that value.
E_RULE = {
    ("adam_yaml", "exp_avg"): "E 3.2e-10 .. 6.4e-10 at max 1.7e-3 .. 4.1e-3",
    ("adam_yaml", "exp_avg_sq"): "E 1.1e-13 .. 1.8e-13 at max 2.8e-7 .. 6.1e-7",
    ("adamw_yaml", "exp_avg"): "E 3.2e-10 .. 6.4e-10 at max 1.7e-3 .. 4.1e-3",
    ("adamw_yaml", "exp_avg_sq"): "E 1.1e-13 .. 1.8e-13 at max 2.8e-7 .. 6.1e-7",
    ("sgd_yaml", "momentum_buffer"): "E 2.6e-9 .. 6.7e-9 at max 1.7e-2 .. 4.1e-2",
}


def _ulp(x):
    return float(np.spacing(np.float32(x)))


@gpu
@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("case", ["adam_yaml", "adamw_yaml", "sgd_yaml", "sgd_plain"])
def test_update_rules_match_torch_optim(case, clipped):
    op = _Op()
    name, kwargs = optimref.CASES[case]
    desc = _desc(name, kwargs)
    n = 10007
    p0, grads = optimref.gradient_schedule(n)
    max_norm = 0.5 * float(grads[0].norm()) if clipped else None
    ref = torch.nn.Parameter(p0.clone())
    opt = optimref.make_torch(name, [ref], kwargs)
    exact = optimref.make(name, p0.double().numpy(), kwargs)
    p, s1, s2 = p0.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    has_buf = name != "sgd" or kwargs.get("momentum", 0) != 0
    states = {"adam": ("exp_avg", "exp_avg_sq"), "adamw": ("exp_avg", "exp_avg_sq"), "sgd": ("momentum_buffer",) if has_buf else ()}[name]
    for step, g in enumerate(grads, 1):
        ref.grad = g.clone()
        if clipped:
            torch.nn.utils.clip_grad_norm_([ref], max_norm)
        opt.step()
        exact.step(g.double().numpy(), max_norm)
        gd = g.cuda()
        coef = None
        if clipped:
            _, coef = op.norm(gd, max_norm)
        assert op.step(desc, p, gd, s1 if has_buf else None, s2 if name != "sgd" else None, step, coef) == 0
        torch.cuda.synchronize()
        assert torch.equal(gd.cpu(), g)                              # clipping does not write the gradient back
        if clipped:
            assert abs(float(coef[0]) - float(g.double().norm())) <= 2.0 ** -23 * float(g.double().norm())
            assert (step == 1) == (abs(float(coef[1]) - 0.5) < 1e-5) and float(coef[1]) <= 1.0
        pairs = [("param", p.cpu(), ref.detach(), exact.p)]
        pairs += [(s, t.cpu(), opt.state[ref][s], exact.state()[s]) for s, t in zip(states, (s1, s2))]
        for what, mine, theirs, exact64 in pairs:
            top = float(theirs.abs().max())
            err = float((mine - theirs).abs().max())
            E = float(np.abs(theirs.double().numpy() - exact64).max())
            print(f"{case} clipped={clipped} step {step} {what}: err {err:.3e}  2e-7*max {2e-7 * top:.3e}  E {E:.3e}  ulp(max) {_ulp(top):.3e}")
            bound = 2.0 * E + _ulp(top) if clipped and (case, what) in E_RULE else 2e-7 * top
            assert err <= bound, (step, what, err, bound)


# --------------------------------------------------------------------------------------------------------- 4. the whole network
def _batch(B=2, seed=9):            # (the batch of tests/test_train_optim.py)
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 3, 128, 128, generator=g), torch.randn(B, 3, 256, 256, generator=g),
            torch.rand(B, 4, 16, 16, generator=g) * 60 + 1, (torch.rand(B, 1, 16, 16, generator=g) > 0.8).float(),
            (torch.rand(B, 16, 16, generator=g) > 0.85).float())


NET_CASES = {"adam": dict(lr=1e-3), "adamw": optimref.CASES["adamw_yaml"][1], "sgd": optimref.CASES["sgd_yaml"][1]}


def _compare_network(net, ora, it):
    mine = net.state_dict()
    for n, p in ora.named_parameters():
        d = float((mine[n] - p.detach()).abs().max())
        assert mine[n].shape == p.shape and d <= 1e-6 * max(1.0, float(p.detach().abs().max())), (it, n, d)


@gpu
@pytest.mark.parametrize("source", ["autograd", "step"])
@pytest.mark.parametrize("name", ["adam", "adamw", "sgd"])
def test_clipped_optimisers_on_the_network_match_clip_grad_norm_and_torch_optim(name, source):
    """Every one of the 195 tensors after two clipped steps, and the norm the optimiser reports.  "autograd": the checker's
    gradients as a plain dict (laid out into the staging buffer); "step": the network's own `GradDict`, whose flat buffer the
    optimiser reads as it stands — there the norm is also held against the float64 norm over the dict's values, which no
    padding element of the kernel layout may enter."""
    from feartracker_amd.optim import make_optimizer
    from feartracker_amd.train_net import FEARNetTrainHIP
    from oracle.fear_train_oracle import FEARNetTrainOracle, fear_loss, random_init_state
    sd = random_init_state(5)
    ora = FEARNetTrainOracle().train()
    ora.load_state_dict(sd, strict=False)
    net = FEARNetTrainHIP(sd, device=0)
    ref_opt = optimref.make_torch(name, ora.parameters(), NET_CASES[name])
    hip_opt = make_optimizer(net, dict(NET_CASES[name], name=name), gradient_clip_val=1.0)
    tmpl, srch, gt_reg, gt_cls, gt_w = _batch()
    max_norm = None
    for it in range(2):
        ref_opt.zero_grad()
        if source == "autograd":
            bbox, cls = ora(tmpl, srch)
            lc, lr = fear_loss(bbox, cls, gt_reg, gt_cls, gt_w)
            (lc + lr).backward()
            grads = {n: p.grad.detach().clone() for n, p in ora.named_parameters()}
        else:
            grads = net.step(tmpl, srch, gt_reg, gt_cls, gt_w)["grads"]
            assert grads.current_flat() is not None and grads.current_flat().numel() == net.param_flat.numel()
            for n, p in ora.named_parameters():
                p.grad = grads[n].detach().cpu().reshape(p.shape).clone()
        exact = math.sqrt(sum(float((grads[n].double() ** 2).sum()) for n, _ in ora.named_parameters()))
        if max_norm is None:
            max_norm = hip_opt.max_grad_norm = 0.5 * exact          # half the first step's norm: the first step is clipped for certain
        norm = torch.nn.utils.clip_grad_norm_(ora.parameters(), max_norm)
        ref_opt.step()
        hip_opt.step(grads)
        torch.cuda.synchronize()
        got = hip_opt.last_grad_norm
        assert got.dim() == 0 and got.is_cuda
        print(f"{name} {source} step {it}: norm {float(got):.9g} torch {float(norm):.9g} float64 over the dict {exact:.9g}")
        assert abs(float(got) - float(norm)) <= 1e-6 * float(norm)
        assert abs(float(got) - exact) <= 1e-6 * exact
        _compare_network(net, ora, it)
    assert hip_opt.steps == 2


@gpu
def test_clipped_sgd_on_the_head_alone_updates_tensor_by_tensor(golden_dir):
    """`BoxTowerTrainHIP` has no flat buffer: one sum of squares per tensor into consecutive partials, one finalize, one update
    per tensor.  The torch side (clip_grad_norm_ + torch.optim.SGD, fp32) runs on the device, where the gradients are: a reference
    has to sit well inside the 1e-6 it is used for, and torch's fp32 norm on the CPU does not on these tensors — on the fixture's
    own gradients it returns 0.07824480534 where float64 gives 0.07824489689 (-1.17e-6 relative; -2.8e-6 on the 256 x 320
    pointwise weight alone), so it would turn away the correctly rounded 0.07824489474.  torch's distance from the float64 norm
    is printed at every step."""
    from feartracker_amd.optim import SGDHIP
    from feartracker_amd.train_head import BoxTowerTrainHIP
    d = np.load(f"{golden_dir}/head_train_step.npz")
    sd = {k[len("param."):]: d[k] for k in d.files if k.startswith("param.")}
    net = BoxTowerTrainHIP(sd, device=0)
    assert getattr(net, "param_flat", None) is None
    slots = net.parameter_slots()
    params = {k: torch.nn.Parameter(to_torch(t).detach().clone().contiguous()) for k, (t, _, to_torch) in slots.items()}
    kwargs = optimref.CASES["sgd_yaml"][1]
    ref_opt = torch.optim.SGD(list(params.values()), **kwargs)
    hip_opt = SGDHIP(net, max_grad_norm=1.0, **kwargs)
    inputs = [torch.from_numpy(d[k]) for k in ("in_search", "in_template", "gt_reg", "gt_cls", "gt_weight")]
    max_norm = None
    for it in range(2):
        grads = net.step(*inputs)["grads"]
        for k, p in params.items():
            p.grad = grads[k].detach().reshape(p.shape).clone()
        exact = math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in params.values()))
        if max_norm is None:
            max_norm = hip_opt.max_grad_norm = 0.5 * exact
        norm = torch.nn.utils.clip_grad_norm_(list(params.values()), max_norm)
        ref_opt.step()
        hip_opt.step(grads)
        torch.cuda.synchronize()
        got = float(hip_opt.last_grad_norm)
        print(f"head step {it}: norm {got:.10g}  torch {float(norm):.10g} ({(float(norm) - exact) / exact:+.2e} from float64)  float64 {exact:.10g}")
        assert abs(got - float(norm)) <= 1e-6 * float(norm)
        assert abs(got - exact) <= 1e-6 * exact
        for k, (t, _, to_torch) in net.parameter_slots().items():
            dist = float((to_torch(t) - params[k].detach()).abs().max())
            assert dist <= 1e-6 * max(1.0, float(params[k].detach().abs().max())), (it, k, dist)


# -------------------------------------------------------------------------------------------------------------------- 5. resume
@gpu
def test_a_run_resumed_from_a_checkpoint_continues_bit_for_bit(tmp_path):
    from feartracker_amd.optim import AdamHIP
    from feartracker_amd.schedule import load_training_checkpoint, save_training_checkpoint
    from feartracker_amd.train_net import FEARNetTrainHIP
    from oracle.fear_train_oracle import random_init_state
    batch = _batch()

    def run(net, opt, steps):
        for _ in range(steps):
            opt.step(net.step(*batch)["grads"])
        torch.cuda.synchronize()

    def fresh(seed):
        net = FEARNetTrainHIP(random_init_state(seed), device=0)
        return net, AdamHIP(net, lr=1e-3, weight_decay=1e-4, max_grad_norm=0.5)

    net_a, opt_a = fresh(5)
    opt_a.lr = 5e-4                                                  # (as a schedule leaves it)
    run(net_a, opt_a, 4)
    net_b, opt_b = fresh(5)
    opt_b.lr = 5e-4
    run(net_b, opt_b, 2)
    path = os.path.join(tmp_path, "run.pt")
    save_training_checkpoint(path, net_b, opt_b, epoch=3)
    sd = opt_b.state_dict()
    model = net_b.state_dict()
    for key in ("trunk.1.dw.conv.weight", "stem.conv.weight", "trunk.1.pwl.conv.weight"):
        entry = sd["state"][key]
        assert entry["step"] == 2 and not entry["exp_avg"].is_cuda
        assert entry["exp_avg"].shape == model[key].shape == entry["exp_avg_sq"].shape, key
    assert model["trunk.1.dw.conv.weight"].shape[1:] == (1, 3, 3) and model["stem.conv.weight"].shape == (16, 3, 3, 3)
    assert sd["param_groups"][0]["lr"] == 5e-4 and sd["param_groups"][0]["params"] == list(sd["state"])
    del net_b, opt_b
    net_c, opt_c = fresh(6)                                          # other parameters, default learning rate
    flat_address, moment_address = net_c.param_flat.data_ptr(), opt_c.exp_avg_flat.data_ptr()
    assert load_training_checkpoint(path, net_c, opt_c) == {"epoch": 3}
    assert (net_c.param_flat.data_ptr(), opt_c.exp_avg_flat.data_ptr()) == (flat_address, moment_address)
    assert opt_c.steps == 2 and opt_c.lr == 5e-4
    run(net_c, opt_c, 2)
    want, got = net_a.state_dict(), net_c.state_dict()              # parameters and running statistics
    assert sorted(want) == sorted(got)
    for k in want:
        assert torch.equal(want[k], got[k]), k
    want, got = opt_a.state_dict(), opt_c.state_dict()
    assert want["param_groups"] == got["param_groups"]
    for k, entry in want["state"].items():
        assert entry["step"] == got["state"][k]["step"] == 4
        assert torch.equal(entry["exp_avg"], got["state"][k]["exp_avg"]) and torch.equal(entry["exp_avg_sq"], got["state"][k]["exp_avg_sq"]), k


# ----------------------------------------------------------------------------------------------------------- 6. argument checks
@gpu
def test_argument_errors_leave_the_parameters_untouched():
    op = _Op()
    p0 = torch.randn(1001, generator=torch.Generator().manual_seed(1))
    p, g, s1, s2 = p0.clone().cuda(), torch.ones(1001, device="cuda"), torch.zeros(1001, device="cuda"), torch.zeros(1001, device="cuda")
    adam, sgd = _desc("adam", {}), _desc("sgd", dict(lr=0.1, momentum=0.9))
    assert op.step(adam, p, g, s1, s2, 0) == -2                                             # steps count from 1
    bad = _desc("adam", {})
    bad.kind = 3
    assert op.step(bad, p, g, s1, s2, 1) == -2
    assert op.step(_desc("adam", dict(betas=(1.0, 0.999))), p, g, s1, s2, 1) == -2
    assert op.step(_desc("adamw", dict(betas=(0.9, -0.1))), p, g, s1, s2, 1) == -2
    assert op.step(_desc("sgd", dict(lr=0.1, nesterov=True)), p, g, s1, None, 1) == -2          # nesterov without momentum
    assert op.step(_desc("sgd", dict(lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)), p, g, s1, None, 1) == -2
    assert op.step(_desc("sgd", dict(lr=0.1, momentum=-0.5)), p, g, s1, None, 1) == -2
    assert op.step(adam, p, g, s1, None, 1) == -1 and op.step(adam, p, g, None, s2, 1) == -1
    assert op.step(sgd, p, g, None, None, 1) == -1                                          # momentum needs its buffer
    assert op.step(adam, None, g, s1, s2, 1) == -1 and op.step(adam, p, None, s1, s2, 1) == -1
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), p0) and float(s1.abs().max()) == 0 and float(s2.abs().max()) == 0
    assert op.step(_desc("sgd", dict(lr=0.1)), p, g, None, None, 1) == 0                    # no momentum: no state at all
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), p0 - torch.tensor(0.1) * 1.0)
