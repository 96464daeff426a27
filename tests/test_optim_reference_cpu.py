"""The float64 restatements of tests/optimref.py against torch.optim.Adam / AdamW / SGD and clip_grad_norm_ run in float64
(the yardstick of the GPU optimiser tests must itself be right), and the host logic of `optim.make_optimizer`."""
import numpy as np
import pytest
import torch

import optimref


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("case", sorted(optimref.CASES))
def test_restatement_equals_torch_in_float64(case, clip):
    name, kwargs = optimref.CASES[case]
    p0, grads = optimref.gradient_schedule(1003)
    ref = torch.nn.Parameter(p0.double().clone())
    opt = optimref.make_torch(name, [ref], kwargs)
    mine = optimref.make(name, p0.double().numpy(), kwargs)
    max_norm = 0.5 * float(grads[0].double().norm()) if clip else None
    for step, g in enumerate(grads, 1):
        ref.grad = g.double().clone()
        if clip:
            norm = torch.nn.utils.clip_grad_norm_([ref], max_norm)
            want_norm, want_coef = optimref.clip_coef([g.double().numpy()], max_norm)
            assert abs(float(norm) - want_norm) <= 1e-12 * want_norm
            assert float((ref.grad - g.double() * want_coef).abs().max()) <= 1e-12 * float(g.abs().max())
        opt.step()
        p = mine.step(g.double().numpy(), max_norm)
        scale = max(1.0, float(ref.detach().abs().max()))
        assert float(np.abs(p - ref.detach().numpy()).max()) <= 1e-12 * scale, (case, step)
        torch_state = opt.state[ref]
        for key, value in mine.state().items():
            t = torch_state[key].numpy()
            assert float(np.abs(value - t).max()) <= 1e-12 * max(1.0, float(np.abs(t).max())), (case, step, key)
    if name == "sgd" and kwargs.get("momentum", 0) == 0:
        assert mine.state() == {} and opt.state[ref].get("momentum_buffer") is None


def test_clip_coef_over_several_tensors():
    g = torch.Generator().manual_seed(1)
    tensors = [torch.randn(s, generator=g, dtype=torch.float64) for s in ((3, 5), (7,), (2, 2, 2))]
    params = [torch.nn.Parameter(torch.zeros_like(t)) for t in tensors]
    for max_norm in (0.3, 100.0):
        for p, t in zip(params, tensors):
            p.grad = t.clone()
        norm, coef = optimref.clip_coef([t.numpy() for t in tensors], max_norm)
        got = torch.nn.utils.clip_grad_norm_(params, max_norm)
        assert abs(float(got) - norm) <= 1e-12 * norm
        assert coef == min(1.0, max_norm / (norm + 1e-6)) and (coef == 1.0) == (max_norm > norm)


def test_make_optimizer_maps_the_reference_configurations():
    from feartracker_amd.optim import AdamHIP, AdamWHIP, SGDHIP, optimizer_arguments
    assert optimizer_arguments({"name": "adam", "lr": 1e-4}) == (AdamHIP, {"lr": 1e-4})
    assert optimizer_arguments({"name": "adamw", "lr": 3e-3, "eps": 1e-6, "weight_decay": 2e-6}) == \
        (AdamWHIP, {"lr": 3e-3, "eps": 1e-6, "weight_decay": 2e-6})
    cfg = {"name": "sgd", "lr": 1e-2, "momentum": 0.9, "nesterov": True, "weight_decay": 1e-6}
    assert optimizer_arguments(cfg) == (SGDHIP, {k: v for k, v in cfg.items() if k != "name"})
    assert cfg["name"] == "sgd"                                     # the caller's mapping is left alone
    # every key is an argument of the class it is handed to
    import inspect
    for name, kwargs in optimref.CASES.values():
        cls, kw = optimizer_arguments(dict(kwargs, name=name))
        assert set(kw) <= set(inspect.signature(cls.__init__).parameters)


@pytest.mark.parametrize("cfg, word", [
    ({"name": "lamb", "lr": 1e-3}, "lamb"),
    ({"name": "adam", "lr": 1e-3, "momentum": 0.9}, "momentum"),
    ({"name": "sgd", "lr": 1e-2, "betas": (0.9, 0.99)}, "betas"),
    ({"name": "adamw", "lr": 1e-3, "amsgrad": True}, "amsgrad"),
    ({"lr": 1e-3}, "name"),
    ({"name": "sgd", "momentum": 0.9}, "lr"),
])
def test_make_optimizer_rejects_unknown_names_and_keys(cfg, word):
    from feartracker_amd.optim import make_optimizer
    with pytest.raises(ValueError, match=word):
        make_optimizer(None, cfg)                                   # rejected before the network is touched
