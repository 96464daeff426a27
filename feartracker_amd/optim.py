"""`torch.optim.Adam`, `AdamW` and `SGD` for the HIP training step, with gradient-norm clipping: the reference's optimiser is
Adam(lr = 1e-4) on every parameter (model_training/train/base_lightning_model.py:63-64), its configuration also offers
config/optimizer/{adamw,sgd}.yaml and `gradient_clip_val` (train/trainer.py:59: Lightning's `clip_grad_norm_` over all parameters).

    net = FEARNetTrainHIP(state)
    opt = AdamHIP(net)                       # lr 1e-4, betas (0.9, 0.999), eps 1e-8, no weight decay: torch's defaults
    opt = make_optimizer(net, {"name": "sgd", "lr": 1e-2, "momentum": 0.9, "nesterov": True}, gradient_clip_val=1.0)
    out = net.step(template, search, gt_reg, gt_cls, gt_weight)
    opt.step(net.allreduce_gradients(out["grads"]))      # (the all-reduce only with several ranks)

The update runs on the device, on the tensors the kernels read (kernel layouts, so no re-layout of the weights between steps);
first / second moments (the momentum buffer) are kept in the same layout.  `FEARNetTrainHIP` keeps all 195 parameter tensors
(1.37 M floats) in ONE flat buffer (`param_flat`) and hands its gradients out as views of one buffer of the same layout
(`GradDict.flat`): the whole update is ONE launch over (parameters, gradients, state) — `fear_adam_step` for `AdamHIP` without
clipping, `fear_optim_step` otherwise.  Gradients that arrive as a plain dict in the reference's layouts (the checker's autograd
in the tests) are first laid out into a staging buffer of that layout; a model without `param_flat` (the head alone,
`BoxTowerTrainHIP`) is updated tensor by tensor.  The learning-rate schedule of the reference (ReduceLROnPlateau) only changes `lr`.

Clipping (`max_grad_norm`) adds two launches in front of the update and no host synchronisation: the 2-norm of the gradient buffer
in a fixed order (`fear_grad_sumsq`, `fear_grad_norm_finalize`) and, inside the update, g = grad * coef.  The gradient buffer itself
is NOT scaled (torch scales it in place): `grads` read after `step` are the unclipped ones.  Padding of the kernel layout (gaps
between 16-byte slots, column 27 of the stem's rows, padded pointwise rows) holds zeros in every gradient buffer the step or the
staging produces, so the norm is that of the gradients in the reference's layouts.

`state_dict()` / `load_state_dict()` have torch.optim's shape with parameter NAMES as keys and CPU tensors in the reference's
layouts; with `schedule.save_training_checkpoint` a run is resumable.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, List, Mapping, Optional, Tuple

import torch

from .train_abi import FEAR_OPT_ADAM, FEAR_OPT_ADAMW, FEAR_OPT_SGD, FearOptim, TrainError, _p, launch, load_train_library


class _OptimHIP:
    """What the three optimisers share: slot discovery, the flat / staging / per-tensor paths, the `steps` counter, the plain `lr`
    attribute that `PlateauSchedule` writes, clipping and the checkpoint form.  A subclass names its rule (`kind`), its state
    tensors as torch.optim names them (`state_names`) and its hyper-parameters (`_hyper`, `_descriptor`)."""
    kind = -1
    state_names: Tuple[str, ...] = ()

    def __init__(self, net, lr: float, weight_decay: float, max_grad_norm: Optional[float]):
        self.lib = load_train_library()
        self.net = net
        self.lr, self.weight_decay = float(lr), float(weight_decay)
        self.max_grad_norm = None if not max_grad_norm else float(max_grad_norm)      # None or 0 (Lightning's "off"): no clipping
        if self.max_grad_norm is not None and not self.max_grad_norm > 0:
            raise ValueError("max_grad_norm must be positive (None or 0 turns clipping off)")
        self.slots = net.parameter_slots()
        self.flat = getattr(net, "param_flat", None)
        n_state = len(self.state_names)
        if self.flat is not None:
            base = self.flat.data_ptr()
            self._off = {}
            for k, (t, _, _) in self.slots.items():
                off = (t.data_ptr() - base) // 4
                if not (0 <= off and off + t.numel() <= self.flat.numel() and t.is_contiguous()):
                    raise ValueError(f"{k}: parameter storage is not a slot of the network's flat buffer")
                self._off[k] = off
            self._state_flat = [torch.zeros_like(self.flat) for _ in range(n_state)]
            view = lambda buf, k, t: buf[self._off[k]: self._off[k] + t.numel()].view(t.shape)
            self._state = [{k: view(buf, k, t) for k, (t, _, _) in self.slots.items()} for buf in self._state_flat]
            self._stage = None
        else:
            self._state_flat = [None] * n_state
            self._state = [{k: torch.zeros_like(t) for k, (t, _, _) in self.slots.items()} for _ in range(n_state)]
        self.steps = 0
        self.last_grad_norm: Optional[torch.Tensor] = None
        self._norm2 = None            # device [norm, coef] (fp32) and the float64 partial sums in front of them
        self._partials = None

    # ------------------------------------------------------------------ the rule
    def _hyper(self) -> Dict[str, Any]:
        raise NotImplementedError

    def _descriptor(self) -> FearOptim:
        raise NotImplementedError

    def _update(self, param, grad, states, n, st, coef, what) -> None:
        s = [_p(t) for t in states] + [None, None]
        o = self._descriptor()
        rc = self.lib.fear_optim_step(ctypes.byref(o), _p(param), _p(grad), s[0], s[1], n, self.steps, coef, st)
        if rc != 0:
            raise TrainError(f"fear_optim_step failed with status {rc} on {what}")

    # ------------------------------------------------------------------ clipping
    def _norm(self, pieces: List[torch.Tensor], st):
        """The 2-norm of the concatenation of `pieces` and the clipping coefficient, on the device; returns the coefficient's
        device address."""
        counts = [int(self.lib.fear_grad_sumsq_partials(g.numel())) for g in pieces]
        total = sum(counts)
        dev = pieces[0].device
        if self._partials is None or self._partials.numel() < total:
            self._partials = torch.empty(max(total, 1), dtype=torch.float64, device=dev)
            self._norm2 = torch.zeros(2, dtype=torch.float32, device=dev)
        off = 0
        for g, c in zip(pieces, counts):
            launch(self.lib, "fear_grad_sumsq", _p(g), g.numel(), ctypes.c_void_p(self._partials.data_ptr() + 8 * off), st)
            off += c
        launch(self.lib, "fear_grad_norm_finalize", _p(self._partials), total, self.max_grad_norm, _p(self._norm2), st)
        self.last_grad_norm = self._norm2[0]
        return _p(self._norm2, 1)

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, grads: Dict[str, torch.Tensor]) -> None:
        """One update from gradients in the reference's layouts ({parameter name: tensor}, as `net.step` returns them).
        Every parameter must have a gradient (the reference's graph leaves none unused).  With `max_grad_norm`,
        `last_grad_norm` is afterwards the norm before clipping, a 0-dim device tensor that the next step overwrites."""
        missing = [k for k in self.slots if k not in grads]
        if missing:
            raise KeyError(f"no gradient for {missing[:3]}{'...' if len(missing) > 3 else ''}")
        self.steps += 1
        dev = self.net.device
        with torch.cuda.device(dev):
            st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            if self.flat is not None:
                # (GradDict.current_flat: None once an entry was rebound or a re-laid-out copy edited — the dict's values then count)
                gflat = grads.current_flat() if hasattr(grads, "current_flat") else getattr(grads, "flat", None)
                if gflat is None or gflat.numel() != self.flat.numel() or gflat.device != self.flat.device:
                    # gradients from somewhere else: lay them out like the parameters (padding between slots stays zero)
                    if self._stage is None:
                        self._stage = torch.zeros_like(self.flat)
                    gflat = self._stage
                    for name, (param, to_storage, _) in self.slots.items():
                        g = to_storage(grads[name].to(dev, torch.float32))
                        if g.shape != param.shape:
                            raise ValueError(f"{name}: gradient {tuple(grads[name].shape)} does not fit parameter storage {tuple(param.shape)}")
                        gflat[self._off[name]: self._off[name] + g.numel()].view(g.shape).copy_(g)
                coef = self._norm([gflat], st) if self.max_grad_norm is not None else None
                self._update(self.flat, gflat, self._state_flat, self.flat.numel(), st, coef, "the flat parameter buffer")
                return
            laid = {}
            for name, (param, to_storage, _) in self.slots.items():
                g = to_storage(grads[name].to(dev, torch.float32))
                if g.shape != param.shape:
                    raise ValueError(f"{name}: gradient {tuple(grads[name].shape)} does not fit parameter storage {tuple(param.shape)}")
                laid[name] = g
            coef = self._norm(list(laid.values()), st) if self.max_grad_norm is not None else None
            for name, (param, _, _) in self.slots.items():
                self._update(param, laid[name], [s[name] for s in self._state], param.numel(), st, coef, name)

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self) -> Dict[str, Any]:
        """torch.optim's form, keyed by parameter name: {"state": {name: {"step": int, <state name>: CPU tensor in the reference's
        layout}}, "param_groups": [{hyper-parameters, lr as the schedule left it, "params": names}]}."""
        state = {}
        for name, (_, _, to_torch) in self.slots.items():
            entry: Dict[str, Any] = {"step": int(self.steps)}
            for sname, views in zip(self.state_names, self._state):
                entry[sname] = to_torch(views[name]).contiguous().cpu()
            state[name] = entry
        return {"state": state, "param_groups": [dict(self._hyper(), params=list(self.slots))]}

    @torch.no_grad()
    def load_state_dict(self, sd: Mapping[str, Any]) -> None:
        """The inverse of `state_dict`: hyper-parameters from the group, the step count, and the state tensors laid out into the
        optimiser's own buffers (whose addresses do not change)."""
        groups = sd["param_groups"]
        if len(groups) != 1:
            raise ValueError("one parameter group expected")
        group = dict(groups[0])
        names = group.pop("params", list(self.slots))
        if set(names) != set(self.slots) or set(sd["state"]) != set(self.slots):
            raise ValueError("the optimiser state names other parameters than the network has")
        unknown = sorted(set(group) - set(self._hyper()))
        if unknown:
            raise ValueError(f"unknown hyper-parameter {unknown[0]!r} for {type(self).__name__}")
        steps = {int(e["step"]) for e in sd["state"].values()}
        if len(steps) != 1:
            raise ValueError("every parameter must be at the same step")
        laid = []
        for name, (param, to_storage, _) in self.slots.items():
            for sname, views in zip(self.state_names, self._state):
                t = to_storage(torch.as_tensor(sd["state"][name][sname]).to(param.device, torch.float32))
                if t.shape != param.shape:
                    raise ValueError(f"{name}: {sname} {tuple(sd['state'][name][sname].shape)} does not fit parameter storage {tuple(param.shape)}")
                laid.append((views[name], t))
        for dst, t in laid:
            dst.copy_(t)
        self._set_hyper(group)
        self.steps = steps.pop()

    def _set_hyper(self, group: Dict[str, Any]) -> None:
        for k, v in group.items():
            setattr(self, k, type(getattr(self, k))(v) if not isinstance(v, (tuple, list)) else tuple(float(x) for x in v))


class AdamHIP(_OptimHIP):
    kind = FEAR_OPT_ADAM
    state_names = ("exp_avg", "exp_avg_sq")

    def __init__(self, net, lr: float = 1e-4, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, max_grad_norm: Optional[float] = None):
        super().__init__(net, lr, weight_decay, max_grad_norm)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.exp_avg_flat, self.exp_avg_sq_flat = self._state_flat
        self.exp_avg, self.exp_avg_sq = self._state

    def _hyper(self):
        return {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay}

    def _descriptor(self) -> FearOptim:
        return FearOptim(kind=self.kind, lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, weight_decay=self.weight_decay)

    def _update(self, param, grad, states, n, st, coef, what) -> None:
        if coef is not None or self.kind != FEAR_OPT_ADAM:
            return super()._update(param, grad, states, n, st, coef, what)
        rc = self.lib.fear_adam_step(_p(param), _p(grad), _p(states[0]), _p(states[1]), n, self.lr, self.betas[0], self.betas[1], self.eps,
                                     self.weight_decay, self.steps, st)
        if rc != 0:
            raise TrainError(f"fear_adam_step failed with status {rc} on {what}")


class AdamWHIP(AdamHIP):
    """torch.optim.AdamW: the weight decay multiplies the parameter (p *= 1 - lr * weight_decay) instead of joining the gradient."""
    kind = FEAR_OPT_ADAMW

    def __init__(self, net, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_grad_norm: Optional[float] = None):
        super().__init__(net, lr, betas, eps, weight_decay, max_grad_norm)


class SGDHIP(_OptimHIP):
    """torch.optim.SGD; `momentum_buffer` exists only with momentum."""
    kind = FEAR_OPT_SGD

    def __init__(self, net, lr: float, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                 nesterov: bool = False, max_grad_norm: Optional[float] = None):
        if momentum < 0:
            raise ValueError("momentum must not be negative")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self.state_names = ("momentum_buffer",) if momentum != 0 else ()
        super().__init__(net, lr, weight_decay, max_grad_norm)
        self.momentum, self.dampening, self.nesterov = float(momentum), float(dampening), bool(nesterov)

    def _hyper(self):
        return {"lr": self.lr, "momentum": self.momentum, "dampening": self.dampening, "weight_decay": self.weight_decay,
                "nesterov": self.nesterov}

    def _descriptor(self) -> FearOptim:
        return FearOptim(kind=self.kind, nesterov=int(self.nesterov), lr=self.lr, weight_decay=self.weight_decay,
                         momentum=self.momentum, dampening=self.dampening)

    def _set_hyper(self, group):
        if (float(group.get("momentum", self.momentum)) != 0) != bool(self.state_names):
            raise ValueError("a momentum buffer cannot appear or vanish on load: build the optimiser with the checkpoint's momentum")
        super()._set_hyper(group)


# the keys of the reference's config/optimizer/*.yaml -> (class, its constructor's own names)
_OPTIMIZERS = {
    "adam": (AdamHIP, ("lr", "betas", "eps", "weight_decay")),
    "adamw": (AdamWHIP, ("lr", "betas", "eps", "weight_decay")),
    "sgd": (SGDHIP, ("lr", "momentum", "dampening", "weight_decay", "nesterov")),
}


def optimizer_arguments(cfg: Mapping[str, Any]) -> Tuple[type, Dict[str, Any]]:
    """(class, keyword arguments) for a mapping with the keys of the reference's optimiser YAMLs: `name` in adam | adamw | sgd
    plus that optimiser's fields.  An unknown name or key raises ValueError naming it.  Host logic only."""
    cfg = dict(cfg)
    if "name" not in cfg:
        raise ValueError("the optimiser configuration has no 'name'")
    name = cfg.pop("name")
    if name not in _OPTIMIZERS:
        raise ValueError(f"unknown optimizer {name!r}: expected one of {sorted(_OPTIMIZERS)}")
    cls, keys = _OPTIMIZERS[name]
    for k in cfg:
        if k not in keys:
            raise ValueError(f"unknown key {k!r} for optimizer {name!r}: expected {list(keys)}")
    if name == "sgd" and "lr" not in cfg:
        raise ValueError("optimizer 'sgd' needs the key 'lr'")
    return cls, cfg


def make_optimizer(net, cfg: Mapping[str, Any], gradient_clip_val: float = 0):
    """The optimiser the reference's configuration names (config/optimizer/*.yaml as a mapping) with the trainer's
    `gradient_clip_val` (0 = off)."""
    cls, kwargs = optimizer_arguments(cfg)
    return cls(net, max_grad_norm=gradient_clip_val or None, **kwargs)
