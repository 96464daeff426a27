"""float64 restatements of torch.optim.Adam / AdamW / SGD (no amsgrad, no maximize) and of torch.nn.utils.clip_grad_norm_
(norm_type = 2), written from the algorithms in torch's documentation.  A helper module of the optimiser tests (not collected):
tests/test_optim_reference_cpu.py pins it to torch itself in float64, tests/test_optim_family_gpu.py measures against it how far
an fp32 evaluation of the same formulas lies from the exact result."""
import math

import numpy as np


def clip_coef(grads, max_norm):
    """(total norm, coefficient) of clip_grad_norm_: the 2-norm over all tensors, min(1, max_norm / (norm + 1e-6))."""
    norm = math.sqrt(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads))
    return norm, min(1.0, max_norm / (norm + 1e-6))


class Adam:
    """torch.optim.Adam: the L2 term joins the gradient; `decoupled` makes it AdamW (the parameter shrinks by lr * weight_decay)."""

    def __init__(self, p, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False):
        self.p = np.array(p, dtype=np.float64)
        self.lr, self.betas, self.eps, self.weight_decay, self.decoupled = lr, betas, eps, weight_decay, decoupled
        self.exp_avg, self.exp_avg_sq, self.t = np.zeros_like(self.p), np.zeros_like(self.p), 0

    def step(self, grad, max_norm=None):
        g = np.array(grad, dtype=np.float64)
        if max_norm:
            g = g * clip_coef([g], max_norm)[1]
        self.t += 1
        b1, b2 = self.betas
        if self.decoupled:
            self.p = self.p - self.lr * self.weight_decay * self.p
        elif self.weight_decay != 0:
            g = g + self.weight_decay * self.p
        self.exp_avg = b1 * self.exp_avg + (1 - b1) * g
        self.exp_avg_sq = b2 * self.exp_avg_sq + (1 - b2) * g * g
        m_hat = self.exp_avg / (1 - b1 ** self.t)
        v_hat = self.exp_avg_sq / (1 - b2 ** self.t)
        self.p = self.p - self.lr * m_hat / (np.sqrt(v_hat) + self.eps)
        return self.p

    def state(self):
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}


class AdamW(Adam):
    def __init__(self, p, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(p, lr, betas, eps, weight_decay, decoupled=True)


class SGD:
    """torch.optim.SGD: b_1 = g_1, b_t = momentum * b_{t-1} + (1 - dampening) * g_t; Nesterov: g_t + momentum * b_t."""

    def __init__(self, p, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        self.p = np.array(p, dtype=np.float64)
        self.lr, self.momentum, self.dampening, self.weight_decay, self.nesterov = lr, momentum, dampening, weight_decay, nesterov
        self.buf, self.t = None, 0

    def step(self, grad, max_norm=None):
        g = np.array(grad, dtype=np.float64)
        if max_norm:
            g = g * clip_coef([g], max_norm)[1]
        self.t += 1
        if self.weight_decay != 0:
            g = g + self.weight_decay * self.p
        if self.momentum != 0:
            self.buf = g.copy() if self.buf is None else self.momentum * self.buf + (1 - self.dampening) * g
            g = g + self.momentum * self.buf if self.nesterov else self.buf
        self.p = self.p - self.lr * g
        return self.p

    def state(self):
        return {} if self.buf is None else {"momentum_buffer": self.buf}


# the reference's config/optimizer/{adam,adamw,sgd}.yaml (values only; `name` picks the rule) and the further cases of the tests
CASES = {
    "adam_yaml": ("adam", dict(lr=1e-4)),
    "adamw_yaml": ("adamw", dict(lr=3e-3, eps=1e-6, weight_decay=2e-6)),
    "sgd_yaml": ("sgd", dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-6)),
    "sgd_plain": ("sgd", dict(lr=1e-2, momentum=0.0)),
    "sgd_dampening": ("sgd", dict(lr=1e-2, momentum=0.9, dampening=0.5, weight_decay=1e-6)),
    "adam_l2": ("adam", dict(lr=1e-3, weight_decay=0.01)),
}


def make(name, p, kwargs):
    return {"adam": Adam, "adamw": AdamW, "sgd": SGD}[name](p, **kwargs)


def make_torch(name, params, kwargs):
    import torch
    return {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "sgd": torch.optim.SGD}[name](params, **kwargs)


def gradient_schedule(n, steps=5, seed=3):
    """(p0, [gradients]) of tests/test_train_optim.py::test_adam_operator_matches_torch: randn * 10^(step - 3), fp32 tensors."""
    import torch
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    return p0, [torch.randn(n, generator=g) * (10.0 ** (step - 3)) for step in range(1, steps + 1)]
