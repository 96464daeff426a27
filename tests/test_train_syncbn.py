"""SyncBatchNorm operators (include/fear_train.h; the reference's multi-GPU backends train with sync_bn: True,
config/backend/{2,4}gpu.yaml -> trainer.py:52).  One GPU here, so the semantics are checked by playing two ranks on it: the
two halves of a batch reduce separately, their float64 sums are added (what the all-reduce does), and the result must equal
BatchNorm over the whole batch; the torch.distributed plumbing runs with a one-rank RCCL group."""
import ctypes
import os
import socket

import pytest
import torch

from syncref import PWBN_SYNC_CASES, SEPBN_SYNC_CASES, STEM_SYNC_CASES

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_half_batches_with_added_sums_equal_full_batch_batchnorm():
    from feartracker_amd.train_head import _p, load_train_library
    lib = load_train_library()
    dev = torch.device("cuda:0")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(5)
    M, C = 2 * 1536, 96
    x = (torch.randn(M, C, generator=g) * 2 + 0.7).to(dev)
    dy = torch.randn(M, C, generator=g).to(dev)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.rand(C, generator=g) - 0.5).to(dev)
    ws = torch.empty(lib.fear_train_workspace_bytes(M, C) // 4 + 1024, device=dev)
    wsb = ws.numel() * 4
    new = lambda *s: torch.empty(s, device=dev)
    # ---- whole batch, plain BatchNorm
    y, mean, rstd = new(M, C), new(C), new(C)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    assert lib.fear_bn_train_forward(_p(x), C, _p(gamma), _p(beta), _p(y), C, _p(mean), _p(rstd), _p(rm), _p(rv), 0.1, 1e-5, M, C, 1,
                                     _p(ws), wsb, st) == 0
    dx, dgamma, dbeta = new(M, C), new(C), new(C)
    assert lib.fear_bn_train_backward(_p(dy), C, _p(y), C, _p(x), C, _p(mean), _p(rstd), _p(gamma), _p(dx), C, _p(dgamma), _p(dbeta),
                                      M, C, _p(ws), wsb, st) == 0
    # ---- two "ranks": halves of the batch, sums added in between
    h = M // 2
    halves = [(x[:h].contiguous(), dy[:h].contiguous()), (x[h:].contiguous(), dy[h:].contiguous())]
    sums = [torch.empty(2 * C, dtype=torch.float64, device=dev) for _ in halves]
    for (xh, _), s in zip(halves, sums):
        assert lib.fear_bn_reduce(_p(xh), C, _p(s), h, C, _p(ws), wsb, st) == 0
    total = sums[0] + sums[1]
    outs = []
    for xh, _ in halves:
        yh, mh, rh = new(h, C), new(C), new(C)
        rmh, rvh = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        assert lib.fear_bn_forward_from_sums(_p(xh), C, _p(total), float(M), _p(gamma), _p(beta), _p(yh), C, _p(mh), _p(rh), _p(rmh),
                                             _p(rvh), 0.1, 1e-5, h, C, 1, st) == 0
        outs.append((yh, mh, rh, rmh, rvh))
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([o[0] for o in outs]), y)                  # same float64 sums up to the order of two additions:
    for o in outs:                                                           # the statistics agree to fp32 rounding, y bit for bit here
        for a, b in zip(o[1:], (mean, rstd, rm, rv)):
            assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())
    bsums = [torch.empty(2 * C, dtype=torch.float64, device=dev) for _ in halves]
    for (xh, dyh), o, s in zip(halves, outs, bsums):
        assert lib.fear_bn_backward_reduce(_p(dyh), C, _p(o[0]), C, _p(xh), C, _p(o[1]), _p(o[2]), _p(s), h, C, _p(ws), wsb, st) == 0
    btotal = bsums[0] + bsums[1]
    dxs, dgs, dbs = [], [], []
    for (xh, dyh), o, s in zip(halves, outs, bsums):
        dxh, dgh, dbh = new(h, C), new(C), new(C)
        assert lib.fear_bn_backward_from_sums(_p(dyh), C, _p(o[0]), C, _p(xh), C, _p(o[1]), _p(o[2]), _p(gamma), _p(btotal), float(M),
                                              _p(s), _p(dxh), C, _p(dgh), _p(dbh), _p(ws), wsb, h, C, st) == 0
        dxs.append(dxh); dgs.append(dgh); dbs.append(dbh)
    torch.cuda.synchronize()
    scale = float(dx.abs().max())
    assert float((torch.cat(dxs) - dx).abs().max()) <= 1e-5 * scale
    assert float((dgs[0] + dgs[1] - dgamma).abs().max()) <= 1e-5 * float(dgamma.abs().max())       # local sums add up to the
    assert float((dbs[0] + dbs[1] - dbeta).abs().max()) <= 1e-5 * float(dbeta.abs().max())         # full-batch parameter gradients
    # argument checks: count below the local row count is refused
    assert lib.fear_bn_forward_from_sums(_p(halves[0][0]), C, _p(total), float(h - 1), _p(gamma), _p(beta), _p(outs[0][0]), C,
                                         _p(outs[0][1]), _p(outs[0][2]), None, None, 0.1, 1e-5, h, C, 1, st) == -2


def test_sync_bn_step_with_a_one_rank_group_equals_the_plain_step():
    """The all-reduce plumbing (float64 sums on the device through RCCL, stream ordering against the operators): with one
    rank SyncBatchNorm is BatchNorm, so the whole training step must come out bit for bit."""
    import torch.distributed as dist
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    dev = torch.device("cuda:0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        sd = random_init_state(2)
        g = torch.Generator().manual_seed(4)
        B = 2
        tmpl, srch = torch.randn(B, 3, 128, 128, generator=g), torch.randn(B, 3, 256, 256, generator=g)
        gt_reg = torch.rand(B, 4, 16, 16, generator=g) * 60 + 1
        gt_cls = (torch.rand(B, 1, 16, 16, generator=g) > 0.8).float()
        gt_w = (torch.rand(B, 16, 16, generator=g) > 0.85).float()
        # (the layer-wise implementation of the trunk, its all-reduces between the passes; the block-fused default has its own test below)
        plain = FEARNetTrainHIP(sd, device=0, mode="layerwise").step(tmpl, srch, gt_reg, gt_cls, gt_w)
        net = FEARNetTrainHIP(sd, device=0, sync_bn=True, mode="layerwise")
        synced = net.step(tmpl, srch, gt_reg, gt_cls, gt_w)
        torch.cuda.synchronize()
        assert torch.equal(plain["bbox"], synced["bbox"]) and torch.equal(plain["cls"], synced["cls"])
        assert set(plain["grads"]) == set(synced["grads"])
        for k, v in plain["grads"].items():
            d = float((v - synced["grads"][k]).abs().max())
            assert d <= 1e-6 * max(float(v.abs().max()), 1e-12), (k, d)
        rs = net.running_stats()
        assert all(torch.isfinite(v).all() for v in rs.values())
    finally:
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------------------------
# Block-fused operators (round 6): the BatchNorm reductions sit inside one C call, the ranks' all-reduce is the library's hook
# (include/fear_train.h fear_train_sync_bind, feartracker_amd/train_head.SyncHook).


class _TwoRanksOnOneGPU:
    """`.world` / `.all_reduce(tensor)` for two host threads that play two ranks on one device: both deposit their buffer, meet at
    a barrier, and each leaves with the sum — what an all-reduce over two ranks does, in the issue order of the two threads."""

    def __init__(self):
        import threading
        self.world = 2
        self.barrier = threading.Barrier(2)
        self.slots = {}
        self.calls = 0
        self.local = threading.local()

    def all_reduce(self, t: torch.Tensor) -> None:
        rank = self.local.rank
        torch.cuda.current_stream().synchronize()           # this rank's sums are complete
        self.slots[rank] = t
        self.barrier.wait()
        total = self.slots[0] + self.slots[1]               # (fixed order: both ranks get the same bits)
        torch.cuda.current_stream().synchronize()
        self.barrier.wait()                                  # both have read both buffers
        t.copy_(total)
        if rank == 0:
            self.calls += 1
        self.barrier.wait()


def test_block_mode_two_half_batches_through_the_hook_equal_the_full_batch():
    """The trunk's block-fused forward and backward (fear_stem_train_*, fear_irb_train_* incl. the virtual expansions whose
    statistics come from the input's Gram matrix, fear_pwbn_train_*) on two half batches — two host threads, each with its own
    network object and streams, exchanging sums through the hook — against the same operators on the whole batch: the same
    features to fp32 rounding (the float64 sums meet in another order), running statistics equal, 94 all-reduces, and the two
    ranks' parameter gradients add up to the full batch's — to 2e-2 only: the float64 sums of two halves round differently from
    the whole batch's in the last bit, and 50 BatchNorms of a random-init ReLU network at 4 crops amplify that on the way back
    (the deviation is 5e-6 from the neck down to the last-but-one block and jumps where a low-variance channel sits;
    tools/r6_syncdiag.py prints it per tensor).  What pins the hook's arithmetic are the operator-level tests below, each against
    float64 autograd on the whole batch at 2e-4 of the tensor's largest entry: the inverted-residual block, and the stem, the neck
    unit and the head's layer in two-rank tests of their own."""
    import threading
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    dev = torch.device("cuda:0")
    sd = random_init_state(3)
    g = torch.Generator().manual_seed(9)
    B = 4
    img = torch.randn(B, 3, 128, 128, generator=g).to(dev)
    dfeat = torch.randn(B * 64, 256, generator=g).to(dev)

    def run(net, x, dy, bound):
        with torch.cuda.device(dev):
            stream = torch.cuda.Stream(device=dev)
            stream.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(stream):
                ctxm = net.hook.bound(stream) if bound else _null()
                with ctxm:
                    feats, ctx = net._features_forward_b(x)
                    gbuf = torch.zeros(net._ptotal, dtype=torch.float32, device=dev)
                    net._features_backward_b(ctx, dy, gbuf)
                stream.synchronize()
        return feats, gbuf, net.running_stats()

    import contextlib
    _null = contextlib.nullcontext
    full = run(FEARNetTrainHIP(sd, device=0, mode="block"), img, dfeat, False)
    fake = _TwoRanksOnOneGPU()
    nets = [FEARNetTrainHIP(sd, device=0, mode="block", sync_bn=fake) for _ in range(2)]
    out, errs = [None, None], []

    def rank_main(r):
        try:
            fake.local.rank = r
            h = B // 2
            out[r] = run(nets[r], img[r * h:(r + 1) * h].contiguous(), dfeat[r * h * 64:(r + 1) * h * 64].contiguous(), True)
        except BaseException as exc:      # noqa: BLE001
            errs.append(exc)
            fake.barrier.abort()
    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    assert fake.calls > 90          # stem + 16 blocks x (2 or 3) + neck BatchNorms, forward and backward
    feats = torch.cat([out[0][0], out[1][0]])
    scale = float(full[0].abs().max())
    assert float((feats - full[0]).abs().max()) <= 2e-5 * scale
    gsum = out[0][1] + out[1][1]
    gs = float(full[1].abs().max())
    assert float((gsum - full[1]).abs().max()) <= 2e-2 * gs, float((gsum - full[1]).abs().max()) / gs
    for r in range(2):              # both ranks track the statistics of ALL rows
        for k, v in full[2].items():
            if k.startswith("connect_model."):
                continue
            assert float((out[r][2][k] - v).abs().max()) <= 1e-5 * float(v.abs().max()) + 1e-6, k


def test_block_mode_sync_bn_step_with_a_one_rank_group_equals_the_plain_block_step():
    """FEARNetTrainHIP(mode="block", sync_bn=True) through a real RCCL group of one rank: every BatchNorm of the step goes local
    sums -> hook -> RCCL all-reduce -> finalize on its stream (two streams + the weight-gradient stream, as on one rank) and must
    come out bit for bit as the plain block step — with one rank the two-stage finalize adds one term."""
    import torch.distributed as dist
    from feartracker_amd.train_net import FEARNetTrainHIP, random_init_state
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    dev = torch.device("cuda:0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        sd = random_init_state(2)
        g = torch.Generator().manual_seed(4)
        B = 2
        tmpl, srch = torch.randn(B, 3, 128, 128, generator=g), torch.randn(B, 3, 256, 256, generator=g)
        gt_reg = torch.rand(B, 4, 16, 16, generator=g) * 60 + 1
        gt_cls = (torch.rand(B, 1, 16, 16, generator=g) > 0.8).float()
        gt_w = (torch.rand(B, 16, 16, generator=g) > 0.85).float()
        plain_net = FEARNetTrainHIP(sd, device=0, mode="block")
        plain = plain_net.step(tmpl, srch, gt_reg, gt_cls, gt_w)
        net = FEARNetTrainHIP(sd, device=0, mode="block", sync_bn=True)
        assert net.mode == "block" and net.hook is not None and net.two_streams
        synced = net.step(tmpl, srch, gt_reg, gt_cls, gt_w)
        torch.cuda.synchronize()
        assert torch.equal(plain["bbox"], synced["bbox"]) and torch.equal(plain["cls"], synced["cls"])
        assert set(plain["grads"]) == set(synced["grads"])
        for k, v in plain["grads"].items():
            assert torch.equal(v, synced["grads"][k]), k
        for k, v in plain_net.running_stats().items():
            assert torch.equal(v, net.running_stats()[k]), k
        # the binding is the step's: afterwards the streams run the one-rank form again
        again = FEARNetTrainHIP(sd, device=0, mode="block").step(tmpl, srch, gt_reg, gt_cls, gt_w)
        assert torch.equal(again["bbox"], plain["bbox"])
    finally:
        dist.destroy_process_group()


def test_sync_bind_argument_checks():
    from feartracker_amd.train_head import FearSync, _ALLREDUCE_FN, load_train_library
    lib = load_train_library()
    cb = _ALLREDUCE_FN(lambda *a: 0)
    buf = torch.zeros(2048, dtype=torch.float64, device="cuda:0")
    st = ctypes.c_void_p(torch.cuda.Stream().cuda_stream)
    assert lib.fear_train_sync_bind(st, ctypes.byref(FearSync(cb, None, None, 16384, 1))) == -1           # no buffer
    assert lib.fear_train_sync_bind(st, ctypes.byref(FearSync(cb, None, buf.data_ptr(), 1024, 1))) == -2  # buffer too small
    assert lib.fear_train_sync_bind(st, ctypes.byref(FearSync(cb, None, buf.data_ptr(), 16384, 0))) == -2  # world < 1
    assert lib.fear_train_sync_bind(st, ctypes.byref(FearSync(cb, None, buf.data_ptr(), 16384, 2))) == 0
    assert lib.fear_train_sync_bind(st, None) == 0
    assert lib.fear_train_sync_bind(st, None) == 0                                                           # unbinding twice is fine


SYNC_BLOCK_CASES = [
    # cin, cexp, cout, k, stride, expand, residual,   B (all ranks), H, flags
    ((16, 16, 16, 3, 1, 0, 1), 4, 32, 0),
    ((16, 96, 24, 3, 2, 1, 0), 4, 32, 4),        # virtual expansion: BatchNorm1's statistics from the all-reduced Gram matrix
    ((24, 144, 32, 5, 2, 1, 0), 2, 32, 4),
    ((32, 192, 32, 5, 1, 1, 1), 4, 16, 0),       # E-free BatchNorm1 backward (chosen by the call: 32 input channels)
    ((64, 384, 112, 5, 1, 1, 0), 6, 16, 0),
    ((112, 672, 112, 5, 1, 1, 1), 4, 8, 0),      # the template branch's last stage, 8 x 8 tiles
    ((112, 336, 112, 5, 1, 1, 1), 2, 16, 0),
]


# ---- one rank's side of an operator: device buffers from the float64 inputs, forward(st) / backward(st, aux) -> status,
# state() = what a failed forward must leave as it was, result() = what syncref.compare reads.  The two-rank tests build one per
# played rank from its half of the batch; the failing-all-reduce tests build one and play two ranks holding the same data.

def _f32(t, dev):
    return None if t is None else t.detach().to(dev, torch.float32).contiguous()


class _PwbnRank:
    def __init__(self, lib, dev, inp, sl, relu, need_dx):
        self.lib, self.relu = lib, relu
        self.x, self.dy = _f32(inp["x"][sl], dev), _f32(inp["dy"][sl], dev)
        self.w, self.gamma, self.beta = (_f32(inp[k], dev) for k in ("w", "gamma", "beta"))
        self.M, self.K = self.x.shape
        self.N = N = self.w.shape[0]
        self.rm, self.rv = torch.zeros(N, device=dev), torch.ones(N, device=dev)
        self.raw, self.out = torch.empty(self.M, N, device=dev), torch.empty(self.M, N, device=dev)
        self.vec = torch.full((4 * N,), -7.0, device=dev)
        self.ws = torch.empty(int(lib.fear_pwbn_workspace_bytes(self.M, self.K, N)) // 4 + 64, device=dev)
        nan = lambda *sh: torch.full(sh, float("nan"), device=dev)
        self.dw, self.dg, self.db = nan(N, self.K), nan(N), nan(N)
        self.dx = nan(self.M, self.K) if need_dx else None

    def forward(self, st):
        from feartracker_amd.train_head import _p
        return self.lib.fear_pwbn_train_forward(_p(self.x), self.K, _p(self.w), _p(self.gamma), _p(self.beta), _p(self.rm), _p(self.rv), _p(self.raw),
                                                _p(self.vec), self.relu, _p(self.out), self.M, self.K, self.N, 0.1, 1e-5, _p(self.ws),
                                                self.ws.numel() * 4, st)

    def backward(self, st, aux=None):
        from feartracker_amd.train_head import _p
        return self.lib.fear_pwbn_train_backward(_p(self.dy), _p(self.raw), _p(self.vec), self.relu, _p(self.x), self.K, _p(self.w), _p(self.gamma),
                                                 _p(self.dw), _p(self.dg), _p(self.db), _p(self.dx), self.M, self.K, self.N, _p(self.ws),
                                                 self.ws.numel() * 4, st, aux)

    def state(self, failed=0):
        return [self.rm, self.rv, self.vec]

    def result(self):
        return {"out": self.out, "dx": self.dx, "d w": self.dw, "d gamma": self.dg, "d beta": self.db, "running_mean": self.rm, "running_var": self.rv}


class _StemRank:
    def __init__(self, lib, dev, inp, sl, rows_sl):
        self.lib = lib
        self.x, self.dy = _f32(inp["x"][sl], dev), _f32(inp["dy"][rows_sl], dev)
        self.n, _, self.H, self.W = self.x.shape
        self.M = self.dy.shape[0]
        self.w28 = torch.zeros(16, 28, device=dev)
        self.w28[:, :27] = _f32(inp["w"], dev).reshape(16, 27)
        self.gamma, self.beta = _f32(inp["gamma"], dev), _f32(inp["beta"], dev)
        self.rm, self.rv = torch.zeros(16, device=dev), torch.ones(16, device=dev)
        self.raw, self.out = torch.empty(self.M, 16, device=dev), torch.empty(self.M, 16, device=dev)
        self.vec = torch.full((64,), -7.0, device=dev)
        self.ws = torch.empty(int(lib.fear_stem_workspace_bytes(self.n, self.H, self.W)) // 4 + 64, device=dev)
        nan = lambda *sh: torch.full(sh, float("nan"), device=dev)
        self.dw, self.dg, self.db = nan(16, 28), nan(16), nan(16)

    def forward(self, st):
        from feartracker_amd.train_head import _p
        return self.lib.fear_stem_train_forward(_p(self.x), _p(self.w28), _p(self.gamma), _p(self.beta), _p(self.rm), _p(self.rv), _p(self.raw),
                                                _p(self.vec), _p(self.out), self.n, self.H, self.W, 0.1, 1e-5, _p(self.ws), self.ws.numel() * 4, st)

    def backward(self, st, aux=None):
        from feartracker_amd.train_head import _p
        return self.lib.fear_stem_train_backward(_p(self.dy), _p(self.raw), _p(self.vec), _p(self.x), _p(self.gamma), _p(self.dw), _p(self.dg),
                                                 _p(self.db), self.n, self.H, self.W, _p(self.ws), self.ws.numel() * 4, st, aux)

    def state(self, failed=0):
        return [self.rm, self.rv, self.vec]

    def result(self):
        return {"out": self.out, "d w": self.dw[:, :27].reshape(16, 3, 3, 3), "d gamma": self.dg, "d beta": self.db, "running_mean": self.rm,
                "running_var": self.rv}


class _SepbnRank:
    def __init__(self, lib, dev, inp, sl, rows_sl, ldx_pad, ldo_pad):
        from feartracker_amd.train_head import FearSepGrads, FearSepLayer
        from syncref import rows
        self.lib = lib
        x = inp["x"][sl]
        self.B, self.cin, self.H, self.W = x.shape
        self.cout = cout = inp["w"].shape[0]
        self.M = M = self.B * self.H * self.W
        self.ldx, self.ldo = self.cin + ldx_pad, cout + ldo_pad
        self.x = torch.zeros(M, self.ldx, device=dev)
        self.x[:, :self.cin] = _f32(rows(x), dev)
        self.dy = _f32(inp["dy"][rows_sl], dev)
        self.par = [_f32(inp[k], dev) for k in ("taps", "b_dw", "w", "b_pw", "gamma", "beta")]
        self.rm, self.rv = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()
        self.L = FearSepLayer(self.cin, cout, *(ptr(t) for t in self.par), ptr(self.rm), ptr(self.rv))
        self.ws = torch.empty(int(lib.fear_sepbn_workspace_bytes(ctypes.byref(self.L), self.B, self.H, self.W)) // 4 + 64, device=dev)
        self.d, self.raw = torch.empty(M, self.cin, device=dev), torch.empty(M, cout, device=dev)
        self.vec = torch.full((4 * cout,), -7.0, device=dev)
        self.outp = torch.full((M, self.ldo), 7.0, device=dev)
        nan = lambda *sh: torch.full(sh, float("nan"), device=dev)
        self.gt, self.gw, self.gg, self.gb = nan(9, self.cin), nan(cout, self.cin), nan(cout), nan(cout)
        self.dd, self.coef, self.dx = torch.empty(M, self.cin, device=dev), torch.empty(4 * cout, device=dev), nan(M, self.cin)
        self.G = FearSepGrads(self.gt.data_ptr(), self.gw.data_ptr(), self.gg.data_ptr(), self.gb.data_ptr())

    def forward(self, st):
        from feartracker_amd.train_head import _p
        return self.lib.fear_sepbn_train_forward(ctypes.byref(self.L), _p(self.x), self.ldx, _p(self.d), _p(self.raw), _p(self.vec), _p(self.outp),
                                                 self.ldo, self.B, self.H, self.W, 0.1, 1e-5, _p(self.ws), self.ws.numel() * 4, st)

    def backward(self, st, aux=None):
        from feartracker_amd.train_head import _p
        return self.lib.fear_sepbn_train_backward(ctypes.byref(self.L), ctypes.byref(self.G), _p(self.x), self.ldx, _p(self.d), _p(self.raw),
                                                  _p(self.vec), _p(self.dy), _p(self.dd), _p(self.coef), _p(self.dx), self.B, self.H, self.W,
                                                  _p(self.ws), self.ws.numel() * 4, st, aux)

    def state(self, failed=0):
        return [self.rm, self.rv, self.vec]

    def result(self):
        return {"out": self.outp[:, :self.cout], "dx": self.dx, "d taps": self.gt, "d w": self.gw, "d gamma": self.gg, "d beta": self.gb,
                "running_mean": self.rm, "running_var": self.rv}


class _IrbRank:
    def __init__(self, lib, dev, cfg, flags, p, x, dout):
        """x, dout: this rank's (b, C, H, W) float64 halves; p: the block's float64 parameters"""
        from feartracker_amd.train_head import FearIrbBlock, FearIrbGrads, FearIrbSaved
        from syncref import rows
        self.lib = lib
        cin, cexp, cout, k, stride, expand, residual = cfg
        self.expand, self.chans = expand, (cexp, cexp, cout)
        self.b, _, self.H, self.W = b, _, H, W = x.shape
        rows_in, rows_out = b * H * W, b * (H // stride) * (W // stride)
        self.blk = blk = FearIrbBlock()
        blk.cin, blk.cexp, blk.cout, blk.k, blk.stride, blk.expand, blk.residual, blk.flags = cin, cexp, cout, k, stride, expand, residual, flags
        self.keep = keep = {n_: _f32(v, dev) for n_, v in p.items()}
        blk.w_pw, blk.w_dw, blk.w_pwl = (keep["w_pw"].data_ptr() if expand else None), keep["w_dw"].data_ptr(), keep["w_pwl"].data_ptr()
        self.rm, self.rv = [], []
        for i in range(3):
            self.rm.append(torch.zeros(self.chans[i], device=dev)); self.rv.append(torch.ones(self.chans[i], device=dev))
            blk.gamma[i], blk.beta[i] = keep[f"g{i}"].data_ptr(), keep[f"b{i}"].data_ptr()
            blk.running_mean[i], blk.running_var[i] = self.rm[i].data_ptr(), self.rv[i].data_ptr()
        self.ws = torch.empty(int(lib.fear_irb_workspace_bytes(ctypes.byref(blk), b, H, W)) // 4 + 64, device=dev)
        self.scratch = torch.empty(int(lib.fear_irb_scratch_floats(ctypes.byref(blk), b, H, W)) + 64, device=dev)
        self.sv = sv = FearIrbSaved()
        self.e = torch.empty(rows_in, cexp, device=dev) if expand and not flags & 4 else None
        self.d, self.pp = torch.empty(rows_out, cexp, device=dev), torch.empty(rows_out, cout, device=dev)
        self.vec = [torch.full((4 * c,), -7.0, device=dev) for c in self.chans]
        sv.e, sv.d, sv.p = (self.e.data_ptr() if self.e is not None else None), self.d.data_ptr(), self.pp.data_ptr()
        for i in range(3):
            sv.vec[i] = self.vec[i].data_ptr()
        self.xd, self.dyd = _f32(rows(x), dev), _f32(rows(dout), dev)
        self.out = torch.empty(rows_out, cout, device=dev)
        nan = lambda *sh: torch.full(sh, float("nan"), device=dev)
        self.gr = gr = FearIrbGrads()
        self.gw_pw = nan(cexp, cin) if expand else None
        self.gw_dw, self.gw_pwl = nan(k * k, cexp), nan(cout, cexp)
        gr.w_pw, gr.w_dw, gr.w_pwl = (self.gw_pw.data_ptr() if expand else None), self.gw_dw.data_ptr(), self.gw_pwl.data_ptr()
        self.gg, self.gb = [nan(c) for c in self.chans], [nan(c) for c in self.chans]
        for i in range(3):
            gr.gamma[i], gr.beta[i] = self.gg[i].data_ptr(), self.gb[i].data_ptr()
        self.dx = nan(rows_in, cin)

    def forward(self, st):
        from feartracker_amd.train_head import _p
        return self.lib.fear_irb_train_forward(ctypes.byref(self.blk), ctypes.byref(self.sv), _p(self.xd), _p(self.out), self.b, self.H, self.W, 0.1,
                                               1e-5, _p(self.ws), self.ws.numel() * 4, st)

    def backward(self, st, aux=None):
        from feartracker_amd.train_head import _p
        return self.lib.fear_irb_train_backward(ctypes.byref(self.blk), ctypes.byref(self.sv), ctypes.byref(self.gr), _p(self.xd), _p(self.dyd),
                                                _p(self.dx), _p(self.scratch), self.b, self.H, self.W, _p(self.ws), self.ws.numel() * 4, st, aux)

    def first_bn(self):
        return 0 if self.expand else 1

    def state(self, failed=0):
        """the BatchNorms from the `failed`-th all-reduce of a forward on (those before it completed, and rightly updated theirs)"""
        return [t for i in range(self.first_bn() + failed, 3) for t in (self.rm[i], self.rv[i], self.vec[i])]

    def result(self):
        res = {"out": self.out, "dx": self.dx, "d w_dw": self.gw_dw, "d w_pwl": self.gw_pwl, "d w_pw": self.gw_pw}
        for i in range(self.first_bn(), 3):
            res.update({f"d gamma{i}": self.gg[i], f"d beta{i}": self.gb[i], f"running_mean{i}": self.rm[i], f"running_var{i}": self.rv[i]})
        return res


def _irb_reference(cfg, B, H, W, seed, doubled=False):
    """float64 parameters, input, output gradient and torch autograd on the whole batch for one inverted-residual block (with
    `doubled`, the drawn batch twice: two ranks that hold the same data), in syncref.compare's keys"""
    from syncref import rows
    from test_train_block import _torch_block
    cin, cexp, cout, k, stride, expand, residual = cfg
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64)
    p = {"w_dw": torch.randn(k * k, cexp, generator=g, dtype=torch.float64) * (2.0 / (k * k)) ** 0.5,
         "w_pwl": torch.randn(cout, cexp, generator=g, dtype=torch.float64) * (2.0 / cexp) ** 0.5}
    if expand:
        p["w_pw"] = torch.randn(cexp, cin, generator=g, dtype=torch.float64) * (2.0 / cin) ** 0.5
    chans = (cexp, cexp, cout)
    for i in range(3):
        p[f"g{i}"] = torch.rand(chans[i], generator=g, dtype=torch.float64) + 0.5
        p[f"b{i}"] = torch.randn(chans[i], generator=g, dtype=torch.float64) * 0.3
    if doubled:
        x = torch.cat([x, x])
    x.requires_grad_(True)
    for v in p.values():
        v.requires_grad_(True)
    stats = {}
    for i in range(3):
        stats[f"rm{i}"] = torch.zeros(chans[i], dtype=torch.float64)
        stats[f"rv{i}"] = torch.ones(chans[i], dtype=torch.float64)
    y = _torch_block(x, p, cfg, stats)
    dout = torch.randn(y.shape[0] // (2 if doubled else 1), *y.shape[1:], generator=g, dtype=torch.float64)
    if doubled:
        dout = torch.cat([dout, dout])
    y.backward(dout)
    ref = {"out": rows(y), "dx": rows(x.grad), "d w_dw": p["w_dw"].grad, "d w_pwl": p["w_pwl"].grad, "d w_pw": p["w_pw"].grad if expand else None}
    for i in range(0 if expand else 1, 3):
        ref.update({f"d gamma{i}": p[f"g{i}"].grad, f"d beta{i}": p[f"b{i}"].grad, f"running_mean{i}": stats[f"rm{i}"],
                    f"running_var{i}": stats[f"rv{i}"]})
    return {n_: v.detach() for n_, v in p.items()}, x.detach(), dout, ref


def _play_two_ranks(make_rank, aux_stream=False):
    """The per-rank boilerplate of every two-rank test: two host threads, each with a stream of its own bound to the all-reduce
    hook, run `make_rank(r)`'s forward and backward (with `aux_stream`, the weight gradients on a second, unbound stream).
    Returns the fake group and both ranks' results."""
    import threading
    from feartracker_amd.train_head import SyncHook, load_train_library
    lib = load_train_library()
    dev = torch.device("cuda:0")
    fake = _TwoRanksOnOneGPU()
    res, errs_t = [None, None], []

    def rank_main(r):
        try:
            fake.local.rank = r
            op = make_rank(lib, dev, r)
            stream = torch.cuda.Stream(device=dev)
            aux = torch.cuda.Stream(device=dev) if aux_stream else None
            stream.wait_stream(torch.cuda.current_stream(dev))       # the fills of the rank's buffers
            hook = SyncHook(lib, fake, dev)
            with torch.cuda.stream(stream), hook.bound(stream):
                st = ctypes.c_void_p(stream.cuda_stream)
                assert op.forward(st) == 0
                assert op.backward(st, ctypes.c_void_p(aux.cuda_stream) if aux else None) == 0
                stream.synchronize()
                if aux:
                    aux.synchronize()
            assert hook.error is None, hook.error
            res[r] = (op, op.result())
        except BaseException as exc:      # noqa: BLE001
            errs_t.append(exc)
            fake.barrier.abort()
    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs_t, errs_t
    return fake, [r[0] for r in res], [r[1] for r in res]


def _assert_within_tolerance(ranks, ref):
    from syncref import TOL, compare
    errs = compare(ranks, ref)
    print({k_: f"{v:.1e}" for k_, v in errs.items()})
    bad = {k_: v for k_, v in errs.items() if not v < TOL}
    assert not bad, bad


@pytest.mark.parametrize("cfg,B,H,flags", SYNC_BLOCK_CASES,
                         ids=[f"{c[0]}x{c[1]}x{c[2]}k{c[3]}s{c[4]}_b{b}h{h}" + ("_virtual" if f else "") for c, b, h, f in SYNC_BLOCK_CASES])
def test_irb_block_on_two_ranks_through_the_hook_matches_full_batch_autograd(cfg, B, H, flags):
    """One inverted-residual block (fear_irb_train_forward / _backward) on the two halves of a batch — two host threads, each stream
    bound to the all-reduce hook — against torch autograd (float64) on the WHOLE batch: outputs and input gradients of both halves,
    the running statistics of both ranks, and the two ranks' parameter gradients added up (what DDP's gradient all-reduce does,
    up to the division by the world size)."""
    cin, cexp, cout, k, stride, expand, residual = cfg
    p, x, dout, ref = _irb_reference(cfg, B, H, H, 300 + cin + cexp + k + stride + H)
    h = B // 2
    fake, _, ranks = _play_two_ranks(lambda lib, dev, r: _IrbRank(lib, dev, cfg, flags, p, x[r * h:(r + 1) * h], dout[r * h:(r + 1) * h]))
    assert fake.calls == (6 if expand else 4)
    _assert_within_tolerance(ranks, ref)


# ---- the other operators with a BatchNorm inside on two played ranks.  Inputs and the whole-batch float64 reference: tests/syncref.py
# (rank 1's half is 1.5 x + 1.0 of its draw; tests/test_syncbn_reference_cpu.py shows on these very inputs that a finalize from the
# local sums, a count without the world size, d gamma / d beta from the all-reduced sums or a forgotten bias shift is off by > 10 x
# the tolerance).  Each: one all-reduce in the forward, one in the backward.


@pytest.mark.parametrize("M,K,N,relu,need_dx", PWBN_SYNC_CASES)
def test_pwbn_unit_on_two_ranks_through_the_hook_matches_full_batch_autograd(M, K, N, relu, need_dx):
    """fear_pwbn_train_* (the neck: 112 -> 256 without ReLU, through the LDS-staged GEMM; 28 -> 16 and 24 -> 40 through pw_stat_kernel,
    the last with 333 rows per rank — no multiple of the 128-row tile)."""
    import syncref
    inp = syncref.pwbn_sync_inputs(M, K, N, relu, need_dx)
    ref = syncref.pwbn_sync_reference(inp, relu)
    h = M // 2
    fake, _, ranks = _play_two_ranks(lambda lib, dev, r: _PwbnRank(lib, dev, inp, slice(r * h, (r + 1) * h), relu, need_dx))
    assert fake.calls == 2
    _assert_within_tolerance(ranks, ref)


@pytest.mark.parametrize("n,H,W", STEM_SYNC_CASES)
def test_stem_on_two_ranks_through_the_hook_matches_full_batch_autograd(n, H, W):
    """fear_stem_train_* on the two halves of an image batch (rank 1's images are 1.5 x + 1.0 of their draw)."""
    import syncref
    inp = syncref.stem_sync_inputs(n, H, W)
    ref = syncref.stem_sync_reference(inp)
    h, hr = n // 2, (n // 2) * (H // 2) * (W // 2)
    fake, ops, ranks = _play_two_ranks(lambda lib, dev, r: _StemRank(lib, dev, inp, slice(r * h, (r + 1) * h), slice(r * hr, (r + 1) * hr)))
    assert fake.calls == 2
    _assert_within_tolerance(ranks, ref)
    for op in ops:
        assert float(op.dw[:, 27].abs().max()) == 0.0


@pytest.mark.parametrize("B,H,W,cin,cout,bias,ldx_pad,ldo_pad", SEPBN_SYNC_CASES)
def test_sepbn_layer_on_two_ranks_through_the_hook_matches_full_batch_autograd(B, H, W, cin, cout, bias, ldx_pad, ldo_pad):
    """fear_sepbn_train_* (the head's layer): with biases the tracked running mean includes the pointwise bias, which the kernels keep
    out of `raw` (mean_shift in the synced finalize); rows with a pitch on either side; the rectangular case runs its backward with the
    weight gradients on a second stream, which is NOT bound — only the stream of the BatchNorm sums is."""
    import syncref
    inp = syncref.sepbn_sync_inputs(B, H, W, cin, cout, bias)
    ref = syncref.sepbn_sync_reference(inp)
    h, hr = B // 2, (B // 2) * H * W
    fake, ops, ranks = _play_two_ranks(lambda lib, dev, r: _SepbnRank(lib, dev, inp, slice(r * h, (r + 1) * h), slice(r * hr, (r + 1) * hr),
                                                                      ldx_pad, ldo_pad), aux_stream=H != W)
    assert fake.calls == 2
    _assert_within_tolerance(ranks, ref)
    for op in ops:
        assert ldo_pad == 0 or bool((op.outp[:, cout:] == 7.0).all())        # nothing written beyond the layer's own columns


# ---------------------------------------------------------------------------------------------------------------------------
# A failing all-reduce (include/fear_train.h, FEAR_TRAIN_ERR_SYNC): the entry point returns at once, the running statistics and the
# failed BatchNorm's `vec` are not written, and nothing of the failure is left for the next call of the thread.


class _TwoRanksWithTheSameData:
    """`.world` = 2 / `.all_reduce(t)` for ONE host thread: the other rank holds the same rows, so the sum is 2 t — a doubled batch
    has the same mean and biased variance, the unbiased running variance counts 2 M rows.  Raises on its `fail_at`-th call."""

    def __init__(self):
        self.world, self.calls, self.fail_at = 2, 0, 0

    def all_reduce(self, t: torch.Tensor) -> None:
        self.calls += 1
        if self.calls == self.fail_at:
            raise RuntimeError(f"all-reduce {self.calls} failed (played)")
        t.mul_(2)


def _fail_then_retry(make_op, ref, direction, fail_at=1):
    from feartracker_amd.train_head import SyncHook, _p, load_train_library
    lib = load_train_library()
    dev = torch.device("cuda:0")
    op = make_op(lib, dev)
    fake = _TwoRanksWithTheSameData()
    hook = SyncHook(lib, fake, dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    call = op.forward if direction == "forward" else op.backward
    with torch.cuda.stream(stream), hook.bound(stream):
        st = ctypes.c_void_p(stream.cuda_stream)
        if direction == "backward":
            assert op.forward(st) == 0
        stream.synchronize()
        everything = [t.clone() for t in op.state()]
        before = [t.clone() for t in op.state(fail_at - 1)]
        fake.calls, fake.fail_at = 0, fail_at
        rc = call(st)
        stream.synchronize()
        assert rc == -8, rc                                             # FEAR_TRAIN_ERR_SYNC
        assert isinstance(hook.error, RuntimeError) and "played" in str(hook.error)
        assert fake.calls == fail_at                                    # nothing went on to a later BatchNorm
        for i, (a, b) in enumerate(zip(op.state(fail_at - 1), before)):
            assert torch.equal(a, b), f"state tensor {i} was written by the failed call"
        # an operator that is not bound to the hook, in between: no trace of the failure on this thread
        xa = torch.ones(8, 4, device=dev)
        ab = torch.ones(4, device=dev)
        ya = torch.empty(8, 4, device=dev)
        stream.synchronize()
        assert lib.fear_bn_act(_p(xa), 4, _p(ab), _p(ab), 0, None, 0, _p(ya), 4, 8, 4, None) == 0
        torch.cuda.synchronize()
        assert bool((ya == 2.0).all())
        # the same operator again with a working all-reduce (BatchNorms that had completed before the failure take their first update
        # again: put back what they held, so that the reference's single update applies)
        for t, t0 in zip(op.state(), everything):
            t.copy_(t0)
        hook.error, fake.calls, fake.fail_at = None, 0, 0
        assert call(st) == 0
        stream.synchronize()
    assert hook.error is None
    res = op.result()
    if direction == "forward":
        res = {k_: v for k_, v in res.items() if k_ == "out" or k_.startswith("running_")}
    _assert_within_tolerance([res, res], ref)                            # two ranks with the same rows


_IRB_FAIL = (16, 96, 24, 3, 2, 1, 0)


def _irb_fail_op(flags):
    p, x, dout, ref = _irb_reference(_IRB_FAIL, 2, 16, 16, 77, doubled=True)
    return (lambda lib, dev: _IrbRank(lib, dev, _IRB_FAIL, flags, p, x[:2], dout[:2])), ref


def _pwbn_fail_op():
    import syncref
    M, K, N, relu, need_dx = 333, 24, 40, 1, True
    inp = syncref.pwbn_sync_inputs(M, K, N, relu, need_dx)
    two = {k_: torch.cat([v, v]) if k_ in ("x", "dy") else v for k_, v in inp.items()}
    return (lambda lib, dev: _PwbnRank(lib, dev, inp, slice(0, M), relu, need_dx)), syncref.pwbn_sync_reference(two, relu)


def _stem_fail_op():
    import syncref
    inp = syncref.stem_sync_inputs(2, 24, 40)
    two = {k_: torch.cat([v, v]) if k_ in ("x", "dy") else v for k_, v in inp.items()}
    return (lambda lib, dev: _StemRank(lib, dev, inp, slice(0, 2), slice(0, inp["dy"].shape[0]))), syncref.stem_sync_reference(two)


def _sepbn_fail_op():
    import syncref
    inp = syncref.sepbn_sync_inputs(2, 8, 8, 64, 48, True)
    two = {k_: torch.cat([v, v]) if k_ in ("x", "dy") else v for k_, v in inp.items()}
    return (lambda lib, dev: _SepbnRank(lib, dev, inp, slice(0, 2), slice(0, inp["dy"].shape[0]), 16, 0)), syncref.sepbn_sync_reference(two)


_FAIL_CASES = {
    "pwbn_forward": (_pwbn_fail_op, "forward", 1),
    "stem_forward": (_stem_fail_op, "forward", 1),
    "sepbn_forward": (_sepbn_fail_op, "forward", 1),
    "irb_forward": (lambda: _irb_fail_op(0), "forward", 1),
    "irb_forward_virtual": (lambda: _irb_fail_op(4), "forward", 1),          # the fp32 Gram all-reduce (is_f32) of FEAR_IRB_VIRTUAL_E
    "irb_forward_second_call": (lambda: _irb_fail_op(0), "forward", 2),      # BatchNorm0 completes, the depthwise BatchNorm's fails
    "pwbn_backward": (_pwbn_fail_op, "backward", 1),
    "irb_backward": (lambda: _irb_fail_op(0), "backward", 1),
}


@pytest.mark.parametrize("name", list(_FAIL_CASES))
def test_a_failing_all_reduce_returns_err_sync_and_leaves_the_statistics_and_the_thread_untouched(name):
    """The all-reduce callback raises on its k-th call (a host callback returning non-zero; every kernel runs on valid buffers): the
    entry point returns FEAR_TRAIN_ERR_SYNC, SyncHook.error holds the exception, the running statistics and the failed BatchNorm's
    vec (prefilled with a sentinel) are bit-equal to before, an unbound operator in between returns 0, and the same call with a working
    callback returns 0 with results within 2e-4 of float64 autograd on the doubled batch.  (Before the fix the second finalize ran
    over the un-reduced buffer with count * world rows and wrote all three.)"""
    make, direction, fail_at = _FAIL_CASES[name]
    make_op, ref = make()
    _fail_then_retry(make_op, ref, direction, fail_at)
