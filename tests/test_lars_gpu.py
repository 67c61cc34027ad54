"""LARS on the GPU: the fused HIP kernels (csrc/kernels/sgd.hip lars_norms_kernel /
lars_update_kernel) against the fp64 oracle backend, their determinism and composition, and the
executor's eager / graph / plan steps with optimizer="lars"."""
import pytest
import torch

from test_lars import HAND_SLOTS, HAND_TOTAL, TRAIN_LR, hand_buffers

from distributed_resnet_tensorflow_amd.models.spec import cifar_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import LARS_CHUNK, LARS_EXCLUDED, HipBackend, LarsTable, RefBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

# the hand-built list + a 300,000-element slot (37 chunks feed one norm) + a slot whose last two
# elements form a chunk of their own (8194 = one full chunk + 2); 308,480 elements = 1.23 MB of fp32
BIG = HAND_TOTAL
SLOTS = HAND_SLOTS + [(BIG, 300000, 300000, 1), (BIG + 300000, LARS_CHUNK + 2, LARS_CHUNK + 16, 1)]
TOTAL = BIG + 300000 + LARS_CHUNK + 16
HP = dict(lr=0.3, mu=0.9, wd=2e-4, gs=0.5, eta=0.001, eps=1e-9)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (a - b).norm().item() / max(b.norm().item(), 1e-300)


def _inside():
    inside = torch.zeros(TOTAL, dtype=torch.bool)
    for off, n, _, _ in SLOTS:
        inside[off:off + n] = True
    return inside


@pytest.fixture(scope="module")
def inputs():
    """w, m, g (fp64, CPU) drawn once and never modified."""
    return hand_buffers(TOTAL, SLOTS)


@pytest.fixture(scope="module")
def oracle(inputs):
    """RefBackend.lars_momentum in fp64 for the fp32 gradient and for the bf16-rounded gradient."""
    w0, m0, g0 = inputs
    be, out = RefBackend("cpu", dtype=torch.float64), {}
    table = LarsTable(SLOTS)
    for key, g in (("fp32", g0.float().double()), ("bf16", g0.bfloat16().double())):
        w, m, trust = w0.float().double(), m0.float().double(), torch.zeros(table.n)
        be.lars_momentum(w, m, g, None, table, 0, table.n, None, trust, torch.tensor([HP["lr"]], dtype=torch.float64),
                         HP["mu"], HP["wd"], HP["gs"], HP["eta"], HP["eps"])
        out[key] = (w, m, trust)
    RefBackend("cpu")  # (the process-wide reference dtype back to fp32)
    return out


class Dev:
    """Device copies of the inputs + workspaces; run() applies slots [first, first + n)."""

    def __init__(self, inputs, wire="fp32", skip=None):
        w0, m0, g0 = inputs
        self.table = LarsTable(SLOTS, "cuda")
        self.w, self.m = w0.float().cuda(), m0.float().cuda()
        self.g = g0.float().cuda() if wire == "fp32" else g0.bfloat16().cuda()
        gen = torch.Generator().manual_seed(77)
        self.wb = torch.randn(TOTAL, generator=gen).bfloat16().cuda()
        self.partials = torch.zeros(2 * self.table.chunks, device="cuda")
        self.trust = torch.full((self.table.n,), -1.0, device="cuda")
        self.lr = torch.tensor([HP["lr"]], device="cuda")
        self.skip = None if skip is None else torch.tensor([skip], dtype=torch.int32, device="cuda")

    def run(self, hip, first=0, n=None):
        hip.lars_momentum(self.w, self.m, self.g, self.wb, self.table, first, self.table.n if n is None else n,
                          self.partials, self.trust, self.lr, HP["mu"], HP["wd"], HP["gs"], HP["eta"], HP["eps"],
                          self.skip)
        torch.cuda.synchronize()
        return self

    def state(self):
        return [t.clone() for t in (self.w, self.m, self.wb, self.trust)]


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_lars_momentum_matches_fp64_oracle(hip, inputs, oracle, wire):
    """trust within 1e-4 relative (fp32 serial sums of <= 32 terms + a tree: ~1e-5 worst case), w and
    m rel() < 1e-4, w_bf16 rel() < 4e-3; padding inside slots and the gap between slots bitwise
    unchanged in all three buffers."""
    d = Dev(inputs, wire)
    w_in, m_in, wb_in = d.w.clone(), d.m.clone(), d.wb.clone()
    d.run(hip)
    we, me, te = oracle[wire]
    trust = d.trust.cpu().double()
    for i in range(d.table.n):
        print(f"slot {i}: trust hip {trust[i]:.9g} oracle {te[i]:.9g}")
        assert abs(trust[i] - te[i].double()) <= 1e-4 * abs(te[i].double()), i
    assert trust[1] == 1.0 and trust[3] == 1.0 and trust[4] == 1.0  # excluded / zero gradient / zero weights
    inside = _inside().cuda()
    figures = (rel(d.w[inside], we[inside.cpu()]), rel(d.m[inside], me[inside.cpu()]),
               rel(d.wb[inside].float(), we[inside.cpu()]))
    print("rel w, m, w_bf16:", figures)
    assert figures[0] < 1e-4 and figures[1] < 1e-4 and figures[2] < 4e-3
    assert torch.equal(d.wb[inside], d.w[inside].bfloat16())
    for got, before in ((d.w, w_in), (d.m, m_in), (d.wb, wb_in)):
        assert torch.equal(got[~inside], before[~inside])
        assert not torch.equal(got[inside], before[inside])


def test_lars_momentum_is_deterministic_and_composes(hip, inputs):
    """Bitwise: the same call twice; one call over all slots vs three calls over consecutive slot
    sub-ranges; a non-zero skip word changes nothing, lars_trust included."""
    a, b = Dev(inputs).run(hip).state(), Dev(inputs).run(hip).state()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = Dev(inputs)
    c.run(hip, 0, 2).run(hip, 2, 3).run(hip, 5, 2)
    for x, y in zip(a, c.state()):
        assert torch.equal(x, y)
    s = Dev(inputs, skip=1)
    before = s.state()
    s.run(hip)
    for x, y in zip(before, s.state()):
        assert torch.equal(x, y)
    assert float(s.trust[0]) == -1.0
    z = Dev(inputs, skip=0).run(hip)  # a zero skip word: the update runs
    for x, y in zip(a, z.state()):
        assert torch.equal(x, y)


def test_lars_with_unit_trust_is_the_momentum_kernel(hip, inputs):
    """Non-adapting slots (trust 1) get bit for bit the update of drn_sgd_momentum."""
    w0, m0, g0 = inputs
    n = 4096 + 16
    slots = [(0, 4096, 4096, 0), (4096, 16, 16, 0)]
    table = LarsTable(slots, "cuda")
    lr = torch.tensor([HP["lr"]], device="cuda")
    res = []
    for lars in (True, False):
        w, m, g = w0[:n].float().cuda(), m0[:n].float().cuda(), g0[:n].float().cuda()
        wb = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
        if lars:
            hip.lars_momentum(w, m, g, wb, table, 0, 2, torch.zeros(4, device="cuda"), torch.zeros(2, device="cuda"),
                              lr, HP["mu"], HP["wd"], HP["gs"], HP["eta"], HP["eps"])
        else:
            hip.sgd_momentum(w, m, g, wb, lr, HP["mu"], HP["wd"], HP["gs"])
        torch.cuda.synchronize()
        res.append((w, m, wb))
    for x, y in zip(*res):
        assert torch.equal(x, y)


# -- executor ----------------------------------------------------------------------------------------
def _lars_ex(spec, N, seed=3, data_seed=9, lr=0.5, **kw):
    ex = Executor(spec, N, HipBackend("cuda"), "cuda", seed=seed, optimizer="lars", **kw)
    g = torch.Generator().manual_seed(data_seed)
    ex.images.zero_()
    ex.images[..., :3] = torch.randn(N, 32, 32, 3, generator=g).bfloat16().cuda()
    ex.labels.copy_(torch.randint(0, 10, (N,), generator=g, dtype=torch.int32))
    ex.set_lr(lr)
    return ex


def _state(ex):
    torch.cuda.synchronize()
    return [t.clone() for t in (ex.P.master, ex.P.momentum, ex.P.bn_state, ex.lars_trust)]


def test_lars_joined_deferred_graph_and_plan_steps_are_bitwise_equal(monkeypatch):
    """tests/test_executor_gpu.py::test_deferred_stem_gradient_matches_joined_step with
    optimizer="lars" (the deferred tail updates the slot ranges [lo:], [hi:lo] and [:hi] in three
    calls), plus a native-plan replay as in tests/test_plan_gpu.py."""
    from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph
    from distributed_resnet_tensorflow_amd.runtime.plan import StepPlan
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    monkeypatch.setenv("DRN_DEFER_TAIL", "1")
    spec, N = cifar_resnet_v2(14), 16
    outs = {}
    for mode in ("joined", "deferred", "graph", "plan"):
        ex = _lars_ex(spec, N)
        assert ex._stem_hi == ex.stem_op.dw.numel() and ex.side is not None
        fn = lambda: (ex.forward(True), ex.backward(defer_tail=mode != "joined"), ex.apply_gradients())  # noqa: E731
        if mode == "graph":
            StepGraph(fn, warmup=2).replay()
        elif mode == "plan":
            plan = StepPlan(ex, warmup=1)
            for _ in range(2):
                plan.replay()
        else:
            for _ in range(3):
                fn()
        outs[mode] = _state(ex)
    trust = outs["joined"][3]
    assert bool(((trust > 0) & (trust <= 1)).all()) and bool((trust < 1).any())
    for mode in ("deferred", "graph", "plan"):
        for name, a, b in zip(("master", "momentum", "bn_state", "lars_trust"), outs["joined"], outs[mode]):
            assert torch.equal(a, b), (mode, name)


# Per-slot ||g|| of the HIP executor over the fp32 oracle executor's, conv and dense kernels (one
# momentum step of cifar_resnet_v2(8), N = 16, seed 5, from the same bf16-representable weights; the
# forward / backward kernels are those of the commit before LARS). Measured on an MI355X: ratios
# 0.99916 .. 1.00942, largest |ratio - 1| = 0.00942 (conv2d_2/kernel; the figure moves by ~2e-3
# from run to run with the fp32 atomics of the weight gradients). trust = eta |w| / (|g| + wd |w| +
# eps) moves by at most the relative change of |g|; the test allows twice the measured deviation.
# (The LARS run of the same step showed trust deviations of up to 0.00903.)
MEASURED_GNORM_DEV = 0.00942
TRUST_BOUND = 2 * MEASURED_GNORM_DEV


def gnorm_and_trust(optimizer):
    """(per-slot ||g|| ratio HIP / oracle, per-slot trust of both) after one step from equal weights."""
    spec, N = cifar_resnet_v2(8), 16
    torch.manual_seed(0)
    imgs = torch.randn(N, 32, 32, 3).bfloat16().float()
    labels = torch.randint(0, 10, (N,), dtype=torch.int32)
    exs = []
    for be, dev in ((RefBackend(), "cpu"), (HipBackend("cuda"), "cuda")):
        ex = Executor(spec, N, be, dev, seed=5, optimizer=optimizer)
        ex.P.master.copy_(ex.P.master.bfloat16().float())
        ex.sync_weights()
        ex.images.zero_()
        ex.images[..., :3] = imgs.to(dev)
        ex.labels.copy_(labels.to(dev))
        ex.train_step(lr=0.1)
        exs.append(ex)
    torch.cuda.synchronize()
    r, h = exs
    rows = []
    for i, s in enumerate(r.P.slots):
        if s.kind in LARS_EXCLUDED:
            continue
        sl = slice(s.offset, s.offset + s.numel)
        ratio = float(h.P.grad[sl].double().norm().cpu() / r.P.grad[sl].double().norm())
        tr = (float(h.lars_trust[i]), float(r.lars_trust[i])) if optimizer == "lars" else None
        rows.append((s.name, ratio, tr))
    return rows


def test_executor_trust_tracks_the_oracle_executor():
    rows = gnorm_and_trust("lars")
    worst = 0.0
    for name, ratio, (th, tr) in rows:
        print(f"{name}: |g| hip/oracle {ratio:.6f}  trust hip {th:.6g} oracle {tr:.6g}  dev {abs(th / tr - 1):.3g}")
        worst = max(worst, abs(th / tr - 1))
    assert len(rows) == 11 and worst <= TRUST_BOUND, worst  # 10 conv kernels + the dense kernel


def test_lars_training_halves_the_loss():
    """30 LARS steps on a fixed batch (cifar_resnet_v2(8), N = 32, eta = 0.001) at the constant LR
    picked on the oracle executor (tests/test_lars.py TRAIN_LR): the loss at least halves."""
    N = 32
    ex = Executor(cifar_resnet_v2(8), N, HipBackend("cuda"), "cuda", seed=3, optimizer="lars", lars_eta=0.001)
    g = torch.Generator().manual_seed(11)
    ex.images.zero_()
    ex.images[..., :3] = torch.randn(N, 32, 32, 3, generator=g).bfloat16().cuda()
    ex.labels.copy_(torch.randint(0, 10, (N,), generator=g, dtype=torch.int32))
    ex.set_lr(TRAIN_LR)
    ex.forward(train=True)
    first = float(ex.loss_vec.double().mean())
    for _ in range(30):
        ex.train_step()
    ex.forward(train=True)
    final = float(ex.loss_vec.double().mean())
    print("loss", first, "->", final)
    assert final == final and final <= 0.5 * first, (first, final)
