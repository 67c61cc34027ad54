"""AdamW / LAMB on the GPU: the fused HIP kernels (csrc/kernels/adam.hip) element by element against
fp64 references with derived bounds (adam_refs.adamw_ref) and against the fp64 oracle backend, their
determinism and composition, and the executor's eager / graph / plan steps."""
import pytest
import torch

import kernel_cases as kc
import kernel_refs as kr
from adam_refs import ADAM_HP, TRAIN_LR, adamw_ref, fixed_batch_executor, hand_adam_buffers
from test_lars_gpu import SLOTS, TOTAL, rel

from distributed_resnet_tensorflow_amd.ops._lib import KernelLibraryError
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend, LarsTable, RefBackend

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

HP = ADAM_HP
DECAY = 0.9
ARGS = (HP["b1"], HP["b2"], HP["eps"], HP["wd"], HP["gs"])


def _dev_scalars():
    lr = torch.tensor([HP["lr"]], device="cuda")
    bc = torch.tensor([HP["c1"], HP["c2"]], dtype=torch.float32, device="cuda")
    decay = torch.tensor([DECAY], device="cuda")
    return lr, bc, decay


# -- 8. adamw, element by element -----------------------------------------------------------------------
_adamw_cache: dict = {}


def adamw_inputs(n):
    """w0, m0, v0 (>= 0), e0 in fp32 and a bf16-representable gradient (one reference serves both
    gradient types), with the fp64 results and bounds; the latest size only is kept."""
    if n not in _adamw_cache:
        _adamw_cache.clear()
        g = torch.Generator().manual_seed(1000 + n % 997)
        w0, m0, e0 = (torch.randn(n, generator=g) for _ in range(3))
        v0 = torch.randn(n, generator=g) ** 2
        gr = torch.randn(n, generator=g).bfloat16().float()
        ref = adamw_ref(w0, m0, v0, gr, HP["lr"], *ARGS, HP["c1"], HP["c2"], e0=e0, decay=DECAY)
        _adamw_cache[n] = (w0, m0, v0, e0, gr, ref)
    return _adamw_cache[n]


def run_adamw(hip, n, g_bf16, with_wb, with_ema, skip):
    w0, m0, v0, e0, gr, ref = adamw_inputs(n)
    w, m, v, e = (t.cuda() for t in (w0, m0, v0, e0))
    wb0 = torch.full((n,), 7.0, dtype=torch.bfloat16, device="cuda")
    wb = wb0.clone() if with_wb else None
    lr, bc, decay = _dev_scalars()
    ema = dict(ema=e, ema_decay_t=decay) if with_ema else {}
    hip.adamw(w, m, v, gr.cuda().to(torch.bfloat16 if g_bf16 else torch.float32), wb, lr, bc, *ARGS,
              skip=torch.tensor([skip], dtype=torch.int32, device="cuda"), **ema)
    torch.cuda.synchronize()
    what = f"n {n} bf16 grad {g_bf16} wb {with_wb} ema {with_ema}"
    if skip:
        for got, before in ((w, w0), (m, m0), (v, v0), (e, e0)):
            assert torch.equal(got.cpu(), before), what
        assert wb is None or torch.equal(wb, wb0)
        return
    for key, got in (("w", w), ("m", m), ("v", v)) + ((("ema", e),) if with_ema else ()):
        kr.assert_within(got, ref[key][0], ref[key][1], f"adamw {key}: {what}")
    if not with_ema:
        assert torch.equal(e.cpu(), e0)
    if with_wb:
        assert torch.equal(wb, w.bfloat16()), "w_bf16 is not the bf16 rounding of w"


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("with_ema", [False, True])
@pytest.mark.parametrize("with_wb", [False, True])
@pytest.mark.parametrize("g_bf16", [False, True])
@pytest.mark.parametrize("n", [4, 1020])
def test_adamw(hip, n, g_bf16, with_wb, with_ema, skip):
    run_adamw(hip, n, g_bf16, with_wb, with_ema, skip)


# adamw_kernel's grid is capped like sgd_momentum_kernel's (8192 x 256 threads), so SGD_N["pair-first"]
# is also the first size at which its first thread enters the two-groups-in-flight loop
@pytest.mark.parametrize("g_bf16,with_wb,with_ema,skip", [
    (False, True, False, 0), (True, False, False, 0), (True, True, True, 0), (False, False, True, 0),
    (False, True, True, 1)])
def test_adamw_capped_grid(hip, g_bf16, with_wb, with_ema, skip):
    run_adamw(hip, kc.SGD_N["pair-first"], g_bf16, with_wb, with_ema, skip)


def test_adamw_rejects_a_length_not_a_multiple_of_4(hip):
    lr, bc, _ = _dev_scalars()
    w, m, v, g = (torch.zeros(6, device="cuda") for _ in range(4))
    with pytest.raises(KernelLibraryError):
        hip.adamw(w, m, v, g, None, lr, bc, *ARGS)


# -- 9. / 10. lamb ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs():
    """w, m, v, g (fp64, CPU) over the slot list of tests/test_lars_gpu.py, drawn once, never modified."""
    return hand_adam_buffers(TOTAL, SLOTS)


@pytest.fixture(scope="module")
def oracle(inputs):
    """RefBackend.lamb in fp64 for the fp32 gradient and for the bf16-rounded gradient."""
    w0, m0, v0, g0 = inputs
    be, out = RefBackend("cpu", dtype=torch.float64), {}
    table = LarsTable(SLOTS)
    bc = torch.tensor([kr.f32(HP["c1"]), kr.f32(HP["c2"])], dtype=torch.float64)
    lr = torch.tensor([kr.f32(HP["lr"])], dtype=torch.float64)
    for key, g in (("fp32", g0.float().double()), ("bf16", g0.bfloat16().double())):
        w, m, v, trust = w0.float().double(), m0.float().double(), v0.float().double(), torch.zeros(table.n)
        be.lamb(w, m, v, g, None, table, 0, table.n, None, trust, lr, bc, *(kr.f32(x) for x in ARGS))
        out[key] = (w, m, v, trust)
    RefBackend("cpu")  # (the process-wide reference dtype back to fp32)
    return out


def _inside():
    inside = torch.zeros(TOTAL, dtype=torch.bool)
    for off, n, _, _ in SLOTS:
        inside[off:off + n] = True
    return inside


class Dev:
    """Device copies of the inputs + workspaces; run() applies slots [first, first + n)."""

    def __init__(self, inputs, wire="fp32", skip=None, ema=False):
        w0, m0, v0, g0 = inputs
        self.table = LarsTable(SLOTS, "cuda")
        self.w, self.m, self.v = w0.float().cuda(), m0.float().cuda(), v0.float().cuda()
        self.g = g0.float().cuda() if wire == "fp32" else g0.bfloat16().cuda()
        gen = torch.Generator().manual_seed(77)
        self.wb = torch.randn(TOTAL, generator=gen).bfloat16().cuda()
        self.ema = torch.randn(TOTAL, generator=gen).cuda() if ema else None
        self.partials = torch.zeros(2 * self.table.chunks, device="cuda")
        self.trust = torch.full((self.table.n,), -1.0, device="cuda")
        self.lr, self.bc, self.decay = _dev_scalars()
        self.skip = None if skip is None else torch.tensor([skip], dtype=torch.int32, device="cuda")

    def run(self, hip, first=0, n=None):
        ema = {} if self.ema is None else dict(ema=self.ema, ema_decay_t=self.decay)
        hip.lamb(self.w, self.m, self.v, self.g, self.wb, self.table, first, self.table.n if n is None else n,
                 self.partials, self.trust, self.lr, self.bc, *ARGS, self.skip, **ema)
        torch.cuda.synchronize()
        return self

    def state(self):
        return [t.clone() for t in (self.w, self.m, self.v, self.wb, self.trust)]


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_lamb_matches_fp64_oracle(hip, inputs, oracle, wire):
    """trust within 1e-4 relative, w, m, v rel() < 1e-4, w_bf16 rel() < 4e-3 (the figures of
    test_lars_momentum_matches_fp64_oracle, the same reduction shape); padding inside slots and the
    gap between slots bitwise unchanged in all four buffers."""
    d = Dev(inputs, wire)
    before = [t.clone() for t in (d.w, d.m, d.v, d.wb)]
    d.run(hip)
    we, me, ve, te = oracle[wire]
    trust = d.trust.cpu().double()
    for i in range(d.table.n):
        print(f"slot {i}: trust hip {trust[i]:.9g} oracle {te[i]:.9g}")
        assert abs(trust[i] - te[i].double()) <= 1e-4 * abs(te[i].double()), i
    assert trust[1] == 1.0 and trust[4] == 1.0   # excluded / zero weights
    assert all(0 < float(trust[i]) < float("inf") and trust[i] != 1.0 for i in (0, 2, 5, 6))
    inside = _inside().cuda()
    ic = inside.cpu()
    figures = (rel(d.w[inside], we[ic]), rel(d.m[inside], me[ic]), rel(d.v[inside], ve[ic]),
               rel(d.wb[inside].float(), we[ic]))
    print("rel w, m, v, w_bf16:", figures)
    assert figures[0] < 1e-4 and figures[1] < 1e-4 and figures[2] < 1e-4 and figures[3] < 4e-3
    assert torch.equal(d.wb[inside], d.w[inside].bfloat16())
    for got, was in zip((d.w, d.m, d.v, d.wb), before):
        assert torch.equal(got[~inside], was[~inside])
        assert not torch.equal(got[inside], was[inside])


def test_lamb_is_deterministic_and_composes(hip, inputs):
    """Bitwise: the same call twice; one call over all slots vs three calls over consecutive slot
    sub-ranges; the EMA variant's w, m, v, w_bf16, trust vs the plain variant's; a non-zero skip word
    changes nothing, trust and the EMA included."""
    a, b = Dev(inputs).run(hip).state(), Dev(inputs).run(hip).state()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = Dev(inputs)
    c.run(hip, 0, 2).run(hip, 2, 3).run(hip, 5, 2)
    for x, y in zip(a, c.state()):
        assert torch.equal(x, y)
    e = Dev(inputs, ema=True)
    ema0 = e.ema.clone()
    e.run(hip)
    for x, y in zip(a, e.state()):
        assert torch.equal(x, y)
    # the EMA of the updated elements against its definition (bound: adam_refs.adamw_ref's, w exact here)
    inside = _inside().cuda()
    om = 1.0 - kr.f32(DECAY)
    df = ema0.double() - e.w.double()
    want = ema0.double() - om * df
    bound = (1 + 2.0 ** -10) * kr.U * (om * df.abs() + 2 * (om * df).abs() + ema0.double().abs() + (om * df).abs())
    kr.assert_within(e.ema[inside], want[inside].cpu(), bound[inside].cpu(), "lamb ema")
    assert torch.equal(e.ema[~inside], ema0[~inside])
    s = Dev(inputs, skip=1, ema=True)
    before, ema_before = s.state(), s.ema.clone()
    s.run(hip)
    for x, y in zip(before, s.state()):
        assert torch.equal(x, y)
    assert torch.equal(s.ema, ema_before) and float(s.trust[0]) == -1.0
    z = Dev(inputs, skip=0).run(hip)  # a zero skip word: the update runs
    for x, y in zip(a, z.state()):
        assert torch.equal(x, y)


# -- 11. executor step modes ------------------------------------------------------------------------------
def _hip_ex(opt, N=32, **kw):
    return fixed_batch_executor(opt, N=N, backend=HipBackend("cuda"), device="cuda", **kw)


def _snap(ex):
    torch.cuda.synchronize()
    return [t.clone() for t in (ex.P.master, ex.P.momentum, ex.P.adam_v)]


def _run_mode(ex, mode, steps=3):
    from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph
    from distributed_resnet_tensorflow_amd.runtime.plan import StepPlan
    fn = lambda: (ex.forward(True), ex.backward(defer_tail=mode != "joined"), ex.apply_gradients())  # noqa: E731

    def host(t):   # what train/session.py writes in front of every step
        ex.set_lr(TRAIN_LR[ex.optimizer] * (1 + t))
        ex.set_ema_decay(t)
        ex.set_adam_step(t)
    host(0)
    if mode in ("joined", "eager"):
        for t in range(steps):
            host(t)
            fn()
    else:
        runner = StepGraph(fn, warmup=1) if mode == "graph" else StepPlan(ex, warmup=1)   # (one eager step first)
        for t in range(1, steps):
            host(t)
            runner.replay()
    return _snap(ex)


@pytest.mark.parametrize("opt", ["adamw", "lamb"])
def test_eager_graph_and_plan_steps_are_bitwise_equal(monkeypatch, opt):
    """Three steps with a per-step LR and the per-step bias corrections: joined, deferred-tail eager
    (three update ranges), HIP graph and native plan leave bitwise equal master, m and v -- a
    replay must read the (c1, c2) the host wrote for its step, not those of the capture."""
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    monkeypatch.setenv("DRN_DEFER_TAIL", "1")
    outs = {}
    for mode in ("joined", "eager", "graph", "plan"):
        ex = _hip_ex(opt)
        assert ex._stem_hi == ex.stem_op.dw.numel() and ex.side is not None
        outs[mode] = _run_mode(ex, mode)
    assert bool(outs["joined"][2].abs().sum() > 0)
    for mode in ("eager", "graph", "plan"):
        for name, a, b in zip(("master", "momentum", "adam_v"), outs["joined"], outs[mode]):
            assert torch.equal(a, b), (mode, name)
    # a replay with the capture's corrections instead would differ: t = 1 vs t = 3 is 0.1 vs 0.271
    ex = _hip_ex(opt)
    assert ex.adam_bias_corrections(0) != ex.adam_bias_corrections(2)


@pytest.mark.parametrize("kw", [dict(clip_grad_norm=0.5), dict(ema_decay=0.9)], ids=["clip", "ema"])
@pytest.mark.parametrize("opt", ["adamw", "lamb"])
def test_eager_and_graph_agree_with_clip_and_ema(monkeypatch, opt, kw):
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    outs = {}
    for mode in ("eager", "graph"):
        ex = _hip_ex(opt, **kw)
        outs[mode] = _run_mode(ex, mode) + ([ex.P.ema.clone()] if "ema_decay" in kw else [])
        if "clip_grad_norm" in kw:
            st = ex.grad_guard_stats()
            assert st["steps_total"] == 3 and st["clipped_total"] >= 1 and st["skipped_total"] == 0
    for a, b in zip(outs["eager"], outs["graph"]):
        assert torch.equal(a, b)


# -- 12. the executor's update, teacher-forced ------------------------------------------------------------
@pytest.mark.parametrize("opt", ["adamw", "lamb"])
def test_executor_update_matches_the_oracle_on_its_own_gradient(opt):
    """One HIP forward + backward, then the HIP update against the fp64 update of the SAME gradient
    buffer and pre-step state (second update, so the moments are not zero): AdamW element by element
    within adamw_ref's bounds, LAMB with the figures of test_lamb_matches_fp64_oracle."""
    ex = _hip_ex(opt, N=16)
    ex.train_step(lr=TRAIN_LR[opt])          # (non-zero moments for the step under test)
    ex.P.global_step += 1
    ex.set_lr(TRAIN_LR[opt])
    ex.set_adam_step(1)
    ex.forward(True)
    ex.backward()
    torch.cuda.synchronize()
    P = ex.P
    g, w0, m0, v0 = (t.clone().cpu() for t in (P.grad, P.master, P.momentum, P.adam_v))
    bc = ex.adam_bc_t.cpu().double()
    ex.apply_gradients()
    torch.cuda.synchronize()
    lr = float(ex.lr_t.cpu()[0])
    if opt == "adamw":
        ref = adamw_ref(w0, m0, v0, g, lr, ex.adam_beta1, ex.adam_beta2, ex.adam_eps, ex.wd, 1.0, float(bc[0]),
                        float(bc[1]))
        for key, got in (("w", P.master), ("m", P.momentum), ("v", P.adam_v)):
            kr.assert_within(got, ref[key][0], ref[key][1], f"executor adamw {key}")
    else:
        be = RefBackend("cpu", dtype=torch.float64)
        from distributed_resnet_tensorflow_amd.ops.backend import lars_table
        table = lars_table(P, "cpu")
        w, m, v, trust = w0.double(), m0.double(), v0.double(), torch.zeros(table.n)
        be.lamb(w, m, v, g.double(), None, table, 0, table.n, None, trust, torch.tensor([lr], dtype=torch.float64), bc,
                *(kr.f32(x) for x in (ex.adam_beta1, ex.adam_beta2, ex.adam_eps, ex.wd)), 1.0)
        RefBackend("cpu")
        th = ex.lars_trust.cpu().double()
        assert bool(((th - trust.double()).abs() <= 1e-4 * trust.double().abs()).all())
        figures = (rel(P.master, w), rel(P.momentum, m), rel(P.adam_v, v))
        print("rel w, m, v:", figures)
        assert max(figures) < 1e-4
    assert torch.equal(P.wbf16, P.master.bfloat16())


# -- 13. training -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["adamw", "lamb"])
def test_training_halves_the_loss(opt):
    """30 steps on a fixed batch (cifar_resnet_v2(8), N = 32) at the constant LR picked on the oracle
    executor (adam_refs.TRAIN_LR): the loss at least halves."""
    ex = _hip_ex(opt)
    ex.forward(train=True)
    first = float(ex.loss_vec.double().mean())
    for _ in range(30):
        ex.train_step(lr=TRAIN_LR[opt])
        ex.P.global_step += 1
    ex.forward(train=True)
    final = float(ex.loss_vec.double().mean())
    print("loss", first, "->", final)
    assert final == final and final < first / 2, (first, final)
