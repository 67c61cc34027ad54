"""Squeeze-and-Excitation on the gfx950 kernels (csrc/kernels/se.hip): every kernel per element against
fp64 (tests/se_refs.py), every SE block against the fp32 reference executor, and a training step replayed
from a HIP graph / a native plan against the eager step."""
import functools

import pytest
import torch

import se_refs as sr
from kernel_refs import assert_within, conv_stats
from distributed_resnet_tensorflow_amd.models.spec import cifar_resnet_v2, imagenet_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend, RefBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

# (N, H, W, C, r): N below / at / above a 16-row tile; one pixel, an odd plane, the shortest pixel row
# (32 bytes), the widest gate (Cr = 128), the longest reduction with S > 1
CASES = [(3, 1, 1, 16, 4), (5, 7, 7, 64, 16), (17, 2, 2, 2048, 16), (2, 56, 56, 256, 16), (16, 8, 8, 32, 4)]
cases = pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))


@functools.lru_cache(maxsize=None)
def _run(case):
    """One forward and one backward chain of the six kernels on the GPU; every tensor each kernel read or
    wrote, on the CPU. Outputs are prefilled with NaN."""
    N, H, W, C, r = case
    Cr, hw = max(C // r, 8), H * W
    g = torch.Generator().manual_seed(sum(case))
    rn = lambda *sh: torch.randn(*sh, generator=g)
    t = {"u": (rn(N, H, W, C) + rn(N, 1, 1, C)).bfloat16(), "sc": rn(N, H, W, C).bfloat16(),
         "g": rn(N, H, W, C).bfloat16(),
         # z ~ N(0, 1): l1 ~ N(0, 2), E h^2 ~ 1, pre-sigmoid std ~ 1.5: s spans (0.1, 0.9)
         "w1": rn(C, Cr) * (2.0 / C) ** 0.5, "b1": 0.1 * rn(Cr), "w2": rn(Cr, C) * 1.5 / Cr ** 0.5, "b2": 0.1 * rn(C)}
    be = HipBackend()
    S = be.se_splits(N, hw, C)
    nan = lambda *sh, dt=torch.float32: torch.full(sh, float("nan"), dtype=dt, device="cuda")
    d = {k: v.cuda() for k, v in t.items()}
    for k, sh in (("cells", (N, S, C)), ("dcells", (N, S, C)), ("z", (N, C)), ("h", (N, Cr)), ("s", (N, C)),
                  ("dl2", (N, C)), ("dh", (N, Cr)), ("dzs", (N, C)), ("dw1", (C, Cr)), ("db1", (Cr,)),
                  ("dw2", (Cr, C)), ("db2", (C,))):
        d[k] = nan(*sh)
    d["out"], d["du"] = nan(N, H, W, C, dt=torch.bfloat16), nan(N, H, W, C, dt=torch.bfloat16)
    d["stats"] = torch.zeros(8, 2, C, device="cuda")
    be.se_squeeze(d["u"], d["cells"])
    be.se_gate_fwd(d["cells"], hw, d["w1"], d["b1"], d["w2"], d["b2"], d["z"], d["h"], d["s"])
    be.se_excite(d["u"], d["sc"], d["s"], d["out"], stats=d["stats"])
    be.se_squeeze(d["u"], d["dcells"], g=d["g"])
    be.se_gate_bwd(d["dcells"], hw, d["w1"], d["w2"], d["h"], d["s"], d["dl2"], d["dh"], d["dzs"])
    be.se_gate_wgrad(d["z"], d["h"], d["dl2"], d["dh"], d["dw1"], d["db1"], d["dw2"], d["db2"])
    be.se_scale_bwd(d["g"], d["s"], d["dzs"], d["du"])
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}, hw, S


def _within(d, names, refs, what):
    for n, (ref, bound) in zip(names, refs):
        assert_within(d[n], ref, bound, f"{what}: {n}")


@cases
def test_squeeze(case):
    d, _, S = _run(case)
    assert S > 1 or case[1] < 56
    for cells, g in (("cells", None), ("dcells", d["g"])):
        ref, bound = sr.squeeze(d["u"], g, S)
        assert_within(d[cells].double().sum(1), ref, bound, f"se_squeeze: {cells}")


@cases
def test_gate_fwd(case):
    d, hw, _ = _run(case)
    _within(d, "zhs", sr.gate_fwd(d["cells"], hw, d["w1"], d["b1"], d["w2"], d["b2"]), "se_gate_fwd")
    assert d["s"].quantile(0.1) < 0.4 and d["s"].quantile(0.9) > 0.6   # (the gate is not sitting at 0.5)


@cases
def test_excite_and_statistics(case):
    d, _, _ = _run(case)
    assert_within(d["out"], *sr.scale_add(d["s"], d["u"], d["sc"].double()), "se_excite: out")
    assert_within(d["stats"].double().sum(0), *conv_stats(d["out"], 8), "se_excite: stats")


@cases
def test_gate_bwd(case):
    d, hw, _ = _run(case)
    _within(d, ("dl2", "dh", "dzs"), sr.gate_bwd(d["dcells"], hw, d["w1"], d["w2"], d["h"], d["s"]), "se_gate_bwd")


@cases
def test_gate_wgrad(case):
    d, _, _ = _run(case)
    _within(d, ("dw1", "db1", "dw2", "db2"), sr.gate_wgrad(d["z"], d["h"], d["dl2"], d["dh"]), "se_gate_wgrad")


@cases
def test_scale_bwd(case):
    d, _, _ = _run(case)
    assert_within(d["du"], *sr.scale_add(d["s"], d["g"], d["dzs"].double()[:, None, None, :]), "se_scale_bwd: du")


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return (a - b).norm().item() / max(b.norm().item(), 1e-12)


SPECS = {"cifar8_r4": lambda: cifar_resnet_v2(8, se_ratio=4),   # basic blocks, C = 16 / 32 / 64
         # SE-ResNeXt bottlenecks, C = 256 .. 2048, planes 16^2 .. 2^2
         "se_resnext50": lambda: imagenet_resnet_v2(50, 10, image_size=64, groups=32, width_per_group=4, se_ratio=16)}


@pytest.mark.parametrize("name", list(SPECS))
def test_every_block_teacher_forced(name):
    """The procedure and tolerances of test_resnext_gpu.py::test_every_block_teacher_forced, + the four SE
    gradients of each block (kernels 1e-1, biases by direction)."""
    spec, N = SPECS[name](), 8
    torch.manual_seed(0)
    h = Executor(spec, N, HipBackend(), "cuda", seed=5)
    r = Executor(spec, N, RefBackend(), "cpu", seed=5)
    for ex in (h, r):
        ex.P.master.copy_(h.P.master.cpu().bfloat16().float().to(ex.device))
        ex.sync_weights()
    errs = []
    for bi, (bh, br) in enumerate(zip(h.blocks, r.blocks)):
        x = (torch.randn(bh.x.shape) * 2 + 0.3).bfloat16()
        dout = (torch.randn(bh.out.shape) * 0.1).bfloat16()
        for ex, bp in ((h, bh), (r, br)):
            bp.x.copy_(x.to(ex.device, bp.x.dtype))
            ex.be.zero_(bp.bn[0].stats)
            ex.be.bn_stats(bp.x, bp.bn[0].stats)
            ex._block_fwd(bp, train=True)
            bufs = [ex.g_a, ex.g_b, ex.g_c]
            ex._view(bufs[0], bp.out).copy_(dout.to(ex.device, bp.out.dtype))
            bp._din = ex._view(bufs[ex._block_bwd(bp, bufs, 0)], bp.x)
            if bp is bh:
                ex.be.zero_(bp.out_stats)
        torch.cuda.synchronize()
        errs.append((bi, "out", rel(bh.out, br.out), 2e-2))
        errs.append((bi, "din", rel(bh._din, br._din), 1e-1))
        e = bh.blk.se.name
        for n in [f"{c.conv.name}/kernel" for c in bh.convs + ([bh.proj] if bh.proj else [])] + \
                [f"{e}/reduce/kernel", f"{e}/expand/kernel"]:
            errs.append((bi, n, rel(h.P.g(n), r.P.g(n)), 1e-1))
        for n in [f"{b.bn.name}/{v}" for b in bh.bn for v in ("gamma", "beta")] + [f"{e}/reduce/bias", f"{e}/expand/bias"]:
            cos = torch.nn.functional.cosine_similarity(h.P.g(n).cpu(), r.P.g(n), dim=0).item()
            errs.append((bi, n, 1 - cos, 5e-3))   # sums with cancellation: compare by direction
    bad = [e for e in errs if not e[2] < e[3]]
    assert not bad, bad


@pytest.mark.parametrize("mode", ["graph", "plan"])
def test_replayed_step_is_bitwise_the_eager_step(monkeypatch, mode):
    """DRN_DETERMINISTIC=1: one eager step + two replayed steps leave the bits of three eager steps (the
    procedure of test_resnext_gpu.py): every SE launch is recorded, no result depends on execution order."""
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph
    from distributed_resnet_tensorflow_amd.runtime.plan import StepPlan

    def make():
        be = HipBackend()
        ex = Executor(SPECS["cifar8_r4"](), 4, be, "cuda", seed=3, weight_decay=1e-4)
        be.synthetic_images(ex.images, seed=9)
        ex.labels.copy_(torch.arange(4, dtype=torch.int32))
        ex.set_lr(0.02)
        return ex

    def state(ex):
        torch.cuda.synchronize()
        return [t.clone() for t in (ex.P.master, ex.P.momentum, ex.P.bn_state, ex.P.wbf16)]
    step = lambda ex: (ex.forward(train=True), ex.backward(defer_tail=True), ex.apply_gradients())  # noqa: E731
    a = make()
    for _ in range(3):
        step(a)
    want = state(a)
    b = make()
    runner = StepGraph(lambda: step(b), warmup=1) if mode == "graph" else StepPlan(b, warmup=1)
    for _ in range(2):
        runner.replay()
    for name, x, y in zip(("master", "momentum", "bn_state", "wbf16"), state(b), want):
        assert torch.equal(x, y), name
