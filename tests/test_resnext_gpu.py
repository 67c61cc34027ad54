"""ResNeXt-50 32x4d on the gfx950 kernels: every block against the fp32 reference executor, and a
training step replayed from a HIP graph / a native plan against the eager step."""
import pytest
import torch

from distributed_resnet_tensorflow_amd.models.spec import imagenet_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend, RefBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]


def _spec():
    # 64 px: stage 4 runs at 2x2, the smallest grid the grouped kernels see
    return imagenet_resnet_v2(50, num_classes=10, image_size=64, groups=32, width_per_group=4)


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return (a - b).norm().item() / max(b.norm().item(), 1e-12)


def test_every_block_teacher_forced():
    """The procedure and tolerances of test_executor_gpu.py::test_every_block_teacher_forced: each
    bottleneck (grouped 3x3 of width 4 / 8 / 16 / 32, stride 1 and 2) from the SAME bf16 block input and
    output gradient as the fp32 reference."""
    spec, N = _spec(), 8
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
        for c in bh.convs + ([bh.proj] if bh.proj else []):
            n = f"{c.conv.name}/kernel"
            errs.append((bi, n, rel(h.P.g(n), r.P.g(n)), 1e-1))
        for b in bh.bn:  # sums with cancellation: compare by direction
            for v in ("gamma", "beta"):
                n = f"{b.bn.name}/{v}"
                cos = torch.nn.functional.cosine_similarity(h.P.g(n).cpu(), r.P.g(n), dim=0).item()
                errs.append((bi, n, 1 - cos, 5e-3))
    bad = [e for e in errs if not e[2] < e[3]]
    assert not bad, bad


@pytest.mark.parametrize("mode", ["graph", "plan"])
def test_replayed_step_is_bitwise_the_eager_step(monkeypatch, mode):
    """DRN_DETERMINISTIC=1: one eager step + two replayed steps leave the bits of three eager steps, so
    the grouped launches are recorded and the weight gradient does not depend on execution order."""
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph
    from distributed_resnet_tensorflow_amd.runtime.plan import StepPlan

    def make():
        be = HipBackend()
        ex = Executor(_spec(), 4, be, "cuda", seed=3, weight_decay=1e-4)
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
    if mode == "graph":
        runner = StepGraph(lambda: step(b), warmup=1)   # (one eager step, then the capture)
    else:
        runner = StepPlan(b, warmup=1)
        assert runner.launches > 300, runner.launches
    for _ in range(2):
        runner.replay()
    for name, x, y in zip(("master", "momentum", "bn_state", "wbf16"), state(b), want):
        assert torch.equal(x, y), name
