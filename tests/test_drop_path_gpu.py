"""Stochastic depth on the gfx950 kernels (csrc/kernels/drop_path.hip): both kernels per element against fp64, a
training step against the autograd oracle with the same table, the rate-0 no-op, replays that follow the table."""
import functools

import pytest
import torch

from distributed_resnet_tensorflow_amd.models import oracle
from distributed_resnet_tensorflow_amd.models.spec import cifar_resnet_v2, imagenet_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor
from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph
from distributed_resnet_tensorflow_amd.runtime.plan import StepPlan

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

# (N, H = W, C): an odd pixel count; 9 chunks per pixel and two pixel splits of 41 + 40; one pixel, 8 slabs
SHAPES = [(3, 5, 16), (4, 9, 72), (2, 1, 2048)]
FACTORS = [1.0, 0.0, 1 / (1 - 0.5), 1 / (1 - 0.2)]   # sample n of row r gets FACTORS[(n + r) % 4]
cases = pytest.mark.parametrize("case", [s + (r,) for s in SHAPES for r in (0, 1)], ids=lambda c: "x".join(map(str, c)))


@functools.lru_cache(maxsize=None)
def _case(case):
    """Both kernels once (outputs prefilled with NaN; u and d_out NaN on dropped samples); every tensor on the CPU."""
    N, H, C, r = case
    g = torch.Generator().manual_seed(sum(case))
    f = torch.tensor([FACTORS[(n + r) % 4] for n in range(N)])
    t = {k: torch.randn(N, H, H, C, generator=g).bfloat16() for k in ("u", "sc", "g")}
    t["u"][f == 0] = t["g"][f == 0] = float("nan")
    d = {**{k: v.cuda() for k, v in t.items()}, "f": f.cuda()}
    for k in ("out", "du"):
        d[k] = torch.full((N, H, H, C), float("nan"), dtype=torch.bfloat16, device="cuda")
    d["stats"], d["inplace"] = torch.zeros(8, 2, C, device="cuda"), d["sc"].clone()
    be = HipBackend()
    be.drop_path_fwd(d["u"], d["sc"], d["f"], d["out"], stats=d["stats"])
    be.drop_path_fwd(d["u"], d["inplace"], d["f"], d["inplace"])   # out IS the shortcut buffer
    be.drop_path_bwd(d["g"], d["f"], d["du"])
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}, be.drop_path_splits(N, H * H, C)


@cases
def test_forward_add_and_statistics(case):
    d, splits = _case(case)
    assert (splits > 1) == (case[:3] == (4, 9, 72))
    f, out, drop = d["f"], d["out"], d["f"] == 0
    assert drop.any() and (~drop).any() and not out.isnan().any()
    assert torch.equal(out[drop].view(torch.int16), d["sc"][drop].view(torch.int16))
    assert torch.equal(d["inplace"].view(torch.int16), out.view(torch.int16))
    fu = (f.double()[:, None, None, None] * d["u"].double())[~drop]
    sc = d["sc"].double()[~drop]
    err = (out.double()[~drop] - (sc + fu)).abs()
    assert (err <= 2.0 ** -8 * (sc + fu).abs() + 2.0 ** -22 * (sc.abs() + fu.abs())).all(), err.max()
    ys = out.double().reshape(-1, out.shape[-1])
    got = d["stats"].double().sum(0)
    for which, terms in enumerate((ys, ys * ys)):
        assert ((got[which] - terms.sum(0)).abs() <= ys.shape[0] * 2.0 ** -24 * terms.abs().sum(0)).all(), which


@cases
def test_backward_branch_gradient(case):
    d, _ = _case(case)
    drop = d["f"] == 0
    assert (d["du"][drop] == 0).all() and not d["du"].isnan().any()
    ref = (d["f"].double()[:, None, None, None] * d["g"].double())[~drop]
    assert ((d["du"].double()[~drop] - ref).abs() <= 2.0 ** -8 * ref.abs()).all()


def _table(rates, N, shift=0):
    """Every sample kept and scaled, but sample (b + shift) % N of each dropping block b."""
    t = torch.ones(len(rates), N)
    for b, p in enumerate(rates):
        if p > 0:
            t[b] = 1 / (1 - p)
            t[b, (b + shift) % N] = 0.0
    return t


NETS = {"cifar14": lambda: cifar_resnet_v2(14, drop_path_rate=0.5),
        # (128 px: where test_step_matches_reference's bounds hold; at 64 px the net WITHOUT the flag misses them)
        "in50_avgdown": lambda: imagenet_resnet_v2(50, num_classes=10, image_size=128, avg_down=True, drop_path_rate=0.5)}


@pytest.mark.parametrize("which", list(NETS))
def test_step_matches_the_oracle_with_the_same_table(which):
    """The comparisons and bounds of test_executor_gpu.py::test_step_matches_reference."""
    spec, N = NETS[which](), 8
    torch.manual_seed(0)
    h = Executor(spec, N, HipBackend(), "cuda", seed=5)
    h.P.master.copy_(h.P.master.bfloat16().float())
    h.sync_weights()
    imgs = torch.randn(N, spec.image_size, spec.image_size, 3).bfloat16().float()
    labels = torch.randint(0, spec.num_classes, (N,), dtype=torch.int32)
    table = _table(h.drop_rates, N)
    h.images.zero_()
    h.images[..., :3] = imgs.cuda()
    h.labels.copy_(labels.cuda())
    h.set_drop_path(table)
    p = {k: v.detach().cpu().requires_grad_() for k, v in oracle.params_from_store(h.P, False).items()}
    st = oracle.state_from_store(h.P)
    h.forward(train=True)
    h.backward()
    torch.cuda.synchronize()
    logits, xent, _ = oracle.loss_fn(spec, p, st, imgs, labels, drop_path=table)
    xent.backward()
    cos = torch.nn.functional.cosine_similarity
    grad = lambda n: h.P.to_tf(n, buf=h.P.grad, dtype=torch.float32).cpu()  # noqa: E731
    cosl = cos(h.logits.cpu().flatten(), logits.detach().flatten(), dim=0).item()
    slots = h.P.slots[-4:] if which != "cifar14" else h.P.slots
    cosg = {s.name: cos(grad(s.name).flatten(), p[s.name].grad.flatten(), dim=0).item() for s in slots}
    reld = {n: ((grad(n) - p[n].grad).norm() / p[n].grad.norm()).item() for n in ("dense/kernel", "dense/bias")}
    print(f"[{which}] logits cos {cosl:.4f}, least gradient cos {min(cosg.values()):.4f}, dense rel {reld}")
    assert cosl > 0.98 and abs(h.loss_vec.mean().item() - xent.item()) < 0.1
    assert all(c > 0.9 for c in cosg.values()), cosg
    assert all(r < (3e-2 if which == "cifar14" else 2e-1) for r in reld.values()), reld


def _make(**kw):
    be = HipBackend()
    ex = Executor(cifar_resnet_v2(8), 4, be, "cuda", seed=3, weight_decay=1e-4, **kw)
    be.synthetic_images(ex.images, seed=9)
    ex.labels.copy_(torch.arange(4, dtype=torch.int32))
    ex.set_lr(0.02)
    return ex


def _state(ex):
    torch.cuda.synchronize()
    return [t.clone() for t in (ex.P.master, ex.P.momentum, ex.P.bn_state, ex.P.wbf16)]


step = lambda ex: (ex.forward(train=True), ex.backward(defer_tail=True), ex.apply_gradients())  # noqa: E731


def test_rate_zero_is_a_no_op(monkeypatch):
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    exs = [_make(), _make(drop_path_rate=0.0)]
    assert exs[1].drop_table is None and exs[1].drop_u is None
    plans = [StepPlan(ex, warmup=1).stats() for ex in exs]   # (one eager step each, then its recording)
    assert plans[0] == plans[1] and all(torch.equal(x, y) for x, y in zip(_state(exs[0]), _state(exs[1])))


@pytest.mark.parametrize("mode", ["graph", "plan"])
def test_replays_follow_the_table(monkeypatch, mode):
    """A step recorded with one table and replayed with two others leaves the bits of three eager steps."""
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    a, b = _make(drop_path_rate=0.5), _make(drop_path_rate=0.5)
    tables = [_table(a.drop_rates, 4, shift) for shift in range(3)]
    for t in tables:
        a.set_drop_path(t)
        step(a)
    b.set_drop_path(tables[0])
    runner = StepGraph(lambda: step(b), warmup=1) if mode == "graph" else StepPlan(b, warmup=1)
    for t in tables[1:]:
        b.set_drop_path(t)
        runner.replay()
    assert all(torch.equal(x, y) for x, y in zip(_state(b), _state(a)))


def test_refusals():
    from distributed_resnet_tensorflow_amd import flags
    from distributed_resnet_tensorflow_amd.cli import entry_flags
    spec = cifar_resnet_v2(8, drop_path_rate=0.2)
    spec.blocks[1].out_c = 12   # (no builder makes such a net: the executor's build-time refusal alone)
    with pytest.raises(ValueError, match="stochastic depth.*HIP backend"):
        Executor(spec, 2, HipBackend(), "cuda")
    with pytest.raises(flags.FlagsError, match="se_ratio"):
        entry_flags("imagenet_main", ["--se_ratio=16", "--drop_path_rate=0.1"])
