"""Weight EMA on the GPU: the EMA variants of the optimizer kernels (csrc/kernels/sgd.hip
sgd_momentum_ema_kernel / lars_update_ema_kernel) against the plain entry points and an fp64
formula, the executor's eager / graph / plan / deferred-tail steps, and a CLI train -> eval run.

EMA bound (per update): |ema - ref64| <= 2^-21 * max(|ema_prev|, |w_new|), ref64 = the formula
ema_prev - (1 - d) * (ema_prev - w_new) in float64 from the fp32 ema_prev, the fp32 d and the kernel's
own w_new: three fp32 roundings (the difference, the product, the final subtraction; two with FMA
contraction) on operands of at most 2 * max, each at most 2^-24 * 2 * max."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from distributed_resnet_tensorflow_amd.models.spec import cifar_resnet_v2, imagenet_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import LARS_CHUNK, HipBackend, LarsTable
from distributed_resnet_tensorflow_amd.runtime.executor import Executor

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = dict(lr=0.3, mu=0.9, wd=2e-4, gs=0.5, eta=0.001, eps=1e-9)
DECAY = 0.999
EMA_EPS = 2.0 ** -21


def ema_check(ema, ema_prev, w_new, d32, where=slice(None)):
    """Asserts the bound of the module docstring on ema[where]; returns the largest error / bound."""
    e0, w = ema_prev[where].double(), w_new[where].double()
    ref = e0 - (1.0 - float(d32)) * (e0 - w)
    err = (ema[where].double() - ref).abs()
    bound = EMA_EPS * torch.maximum(e0.abs(), w.abs())
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"ema: max |err| {float(err.max()):.3e}, max err / bound {worst:.3f}")
    assert bool((err <= bound).all()), worst
    return worst


def _buffers(n, wire, seed=5):
    gen = torch.Generator().manual_seed(seed)
    w, m, g, e = (torch.randn(n, generator=gen).cuda() for _ in range(4))
    if wire == "bf16":
        g = g.bfloat16()
    wb = torch.randn(n, generator=gen).bfloat16().cuda()
    return w, m, g, wb, e


# n = 4: one float4 group; 4 * 257: ends in a partial block; the last: the grid caps at 8192 x 256
# threads, so only above 2,097,152 float4 groups does the two-in-flight loop run (here: loop + tail)
MOMENTUM_SIZES = [4, 4 * 257, 4 * (2 * 2097152 + 300)]


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
@pytest.mark.parametrize("n", MOMENTUM_SIZES)
def test_momentum_ema_kernel(hip, n, wire):
    lr = torch.tensor([HP["lr"]], device="cuda")
    d = torch.tensor([DECAY], device="cuda")
    w0, m0, g, wb0, e0 = _buffers(n, wire)
    # the plain entry point on the same inputs
    w1, m1, wb1 = w0.clone(), m0.clone(), wb0.clone()
    hip.sgd_momentum(w1, m1, g, wb1, lr, HP["mu"], HP["wd"], HP["gs"])
    w2, m2, wb2, e2 = w0.clone(), m0.clone(), wb0.clone(), e0.clone()
    hip.sgd_momentum(w2, m2, g, wb2, lr, HP["mu"], HP["wd"], HP["gs"], None, ema=e2, ema_decay_t=d)
    torch.cuda.synchronize()
    assert torch.equal(w1, w2) and torch.equal(m1, m2) and torch.equal(wb1, wb2)
    assert not torch.equal(w2, w0) and not torch.equal(e2, e0)
    ema_check(e2, e0, w2, d.cpu()[0])
    # skip word set: nothing moves; clear: the update runs
    for word, moves in ((1, False), (0, True)):
        w3, m3, wb3, e3 = w0.clone(), m0.clone(), wb0.clone(), e0.clone()
        skip = torch.tensor([word], dtype=torch.int32, device="cuda")
        hip.sgd_momentum(w3, m3, g, wb3, lr, HP["mu"], HP["wd"], HP["gs"], skip, ema=e3, ema_decay_t=d)
        torch.cuda.synchronize()
        for got, before, after in ((w3, w0, w2), (m3, m0, m2), (e3, e0, e2), (wb3, wb0, wb2)):
            assert torch.equal(got, after if moves else before)


def test_momentum_ema_reads_the_decay_from_device_memory(hip):
    """The same call with another value in the device scalar gives that value's average."""
    n = 4 * 257
    lr = torch.tensor([HP["lr"]], device="cuda")
    d = torch.tensor([0.1], device="cuda")
    for value in (0.1, 0.5):
        w, m, g, wb, e = _buffers(n, "fp32")
        e0 = e.clone()
        d.fill_(value)
        hip.sgd_momentum(w, m, g, wb, lr, HP["mu"], HP["wd"], HP["gs"], None, ema=e, ema_decay_t=d)
        torch.cuda.synchronize()
        ema_check(e, e0, w, d.cpu()[0])


# a 10-element non-adapting slot (scalar tail), a slot of exactly one chunk, an adapting slot of two
# chunks + one float4 group + a 3-element scalar tail
LARS_SLOTS = [(0, 10, 16, 0), (16, LARS_CHUNK, LARS_CHUNK, 1),
              (16 + LARS_CHUNK, 2 * LARS_CHUNK + 4 + 3, 2 * LARS_CHUNK + 16, 1)]
LARS_TOTAL = 16 + LARS_CHUNK + 2 * LARS_CHUNK + 16


def _lars(hip, bufs, table, skip=None, ema=None, d=None, first=0, n=None):
    w, m, g, wb = bufs
    partials = torch.zeros(2 * table.chunks, device="cuda")
    trust = torch.full((table.n,), -1.0, device="cuda")
    hip.lars_momentum(w, m, g, wb, table, first, table.n if n is None else n, partials, trust,
                      torch.tensor([HP["lr"]], device="cuda"), HP["mu"], HP["wd"], HP["gs"], HP["eta"], HP["eps"], skip,
                      ema=ema, ema_decay_t=d)
    torch.cuda.synchronize()
    return trust


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_lars_ema_kernel(hip, wire):
    assert LARS_CHUNK == 8192
    table = LarsTable(LARS_SLOTS, "cuda")
    d = torch.tensor([DECAY], device="cuda")
    w0, m0, g, wb0, e0 = _buffers(LARS_TOTAL, wire, seed=6)
    inside = torch.zeros(LARS_TOTAL, dtype=torch.bool, device="cuda")
    for off, n, _, _ in LARS_SLOTS:
        inside[off:off + n] = True
    w1, m1, wb1 = w0.clone(), m0.clone(), wb0.clone()
    t1 = _lars(hip, (w1, m1, g, wb1), table)
    w2, m2, wb2, e2 = w0.clone(), m0.clone(), wb0.clone(), e0.clone()
    t2 = _lars(hip, (w2, m2, g, wb2), table, ema=e2, d=d)
    assert torch.equal(w1, w2) and torch.equal(m1, m2) and torch.equal(wb1, wb2) and torch.equal(t1, t2)
    assert float(t2[0]) == 1.0 and 0 < float(t2[1]) < 1 and 0 < float(t2[2]) < 1
    ema_check(e2, e0, w2, d.cpu()[0], inside)
    assert torch.equal(e2[~inside], e0[~inside])            # padding between slots is left alone
    assert not bool((e2[inside] == e0[inside]).all())
    # a sub-range of slots averages only those slots
    w4, m4, wb4, e4 = w0.clone(), m0.clone(), wb0.clone(), e0.clone()
    _lars(hip, (w4, m4, g, wb4), table, ema=e4, d=d, first=1, n=1)
    lo, hi = LARS_SLOTS[1][0], LARS_SLOTS[1][0] + LARS_SLOTS[1][1]
    assert torch.equal(e4[lo:hi], e2[lo:hi]) and torch.equal(e4[:lo], e0[:lo]) and torch.equal(e4[hi:], e0[hi:])
    # skip word set: w, m, ema (and wb, trust) bit for bit unchanged
    w3, m3, wb3, e3 = w0.clone(), m0.clone(), wb0.clone(), e0.clone()
    t3 = _lars(hip, (w3, m3, g, wb3), table, skip=torch.tensor([1], dtype=torch.int32, device="cuda"), ema=e3, d=d)
    for got, before in ((w3, w0), (m3, m0), (e3, e0), (wb3, wb0)):
        assert torch.equal(got, before)
    assert float(t3[0]) == -1.0


# -- executor ------------------------------------------------------------------------------------------
def _ex(spec, N, seed=3, data_seed=9, lr=0.05, **kw):
    ex = Executor(spec, N, HipBackend("cuda"), "cuda", seed=seed, **kw)
    g = torch.Generator().manual_seed(data_seed)
    ex.images.zero_()
    ex.images[..., :3] = torch.randn(N, spec.image_size, spec.image_size, 3, generator=g).bfloat16().cuda()
    ex.labels.copy_(torch.randint(0, spec.num_classes, (N,), generator=g, dtype=torch.int32))
    ex.set_lr(lr)
    return ex


def _snap(ex, *names):
    torch.cuda.synchronize()
    return [getattr(ex.P, n).clone() for n in names]


def test_eager_graph_and_plan_read_each_steps_decay(monkeypatch):
    """Three steps with warm-up (d_t = 0.1, 2/11, 3/12): a replayed graph / plan must average with
    the decay the host wrote for the step, not the one of its capture."""
    from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph
    from distributed_resnet_tensorflow_amd.runtime.plan import StepPlan
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    spec, N = cifar_resnet_v2(8), 8
    out = {}
    for mode in ("eager", "graph", "plan"):
        ex = _ex(spec, N, ema_decay=DECAY)
        assert torch.equal(ex.P.ema, ex.P.master)
        fn = lambda: (ex.forward(True), ex.backward(defer_tail=True), ex.apply_gradients())  # noqa: E731
        ex.set_ema_decay(0)
        if mode == "eager":
            # every step against the formula, from the device's own previous average and new weights
            # ... and a host fp32 replay of the whole recurrence over the per-step weights: each side
            # adds at most the per-update bound to an error that the update scales by d_t < 1
            host = ex.P.ema.cpu().clone()
            slack = torch.zeros_like(host, dtype=torch.float64)
            for t in range(3):
                ex.set_ema_decay(t)
                prev, = _snap(ex, "ema")
                fn()
                ema, w = _snap(ex, "ema", "master")
                d32 = ex.ema_decay_t.cpu()[0]
                assert float(d32) == float(torch.tensor(min(DECAY, (1 + t) / (10 + t)), dtype=torch.float32))
                ema_check(ema, prev, w, d32)
                step_bound = EMA_EPS * torch.maximum(host.abs().double() + slack, w.cpu().abs().double())
                slack = float(d32) * slack + 2 * step_bound
                host = host - (1 - d32) * (host - w.cpu())
            assert bool(((ema.cpu().double() - host.double()).abs() <= slack).all())
        elif mode == "graph":
            g = StepGraph(fn, warmup=1)        # (one eager step, then the capture)
            for t in (1, 2):
                ex.set_ema_decay(t)
                g.replay()
        else:
            plan = StepPlan(ex, warmup=1)
            for t in (1, 2):
                ex.set_ema_decay(t)
                plan.replay()
        out[mode] = _snap(ex, "ema", "master", "momentum", "bn_state")
    assert not torch.equal(out["eager"][0], out["eager"][1])
    for mode in ("graph", "plan"):
        for name, a, b in zip(("ema", "master", "momentum", "bn_state"), out["eager"], out[mode]):
            assert torch.equal(a, b), (mode, name)


def test_ema_off_allocates_nothing_and_ema_on_leaves_training_alone(monkeypatch):
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    spec, N = cifar_resnet_v2(8), 8
    out = {}
    for decay in (0.0, DECAY):
        ex = _ex(spec, N, ema_decay=decay)
        assert (ex.P.ema is None) == (decay == 0.0)
        for t in range(3):
            ex.P.global_step = t
            ex.train_step()
        out[decay] = _snap(ex, "master", "momentum", "bn_state")
    for name, a, b in zip(("master", "momentum", "bn_state"), out[0.0], out[DECAY]):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("optimizer", ["momentum", "lars"])
def test_deferred_tail_updates_carry_their_ema_range(monkeypatch, optimizer):
    """ImageNet-style stem with DRN_DEFER_TAIL=1: the split updates [lo:), [hi:lo), [0:hi) each
    average their own range -- bitwise the joined step's P.ema; training state as without EMA."""
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    monkeypatch.setenv("DRN_DEFER_TAIL", "1")
    spec, N = imagenet_resnet_v2(18, num_classes=10, image_size=64), 8
    out = {}
    for mode, decay in (("joined", DECAY), ("deferred", DECAY), ("deferred_off", 0.0)):
        ex = _ex(spec, N, optimizer=optimizer, ema_decay=decay, lr=0.5 if optimizer == "lars" else 0.05)
        assert ex._stem_hi == ex.stem_op.dw.numel() > 0 and ex.side is not None and ex.early_sgd
        for t in range(3):
            ex.set_ema_decay(t)
            ex.forward(True)
            ex.backward(defer_tail=mode != "joined")
            assert (ex._tail_ev is not None) == (mode != "joined")
            ex.apply_gradients()
        out[mode] = _snap(ex, "master", "momentum", "bn_state") + (_snap(ex, "ema") if decay else [])
    for name, a, b in zip(("master", "momentum", "bn_state", "ema"), out["joined"], out["deferred"]):
        assert torch.equal(a, b), name
    for name, a, b in zip(("master", "momentum", "bn_state"), out["deferred"], out["deferred_off"]):
        assert torch.equal(a, b), name
    ema, master = out["deferred"][3], out["deferred"][0]
    sl = ex.P.slots
    for s in (sl[0], sl[1], sl[-1]):      # the stem (updated last), the first block, the dense bias
        assert not torch.equal(ema[s.offset:s.offset + s.numel], master[s.offset:s.offset + s.numel]), s.name


# -- CLI -----------------------------------------------------------------------------------------------
def _run(args, timeout=280):
    e = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-u"] + args, cwd=REPO, capture_output=True, text=True, timeout=timeout, env=e)
    assert r.returncode == 0, (args[0], r.stdout[-4000:], r.stderr[-4000:])
    return r.stdout + r.stderr


def test_cli_train_with_ema_then_eval_plain_and_eval_ema(tmp_path):
    from distributed_resnet_tensorflow_amd import cli
    from distributed_resnet_tensorflow_amd.ckpt.saver import Saver, latest_checkpoint
    from distributed_resnet_tensorflow_amd.data.cifar import write_fake_cifar
    from distributed_resnet_tensorflow_amd.parallel.cluster import ClusterInfo
    from distributed_resnet_tensorflow_amd.runtime.state import EMA_SUFFIX, import_state
    from distributed_resnet_tensorflow_amd.train.trainer import make_feeder
    data = str(tmp_path / "data")
    write_fake_cifar(data, 200, learnable=True)
    ck = str(tmp_path / "ck")
    out = _run(["resnet_cifar_main.py", "--num_gpus=1", f"--train_data_path={data}", f"--log_root={ck}",
                "--resnet_size=8", "--batch_size=32", "--train_steps=40", "--log_every_n_steps=20",
                "--ema_decay=0.9"])
    assert "global step 40" in out, out[-2000:]
    prefix = latest_checkpoint(ck)
    t = Saver.restore(prefix)
    assert json.load(open(prefix + ".meta"))["ema_decay"] == 0.9
    names = [k for k in t if k + "/Momentum" in t]
    assert names and all(k + EMA_SUFFIX in t for k in names)
    assert any(not (t[k] == t[k + EMA_SUFFIX]).all() for k in names)
    common = ["resnet_cifar_eval.py", "--mode=eval", "--eval_once=True", "--num_gpus=1",
              f"--eval_data_path={data}/cifar-10-batches-bin/test_batch*", f"--log_root={ck}", "--resnet_size=8",
              "--eval_batch_count=2"]
    prec = {}
    for name, extra in (("plain", []), ("ema", ["--eval_ema=True"])):
        out = _run(common + [f"--eval_dir={tmp_path}/ev_{name}"] + extra)
        m = re.findall(r"precision: ([0-9.]+), best precision", out)
        assert m, out[-2000:]
        prec[name] = json.load(open(tmp_path / f"ev_{name}" / "best_precision.json"))
    assert prec["ema"]["ema"] is True and "ema" not in prec["plain"] and prec["ema"]["step"] == 40
    # an executor loaded with the EMA tensors, over the same two batches of 100
    ex = Executor(cifar_resnet_v2(8), 100, HipBackend("cuda"), "cuda")
    import_state(ex, {k: (t[k + EMA_SUFFIX] if k + EMA_SUFFIX in t else v) for k, v in t.items()})
    F = cli.entry_flags("cifar_eval_main", [f"--eval_data_path={data}/cifar-10-batches-bin/test_batch*"])
    feeder = make_feeder(F, ex, ClusterInfo(device="cuda"), False, batch=100)
    correct = 0
    try:
        for _ in range(2):
            assert feeder.next()
            ex.forward(train=False)
            correct += int(ex.correct.sum())
    finally:
        feeder.close()
    assert prec["ema"]["best_precision"] == correct / 200
