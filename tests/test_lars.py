"""LARS optimizer and the warm-up / polynomial-decay LR policy: CPU tests (oracle backend, flags,
schedule, two-rank gloo run). The HIP kernels are covered by tests/test_lars_gpu.py."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from distributed_resnet_tensorflow_amd import cli
from distributed_resnet_tensorflow_amd.flags import FlagsError
from distributed_resnet_tensorflow_amd.models.spec import cifar_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import LARS_EXCLUDED, LarsTable, RefBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor
from distributed_resnet_tensorflow_amd.train import lr as lr_mod

# (offset, numel, padded, adapt): a 16-element adapting slot, a 10-in-16 excluded slot (a bias), a
# 144-element slot, a gap of 16 elements, a slot whose gradient is all zero, a slot whose weights
# are all zero
HAND_SLOTS = [(0, 16, 16, 1), (16, 10, 16, 0), (32, 144, 144, 1), (192, 32, 32, 1), (224, 32, 32, 1)]
ZERO_GRAD_SLOT, ZERO_WEIGHT_SLOT = 3, 4
HAND_TOTAL = 256
# constant LR of the 30-step fixed-batch training test (cifar_resnet_v2(8), N = 32, eta = 0.001): the
# fp32 oracle executor takes the cross entropy from 2.49 to 0.03 with it (lr 4 also converges,
# lr 16 first climbs to 6.0); shared with tests/test_lars_gpu.py
TRAIN_LR = 1.0


def hand_buffers(total, slots, seed=5):
    """Random w, m, g over the whole buffer (padding and gaps included) with the two all-zero slots."""
    gen = torch.Generator().manual_seed(seed)
    w, m, g = (torch.randn(total, generator=gen, dtype=torch.float64) for _ in range(3))
    off, n = slots[ZERO_GRAD_SLOT][:2]
    g[off:off + n] = 0
    off, n = slots[ZERO_WEIGHT_SLOT][:2]
    w[off:off + n] = 0
    return w, m, g


def numpy_lars(w, m, g, slots, lr, mu, wd, gs, eta, eps):
    """The issue's definition, per slot, in float64 numpy."""
    w, m, trust = w.copy(), m.copy(), np.ones(len(slots))
    for i, (off, n, _, adapt) in enumerate(slots):
        ws, sg = w[off:off + n], gs * g[off:off + n]
        wn, gn = np.sqrt((ws * ws).sum()), np.sqrt((sg * sg).sum())
        if adapt and wn > 0 and gn > 0:
            trust[i] = eta * wn / (gn + wd * wn + eps)
        m[off:off + n] = mu * m[off:off + n] + trust[i] * (sg + wd * ws)
        w[off:off + n] = ws - lr * m[off:off + n]
    return w, m, trust


@pytest.fixture
def ref64():
    """The fp64 oracle backend; the process-wide reference dtype goes back to fp32 afterwards."""
    yield RefBackend("cpu", dtype=torch.float64)
    RefBackend("cpu")


# -- schedule ------------------------------------------------------------------------------------
def test_poly_schedule_values():
    """LR applied to step s under the LRSchedule protocol (derived from the global step the
    previous step returned): 0 at step 0, linear to peak at warmup_steps, polynomial to end_lr."""
    peak, warm, total, power, end = 3.2, 10, 110, 2.0, 0.01
    sch = lr_mod.poly(peak, warm, total, power, end)
    applied = {}
    for s in range(total + 1):
        applied[s] = sch.lr_for_step()
        sch.after_step(s + 1)  # the step returns global step s + 1
    assert applied[0] == 0.0
    assert applied[5] == pytest.approx(peak * 5 / 10, rel=1e-12)
    assert applied[warm] == pytest.approx(peak, rel=1e-12)
    assert applied[60] == pytest.approx(end + (peak - end) * (1 - 50 / 100) ** 2, rel=1e-12)
    assert applied[total] == pytest.approx(end, rel=1e-12)
    assert all(applied[s] > applied[s + 1] for s in range(warm, total))
    # power 1 is a straight line; the reference schedules are untouched
    assert lr_mod.poly_lr(60, 1.0, 10, 110, 1.0, 0.0) == pytest.approx(0.5)
    assert lr_mod.for_dataset("cifar10").lr_for_step() == 0.1
    assert lr_mod.for_dataset("imagenet").lr_for_step() == 0.4
    with pytest.raises(ValueError):
        lr_mod.poly(1.0, 10, 10)


# -- flags ---------------------------------------------------------------------------------------
def test_flags_parse_and_reject_sharded_lars():
    F = cli.entry_flags("cifar_main", [])
    assert (F.optimizer, F.lars_eta, F.lars_eps, F.lr_policy, F.poly_power, F.end_lr) == \
        ("momentum", 0.001, 1e-9, "reference", 2.0, 0.0)
    assert lr_mod.from_flags(F).lr_for_step() == 0.1
    F = cli.entry_flags("imagenet_main", ["--optimizer=lars", "--lars_eta", "0.002", "--lars_eps=1e-8",
                                          "--lr_policy=poly", "--peak_lr=6.4", "--warmup_steps=50",
                                          "--poly_power=1.5", "--end_lr=0.001", "--train_steps=1000"])
    assert (F.optimizer, F.lars_eta, F.lars_eps, F.lr_policy) == ("lars", 0.002, 1e-8, "poly")
    assert (F.peak_lr, F.warmup_steps, F.poly_power, F.end_lr) == (6.4, 50, 1.5, 0.001)
    sch = lr_mod.from_flags(F)
    sch.after_step(50)
    assert sch.lr_for_step() == pytest.approx(6.4)
    with pytest.raises(FlagsError, match="optimizer_sharding"):
        cli.entry_flags("cifar_main", ["--optimizer=lars", "--optimizer_sharding"])
    with pytest.raises(FlagsError):
        cli.entry_flags("cifar_main", ["--optimizer=adam"])
    with pytest.raises(FlagsError):
        cli.entry_flags("cifar_main", ["--lr_policy=cosine"])
    assert cli.entry_flags("cifar_main", ["--optimizer_sharding"]).optimizer_sharding  # (momentum: still fine)


def test_checkpoint_meta_names_the_optimizer():
    from distributed_resnet_tensorflow_amd.train.trainer import _meta, model_spec_from_flags
    F = cli.entry_flags("cifar_main", ["--optimizer=lars", "--lars_eta=0.002", "--resnet_size=8"])
    meta = _meta(F, model_spec_from_flags(F))
    assert (meta["optimizer"], meta["eta"], meta["eps"]) == ("lars", 0.002, 1e-9)


# -- oracle backend --------------------------------------------------------------------------------
def test_ref_lars_momentum_fp64_matches_numpy(ref64):
    lr, mu, wd, gs, eta, eps = 0.3, 0.9, 2e-4, 0.5, 0.001, 1e-9
    w0, m0, g = hand_buffers(HAND_TOTAL, HAND_SLOTS)
    table = LarsTable(HAND_SLOTS)
    w, m, wb = w0.clone(), m0.clone(), torch.full((HAND_TOTAL,), 7.0, dtype=torch.float64)
    trust = torch.full((len(HAND_SLOTS),), -1.0)
    ref64.lars_momentum(w, m, g, wb, table, 0, table.n, torch.zeros(2 * table.chunks), trust,
                        torch.tensor([lr], dtype=torch.float64), mu, wd, gs, eta, eps)
    we, me, te = numpy_lars(w0.numpy(), m0.numpy(), g.numpy(), HAND_SLOTS, lr, mu, wd, gs, eta, eps)
    np.testing.assert_allclose(w.numpy(), we, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(m.numpy(), me, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(trust.double().numpy(), te, rtol=1e-6)  # (trust is stored in fp32)
    assert trust[1] == 1.0 and trust[ZERO_GRAD_SLOT] == 1.0 and trust[ZERO_WEIGHT_SLOT] == 1.0
    assert 0 < trust[0] < 1 and 0 < trust[2] < 1
    inside = torch.zeros(HAND_TOTAL, dtype=torch.bool)
    for off, n, _, _ in HAND_SLOTS:
        inside[off:off + n] = True
    assert torch.equal(w[~inside], w0[~inside]) and torch.equal(m[~inside], m0[~inside])  # padding, the gap
    assert torch.equal(wb[inside], w[inside]) and bool((wb[~inside] == 7.0).all())
    # a non-zero skip word: nothing changes, trust included
    w2, m2, t2 = w.clone(), m.clone(), trust.clone()
    ref64.lars_momentum(w2, m2, g, None, table, 0, table.n, None, t2, torch.tensor([lr], dtype=torch.float64),
                        mu, wd, gs, eta, eps, skip=torch.tensor([1], dtype=torch.int32))
    assert torch.equal(w2, w) and torch.equal(m2, m) and torch.equal(t2, trust)


def test_lars_table_ranges():
    t = LarsTable(HAND_SLOTS)
    assert t.n == 5 and t.chunks == 5 and list(t.arr["begin"]) == [0, 1, 2, 3, 4, 5]
    assert t.slot_range(0, HAND_TOTAL) == (0, 5)
    assert t.slot_range(16, 176) == (1, 2) and t.slot_range(16, 192) == (1, 2) and t.slot_range(176, 256) == (3, 2)
    for lo, hi in ((8, 256), (0, 100), (20, 32), (0, 26)):
        with pytest.raises(ValueError):
            t.slot_range(lo, hi)
    big = LarsTable([(0, 8192, 8192, 1), (8192, 8194, 8208, 1), (16400, 300000, 300000, 0)])
    assert list(big.arr["begin"]) == [0, 1, 3, 40] and big.chunks == 40
    with pytest.raises(ValueError):
        LarsTable([(0, 16, 16, 1), (8, 16, 16, 1)])  # overlapping slots


# -- executor ----------------------------------------------------------------------------------------
def _executor(optimizer, N=8, seed=3, **kw):
    ex = Executor(cifar_resnet_v2(8), N, RefBackend(), "cpu", seed=seed, optimizer=optimizer, **kw)
    g = torch.Generator().manual_seed(11)
    ex.images.zero_()
    ex.images[..., :3] = torch.randn(N, 32, 32, 3, generator=g).bfloat16().float()
    ex.labels.copy_(torch.randint(0, 10, (N,), generator=g, dtype=torch.int32))
    return ex


def test_executor_lars_two_steps_against_momentum():
    """Step 1 from equal weights: every excluded slot (gamma, beta, dense bias) of the LARS run
    equals the momentum run exactly, and every conv / dense kernel moves by lr * trust * (g + wd * w).
    Step 2 (the two runs' weights, hence gradients, differ by then, so the LARS run is checked
    against its own gradient): excluded slots follow the plain momentum update exactly, adapting
    slots the trust-scaled one."""
    lr, wd, mu = 0.1, 2e-4, 0.9
    a, b = _executor("lars"), _executor("momentum")
    assert a.lars_trust.shape == (len(a.P.slots),) and b.lars_trust is None
    w0 = a.P.master.clone()
    a.train_step(lr=lr)
    b.train_step(lr=lr)
    trust1 = a.lars_trust.clone()
    adapting = 0
    for i, s in enumerate(a.P.slots):
        sl = slice(s.offset, s.offset + s.numel)
        if s.kind in LARS_EXCLUDED:
            assert trust1[i] == 1.0
            assert torch.equal(a.P.master[sl], b.P.master[sl]), s.name
            assert torch.equal(a.P.momentum[sl], b.P.momentum[sl]), s.name
        else:
            adapting += 1
            assert 0 < trust1[i] < 1, (s.name, float(trust1[i]))
            gg = a.P.grad[sl].double() + wd * w0[sl].double()
            wn, gn = w0[sl].double().norm(), a.P.grad[sl].double().norm()
            assert float(trust1[i]) == pytest.approx(float(0.001 * wn / (gn + wd * wn + 1e-9)), rel=1e-5)
            step = w0[sl].double() - a.P.master[sl].double()
            want = lr * float(trust1[i]) * gg
            # w is stored in fp32: each element of the observed step carries up to one rounding of w
            # (2^-24 |w|) on top of the fp32 arithmetic of the step itself
            bound = 2.0 ** -23 * float(w0[sl].double().norm()) + 1e-5 * float(want.norm())
            assert float((step - want).norm()) < bound, s.name
            assert float(step.norm()) > 100 * 2.0 ** -23 * float(w0[sl].double().norm())  # (a real move)
            assert not torch.equal(a.P.master[sl], b.P.master[sl])
    assert adapting == sum(s.kind in ("conv", "dense_w") for s in a.P.slots) > 0
    w1, m1 = a.P.master.clone(), a.P.momentum.clone()
    a.train_step(lr=lr)
    for i, s in enumerate(a.P.slots):
        sl = slice(s.offset, s.offset + s.numel)
        gg = a.P.grad[sl] * 1.0 + wd * w1[sl]
        if s.kind in LARS_EXCLUDED:
            m2 = m1[sl] * mu + gg
            assert torch.equal(a.P.momentum[sl], m2) and torch.equal(a.P.master[sl], w1[sl] - lr * m2), s.name
        else:
            m2 = m1[sl].double() * mu + float(a.lars_trust[i]) * gg.double()
            assert float((a.P.momentum[sl].double() - m2).norm() / m2.norm()) < 1e-5, s.name
    # padding inside the flat buffer stays exactly zero
    inside = torch.zeros(a.P.total, dtype=torch.bool)
    for s in a.P.slots:
        inside[s.offset:s.offset + s.numel] = True
    assert not a.P.master[~inside].any() and not a.P.momentum[~inside].any()


def test_executor_lars_range_must_hold_whole_slots():
    ex = _executor("lars", N=2)
    ex.forward(True)
    ex.backward()
    ex.set_lr(0.1)
    s1 = ex.P.slots[1]
    before = ex.P.master.clone()
    with pytest.raises(ValueError, match="cuts a parameter slot"):
        ex._update(0, ex.P.slots[0].numel // 2, ex.P.grad, 1.0)
    with pytest.raises(ValueError, match="cuts a parameter slot"):
        ex._update(s1.offset + 4, ex.P.total, ex.P.grad, 1.0)
    assert torch.equal(before, ex.P.master)
    ex._update(s1.offset, ex.P.total, ex.P.grad, 1.0)  # a slot boundary: fine
    assert torch.equal(before[:s1.offset], ex.P.master[:s1.offset])
    assert not torch.equal(before[s1.offset:], ex.P.master[s1.offset:])
    with pytest.raises(RuntimeError, match="sharding"):
        ex.sgd_range(0, ex.P.total, 1.0)
    with pytest.raises(ValueError):
        Executor(cifar_resnet_v2(8), 2, RefBackend(), "cpu", optimizer="adam")


def test_oracle_training_halves_the_loss_at_the_recorded_lr():
    """The constant LR the GPU training test uses is one at which the oracle itself at least halves
    the cross entropy in 30 steps on a fixed batch."""
    ex = _executor("lars", N=32, lars_eta=0.001)
    losses = []
    for _ in range(30):
        ex.train_step(lr=TRAIN_LR)
        losses.append(float(ex.loss_vec.double().mean()))
    ex.forward(train=True)
    final = float(ex.loss_vec.double().mean())
    assert np.isfinite(losses).all() and final <= 0.5 * losses[0], (losses[0], final)


def test_summary_hook_writes_trust_scalars():
    from distributed_resnet_tensorflow_amd.train.hooks import SummaryHook

    class W:
        def add_scalars(self, step, scalars):
            self.got = (step, scalars)

    class S:
        pass

    sess, w = S(), W()
    sess.ex = _executor("lars", N=2)
    sess.ex.train_step(lr=0.1)
    metrics = lambda: {"cross_entropy": 1.0, "cost": 2.0, "learning_rate": 0.1, "precision": 0.5}  # noqa: E731
    SummaryHook(w, 1).after_step(sess, 1, metrics)
    sc = w.got[1]
    assert 0 < sc["lars/trust_min"] <= sc["lars/trust_mean"] <= sc["lars/trust_max"] < 1  # (adapting slots only)
    sess.ex = _executor("momentum", N=2)
    SummaryHook(w, 1).after_step(sess, 1, metrics)
    assert not any(k.startswith("lars/") for k in w.got[1])


# -- two ranks over gloo ---------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, mode, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from distributed_resnet_tensorflow_amd.parallel.engine import DataParallelEngine
        N = 4
        ex = Executor(cifar_resnet_v2(8), N, RefBackend(), "cpu", seed=1 + rank, optimizer="lars")
        eng = DataParallelEngine(ex, bucket_mb=0.05, mode=mode)
        eng.broadcast_parameters()
        g = torch.Generator().manual_seed(100 + rank)  # every rank trains on its own shard
        for _ in range(3):
            ex.images[..., :3] = torch.randn(N, 32, 32, 3, generator=g)
            ex.labels.copy_(torch.randint(0, 10, (N,), generator=g, dtype=torch.int32))
            ex.set_lr(0.5)
            ex.forward(True)
            eng.begin_step()
            ex.backward()
            eng.apply_gradients(eng.finish(), 1.0 / world)
        state = torch.cat([ex.P.master, ex.P.momentum, ex.lars_trust])
        gathered = [torch.zeros_like(state) for _ in range(world)]
        dist.all_gather(gathered, state)
        same = all(torch.equal(gathered[0], t) for t in gathered)
        moved = bool(ex.P.momentum.abs().sum() > 0) and bool((ex.lars_trust != 1).any())
        q.put((rank, same and moved, ""))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, False, repr(e) + traceback.format_exc()))


@pytest.mark.parametrize("mode", ["sync", "delayed"])
def test_gloo_two_ranks_stay_bitwise_in_sync_under_lars(mode):
    """After 3 LARS steps (every rank on its own data shard) both ranks hold bitwise equal master
    weights, momentum and trust ratios; delayed = the 1-step-delayed all-reduce."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_dp_worker, args=(r, world, port, mode, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = [q.get(timeout=300) for _ in ps]
    for p in ps:
        p.join(timeout=60)
    for rank, ok, err in res:
        assert ok, (rank, err)

