"""AdamW / LAMB optimizers and the warm-up + cosine LR schedule: CPU tests (oracle backend, bias
correction, schedule, flags, checkpoints, two-rank gloo run). The HIP kernels are covered by
tests/test_adam_gpu.py."""
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from adam_refs import ADAM_HP, TRAIN_LR, fixed_batch_executor, hand_adam_buffers, numpy_adam
from test_lars import HAND_SLOTS, HAND_TOTAL, ZERO_WEIGHT_SLOT, _free_port

from distributed_resnet_tensorflow_amd import cli
from distributed_resnet_tensorflow_amd.ckpt.saver import Saver
from distributed_resnet_tensorflow_amd.flags import FlagsError
from distributed_resnet_tensorflow_amd.models.spec import cifar_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import LarsTable, RefBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor
from distributed_resnet_tensorflow_amd.runtime.state import export_state, import_state
from distributed_resnet_tensorflow_amd.train import lr as lr_mod

ZERO_U_SLOT = 3   # the hand list's zero-gradient slot, given zero moments and wd = 0: u is identically 0


@pytest.fixture
def ref64():
    """The fp64 oracle backend; the process-wide reference dtype goes back to fp32 afterwards."""
    yield RefBackend("cpu", dtype=torch.float64)
    RefBackend("cpu")


def _t64(*v):
    return torch.tensor(list(v), dtype=torch.float64)


# -- 1. the oracle against the definition -------------------------------------------------------------
@pytest.mark.parametrize("wd", [ADAM_HP["wd"], 0.0])
@pytest.mark.parametrize("opt", ["adamw", "lamb"])
def test_ref_fp64_matches_the_numpy_definition(ref64, opt, wd):
    hp = dict(ADAM_HP, wd=wd)
    w0, m0, v0, g = hand_adam_buffers(HAND_TOTAL, HAND_SLOTS)
    off, n = HAND_SLOTS[ZERO_U_SLOT][:2]
    m0[off:off + n] = 0
    v0[off:off + n] = 0
    table = LarsTable(HAND_SLOTS)
    inside = torch.zeros(HAND_TOTAL, dtype=torch.bool)
    for o, k, _, _ in HAND_SLOTS:
        inside[o:o + k] = True
    w, m, v = w0.clone(), m0.clone(), v0.clone()
    wb = torch.full((HAND_TOTAL,), 7.0, dtype=torch.float64)
    trust = torch.full((len(HAND_SLOTS),), -1.0)
    lr_t, bc_t = _t64(hp["lr"]), _t64(hp["c1"], hp["c2"])
    args = (hp["b1"], hp["b2"], hp["eps"], hp["wd"], hp["gs"])
    if opt == "adamw":
        # (element-wise over a flat range: applied to the slots' union, one slot at a time)
        for o, k, _, _ in HAND_SLOTS:
            ref64.adamw(w[o:o + k], m[o:o + k], v[o:o + k], g[o:o + k], wb[o:o + k], lr_t, bc_t, *args)
    else:
        ref64.lamb(w, m, v, g, wb, table, 0, table.n, None, trust, lr_t, bc_t, *args)
    we, me, ve, te = numpy_adam(w0.numpy(), m0.numpy(), v0.numpy(), g.numpy(), HAND_SLOTS, lamb=opt == "lamb", **hp)
    for got, want in ((w, we), (m, me), (v, ve)):
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-13, atol=1e-15)
    assert torch.equal(w[~inside], w0[~inside]) and torch.equal(m[~inside], m0[~inside])  # padding, the gap
    assert torch.equal(v[~inside], v0[~inside])
    assert torch.equal(wb[inside], w[inside]) and bool((wb[~inside] == 7.0).all())
    if opt == "lamb":
        np.testing.assert_allclose(trust.double().numpy(), te, rtol=1e-6)  # (trust is stored in fp32)
        assert trust[1] == 1.0 and trust[ZERO_WEIGHT_SLOT] == 1.0          # excluded; zero weights
        if wd == 0.0:
            assert trust[ZERO_U_SLOT] == 1.0 and not w[off:off + n].ne(w0[off:off + n]).any()  # u == 0
        for i in (0, 2):
            assert 0 < float(trust[i]) < float("inf") and trust[i] != 1.0
    # a non-zero skip word changes nothing, trust included
    w2, m2, v2, t2 = w.clone(), m.clone(), v.clone(), trust.clone()
    skip = torch.tensor([1], dtype=torch.int32)
    if opt == "adamw":
        ref64.adamw(w2, m2, v2, g, None, lr_t, bc_t, *args, skip=skip)
    else:
        ref64.lamb(w2, m2, v2, g, None, table, 0, table.n, None, t2, lr_t, bc_t, *args, skip=skip)
    assert torch.equal(w2, w) and torch.equal(m2, m) and torch.equal(v2, v) and torch.equal(t2, trust)


# -- 2. bias correction -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 10])
def test_bias_correction_recovers_a_constant_gradient(ref64, k):
    """k updates from zero moments with a constant gradient: m / c1 == g' (and v / c2 == g'^2)."""
    b1, b2, gs = 0.9, 0.999, 0.5
    gen = torch.Generator().manual_seed(4)
    g = torch.randn(64, generator=gen, dtype=torch.float64)
    w, m, v = torch.randn(64, generator=gen, dtype=torch.float64), torch.zeros(64).double(), torch.zeros(64).double()
    for t in range(1, k + 1):
        bc = _t64(1 - b1 ** t, 1 - b2 ** t)
        ref64.adamw(w, m, v, g, None, _t64(1e-3), bc, b1, b2, 1e-6, 0.0, gs)
    c1, c2 = 1 - b1 ** k, 1 - b2 ** k
    np.testing.assert_allclose((m / c1).numpy(), (gs * g).numpy(), rtol=1e-12)
    np.testing.assert_allclose((v / c2).numpy(), ((gs * g) ** 2).numpy(), rtol=1e-12)


def test_set_adam_step_counts_from_adam_t0():
    ex = Executor(cifar_resnet_v2(8), 2, RefBackend(), "cpu", optimizer="adamw", adam_beta1=0.8, adam_beta2=0.99)
    assert ex.P.adam_v is not None and ex.P.adam_t0 == 0 and ex.adam_bc_t.shape == (2,)
    fresh = {}
    for s in (0, 1, 9):
        ex.set_adam_step(s)
        fresh[s] = ex.adam_bc_t.clone()
        t = s + 1
        assert ex.adam_bias_corrections(s) == (1 - 0.8 ** t, 1 - 0.99 ** t)
        np.testing.assert_allclose(fresh[s].double().numpy(), [1 - 0.8 ** t, 1 - 0.99 ** t], rtol=2.0 ** -23)
    ex.P.adam_t0 = 1000
    for s in (0, 1, 9):   # the same count of updates since the moments were zero: the same (c1, c2)
        ex.set_adam_step(1000 + s)
        assert torch.equal(ex.adam_bc_t, fresh[s])
    # momentum / LARS keep no second moment and no record
    ex = Executor(cifar_resnet_v2(8), 2, RefBackend(), "cpu", optimizer="lars")
    assert ex.P.adam_v is None and ex.adam_bc_t is None
    ex.set_adam_step(3)
    for bad in (dict(adam_beta1=1.0), dict(adam_beta2=-0.1), dict(adam_eps=0.0)):
        with pytest.raises(ValueError):
            Executor(cifar_resnet_v2(8), 2, RefBackend(), "cpu", optimizer="adamw", **bad)


# -- 3. the cosine schedule ---------------------------------------------------------------------------
def test_cosine_schedule_values():
    peak, warm, total, end = 3.2, 10, 110, 0.01
    sch = lr_mod.cosine(peak, warm, total, end)
    applied = {}
    for s in range(total + 5):
        applied[s] = sch.lr_for_step()
        sch.after_step(s + 1)
    assert applied[0] == 0.0
    assert applied[5] == pytest.approx(peak * 5 / 10, rel=1e-12)
    assert applied[warm] == pytest.approx(peak, rel=1e-12)
    assert applied[60] == pytest.approx(end + (peak - end) * 0.5, rel=1e-12)           # the mid-point
    assert applied[35] == pytest.approx(end + (peak - end) * 0.5 * (1 + np.cos(np.pi * 0.25)), rel=1e-12)
    assert all(applied[s] == pytest.approx(end, rel=1e-12) for s in range(total, total + 5))
    assert all(applied[s] >= applied[s + 1] for s in range(warm, total + 4))
    assert lr_mod.cosine(1.0, 0, 10).lr_for_step() == 1.0   # no warm-up: the first step runs at the peak
    for warm_bad in (10, 11):
        with pytest.raises(ValueError):
            lr_mod.cosine(1.0, warm_bad, 10)


# -- 4. flags and .meta -------------------------------------------------------------------------------
def test_flags_accept_and_reject():
    F = cli.entry_flags("cifar_main", [])
    assert (F.optimizer, F.adam_beta1, F.adam_beta2, F.adam_epsilon) == ("momentum", 0.9, 0.999, 1e-6)
    F = cli.entry_flags("imagenet_main", ["--optimizer=lamb", "--adam_beta1=0.8", "--adam_beta2", "0.99",
                                          "--adam_epsilon=1e-8", "--lr_policy=warmup_cosine", "--peak_lr=0.004",
                                          "--warmup_steps=50", "--end_lr=1e-5", "--train_steps=1000",
                                          "--clip_grad_norm=1.0", "--skip_nonfinite_grads"])
    assert (F.optimizer, F.adam_beta1, F.adam_beta2, F.adam_epsilon, F.lr_policy) == \
        ("lamb", 0.8, 0.99, 1e-8, "warmup_cosine")
    sch = lr_mod.from_flags(F)
    assert sch.lr_for_step() == 0.0
    sch.after_step(50)
    assert sch.lr_for_step() == pytest.approx(0.004)
    sch.after_step(1000)
    assert sch.lr_for_step() == pytest.approx(1e-5)
    assert cli.entry_flags("cifar_main", ["--optimizer=adamw", "--optimizer_sharding"]).optimizer_sharding
    assert cli.entry_flags("cifar_main", ["--optimizer=adamw", "--ema_decay=0.99", "--label_smoothing=0.1",
                                          "--mixup_alpha=0.2"]).optimizer == "adamw"
    for policy_opt in ("momentum", "lars", "adamw", "lamb"):
        assert cli.entry_flags("cifar_main", [f"--optimizer={policy_opt}", "--lr_policy=warmup_cosine",
                                              "--train_steps=10"]).lr_policy == "warmup_cosine"
    with pytest.raises(FlagsError, match="optimizer_sharding"):
        cli.entry_flags("cifar_main", ["--optimizer=lamb", "--optimizer_sharding"])
    for opt in ("adamw", "lamb"):
        with pytest.raises(FlagsError, match="lrnet"):
            cli.entry_flags("cifar_main", [f"--optimizer={opt}", "--model=lrnet"])
    for bad in ("--adam_beta1=1.0", "--adam_beta1=-0.1", "--adam_beta2=1", "--adam_beta2=-1e-3", "--adam_epsilon=0",
                "--adam_epsilon=-1e-8", "--optimizer=adam"):
        with pytest.raises(FlagsError):
            cli.entry_flags("cifar_main", [bad])


def test_meta_round_trips_the_optimizer(tmp_path):
    from distributed_resnet_tensorflow_amd.train.trainer import _meta, model_spec_from_flags
    F = cli.entry_flags("cifar_main", ["--optimizer=adamw", "--adam_beta1=0.8", "--adam_epsilon=1e-7",
                                       "--resnet_size=8"])
    meta = _meta(F, model_spec_from_flags(F))
    assert (meta["optimizer"], meta["adam_beta1"], meta["adam_beta2"], meta["adam_eps"]) == ("adamw", 0.8, 0.999, 1e-7)
    prefix = str(tmp_path / "model.ckpt-1")
    with open(prefix + ".meta", "w") as f:
        json.dump(meta, f)
    back = Saver.restore_meta(prefix)
    assert (back["optimizer"], back["adam_beta1"], back["adam_beta2"], back["adam_eps"]) == ("adamw", 0.8, 0.999, 1e-7)
    old = {k: v for k, v in meta.items() if k not in ("optimizer", "adam_beta1", "adam_beta2", "adam_eps")}
    with open(prefix + ".meta", "w") as f:
        json.dump(old, f)
    back = Saver.restore_meta(prefix)
    assert (back["optimizer"], back["adam_beta1"], back["adam_beta2"], back["adam_eps"]) == \
        ("momentum", 0.9, 0.999, 1e-6)


# -- 5. checkpoints -----------------------------------------------------------------------------------
def _steps(ex, n, lr=1e-3):
    for _ in range(n):
        ex.train_step(lr=lr)
        ex.P.global_step += 1


@pytest.mark.parametrize("opt", ["adamw", "lamb"])
def test_checkpoint_resume_is_bitwise(opt):
    a = fixed_batch_executor(opt, N=4)
    _steps(a, 3)
    tensors = export_state(a)
    s0 = a.P.slots[0].name
    assert f"{s0}/Adam" in tensors and f"{s0}/Adam_1" in tensors and f"{s0}/Momentum" not in tensors
    assert tensors["beta1_power"].dtype == np.float32 and tensors["beta2_power"].dtype == np.float32
    assert float(tensors["beta1_power"]) == pytest.approx(0.9 ** 4, rel=1e-6)   # the 4th update's powers
    assert float(tensors["beta2_power"]) == pytest.approx(0.999 ** 4, rel=1e-6)
    assert tensors["drn/adam_t0"].dtype == np.int64 and int(tensors["drn/adam_t0"]) == 0
    b = fixed_batch_executor(opt, N=4, seed=99)   # other initial weights: everything comes from the checkpoint
    extra = import_state(b, tensors)
    assert "adam_t0" not in extra and b.P.global_step == 3 and b.P.adam_t0 == 0
    a.set_adam_step(3)
    assert torch.equal(b.adam_bc_t, a.adam_bc_t)
    _steps(a, 1)
    _steps(b, 1)
    for name in ("master", "momentum", "adam_v", "bn_state"):
        assert torch.equal(getattr(a.P, name), getattr(b.P, name)), name


def test_momentum_checkpoint_restores_into_adamw_with_zero_moments(caplog):
    a = fixed_batch_executor("momentum", N=4)
    for _ in range(2):
        a.train_step(lr=0.1)
        a.P.global_step += 1
    tensors = export_state(a)
    assert not any(k.endswith("/Adam") or k == "beta1_power" for k in tensors)   # momentum checkpoints are unchanged
    b = fixed_batch_executor("adamw", N=4, seed=99)
    b.P.momentum.fill_(3.0)
    b.P.adam_v.fill_(3.0)
    with caplog.at_level("WARNING", logger="drn"):
        import_state(b, tensors)
    assert "Adam moments" in caplog.text
    assert not b.P.momentum.any() and not b.P.adam_v.any()
    assert b.P.global_step == 2 and b.P.adam_t0 == 2
    assert torch.equal(b.P.master, a.P.master)
    np.testing.assert_allclose(b.adam_bc_t.double().numpy(), [1 - 0.9, 1 - 0.999], rtol=2.0 ** -23)  # t = 1 again
    # ... and an Adam checkpoint into momentum: the momentum starts from zero
    c = fixed_batch_executor("momentum", N=4, seed=99)
    for s in c.P.slots:
        c.P.view(c.P.momentum, s.name).fill_(3.0)
    extra = import_state(c, export_state(b))
    assert not c.P.momentum.any() and "adam_t0" not in extra


# -- 6. sharded AdamW over gloo -----------------------------------------------------------------------
def _zero1_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from distributed_resnet_tensorflow_amd.parallel.engine import DataParallelEngine
        out = {}
        for shard in (False, True):
            ex = Executor(cifar_resnet_v2(8), 4, RefBackend(), "cpu", seed=1, optimizer="adamw")
            g = torch.Generator().manual_seed(100 + rank)
            ex.images[..., :3] = torch.randn(4, 32, 32, 3, generator=g)
            ex.labels.copy_(torch.randint(0, 10, (4,), generator=g, dtype=torch.int32))
            eng = DataParallelEngine(ex, bucket_mb=0.05, shard_optimizer=shard)
            assert eng.zero1 == shard
            eng.broadcast_parameters()
            ex.set_lr(1e-3)
            for step in range(2):
                ex.set_adam_step(step)
                ex.forward(True)
                eng.begin_step()
                ex.backward()
                eng.apply_gradients(eng.finish(), 1.0 / world)
            eng.gather_state()
            out[shard] = [t.clone() for t in (ex.P.master, ex.P.momentum, ex.P.adam_v)]
        same = all(torch.equal(a, b) for a, b in zip(out[True], out[False]))
        moved = bool(out[True][2].abs().sum() > 0)
        refused = False
        try:
            DataParallelEngine(Executor(cifar_resnet_v2(8), 4, RefBackend(), "cpu", optimizer="lamb"),
                               bucket_mb=0.05, shard_optimizer=True)
        except ValueError:
            refused = True
        q.put((rank, same and moved and refused, f"same {same} moved {moved} refused {refused}"))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, False, repr(e) + traceback.format_exc()))


def test_sharded_adamw_matches_the_unsharded_engine_bitwise():
    """ZeRO-1 over gloo, world 2: after 2 steps and gather_state(), master, momentum (m) and adam_v
    equal the all-reduce engine's bit for bit (the update is element-wise); LAMB is refused."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_zero1_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = [q.get(timeout=300) for _ in ps]
    for p in ps:
        p.join(timeout=60)
    for rank, ok, err in res:
        assert ok, (rank, err)


def test_sgd_range_dispatches_adamw_and_refuses_lamb():
    ex = fixed_batch_executor("adamw", N=2)
    ex.forward(True)
    ex.backward()
    ex.set_lr(1e-3)
    w0, v0 = ex.P.master.clone(), ex.P.adam_v.clone()
    ex.sgd_range(64, 256, 1.0)
    changed = (ex.P.master != w0) | (ex.P.adam_v != v0)
    assert bool(changed[64:256].any()) and not changed[:64].any() and not changed[256:].any()
    with pytest.raises(RuntimeError, match="LARS needs every tensor's whole norm"):
        fixed_batch_executor("lamb", N=2).sgd_range(0, 64, 1.0)


# -- 7. training --------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["adamw", "lamb"])
def test_oracle_training_halves_the_loss_at_the_recorded_lr(opt):
    """cifar_resnet_v2(8), N = 32, one fixed batch, 30 steps of the fp32 oracle executor at the
    constant LR of adam_refs.TRAIN_LR (shared with the GPU test). Observed on the CPU:
      adamw  lr 0.01: cross entropy 2.4868 -> 0.0012
      lamb   lr 0.02: cross entropy 2.4868 -> 0.0013
    both far below a quarter of the initial loss; the assertion is final < initial / 2."""
    ex = fixed_batch_executor(opt, N=32)
    ex.forward(train=True)
    first = float(ex.loss_vec.double().mean())
    for _ in range(30):
        ex.train_step(lr=TRAIN_LR[opt])
        ex.P.global_step += 1
    ex.forward(train=True)
    final = float(ex.loss_vec.double().mean())
    print(f"{opt}: loss {first} -> {final}")
    assert np.isfinite(final) and final < first / 2, (first, final)


def test_summary_hook_writes_lamb_trust_scalars():
    from distributed_resnet_tensorflow_amd.train.hooks import SummaryHook

    class W:
        def add_scalars(self, step, scalars):
            self.got = (step, scalars)

    class S:
        pass

    sess, w = S(), W()
    sess.ex = fixed_batch_executor("lamb", N=2)
    sess.ex.train_step(lr=1e-3)
    metrics = lambda: {"cross_entropy": 1.0, "cost": 2.0, "learning_rate": 0.1, "precision": 0.5}  # noqa: E731
    SummaryHook(w, 1).after_step(sess, 1, metrics)
    sc = w.got[1]
    assert 0 < sc["lamb/trust_min"] <= sc["lamb/trust_mean"] <= sc["lamb/trust_max"] < float("inf")
    assert not any(k.startswith("lars/") for k in sc)
