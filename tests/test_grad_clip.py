"""Global-norm gradient clipping and the non-finite step guard: CPU tests on the oracle backend --
flags, RefBackend.grad_guard against an fp64 formula, the executor's clipped and skipped steps, the
summary scalars, the checkpoint meta and a two-rank gloo run. The HIP kernels are covered by
tests/test_grad_clip_gpu.py."""
import math
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
from distributed_resnet_tensorflow_amd.ops.backend import (GUARD_SKIP, RefBackend, guard_record_read,
                                                           guard_record_tensor)
from distributed_resnet_tensorflow_amd.runtime.executor import Executor


def _executor(N=8, seed=1, data_seed=7, **kw):
    ex = Executor(cifar_resnet_v2(8), N, RefBackend(), "cpu", seed=seed, **kw)
    g = torch.Generator().manual_seed(data_seed)
    ex.images.zero_()
    ex.images[..., :3] = torch.randn(N, 32, 32, 3, generator=g)
    ex.labels.copy_(torch.randint(0, 10, (N,), generator=g, dtype=torch.int32))
    ex.set_lr(0.1)
    return ex


# -- flags ---------------------------------------------------------------------------------------------
def test_flags_defaults_validation_and_wiring(monkeypatch):
    F = cli.entry_flags("cifar_main", [])
    assert (F.clip_grad_norm, F.skip_nonfinite_grads) == (0.0, False)
    F = cli.entry_flags("imagenet_main", ["--clip_grad_norm=2.5", "--skip_nonfinite_grads"])
    assert (F.clip_grad_norm, F.skip_nonfinite_grads) == (2.5, True)
    assert cli.entry_flags("cifar_main", ["--clip_grad_norm=0"]).clip_grad_norm == 0.0
    for bad in (["--clip_grad_norm=-1"], ["--clip_grad_norm=nan"], ["--clip_grad_norm=inf"],
                ["--clip_grad_norm=1.0", "--optimizer_sharding"], ["--skip_nonfinite_grads", "--optimizer_sharding"],
                ["--clip_grad_norm=1.0", "--model=lrnet"], ["--skip_nonfinite_grads=True", "--model=lrnet"]):
        with pytest.raises(FlagsError):
            cli.entry_flags("cifar_main", bad)
    cli.entry_flags("cifar_main", ["--optimizer_sharding"])      # (alone: still accepted)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="clip_grad_norm"):
            Executor(cifar_resnet_v2(8), 2, RefBackend(), "cpu", clip_grad_norm=bad)
    from distributed_resnet_tensorflow_amd.parallel.cluster import ClusterInfo
    from distributed_resnet_tensorflow_amd.train import lr as lr_mod
    from distributed_resnet_tensorflow_amd.train import trainer
    from distributed_resnet_tensorflow_amd.train.session import TrainingSession
    seen = {}

    class Stop(Exception):
        pass

    def fake_session(*a, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(trainer, "TrainingSession", fake_session)
    monkeypatch.setattr(trainer, "setup_logging", lambda rank=0: None)
    F = cli.entry_flags("single_main", ["--clip_grad_norm=0.75", "--skip_nonfinite_grads=True", "--resnet_size=8"])
    F.job_name = None
    with pytest.raises(Stop):
        trainer.train(F, ClusterInfo(device="cpu"))
    assert (seen["clip_grad_norm"], seen["skip_nonfinite_grads"]) == (0.75, True)
    assert (seen["meta"]["clip_grad_norm"], seen["meta"]["skip_nonfinite_grads"]) == (0.75, True)
    # the session hands them to its executor and reports the record; the sharded optimizer refuses
    kw = dict(weight_decay=2e-4, lr_schedule=lr_mod.from_flags(F), use_graph=False)
    sess = TrainingSession(cifar_resnet_v2(8), 2, ClusterInfo(device="cpu"), clip_grad_norm=0.75,
                           skip_nonfinite_grads=True, **kw)
    assert sess.ex.guarding and (sess.ex.clip_grad_norm, sess.ex.skip_nonfinite_grads) == (0.75, True)
    sess.step()
    m = sess.metrics()
    assert m["grad_global_norm"] > 0 and 0 < m["grad_clip_scale"] <= 1 and m["grad_skipped_steps"] == 0
    assert m["grad_clipped_steps"] == int(m["grad_clip_scale"] < 1)
    assert "grad_global_norm" not in TrainingSession(cifar_resnet_v2(8), 2, ClusterInfo(device="cpu"), **kw).metrics()
    with pytest.raises(ValueError, match="shard"):
        TrainingSession(cifar_resnet_v2(8), 2, ClusterInfo(device="cpu"), clip_grad_norm=1.0, shard_optimizer=True,
                        **kw)


def test_defaults_allocate_nothing_and_sharded_range_raises():
    off = _executor(N=2)
    assert not off.guarding and off.guard_record is None and off.guard_partials is None
    assert off.grad_guard_stats() is None
    on = _executor(N=2, skip_nonfinite_grads=True)
    assert on.guarding and on.clip_grad_norm == 0.0 and on.grad_guard_stats()["steps_total"] == 0
    with pytest.raises(RuntimeError, match="global norm"):
        on.sgd_range(0, 64, 1.0)
    off.sgd_range(0, 64, 1.0)


# -- the reference op ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
def test_ref_grad_guard_against_the_fp64_formula(dtype):
    be = RefBackend("cpu", dtype=torch.float64 if dtype == torch.float64 else torch.float32)
    try:
        gen = torch.Generator().manual_seed(5)
        g0 = (torch.randn(1003, generator=gen, dtype=torch.float64) * 3).to(dtype)
        gs = 0.5
        norm = math.sqrt(float(((g0.double() * gs) ** 2).sum()))
        tol = 1e-15 if dtype == torch.float64 else 2.0 ** -22

        def run(g, clip, guard, skip_in=None, rec=None):
            rec = guard_record_tensor() if rec is None else rec
            be.grad_guard(g, gs, clip, guard, skip_in, None, rec)
            return rec, guard_record_read(rec)

        # norm <= c and c == 0: scale 1, g untouched
        for c in (0.0, 2 * norm, 1e30):
            g = g0.clone()
            _, r = run(g, c, True)
            assert r["norm"] == pytest.approx(norm, rel=2.0 ** -22) and r["scale"] == 1.0 and torch.equal(g, g0)
            assert (r["skip"], r["skipped_total"], r["clipped_total"], r["steps_total"]) == (0, 0, 0, 1)
        # norm > c: scale = c / norm, g scaled in place (rounded to its own dtype)
        c = 0.25 * norm
        g = g0.clone()
        rec, r = run(g, c, False)
        assert r["scale"] == pytest.approx(0.25, rel=2.0 ** -21) and r["clipped_total"] == 1 and r["skip"] == 0
        want = g0.double() * (c / max(norm, c))
        if dtype == torch.bfloat16:
            torch.testing.assert_close(g.double(), want, rtol=2.0 ** -8, atol=0)
            assert torch.equal(g, (g0.float() * rec[:2].view(torch.float32)[1]).bfloat16())
        else:
            torch.testing.assert_close(g.double(), want, rtol=tol, atol=0)
        assert float(torch.linalg.vector_norm(g.double() * gs)) == pytest.approx(c, rel=2.0 ** -7 if
                                                                                 dtype == torch.bfloat16 else 1e-6)
        # NaN / Inf: guarded -> skip, g untouched, counted; a clean call on the same record clears skip
        for bad in (float("nan"), float("inf"), float("-inf")):
            gb = g0.clone()
            gb[17] = bad
            g = gb.clone()
            rec, r = run(g, c, True)
            assert (r["skip"], r["scale"], r["skipped_total"], r["clipped_total"]) == (1, 1.0, 1, 0)
            assert not math.isfinite(r["norm"])
            assert torch.equal(torch.nan_to_num(g.double(), 7.0, 8.0, 9.0), torch.nan_to_num(gb.double(), 7.0, 8.0, 9.0))
            _, r = run(g0.clone(), c, True, rec=rec)
            assert (r["skip"], r["skipped_total"], r["clipped_total"], r["steps_total"]) == (0, 1, 1, 2)
            # clipping alone: the gradient is left untouched and the update is not gated
            g = gb.clone()
            _, r = run(g, c, False)
            assert (r["skip"], r["scale"], r["skipped_total"], r["clipped_total"]) == (0, 1.0, 0, 0)
            assert torch.equal(torch.nan_to_num(g.double(), 7.0, 8.0, 9.0), torch.nan_to_num(gb.double(), 7.0, 8.0, 9.0))
        # an incoming skip word is ORed in and is not a non-finite skip
        g = g0.clone()
        rec, r = run(g, c, True, skip_in=torch.tensor([3], dtype=torch.int32))
        assert (r["skip"], r["skipped_total"], r["clipped_total"]) == (1, 0, 0) and torch.equal(g, g0)
        _, r = run(g, c, True, skip_in=torch.tensor([0], dtype=torch.int32), rec=rec)
        assert (r["skip"], r["clipped_total"], r["steps_total"]) == (0, 1, 2)
        with pytest.raises(ValueError, match="clip"):
            be.grad_guard(g0.clone(), gs, -1.0, True, None, None, guard_record_tensor())
    finally:
        RefBackend("cpu")


# -- executor ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer", ["momentum", "lars"])
def test_clipped_update_equals_the_plain_update_on_the_scaled_gradient(optimizer):
    probe = _executor(optimizer=optimizer)
    probe.forward(True)
    probe.backward()
    norm = float(torch.linalg.vector_norm(probe.P.grad.double()))
    a = _executor(optimizer=optimizer, clip_grad_norm=0.5 * norm)
    b = _executor(optimizer=optimizer)
    for ex in (a, b):
        ex.forward(True)
        ex.backward(defer_tail=True)
    assert torch.equal(a.P.grad, b.P.grad)
    a.apply_gradients()
    r = a.grad_guard_stats()
    assert r["norm"] == pytest.approx(norm, rel=1e-6) and r["scale"] == pytest.approx(0.5, rel=1e-6)
    assert (r["clipped_total"], r["skipped_total"], r["skip"], r["steps_total"]) == (1, 0, 0, 1)
    b.P.grad.mul_(a.guard_record[:2].view(torch.float32)[1])
    b.apply_gradients()
    assert torch.equal(a.P.grad, b.P.grad)
    for name in ("master", "momentum", "bn_state"):
        assert torch.equal(getattr(a.P, name), getattr(b.P, name)), name
    # a bound the norm stays under changes nothing
    c = _executor(optimizer=optimizer, clip_grad_norm=1e30)
    d = _executor(optimizer=optimizer)
    for ex in (c, d):
        ex.train_step()
    assert torch.equal(c.P.master, d.P.master) and torch.equal(c.P.momentum, d.P.momentum)
    assert c.grad_guard_stats()["clipped_total"] == 0


@pytest.mark.parametrize("optimizer", ["momentum", "lars"])
def test_nan_gradient_skips_the_step_and_the_next_one_updates(optimizer):
    ex = _executor(optimizer=optimizer, skip_nonfinite_grads=True, ema_decay=0.9, ema_warmup=False)
    ex.train_step()
    names = ("master", "momentum", "ema") + (("lars_trust",) if optimizer == "lars" else ())
    get = lambda n: (ex.lars_trust if n == "lars_trust" else getattr(ex.P, n))  # noqa: E731
    before = {n: get(n).clone() for n in names}
    ex.forward(True)
    ex.backward(defer_tail=True)
    ex.P.grad[ex.P.slots[2].offset] = float("nan")
    ex.apply_gradients()
    for n in names:
        assert torch.equal(get(n), before[n]), n
    r = ex.grad_guard_stats()
    assert (r["skip"], r["skipped_total"], r["steps_total"]) == (1, 1, 2) and math.isnan(r["norm"])
    ex.train_step()
    for n in ("master", "momentum", "ema"):
        assert not torch.equal(get(n), before[n]), n
    r = ex.grad_guard_stats()
    assert (r["skip"], r["skipped_total"], r["steps_total"]) == (0, 1, 3)
    assert bool(torch.isfinite(ex.P.master).all())
    # without the guard the same gradient reaches the weights (clipping alone gates nothing)
    ex2 = _executor(optimizer=optimizer, clip_grad_norm=1.0)
    ex2.forward(True)
    ex2.backward()
    ex2.P.grad[ex2.P.slots[2].offset] = float("nan")
    ex2.apply_gradients()
    assert ex2.grad_guard_stats()["skip"] == 0 and not bool(torch.isfinite(ex2.P.master).all())


def test_incoming_skip_word_reaches_the_update():
    ex = _executor(clip_grad_norm=1e-3)
    ex.forward(True)
    ex.backward()
    w, g = ex.P.master.clone(), ex.P.grad.clone()
    ex.apply_gradients(skip=torch.tensor([1], dtype=torch.int32))
    r = ex.grad_guard_stats()
    assert torch.equal(ex.P.master, w) and torch.equal(ex.P.grad, g)
    assert (r["skip"], r["skipped_total"], r["clipped_total"]) == (1, 0, 0)
    assert int(ex.guard_record[GUARD_SKIP]) == 1
    ex.apply_gradients(skip=torch.tensor([0], dtype=torch.int32))
    assert not torch.equal(ex.P.master, w) and ex.grad_guard_stats()["clipped_total"] == 1


# -- summaries, log line, meta -----------------------------------------------------------------------------
def test_summary_hook_writes_the_four_scalars_and_the_log_reports_a_skip_once(caplog):
    from distributed_resnet_tensorflow_amd.train.hooks import LoggingHook, SummaryHook

    class W:
        def add_scalars(self, step, scalars):
            self.got = (step, scalars)

    class S:
        global_step = 0

    sess, w = S(), W()
    sess.ex = _executor(N=2)
    m = {"cross_entropy": 1.0, "cost": 2.0, "learning_rate": 0.1, "precision": 0.5}
    SummaryHook(w, 1).after_step(sess, 1, lambda: dict(m))
    assert not any(k.startswith("grad/") for k in w.got[1])
    gm = dict(m, grad_global_norm=3.5, grad_clip_scale=0.25, grad_clipped_steps=4, grad_skipped_steps=1)
    SummaryHook(w, 1).after_step(sess, 1, lambda: dict(gm))
    assert {k: v for k, v in w.got[1].items() if k.startswith("grad/")} == \
        {"grad/global_norm": 3.5, "grad/clip_scale": 0.25, "grad/clipped_steps": 4, "grad/skipped_steps": 1}
    hook = LoggingHook(1, 2)
    hook.begin(sess)
    with caplog.at_level("INFO", logger="drn"):
        hook.after_step(sess, 1, lambda: dict(m))
        hook.after_step(sess, 2, lambda: dict(gm))
        hook.after_step(sess, 3, lambda: dict(gm))
        hook.after_step(sess, 4, lambda: dict(gm, grad_skipped_steps=3))
    skips = [r.getMessage() for r in caplog.records if "non-finite" in r.getMessage()]
    assert len(skips) == 2 and "skipped 1 step" in skips[0] and "skipped 2 step" in skips[1] and "3 in total" in skips[1]


def test_checkpoint_meta_round_trips_and_an_old_meta_reads_as_off(tmp_path):
    from distributed_resnet_tensorflow_amd.ckpt.saver import Saver
    from distributed_resnet_tensorflow_amd.train.trainer import _meta, model_spec_from_flags
    F = cli.entry_flags("cifar_main", ["--clip_grad_norm=1.5", "--skip_nonfinite_grads=True", "--resnet_size=8"])
    meta = _meta(F, model_spec_from_flags(F))
    assert (meta["clip_grad_norm"], meta["skip_nonfinite_grads"]) == (1.5, True)
    s = Saver(str(tmp_path))
    new = s.save(1, {"global_step": np.array(1)}, meta)
    old = s.save(2, {"global_step": np.array(2)}, {"optimizer": "lars"})     # (written before the keys)
    got = Saver.restore_meta(new)
    assert (got["clip_grad_norm"], got["skip_nonfinite_grads"]) == (1.5, True)
    for prefix in (old, new + "-missing"):
        got = Saver.restore_meta(prefix)
        assert (got["clip_grad_norm"], got["skip_nonfinite_grads"]) == (0.0, False)
    F0 = cli.entry_flags("cifar_main", ["--resnet_size=8"])
    meta0 = _meta(F0, model_spec_from_flags(F0))
    assert (meta0["clip_grad_norm"], meta0["skip_nonfinite_grads"]) == (0.0, False)


# -- two ranks over gloo -------------------------------------------------------------------------------
STEPS, CLIP = 3, 0.05


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_batches(rank, N):
    g = torch.Generator().manual_seed(100 + rank)
    return [(torch.randn(N, 32, 32, 3, generator=g), torch.randint(0, 10, (N,), generator=g, dtype=torch.int32))
            for _ in range(STEPS)]


def _dp_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from distributed_resnet_tensorflow_amd.parallel.engine import DataParallelEngine
        N = 4
        ex = Executor(cifar_resnet_v2(8), N, RefBackend(), "cpu", seed=1 + rank, clip_grad_norm=CLIP,
                      skip_nonfinite_grads=True)
        eng = DataParallelEngine(ex, bucket_mb=0.05)
        eng.broadcast_parameters()
        recs = []
        for images, labels in _shard_batches(rank, N):
            ex.images[..., :3] = images
            ex.labels.copy_(labels)
            ex.set_lr(0.1)
            ex.forward(True)
            eng.begin_step()
            ex.backward()
            eng.apply_gradients(eng.finish(), 1.0 / world)
            recs.append(ex.guard_record.clone())
        q.put((rank, None, torch.stack(recs), ex.P.master.clone(), ex.P.momentum.clone()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, repr(e) + traceback.format_exc(), None, None, None))


def test_two_ranks_stay_bit_identical_with_clipping_active():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=300) for _ in ps), key=lambda t: t[0])
    for p in ps:
        p.join(timeout=60)
    for rank, err, *_ in res:
        assert err is None, (rank, err)
    (_, _, rec0, w0, m0), (_, _, rec1, w1, m1) = res
    assert torch.equal(rec0, rec1) and torch.equal(w0, w1) and torch.equal(m0, m1)
    last = guard_record_read(rec0[-1])
    assert (last["clipped_total"], last["steps_total"], last["skipped_total"], last["skip"]) == (STEPS, STEPS, 0, 0)
    assert all(0 < guard_record_read(r)["scale"] < 1 for r in rec0)
    assert len({guard_record_read(r)["norm"] for r in rec0}) == STEPS
