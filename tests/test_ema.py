"""Weight EMA (tf.train.ExponentialMovingAverage fused into the optimizer update): CPU tests on the
oracle backend -- flags, the warm-up table, checkpoints and resume, a two-rank gloo run, the
evaluator's --eval_ema. The HIP kernels are covered by tests/test_ema_gpu.py."""
import json
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
from distributed_resnet_tensorflow_amd.ops.backend import RefBackend, lars_table
from distributed_resnet_tensorflow_amd.runtime.executor import Executor
from distributed_resnet_tensorflow_amd.runtime.state import EMA_SUFFIX, NoEmaInCheckpoint, export_state, import_state

EMA = EMA_SUFFIX  # "/ExponentialMovingAverage"


def _executor(N=4, seed=1, data_seed=7, **kw):
    ex = Executor(cifar_resnet_v2(8), N, RefBackend(), "cpu", seed=seed, **kw)
    g = torch.Generator().manual_seed(data_seed)
    ex.images.zero_()
    ex.images[..., :3] = torch.randn(N, 32, 32, 3, generator=g)
    ex.labels.copy_(torch.randint(0, 10, (N,), generator=g, dtype=torch.int32))
    return ex


# -- flags ---------------------------------------------------------------------------------------------
def test_flags_defaults_and_validation(monkeypatch):
    F = cli.entry_flags("cifar_main", [])
    assert (F.ema_decay, F.ema_warmup, F.eval_ema) == (0.0, True, False)
    F = cli.entry_flags("imagenet_main", ["--ema_decay=0.9999", "--ema_warmup=False"])
    assert (F.ema_decay, F.ema_warmup) == (0.9999, False)
    assert cli.entry_flags("cifar_eval_main", ["--eval_ema=True"]).eval_ema is True
    assert cli.entry_flags("cifar_main", ["--ema_decay=0"]).ema_decay == 0.0
    for bad in (["--ema_decay=1.0"], ["--ema_decay=-0.1"], ["--ema_decay=1.5"], ["--ema_decay=0.9", "--model=lrnet"]):
        with pytest.raises(FlagsError):
            cli.entry_flags("cifar_main", bad)
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError, match="ema_decay"):
            Executor(cifar_resnet_v2(8), 2, RefBackend(), "cpu", ema_decay=bad)
    # trainer.train hands both to the TrainingSession, and the checkpoint meta records the decay
    from distributed_resnet_tensorflow_amd.parallel.cluster import ClusterInfo
    from distributed_resnet_tensorflow_amd.train import trainer
    seen = {}

    class Stop(Exception):
        pass

    def fake_session(*a, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(trainer, "TrainingSession", fake_session)
    monkeypatch.setattr(trainer, "setup_logging", lambda rank=0: None)
    F = cli.entry_flags("single_main", ["--ema_decay=0.99", "--ema_warmup=False", "--resnet_size=8"])
    F.job_name = None
    with pytest.raises(Stop):
        trainer.train(F, ClusterInfo(device="cpu"))
    assert (seen["ema_decay"], seen["ema_warmup"]) == (0.99, False) and seen["meta"]["ema_decay"] == 0.99


# -- semantics -----------------------------------------------------------------------------------------
# d_t = min(0.999, (1 + t) / (10 + t)), written out by hand
WARMUP_TABLE = {0: 0.1, 1: 2.0 / 11.0, 9: 10.0 / 19.0, 1000: 1001.0 / 1010.0}


def test_warmup_table_and_the_device_scalar():
    ex = _executor(N=2, ema_decay=0.999)
    for t, d in WARMUP_TABLE.items():
        assert ex.ema_decay_at(t) == pytest.approx(d, rel=1e-15)
        ex.set_ema_decay(t)
        assert float(ex.ema_decay_t) == np.float32(d)
    assert WARMUP_TABLE[1000] < 0.999 and ex.ema_decay_at(10**6) == 0.999
    flat = _executor(N=2, ema_decay=0.999, ema_warmup=False)
    assert [flat.ema_decay_at(t) for t in WARMUP_TABLE] == [0.999] * 4
    off = _executor(N=2)
    assert off.P.ema is None and off.ema_decay_t is None
    off.set_ema_decay(3)  # a no-op, not an error


@pytest.mark.parametrize("optimizer", ["momentum", "lars"])
def test_oracle_update_follows_the_formula_and_leaves_the_weights_alone(optimizer):
    """Three steps: P.ema is the recurrence over the per-step weights; master / momentum / BN state
    are bit for bit those of the run without the EMA; shadows start equal to the variables."""
    a = _executor(optimizer=optimizer)
    b = _executor(optimizer=optimizer, ema_decay=0.999)
    assert torch.equal(b.P.ema, b.P.master) and b.P.ema.data_ptr() != b.P.master.data_ptr()
    ref = b.P.master.double().clone()
    for t in range(3):
        for ex in (a, b):
            ex.P.global_step = t
            ex.train_step(lr=0.1)
        d = float(np.float32(min(0.999, (1.0 + t) / (10.0 + t))))   # (the kernel reads an fp32 scalar)
        ref -= (1.0 - d) * (ref - b.P.master.double())
    for x, y in ((a.P.master, b.P.master), (a.P.momentum, b.P.momentum), (a.P.bn_state, b.P.bn_state)):
        assert torch.equal(x, y)
    assert not torch.equal(b.P.ema, b.P.master)
    torch.testing.assert_close(b.P.ema.double(), ref, rtol=0, atol=1e-6)


def test_skip_word_and_ranges_and_fp64_oracle():
    be = RefBackend("cpu", dtype=torch.float64)
    try:
        g = torch.Generator().manual_seed(3)
        w, m, gr, e = (torch.randn(64, generator=g, dtype=torch.float64) for _ in range(4))
        lr, d = torch.tensor([0.1], dtype=torch.float64), torch.tensor([0.75], dtype=torch.float32)
        w0, e0 = w.clone(), e.clone()
        be.sgd_momentum(w, m, gr, None, lr, 0.9, 1e-4, 1.0, torch.tensor([1], dtype=torch.int32), ema=e, ema_decay_t=d)
        assert torch.equal(w, w0) and torch.equal(e, e0)
        be.sgd_momentum(w[:32], m[:32], gr[:32], None, lr, 0.9, 1e-4, 1.0, None, ema=e[:32], ema_decay_t=d)
        assert torch.equal(e[32:], e0[32:])
        torch.testing.assert_close(e[:32], e0[:32] - 0.25 * (e0[:32] - w[:32]), rtol=0, atol=1e-15)
    finally:
        RefBackend("cpu")
    # LARS: only the slots of the call are averaged
    ex = _executor(optimizer="lars", ema_decay=0.5, ema_warmup=False)
    ex.forward(True)
    ex.backward()
    ex.set_lr(0.1)
    before = ex.P.ema.clone()
    s1 = ex.P.slots[1]
    ex._update(s1.offset, ex.P.total, ex.P.grad, 1.0)
    assert torch.equal(before[:s1.offset], ex.P.ema[:s1.offset])
    torch.testing.assert_close(ex.P.ema[s1.offset:], 0.5 * (before + ex.P.master)[s1.offset:])
    assert lars_table(ex.P).n == len(ex.P.slots)


def test_ema_weights_context_evaluates_the_average_and_restores_training_state():
    ex = _executor(ema_decay=0.5, ema_warmup=False)
    for _ in range(2):
        ex.train_step(lr=0.2)
    master = ex.P.master.clone()
    ex.forward(train=False)
    plain = float(ex.loss_vec.double().mean())
    with ex.ema_weights():
        assert torch.equal(ex.P.master, ex.P.ema)
        ex.forward(train=False)
        avg = float(ex.loss_vec.double().mean())
    assert torch.equal(ex.P.master, master) and avg != plain
    ex.forward(train=False)
    assert float(ex.loss_vec.double().mean()) == plain
    with pytest.raises(RuntimeError, match="no weight EMA"):
        with _executor(N=2).ema_weights():
            pass


def test_summary_hook_writes_the_effective_decay():
    from distributed_resnet_tensorflow_amd.train.hooks import SummaryHook

    class W:
        def add_scalars(self, step, scalars):
            self.got = (step, scalars)

    class S:
        pass

    sess, w = S(), W()
    sess.ex = _executor(N=2)
    m = {"cross_entropy": 1.0, "cost": 2.0, "learning_rate": 0.1, "precision": 0.5}
    SummaryHook(w, 1).after_step(sess, 1, lambda: dict(m))
    assert "ema/decay" not in w.got[1]
    SummaryHook(w, 1).after_step(sess, 1, lambda: dict(m, ema_decay=0.1))
    assert w.got[1]["ema/decay"] == 0.1


# -- checkpoints ---------------------------------------------------------------------------------------
def test_export_import_names_layout_and_seeding(caplog):
    ex = _executor(ema_decay=0.9)
    for _ in range(2):
        ex.train_step(lr=0.1)
    t = export_state(ex)
    trainable = {s.name for s in ex.P.slots}
    assert {k[:-len(EMA)] for k in t if k.endswith(EMA)} == trainable      # every trainable variable ...
    assert not any("moving_" in k and k.endswith(EMA) for k in t)           # ... and nothing else
    assert t["conv2d/kernel" + EMA].shape == t["conv2d/kernel"].shape == (3, 3, 3, 16)   # TF layout (HWIO)
    assert not np.array_equal(t["conv2d/kernel" + EMA], t["conv2d/kernel"])
    assert not any(k.endswith(EMA) for k in export_state(_executor(N=2)))
    # round trip
    b = _executor(seed=9, ema_decay=0.9)
    import_state(b, t)
    assert torch.equal(b.P.ema, ex.P.ema) and torch.equal(b.P.master, ex.P.master)
    # a checkpoint without EMA: the shadows are seeded from the restored weights, with a warning
    plain = {k: v for k, v in t.items() if not k.endswith(EMA)}
    c = _executor(seed=9, ema_decay=0.9)
    with caplog.at_level("WARNING", logger="drn"):
        import_state(c, plain)
    assert torch.equal(c.P.ema, c.P.master) and torch.equal(c.P.master, ex.P.master)
    assert any("ExponentialMovingAverage" in r.getMessage() for r in caplog.records)
    # an executor without EMA ignores the extra keys
    d = _executor(seed=9)
    import_state(d, t)
    assert d.P.ema is None and torch.equal(d.P.master, ex.P.master)
    # use_ema: the variables take the averages; a checkpoint without them is an error
    import_state(d, t, use_ema=True)
    assert torch.equal(d.P.master, ex.P.ema)
    with pytest.raises(NoEmaInCheckpoint, match="ExponentialMovingAverage"):
        import_state(d, plain, use_ema=True)


@pytest.fixture(scope="module")
def cifar_dir(tmp_path_factory):
    from distributed_resnet_tensorflow_amd.data.cifar import write_fake_cifar
    d = tmp_path_factory.mktemp("cifar")
    write_fake_cifar(str(d), 64)
    return str(d)


def _train(cifar_dir, ck, steps, extra=()):
    from distributed_resnet_tensorflow_amd.parallel.cluster import ClusterInfo
    from distributed_resnet_tensorflow_amd.train import trainer
    F = cli.entry_flags("single_main", [f"--train_steps={steps}", f"--train_data_path={cifar_dir}",
                                        f"--log_root={ck}", "--resnet_size=8", "--batch_size=8",
                                        "--log_every_n_steps=100", "--save_summaries_steps=0"] + list(extra))
    F.job_name = None
    assert trainer.train(F, ClusterInfo(device="cpu")) == 0


def _ckpt(ck):
    from distributed_resnet_tensorflow_amd.ckpt.saver import Saver, latest_checkpoint
    prefix = latest_checkpoint(ck)
    return prefix, Saver.restore(prefix)


@pytest.fixture(scope="module")
def ema_run(cifar_dir, tmp_path_factory):
    """Six steps with --ema_decay=0.9 in one go (shared by the resume and the evaluator tests)."""
    ck = str(tmp_path_factory.mktemp("ema_run") / "ck")
    _train(cifar_dir, ck, 6, ["--ema_decay=0.9"])
    return ck


def test_training_checkpoint_has_the_names_and_the_meta(ema_run):
    prefix, t = _ckpt(ema_run)
    assert prefix.endswith("model.ckpt-6")
    trainable = [k for k in t if k + "/Momentum" in t]
    assert len(trainable) == 26 and all(k + EMA in t for k in trainable)
    assert sum(k.endswith(EMA) for k in t) == len(trainable)
    assert json.load(open(prefix + ".meta"))["ema_decay"] == 0.9
    from distributed_resnet_tensorflow_amd.ckpt.saver import Saver
    assert Saver.restore_meta(prefix)["ema_decay"] == 0.9
    assert Saver.restore_meta(prefix + "-missing")["ema_decay"] == 0.0   # an absent key means 0


def test_resume_gives_the_uninterrupted_ema(cifar_dir, ema_run, tmp_path):
    """A run stopped after 3 of 6 steps and resumed from its checkpoint ends with the EMA (and the
    weights) of the uninterrupted run: the shadows, the step count behind the warm-up decay and the
    input position all come back from the checkpoint."""
    ck = str(tmp_path / "ck")
    _train(cifar_dir, ck, 3, ["--ema_decay=0.9"])
    assert _ckpt(ck)[0].endswith("model.ckpt-3")
    _train(cifar_dir, ck, 6, ["--ema_decay=0.9"])
    _, got = _ckpt(ck)
    _, want = _ckpt(ema_run)
    for k in want:
        if k.endswith(EMA) or k + EMA in want:
            assert np.array_equal(got[k], want[k]), k


def test_resume_without_ema_in_the_checkpoint_seeds_the_shadows(cifar_dir, tmp_path):
    ck = str(tmp_path / "ck")
    _train(cifar_dir, ck, 2)
    _, t = _ckpt(ck)
    assert not any(k.endswith(EMA) for k in t)
    _train(cifar_dir, ck, 2, ["--ema_decay=0.9"])     # restores at step 2, trains nothing, saves
    _, t2 = _ckpt(ck)
    for k in t:
        if k + "/Momentum" in t:
            assert np.array_equal(t2[k + EMA], t[k]) and np.array_equal(t2[k], t[k]), k


# -- evaluator -----------------------------------------------------------------------------------------
def _evaluate(cifar_dir, ck, ev, extra=()):
    from distributed_resnet_tensorflow_amd.train.evaluator import evaluate
    F = cli.entry_flags("cifar_eval_main", ["--eval_once=True", f"--eval_data_path={cifar_dir}", f"--log_root={ck}",
                                            f"--eval_dir={ev}", "--resnet_size=8", "--eval_batch_count=2"] + list(extra))
    return evaluate(F, eval_batch_size=16)


def test_evaluator_eval_ema(cifar_dir, ema_run, tmp_path):
    plain = _evaluate(cifar_dir, ema_run, str(tmp_path / "ev_plain"))[-1]
    avg = _evaluate(cifar_dir, ema_run, str(tmp_path / "ev_ema"), ["--eval_ema=True"])[-1]
    assert "ema" not in json.load(open(tmp_path / "ev_plain" / "best_precision.json"))
    assert json.load(open(tmp_path / "ev_ema" / "best_precision.json"))["ema"] is True
    # the loss of an executor loaded with the EMA tensors, over the same two batches
    from distributed_resnet_tensorflow_amd.parallel.cluster import ClusterInfo
    from distributed_resnet_tensorflow_amd.train.trainer import WEIGHT_DECAY, make_feeder
    _, t = _ckpt(ema_run)
    swapped = {k: (t[k + EMA] if k + EMA in t else v) for k, v in t.items()}
    ex = Executor(cifar_resnet_v2(8), 16, RefBackend(), "cpu", weight_decay=WEIGHT_DECAY["cifar10"])
    import_state(ex, swapped)
    F = cli.entry_flags("cifar_eval_main", [f"--eval_data_path={cifar_dir}", "--resnet_size=8"])
    feeder = make_feeder(F, ex, ClusterInfo(device="cpu"), False, batch=16)
    loss, n = 0.0, 0
    try:
        for _ in range(2):
            assert feeder.next()
            ex.forward(train=False)
            loss += float(ex.loss_vec.double().sum())
            n += ex.N
    finally:
        feeder.close()
    want = loss / n + ex.wd * float(ex.P.trainable_l2())
    assert avg["loss"] == pytest.approx(want, rel=1e-9)
    assert avg["loss"] != plain["loss"] and abs(avg["loss"] - plain["loss"]) > 1e-6 * plain["loss"]


def test_evaluator_eval_ema_raises_without_ema(cifar_dir, tmp_path):
    ck = str(tmp_path / "ck")
    _train(cifar_dir, ck, 1)
    with pytest.raises(NoEmaInCheckpoint, match="--ema_decay"):
        _evaluate(cifar_dir, ck, str(tmp_path / "ev"), ["--eval_ema=True"])


# -- two ranks over gloo -------------------------------------------------------------------------------
STEPS, DECAY = 3, 0.9


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


def _single_process_reference(world, N):
    """The same steps in one process on the concatenated batch: the gradient of every shard of the
    batch (per-replica BatchNorm, the reference's semantics, as in tests/test_distributed.py) from
    the same weights, their mean applied by one optimizer update with the EMA."""
    exs = [Executor(cifar_resnet_v2(8), N, RefBackend(), "cpu", seed=1, ema_decay=DECAY if r == 0 else 0.0)
           for r in range(world)]
    data = [_shard_batches(r, N) for r in range(world)]
    main = exs[0]
    for t in range(STEPS):
        total = torch.zeros_like(main.P.grad)
        for r, ex in enumerate(exs):
            ex.P.master.copy_(main.P.master)
            ex.sync_weights()
            ex.images[..., :3] = data[r][t][0]
            ex.labels.copy_(data[r][t][1])
            ex.forward(True)
            ex.backward()
            total += ex.P.grad
        main.set_lr(0.1)
        main.set_ema_decay(t)
        main.apply_gradients(grad_scale=1.0 / world, grad=total)
    return main.P.ema.clone(), main.P.master.clone()


def _dp_worker(rank, world, port, shard, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from distributed_resnet_tensorflow_amd.parallel.engine import DataParallelEngine
        N = 4
        ex = Executor(cifar_resnet_v2(8), N, RefBackend(), "cpu", seed=1 + rank, ema_decay=DECAY)
        eng = DataParallelEngine(ex, bucket_mb=0.05, shard_optimizer=shard)
        assert eng.zero1 == shard
        eng.broadcast_parameters()          # (different seeds on purpose: P.ema is broadcast too)
        assert torch.equal(ex.P.ema, ex.P.master)
        for t, (images, labels) in enumerate(_shard_batches(rank, N)):
            ex.images[..., :3] = images
            ex.labels.copy_(labels)
            ex.set_lr(0.1)
            ex.set_ema_decay(t)
            ex.forward(True)
            eng.begin_step()
            ex.backward()
            eng.apply_gradients(eng.finish(), 1.0 / world)
        eng.gather_state()
        gathered = [torch.zeros_like(ex.P.ema) for _ in range(world)]
        dist.all_gather(gathered, ex.P.ema)
        same = all(torch.equal(gathered[0], t) for t in gathered)
        q.put((rank, same, ex.P.ema.clone(), ex.P.master.clone()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, repr(e) + traceback.format_exc(), None, None))


@pytest.mark.parametrize("shard", [False, True], ids=["allreduce", "optimizer_sharding"])
def test_two_rank_ema_is_equal_on_both_ranks_and_matches_one_process(shard):
    world, N = 2, 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_dp_worker, args=(r, world, port, shard, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = [q.get(timeout=300) for _ in ps]
    for p in ps:
        p.join(timeout=60)
    ema1, w1 = _single_process_reference(world, N)
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()  # noqa: E731
    for rank, same, ema, w in res:
        assert same is True, same
        assert not torch.equal(ema, w)
        # (tests/test_distributed.py's bound for weights trained two ways: relative error < 1e-6)
        assert rel(w, w1) < 1e-6 and rel(ema, ema1) < 1e-6, (rank, rel(w, w1), rel(ema, ema1))
