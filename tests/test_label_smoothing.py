"""Label smoothing and top-k precision in the classifier head: CPU tests (oracle backend, rank
rule, flags, executor against the autograd oracle, hooks and evaluator through the command-line
entry points). The HIP kernel is covered by tests/test_label_smoothing_gpu.py."""
import json
import math
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from distributed_resnet_tensorflow_amd import cli
from distributed_resnet_tensorflow_amd.flags import FlagsError
from distributed_resnet_tensorflow_amd.models import oracle
from distributed_resnet_tensorflow_amd.models.spec import cifar_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import RefBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entropy of the smoothed target at K = 10, eps = 0.1 (t_y = 0.91, the other nine 0.01): the smoothed
# loss of ANY logits row is at least this
SMOOTHED_TARGET_ENTROPY = -(0.91 * math.log(0.91) + 9 * 0.01 * math.log(0.01))
# the fixed-batch training run shared with tests/test_label_smoothing_gpu.py: N, steps and LR of
# tests/test_executor_gpu.py::test_training_reduces_loss_on_fixed_batch
TRAIN_N, TRAIN_STEPS, TRAIN_LR, TRAIN_EPS = 32, 30, 0.05, 0.1


@pytest.fixture
def ref64():
    """The fp64 oracle backend; the process-wide reference dtype goes back to fp32 afterwards."""
    yield RefBackend("cpu", dtype=torch.float64)
    RefBackend("cpu")


def rank_rule(logits, labels, top_k):
    """The issue's definition, row by row in plain Python on the logits as given:
    rank = #{j : z_j > z_y} + #{j < y : z_j == z_y}; correct_k = rank < top_k, 0 for a NaN z_y."""
    out = []
    for row, y in zip(logits.tolist(), labels.tolist()):
        zy = row[y]
        rank = sum(v > zy for v in row) + sum(v == zy for v in row[:y])
        out.append(int(zy == zy and rank < top_k))
    return torch.tensor(out, dtype=torch.int32)


def fixed_batch(N, seed=11):
    """(images, labels) of the fixed-batch runs: bf16-representable images, CIFAR shapes."""
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(N, 32, 32, 3, generator=g).bfloat16().float()
    labels = torch.randint(0, 10, (N,), generator=g, dtype=torch.int32)
    return images, labels


def check_smoothed_training(ex, steps=TRAIN_STEPS, lr=TRAIN_LR):
    """Every step's mean loss >= H - 1e-3 (a bound that holds for any logits), the excess over H at
    least halves, precision_top_k >= precision at every step."""
    H = SMOOTHED_TARGET_ENTROPY
    losses = []
    for _ in range(steps):
        ex.train_step(lr=lr)
        m = ex.metrics()
        losses.append(m["cross_entropy"])
        assert m["precision_top_k"] >= m["precision"], m
    print("H", H, "losses", losses)
    assert all(v >= H - 1e-3 for v in losses), (H, losses)
    assert losses[-1] - H <= 0.5 * (losses[0] - H), (H, losses)


# -- oracle backend ----------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
def test_ref_softmax_xent_ex_fp64_matches_torch(ref64, eps):
    """Loss per sample and the gradient against F.cross_entropy(label_smoothing=eps) and autograd,
    to 1e-12, logits with a spread of +-20 and a large common offset."""
    g = torch.Generator().manual_seed(3)
    N, K, gs = 7, 13, 0.25
    z = (torch.randn(N, K, generator=g, dtype=torch.float64) * 8 + 300.0).requires_grad_(True)
    labels = torch.tensor([0, K - 1, 3, 3, 7, 12, 1], dtype=torch.int32)
    want = F.cross_entropy(z, labels.long(), label_smoothing=eps, reduction="none")
    grad, = torch.autograd.grad(want.sum(), z)
    dl, probs = torch.zeros(N, K, dtype=torch.float64), torch.zeros(N, K, dtype=torch.float64)
    loss = torch.zeros(N, dtype=torch.float64)
    correct, correct_k = torch.zeros(N, dtype=torch.int32), torch.zeros(N, dtype=torch.int32)
    ref64.softmax_xent_ex(z.detach(), labels, gs, dl, loss, correct, probs=probs, smoothing=eps, top_k=1,
                          correct_k=correct_k)
    assert float((loss - want.detach()).abs().max()) <= 1e-12
    assert float((dl - gs * grad).abs().max()) <= 1e-12
    assert float((probs - torch.softmax(z.detach(), 1)).abs().max()) <= 1e-12
    assert torch.equal(correct, (z.detach().argmax(1) == labels.long()).int()) and torch.equal(correct_k, correct)
    # the optional outputs may be left out
    loss2 = torch.zeros(N, dtype=torch.float64)
    ref64.softmax_xent_ex(z.detach(), labels, gs, None, loss2, None, smoothing=eps)
    assert torch.equal(loss, loss2)


def test_ref_softmax_xent_ex_at_zero_smoothing_is_softmax_xent(ref):
    g = torch.Generator().manual_seed(4)
    N, K = 5, 10
    z, labels = torch.randn(N, K, generator=g), torch.randint(0, K, (N,), generator=g, dtype=torch.int32)
    outs = []
    for ex in (False, True):
        dl, loss, c = torch.zeros(N, K), torch.zeros(N), torch.zeros(N, dtype=torch.int32)
        (ref.softmax_xent_ex if ex else ref.softmax_xent)(z, labels, 0.2, dl, loss, c)
        outs.append((dl, loss, c))
    assert torch.allclose(outs[0][0], outs[1][0], atol=1e-7) and torch.allclose(outs[0][1], outs[1][1], atol=1e-6)
    assert torch.equal(outs[0][2], outs[1][2])


def test_rank_rule_on_hand_made_rows(ref):
    nan = float("nan")
    rows = [
        ([2.0] * 8, 0),                                   # all equal, label 0: rank 0
        ([2.0] * 8, 4),                                   # all equal: four earlier ties, rank 4
        ([2.0] * 8, 7),                                   # all equal, label K-1: rank 7
        ([1.0, 5.0, 5.0, 5.0, 0.0, 0.0, 0.0, 0.0], 2),    # tied with an earlier and a later index: rank 1
        ([9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0], 0),    # label 0 the maximum
        ([9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0], 7),    # label K-1 the minimum: rank 7
        ([9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0], 4),    # rank 4: in the top 5, not the top 4
        ([9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0], 5),    # rank 5: just outside the top 5
        ([1.0, nan, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0], 1),    # a NaN label logit never counts
        ([1.0, nan, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0], 2),    # a NaN elsewhere compares false: rank 0
    ]
    z = torch.tensor([r for r, _ in rows])
    labels = torch.tensor([y for _, y in rows], dtype=torch.int32)
    want = {1: [1, 0, 0, 0, 1, 0, 0, 0, 0, 1],
            5: [1, 1, 0, 1, 1, 0, 1, 0, 0, 1],
            8: [1, 1, 1, 1, 1, 1, 1, 1, 0, 1],    # k >= K: every row with a non-NaN label logit
            100: [1, 1, 1, 1, 1, 1, 1, 1, 0, 1]}
    for k, expect in want.items():
        loss, ck = torch.zeros(len(rows)), torch.full((len(rows),), -1, dtype=torch.int32)
        ref.softmax_xent_ex(z, labels, 1.0, None, loss, None, smoothing=0.1, top_k=k, correct_k=ck)
        assert ck.tolist() == expect, (k, ck.tolist())
        assert torch.equal(ck, rank_rule(z, labels, k))
    for bad in (dict(smoothing=1.0), dict(smoothing=-0.1), dict(top_k=0)):
        with pytest.raises(ValueError):
            ref.softmax_xent_ex(z, labels, 1.0, None, torch.zeros(len(rows)), None, **bad)


# -- flags, checkpoint meta ----------------------------------------------------------------------------
def test_flags_defaults_ranges_and_reach_the_executor(monkeypatch):
    F_ = cli.entry_flags("cifar_main", [])
    assert (F_.label_smoothing, F_.top_k) == (0.0, 0)
    F_ = cli.entry_flags("imagenet_main", ["--label_smoothing=0.1", "--top_k", "5"])
    assert (F_.label_smoothing, F_.top_k) == (0.1, 5)
    assert cli.entry_flags("cifar_eval_main", ["--top_k=5"]).top_k == 5
    for bad in (["--label_smoothing=1.0"], ["--label_smoothing=-0.01"], ["--label_smoothing=1.5"], ["--top_k=-1"]):
        with pytest.raises(FlagsError):
            cli.entry_flags("cifar_main", bad)
    assert cli.entry_flags("cifar_main", ["--label_smoothing=0.999", "--top_k=1"]).top_k == 1
    # trainer.train hands both to the TrainingSession, which hands them to its Executor
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
    F_ = cli.entry_flags("single_main", ["--label_smoothing=0.2", "--top_k=3", "--resnet_size=8"])
    F_.job_name = None
    with pytest.raises(Stop):
        trainer.train(F_, ClusterInfo(device="cpu"))
    assert (seen["label_smoothing"], seen["top_k"]) == (0.2, 3)
    sess = TrainingSession(cifar_resnet_v2(8), 2, ClusterInfo(device="cpu"), weight_decay=2e-4,
                           lr_schedule=lr_mod.from_flags(F_), use_graph=False, label_smoothing=0.2, top_k=3)
    assert (sess.ex.label_smoothing, sess.ex.top_k) == (0.2, 3) and sess.ex.correct_k.shape == (2,)


def test_checkpoint_meta_records_label_smoothing(tmp_path):
    from distributed_resnet_tensorflow_amd.ckpt.saver import Saver
    from distributed_resnet_tensorflow_amd.train.trainer import _meta, model_spec_from_flags
    F_ = cli.entry_flags("cifar_main", ["--label_smoothing=0.1", "--resnet_size=8"])
    meta = _meta(F_, model_spec_from_flags(F_))
    assert meta["label_smoothing"] == 0.1 and meta["optimizer"] == "momentum"
    s = Saver(str(tmp_path))
    new = s.save(1, {"global_step": torch.tensor(1).numpy()}, meta)
    old = s.save(2, {"global_step": torch.tensor(2).numpy()}, {"optimizer": "lars"})  # (written before the key)
    assert Saver.restore_meta(new)["label_smoothing"] == 0.1
    assert Saver.restore_meta(old)["label_smoothing"] == 0.0 and Saver.restore_meta(old)["optimizer"] == "lars"
    assert Saver.restore_meta(str(tmp_path / "model.ckpt-404"))["label_smoothing"] == 0.0


# -- executor ----------------------------------------------------------------------------------------
def _executor(N=8, seed=1, **kw):
    ex = Executor(cifar_resnet_v2(8), N, RefBackend(), "cpu", seed=seed, **kw)
    images, labels = fixed_batch(N)
    ex.images.zero_()
    ex.images[..., :3] = images
    ex.labels.copy_(labels)
    return ex


def test_executor_smoothed_step_matches_oracle():
    """tests/test_executor.py::_check (fp32, tol 1e-4) with label_smoothing = 0.1 on both sides: logits,
    mean loss, every parameter gradient, the moving statistics."""
    tol, eps = 1e-4, 0.1
    spec = cifar_resnet_v2(8)
    ex = _executor(label_smoothing=eps, top_k=5)
    p, st = oracle.params_from_store(ex.P), oracle.state_from_store(ex.P)
    ex.forward(train=True)
    ex.backward()
    logits, xent, _ = oracle.loss_fn(spec, p, st, ex.images, ex.labels.long(), label_smoothing=eps)
    xent.backward()
    assert torch.allclose(logits, ex.logits, atol=tol * 10, rtol=tol * 10)
    assert abs(xent.item() - ex.loss_vec.mean().item()) < tol * 10
    plain = F.cross_entropy(logits.detach(), ex.labels.long()).item()
    assert abs(xent.item() - plain) > 100 * tol  # (the smoothing term is far above the tolerance)
    for s in ex.P.slots:
        g_ex, g_or = ex.P.to_tf(s.name, buf=ex.P.grad, dtype=torch.float32), p[s.name].grad
        err = ((g_ex - g_or).norm() / (g_or.norm() + 1e-30)).item()
        assert err < tol, (s.name, err)
    for k in st:
        m, v = ex.P.moving(k)
        assert torch.allclose(m, st[k][0], atol=tol) and torch.allclose(v, st[k][1], atol=tol * 10)
    assert torch.equal(ex.correct_k, rank_rule(ex.logits, ex.labels, 5))
    # the evaluation forward reports the plain cross-entropy (and still fills correct_k)
    ex.correct_k.fill_(-1)
    ex.forward(train=False)
    want = F.cross_entropy(ex.logits, ex.labels.long(), reduction="none")
    assert torch.allclose(ex.loss_vec, want, atol=1e-5)
    assert torch.equal(ex.correct_k, rank_rule(ex.logits, ex.labels, 5))


def test_executor_metrics_and_argument_checks():
    a, b, c = _executor(N=4), _executor(N=4, top_k=1), _executor(N=4, top_k=5, label_smoothing=0.1)
    for ex in (a, b, c):
        ex.forward(train=True)
    assert a.correct_k is None and b.correct_k is None and c.correct_k.dtype == torch.int32
    keys = {"cross_entropy", "cost", "precision"}
    assert set(a.metrics()) == keys and set(b.metrics()) == keys
    m = c.metrics()
    assert set(m) == keys | {"precision_top_k"} and 0.0 <= m["precision"] <= m["precision_top_k"] <= 1.0
    assert m["cross_entropy"] >= SMOOTHED_TARGET_ENTROPY - 1e-3
    assert torch.equal(a.loss_vec, b.loss_vec) and torch.equal(a.dlogits, b.dlogits)  # (top_k = 1: today's call)
    for bad in (dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(top_k=-1), dict(top_k=2.5)):
        with pytest.raises(ValueError):
            Executor(cifar_resnet_v2(8), 2, RefBackend(), "cpu", **bad)


def test_default_forward_calls_todays_softmax_xent():
    """label_smoothing = 0 and top_k < 2: forward() calls be.softmax_xent with today's arguments and
    never softmax_xent_ex; otherwise the other way round (evaluation: smoothing 0)."""
    calls = []

    class Spy(RefBackend):
        def softmax_xent(self, *a, **kw):
            calls.append(("plain", len(a), dict(kw)))
            return super().softmax_xent(*a, **kw)

        def softmax_xent_ex(self, *a, **kw):
            calls.append(("ex", len(a), dict(kw)))
            return super().softmax_xent_ex(*a, **kw)

    for kw in ({}, dict(top_k=1)):
        ex = Executor(cifar_resnet_v2(8), 2, Spy(), "cpu", **kw)
        ex.forward(train=True)
        ex.forward(train=False)
    assert calls == [("plain", 6, {})] * 4
    del calls[:]
    ex = Executor(cifar_resnet_v2(8), 2, Spy(), "cpu", label_smoothing=0.1)
    ex.forward(train=True)
    ex.forward(train=False)  # (evaluation without top-k: the plain kernel)
    ex = Executor(cifar_resnet_v2(8), 2, Spy(), "cpu", label_smoothing=0.1, top_k=5)
    ex.forward(train=True)
    ex.forward(train=False)
    assert [c[0] for c in calls] == ["ex", "plain", "ex", "ex"]
    assert [c[2].get("smoothing") for c in calls] == [0.1, None, 0.1, 0.0]
    assert calls[2][2]["top_k"] == 5 and calls[0][2]["top_k"] == 1 and calls[0][2]["correct_k"] is None


def test_oracle_executor_smoothed_training_on_fixed_batch():
    """The settings of the GPU training test hold on the reference executor first."""
    check_smoothed_training(_executor(N=TRAIN_N, seed=7, label_smoothing=TRAIN_EPS, top_k=5))


def test_summary_and_logging_hooks_default_and_top_k(caplog):
    from distributed_resnet_tensorflow_amd.train.hooks import LoggingHook, SummaryHook

    class W:
        def add_scalars(self, step, scalars):
            self.got = (step, scalars)

    class S:
        global_step = 0

    base = {"cross_entropy": 1.0, "cost": 2.0, "learning_rate": 0.1, "precision": 0.5}
    for top_k, extra in ((0, {}), (5, {"precision_top_k": 0.75})):
        sess, w = S(), W()
        sess.ex = _executor(N=2, top_k=top_k)
        SummaryHook(w, 1).after_step(sess, 1, lambda: dict(base, **extra))
        want = {"cross_entropy": 1.0, "cost": 2.0, "learning_rate": 0.1, "Precision": 0.5}
        if top_k:
            want["Precision@5"] = 0.75
        assert w.got == (1, want)
        h = LoggingHook(1, 2)
        h.begin(sess)
        with caplog.at_level("INFO", logger="drn"):
            caplog.clear()
            h.after_step(sess, 1, lambda: dict(base, **extra))
        line = caplog.records[-1].getMessage()
        mid = ", precision@5 = 0.75000" if top_k else ""
        assert re.fullmatch(r"step = 1, loss = 2\.00000, precision = 0\.50000" + re.escape(mid) +
                            r", lr = 0\.1, \(\S+ steps/sec, \S+ images/sec\)", line), line


# -- command-line entry points (the CPU path of tests/test_cli_e2e.py, at its sizes) ----------------------
def _run(args):
    env = dict(os.environ)
    env.setdefault("PYTHONPATH", REPO)
    return subprocess.run([sys.executable] + args, cwd=REPO, capture_output=True, text=True, timeout=600, env=env)


def _tags(logdir):
    from distributed_resnet_tensorflow_amd.utils.events import read_events
    tags = set()
    for fn in os.listdir(logdir):
        if fn.startswith("events.out.tfevents"):
            for _, _, sc in read_events(os.path.join(logdir, fn)):
                tags |= set(sc)
    return tags


@pytest.fixture(scope="module")
def cifar_dir(tmp_path_factory):
    from distributed_resnet_tensorflow_amd.data.cifar import write_fake_cifar
    d = tmp_path_factory.mktemp("cifar")
    write_fake_cifar(str(d), 64)
    return str(d)


LOG_LINE = (r"step = 10, loss = \d+\.\d{5}, precision = \d\.\d{5}%s, lr = \S+, "
            r"\(\d+\.\d\d steps/sec, \d+\.\d images/sec\)")
EVAL_LINE = r"loss: \d+\.\d{3}, precision: \d\.\d{3}, best precision: \d\.\d{3}%s"


@pytest.mark.parametrize("top_k", [0, 5])
def test_cli_train_and_eval_lines_and_summary_tags(cifar_dir, tmp_path, top_k):
    """Defaults: the training log line, the evaluator's line, both sets of summary tags and
    best_precision.json are exactly what they were; --top_k=5 (with --label_smoothing=0.1) adds
    precision@5 to each."""
    ck, tr, ev = str(tmp_path / "ck"), str(tmp_path / "train_ev"), str(tmp_path / "eval_ev")
    extra = ["--top_k=5"] if top_k else []
    r = _run(["resnet_single.py", "--train_steps=12", f"--train_data_path={cifar_dir}", f"--log_root={ck}",
              f"--eval_dir={tr}", "--resnet_size=8", "--batch_size=16", "--log_every_n_steps=5",
              "--save_summaries_steps=5"] + extra + (["--label_smoothing=0.1"] if top_k else []))
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if "step = 10," in ln][0]
    line = line[line.index("step = 10,"):]
    assert re.fullmatch(LOG_LINE % (r", precision@5 = \d\.\d{5}" if top_k else ""), line), line
    tags = {"cross_entropy", "cost", "learning_rate", "Precision"}
    assert _tags(tr) == (tags | {"Precision@5"} if top_k else tags)
    meta = json.load(open(os.path.join(ck, "model.ckpt-12.meta")))
    assert meta["label_smoothing"] == (0.1 if top_k else 0.0)
    r = _run(["resnet_cifar_eval.py", "--mode=eval", "--eval_once=True", f"--eval_data_path={cifar_dir}",
              f"--log_root={ck}", f"--eval_dir={ev}", "--resnet_size=8", "--eval_batch_count=2"] + extra)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if "best precision:" in ln][0]
    line = line[line.index("loss:"):]
    assert re.fullmatch(EVAL_LINE % (r", precision@5: \d\.\d{3}" if top_k else ""), line), line
    tags = {"Precision", "Best Precision"}
    assert _tags(ev) == (tags | {"Precision@5", "Best Precision@5"} if top_k else tags)
    best = json.load(open(os.path.join(ev, "best_precision.json")))
    if top_k:
        assert set(best) == {"best_precision", "step", "precision_top_k", "best_precision_top_k", "top_k"}
        assert best["top_k"] == 5 and best["best_precision"] <= best["precision_top_k"] <= 1.0
    else:
        assert set(best) == {"best_precision", "step"} and best["step"] == 12
