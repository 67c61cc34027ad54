"""Mixup / CutMix: CPU tests (the host sampler, the oracle backend's mix_pairs / softmax_xent_mix, the
executor against the autograd oracle, flags, checkpoint meta, feeder resume, the command-line entry
point). The HIP kernels are covered by tests/test_mix_gpu.py, which shares the helpers below."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_label_smoothing import _run, _tags, fixed_batch, rank_rule

from distributed_resnet_tensorflow_amd import cli
from distributed_resnet_tensorflow_amd.data.mix import MixSampler
from distributed_resnet_tensorflow_amd.flags import FlagsError
from distributed_resnet_tensorflow_amd.models import oracle
from distributed_resnet_tensorflow_amd.models.spec import cifar_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import MIX_REC, RefBackend, mix_identity, mix_table_tensor
from distributed_resnet_tensorflow_amd.runtime.executor import Executor

# the fixed-mixed-batch training run shared with tests/test_mix_gpu.py
TRAIN_N, TRAIN_STEPS, TRAIN_LR, TRAIN_EPS = 32, 30, 0.05, 0.1


@pytest.fixture
def ref64():
    """The fp64 oracle backend; the process-wide reference dtype goes back to fp32 afterwards."""
    yield RefBackend("cpu", dtype=torch.float64)
    RefBackend("cpu")


# -- helpers (shared with the GPU file) ----------------------------------------------------------------
def make_table(recs, labels=None):
    """MIX_REC table from (w, lam, y0, x0, y1, x1) tuples; label_b = the labels reversed."""
    t = mix_identity(len(recs))
    for i, r in enumerate(recs):
        t[i] = tuple(r) + (0, 0)
    if labels is not None:
        t["label_b"] = np.asarray(labels)[::-1]
    return t


def torch_mix(images, table):
    """The contract in plain torch, pixel boxes by slicing, in the images' dtype: (N, H, W, C)."""
    N = images.shape[0]
    out = images.clone()
    for n in range(N):
        m = N - 1 - n
        if m == n:
            continue
        r = table[n]
        w = float(r["w"])
        out[n] = w * images[n] + (1.0 - w) * images[m] if w != 1.0 else images[n]
        out[n, r["y0"]:r["y1"], r["x0"]:r["x1"]] = images[m, r["y0"]:r["y1"], r["x0"]:r["x1"]]
    return out


def mixed_loss(logits, labels, table, eps):
    """Per-sample lam CE(z, ya, eps) + (1 - lam) CE(z, yb, eps) with F.cross_entropy, in logits' dtype."""
    lam = torch.from_numpy(table["lam"].copy()).to(logits.dtype)
    ya, yb = labels.long(), torch.from_numpy(table["label_b"].astype(np.int64))
    ca = F.cross_entropy(logits, ya, label_smoothing=eps, reduction="none")
    cb = F.cross_entropy(logits, yb, label_smoothing=eps, reduction="none")
    return lam * ca + (1.0 - lam) * cb


def mixed_target_entropy(labels, table, eps, K):
    """Mean entropy of the mixed targets t = (1 - eps)(lam e_ya + (1 - lam) e_yb) + eps / K: the mixed
    loss of ANY logits is at least this."""
    hs = []
    for ya, r in zip(np.asarray(labels).tolist(), table):
        t = np.full(K, eps / K)
        t[ya] += (1.0 - eps) * float(r["lam"])
        t[int(r["label_b"])] += (1.0 - eps) * (1.0 - float(r["lam"]))
        hs.append(-sum(v * math.log(v) for v in t if v > 0))
    return float(np.mean(hs))


def dominant(labels, table):
    lab = torch.as_tensor(np.asarray(labels)).int()
    return torch.where(torch.from_numpy(table["lam"].copy()) >= 0.5, lab, torch.from_numpy(table["label_b"].copy()))


def training_case(kind, N=TRAIN_N):
    """(images fp32 [N,32,32,3], labels, table) of the fixed mixed batch: (a) Mixup with lam = 0.7
    everywhere, (b) CutMix with the box [8, 24) x [4, 20) everywhere, lam = 0.75."""
    images, labels = fixed_batch(N)
    rec = (0.7, 0.7, 0, 0, 0, 0) if kind == "mixup" else (1.0, 0.75, 8, 4, 24, 20)
    return images, labels, make_table([rec] * N, labels.numpy())


def load_mixed(ex, images, labels, table):
    """Mix the batch through the executor's own backend (in place) and hand it the table."""
    ex.images.zero_()
    ex.images[..., :3] = images.to(ex.images.device, ex.images.dtype)
    ex.labels.copy_(labels.to(ex.labels.device))
    t = mix_table_tensor(table).to(ex.images.device)
    ex.be.mix_pairs(ex.images, ex.images, t)
    ex.set_mix(t)


def check_mixed_training(ex, labels, table, steps=TRAIN_STEPS, lr=TRAIN_LR, eps=TRAIN_EPS):
    """Every step's mean loss >= H - 1e-3 (H = the mean entropy of the mixed targets, a bound that
    holds for any logits); the excess over H at least halves."""
    H = mixed_target_entropy(labels.numpy(), table, eps, 10)
    losses = []
    for _ in range(steps):
        ex.train_step(lr=lr)
        losses.append(ex.metrics()["cross_entropy"])
    print("H", H, "losses", losses, "excess ratio", (losses[-1] - H) / (losses[0] - H))
    assert all(v >= H - 1e-3 for v in losses), (H, losses)
    assert losses[-1] - H <= 0.5 * (losses[0] - H), (H, losses)


# -- 1. MixSampler -------------------------------------------------------------------------------------
def test_sampler_is_counter_based():
    kw = dict(mixup_alpha=0.4, cutmix_alpha=1.0, per_sample=True, seed=5)
    labels = np.arange(8, dtype=np.int32)
    a = MixSampler(8, 32, 32, rank=1, **kw)
    b = MixSampler(8, 32, 32, rank=1, **kw)
    for i in (0, 3, 1000):
        assert a.draw(i, labels).tobytes() == b.draw(i, labels).tobytes()
    assert a.draw(3, labels).tobytes() == a.draw(3, labels).tobytes()   # (no state between draws)
    assert a.draw(3, labels).tobytes() != a.draw(4, labels).tobytes()
    assert a.draw(3, labels).tobytes() != MixSampler(8, 32, 32, rank=0, **kw).draw(3, labels).tobytes()
    assert a.draw(3, labels).tobytes() != MixSampler(8, 32, 32, rank=1, **dict(kw, seed=6)).draw(3, labels).tobytes()
    t = a.draw(0, labels)
    assert t.dtype == MIX_REC and MIX_REC.itemsize == 32 and t.shape == (8,)
    assert t["label_b"].tolist() == labels[::-1].tolist()
    assert a.draw(0)["label_b"].tolist() == [0] * 8


@pytest.mark.parametrize("H,W", [(32, 32), (7, 9), (224, 224)])
def test_sampler_records(H, W):
    N = 16
    cut = MixSampler(N, H, W, cutmix_alpha=1.0, per_sample=True, seed=1)
    mup = MixSampler(N, H, W, mixup_alpha=0.2, per_sample=True, seed=1)
    both = MixSampler(N, H, W, mixup_alpha=0.2, cutmix_alpha=1.0, per_sample=True, seed=1)
    kinds = set()
    for i in range(40):
        for s in (cut, mup, both):
            t = s.draw(i)
            assert ((t["lam"] >= 0) & (t["lam"] <= 1)).all()
            assert ((0 <= t["y0"]) & (t["y0"] <= t["y1"]) & (t["y1"] <= H)).all()
            assert ((0 <= t["x0"]) & (t["x0"] <= t["x1"]) & (t["x1"] <= W)).all()
            area = (t["y1"] - t["y0"]).astype(np.int64) * (t["x1"] - t["x0"])
            is_cut = t["w"] == 1.0
            if s is cut:
                assert is_cut.all()
            if s is mup:
                assert (area == 0).all()
            # CutMix: lam is exactly the kept area; Mixup: empty box and w == lam
            assert (t["lam"][is_cut] == (1.0 - area[is_cut] / (H * W)).astype(np.float32)).all()
            assert (area[~is_cut] == 0).all() and (t["w"][~is_cut] == t["lam"][~is_cut]).all()
            if s is both:
                kinds |= {"cut" if c else "mix" for c in is_cut}
    assert kinds == {"cut", "mix"}


def test_sampler_prob_switch_and_batch_mode():
    labels = np.arange(8, dtype=np.int32)
    ident = mix_identity(8)
    ident["label_b"] = labels[::-1]
    off = MixSampler(8, 32, 32, mixup_alpha=0.2, prob=0.0)
    assert all(off.draw(i, labels).tobytes() == ident.tobytes() for i in range(5))
    half = MixSampler(8, 32, 32, mixup_alpha=0.2, prob=0.5)
    mixed = [half.draw(i, labels).tobytes() != ident.tobytes() for i in range(200)]
    assert 60 <= sum(mixed) <= 140   # (p = 0.5, 200 draws: 5.6 sigma)
    assert (MixSampler(8, 32, 32, mixup_alpha=1.0, cutmix_alpha=1.0, switch_prob=1.0).draw(0)["w"] == 1.0).all()
    assert (MixSampler(8, 32, 32, mixup_alpha=1.0, cutmix_alpha=1.0, switch_prob=0.0).draw(0)["y1"] == 0).all()
    per = MixSampler(8, 32, 32, mixup_alpha=1.0, per_sample=True).draw(0)
    batch = MixSampler(8, 32, 32, mixup_alpha=1.0, cutmix_alpha=1.0, per_sample=False)
    assert len(set(per["lam"].tolist())) > 1
    for i in range(10):
        t = batch.draw(i)
        for k in ("w", "lam", "y0", "x0", "y1", "x1"):
            assert len(set(t[k].tolist())) == 1, (i, k)
    for bad in (dict(), dict(mixup_alpha=-1.0), dict(mixup_alpha=1.0, prob=1.5), dict(cutmix_alpha=1.0, switch_prob=-0.1)):
        with pytest.raises(ValueError):
            MixSampler(8, 32, 32, **bad)


# -- 2. RefBackend.mix_pairs ----------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W", [(1, 8, 8), (5, 7, 9), (4, 32, 32)])
def test_ref_mix_pairs_fp64(ref64, N, H, W):
    g = torch.Generator().manual_seed(N * 100 + H)
    src = torch.zeros(N, H, W, 8, dtype=torch.float64)
    src[..., :3] = torch.randn(N, H, W, 3, generator=g, dtype=torch.float64)
    recs = [(0.3, 0.3, 0, 0, 0, 0), (1.0, 0.5, 1, 2, H - 1, W - 2), (1.0, 1.0, 0, 0, 0, 0), (0.0, 0.0, 0, 0, 0, 0),
            (1.0, 0.0, 0, 0, H, W)]
    table = make_table([recs[i % len(recs)] for i in range(N)])
    want = torch_mix(src, table)
    dst = torch.full_like(src, -7.0)
    ref64.mix_pairs(src, dst, mix_table_tensor(table))
    assert float((dst - want).abs().max()) <= 1e-15
    # boxes and w in {0, 1} move values unchanged
    for n in range(N):
        if float(table[n]["w"]) in (0.0, 1.0):
            assert torch.equal(dst[n], want[n]), n
    inplace = src.clone()
    ref64.mix_pairs(inplace, inplace, mix_table_tensor(table))
    assert torch.equal(inplace, dst)
    if N % 2:
        assert torch.equal(dst[N // 2], src[N // 2])
    ident = src.clone()
    ref64.mix_pairs(ident, ident, mix_table_tensor(mix_identity(N)))
    assert torch.equal(ident, src)
    assert torch.equal(dst[..., 3:], torch.zeros_like(dst[..., 3:]))


# -- 3. RefBackend.softmax_xent_mix -----------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
def test_ref_softmax_xent_mix_fp64_matches_torch(ref64, eps):
    """Loss and gradient against lam CE(z, ya, eps) + (1 - lam) CE(z, yb, eps) from F.cross_entropy and
    autograd, to 1e-12; logits with a spread of +-20 and a large common offset."""
    g = torch.Generator().manual_seed(3)
    N, K, gs = 7, 13, 0.25
    z = (torch.randn(N, K, generator=g, dtype=torch.float64) * 8 + 300.0).requires_grad_(True)
    labels = torch.tensor([0, K - 1, 3, 3, 7, 12, 1], dtype=torch.int32)
    lams = [0.7, 0.25, 0.5, 1.0, 0.0, 0.999, 0.3]
    table = make_table([(l, l, 0, 0, 0, 0) for l in lams], labels.numpy())
    want = mixed_loss(z, labels, table, eps)
    grad, = torch.autograd.grad(want.sum(), z)
    dl, probs = torch.zeros(N, K, dtype=torch.float64), torch.zeros(N, K, dtype=torch.float64)
    loss = torch.zeros(N, dtype=torch.float64)
    correct, correct_k = torch.zeros(N, dtype=torch.int32), torch.zeros(N, dtype=torch.int32)
    ref64.softmax_xent_mix(z.detach(), labels, mix_table_tensor(table), gs, dl, loss, correct, probs=probs,
                           smoothing=eps, top_k=3, correct_k=correct_k)
    assert float((loss - want.detach()).abs().max()) <= 1e-12
    assert float((dl - gs * grad).abs().max()) <= 1e-12
    assert float((probs - torch.softmax(z.detach(), 1)).abs().max()) <= 1e-12
    dom = dominant(labels.numpy(), table)
    assert torch.equal(correct, rank_rule(z.detach(), dom, 1)) and torch.equal(correct_k, rank_rule(z.detach(), dom, 3))
    loss2 = torch.zeros(N, dtype=torch.float64)
    ref64.softmax_xent_mix(z.detach(), labels, mix_table_tensor(table), gs, None, loss2, None, smoothing=eps)
    assert torch.equal(loss, loss2)
    for bad in (dict(smoothing=1.0), dict(top_k=0)):
        with pytest.raises(ValueError):
            ref64.softmax_xent_mix(z.detach(), labels, mix_table_tensor(table), gs, None, loss2, None, **bad)


def test_ref_softmax_xent_mix_at_lam_one_is_softmax_xent_ex(ref64):
    g = torch.Generator().manual_seed(4)
    N, K = 6, 10
    z = torch.randn(N, K, generator=g, dtype=torch.float64)
    labels = torch.randint(0, K, (N,), generator=g, dtype=torch.int32)
    table = mix_identity(N)
    table["label_b"] = [3, -1, K, 10 ** 6, 0, 9]    # (never looked at when lam == 1)
    outs = []
    for mix in (False, True):
        dl, loss = torch.zeros(N, K, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
        c, ck = torch.zeros(N, dtype=torch.int32), torch.zeros(N, dtype=torch.int32)
        if mix:
            ref64.softmax_xent_mix(z, labels, mix_table_tensor(table), 0.5, dl, loss, c, smoothing=0.1, top_k=5,
                                   correct_k=ck)
        else:
            ref64.softmax_xent_ex(z, labels, 0.5, dl, loss, c, smoothing=0.1, top_k=5, correct_k=ck)
        outs.append((dl, loss, c, ck))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_dominant_label_rule_on_hand_made_rows(ref):
    rows = [
        ([9.0, 8.0, 7.0, 6.0], 0, 1, 0.7),    # own label dominant and the maximum
        ([9.0, 8.0, 7.0, 6.0], 0, 1, 0.3),    # partner's label dominant: rank 1
        ([9.0, 8.0, 7.0, 6.0], 1, 0, 0.3),    # partner's label dominant and the maximum
        ([9.0, 8.0, 7.0, 6.0], 1, 0, 0.5),    # lam == 0.5: the own label (rank 1)
        ([9.0, 8.0, 7.0, 6.0], 0, 3, 0.5),    # lam == 0.5: the own label (rank 0)
        ([9.0, 8.0, 7.0, 6.0], 2, 2, 0.2),    # ya == yb: rank 2 either way
        ([5.0, 5.0, 5.0, 5.0], 3, 1, 0.4),    # ties: the partner's label 1 has one earlier tie
    ]
    z = torch.tensor([r[0] for r in rows])
    labels = torch.tensor([r[1] for r in rows], dtype=torch.int32)
    table = make_table([(r[3], r[3], 0, 0, 0, 0) for r in rows])
    table["label_b"] = [r[2] for r in rows]
    want = {1: [1, 0, 1, 0, 1, 0, 0], 2: [1, 1, 1, 1, 1, 0, 1], 3: [1, 1, 1, 1, 1, 1, 1]}
    for k, expect in want.items():
        loss = torch.zeros(len(rows))
        c, ck = torch.full((len(rows),), -1, dtype=torch.int32), torch.full((len(rows),), -1, dtype=torch.int32)
        ref.softmax_xent_mix(z, labels, mix_table_tensor(table), 1.0, None, loss, c, smoothing=0.1, top_k=k,
                             correct_k=ck)
        assert ck.tolist() == expect, (k, ck.tolist())
        assert c.tolist() == want[1]
        assert torch.equal(ck, rank_rule(z, dominant(labels.numpy(), table), k))
    # ya == yb: the target is the plain smoothed one-hot
    l1, l2 = torch.zeros(1), torch.zeros(1)
    ref.softmax_xent_mix(z[5:6], labels[5:6], mix_table_tensor(table[5:6]), 1.0, None, l1, None, smoothing=0.1)
    ref.softmax_xent_ex(z[5:6], labels[5:6], 1.0, None, l2, None, smoothing=0.1)
    assert torch.allclose(l1, l2, atol=1e-6)


# -- 4. / 5. executor --------------------------------------------------------------------------------------
def _executor(N=8, seed=1, **kw):
    return Executor(cifar_resnet_v2(8), N, RefBackend(), "cpu", seed=seed, **kw)


def _per_sample_table(N, labels, seed=2):
    """Both kinds in one table, drawn per sample, with an identity record and a full box among them."""
    t = MixSampler(N, 32, 32, mixup_alpha=0.4, cutmix_alpha=1.0, per_sample=True, seed=seed).draw(0, labels)
    assert set((t["w"] == 1.0).tolist()) == {True, False}
    return t


def test_executor_mixed_step_matches_oracle():
    """tests/test_executor.py::_check (fp32, tol 1e-4) on a mixed batch: logits, mean loss, every
    parameter gradient, the moving statistics; the oracle's mixed loss is computed here from its logits."""
    tol, eps, N = 1e-4, 0.1, 8
    spec = cifar_resnet_v2(8)
    ex = _executor(N, label_smoothing=eps, top_k=5, mix=True)
    images, labels = fixed_batch(N)
    table = _per_sample_table(N, labels.numpy())
    load_mixed(ex, images, labels, table)
    assert torch.allclose(ex.images[..., :3], torch_mix(images, table), atol=1e-6)
    p, st = oracle.params_from_store(ex.P), oracle.state_from_store(ex.P)
    ex.forward(train=True)
    ex.backward()
    logits, plain, _ = oracle.loss_fn(spec, p, st, ex.images, ex.labels.long(), label_smoothing=eps)
    xent = mixed_loss(logits, ex.labels, table, eps).mean()
    xent.backward()
    assert torch.allclose(logits, ex.logits, atol=tol * 10, rtol=tol * 10)
    assert abs(xent.item() - ex.loss_vec.mean().item()) < tol * 10
    assert abs(xent.item() - plain.item()) > 100 * tol   # (the mixing term is far above the tolerance)
    for s in ex.P.slots:
        g_ex, g_or = ex.P.to_tf(s.name, buf=ex.P.grad, dtype=torch.float32), p[s.name].grad
        err = ((g_ex - g_or).norm() / (g_or.norm() + 1e-30)).item()
        assert err < tol, (s.name, err)
    for k in st:
        m, v = ex.P.moving(k)
        assert torch.allclose(m, st[k][0], atol=tol) and torch.allclose(v, st[k][1], atol=tol * 10)
    dom = dominant(labels.numpy(), table)
    assert torch.equal(ex.correct, rank_rule(ex.logits, dom, 1))
    assert torch.equal(ex.correct_k, rank_rule(ex.logits, dom, 5))
    assert set(ex.metrics()) == {"cross_entropy", "cost", "precision", "precision_top_k"}
    # evaluation never mixes: the plain cross-entropy against ex.labels
    ex.forward(train=False)
    want = F.cross_entropy(ex.logits, ex.labels.long(), reduction="none")
    assert torch.allclose(ex.loss_vec, want, atol=1e-5)
    assert torch.equal(ex.correct_k, rank_rule(ex.logits, ex.labels, 5))


def test_defaults_are_untouched_and_set_mix_checks():
    calls = []

    class Spy(RefBackend):
        def mix_pairs(self, *a, **kw):
            calls.append("mix_pairs")
            return super().mix_pairs(*a, **kw)

        def softmax_xent_mix(self, *a, **kw):
            calls.append("softmax_xent_mix")
            return super().softmax_xent_mix(*a, **kw)

        def softmax_xent(self, *a, **kw):
            calls.append("softmax_xent")
            return super().softmax_xent(*a, **kw)

    for kw in ({}, dict(mix=False)):
        ex = Executor(cifar_resnet_v2(8), 2, Spy(), "cpu", **kw)
        ex.train_step(lr=0.1)
        ex.forward(train=False)
        assert getattr(ex, "mix_table", None) is None
        with pytest.raises(RuntimeError):
            ex.set_mix(mix_identity(2))
    assert calls == ["softmax_xent"] * 4
    del calls[:]
    ex = Executor(cifar_resnet_v2(8), 2, Spy(), "cpu", mix=True)
    assert ex.mix_table.dtype == torch.int32 and tuple(ex.mix_table.shape) == (2, 8)
    assert ex.mix_table.numpy().tobytes() == mix_identity(2).tobytes()
    ex.forward(train=True)
    ex.forward(train=False)
    assert calls == ["softmax_xent_mix", "softmax_xent"]
    with pytest.raises(ValueError):
        ex.set_mix(mix_identity(3))
    t = make_table([(0.25, 0.25, 0, 0, 0, 0), (1.0, 0.5, 0, 0, 16, 32)], [4, 6])
    ex.set_mix(t)
    assert ex.mix_table.numpy().tobytes() == t.tobytes()


# -- 6. flags, wiring, resume ------------------------------------------------------------------------------
def test_flags_defaults_ranges_and_wiring(monkeypatch):
    F_ = cli.entry_flags("cifar_main", [])
    assert (F_.mixup_alpha, F_.cutmix_alpha, F_.mix_prob, F_.mix_switch_prob, F_.mix_per_sample) == \
        (0.0, 0.0, 1.0, 0.5, False)
    F_ = cli.entry_flags("imagenet_main", ["--mixup_alpha=0.2", "--cutmix_alpha", "1.0", "--mix_prob=0.9",
                                           "--mix_switch_prob=0.25", "--mix_per_sample"])
    assert (F_.mixup_alpha, F_.cutmix_alpha, F_.mix_prob, F_.mix_switch_prob, F_.mix_per_sample) == \
        (0.2, 1.0, 0.9, 0.25, True)
    for bad in (["--mixup_alpha=-0.1"], ["--cutmix_alpha=-1"], ["--mix_prob=1.5"], ["--mix_prob=-0.1"],
                ["--mix_switch_prob=2"], ["--mixup_alpha=0.2", "--model=lrnet"]):
        with pytest.raises(FlagsError):
            cli.entry_flags("cifar_main", bad)
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
    for args, want in ((["--cutmix_alpha=1.0"], True), (["--mixup_alpha=0.2"], True), ([], False)):
        F_ = cli.entry_flags("single_main", args + ["--resnet_size=8"])
        F_.job_name = None
        with pytest.raises(Stop):
            trainer.train(F_, ClusterInfo(device="cpu"))
        assert seen["mix"] is want
    sess = TrainingSession(cifar_resnet_v2(8), 2, ClusterInfo(device="cpu"), weight_decay=2e-4,
                           lr_schedule=lr_mod.from_flags(F_), use_graph=False, mix=True)
    assert sess.ex.mix and sess.ex.mix_table is not None
    sess.ex.set_mix(make_table([(0.25, 0.25, 0, 0, 0, 0), (1.0, 0.5, 0, 0, 16, 32)]))
    sess.ex.forward(train=True)
    assert sess.metrics()["mix_lam"] == 0.375
    # the sampler takes the cluster rank, the flags and the executor's geometry
    F_ = cli.entry_flags("cifar_main", ["--mixup_alpha=0.2", "--cutmix_alpha=1.0", "--mix_prob=0.9",
                                        "--mix_switch_prob=0.25", "--mix_per_sample", "--seed=4"])
    s = trainer.make_mix_sampler(F_, sess.ex, ClusterInfo(device="cpu", rank=3, world=4))
    assert (s.N, s.H, s.W, s.mixup_alpha, s.cutmix_alpha, s.prob, s.switch_prob, s.per_sample, s.seed, s.rank) == \
        (2, 32, 32, 0.2, 1.0, 0.9, 0.25, True, 4, 3)
    assert trainer.make_mix_sampler(cli.entry_flags("cifar_main", []), sess.ex, ClusterInfo(device="cpu")) is None


def test_checkpoint_meta_records_the_alphas(tmp_path):
    from distributed_resnet_tensorflow_amd.ckpt.saver import Saver
    from distributed_resnet_tensorflow_amd.train.trainer import _meta, model_spec_from_flags
    F_ = cli.entry_flags("cifar_main", ["--mixup_alpha=0.2", "--cutmix_alpha=1.0", "--resnet_size=8"])
    meta = _meta(F_, model_spec_from_flags(F_))
    assert (meta["mixup_alpha"], meta["cutmix_alpha"]) == (0.2, 1.0)
    s = Saver(str(tmp_path))
    new = s.save(1, {"global_step": torch.tensor(1).numpy()}, meta)
    old = s.save(2, {"global_step": torch.tensor(2).numpy()}, {"optimizer": "lars"})  # (written before the keys)
    assert (Saver.restore_meta(new)["mixup_alpha"], Saver.restore_meta(new)["cutmix_alpha"]) == (0.2, 1.0)
    assert (Saver.restore_meta(old)["mixup_alpha"], Saver.restore_meta(old)["cutmix_alpha"]) == (0.0, 0.0)


@pytest.fixture(scope="module")
def cifar_dir(tmp_path_factory):
    from distributed_resnet_tensorflow_amd.data.cifar import write_fake_cifar
    d = tmp_path_factory.mktemp("cifar")
    write_fake_cifar(str(d), 64)
    return str(d)


def test_cifar_feeder_mixes_and_resumes(cifar_dir):
    """A CifarFeeder restored from state() after 3 batches produces the same images and tables as the
    uninterrupted one; its images are the mix of an unmixed feeder's; the evaluation feeder never mixes."""
    from distributed_resnet_tensorflow_amd.parallel.cluster import ClusterInfo
    from distributed_resnet_tensorflow_amd.train.trainer import make_feeder
    args = [f"--train_data_path={cifar_dir}", f"--eval_data_path={cifar_dir}", "--resnet_size=8", "--seed=3"]
    Fm = cli.entry_flags("cifar_main", args + ["--mixup_alpha=0.4", "--cutmix_alpha=1.0", "--mix_per_sample",
                                               "--mix_prob=0.7"])
    F0 = cli.entry_flags("cifar_main", args)
    cluster = ClusterInfo(device="cpu")

    def run(F_, n, mix, state=None):
        ex = _executor(8, mix=mix)
        fd = make_feeder(F_, ex, cluster, True, state)
        out = []
        try:
            for _ in range(n):
                assert fd.next()
                out.append((ex.images.clone(), ex.labels.clone(),
                            ex.mix_table.clone() if mix else None, fd.state()))
        finally:
            fd.close()
        return out

    full, plain = run(Fm, 6, True), run(F0, 6, False)
    assert [o[3]["mix_batch"] for o in full] == [1, 2, 3, 4, 5, 6] and "mix_batch" not in plain[0][3]
    assert {k: v for k, v in full[2][3].items() if k != "mix_batch"} == plain[2][3]
    sampler = MixSampler(8, 32, 32, mixup_alpha=0.4, cutmix_alpha=1.0, prob=0.7, per_sample=True, seed=3)
    for i, (m, p) in enumerate(zip(full, plain)):
        table = sampler.draw(i, p[1].numpy())
        assert m[2].numpy().tobytes() == table.tobytes(), i
        assert torch.equal(m[1], p[1])
        assert torch.allclose(m[0], torch_mix(p[0], table), atol=1e-6), i
        if (table["w"] == 1.0).all() and (table["y1"] == table["y0"]).all():   # an unmixed batch (prob 0.3)
            assert torch.equal(m[0], p[0])
    resumed = run(Fm, 3, True, full[2][3])
    for a, b in zip(full[3:], resumed):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]
    # evaluation feeders never mix
    ex = _executor(8, mix=True)
    fd = make_feeder(Fm, ex, cluster, False)
    try:
        assert fd.next() and fd.mix is None and "mix_batch" not in fd.state()
        assert ex.mix_table.numpy().tobytes() == mix_identity(8).tobytes()
    finally:
        fd.close()


def test_synthetic_feeder_does_not_compound():
    from distributed_resnet_tensorflow_amd.train.feeder import SyntheticFeeder
    ex = _executor(4, mix=True)
    sampler = MixSampler(4, 32, 32, mixup_alpha=0.4, cutmix_alpha=1.0, per_sample=True, seed=1)
    fd = SyntheticFeeder(ex, seed=5, mix=sampler)
    pristine, labels = ex.images.clone(), ex.labels.clone()
    for _ in range(3):
        fd.next()
    table = sampler.draw(2, labels.numpy())
    assert torch.allclose(ex.images, torch_mix(pristine, table), atol=1e-6)
    assert ex.mix_table.numpy().tobytes() == table.tobytes() and fd.state() == {"mix_batch": 3}
    assert torch.equal(fd.pristine, pristine)
    plain = SyntheticFeeder(_executor(4), seed=5)
    assert plain.next() and plain.state() == {}


# -- 7. training on a fixed mixed batch -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixup", "cutmix"])
def test_oracle_executor_mixed_training_on_fixed_batch(kind):
    """Reference executor, N 32, 30 steps, lr 0.05, eps 0.1: every step's mean loss >= H - 1e-3 and the
    excess over H at least halves (the run ends at an excess ratio of 0.063 for Mixup with lam = 0.7
    and 0.081 for CutMix with the box [8, 24) x [4, 20); the factor 2 leaves more than 6x margin)."""
    images, labels, table = training_case(kind)
    assert table["lam"][0] == np.float32(0.7 if kind == "mixup" else 1 - 16 * 16 / 1024)
    ex = _executor(TRAIN_N, seed=7, label_smoothing=TRAIN_EPS, mix=True)
    load_mixed(ex, images, labels, table)
    check_mixed_training(ex, labels, table)


# -- 8. command line -----------------------------------------------------------------------------------------
def test_cli_mixed_training_run(cifar_dir, tmp_path):
    """resnet_single.py with Mixup + CutMix + label smoothing, at the sizes of
    tests/test_label_smoothing.py::test_cli_train_and_eval_lines_and_summary_tags: exit 0, the .meta
    keys, the mix/lam tag; the default run's tags are what they were."""
    base = ["resnet_single.py", "--train_steps=12", f"--train_data_path={cifar_dir}", "--resnet_size=8",
            "--batch_size=16", "--log_every_n_steps=5", "--save_summaries_steps=5"]
    tags = {"cross_entropy", "cost", "learning_rate", "Precision"}
    for name, extra in (("mix", ["--mixup_alpha=0.2", "--cutmix_alpha=1.0", "--label_smoothing=0.1"]), ("plain", [])):
        ck, tr = str(tmp_path / f"ck_{name}"), str(tmp_path / f"ev_{name}")
        r = _run(base + [f"--log_root={ck}", f"--eval_dir={tr}"] + extra)
        assert r.returncode == 0, r.stdout + r.stderr
        meta = json.load(open(os.path.join(ck, "model.ckpt-12.meta")))
        if extra:
            assert (meta["mixup_alpha"], meta["cutmix_alpha"], meta["label_smoothing"]) == (0.2, 1.0, 0.1)
            assert _tags(tr) == tags | {"mix/lam"}
            rows = [json.loads(ln) for ln in open(os.path.join(ck, "metrics.jsonl"))]
            assert all(0.0 <= row["mix_lam"] <= 1.0 for row in rows) and rows
        else:
            assert (meta["mixup_alpha"], meta["cutmix_alpha"]) == (0.0, 0.0)
            assert _tags(tr) == tags
