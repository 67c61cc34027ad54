"""Label smoothing and top-k precision on the GPU: the fused HIP kernel (csrc/kernels/head.hip
softmax_xent_ex_kernel) against an fp64 reference on the same fp32 logits and against the existing
softmax_xent kernel, and the executor's eager / graph / plan steps with label_smoothing / top_k."""
import pytest
import torch
import torch.nn.functional as F

from test_label_smoothing import TRAIN_EPS, TRAIN_N, check_smoothed_training, fixed_batch, rank_rule
from test_ops_gpu import rel

from distributed_resnet_tensorflow_amd.models.spec import cifar_resnet_v2
from distributed_resnet_tensorflow_amd.ops import _lib
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend, RefBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

# rows shorter than a wave, not a multiple of 64 / 256, the benchmark's class count, one row past
# the 2048 classes the kernel keeps in registers (the re-reading variant)
SHAPES = [(3, 10), (5, 100), (4, 1001), (2, 257), (2, 2500)]
# rel() (tests/test_ops_gpu.py) of the EXISTING drn_softmax_xent against the fp64 reference on the
# same fp32 logits, worst of loss / dlogits / probs over SHAPES x {random, small-integer} logits,
# measured on an MI355X: 1.6471e-07 (probs at 4 x 1001, random logits; loss at most 7.7e-08, dlogits
# 8.8e-08; test_existing_kernel_figure prints the figures of the run). The new kernel, which adds one
# more reduction and two more multiply-adds per element, is allowed 4x that: 6.6e-07. (Its own worst
# figures in that run: probs 1.6471e-07 -- the same bits --, loss 1.03e-07, dlogits 8.9e-08.)
MEASURED_REL = 1.65e-7
BOUND = 4 * MEASURED_REL


def _logits(N, K, kind):
    g = torch.Generator().manual_seed(1000 * N + K)
    z = torch.randn(N, K, generator=g) * 4.0
    if kind == "ints":  # small integers: ties are common (and the label is often among them)
        z = z.round().clamp_(-3, 3)
    labels = torch.randint(0, K, (N,), generator=g, dtype=torch.int32)
    labels[0], labels[-1] = 0, K - 1
    return z, labels


def _reference(z, labels, eps, gs):
    """loss, dlogits, probs in fp64 from the issue's formulas on the fp32 logits."""
    K = z.shape[1]
    lp = torch.log_softmax(z.double(), 1)
    t = (1.0 - eps) * F.one_hot(labels.long(), K).double() + eps / K
    return -(t * lp).sum(1), (lp.exp() - t) * gs, lp.exp()


@pytest.fixture(scope="module")
def cases():
    """{(N, K, kind): (logits, labels, gs, {eps: (loss, dlogits, probs)}, {k: correct_k})}, computed
    once on the CPU and never modified."""
    out = {}
    for N, K in SHAPES:
        for kind in ("randn", "ints"):
            z, labels = _logits(N, K, kind)
            gs = 1.0 / N
            out[(N, K, kind)] = (z, labels, gs, {eps: _reference(z, labels, eps, gs) for eps in (0.0, 0.1)},
                                 {k: rank_rule(z, labels, k) for k in (1, 5, K)})
    return out


def _run(hip, z, labels, gs, eps=0.0, k=1, ex=True, dlogits=True, probs=True, correct=True, correct_k=True):
    """One launch on device copies; returns dict of the outputs asked for (CPU tensors)."""
    N, K = z.shape
    zd, ld = z.cuda(), labels.cuda()
    o = {"loss": torch.full((N,), -7.0, device="cuda")}
    if dlogits:
        o["dlogits"] = torch.full((N, K), -7.0, device="cuda")
    if probs:
        o["probs"] = torch.full((N, K), -7.0, device="cuda")
    if correct:
        o["correct"] = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    if ex:
        if correct_k:
            o["correct_k"] = torch.full((N,), -7, dtype=torch.int32, device="cuda")
        hip.softmax_xent_ex(zd, ld, gs, o.get("dlogits"), o["loss"], o.get("correct"), probs=o.get("probs"),
                            smoothing=eps, top_k=k, correct_k=o.get("correct_k"))
    else:
        hip.softmax_xent(zd, ld, gs, o.get("dlogits"), o["loss"], o.get("correct"), probs=o.get("probs"))
    torch.cuda.synchronize()
    return {n: t.cpu() for n, t in o.items()}


def _figures(out, want):
    return {n: rel(out[n], w) for n, w in zip(("loss", "dlogits", "probs"), want)}


def test_existing_kernel_figure(hip, cases):
    """The measurement behind MEASURED_REL, repeated: the existing kernel's worst rel() is printed
    and must not exceed the recorded value (the inputs are fixed and the kernel is deterministic)."""
    worst = 0.0
    for key, (z, labels, gs, refs, _) in cases.items():
        fig = _figures(_run(hip, z, labels, gs, ex=False), refs[0.0])
        print("drn_softmax_xent", key, fig)
        worst = max(worst, *fig.values())
    print("worst", worst)
    assert worst <= MEASURED_REL, worst


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_kernel_matches_fp64_reference(hip, cases, eps, k):
    """loss, dlogits, probs within BOUND = 4 x MEASURED_REL = 6.6e-07 of the fp64 reference (rel() of
    tests/test_ops_gpu.py; the existing kernel measures 1.65e-07, this one 1.65e-07 at most); correct
    and correct_k exactly the rank rule, ties included."""
    worst = 0.0
    for key, (z, labels, gs, refs, ranks) in cases.items():
        out = _run(hip, z, labels, gs, eps, k)
        fig = _figures(out, refs[eps])
        print("drn_softmax_xent_ex", key, eps, k, fig)
        worst = max(worst, *fig.values())
        assert torch.equal(out["correct"], ranks[1]), key
        assert torch.equal(out["correct_k"], ranks[k]), key
    print("worst", worst, "bound", BOUND)
    assert worst <= BOUND, worst


def test_kernel_optional_outputs_and_top_k_at_least_ncls(hip, cases):
    """dlogits null with probs non-null and correct / correct_k null: the remaining outputs are the
    same bits as the full call's. top_k >= ncls: every row counts (the logits are finite)."""
    for key, (z, labels, gs, _, ranks) in cases.items():
        full = _run(hip, z, labels, gs, 0.1, 5)
        part = _run(hip, z, labels, gs, 0.1, 5, dlogits=False, correct=False, correct_k=False)
        assert set(part) == {"loss", "probs"}
        assert torch.equal(part["loss"], full["loss"]) and torch.equal(part["probs"], full["probs"])
        only_k = _run(hip, z, labels, gs, 0.1, 5, dlogits=False, probs=False, correct=False)
        assert torch.equal(only_k["correct_k"], full["correct_k"])
        for k in (key[1], key[1] + 7):
            assert torch.equal(_run(hip, z, labels, gs, 0.1, k)["correct_k"], ranks[key[1]])
            assert bool(ranks[key[1]].all())


def test_kernel_rank_rule_special_rows(hip):
    """All logits equal; a NaN label logit (correct_k 0) and a NaN elsewhere (ignored)."""
    nan = float("nan")
    z = torch.tensor([[2.0] * 8, [2.0] * 8, [2.0] * 8, [1.0, nan, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                      [1.0, nan, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    labels = torch.tensor([0, 4, 7, 1, 2], dtype=torch.int32)
    for k, want in ((1, [1, 0, 0, 0, 1]), (5, [1, 1, 0, 0, 1]), (8, [1, 1, 1, 0, 1])):
        out = _run(hip, z, labels, 1.0, 0.1, k)
        assert out["correct_k"].tolist() == want == rank_rule(z, labels, k).tolist(), k
    assert _run(hip, z, labels, 1.0, 0.0, 1)["correct"].tolist()[:3] == [1, 0, 0]


def test_kernel_rejects_bad_arguments(hip):
    z, labels = torch.zeros(2, 10, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    loss = torch.zeros(2, device="cuda")
    for kw in (dict(smoothing=1.0), dict(smoothing=-0.5), dict(top_k=0)):
        with pytest.raises(_lib.KernelLibraryError):
            hip.softmax_xent_ex(z, labels, 1.0, None, loss, None, **kw)


def test_smoothing_term_without_a_tolerance_choice(hip, cases):
    """At fixed logits dlogits(eps = 0.1) - dlogits(eps = 0) = (eps [j == y] - eps / K) grad_scale up
    to 4 * 2^-24 * grad_scale per element: the probabilities are the same bits in both calls (checked)
    and only a few roundings of values <= 1 separate the two results."""
    eps = 0.1
    for key, (z, labels, gs, _, _) in cases.items():
        a, b = _run(hip, z, labels, gs, 0.0, 1), _run(hip, z, labels, gs, eps, 1)
        assert torch.equal(a["probs"], b["probs"]), key
        K = z.shape[1]
        want = (eps * F.one_hot(labels.long(), K).double() - eps / K) * gs
        err = ((b["dlogits"].double() - a["dlogits"].double()) - want).abs().max().item()
        print(key, "max error", err, "bound", 4 * 2.0 ** -24 * gs)
        assert err <= 4 * 2.0 ** -24 * gs, (key, err)


def test_equals_existing_kernel_at_zero_smoothing_and_is_deterministic(hip, cases):
    """eps = 0, k = 1: dlogits, probs, correct (and the loss, which is then computed by the existing
    kernel's own expression) are the bits of drn_softmax_xent, and correct_k == correct. The same call
    twice gives the same bits, smoothed or not."""
    for key, (z, labels, gs, _, _) in cases.items():
        old, new = _run(hip, z, labels, gs, ex=False), _run(hip, z, labels, gs, 0.0, 1)
        for n in ("dlogits", "probs", "correct"):
            assert torch.equal(old[n], new[n]), (key, n)
        assert rel(new["loss"], old["loss"]) <= BOUND and torch.equal(old["loss"], new["loss"]), key
        assert torch.equal(new["correct_k"], new["correct"]), key
        for eps, k in ((0.0, 1), (0.1, 5)):
            a, b = _run(hip, z, labels, gs, eps, k), _run(hip, z, labels, gs, eps, k)
            for n in a:
                assert torch.equal(a[n], b[n]), (key, eps, n)


# -- executor ----------------------------------------------------------------------------------------
def _ex(spec, N, seed=3, lr=0.1, backend=None, data_seed=9, **kw):
    dev = "cpu" if backend is not None else "cuda"
    ex = Executor(spec, N, backend or HipBackend("cuda"), dev, seed=seed, **kw)
    images, labels = fixed_batch(N, seed=data_seed)
    ex.images.zero_()
    ex.images[..., :3] = images.to(dev, ex.images.dtype)
    ex.labels.copy_(labels.to(dev))
    ex.set_lr(lr)
    return ex


def _state(ex):
    torch.cuda.synchronize()
    return [t.clone() for t in (ex.P.master, ex.P.momentum, ex.P.bn_state, ex.loss_vec)]


def test_smoothed_step_matches_reference_executor():
    """tests/test_executor_gpu.py::test_step_matches_reference (cifar8 bounds) with label_smoothing =
    0.1 and top_k = 5 on both sides; correct_k is the rank rule on the executor's own logits."""
    spec, N = cifar_resnet_v2(8), 8
    exs = {}
    for dev, be in (("cpu", RefBackend()), ("cuda", None)):
        ex = _ex(spec, N, seed=5, backend=be, label_smoothing=0.1, top_k=5)
        ex.P.master.copy_(ex.P.master.bfloat16().float())  # identical (bf16-representable) weights
        ex.sync_weights()
        ex.forward(train=True)
        ex.backward()
        exs[dev] = ex
    torch.cuda.synchronize()
    r, h = exs["cpu"], exs["cuda"]
    cosl = F.cosine_similarity(h.logits.cpu().flatten(), r.logits.flatten(), dim=0).item()
    assert cosl > 0.98, cosl
    assert abs(h.loss_vec.mean().item() - r.loss_vec.mean().item()) < 0.1
    for s in h.P.slots:
        a, b = h.P.g(s.name).float().cpu().flatten(), r.P.g(s.name).float().cpu().flatten()
        cos = F.cosine_similarity(a, b, dim=0).item()
        assert cos > 0.9, (s.name, cos)
    for name in ("dense/kernel", "dense/bias"):
        assert rel(h.P.g(name), r.P.g(name)) < 3e-2
    assert torch.equal(h.correct_k.cpu(), rank_rule(h.logits.cpu(), h.labels.cpu(), 5))
    assert torch.equal(h.correct.cpu(), rank_rule(h.logits.cpu(), h.labels.cpu(), 1))
    want = F.cross_entropy(h.logits.cpu().double(), h.labels.cpu().long(), label_smoothing=0.1, reduction="none")
    print("executor loss_vec rel", rel(h.loss_vec, want), "bound", BOUND)
    assert rel(h.loss_vec, want) <= BOUND


def test_smoothed_eager_graph_and_plan_steps_are_bitwise_equal(monkeypatch):
    """tests/test_lars_gpu.py::test_lars_joined_deferred_graph_and_plan_steps_are_bitwise_equal with
    label_smoothing = 0.1, top_k = 5 and optimizer = "lars": the smoothing and top_k arguments are
    captured by value into the HIP graph and recorded by value into the native plan."""
    from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph
    from distributed_resnet_tensorflow_amd.runtime.plan import StepPlan
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    monkeypatch.setenv("DRN_DEFER_TAIL", "1")
    spec, N = cifar_resnet_v2(14), 16
    outs = {}
    for mode in ("eager", "graph", "plan"):
        ex = _ex(spec, N, lr=0.5, optimizer="lars", label_smoothing=0.1, top_k=5)
        fn = lambda: (ex.forward(True), ex.backward(defer_tail=mode != "eager"), ex.apply_gradients())  # noqa: E731
        if mode == "graph":
            StepGraph(fn, warmup=2).replay()
        elif mode == "plan":
            plan = StepPlan(ex, warmup=1)
            for _ in range(2):
                plan.replay()
        else:
            for _ in range(3):
                fn()
        outs[mode] = _state(ex) + [ex.correct_k.clone(), ex.dlogits.clone()]
    assert bool(outs["eager"][4].any())  # (correct_k, written by the new kernel only)
    for mode in ("graph", "plan"):
        for name, a, b in zip(("master", "momentum", "bn_state", "loss_vec", "correct_k", "dlogits"),
                              outs["eager"], outs[mode]):
            assert torch.equal(a, b), (mode, name)


def test_default_path_is_unchanged_and_top_k_only_observes(monkeypatch):
    """Defaults vs label_smoothing = 0.0, top_k = 0 passed explicitly vs top_k = 5 at eps = 0: weights,
    momentum, moving statistics and loss_vec after 3 steps are bitwise equal."""
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    spec, N = cifar_resnet_v2(8), 8
    outs = []
    for kw in ({}, dict(label_smoothing=0.0, top_k=0), dict(top_k=5)):
        ex = _ex(spec, N, **kw)
        for _ in range(3):
            ex.train_step()
        outs.append(_state(ex))
        if kw.get("top_k"):
            assert torch.equal(ex.correct_k.cpu(), rank_rule(ex.logits.cpu(), ex.labels.cpu(), 5))
            assert "precision_top_k" in ex.metrics()
        else:
            assert ex.correct_k is None and "precision_top_k" not in ex.metrics()
    for o in outs[1:]:
        for name, a, b in zip(("master", "momentum", "bn_state", "loss_vec"), outs[0], o):
            assert torch.equal(a, b), name


def test_smoothed_training_on_fixed_batch():
    """N, steps and LR of tests/test_executor_gpu.py::test_training_reduces_loss_on_fixed_batch with
    eps = 0.1: every step's mean loss >= H - 1e-3 (H = 0.500, the entropy of the smoothed target at
    K = 10), the excess over H at least halves, precision_top_k >= precision at every step (confirmed
    first on the reference executor: tests/test_label_smoothing.py)."""
    check_smoothed_training(_ex(cifar_resnet_v2(8), TRAIN_N, seed=7, data_seed=11, label_smoothing=TRAIN_EPS,
                                top_k=5))
