"""Mixup / CutMix on the GPU: the pair-mix kernel (csrc/kernels/mix.hip) and the mixed-target loss kernel
(csrc/kernels/head.hip softmax_xent_mix_kernel) against fp64 references, the executor's eager / graph /
plan steps with a mix table in device memory, and the feeders."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_label_smoothing import fixed_batch, rank_rule
from test_label_smoothing_gpu import SHAPES, _logits
from test_mix import (TRAIN_EPS, TRAIN_N, check_mixed_training, dominant, load_mixed, make_table, torch_mix,
                      training_case)
from test_ops_gpu import rel

from distributed_resnet_tensorflow_amd.data.mix import MixSampler
from distributed_resnet_tensorflow_amd.models.spec import cifar_resnet_v2
from distributed_resnet_tensorflow_amd.ops import _lib
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend, RefBackend, mix_identity, mix_table_tensor
from distributed_resnet_tensorflow_amd.runtime.executor import Executor

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

# a self-pair; odd N with a pixel count that is no block multiple; more than one block; ImageNet rows
MIX_SHAPES = [(1, 8, 8), (5, 7, 9), (4, 32, 32), (2, 224, 224)]
CANARY = 4096   # bf16 elements after the image buffers, which no launch may touch


def _records(H, W):
    """(w, lam, y0, x0, y1, x1): Mixup; boxes that are empty, full, at each border, one pixel wide, one
    pixel; identity; w of 0 and 1; a blend with a box."""
    return [(0.3, 0.3, 0, 0, 0, 0), (1.0, 1.0, 2, 2, 2, 5), (1.0, 0.0, 0, 0, H, W), (1.0, 0.5, 0, 0, 2, W),
            (1.0, 0.5, H - 2, 0, H, W), (1.0, 0.5, 0, 0, H, 2), (1.0, 0.5, 0, W - 2, H, W), (1.0, 0.9, 0, 3, H, 4),
            (1.0, 0.9, 2, 3, 3, 4), (1.0, 1.0, 0, 0, 0, 0), (0.0, 0.0, 0, 0, 0, 0), (1.0, 0.7, 1, 1, H - 1, W - 1),
            (0.6, 0.6, 1, 2, 4, 6), (0.8125, 0.8125, 0, 0, 0, 0)]


def _tables(N, H, W):
    """Per-sample tables that walk through every record kind, N at a time (+ the all-identity one)."""
    recs = _records(H, W)
    out = [make_table([recs[(s + i) % len(recs)] for i in range(N)]) for s in range(0, len(recs), max(1, N - 1))]
    return out + [mix_identity(N)]


def _fp64_mix(src, table):
    """RefBackend.mix_pairs in fp64 on the bf16 images (the process-wide dtype goes back to fp32)."""
    ref = RefBackend("cpu", dtype=torch.float64)
    try:
        dst = torch.empty(src.shape, dtype=torch.float64)
        ref.mix_pairs(src.double(), dst, mix_table_tensor(table))
    finally:
        RefBackend("cpu")
    return dst


def _bits(t):
    return t.contiguous().view(torch.int16)


def _images(N, H, W, same_sign):
    """bf16 images, 3 live channels of 8. same_sign: positive and negative values, but every (pixel,
    channel) has one sign across the batch, so w a + (1 - w) b never cancels."""
    g = torch.Generator().manual_seed(N * 1000 + H)
    src = torch.zeros(N, H, W, 8)
    v = torch.randn(N, H, W, 3, generator=g) * 2
    if same_sign:
        v = v.abs() * torch.where(torch.rand(1, H, W, 3, generator=g) < 0.5, -1.0, 1.0)
    src[..., :3] = v
    return src.bfloat16()


def _within_one_ulp(out, want, src=None, table=None):
    """|out - bf16(ref)| <= one bf16 ulp of bf16(ref) (2^(e - 7) for a value in [2^e, 2^(e + 1)), i.e.
    between 2^-8 and 2^-7 of it): one fp32 evaluation rounded once to bf16 lands on bf16(ref) or, where
    the fp64 value lies next to a rounding midpoint, on its neighbour -- when the terms do not cancel.
    With src / table the fp32 evaluation's own error is allowed on top, 2^-22 (|w a| + |(1 - w) b|) (three
    fp32 roundings of values of that size): it only shows where the two terms cancel to below 2^-14 of
    their size, which images of mixed sign do somewhere."""
    rounded = want.bfloat16().double()
    err = (out.double() - rounded).abs()
    bound = torch.where(rounded == 0, 0.0, torch.ldexp(torch.ones_like(rounded), torch.frexp(rounded)[1] - 8))
    if src is not None:
        w = torch.from_numpy(table["w"].copy()).double()[:, None, None, None]
        a = src.double()
        bound = bound + 2.0 ** -22 * (w.abs() * a.abs() + (1.0 - w).abs() * a.flip(0).abs())
    worst = float((err / want.abs().clamp_min(1e-30)).max())
    return bool((err <= bound).all()), worst


@pytest.fixture(scope="module")
def mix_cases():
    """{shape: (src bf16 CPU, [(table, fp64 reference)])}, computed once and never modified."""
    out = {}
    for N, H, W in MIX_SHAPES:
        src = _images(N, H, W, same_sign=True)
        out[(N, H, W)] = (src, [(t, _fp64_mix(src, t)) for t in _tables(N, H, W)])
    return out


def _launch(hip, src, table, inplace):
    """One launch on a buffer with a canary tail; (result CPU, canary intact)."""
    n = src.numel()
    bufs = [torch.full((n + CANARY,), 77.0, dtype=torch.bfloat16, device="cuda") for _ in range(1 if inplace else 2)]
    s = bufs[0][:n].view(src.shape)
    s.copy_(src)
    d = s if inplace else bufs[1][:n].view(src.shape)
    hip.mix_pairs(s, d, mix_table_tensor(table).cuda())
    torch.cuda.synchronize()
    ok = all(bool((b[n:] == 77.0).all()) for b in bufs) and (inplace or torch.equal(s.cpu(), src))
    return d.cpu(), ok


@pytest.mark.parametrize("shape", MIX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mix_pairs_matches_fp64_reference(hip, mix_cases, shape):
    """Outside boxes within one bf16 ulp of the reference rounded to bf16 (_within_one_ulp: one fp32
    evaluation rounded once; the images have one sign per pixel and channel, so no blend cancels; measured
    on an MI355X: the worst difference is exactly one ulp, 0.0058 to 0.0078 of the value); the partner's / own bits inside boxes, at w of 0 / 1, for identity records
    and for the self-pair; channels 3..7 stay zero; in place == out of place; the canaries are untouched."""
    N, H, W = shape
    src, cases = mix_cases[shape]
    ys, xs = torch.arange(H)[None, :, None], torch.arange(W)[None, None, :]
    for table, want in cases:
        out, ok = _launch(hip, src, table, inplace=False)
        assert ok, "canary / source changed (out of place)"
        inp, ok = _launch(hip, src, table, inplace=True)
        assert ok, "canary changed (in place)"
        assert torch.equal(_bits(out), _bits(inp))
        ok, worst = _within_one_ulp(out, want)
        print(shape, "worst |out - bf16(ref)| / |ref|", worst)
        assert ok, worst
        t = torch.from_numpy
        box = ((ys >= t(table["y0"].copy())[:, None, None]) & (ys < t(table["y1"].copy())[:, None, None])
               & (xs >= t(table["x0"].copy())[:, None, None]) & (xs < t(table["x1"].copy())[:, None, None]))
        w = t(table["w"].copy())[:, None, None].expand(N, H, W)
        own, partner = (w == 1.0) & ~box, box | (w == 0.0)
        if N % 2:
            own[N // 2], partner[N // 2] = True, False
        assert torch.equal(_bits(out)[own], _bits(src)[own])
        assert torch.equal(_bits(out)[partner], _bits(src.flip(0))[partner])
        assert not bool(_bits(out)[..., 3:].any())


def test_mix_pairs_images_of_mixed_sign(hip):
    """Blends of images whose values differ in sign (the terms may cancel): the bound of
    _within_one_ulp with the fp32 evaluation's own error."""
    N, H, W = 4, 32, 32
    src = _images(N, H, W, same_sign=False)
    table = make_table([(0.3, 0.3, 0, 0, 0, 0), (0.8125, 0.8125, 0, 0, 0, 0), (0.6, 0.6, 1, 2, 4, 6),
                        (0.5, 0.5, 0, 0, 0, 0)])
    out, ok = _launch(hip, src, table, inplace=True)
    assert ok
    ok, worst = _within_one_ulp(out, _fp64_mix(src, table), src, table)
    print("worst |out - bf16(ref)| / |ref|", worst)
    assert ok, worst


def test_mix_pairs_rejects_bad_arguments(hip):
    x = torch.zeros(2, 4, 4, 8, dtype=torch.bfloat16, device="cuda")
    t = mix_table_tensor(mix_identity(2)).cuda()
    L, p, tp = hip.L, x.data_ptr(), t.data_ptr()
    assert L.drn_mix_pairs(p, p, tp, 2, 16, 4, hip.stream()) == 0
    for args in ((p, p, tp, 0, 16, 4), (p, p, tp, 2, 0, 4), (p, p, tp, 2, -16, 4), (p, p, None, 2, 16, 4),
                 (p, p, tp, 2, 16, 0), (p, p, tp, 2, 16, 3), (None, p, tp, 2, 16, 4), (p, None, tp, 2, 16, 4)):
        assert L.drn_mix_pairs(*args, hip.stream()) != 0, args
    torch.cuda.synchronize()
    with pytest.raises(AssertionError):
        hip.mix_pairs(x, x, mix_table_tensor(mix_identity(3)).cuda())
    with pytest.raises(AssertionError):
        hip.mix_pairs(x, x.float(), t)
    buf = torch.zeros(3 * 4 * 4 * 8, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(AssertionError):   # partly overlapping src / dst
        hip.mix_pairs(buf[:256].view(2, 4, 4, 8), buf[128:384].view(2, 4, 4, 8), t)
    loss, z = torch.zeros(2, device="cuda"), torch.zeros(2, 10, device="cuda")
    lab = torch.zeros(2, dtype=torch.int32, device="cuda")
    for kw in (dict(smoothing=1.0), dict(smoothing=-0.5), dict(top_k=0)):
        with pytest.raises(_lib.KernelLibraryError):
            hip.softmax_xent_mix(z, lab, t, 1.0, None, loss, None, **kw)
    assert L.drn_softmax_xent_mix(z.data_ptr(), lab.data_ptr(), None, 2, 10, 1.0, 0.0, 1, None, loss.data_ptr(), None,
                                  None, None, hip.stream()) != 0


# -- the loss kernel ---------------------------------------------------------------------------------------
def _mix_table_for(N, K, labels):
    """lam of 0.7, 0.25, 0.5, 1, 0 and random ones; label_b random, sometimes the sample's own label."""
    g = torch.Generator().manual_seed(77 * N + K)
    lam = torch.rand(N, generator=g)
    for i, v in enumerate((0.7, 0.25, 0.5, 1.0, 0.0)[:N]):
        lam[i] = v
    t = make_table([(float(l), float(l), 0, 0, 0, 0) for l in lam])
    lb = torch.randint(0, K, (N,), generator=g, dtype=torch.int32)
    lb[-1] = labels[-1]
    t["label_b"] = lb.numpy()
    return t


def _reference(z, labels, table, eps, gs):
    """loss, dlogits, probs in fp64 from the contract's formulas on the fp32 logits."""
    K = z.shape[1]
    lp = torch.log_softmax(z.double(), 1)
    lam = torch.from_numpy(table["lam"].copy()).double()[:, None]
    yb = torch.from_numpy(table["label_b"].astype(np.int64))
    t = (1.0 - eps) * (lam * F.one_hot(labels.long(), K) + (1.0 - lam) * F.one_hot(yb, K)) + eps / K
    return -(t * lp).sum(1), (lp.exp() - t) * gs, lp.exp()


def _reference_ex(z, labels, eps, gs):
    K = z.shape[1]
    lp = torch.log_softmax(z.double(), 1)
    t = (1.0 - eps) * F.one_hot(labels.long(), K).double() + eps / K
    return -(t * lp).sum(1), (lp.exp() - t) * gs, lp.exp()


def _run(hip, z, labels, gs, eps=0.0, k=1, table=None, kind="mix"):
    """One launch on device copies: kind mix / ex / plain; the outputs as CPU tensors."""
    N, K = z.shape
    zd, ld = z.cuda(), labels.cuda()
    o = {"loss": torch.full((N,), -7.0, device="cuda"), "dlogits": torch.full((N, K), -7.0, device="cuda"),
         "probs": torch.full((N, K), -7.0, device="cuda"),
         "correct": torch.full((N,), -7, dtype=torch.int32, device="cuda")}
    if kind == "plain":
        hip.softmax_xent(zd, ld, gs, o["dlogits"], o["loss"], o["correct"], probs=o["probs"])
    else:
        o["correct_k"] = torch.full((N,), -7, dtype=torch.int32, device="cuda")
        kw = dict(probs=o["probs"], smoothing=eps, top_k=k, correct_k=o["correct_k"])
        if kind == "ex":
            hip.softmax_xent_ex(zd, ld, gs, o["dlogits"], o["loss"], o["correct"], **kw)
        else:
            hip.softmax_xent_mix(zd, ld, mix_table_tensor(table).cuda(), gs, o["dlogits"], o["loss"], o["correct"], **kw)
    torch.cuda.synchronize()
    return {n: t.cpu() for n, t in o.items()}


@pytest.fixture(scope="module")
def cases():
    """{(N, K, kind): (logits, labels, gs, table)} -- the SHAPES and logit kinds of
    tests/test_label_smoothing_gpu.py; references are computed per (eps) in the tests' one pass."""
    out = {}
    for N, K in SHAPES:
        for kind in ("randn", "ints"):
            z, labels = _logits(N, K, kind)
            out[(N, K, kind)] = (z, labels, 1.0 / N, _mix_table_for(N, K, labels))
    return out


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_loss_kernel_matches_fp64_reference(hip, cases, eps, k):
    """loss, dlogits, probs of drn_softmax_xent_mix against the fp64 reference: worst rel() (tests/
    test_ops_gpu.py) at most 4 x the worst rel() of the untouched drn_softmax_xent_ex against its own fp64
    reference on the same logits, measured in the same run (one more gather and two more multiply-adds
    per element, the reasoning of tests/test_label_smoothing_gpu.py BOUND). Measured on an MI355X, for
    each of the four (eps, k): drn_softmax_xent_ex 1.6471e-07 and drn_softmax_xent_mix 1.6471e-07 (both the
    probs at 4 x 1001, random logits -- the same bits), so the bound is 6.588e-07; the mixed loss measures
    at most 1.21e-07, the mixed dlogits 1.06e-07. correct and correct_k: exactly the rank rule on the
    dominant label."""
    worst_ex = worst_mix = 0.0
    for key, (z, labels, gs, table) in cases.items():
        ex = _run(hip, z, labels, gs, eps, k, kind="ex")
        fig_ex = {n: rel(ex[n], w) for n, w in zip(("loss", "dlogits", "probs"), _reference_ex(z, labels, eps, gs))}
        out = _run(hip, z, labels, gs, eps, k, table)
        fig = {n: rel(out[n], w) for n, w in zip(("loss", "dlogits", "probs"), _reference(z, labels, table, eps, gs))}
        print(key, eps, k, "ex", fig_ex, "mix", fig)
        worst_ex, worst_mix = max(worst_ex, *fig_ex.values()), max(worst_mix, *fig.values())
        dom = dominant(labels.numpy(), table)
        assert torch.equal(out["correct"], rank_rule(z, dom, 1)), key
        assert torch.equal(out["correct_k"], rank_rule(z, dom, k)), key
    print("eps", eps, "k", k, "worst ex", worst_ex, "worst mix", worst_mix, "bound", 4 * worst_ex)
    assert worst_mix <= 4 * worst_ex, (worst_mix, worst_ex)


def test_loss_kernel_is_softmax_xent_ex_at_lam_one(hip, cases):
    """lam == 1 in every record (label_b then anything, outside the row included): every output is the
    bits of drn_softmax_xent_ex for the same (eps, top_k); at eps = 0 those of drn_softmax_xent; the same
    call twice gives the same bits, mixed or not."""
    for key, (z, labels, gs, mixed) in cases.items():
        N, K = z.shape
        table = mix_identity(N)
        table["label_b"] = [(-5, K, 2 ** 30, 3 % K, -1)[i % 5] for i in range(N)]
        for eps, k in ((0.0, 1), (0.1, 1), (0.1, 5), (0.0, 5)):
            a, b = _run(hip, z, labels, gs, eps, k, kind="ex"), _run(hip, z, labels, gs, eps, k, table)
            for n in a:
                assert torch.equal(a[n], b[n]), (key, eps, k, n)
        old, new = _run(hip, z, labels, gs, kind="plain"), _run(hip, z, labels, gs, 0.0, 1, table)
        for n in old:
            assert torch.equal(old[n], new[n]), (key, n)
        a, b = _run(hip, z, labels, gs, 0.1, 5, mixed), _run(hip, z, labels, gs, 0.1, 5, mixed)
        for n in a:
            assert torch.equal(a[n], b[n]), (key, n)


# -- executor ----------------------------------------------------------------------------------------------
def _ex(spec, N, seed=3, lr=0.1, backend=None, **kw):
    dev = "cpu" if backend is not None else "cuda"
    ex = Executor(spec, N, backend or HipBackend("cuda"), dev, seed=seed, **kw)
    ex.set_lr(lr)
    return ex


def _per_sample_table(N, labels, index=0):
    return MixSampler(N, 32, 32, mixup_alpha=0.4, cutmix_alpha=1.0, per_sample=True, seed=2).draw(index, labels.numpy())


def _state(ex):
    torch.cuda.synchronize()
    return [t.clone() for t in (ex.P.master, ex.P.momentum, ex.P.bn_state, ex.loss_vec)]


def test_mixed_step_matches_reference_executor():
    """tests/test_label_smoothing_gpu.py::test_smoothed_step_matches_reference_executor (its bounds) with
    a per-sample table mixing both kinds on both sides, each side mixing the images with its own backend."""
    spec, N = cifar_resnet_v2(8), 8
    images, labels = fixed_batch(N, seed=9)
    table = _per_sample_table(N, labels)
    exs = {}
    for dev, be in (("cpu", RefBackend()), ("cuda", None)):
        ex = _ex(spec, N, seed=5, backend=be, label_smoothing=0.1, top_k=5, mix=True)
        ex.P.master.copy_(ex.P.master.bfloat16().float())  # identical (bf16-representable) weights
        ex.sync_weights()
        load_mixed(ex, images, labels, table)
        ex.forward(train=True)
        ex.backward()
        exs[dev] = ex
    torch.cuda.synchronize()
    r, h = exs["cpu"], exs["cuda"]
    assert rel(h.images, r.images) < 2.0 ** -8
    cosl = F.cosine_similarity(h.logits.cpu().flatten(), r.logits.flatten(), dim=0).item()
    assert cosl > 0.98, cosl
    assert abs(h.loss_vec.mean().item() - r.loss_vec.mean().item()) < 0.1
    for s in h.P.slots:
        a, b = h.P.g(s.name).float().cpu().flatten(), r.P.g(s.name).float().cpu().flatten()
        cos = F.cosine_similarity(a, b, dim=0).item()
        assert cos > 0.9, (s.name, cos)
    for name in ("dense/kernel", "dense/bias"):
        assert rel(h.P.g(name), r.P.g(name)) < 3e-2
    dom = dominant(labels.numpy(), table)
    assert torch.equal(h.correct_k.cpu(), rank_rule(h.logits.cpu(), dom, 5))
    assert torch.equal(h.correct.cpu(), rank_rule(h.logits.cpu(), dom, 1))
    want = _reference(h.logits.cpu(), labels, table, 0.1, 1.0 / N)[0]
    print("executor loss_vec rel", rel(h.loss_vec, want))
    assert rel(h.loss_vec, want) <= 4 * 1.65e-7   # (tests/test_label_smoothing_gpu.py BOUND)
    h.forward(train=False)   # evaluation never mixes
    torch.cuda.synchronize()
    plain = F.cross_entropy(h.logits.cpu().double(), labels.long(), reduction="none")
    assert rel(h.loss_vec, plain) <= 4 * 1.65e-7


def test_mixed_eager_graph_and_plan_steps_are_bitwise_equal(monkeypatch):
    """The sizes of test_smoothed_eager_graph_and_plan_steps_are_bitwise_equal with mixing on: 3 steps with
    table A, then table B is written and one more step runs -- a replay, for the graph and the plan. They
    equal eager with A, A, A, B: the recorded loss kernel reads the table, it did not capture it."""
    from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph
    from distributed_resnet_tensorflow_amd.runtime.plan import StepPlan
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    monkeypatch.setenv("DRN_DEFER_TAIL", "1")
    spec, N = cifar_resnet_v2(14), 16
    images, labels = fixed_batch(N, seed=9)
    A, B = _per_sample_table(N, labels, 0), _per_sample_table(N, labels, 1)
    assert A.tobytes() != B.tobytes()
    outs = {}
    for mode in ("eager", "graph", "plan", "eager_A_only"):
        ex = _ex(spec, N, lr=0.5, optimizer="lars", label_smoothing=0.1, top_k=5, mix=True)
        load_mixed(ex, images, labels, A)
        fn = lambda: (ex.forward(True), ex.backward(defer_tail=not mode.startswith("eager")),  # noqa: E731
                      ex.apply_gradients())
        if mode == "graph":
            g = StepGraph(fn, warmup=2)
            g.replay()
            step = g.replay
        elif mode == "plan":
            plan = StepPlan(ex, warmup=1)
            for _ in range(2):
                plan.replay()
            step = plan.replay
        else:
            for _ in range(3):
                fn()
            step = fn
        torch.cuda.synchronize()
        if mode != "eager_A_only":
            ex.set_mix(B)
            torch.cuda.synchronize()
        step()
        outs[mode] = _state(ex) + [ex.correct_k.clone(), ex.dlogits.clone()]
    names = ("master", "momentum", "bn_state", "loss_vec", "correct_k", "dlogits")
    for mode in ("graph", "plan"):
        for name, a, b in zip(names, outs["eager"], outs[mode]):
            assert torch.equal(a, b), (mode, name)
    # (and table B does change the step: the comparison above is not vacuous)
    assert not torch.equal(outs["eager"][3], outs["eager_A_only"][3])
    assert not torch.equal(outs["eager"][0], outs["eager_A_only"][0])


def test_default_path_is_unchanged(monkeypatch):
    """mix=False passed explicitly gives the bits of not passing it: weights, momentum, moving statistics
    and loss_vec after 3 steps; nothing is allocated."""
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    spec, N = cifar_resnet_v2(8), 8
    images, labels = fixed_batch(N, seed=9)
    outs = []
    for kw in ({}, dict(mix=False)):
        ex = _ex(spec, N, **kw)
        ex.images.zero_()
        ex.images[..., :3] = images.to("cuda", ex.images.dtype)
        ex.labels.copy_(labels.cuda())
        for _ in range(3):
            ex.train_step()
        outs.append(_state(ex))
        assert ex.mix_table is None
    for name, a, b in zip(("master", "momentum", "bn_state", "loss_vec"), *outs):
        assert torch.equal(a, b), name


# -- feeders -----------------------------------------------------------------------------------------------
def test_cifar_feeder_mixes_in_place(tmp_path):
    """CifarFeeder with mixing: ex.images within one bf16 ulp of the reference mix (fp64, rounded to bf16)
    of an unmixed feeder's output over the same loader, the same bits for unmixed batches; the table in
    ex.mix_table is the sampler's draw for the batch."""
    from distributed_resnet_tensorflow_amd import cli
    from distributed_resnet_tensorflow_amd.data.cifar import write_fake_cifar
    from distributed_resnet_tensorflow_amd.parallel.cluster import ClusterInfo
    from distributed_resnet_tensorflow_amd.train.trainer import make_feeder
    write_fake_cifar(str(tmp_path), 64)
    args = [f"--train_data_path={tmp_path}", "--resnet_size=8", "--seed=3"]
    Fm = cli.entry_flags("cifar_main", args + ["--mixup_alpha=0.4", "--cutmix_alpha=1.0", "--mix_per_sample",
                                               "--mix_prob=0.6"])
    F0 = cli.entry_flags("cifar_main", args)
    cluster, spec, N = ClusterInfo(device="cuda"), cifar_resnet_v2(8), 8
    got = {}
    for name, F_ in (("mix", Fm), ("plain", F0)):
        ex = Executor(spec, N, HipBackend("cuda"), "cuda", mix=name == "mix")
        fd = make_feeder(F_, ex, cluster, True)
        got[name] = []
        try:
            for _ in range(6):
                assert fd.next()
                fd.prefetch()
                torch.cuda.synchronize()
                got[name].append((ex.images.cpu(), ex.labels.cpu(), ex.mix_table.cpu() if ex.mix else None))
        finally:
            fd.close()
    sampler = MixSampler(N, 32, 32, mixup_alpha=0.4, cutmix_alpha=1.0, prob=0.6, per_sample=True, seed=3)
    kinds = set()
    for i, (m, p) in enumerate(zip(got["mix"], got["plain"])):
        table = sampler.draw(i, p[1].numpy())
        assert m[2].numpy().tobytes() == table.tobytes() and torch.equal(m[1], p[1]), i
        ok, worst = _within_one_ulp(m[0], _fp64_mix(p[0], table), p[0], table)   # (standardised images: both signs)
        assert ok, (i, worst)
        unmixed = bool((table["w"] == 1.0).all() and (table["y1"] == table["y0"]).all())
        kinds.add(unmixed)
        if unmixed:
            assert torch.equal(_bits(m[0]), _bits(p[0])), i
    print("unmixed batches seen:", kinds)


def test_synthetic_feeder_does_not_compound():
    """After 3 next() calls the images are the mix of the pristine batch with draw 2, not a mix of mixes."""
    from distributed_resnet_tensorflow_amd.train.feeder import SyntheticFeeder
    N = 4
    ex = Executor(cifar_resnet_v2(8), N, HipBackend("cuda"), "cuda", mix=True)
    sampler = MixSampler(N, 32, 32, mixup_alpha=0.4, cutmix_alpha=1.0, per_sample=True, seed=1)
    fd = SyntheticFeeder(ex, seed=5, mix=sampler)
    pristine, labels = ex.images.cpu(), ex.labels.cpu()
    for _ in range(3):
        fd.next()
    torch.cuda.synchronize()
    table = sampler.draw(2, labels.numpy())
    ok, worst = _within_one_ulp(ex.images.cpu(), _fp64_mix(pristine, table), pristine, table)
    assert ok, worst
    assert ex.mix_table.cpu().numpy().tobytes() == table.tobytes() and fd.state() == {"mix_batch": 3}
    assert torch.equal(_bits(fd.pristine.cpu()), _bits(pristine))
    assert not torch.equal(_bits(ex.images.cpu()), _bits(pristine))


# -- training ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixup", "cutmix"])
def test_mixed_training_on_fixed_batch(kind):
    """tests/test_mix.py::test_oracle_executor_mixed_training_on_fixed_batch on the HIP executor."""
    images, labels, table = training_case(kind)
    ex = _ex(cifar_resnet_v2(8), TRAIN_N, seed=7, label_smoothing=TRAIN_EPS, mix=True)
    load_mixed(ex, images, labels, table)
    check_mixed_training(ex, labels, table)
