"""Global-norm gradient clipping and the non-finite step guard on the GPU: the two kernels of
csrc/kernels/gradguard.hip against an fp64 sum of squares of the same bits, their bitwise scaling,
determinism and skip rules, the entry point's argument checks, the executor's eager / graph / plan
steps, the ImageNet-style stem (no deferred tail while guarding) and a CLI run.

Sum-of-squares bound: |sumsq - ref| <= (L + 2) * 2^-24 * ref, with sumsq the kernel's fp32 sum
(record.norm is its correctly rounded square root, which the test checks bit for bit by re-adding the
published partials in the kernel's order) and ref = sum_i v_i^2 in float64 over the same fp32 values
v_i = fp32(grad_scale * g_i). Every term is >= 0, so a chain of L fp32 additions multiplies a term
by at most (1 + u)^L, u = 2^-24; the square v_i * v_i adds one more rounding (none with FMA
contraction); (1 + u)^(L + 1) - 1 <= (L + 2) u for the L used here (L u < 2^-9). L is the longest
chain one element passes through in the kernels as written, for V = 4 (fp32) / 8 (bf16) elements per
16-byte group, grid x block = GRID x BLOCK threads:
  grad_sumsq_kernel     a thread takes ceil(groups / (GRID * BLOCK)) groups; element j of a group goes
                        to accumulator j % 4, so V / 4 additions per group and accumulator; the n % V
                        trailing elements add at most V / 4 more (thread 0 of workgroup 0); the four
                        accumulators combine as (s0 + s1) + (s2 + s3): 2; wave64 butterfly: 6; the four
                        wave sums in LDS, in order: 3.
  grad_guard_apply      thread t re-adds partials t, t + BLOCK, ...: GRID / BLOCK additions; then the
                        same butterfly and LDS combine: 6 + 3.
"""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from distributed_resnet_tensorflow_amd.models.spec import cifar_resnet_v2, imagenet_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import (GUARD_GRID, GUARD_SKIP, HipBackend, guard_record_read,
                                                           guard_record_tensor)
from distributed_resnet_tensorflow_amd.runtime.executor import Executor

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 256
U = 2.0 ** -24
DTYPES = {"fp32": (torch.float32, 4), "bf16": (torch.bfloat16, 8)}


def sizes(V):
    """One 16-byte group; a size ending in a partial block plus a scalar tail; and just past grid x
    block x two groups in flight, so the first 300 threads run the main loop AND its one-group tail
    (the other threads the main loop alone), again with a scalar tail."""
    return [V, V * (BLOCK + 1) + V - 1, V * (2 * GUARD_GRID * BLOCK + 300) + 3]


def chain_length(n, V):
    groups = n // V
    per_thread = -(-groups // (GUARD_GRID * BLOCK))
    tail = -(-(n % V) // 4)
    return (V // 4) * per_thread + tail + 2 + 6 + 3 + GUARD_GRID // BLOCK + 6 + 3


def _grad(n, dtype, seed=11, amp=3.0):
    g = torch.Generator().manual_seed(seed + n % 97)
    return (torch.randn(n, generator=g) * amp).to(dtype).cuda()


def _guard(hip, g, gs=1.0, clip=0.0, guard=False, skip_in=None, record=None):
    partials = torch.full((GUARD_GRID,), float("nan"), device="cuda")   # (every cell must be written)
    record = guard_record_tensor("cuda") if record is None else record
    hip.grad_guard(g, gs, clip, guard, skip_in, partials, record)
    torch.cuda.synchronize()
    return partials, record


def _readd(partials):
    """grad_guard_apply_kernel's re-add of the partials, in fp32 on the host, in its order."""
    p = partials.cpu().view(GUARD_GRID // BLOCK, BLOCK)
    t = torch.zeros(BLOCK)
    for row in p:
        t = t + row
    x = t.view(BLOCK // 64, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[:, lane ^ o]
    assert bool((x == x[:, :1]).all())
    return ((x[0, 0] + x[1, 0]) + x[2, 0]) + x[3, 0]


def _words(record):
    return record.cpu().tolist()


# -- the kernels -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_norm_against_fp64_sum_of_squares(hip, wire):
    assert hip.L.drn_grad_guard_grid() == GUARD_GRID and hip.L.drn_grad_guard_block() == BLOCK
    dtype, V = DTYPES[wire]
    worst = 0.0
    for n in sizes(V):
        for gs in (1.0, 1.0 / 3.0):
            g = _grad(n, dtype)
            g0 = g.clone()
            partials, record = _guard(hip, g, gs=gs)
            v = g.float() * gs                              # fp32(gs * g): the kernel's own factor
            ref = float((v.double() ** 2).sum())
            s32 = _readd(partials)
            r = guard_record_read(record)
            assert r["norm"] == float(torch.sqrt(s32)), (n, gs)          # bit for bit
            err, bound = abs(float(s32.double()) - ref), (chain_length(n, V) + 2) * U * ref
            worst = max(worst, err / bound)
            print(f"{wire} n={n} gs={gs:.3g}: L={chain_length(n, V)} err={err:.3e} bound={bound:.3e} "
                  f"err/bound={err / bound:.4f}")
            assert err <= bound, (n, gs, err, bound)
            assert (r["scale"], r["skip"], r["skipped_total"], r["clipped_total"], r["steps_total"]) == (1.0, 0, 0, 0, 1)
            assert torch.equal(g, g0)                       # clip = 0: never scaled
    print(f"{wire}: worst err / bound {worst:.4f}")


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_scale_is_bitwise_and_unclipped_steps_leave_g_alone(hip, wire):
    dtype, V = DTYPES[wire]
    for n in sizes(V):
        g0 = _grad(n, dtype)
        _, rec = _guard(hip, g0.clone())
        norm = guard_record_read(rec)["norm"]
        # norm <= c (a huge bound, and c == norm exactly): untouched, scale 1, nothing counted
        for c in (1e30, norm):
            g = g0.clone()
            _, rec = _guard(hip, g, clip=c)
            r = guard_record_read(rec)
            assert torch.equal(g, g0) and r["scale"] == 1.0 and r["clipped_total"] == 0 and r["norm"] == norm
        c = 0.37 * norm
        g = g0.clone()
        _, rec = _guard(hip, g, clip=c)
        r = guard_record_read(rec)
        f = rec[:2].view(torch.float32)
        c32 = torch.tensor(c, dtype=torch.float32, device="cuda")
        want = c32 / torch.maximum(f[0], c32)               # fp32, from the record's own norm
        assert float(f[1]) == float(want) and 0.36 < r["scale"] < 0.38 and r["norm"] == norm
        assert (r["skip"], r["clipped_total"], r["steps_total"]) == (0, 1, 1)
        expect = g0 * f[1] if dtype == torch.float32 else (g0.float() * f[1]).bfloat16()
        assert torch.equal(g, expect), (wire, n)


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_two_runs_give_identical_partials_and_record(hip, wire):
    dtype, V = DTYPES[wire]
    for n in sizes(V)[1:]:
        g0 = _grad(n, dtype)
        c = 0.5 * guard_record_read(_guard(hip, g0.clone())[1])["norm"]
        runs = []
        for _ in range(2):
            g = g0.clone()
            partials, rec = _guard(hip, g, gs=0.5, clip=0.5 * c)
            runs.append((partials, rec, g))
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        assert guard_record_read(runs[0][1])["clipped_total"] == 1


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_non_finite_inputs(hip, wire):
    dtype, V = DTYPES[wire]
    for n in sizes(V)[1:]:
        clean = _grad(n, dtype)
        body = (n // V) * V
        assert body < n
        for bad in (float("nan"), float("inf")):
            for pos in (0, body - 1, n - 1):
                g0 = clean.clone()
                g0[pos] = bad
                # with the guard (and a clip that would trigger): skipped, g untouched, counted once
                g = g0.clone()
                _, rec = _guard(hip, g, clip=1e-3, guard=True)
                r = guard_record_read(rec)
                assert (r["skip"], r["scale"], r["skipped_total"], r["clipped_total"], r["steps_total"]) == \
                    (1, 1.0, 1, 0, 1), (n, bad, pos, r)
                assert not math.isfinite(r["norm"])
                assert torch.equal(g.view(torch.int16 if V == 8 else torch.int32),
                                   g0.view(torch.int16 if V == 8 else torch.int32))
                # a following clean call on the same record clears skip and keeps the count
                g = clean.clone()
                _guard(hip, g, clip=1e-3, guard=True, record=rec)
                r = guard_record_read(rec)
                assert (r["skip"], r["skipped_total"], r["clipped_total"], r["steps_total"]) == (0, 1, 1, 2)
                assert r["scale"] < 1.0 and not torch.equal(g, clean)
                # without the guard: the update is not gated and the gradient not touched
                g = g0.clone()
                _, rec = _guard(hip, g, clip=1e-3, guard=False)
                r = guard_record_read(rec)
                assert (r["skip"], r["scale"], r["skipped_total"], r["clipped_total"]) == (0, 1.0, 0, 0), (n, bad, pos)
                assert torch.equal(g.view(torch.int16 if V == 8 else torch.int32),
                                   g0.view(torch.int16 if V == 8 else torch.int32))


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_incoming_skip_word(hip, wire):
    dtype, V = DTYPES[wire]
    n = sizes(V)[1]
    g0 = _grad(n, dtype)
    word = torch.tensor([1], dtype=torch.int32, device="cuda")
    g = g0.clone()
    _, rec = _guard(hip, g, clip=1e-3, guard=True, skip_in=word)
    r = guard_record_read(rec)
    assert (r["skip"], r["skipped_total"], r["clipped_total"], r["steps_total"]) == (1, 0, 0, 1)
    assert torch.equal(g, g0) and math.isfinite(r["norm"]) and int(word) == 1
    word.zero_()
    _guard(hip, g, clip=1e-3, guard=True, skip_in=word, record=rec)
    r = guard_record_read(rec)
    assert (r["skip"], r["skipped_total"], r["clipped_total"], r["steps_total"]) == (0, 0, 1, 2)
    assert not torch.equal(g, g0)
    # the optimizer kernels take the record's skip word as theirs (drn_sgd_momentum wants n % 4 == 0)
    n4 = 4 * (BLOCK + 1)
    g = _grad(n4, dtype)
    w, m = torch.ones(n4, device="cuda"), torch.zeros(n4, device="cuda")
    lr = torch.tensor([0.1], device="cuda")
    word.fill_(7)
    _guard(hip, g, guard=True, skip_in=word, record=rec)
    hip.sgd_momentum(w, m, g, None, lr, 0.9, 0.0, 1.0, rec[GUARD_SKIP:GUARD_SKIP + 1])
    torch.cuda.synchronize()
    assert _words(rec)[GUARD_SKIP] == 1 and bool((w == 1).all()) and bool((m == 0).all())


def test_entry_point_rejects_bad_arguments(hip):
    g = torch.zeros(64, device="cuda")
    part = torch.zeros(GUARD_GRID, device="cuda")
    rec = guard_record_tensor("cuda")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    L, gp, pp, rp, wp = hip.L, g.data_ptr(), part.data_ptr(), rec.data_ptr(), word.data_ptr()
    s = hip.stream()
    assert L.drn_grad_guard(gp, 0, 64, 1.0, 0.5, 1, wp, pp, rp, s) == 0
    assert L.drn_grad_guard(gp, 1, 128, 1.0, 0.0, 0, None, pp, rp, s) == 0
    for args in ((None, 0, 64, 1.0, 0.5, 1, wp, pp, rp),               # null gradient
                 (gp, 0, 64, 1.0, 0.5, 1, wp, None, rp),               # null workspace
                 (gp, 0, 64, 1.0, 0.5, 1, wp, pp, None),               # null record
                 (gp, 0, 0, 1.0, 0.5, 1, wp, pp, rp),                  # nothing to do
                 (gp, 0, -4, 1.0, 0.5, 1, wp, pp, rp),
                 (gp, 0, 64, 1.0, -0.5, 1, wp, pp, rp),                # negative clip
                 (gp, 0, 64, 1.0, float("nan"), 1, wp, pp, rp),
                 (gp, 0, 64, 1.0, float("inf"), 1, wp, pp, rp),
                 (gp, 0, 64, float("nan"), 0.5, 1, wp, pp, rp),
                 (gp + 4, 0, 60, 1.0, 0.5, 1, wp, pp, rp),             # 16-byte loads from a misaligned pointer
                 (gp + 2, 1, 64, 1.0, 0.5, 1, wp, pp, rp),
                 (gp, 0, 64, 1.0, 0.5, 1, wp, pp + 2, rp),
                 (gp, 0, 64, 1.0, 0.5, 1, wp, pp, rp + 2),
                 (gp, 0, 64, 1.0, 0.5, 1, rp + 4 * GUARD_SKIP, pp, rp)):  # the incoming word inside the record
        assert L.drn_grad_guard(*args, s) != 0, args
    torch.cuda.synchronize()
    assert guard_record_read(rec)["steps_total"] == 2               # the rejected calls launched nothing
    with pytest.raises(AssertionError):
        hip.grad_guard(g.double(), 1.0, 0.0, True, None, part, rec)
    with pytest.raises(AssertionError):
        hip.grad_guard(g, 1.0, 0.0, True, None, part[:8], rec)
    with pytest.raises(AssertionError):
        hip.grad_guard(g, 1.0, 0.0, True, None, part, rec[:4])


# -- executor ----------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def first_norm():
    """||P.grad|| of the first step of the executor tests' network and batch (fp64, computed once)."""
    mp = pytest.MonkeyPatch()
    mp.setenv("DRN_DETERMINISTIC", "1")
    try:
        ex = _ex(cifar_resnet_v2(8), 8)
        ex.forward(True)
        ex.backward()
        torch.cuda.synchronize()
        return float(torch.linalg.vector_norm(ex.P.grad.double()))
    finally:
        mp.undo()


def test_huge_bound_is_bitwise_the_feature_off(monkeypatch):
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    out = {}
    for c in (0.0, 1e30):
        ex = _ex(cifar_resnet_v2(8), 8, clip_grad_norm=c)
        assert (ex.guard_record is None and ex.guard_partials is None and ex.grad_guard_stats() is None) == (c == 0.0)
        assert ex.guarding == (c > 0)
        for _ in range(3):
            ex.train_step()
        out[c] = _snap(ex, "master", "momentum", "bn_state")
        if c:
            r = ex.grad_guard_stats()
            assert (r["steps_total"], r["clipped_total"], r["skipped_total"], r["skip"], r["scale"]) == (3, 0, 0, 0, 1.0)
            assert r["norm"] > 0
    for name, a, b in zip(("master", "momentum", "bn_state"), out[0.0], out[1e30]):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("optimizer", ["momentum", "lars"])
def test_clipped_update_is_the_plain_update_on_the_scaled_gradient(hip, monkeypatch, first_norm, optimizer):
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    lr = 0.5 if optimizer == "lars" else 0.05
    ex = _ex(cifar_resnet_v2(8), 8, clip_grad_norm=0.5 * first_norm, optimizer=optimizer, lr=lr)
    ex.forward(True)
    ex.backward(defer_tail=True)
    g0, w, m, wb = _snap(ex, "grad", "master", "momentum", "wbf16")
    ex.apply_gradients()
    torch.cuda.synchronize()
    r = ex.grad_guard_stats()
    assert r["norm"] == pytest.approx(first_norm, rel=1e-5) and r["scale"] == pytest.approx(0.5, rel=1e-5)
    assert (r["clipped_total"], r["skip"]) == (1, 0)
    scale = ex.guard_record[:2].view(torch.float32)[1]
    g = g0 * scale
    assert torch.equal(ex.P.grad, g)
    if optimizer == "momentum":
        hip.sgd_momentum(w, m, g, wb, ex.lr_t, ex.mom, ex.wd, 1.0)
    else:
        partials = torch.zeros_like(ex.lars_partials)
        trust = torch.ones_like(ex.lars_trust)
        hip.lars_momentum(w, m, g, wb, ex.lars_table, 0, ex.lars_table.n, partials, trust, ex.lr_t, ex.mom, ex.wd,
                          1.0, ex.lars_eta, ex.lars_eps)
        torch.cuda.synchronize()
        assert torch.equal(trust, ex.lars_trust)
    torch.cuda.synchronize()
    assert torch.equal(w, ex.P.master) and torch.equal(m, ex.P.momentum) and torch.equal(wb, ex.P.wbf16)


def test_eager_graph_and_plan_clip_each_steps_gradient(monkeypatch, first_norm):
    from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph
    from distributed_resnet_tensorflow_amd.runtime.plan import StepPlan
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    out, recs = {}, {}
    for mode in ("eager", "graph", "plan"):
        ex = _ex(cifar_resnet_v2(8), 8, clip_grad_norm=0.25 * first_norm)
        fn = lambda: (ex.forward(True), ex.backward(defer_tail=True), ex.apply_gradients())  # noqa: E731
        norms = []
        if mode == "eager":
            for _ in range(3):
                fn()
                norms.append(ex.grad_guard_stats()["norm"])
        elif mode == "graph":
            g = StepGraph(fn, warmup=1)        # (one eager step, then the capture)
            norms.append(ex.grad_guard_stats()["norm"])
            for _ in range(2):
                g.replay()
                norms.append(ex.grad_guard_stats()["norm"])
        else:
            plan = StepPlan(ex, warmup=1)
            norms.append(ex.grad_guard_stats()["norm"])
            for _ in range(2):
                plan.replay()
                norms.append(ex.grad_guard_stats()["norm"])
        out[mode] = _snap(ex, "master", "momentum", "bn_state", "grad")
        recs[mode] = (ex.grad_guard_stats(), norms)
        r = recs[mode][0]
        assert (r["clipped_total"], r["steps_total"], r["skipped_total"]) == (3, 3, 0), (mode, r)
    assert len(set(recs["eager"][1])) == 3                 # every step had its own norm ...
    for mode in ("graph", "plan"):
        assert recs[mode] == recs["eager"], mode           # ... which the replays followed
        for name, a, b in zip(("master", "momentum", "bn_state", "grad"), out["eager"], out[mode]):
            assert torch.equal(a, b), (mode, name)


def test_inf_gradient_skips_the_whole_update_and_the_next_step_moves(monkeypatch):
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    ex = _ex(cifar_resnet_v2(8), 8, skip_nonfinite_grads=True, ema_decay=0.9, ema_warmup=False)
    ex.train_step()
    names = ("master", "momentum", "wbf16", "ema")
    before = _snap(ex, *names)
    ex.forward(True)
    ex.backward(defer_tail=True)
    s = ex.P.slots[3]
    ex.P.grad[s.offset + 1] = float("inf")
    ex.apply_gradients()
    after = _snap(ex, *names)
    for name, a, b in zip(names, before, after):
        assert torch.equal(a, b), name
    r = ex.grad_guard_stats()
    assert (r["skip"], r["skipped_total"], r["clipped_total"], r["steps_total"]) == (1, 1, 0, 2)
    ex.train_step()
    moved = _snap(ex, *names)
    for name, a, b in zip(names, after, moved):
        assert not torch.equal(a, b), name
    r = ex.grad_guard_stats()
    assert (r["skip"], r["skipped_total"], r["steps_total"]) == (0, 1, 3) and math.isfinite(r["norm"])
    assert bool(torch.isfinite(ex.P.master).all())


def test_guarding_never_defers_the_tail(monkeypatch):
    """ImageNet-style stem with DRN_DEFER_TAIL=1: an unguarded backward(defer_tail=True) defers; a
    guarded one joins, and its update is bitwise the joined step's on the clipped gradient."""
    monkeypatch.setenv("DRN_DETERMINISTIC", "1")
    monkeypatch.setenv("DRN_DEFER_TAIL", "1")
    spec, N = imagenet_resnet_v2(18, num_classes=10, image_size=64), 8
    plain = _ex(spec, N)
    assert plain._stem_hi == plain.stem_op.dw.numel() > 0 and plain.side is not None
    plain.forward(True)
    plain.backward(defer_tail=True)
    assert plain._tail_ev is not None                      # (the feature off: deferred as before)
    plain.join_grads()
    torch.cuda.synchronize()
    c = 0.5 * float(torch.linalg.vector_norm(plain.P.grad.double()))
    ex = _ex(spec, N, clip_grad_norm=c)
    ex.forward(True)
    ex.backward(defer_tail=True)
    assert ex._tail_ev is None and ex._pre_ev is None
    ex.apply_gradients()
    got = _snap(ex, "master", "momentum", "bn_state")
    r = ex.grad_guard_stats()
    assert r["clipped_total"] == 1 and r["scale"] == pytest.approx(0.5, rel=1e-5)
    ref = _ex(spec, N)
    ref.forward(True)
    ref.backward(defer_tail=False)
    torch.cuda.synchronize()
    ref.P.grad.mul_(ex.guard_record[:2].view(torch.float32)[1])
    ref.apply_gradients()
    want = _snap(ref, "master", "momentum", "bn_state")
    for name, a, b in zip(("master", "momentum", "bn_state"), got, want):
        assert torch.equal(a, b), name


# -- CLI ---------------------------------------------------------------------------------------------------
def test_cli_run_with_both_flags(tmp_path):
    from distributed_resnet_tensorflow_amd.ckpt.saver import latest_checkpoint
    from distributed_resnet_tensorflow_amd.utils import events
    ck, ev = str(tmp_path / "ck"), str(tmp_path / "ev")
    e = dict(os.environ, PYTHONPATH=REPO)
    args = ["resnet_cifar_main.py", "--num_gpus=1", "--synthetic_data=True", f"--log_root={ck}", f"--eval_dir={ev}",
            "--resnet_size=8", "--batch_size=32", "--train_steps=20", "--log_every_n_steps=10",
            "--save_summaries_steps=10", "--clip_grad_norm=0.5", "--skip_nonfinite_grads=True"]
    r = subprocess.run([sys.executable, "-u"] + args, cwd=REPO, capture_output=True, text=True, timeout=280, env=e)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    meta = json.load(open(latest_checkpoint(ck) + ".meta"))
    assert meta["clip_grad_norm"] == 0.5 and meta["skip_nonfinite_grads"] is True
    found = {}
    for root, _, files in os.walk(str(tmp_path)):
        if any("tfevents" in f for f in files):
            for tag in ("grad/global_norm", "grad/clip_scale", "grad/clipped_steps", "grad/skipped_steps"):
                s = events.scalar_series(root, tag)
                if s:
                    found[tag] = s
    assert set(found) == {"grad/global_norm", "grad/clip_scale", "grad/clipped_steps", "grad/skipped_steps"}, found
    assert all(math.isfinite(v) and v > 0 for _, v in found["grad/global_norm"])
    assert all(0 < v <= 1 for _, v in found["grad/clip_scale"])
    assert all(v == 0 for _, v in found["grad/skipped_steps"])
