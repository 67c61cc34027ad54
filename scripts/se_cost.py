"""Cost of the Squeeze-and-Excitation kernels (csrc/kernels/se.hip) at the four SE-ResNet-50 geometries
of batch 128 (256 ch @ 56x56, 512 @ 28x28, 1024 @ 14x14, 2048 @ 7x7, r = 16): all six kernels, and for the
three streaming ones the in-tree materialising bn_apply on the same tensor (a read + write streaming kernel
of the same layout) with the ratio of achieved GB/s.

Each timed window is one replay of a HIP graph of `--burst` back-to-back calls between two device events.
All cases of a geometry alternate window by window in one process; the figure per case is the median over
`--iters` windows, printed for each of `--repeats` repeats (their spread shows the noise). Bytes are the
compulsory ones: every operand and result once.

Then (unless --no_step) Executor.train_step, eager, of ResNet-50 beside SE-ResNet-50 (r = 16) at batch
128, alternating in one process. Writes profiles/se_cost.txt (--out).

--sigmoid instead measures the gate's sigmoid against fp64 (tests/se_refs.py SIGMOID_ULPS): with zero
expand weights the pre-activation is the bias, exactly, so the error is expf's and the division's alone.

    python scripts/se_cost.py [--out FILE] [--iters 10] [--burst 100] [--repeats 3] [--no_step] [--sigmoid]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_resnet_tensorflow_amd.models.spec import build_spec  # noqa: E402
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.executor import Executor  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph  # noqa: E402

LAYERS = [(256, 56), (512, 28), (1024, 14), (2048, 7)]
RATIO = 16


def window_us(graph, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / burst


def layer_cases(be, N, C, H):
    """{kernel: (fn, compulsory bytes, streaming)} of one geometry."""
    Cr, hw = C // RATIO, H * H
    f32 = lambda *sh: torch.randn(*sh, device="cuda")
    act = lambda: torch.randn(N, H, H, C, device="cuda").bfloat16()
    u, sc, g, out = act(), act(), act(), act()
    S = be.se_splits(N, hw, C)
    cells, w1, b1, w2, b2 = f32(N, S, C), f32(C, Cr) * 0.05, f32(Cr), f32(Cr, C) * 0.05, f32(C)
    z, h, s, dl2, dh, dzs = f32(N, C), f32(N, Cr), f32(N, C).sigmoid(), f32(N, C), f32(N, Cr), f32(N, C)
    dw1, db1, dw2, db2 = f32(C, Cr), f32(Cr), f32(Cr, C), f32(C)
    stats = torch.zeros(be.stats_replicas, 2, C, device="cuda")
    t, gate, wts = u.numel() * 2, N * (2 * C + Cr) * 4, (2 * C * Cr + C + Cr) * 4
    return {
        "squeeze": (lambda: be.se_squeeze(u, cells), t, True),
        "squeeze g*u": (lambda: be.se_squeeze(u, cells, g=g), 2 * t, True),
        "excite+stats": (lambda: be.se_excite(u, sc, s, out, stats=stats), 3 * t, True),
        "scale_bwd": (lambda: be.se_scale_bwd(g, s, dzs, out), 2 * t, True),
        "bn_apply": (lambda: be.bn_apply(u, out, b2, b2, relu=True), 2 * t, True),
        "gate_fwd": (lambda: be.se_gate_fwd(cells, hw, w1, b1, w2, b2, z, h, s), cells.numel() * 4 + gate + wts, False),
        "gate_bwd": (lambda: be.se_gate_bwd(cells, hw, w1, w2, h, s, dl2, dh, dzs),
                     cells.numel() * 4 + 2 * gate + wts, False),
        "gate_wgrad": (lambda: be.se_gate_wgrad(z, h, dl2, dh, dw1, db1, dw2, db2), 2 * gate + wts, False),
    }


def step_times(N, rounds, steps):
    """ms of Executor.train_step, eager, ResNet-50 and SE-ResNet-50 alternating."""
    exs = {}
    for name, spec in (("resnet50", build_spec("imagenet", 50)), ("se_resnet50_r16", build_spec("imagenet", 50, se_ratio=RATIO))):
        be = HipBackend("cuda")
        ex = Executor(spec, N, be, "cuda", seed=0, weight_decay=1e-4)
        be.synthetic_images(ex.images, seed=3)
        ex.labels.copy_(torch.randint(0, 1000, (N,), dtype=torch.int32))
        ex.set_lr(0.01)
        ex.autotune()
        for _ in range(3):
            ex.train_step()
        exs[name] = ex
    out = {k: [] for k in exs}
    for _ in range(rounds):
        for name, ex in exs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                ex.train_step()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) * 1e3 / steps)
    return out


def sigmoid_error(be):
    """max |s - sigmoid(x)| / (2^-24 sigmoid(x)) of se_gate_fwd over x in [-12, 12]."""
    N, C, Cr = 64, 4096, 8
    x = torch.linspace(-12, 12, N * C, device="cuda")
    z, h, s = (torch.empty(N, n, device="cuda") for n in (C, Cr, C))
    worst = 0.0
    for n in range(N):   # (b2 is one row of C values: one row of s per launch is exact x)
        b2 = x[n * C:(n + 1) * C].contiguous()
        be.se_gate_fwd(torch.zeros(N, 1, C, device="cuda"), 1, torch.zeros(C, Cr, device="cuda"),
                       torch.zeros(Cr, device="cuda"), torch.zeros(Cr, C, device="cuda"), b2, z, h, s)
        ref = torch.sigmoid(b2.double())
        worst = max(worst, float(((s[0].double() - ref).abs() / (2.0 ** -24 * ref)).max()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "se_cost.txt"))
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--burst", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no_step", action="store_true")
    ap.add_argument("--sigmoid", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a GPU measurement"
    be = HipBackend("cuda")
    if a.sigmoid:
        print(f"sigmoid: worst error {sigmoid_error(be):.3f} U relative")
        return
    lines = [f"Squeeze-and-Excitation kernel cost, SE-ResNet-50 (r = {RATIO}) geometries, batch {a.batch}, "
             f"{torch.cuda.get_device_name(0)}",
             f"us per call = median of {a.iters} windows of {a.burst} calls in a HIP graph; the column holds that "
             f"median for each of {a.repeats} repeats; GB/s = compulsory bytes / median repeat; vs bn_apply = ratio of "
             "GB/s (streaming kernels)",
             f"{'geometry':<16}{'kernel':<14}{'us (repeats)':<30}{'GB/s':>8}{'vs bn_apply':>13}"]
    for C, H in LAYERS:
        cases = layer_cases(be, a.batch, C, H)
        keys = list(cases)
        for k in keys:
            for _ in range(2):
                cases[k][0]()
        torch.cuda.synchronize()
        graphs = {k: StepGraph(lambda fn=cases[k][0]: [fn() for _ in range(a.burst)], warmup=1) for k in keys}
        reps = {k: [] for k in keys}
        for _ in range(a.repeats):
            win = {k: [] for k in keys}
            for _ in range(a.iters):
                for k in keys:
                    win[k].append(window_us(graphs[k], a.burst))
            for k in keys:
                reps[k].append(sorted(win[k])[len(win[k]) // 2])
        med = {k: sorted(reps[k])[len(reps[k]) // 2] for k in keys}
        gbs = {k: cases[k][1] / med[k] / 1e3 for k in keys}
        for k in keys:
            vs = f"{gbs[k] / gbs['bn_apply']:12.2f}x" if cases[k][2] and k != "bn_apply" else ""
            lines.append(f"{f'{C}ch {H}x{H}':<16}{k:<14}{' '.join(f'{v:8.1f}' for v in reps[k]):<30}{gbs[k]:8.0f}{vs}")
        print("\n".join(lines[-len(keys):]), flush=True)
        del graphs, cases
        torch.cuda.empty_cache()
    if not a.no_step:
        st = step_times(a.batch, rounds=3, steps=10)
        lines.append(f"Executor.train_step, eager, batch {a.batch}, ms per step (3 rounds of 10 steps, alternating)")
        for name, v in st.items():
            lines.append(f"  {name:<18}" + " ".join(f"{t:8.2f}" for t in v))
        print("\n".join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
