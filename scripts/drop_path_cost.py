"""Cost of the stochastic-depth kernels (csrc/kernels/drop_path.hip) at the four ResNet-50 block-output
geometries of batch 128 (256 ch @ 56x56, 512 @ 28x28, 1024 @ 14x14, 2048 @ 7x7): the forward add +
statistics and the backward branch gradient, with every sample kept and with every second sample dropped,
beside the in-tree materialising bn_apply on the same tensor (a read + write streaming kernel of the same
layout) with the ratio of achieved GB/s.

Each timed window is one replay of a HIP graph of `--burst` back-to-back calls between two device events.
All cases of a geometry alternate window by window in one process; the figure per case is the median over
`--iters` windows, printed for each of `--repeats` repeats (their spread shows the noise). Bytes are the
compulsory ones: every operand and result once, a dropped sample's unread operand not at all.

Then (unless --no_step) Executor.train_step, eager, of ResNet-50 with drop_path_rate 0 and 0.1 at batch 128,
alternating in one process; the rate-0.1 executor steps with a fresh host draw each step. Writes
profiles/drop_path_cost.txt (--out).

    python scripts/drop_path_cost.py [--out FILE] [--iters 10] [--burst 100] [--repeats 3] [--no_step]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_resnet_tensorflow_amd.data.drop_path import DropPathSampler  # noqa: E402
from distributed_resnet_tensorflow_amd.models.spec import build_spec  # noqa: E402
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.executor import Executor  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph  # noqa: E402

LAYERS = [(256, 56), (512, 28), (1024, 14), (2048, 7)]


def window_us(graph, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / burst


def layer_cases(be, N, C, H):
    """{case: (fn, compulsory bytes)} of one geometry."""
    act = lambda: torch.randn(N, H, H, C, device="cuda").bfloat16()
    u, sc, g, out = act(), act(), act(), act()
    one = torch.ones(C, device="cuda")
    keep = torch.full((N,), 1 / (1 - 0.1), device="cuda")
    half = keep.clone()
    half[1::2] = 0.0
    stats = torch.zeros(be.stats_replicas, 2, C, device="cuda")
    t = u.numel() * 2
    return {
        "fwd kept": (lambda: be.drop_path_fwd(u, sc, keep, out, stats=stats), 3 * t),
        "fwd half": (lambda: be.drop_path_fwd(u, sc, half, out, stats=stats), 3 * t - t // 2),
        "bwd kept": (lambda: be.drop_path_bwd(g, keep, out), 2 * t),
        "bwd half": (lambda: be.drop_path_bwd(g, half, out), 2 * t - t // 2),
        "bn_apply": (lambda: be.bn_apply(u, out, one, one, relu=True), 2 * t),
    }


def step_times(N, rounds, steps):
    """ms of Executor.train_step, eager, ResNet-50 with rate 0 and rate 0.1, alternating."""
    exs = {}
    for name, rate in (("resnet50 rate 0", 0.0), ("resnet50 rate 0.1", 0.1)):
        be = HipBackend("cuda")
        ex = Executor(build_spec("imagenet", 50, drop_path_rate=rate), N, be, "cuda", seed=0, weight_decay=1e-4)
        be.synthetic_images(ex.images, seed=3)
        ex.labels.copy_(torch.randint(0, 1000, (N,), dtype=torch.int32))
        ex.set_lr(0.01)
        ex.autotune()
        for _ in range(3):
            ex.train_step()
        exs[name] = (ex, DropPathSampler(N, ex.drop_rates, seed=1) if rate else None)
    out = {k: [] for k in exs}
    batch = 0
    for _ in range(rounds):
        for name, (ex, sampler) in exs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                if sampler is not None:
                    ex.set_drop_path(torch.from_numpy(sampler.draw(batch)).pin_memory())
                    batch += 1
                ex.train_step()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) * 1e3 / steps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "drop_path_cost.txt"))
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--burst", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no_step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a GPU measurement"
    be = HipBackend("cuda")
    lines = [f"Stochastic-depth kernel cost, ResNet-50 block-output geometries, batch {a.batch}, "
             f"{torch.cuda.get_device_name(0)}",
             f"us per call = median of {a.iters} windows of {a.burst} calls in a HIP graph; the column holds that "
             f"median for each of {a.repeats} repeats; GB/s = compulsory bytes / median repeat; vs bn_apply = ratio of "
             "GB/s; kept: f = 1 / 0.9 for every sample, half: every second sample dropped",
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
            vs = f"{gbs[k] / gbs['bn_apply']:12.2f}x" if k != "bn_apply" else ""
            lines.append(f"{f'{C}ch {H}x{H}':<16}{k:<14}{' '.join(f'{v:8.1f}' for v in reps[k]):<30}{gbs[k]:8.0f}{vs}")
        print("\n".join(lines[-len(keys):]), flush=True)
        del graphs, cases
        torch.cuda.empty_cache()
    if not a.no_step:
        st = step_times(a.batch, rounds=3, steps=10)
        lines.append(f"Executor.train_step, eager, batch {a.batch}, ms per step (3 rounds of 10 steps, alternating)")
        for name, v in st.items():
            lines.append(f"  {name:<20}" + " ".join(f"{t:8.2f}" for t in v))
        print("\n".join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
