"""Cost of the ResNet-D pooled projection kernels (csrc/kernels/pool_proj.hip) on ResNet-50's three
downsampling geometries at batch 128 (256 @ 56 -> 512 @ 28, 512 @ 28 -> 1024 @ 14, 1024 @ 14 -> 2048 @ 7):
the pooled forward (raw input + BatchNorm prologue, and a materialised input) and the pooled data
gradient, beside the strided 1x1 projection they replace (forward with the fused prologue; the
single-phase data gradient that zero-fills the other phases) and the materialising bn_apply on the same
input tensor as the streaming yardstick.

Each timed window is one replay of a HIP graph of `--burst` back-to-back calls between two device
events. All cases alternate window by window in one process; the figure per case is the median over
`--iters` windows, printed for each of `--repeats` repeats (their spread shows the noise). Bytes are the
compulsory ones, each tensor once: the pooled forward reads the whole input (4x what the strided one
touches) and writes the output and the quarter-size stash; both data gradients write the whole da.

Then (unless --no_step) Executor.train_step, eager, of ResNet-50 with and without avg_down at batch 128,
alternating in one process. Writes profiles/avg_down_cost.txt (--out).

    python scripts/avg_down_cost.py [--out FILE] [--iters 10] [--burst 100] [--repeats 3] [--no_step]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_resnet_tensorflow_amd.models.spec import build_spec  # noqa: E402
from distributed_resnet_tensorflow_amd.ops.backend import ConvGeom, HipBackend, OutMap  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.executor import Executor  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph  # noqa: E402

LAYERS = [(256, 56, 512), (512, 28, 1024), (1024, 14, 2048)]


def window_us(graph, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / burst


def layer_cases(be, N, C, H, K):
    """{case: fn} of one geometry and the compulsory bytes of each."""
    P = H // 2
    bf = dict(dtype=torch.bfloat16, device="cuda")
    x, dy = torch.randn(N, H, H, C, **bf), torch.randn(N, P, P, K, **bf)
    act, da, sc, ap = torch.empty_like(x), torch.empty_like(x), torch.empty_like(dy), torch.empty(N, P, P, C, **bf)
    w, wt = torch.randn(K, 1, 1, C, **bf) * 0.05, torch.randn(C, 1, 1, K, **bf) * 0.05
    scale, shift = torch.randn(C, device="cuda"), torch.randn(C, device="cuda")
    be.bn_apply(x, act, scale, shift, relu=True)
    one, phase = ConvGeom(1, 0, 0, 1), OutMap(P, P, 2, 0, 0)
    fns = {
        "pooled fwd raw": lambda: be.pool_proj_fwd(x, w, sc, ap, in_bn=(scale, shift)),
        "pooled fwd act": lambda: be.pool_proj_fwd(act, w, sc, ap),
        "strided fwd raw": lambda: be.conv_fwd(x, w, sc, ConvGeom(2, 0, 0, 1), in_bn=(scale, shift)),
        "pooled dgrad": lambda: be.pool_proj_dgrad(dy, wt, da),
        "strided dgrad": lambda: be.conv_fwd(dy, wt, da, one, out_map=phase, out_fill=True),
        "bn_apply": lambda: be.bn_apply(x, act, scale, shift, relu=True),
    }
    xb, yb, wb = x.numel() * 2, dy.numel() * 2, w.numel() * 2
    nbytes = {"pooled fwd raw": xb + yb + xb // 4 + wb, "pooled fwd act": xb + yb + xb // 4 + wb,
              "strided fwd raw": xb // 4 + yb + wb, "pooled dgrad": yb + xb + wb, "strided dgrad": yb + xb + wb,
              "bn_apply": 2 * xb}
    return fns, nbytes


def step_times(N, rounds, steps):
    """Median ms of Executor.train_step, eager, ResNet-50 without and with avg_down, alternating."""
    exs = {}
    for name, spec in (("resnet50", build_spec("imagenet", 50)),
                       ("resnet50 avg_down", build_spec("imagenet", 50, avg_down=True))):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "avg_down_cost.txt"))
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--burst", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no_step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a GPU measurement"
    be = HipBackend("cuda")
    lines = [f"ResNet-D pooled projection cost, ResNet-50 downsampling geometries, batch {a.batch}, "
             f"{torch.cuda.get_device_name(0)}",
             f"us per call = median of {a.iters} windows of {a.burst} calls in a HIP graph; the column holds that "
             f"median for each of {a.repeats} repeats; GB/s = compulsory bytes / median repeat",
             f"{'geometry':<26}{'case':<18}{'us (repeats)':<30}{'MB':>8}{'GB/s':>8}{'vs bn_apply GB/s':>18}"]
    for C, H, K in LAYERS:
        fns, nbytes = layer_cases(be, a.batch, C, H, K)
        keys = list(fns)
        for k in keys:   # eager first: kernel attributes, tuning
            for _ in range(2):
                fns[k]()
        torch.cuda.synchronize()
        graphs = {k: StepGraph(lambda fn=fns[k]: [fn() for _ in range(a.burst)], warmup=1) for k in keys}
        reps = {k: [] for k in keys}
        for _ in range(a.repeats):
            win = {k: [] for k in keys}
            for _ in range(a.iters):
                for k in keys:
                    win[k].append(window_us(graphs[k], a.burst))
            for k in keys:
                reps[k].append(sorted(win[k])[len(win[k]) // 2])
        med = {k: sorted(reps[k])[len(reps[k]) // 2] for k in keys}
        rate = {k: nbytes[k] / med[k] / 1e3 for k in keys}
        name = f"{C}@{H} -> {K}@{H // 2}"
        for k in keys:
            lines.append(f"{name:<26}{k:<18}{' '.join(f'{v:8.1f}' for v in reps[k]):<30}{nbytes[k] / 1e6:8.1f}"
                         f"{rate[k]:8.0f}{rate[k] / rate['bn_apply']:17.2f}x")
        print("\n".join(lines[-len(keys):]), flush=True)
        del graphs, fns
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
