"""Cost of the grouped 3x3 convolution kernels (csrc/kernels/conv_group.hip) on the layers of
ResNeXt-50 32x4d at batch 128: the four stride-1 layers (128 ch @ 56x56, 256 @ 28x28, 512 @ 14x14,
1024 @ 7x7) and the three stride-2 transitions; forward with statistics, data gradient and weight
gradient, each against the in-tree DENSE kernels on the same C = K geometry with their tuned default --
code this feature does not touch, i.e. the yardstick of the parent commit (32 / cg times the MFMA
work, the same activation bytes). (A comparison against a library grouped convolution is not part of
this script.)

Each timed window is one replay of a HIP graph of `--burst` back-to-back calls between two device
events. All cases alternate window by window in one process; the figure per case is the median over
`--iters` windows, printed for each of `--repeats` repeats (their spread shows the noise). Bytes are the
compulsory ones: input + output activations + weights, each once.

Then (unless --no_step) Executor.train_step, eager, of ResNeXt-50 32x4d beside ResNet-50 at batch 128,
alternating in one process. Writes profiles/group_conv_cost.txt (--out).

    python scripts/group_conv_cost.py [--out FILE] [--iters 10] [--burst 100] [--repeats 3] [--no_step]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_resnet_tensorflow_amd.models.spec import build_spec  # noqa: E402
from distributed_resnet_tensorflow_amd.ops.backend import ConvGeom, HipBackend, OutMap, dgrad_geom  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.executor import Executor  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph  # noqa: E402

LAYERS = [(128, 56, 1), (256, 28, 1), (512, 14, 1), (1024, 7, 1), (256, 56, 2), (512, 28, 2), (1024, 14, 2)]
GROUPS = 32


def window_us(graph, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / burst


def layer_cases(be, N, C, H, stride):
    """{(pass, impl): fn} of one layer and its compulsory bytes per pass."""
    cg, P = C // GROUPS, (H - 1) // stride + 1
    bf = dict(dtype=torch.bfloat16, device="cuda")
    x, dy = torch.randn(N, H, H, C, **bf), torch.randn(N, P, P, C, **bf)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    wg, wd = torch.randn(C, 3, 3, cg, **bf) * 0.1, torch.randn(C, 3, 3, C, **bf) * 0.03
    dwg, dwd = torch.empty(C, 3, 3, cg, device="cuda"), torch.empty(C, 3, 3, C, device="cuda")
    stats = torch.zeros(be.stats_replicas, 2, C, device="cuda")
    ws = torch.empty(max(16, be.gconv_wgrad_ws_elems(x.shape, dy.shape, wg.shape, stride),
                         be.wgrad_ws_elems(N * P * P, C, 3, 3, C)), device="cuda")
    g = ConvGeom(stride, 1, 1, 1)
    # the dense data gradient as the executor launches it: one flipped conv, or the stride-2 phases
    if stride == 1:
        phases = [(torch.randn(C, 3, 3, C, **bf) * 0.03, dgrad_geom(g, 3, 3), None)]
    else:
        phases = []
        for ph in range(2):
            rs = [r for r in range(3) if (r - ph - 1) % 2 == 0]
            for pw in range(2):
                ss = [s for s in range(3) if (s - pw - 1) % 2 == 0]
                geom = ConvGeom(1, -((ph + 1 - max(rs)) // 2), -((pw + 1 - max(ss)) // 2), 1)
                phases.append((torch.randn(C, len(rs), len(ss), C, **bf) * 0.03, geom,
                               OutMap((H - ph + 1) // 2, (H - pw + 1) // 2, 2, ph, pw)))
    fns = {
        ("fwd+stats", "grouped"): lambda: be.gconv_fwd(x, wg, y, stride, stats=stats),
        ("fwd+stats", "dense"): lambda: be.conv_fwd(x, wd, y, g, stats=stats),
        ("dgrad", "grouped"): lambda: be.gconv_dgrad(dy, wg, dx, stride),
        ("dgrad", "dense"): lambda: [be.conv_fwd(dy, w_, dx, g_, out_map=m_) for w_, g_, m_ in phases],
        ("wgrad", "grouped"): lambda: be.gconv_wgrad(x, dy, dwg, stride, ws=ws),
        ("wgrad", "dense"): lambda: be.conv_wgrad(x, dy, dwd, g, ws=ws),
    }
    act = (x.numel() + y.numel()) * 2
    nbytes = {"fwd+stats": act + wg.numel() * 2, "dgrad": act + wg.numel() * 2, "wgrad": act + dwg.numel() * 4}
    return fns, nbytes


def step_times(N, rounds, steps):
    """Median ms of Executor.train_step, eager, ResNet-50 and ResNeXt-50 32x4d alternating."""
    exs = {}
    for name, spec in (("resnet50", build_spec("imagenet", 50)),
                       ("resnext50_32x4d", build_spec("imagenet", 50, model="resnext"))):
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
                                                  "profiles", "group_conv_cost.txt"))
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--burst", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no_step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a GPU measurement"
    be = HipBackend("cuda")
    lines = [f"grouped 3x3 conv cost, ResNeXt-50 32x4d layers, batch {a.batch}, {torch.cuda.get_device_name(0)}",
             f"us per call = median of {a.iters} windows of {a.burst} calls in a HIP graph; the column holds that "
             f"median for each of {a.repeats} repeats; GB/s = compulsory bytes (input + output + weights) / median repeat",
             f"{'layer':<22}{'pass':<11}{'impl':<9}{'us (repeats)':<30}{'GB/s':>8}{'vs dense':>10}"]
    for C, H, stride in LAYERS:
        fns, nbytes = layer_cases(be, a.batch, C, H, stride)
        keys = list(fns)
        for k in keys:   # eager first: kernel attributes, tuning, library algorithm search
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
        name = f"{C}ch {H}x{H} s{stride} cg{C // GROUPS}"
        for k in keys:
            med = sorted(reps[k])[len(reps[k]) // 2]
            dense = sorted(reps[(k[0], "dense")])[len(reps[k]) // 2]
            note = "  SLOWER than dense" if k[1] == "grouped" and med > dense else ""
            lines.append(f"{name:<22}{k[0]:<11}{k[1]:<9}"
                         f"{' '.join(f'{v:8.1f}' for v in reps[k]):<30}{nbytes[k[0]] / med / 1e3:8.0f}"
                         f"{med / dense:9.2f}x{note}")
        print("\n".join(lines[-len(keys):]), flush=True)
        del graphs, fns
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
