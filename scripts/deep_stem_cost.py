"""Cost of the deep-stem kernels (csrc/kernels/stem_deep.hip) at batch 128, 224 x 224: each fused kernel
beside the composed launches it replaces (the dense conv, the materialising bn_apply, maxpool_fwd) and
beside bn_apply on the 112 x 112 x 32 tensor as the streaming yardstick; then the whole fused forward of
the stem against the composed one (DRN_DEEP_STEM_FUSED=0), both through Executor._deep_stem_fwd.

Each timed window is one replay of a HIP graph of `--burst` back-to-back calls between two device
events. All cases alternate window by window in one process; the figure per case is the median over
`--iters` windows, printed for each of `--repeats` repeats (their spread shows the noise). Bytes are the
compulsory ones, each tensor once (a composed case: of the launches it is made of, so the materialised
activations count twice, written and read).

Then (unless --no_step) Executor.train_step, eager, of ResNet-50 with and without deep_stem at batch 128,
alternating in one process. Writes profiles/deep_stem_cost.txt (--out).

    python scripts/deep_stem_cost.py [--out FILE] [--iters 10] [--burst 20] [--repeats 3] [--no_step]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_resnet_tensorflow_amd.models.spec import build_spec  # noqa: E402
from distributed_resnet_tensorflow_amd.ops.backend import ConvGeom, HipBackend  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.executor import Executor  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph  # noqa: E402


def window_us(graph, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / burst


def kernel_cases(be, N, img):
    """{case: fn} of the three layers and the compulsory bytes of each."""
    bf = dict(dtype=torch.bfloat16, device="cuda")
    hs, ph = img // 2, img // 4
    x = torch.randn(N, img, img, 8, **bf)
    h0, a0, h1, a1 = (torch.randn(N, hs, hs, 32, **bf) for _ in range(4))
    y2 = torch.empty(N, hs, hs, 64, **bf)
    pool, arg = torch.empty(N, ph, ph, 64, **bf), torch.empty(N, ph, ph, 64, dtype=torch.uint8, device="cuda")
    w0, w1, w2 = (torch.randn(k, 3, 3, c, **bf) * 0.05 for k, c in ((32, 8), (32, 32), (64, 32)))
    scale, shift = torch.rand(32, device="cuda") + 0.5, torch.randn(32, device="cuda")
    s32, s64 = torch.zeros(8, 2, 32, device="cuda"), torch.zeros(8, 2, 64, device="cuda")
    g2, g1 = ConvGeom(2, 1, 1, 1), ConvGeom(1, 1, 1, 1)
    bn = (scale, shift)

    def composed1():
        be.bn_apply(h0, a0, scale, shift, relu=True)
        be.conv_fwd(a0, w1, h1, g1, stats=s32)

    def composed2():
        be.bn_apply(h1, a1, scale, shift, relu=True)
        be.conv_fwd(a1, w2, y2, g1)
        be.maxpool_fwd(y2, pool, arg, 3, 2, 0, 0, stats=s64)
    fns = {
        "conv2d fused": lambda: be.stem_deep_conv(x, w0, h0, 2, stats=s32),
        "conv2d dense": lambda: be.conv_fwd(x, w0, h0, g2, stats=s32),
        "conv2d_1 fused": lambda: be.stem_deep_conv(h0, w1, h1, 1, in_bn=bn, stats=s32),
        "conv2d_1 composed": composed1,
        "conv2d_2+pool fused": lambda: be.stem_deep_conv_pool(h1, w2, pool, arg, 1, in_bn=bn, stats=s64),
        "conv2d_2+pool composed": composed2,
        "bn_apply 112x112x32": lambda: be.bn_apply(h0, a0, scale, shift, relu=True),
    }
    xb, hb, yb, pb = x.numel() * 2, h0.numel() * 2, y2.numel() * 2, pool.numel() * 3
    nbytes = {"conv2d fused": xb + hb, "conv2d dense": xb + hb, "conv2d_1 fused": 2 * hb,
              "conv2d_1 composed": 4 * hb, "conv2d_2+pool fused": hb + pb, "conv2d_2+pool composed": 3 * hb + 2 * yb + pb,
              "bn_apply 112x112x32": 2 * hb}
    return fns, nbytes


def forward_cases(N, img):
    """The stem's whole forward through the executor, fused and composed (two executors, one process)."""
    fns = {}
    for name, fused in (("stem forward fused", "1"), ("stem forward composed", "0")):
        os.environ["DRN_DEEP_STEM_FUSED"] = fused
        be = HipBackend("cuda")
        ex = Executor(build_spec("imagenet", 18, deep_stem=True), N, be, "cuda", seed=0)
        be.synthetic_images(ex.images, seed=3)

        def fwd(ex=ex, be=be):
            ex._deep_stem_fwd(True)
            if not ex.deep_fused:
                be.maxpool_fwd(ex.stem_out, ex.pool_out, ex.pool_arg, 3, 2, 0, 0, stats=ex.pool_stats)
        fns[name] = fwd
    os.environ.pop("DRN_DEEP_STEM_FUSED")
    hb = N * (img // 2) ** 2 * 32 * 2
    nbytes = {"stem forward fused": N * img * img * 16 + 4 * hb + N * (img // 4) ** 2 * 64 * 3}
    nbytes["stem forward composed"] = nbytes["stem forward fused"] + 4 * hb + 2 * 2 * hb
    return fns, nbytes


def measure(fns, nbytes, a, lines, yardstick=None):
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
    for k in keys:
        vs = f"{rate[k] / rate[yardstick]:17.2f}x" if yardstick else ""
        lines.append(f"{k:<26}{' '.join(f'{v:8.1f}' for v in reps[k]):<30}{nbytes[k] / 1e6:8.1f}{rate[k]:8.0f}{vs}")
    print("\n".join(lines[-len(keys):]), flush=True)


def step_times(N, rounds, steps):
    """Median ms of Executor.train_step, eager, ResNet-50 without and with deep_stem, alternating."""
    exs = {}
    for name, spec in (("resnet50", build_spec("imagenet", 50)),
                       ("resnet50 deep_stem", build_spec("imagenet", 50, deep_stem=True))):
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
                                                  "profiles", "deep_stem_cost.txt"))
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no_step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a GPU measurement"
    be = HipBackend("cuda")
    lines = [f"Deep stem cost, 224 x 224, batch {a.batch}, {torch.cuda.get_device_name(0)}",
             f"us per call = median of {a.iters} windows of {a.burst} calls in a HIP graph; the column holds that "
             f"median for each of {a.repeats} repeats; GB/s = compulsory bytes / median repeat",
             f"{'case':<26}{'us (repeats)':<30}{'MB':>8}{'GB/s':>8}{'vs bn_apply GB/s':>18}"]
    measure(*kernel_cases(be, a.batch, 224), a, lines, yardstick="bn_apply 112x112x32")
    torch.cuda.empty_cache()
    measure(*forward_cases(a.batch, 224), a, lines)
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
