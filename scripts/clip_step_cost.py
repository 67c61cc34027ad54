"""Cost of the gradient guard (global-norm clipping + non-finite step guard, csrc/kernels/gradguard.hip)
on a ResNet-50-sized flat gradient (25.6 M elements, random values), fp32 and bf16. Three variants per
row, each one call = both launches of drn_grad_guard (or the torch ops of the baseline):

  (a) the guard with no clip triggered (clip far above the norm): one read of the gradient,
  (b) the guard with the clip triggered on every call: one more read and one write,
  (c) a baseline in torch: n = linalg.vector_norm(g) ; g.mul_(c / max(n, c)) (always multiplies).

Each timed window is one replay of a HIP graph of `--burst` back-to-back calls between two device
events; the gradient is restored before every window (outside it), and call k of a burst clips to
0.999^(k+1) of the restored norm, so every call of (b) really scales. The figure is the median (and
minimum) over `--iters` windows, per call, the variants alternating window by window.

Then, unless --no_step: Executor.train_step on ImageNet ResNet-50 (--batch_size, eager steps) without
the guard (the deferred-tail update), with a guard that never clips and with one that always clips
(both join before their single update), alternating in windows of --step_burst steps.

Writes profiles/clip_step_cost.txt (--out).

    python scripts/clip_step_cost.py [--out FILE] [--iters 30] [--burst 20] [--no_step]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_resnet_tensorflow_amd.models.spec import build_spec  # noqa: E402
from distributed_resnet_tensorflow_amd.ops.backend import GUARD_GRID, HipBackend, guard_record_read, guard_record_tensor  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.params import ParamStore  # noqa: E402


def window_us(graph, burst, pre):
    pre()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / burst


def timed(bursts, pre, iters, burst, warmup=3):
    """Median and minimum microseconds per call of each burst function, alternating window by window."""
    graphs = []
    for fn in bursts:
        pre()
        graphs.append(StepGraph(fn, warmup=1))
    for g in graphs:
        for _ in range(warmup):
            window_us(g, burst, pre)
    us = [[] for _ in bursts]
    for _ in range(iters):
        for i, g in enumerate(graphs):
            us[i].append(window_us(g, burst, pre))
    return [(sorted(u)[len(u) // 2], min(u)) for u in us]


def kernel_rows(be, a, lines):
    P = ParamStore(build_spec("imagenet", 50), "cuda", keep_bf16=False, seed=0)
    n = P.total
    partials = torch.zeros(GUARD_GRID, device="cuda")
    lines.append(f"flat gradient of the ResNet-50 ImageNet ParamStore: {n} elements; {torch.cuda.get_device_name(0)}; us per "
                 f"call, median (min) of {a.iters} replays of a HIP graph of {a.burst} back-to-back calls, the gradient "
                 f"restored before each replay, the variants alternating. (a) guard, clip not triggered; (b) guard, clip "
                 f"triggered on every call; (c) torch.linalg.vector_norm + mul_")
    for wire in ("fp32", "bf16"):
        g0 = torch.randn(n, device="cuda") * 1e-3
        g0 = g0 if wire == "fp32" else g0.bfloat16()
        g = g0.clone()
        norm = float(torch.linalg.vector_norm(g0.double()))
        clips = [norm * 0.999 ** (k + 1) for k in range(a.burst)]
        rec = [guard_record_tensor("cuda") for _ in range(2)]

        def restore():
            g.copy_(g0)

        def unclipped():
            for _ in range(a.burst):
                be.grad_guard(g, 1.0, 1e30, True, None, partials, rec[0])

        def clipped():
            for c in clips:
                be.grad_guard(g, 1.0, c, True, None, partials, rec[1])

        cts = [torch.tensor(c, device="cuda") for c in clips]

        def baseline():
            for c in cts:
                nrm = torch.linalg.vector_norm(g, dtype=torch.float32)
                g.mul_((c / torch.maximum(nrm, c)).to(g.dtype))

        (am, alo), (bm, blo), (cm, clo) = timed([unclipped, clipped, baseline], restore, a.iters, a.burst)
        ra, rb = guard_record_read(rec[0]), guard_record_read(rec[1])
        assert ra["clipped_total"] == 0 and rb["clipped_total"] == rb["steps_total"] > 0, (ra, rb)
        esz = 4 if wire == "fp32" else 2
        lines.append(f"grad {wire}:  (a) {am:.1f} ({alo:.1f}) = {n * esz / (am * 1e-6) / 1e12:.2f} TB/s read   "
                     f"(b) {bm:.1f} ({blo:.1f}) = {3 * n * esz / (bm * 1e-6) / 1e12:.2f} TB/s (2 reads + 1 write)   "
                     f"(c) {cm:.1f} ({clo:.1f})   (b) - (a) {bm - am:+.1f}   (c) - (b) {cm - bm:+.1f}")


def step_rows(be, a, lines):
    from distributed_resnet_tensorflow_amd.runtime.executor import Executor
    spec = build_spec("imagenet", 50)
    variants = [("guard off (deferred tail)", {}), ("guard on, never clips", dict(clip_grad_norm=1e30, skip_nonfinite_grads=True)),
                ("guard on, always clips", dict(clip_grad_norm=1e-3, skip_nonfinite_grads=True))]
    exs = []
    for name, kw in variants:
        ex = Executor(spec, a.batch_size, be, "cuda", seed=1234, weight_decay=1e-4, **kw)
        be.synthetic_images(ex.images, seed=17)
        gen = torch.Generator().manual_seed(5)
        ex.labels.copy_(torch.randint(0, spec.num_classes, (a.batch_size,), generator=gen, dtype=torch.int32))
        ex.set_lr(1e-3)
        if not exs:
            ex.autotune()
        exs.append(ex)

    def window_ms(ex):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.step_burst):
            ex.train_step()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / a.step_burst

    for ex in exs:
        window_ms(ex)
    ms = [[] for _ in exs]
    for _ in range(a.step_iters):
        for i, ex in enumerate(exs):
            ms[i].append(window_ms(ex))
    lines.append("")
    lines.append(f"Executor.train_step, ImageNet ResNet-50 bs{a.batch_size}, eager steps (host-issued launches), ms per step, "
                 f"median (min) of {a.step_iters} windows of {a.step_burst} steps, the variants alternating in one process:")
    base = sorted(ms[0])[len(ms[0]) // 2]
    for (name, _), u, ex in zip(variants, ms, exs):
        med = sorted(u)[len(u) // 2]
        r = ex.grad_guard_stats()
        note = "" if r is None else f"   clipped {r['clipped_total']} of {r['steps_total']} steps"
        lines.append(f"  {name:28s} {med:.3f} ({min(u):.3f})   {med - base:+.3f} ms vs off{note}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "clip_step_cost.txt"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--no_step", action="store_true")
    ap.add_argument("--batch_size", type=int, default=128)
    ap.add_argument("--step_iters", type=int, default=7)
    ap.add_argument("--step_burst", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_step_cost.py times HIP kernels: it needs a GPU")
    be = HipBackend("cuda")
    lines = []
    kernel_rows(be, a, lines)
    if not a.no_step:
        step_rows(be, a, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
