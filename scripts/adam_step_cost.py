"""Cost of the AdamW / LAMB updates (csrc/kernels/adam.hip) against the momentum / LARS updates on the
ResNet-50 ImageNet parameter store (25.6 M elements, random gradients): each of the four optimizers
with and without the fused weight EMA, for the fp32 and the bf16 wire gradient -- 16 cases.

Each timed window is one replay of a HIP graph of `--burst` back-to-back updates (no host enqueue cost
in the window, as in a graph / plan step) between two device events. All cases alternate window by
window in one process, so they share clocks and cache state; the figure per case is the median over
`--iters` windows, reported for each of `--repeats` repeats (their spread shows the noise), with the
bytes moved per update and the achieved bytes/s of the median repeat. The yardsticks are measured in
the same run: AdamW's bytes/s against the momentum kernel's, LAMB's (both passes) against LARS's.

Then (unless --no_step) Executor.train_step on ImageNet ResNet-50 for momentum, AdamW and LAMB, the
three alternating in one process. Writes profiles/adam_step_cost.txt (--out).

    python scripts/adam_step_cost.py [--out FILE] [--iters 10] [--burst 20] [--repeats 3] [--no_step]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_resnet_tensorflow_amd.models.spec import build_spec  # noqa: E402
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend, lars_table  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.graph import StepGraph  # noqa: E402
from distributed_resnet_tensorflow_amd.runtime.params import ParamStore  # noqa: E402

DECAY = 0.999


def window_us(graph, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / burst


def bytes_per_element(opt, ema, gsz):
    """fp32 reads and writes + the bf16 weight copy + the gradient (+ 8 for the EMA's read and write).
    momentum: w, m read and written. LARS: + w, g read by the norms pass. AdamW: w, m, v read and
    written. LAMB: pass 1 reads w, m, v, g and writes m, v; pass 2 reads w, m, v and writes w."""
    base = {"momentum": 4 * 4 + 2 + gsz, "lars": 4 * 4 + 2 + gsz + 4 + gsz, "adamw": 6 * 4 + 2 + gsz,
            "lamb": (5 * 4 + gsz) + (4 * 4 + 2)}[opt]
    return base + (8 if ema else 0)


def kernel_rows(be, a, lines):
    P = ParamStore(build_spec("imagenet", 50), "cuda", keep_bf16=True, seed=0, ema=True, adam=True)
    table = lars_table(P)
    partials = torch.zeros(2 * table.chunks, device="cuda")
    trust = torch.ones(table.n, device="cuda")
    lr = torch.full((1,), 1e-6, device="cuda")
    d = torch.full((1,), DECAY, device="cuda")
    bc = torch.tensor([1 - 0.9 ** 100, 1 - 0.999 ** 100], dtype=torch.float32, device="cuda")
    grads = {"fp32": torch.randn(P.total, device="cuda") * 1e-3}
    grads["bf16"] = grads["fp32"].bfloat16()
    P.adam_v.copy_(grads["fp32"] ** 2)

    def update(opt, ema, g):
        kw = dict(ema=P.ema, ema_decay_t=d) if ema else {}
        if opt == "momentum":
            be.sgd_momentum(P.master, P.momentum, g, P.wbf16, lr, 0.9, 1e-4, 1.0, **kw)
        elif opt == "lars":
            be.lars_momentum(P.master, P.momentum, g, P.wbf16, table, 0, table.n, partials, trust, lr, 0.9, 1e-4, 1.0,
                             0.001, 1e-9, **kw)
        elif opt == "adamw":
            be.adamw(P.master, P.momentum, P.adam_v, g, P.wbf16, lr, bc, 0.9, 0.999, 1e-6, 1e-4, 1.0, **kw)
        else:
            be.lamb(P.master, P.momentum, P.adam_v, g, P.wbf16, table, 0, table.n, partials, trust, lr, bc, 0.9, 0.999,
                    1e-6, 1e-4, 1.0, **kw)

    cases = [(opt, ema, wire) for wire in ("fp32", "bf16") for ema in (False, True)
             for opt in ("momentum", "lars", "adamw", "lamb")]
    graphs = [StepGraph(lambda c=c: [update(c[0], c[1], grads[c[2]]) for _ in range(a.burst)], warmup=1)
              for c in cases]
    for g in graphs:
        for _ in range(3):
            window_us(g, a.burst)
    med = [[] for _ in cases]
    for _ in range(a.repeats):
        us = [[] for _ in cases]
        for _ in range(a.iters):
            for i, g in enumerate(graphs):
                us[i].append(window_us(g, a.burst))
        for i, u in enumerate(us):
            med[i].append(sorted(u)[len(u) // 2])
    lines.append(f"ResNet-50 ImageNet ParamStore: {P.total} elements ({table.n} slots); {torch.cuda.get_device_name(0)}; "
                 f"us per update inside a HIP graph of {a.burst} back-to-back updates on the same buffers: the median "
                 f"of {a.iters} replays, for each of {a.repeats} repeats; all {len(cases)} cases alternate window by "
                 f"window. MB per update and TB/s of the median repeat.")
    rate = {}
    for c, m in zip(cases, med):
        opt, ema, wire = c
        mb = P.total * bytes_per_element(opt, ema, 4 if wire == "fp32" else 2) / 1e6
        mid = sorted(m)[len(m) // 2]
        rate[c] = mb / mid   # MB / us = TB/s
        lines.append(f"{opt:8s} ema {'on ' if ema else 'off'} grad {wire}:  " + "  ".join(f"{x:7.1f}" for x in m) +
                     f"  (spread {max(m) - min(m):.1f})   {mb:7.1f} MB   {rate[c]:.2f} TB/s")
    lines.append("")
    lines.append("achieved bytes/s against the yardstick measured in this run (accepted: >= 0.90):")
    for wire in ("fp32", "bf16"):
        for ema in (False, True):
            ra = rate[("adamw", ema, wire)] / rate[("momentum", ema, wire)]
            rl = rate[("lamb", ema, wire)] / rate[("lars", ema, wire)]
            lines.append(f"  grad {wire} ema {'on ' if ema else 'off'}:  adamw / momentum {ra:.3f} "
                         f"{'ok' if ra >= 0.9 else 'MISSES the yardstick'}   lamb / lars {rl:.3f} "
                         f"{'ok' if rl >= 0.9 else 'MISSES the yardstick'}")


def step_rows(be, a, lines):
    from distributed_resnet_tensorflow_amd.runtime.executor import Executor
    spec = build_spec("imagenet", 50)
    exs = []
    for opt in a.step_opts.split(","):
        ex = Executor(spec, a.batch_size, be, "cuda", seed=1234, weight_decay=1e-4, optimizer=opt)
        be.synthetic_images(ex.images, seed=17)
        gen = torch.Generator().manual_seed(5)
        ex.labels.copy_(torch.randint(0, spec.num_classes, (a.batch_size,), generator=gen, dtype=torch.int32))
        ex.set_lr(1e-5)
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
    lines.append(f"Executor.train_step, ImageNet ResNet-50 bs{a.batch_size}, eager steps (host-issued launches), ms per "
                 f"step, median (min) of {a.step_iters} windows of {a.step_burst} steps, the optimizers alternating in "
                 f"one process:")
    names = [ex.optimizer for ex in exs]
    ref = names.index("momentum") if "momentum" in names else 0
    base = sorted(ms[ref])[len(ms[ref]) // 2]
    for ex, u in zip(exs, ms):
        mid = sorted(u)[len(u) // 2]
        lines.append(f"  {ex.optimizer:10s} {mid:.3f} ({min(u):.3f})   {mid - base:+.3f} ms vs {names[ref]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "adam_step_cost.txt"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no_step", action="store_true")
    ap.add_argument("--batch_size", type=int, default=128)
    ap.add_argument("--step_iters", type=int, default=7)
    ap.add_argument("--step_burst", type=int, default=10)
    ap.add_argument("--step_opts", default="momentum,adamw,lamb",
                    help="optimizers of the train_step rows, in the order their executors are built (the first is "
                         "the baseline)")
    ap.add_argument("--no_kernels", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_step_cost.py times HIP kernels: it needs a GPU")
    be = HipBackend("cuda")
    lines = []
    if not a.no_kernels:
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
