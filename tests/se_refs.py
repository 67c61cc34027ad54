"""fp64 references of the Squeeze-and-Excitation kernels (csrc/kernels/se.hip), each with a per-element
bound derived from the operation (the style and the constants of kernel_refs.py):

  * an fp32 sum of n terms in S cells, any order:  (n + S + c) U sum |terms|
  * a K-step MFMA fp32 dot product:                (K + c) A23 sum |a||b|  + the inputs' errors propagated
  * a bf16 output:                                 + BF |ref|
Every reference takes the kernel's ACTUAL inputs (what the previous kernel stored), so a bound covers one
kernel only.
"""
import torch

from kernel_refs import A23, BF, U

# Relative error of the kernel's sigmoid 1 / (1 + expf(-x)) given x, in units of U: the only constant not
# counted from the code. Measured on an MI355X against fp64 over x in [-12, 12] (scripts/se_cost.py
# --sigmoid): maximum 1.993; chosen = twice that.
SIGMOID_ULPS = 4.0


def squeeze(u, g, S):
    """sum_S cells[n, :, c] = sum_hw u (or g * u: the products of two bf16 are exact in fp32)."""
    t = u.double() if g is None else u.double() * g.double()
    t = t.reshape(t.shape[0], -1, t.shape[-1])
    return t.sum(1), (t.shape[1] + S + 2) * U * t.abs().sum(1)


def gate_fwd(cells, hw, w1, b1, w2, b2):
    """(z, h, s) and their bounds: z = sum_S cells * fl(1 / hw) (c = 3); GEMM 1 over C in four wave partials
    (c = 6: partials, bias), ReLU is 1-Lipschitz; GEMM 2 over Cr (c = 2); sigmoid' <= 1 / 4."""
    cells, w1, b1, w2, b2 = (t.double().cpu() for t in (cells, w1, b1, w2, b2))
    S, C, Cr = cells.shape[1], w1.shape[0], w1.shape[1]
    z = cells.sum(1) / hw
    ez = (S + 3) * U * cells.abs().sum(1) / hw
    l1 = z @ w1 + b1
    e1 = (C + 6) * A23 * (z.abs() @ w1.abs() + b1.abs()) + ez @ w1.abs()
    h = l1.clamp_min(0)
    l2 = h @ w2 + b2
    e2 = (Cr + 2) * A23 * (h.abs() @ w2.abs() + b2.abs()) + e1 @ w2.abs()
    s = torch.sigmoid(l2)
    return (z, ez), (h, e1), (s, e2 / 4 + SIGMOID_ULPS * U * s)


def gate_bwd(cells, hw, w1, w2, h, s):
    """(dl2, dh, dzs) from the cells of g * u and the STORED h, s (so the ReLU mask is the kernel's set):
    dl2 = ds s (1 - s), three roundings (c = 4)."""
    cells, w1, w2, h, s = (t.double().cpu() for t in (cells, w1, w2, h, s))
    S, C, Cr = cells.shape[1], w1.shape[0], w1.shape[1]
    sp = s * (1 - s)
    dl2 = cells.sum(1) * sp
    e0 = (S + 1) * U * cells.abs().sum(1) * sp + 4 * U * dl2.abs()
    mask = (h > 0).double()
    dh = (dl2 @ w2.t()) * mask
    e1 = ((C + 6) * A23 * (dl2.abs() @ w2.abs().t()) + e0 @ w2.abs().t()) * mask
    dz = dh @ w1.t()
    e2 = (Cr + 2) * A23 * (dh.abs() @ w1.abs().t()) + e1 @ w1.abs().t()
    return (dl2, e0), (dh, e1), (dz / hw, (e2 + 3 * U * dz.abs()) / hw)


def gate_wgrad(z, h, dl2, dh):
    """dw1 = z^T dh, db1 = sum_n dh, dw2 = h^T dl2, db2 = sum_n dl2: N steps each."""
    z, h, dl2, dh = (t.double().cpu() for t in (z, h, dl2, dh))
    n = z.shape[0] + 2
    return ((z.t() @ dh, n * A23 * (z.abs().t() @ dh.abs())), (dh.sum(0), n * U * dh.abs().sum(0)),
            (h.t() @ dl2, n * A23 * (h.abs().t() @ dl2.abs())), (dl2.sum(0), n * U * dl2.abs().sum(0)))


def scale_add(s, x, add):
    """bf16(fma(s, x, add)), s broadcast over the pixels: one fp32 rounding, then the bf16 one."""
    ref = s.double().cpu()[:, None, None, :] * x.double().cpu() + add
    return ref, BF * ref.abs() + (1 + BF) * U * ref.abs()
