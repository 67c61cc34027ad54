"""Helpers of tests/test_adam.py and tests/test_adam_gpu.py: the AdamW / LAMB definitions in numpy, the
per-element fp64 reference of the AdamW kernel with its rounding bounds (the tests/kernel_refs.py
convention), shared inputs and the recorded training LRs."""
import numpy as np
import torch

from kernel_refs import U, f32
from test_lars import hand_buffers

from distributed_resnet_tensorflow_amd.models.spec import cifar_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import RefBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor

# hyper-parameters of the kernel-level tests; (c1, c2) are the bias corrections of update t = 3
ADAM_HP = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-6, wd=2e-4, gs=0.5, c1=1 - 0.9 ** 3, c2=1 - 0.999 ** 3)
# constant LRs of the 30-step fixed-batch training tests (cifar_resnet_v2(8), N = 32), picked on the
# fp32 oracle executor (tests/test_adam.py test 7 records the losses); shared with the GPU test
TRAIN_LR = {"adamw": 0.01, "lamb": 0.02}


def hand_adam_buffers(total, slots, seed=5):
    """w, m, v, g (fp64) over the whole buffer, padding and gaps included: test_lars.hand_buffers (with
    its all-zero gradient slot and all-zero weight slot) + v drawn as squared normals."""
    w, m, g = hand_buffers(total, slots, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    v = torch.randn(total, generator=gen, dtype=torch.float64) ** 2
    return w, m, v, g


def numpy_adam(w, m, v, g, slots, lamb, lr, b1, b2, eps, wd, gs, c1, c2):
    """The issue's definitions, per slot, in float64 numpy. Returns w, m, v, trust."""
    w, m, v, trust = w.copy(), m.copy(), v.copy(), np.ones(len(slots))
    for i, (off, n, _, adapt) in enumerate(slots):
        sl = slice(off, off + n)
        gp = gs * g[sl]
        m[sl] = b1 * m[sl] + (1 - b1) * gp
        v[sl] = b2 * v[sl] + (1 - b2) * gp * gp
        u = (m[sl] / c1) / (np.sqrt(v[sl] / c2) + eps) + wd * w[sl]
        if lamb and adapt:
            wn, un = np.sqrt((w[sl] * w[sl]).sum()), np.sqrt((u * u).sum())
            if wn > 0 and un > 0:
                trust[i] = wn / un
        w[sl] = w[sl] - lr * trust[i] * u
    return w, m, v, trust


def adamw_ref(w0, m0, v0, g, lr, b1, b2, eps, wd, gs, c1, c2, e0=None, decay=None):
    """The exact AdamW update in fp64 from the values the kernel sees -- fp32 buffers, the gradient as
    given (bf16-rounded by the caller for the bf16 case), every scalar as its fp32 value -- and a
    per-element bound for each output, first order in U = 2^-24 with one U-relative term per fp32
    rounding of csrc/kernels/adam.hip, taken on the magnitude of the rounded value. The kernel is
    compiled without approximate-math flags: its divisions and its square root are the IEEE
    correctly rounded sequences (v_div_scale / v_div_fmas / v_div_fixup; v_sqrt_f32 with the
    one-ulp fix-up), so each counts as one rounding.

      g' = fl(gs g)                                                       1 rounding
      m  = fma(b1, m0, fl(fl(1 - b1) * g'))    1 - b1, the product (each on |(1 - b1) g'|, + g''s), the fma
           bound_m = U (|b1 m0| + 4 |(1 - b1) g'|)
      v  = fma(b2, v0, fl(fl(1 - b2) * fl(g' g')))   g'^2 carries 2 (from g') + 1, then as m
           bound_v = U (|b2 v0| + 6 (1 - b2) g'^2)
      mh = fl(m / c1)        e_mh = bound_m / c1 + U |mh|
      vh = fl(v / c2)        e_vh = bound_v / c2 + U vh
      s  = fl(sqrt(vh))      e_s  = e_vh / (2 s) + U s          (0 where vh == 0: then v0 == g == 0)
      d  = fl(s + eps)       e_d  = e_s + U d
      r  = fl(mh / d)        e_r  = e_mh / d + |r| e_d / d + U |r|
      u  = fma(wd, w0, r)    e_u  = e_r + U (|wd w0| + |r|)
      st = fl(lr u)          e_st = lr e_u + U |lr u|
      w  = fl(w0 - st)       bound_w = e_st + U (|w0| + |lr u|)
      EMA (decay d read as fp32): om = fl(1 - d); ema = fl(e0 - fl(om * fl(e0 - w)))
           e_df = bound_w + U |e0 - w|;  e_p = om e_df + 2 U |om (e0 - w)|;  bound_e = e_p + U (|e0| + |om (e0 - w)|)

    Every bound is scaled by (1 + 2^-10) for the second-order terms. Returns a dict of (ref, bound)
    for "w", "m", "v" (and "ema")."""
    lr, b1, b2, eps, wd, gs, c1, c2 = (f32(x) for x in (lr, b1, b2, eps, wd, gs, c1, c2))
    w0, m0, v0, g = (t.double() for t in (w0, m0, v0, g))
    ob1, ob2 = 1.0 - b1, 1.0 - b2
    gp = gs * g
    m = b1 * m0 + ob1 * gp
    v = b2 * v0 + ob2 * gp * gp
    bm = U * ((b1 * m0).abs() + 4 * (ob1 * gp).abs())
    bv = U * ((b2 * v0).abs() + 6 * ob2 * gp * gp)
    mh, vh = m / c1, v / c2
    e_mh = bm / c1 + U * mh.abs()
    e_vh = bv / c2 + U * vh
    s = vh.sqrt()
    e_s = torch.where(s > 0, e_vh / (2 * s).clamp_min(1e-300), torch.zeros_like(s)) + U * s
    d = s + eps
    e_d = e_s + U * d
    r = mh / d
    e_r = e_mh / d + r.abs() * e_d / d + U * r.abs()
    u = r + wd * w0
    e_u = e_r + U * ((wd * w0).abs() + r.abs())
    e_st = lr * e_u + U * (lr * u).abs()
    w = w0 - lr * u
    bw = e_st + U * (w0.abs() + (lr * u).abs())
    k = 1 + 2.0 ** -10
    out = {"w": (w, k * bw), "m": (m, k * bm), "v": (v, k * bv)}
    if e0 is not None:
        om = 1.0 - f32(decay)
        e0 = e0.double()
        df = e0 - w
        e_p = om * (bw + U * df.abs()) + 2 * U * (om * df).abs()
        out["ema"] = (e0 - om * df, k * (e_p + U * (e0.abs() + (om * df).abs())))
    return out


def fixed_batch_executor(optimizer, N=32, seed=3, backend=None, device="cpu", **kw):
    """cifar_resnet_v2(8) on one fixed batch (the setup of tests/test_lars.py's training test)."""
    ex = Executor(cifar_resnet_v2(8), N, backend or RefBackend(), device, seed=seed, optimizer=optimizer, **kw)
    g = torch.Generator().manual_seed(11)
    ex.images.zero_()
    ex.images[..., :3] = torch.randn(N, 32, 32, 3, generator=g).bfloat16().to(ex.images.dtype).to(device)
    ex.labels.copy_(torch.randint(0, 10, (N,), generator=g, dtype=torch.int32))
    return ex
