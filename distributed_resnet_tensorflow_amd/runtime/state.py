"""Executor <-> checkpoint tensors (TF variable names and layouts).

Names follow tf.layers auto-naming + TF1 optimizer/BN conventions: trainable
`conv2d_7/kernel` (HWIO), `batch_normalization_3/{gamma,beta}`, `dense/{kernel,bias}`, slots
`<var>/Momentum`, non-trainable `batch_normalization_3/{moving_mean,moving_variance}` and
`global_step` (int64 scalar). With the weight EMA on (Executor(ema_decay > 0)) every trainable
variable also has its tf.train.ExponentialMovingAverage shadow `<var>/ExponentialMovingAverage`
(TF layout; the BN moving statistics are averages already and have none). With an Adam-family
optimizer (adamw, lamb) the slots are tf.train.AdamOptimizer's instead of `<var>/Momentum`: `<var>/Adam`
(m), `<var>/Adam_1` (v), the fp32 scalars `beta1_power` / `beta2_power` (the powers the next update
uses) and `drn/adam_t0` (int64: the global_step at which the moments were last zero-initialised).
"""
from __future__ import annotations

import logging
from typing import Dict, Optional

import numpy as np
import torch

GLOBAL_STEP = "global_step"
EMA_SUFFIX = "/ExponentialMovingAverage"
ADAM_M, ADAM_V = "Adam", "Adam_1"   # tf.train.AdamOptimizer's slot names (first / second moment)
ADAM_T0 = "drn/adam_t0"             # global_step at which the moments were last zero-initialised

log = logging.getLogger("drn")


class NoEmaInCheckpoint(RuntimeError):
    """The averaged weights were asked for (--eval_ema) from a checkpoint written without them."""


def has_ema(tensors) -> bool:
    return any(k.endswith(EMA_SUFFIX) for k in tensors)


def export_state(ex, extra: Optional[Dict[str, int]] = None) -> Dict[str, np.ndarray]:
    P = ex.P
    out: Dict[str, np.ndarray] = {}
    adam = getattr(P, "adam_v", None) is not None
    for s in P.slots:
        out[s.name] = P.to_tf(s.name).numpy()
        if adam:   # TF's AdamOptimizer slot names: m, v
            out[f"{s.name}/{ADAM_M}"] = P.to_tf(s.name, buf=P.momentum).numpy()
            out[f"{s.name}/{ADAM_V}"] = P.to_tf(s.name, buf=P.adam_v).numpy()
        else:
            out[f"{s.name}/Momentum"] = P.to_tf(s.name, buf=P.momentum).numpy()
        if P.ema is not None:
            out[s.name + EMA_SUFFIX] = P.to_tf(s.name, buf=P.ema).numpy()
    for bn in P.bn_slots:
        m, v = P.moving(bn)
        out[f"{bn}/moving_mean"] = m.detach().float().cpu().numpy().copy()
        out[f"{bn}/moving_variance"] = v.detach().float().cpu().numpy().copy()
    out[GLOBAL_STEP] = np.array(P.global_step, dtype=np.int64)
    if adam:
        # TF's beta1_power / beta2_power: the powers the next update uses (b^t, t = step - t0 + 1)
        t = max(P.global_step - P.adam_t0, 0) + 1
        out["beta1_power"] = np.array(ex.adam_beta1 ** t, dtype=np.float32)
        out["beta2_power"] = np.array(ex.adam_beta2 ** t, dtype=np.float32)
        out[ADAM_T0] = np.array(P.adam_t0, dtype=np.int64)
    for k, v in (extra or {}).items():
        out[f"drn/{k}"] = np.array(v, dtype=np.int64)
    return out


def import_state(ex, tensors: Dict[str, np.ndarray], strict: bool = True, use_ema: bool = False) -> Dict[str, int]:
    """Load a checkpoint's tensors into the executor. use_ema: the variables take the values of
    their `<var>/ExponentialMovingAverage` shadows (evaluation on the averaged weights);
    NoEmaInCheckpoint if the checkpoint has none. With the executor's own EMA on, the shadows are
    restored, or -- a checkpoint written without them -- seeded from the restored weights."""
    P = ex.P
    if use_ema:
        absent = [s.name for s in P.slots if s.name + EMA_SUFFIX not in tensors]
        if absent:
            raise NoEmaInCheckpoint(f"the checkpoint has no {EMA_SUFFIX[1:]} for {len(absent)} of {len(P.slots)} "
                                    f"variables (e.g. {absent[0]}): it was not trained with --ema_decay")
        tensors = {**tensors, **{s.name: tensors[s.name + EMA_SUFFIX] for s in P.slots}}
    missing, seeded = [], 0
    adam = getattr(P, "adam_v", None) is not None
    # an Adam-family executor takes both moments or neither: a checkpoint without them (e.g. one
    # trained with momentum) restarts them from zero at the restored step
    adam_ok = adam and ADAM_T0 in tensors and all(f"{s.name}/{k}" in tensors for s in P.slots for k in (ADAM_M, ADAM_V))
    if adam and not adam_ok:
        P.momentum.zero_()
        P.adam_v.zero_()
    for s in P.slots:
        if s.name in tensors:
            P.from_tf(s.name, torch.from_numpy(np.asarray(tensors[s.name])))
        else:
            missing.append(s.name)
        if P.ema is not None:
            ek = s.name + EMA_SUFFIX
            if ek in tensors:
                P.from_tf(s.name, torch.from_numpy(np.asarray(tensors[ek])), buf=P.ema)
            else:
                P.seed_ema(s.name)
                seeded += 1
        if adam:
            if adam_ok:
                P.from_tf(s.name, torch.from_numpy(np.asarray(tensors[f"{s.name}/{ADAM_M}"])), buf=P.momentum)
                P.from_tf(s.name, torch.from_numpy(np.asarray(tensors[f"{s.name}/{ADAM_V}"])), buf=P.adam_v)
            continue
        mk = f"{s.name}/Momentum"
        if mk in tensors:
            P.from_tf(s.name, torch.from_numpy(np.asarray(tensors[mk])), buf=P.momentum)
        else:
            P.view(P.momentum, s.name).zero_()
    for bn in P.bn_slots:
        m, v = P.moving(bn)
        for t, key in ((m, "moving_mean"), (v, "moving_variance")):
            k = f"{bn}/{key}"
            if k in tensors:
                t.copy_(torch.from_numpy(np.asarray(tensors[k], dtype=np.float32)).to(t.dtype))
            else:
                missing.append(k)
    if seeded:
        log.warning("checkpoint has no %s for %d of %d variables: their averages start from the restored weights",
                    EMA_SUFFIX[1:], seeded, len(P.slots))
    if strict and missing:
        raise KeyError(f"checkpoint is missing {len(missing)} variables, e.g. {missing[:3]}")
    P.global_step = int(np.asarray(tensors.get(GLOBAL_STEP, 0)))
    if adam:
        if adam_ok:
            P.adam_t0 = int(np.asarray(tensors[ADAM_T0]))
        else:
            P.adam_t0 = P.global_step
            log.warning("checkpoint has no Adam moments (%s, %s): both start from zero at global_step %d",
                        ADAM_M, ADAM_V, P.global_step)
        ex.set_adam_step(P.global_step)
    ex.sync_weights()
    return {k[4:]: int(np.asarray(v)) for k, v in tensors.items() if k.startswith("drn/") and k != ADAM_T0}
