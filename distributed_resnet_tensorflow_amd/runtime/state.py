"""Executor <-> checkpoint tensors (TF variable names and layouts).

Names follow tf.layers auto-naming + TF1 optimizer/BN conventions: trainable
`conv2d_7/kernel` (HWIO), `batch_normalization_3/{gamma,beta}`, `dense/{kernel,bias}`, slots
`<var>/Momentum`, non-trainable `batch_normalization_3/{moving_mean,moving_variance}` and
`global_step` (int64 scalar). With the weight EMA on (Executor(ema_decay > 0)) every trainable
variable also has its tf.train.ExponentialMovingAverage shadow `<var>/ExponentialMovingAverage`
(TF layout; the BN moving statistics are averages already and have none).
"""
from __future__ import annotations

import logging
from typing import Dict, Optional

import numpy as np
import torch

GLOBAL_STEP = "global_step"
EMA_SUFFIX = "/ExponentialMovingAverage"

log = logging.getLogger("drn")


class NoEmaInCheckpoint(RuntimeError):
    """The averaged weights were asked for (--eval_ema) from a checkpoint written without them."""


def has_ema(tensors) -> bool:
    return any(k.endswith(EMA_SUFFIX) for k in tensors)


def export_state(ex, extra: Optional[Dict[str, int]] = None) -> Dict[str, np.ndarray]:
    P = ex.P
    out: Dict[str, np.ndarray] = {}
    for s in P.slots:
        out[s.name] = P.to_tf(s.name).numpy()
        out[f"{s.name}/Momentum"] = P.to_tf(s.name, buf=P.momentum).numpy()
        if P.ema is not None:
            out[s.name + EMA_SUFFIX] = P.to_tf(s.name, buf=P.ema).numpy()
    for bn in P.bn_slots:
        m, v = P.moving(bn)
        out[f"{bn}/moving_mean"] = m.detach().float().cpu().numpy().copy()
        out[f"{bn}/moving_variance"] = v.detach().float().cpu().numpy().copy()
    out[GLOBAL_STEP] = np.array(P.global_step, dtype=np.int64)
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
    ex.sync_weights()
    return {k[4:]: int(np.asarray(v)) for k, v in tensors.items() if k.startswith("drn/")}
