"""`evaluate()` checkpoint poller (reference resnet_cifar_eval.py:85-141,
resnet_imagenet_eval.py:154-210): restore the latest checkpoint in --log_root, run
--eval_batch_count batches in inference mode (BN moving statistics), log
`loss, precision, best precision`, write `Precision` / `Best Precision` summaries at the
checkpoint's global step, sleep and repeat unless --eval_once. With --top_k=K (K >= 2) the top-K
precision is accumulated beside it (`precision@K` in the log, `Precision@K` / `Best Precision@K`
summaries, `precision_top_k` in the results and in best_precision.json); "best" stays top-1.
With --eval_ema the checkpoint's `<var>/ExponentialMovingAverage` tensors (training with
--ema_decay) are evaluated in place of the variables; best_precision.json then records "ema": true.
The ImageNet input pipeline (vgg or inception) is the one the checkpoint's .meta records.

Fixes of reference quirks: no busy-spin when there is no checkpoint (Q8), best precision
persisted in eval_dir/best_precision.json across restarts (Q11), the eval set is read in order
(a --eval_batch_count covering the set is a full deterministic pass, Q10).
"""
from __future__ import annotations

import json
import logging
import os
import time

import torch

from ..ckpt.saver import Saver, latest_checkpoint, step_of
from ..flags import FlagsError
from ..parallel import cluster as cl
from ..runtime.executor import Executor
from ..runtime.state import NoEmaInCheckpoint, has_ema, import_state
from ..utils.events import EventFileWriter
from .session import make_backend
from .trainer import WEIGHT_DECAY, apply_thread_flags, make_feeder, model_spec_from_flags, setup_logging

log = logging.getLogger("drn")


def _load_best(path, key="best_precision"):
    try:
        return float(json.load(open(path))[key])
    except Exception:
        return 0.0


def checkpoint_preprocessing(FLAGS, prefix: str) -> str:
    """The ImageNet input pipeline the checkpoint was trained with (its .meta; absent = vgg), so that
    evaluation normalises the way training did. An explicit --imagenet_preprocessing that contradicts
    the .meta is an error."""
    was = Saver.restore_meta(prefix)["imagenet_preprocessing"]
    if "imagenet_preprocessing" in FLAGS and FLAGS.is_present("imagenet_preprocessing") \
            and FLAGS.imagenet_preprocessing != was:
        raise FlagsError(f"--imagenet_preprocessing={FLAGS.imagenet_preprocessing} contradicts checkpoint {prefix}, "
                         f"whose .meta records imagenet_preprocessing={was}: evaluation must normalise its input "
                         "the way training did (drop the flag; the evaluator reads it from the .meta)")
    return was


def evaluate(FLAGS, eval_batch_size: int = 100, max_evals: int = -1):
    setup_logging(0)
    apply_thread_flags(FLAGS)
    if FLAGS.mode != "eval":
        raise ValueError("this entry point only evaluates: pass --mode=eval (the reference called an "
                         "undefined train() here, SURVEY Q1)")
    FLAGS.job_name = None
    cluster = cl.resolve(FLAGS, env={})
    spec = model_spec_from_flags(FLAGS)
    be = make_backend(cluster.device, getattr(FLAGS, "precision", "bf16"))
    top_k = int(getattr(FLAGS, "top_k", 0))
    top_k = top_k if top_k >= 2 else 0  # K >= 2: precision@K beside precision ("best" stays top-1)
    ex = Executor(spec, eval_batch_size, be, cluster.device, weight_decay=WEIGHT_DECAY.get(FLAGS.dataset, 1e-4),
                  top_k=top_k)
    writer = EventFileWriter(FLAGS.eval_dir) if FLAGS.eval_dir else None
    best_path = os.path.join(FLAGS.eval_dir, "best_precision.json") if FLAGS.eval_dir else None
    best = _load_best(best_path) if best_path else 0.0
    best_k = _load_best(best_path, "best_precision_top_k") if best_path and top_k else 0.0
    eval_ema = bool(getattr(FLAGS, "eval_ema", False))
    last = None
    n_eval = 0
    results = []
    while True:
        prefix = latest_checkpoint(FLAGS.log_root)
        if prefix is None:
            log.info("No model to eval yet at %s", FLAGS.log_root)
        elif prefix == last and not FLAGS.eval_once:
            pass
        else:
            try:
                tensors = Saver.restore(prefix)
                if eval_ema and not has_ema(tensors):
                    # (not a half-written checkpoint: waiting for the next one does not help)
                    raise NoEmaInCheckpoint(f"--eval_ema: checkpoint {prefix} has no ExponentialMovingAverage "
                                            "tensors (train with --ema_decay > 0)")
                import_state(ex, tensors, use_ema=eval_ema)
            except (OSError, ValueError, KeyError) as e:  # half-written / rotated away: retry later
                log.warning("Cannot restore checkpoint %s: %s", prefix, e)
                prefix = None
            if prefix is not None:
                last = prefix
                step = ex.P.global_step or step_of(prefix)
                feeder = make_feeder(FLAGS, ex, cluster, False, batch=eval_batch_size,
                                     preprocessing=checkpoint_preprocessing(FLAGS, prefix))
                total_loss, correct, correct_k, total = 0.0, 0, 0, 0
                try:
                    for _ in range(FLAGS.eval_batch_count):
                        if not feeder.next():
                            break
                        ex.forward(train=False)
                        v = int(getattr(feeder, "valid", ex.N))  # wrapped padding of a final partial batch
                        feeder.prefetch()   # host load of the next batch while this one runs
                        total_loss += float(ex.loss_vec[:v].double().sum())
                        correct += int(ex.correct[:v].sum())
                        if top_k:
                            correct_k += int(ex.correct_k[:v].sum())
                        total += v
                finally:
                    feeder.close()
                precision = correct / max(total, 1)
                loss = total_loss / max(total, 1) + ex.wd * float(ex.P.trainable_l2())
                best = max(best, precision)
                scalars = {"Precision": precision, "Best Precision": best}
                record = {"best_precision": best, "step": step}
                if eval_ema:
                    record["ema"] = True
                result = {"step": step, "loss": loss, "precision": precision, "best_precision": best}
                line = "loss: %.3f, precision: %.3f, best precision: %.3f" % (loss, precision, best)
                if top_k:
                    precision_k = correct_k / max(total, 1)
                    best_k = max(best_k, precision_k)
                    scalars.update({f"Precision@{top_k}": precision_k, f"Best Precision@{top_k}": best_k})
                    record.update({"precision_top_k": precision_k, "best_precision_top_k": best_k, "top_k": top_k})
                    result["precision_top_k"] = precision_k
                    line += ", precision@%d: %.3f" % (top_k, precision_k)
                if writer is not None:
                    writer.add_scalars(step, scalars)
                    writer.flush()
                if best_path:
                    tmp = best_path + ".tmp"
                    with open(tmp, "w") as f:
                        json.dump(record, f)
                    os.replace(tmp, best_path)
                log.info("%s", line)
                results.append(result)
                n_eval += 1
        if FLAGS.eval_once and last is not None:
            break
        if 0 <= max_evals <= n_eval:
            break
        time.sleep(max(1, FLAGS.eval_interval_secs))
    if writer is not None:
        writer.close()
    return results
