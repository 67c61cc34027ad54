"""ResNet-50 with ResNet-D shortcuts on the gfx950 kernels, checked exactly the way tests/test_resnext_gpu.py
checks ResNeXt (its procedures and tolerances, run on this spec): every block teacher-forced against the
fp32 reference executor, and a native-plan replay of a training step against the eager step, bit for bit."""
import pytest
import torch

import test_resnext_gpu as rx
from distributed_resnet_tensorflow_amd.models.spec import imagenet_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import HipBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]


def _spec():   # 64 px: the pooled projections run at 16 -> 8, 8 -> 4 and 4 -> 2
    return imagenet_resnet_v2(50, num_classes=7, image_size=64, avg_down=True)


def test_every_block_teacher_forced(monkeypatch):
    """Output, input gradient, every weight gradient (the projection's from the stash) and BatchNorm gradient
    of each block; the pooled projections read raw tensors here (default BatchNorm policy)."""
    h = Executor(_spec(), 2, HipBackend(), "cuda")
    assert [bp.ap is not None and bp.bn[0].act is None for bp in h.blocks if bp.proj] == [False, True, True, True]
    monkeypatch.setattr(rx, "_spec", _spec)
    rx.test_every_block_teacher_forced()


def test_plan_replay_is_bitwise_the_eager_step(monkeypatch):
    monkeypatch.setattr(rx, "_spec", _spec)
    rx.test_replayed_step_is_bitwise_the_eager_step(monkeypatch, "plan")
