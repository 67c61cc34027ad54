"""Inception-style ImageNet input (--imagenet_preprocessing=inception), CPU side: the fp64 numpy reference of
data/imagenet.py against torch's own anti-aliased interpolate, the host draws, the contrast identity, the
loader's BOX_DESC records, the RefBackend feeder path, flag validation, the checkpoint .meta and the
evaluator's choice of pipeline, and a short CLI train + eval."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_resnet_tensorflow_amd import cli
from distributed_resnet_tensorflow_amd.ckpt.saver import Saver
from distributed_resnet_tensorflow_amd.data import imagenet as inet
from distributed_resnet_tensorflow_amd.flags import FlagsError
from distributed_resnet_tensorflow_amd.models.spec import imagenet_resnet_v2
from distributed_resnet_tensorflow_amd.ops.backend import RefBackend
from distributed_resnet_tensorflow_amd.runtime.executor import Executor
from distributed_resnet_tensorflow_amd.train.feeder import ImagenetFeeder

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# height x width -> output height x width
SHAPES = [(37, 53, 24, 24), (9, 300, 24, 24), (11, 13, 24, 24), (175, 131, 24, 24), (23, 200, 16, 16),
          (64, 48, 32, 32), (500, 375, 224, 224)]


# -- 1. the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,OH,OW", SHAPES)
def test_numpy_reference_equals_torch_antialias(H, W, OH, OW):
    rng = np.random.default_rng(H * 1000 + W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    for box in ((0, 0, H, W), (H // 5, W // 7, H - H // 5 - H // 9, W - W // 7 - W // 11)):
        by, bx, bh, bw = box
        got = inet.box_resample_np(img, by, bx, bh, bw, OH, OW)
        crop = torch.from_numpy(img[by:by + bh, bx:bx + bw].copy()).double().permute(2, 0, 1)[None]
        want = F.interpolate(crop, size=(OH, OW), mode="bilinear", align_corners=False, antialias=True)
        err = np.abs(got - want[0].permute(1, 2, 0).numpy()).max()
        assert err < 1e-9, (box, err)


def test_tap_ranges_are_the_formula_and_weights_sum_to_one():
    for L, O in ((53, 24), (300, 24), (9, 24), (24, 24), (1, 24), (131, 24), (375, 224), (1000, 224), (17, 31)):
        scale = L / O
        support = max(scale, 1.0)
        m = inet.aa_weights(L, O)
        assert np.allclose(m.sum(1), 1.0, atol=1e-14)
        for i in range(O):
            c = scale * (i + 0.5)
            lo, hi = max(0, int(c - support + 0.5)), min(L, int(c + support + 0.5))
            elo, ehi = inet.aa_taps(L, O, i)
            # the exact integer range may differ from the fp64 one only by a tap of weight ~0
            assert abs(lo - elo) <= 1 and abs(hi - ehi) <= 1
            outside = np.concatenate([m[i, :min(lo, elo)], m[i, max(hi, ehi):]])
            assert not outside.any()
            for a, b in ((lo, elo), (hi, ehi)):
                assert np.all(m[i, min(a, b):max(a, b)] < 1e-12)
    assert np.array_equal(inet.aa_weights(24, 24), np.eye(24))


def test_preprocess_flip_and_normalisation():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (40, 30, 3), dtype=np.uint8)
    d = np.zeros((), dtype=inet.BOX_DESC)
    d[()] = (0, 40, 30, 2, 3, 30, 20, 0, inet.ORDER_IDENTITY, 1.0, 1.0, 1.0, (0, 0, 0))
    a = inet.box_preprocess_np(img, d, 16, 16)
    want = (inet.box_resample_np(img, 2, 3, 30, 20, 16, 16) / 255.0 - np.array(inet.NORM_MEAN)) / np.array(inet.NORM_STD)
    assert np.allclose(a, want, atol=1e-14)
    d["flip"] = 1
    assert np.array_equal(inet.box_preprocess_np(img, d, 16, 16), a[:, ::-1])
    with pytest.raises(ValueError):
        inet.box_resample_np(img, 20, 0, 30, 20, 16, 16)


# -- 2. the draws -------------------------------------------------------------------------------------------
def test_training_boxes_lie_inside_and_keep_area_and_ratio():
    rng = np.random.default_rng(0)
    flips, fallbacks = 0, 0
    for k in range(4000):
        h, w = int(rng.integers(20, 600)), int(rng.integers(20, 600))
        smin = (0.08, 0.35, 1.0)[k % 3]
        by, bx, bh, bw, flip = inet.draw_box(h, w, True, rng, smin)
        assert 0 <= by and 0 <= bx and bh >= 1 and bw >= 1 and by + bh <= h and bx + bw <= w
        flips += flip
        # rounding of the two sides: each is within half a pixel of its real value
        lo_r, hi_r = (bw - 0.5) / (bh + 0.5), (bw + 0.5) / max(bh - 0.5, 0.25)
        assert hi_r >= 0.75 and lo_r <= 4.0 / 3.0, (h, w, bh, bw)
        central = (by, bx) == ((h - bh) // 2, (w - bw) // 2) and (bh == h or bw == w)
        fallbacks += central
        if not central:
            assert (bh - 0.5) * (bw - 0.5) <= h * w and (bh + 0.5) * (bw + 0.5) >= smin * h * w, (h, w, bh, bw, smin)
    assert 1700 < flips < 2300


def test_thin_image_always_takes_the_central_fallback():
    for seed in range(200):
        by, bx, bh, bw, _ = inet.draw_box(10, 400, True, np.random.default_rng(seed))
        assert (by, bx, bh, bw) == (0, (400 - 13) // 2, 10, 13)
        assert 0.75 <= bw / bh <= 4.0 / 3.0
    by, bx, bh, bw, _ = inet.draw_box(400, 10, True, np.random.default_rng(1))
    assert (bh, bw, bx) == (13, 10, 0) and by == (400 - 13) // 2


def test_draws_are_a_function_of_seed_rank_batch():
    def draws(seed, rank, b):
        rng = np.random.default_rng([seed, rank, 99, b])
        return [inet.draw_box(333, 500, True, rng) + inet.draw_jitter(0.4, rng) for _ in range(8)]
    assert draws(3, 1, 7) == draws(3, 1, 7)
    assert draws(3, 1, 7) != draws(3, 1, 8) and draws(3, 1, 7) != draws(3, 0, 7) and draws(4, 1, 7) != draws(3, 1, 7)
    order, ab, ac, asat = inet.draw_jitter(0.0, np.random.default_rng(0))
    assert (order, ab, ac, asat) == (inet.ORDER_IDENTITY, 1.0, 1.0, 1.0)
    rng = np.random.default_rng(2)
    seen = set()
    for _ in range(300):
        order, ab, ac, asat = inet.draw_jitter(0.4, rng)
        seen.add(inet.unpack_order(order))
        assert all(0.6 <= v <= 1.4 and v == np.float32(v) for v in (ab, ac, asat))
    assert seen == set(inet.COLOR_ORDERS)


def test_eval_box_is_the_central_square():
    for h, w in ((500, 375), (256, 256), (231, 600), (10, 400)):
        by, bx, bh, bw, flip = inet.draw_box(h, w, False, np.random.default_rng(0))
        side = int(round(min(h, w) * 224 / 256))
        assert (bh, bw, flip) == (side, side, 0) and (by, bx) == ((h - side) // 2, (w - side) // 2)


# -- 3. colour jitter ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ops", inet.COLOR_ORDERS)
def test_contrast_identity_against_step_by_step(ops):
    rng = np.random.default_rng(sum(o * 3 ** k for k, o in enumerate(ops)))
    x0 = rng.random((12, 10, 3))
    ab, ac, asat = 0.6, 1.4, 0.7
    x = x0.copy()
    for op in ops:   # step by step, the mean gray taken from the image when contrast runs
        if op == inet.OP_BRIGHTNESS:
            x = ab * x
        elif op == inet.OP_CONTRAST:
            m = inet.gray_np(x).mean()
            assert abs(m - inet.contrast_mean(inet.gray_np(x0).mean(), ops, ab)) < 1e-14
            x = ac * x + (1 - ac) * m
        else:
            x = asat * x + (1 - asat) * inet.gray_np(x)[..., None]
    got = inet.color_jitter_np(x0, inet.pack_order(ops), ab, ac, asat)
    assert np.abs(got - x).max() < 1e-14
    assert np.array_equal(inet.color_jitter_np(x0, inet.pack_order(ops), 1.0, 1.0, 1.0), x0)


# -- 4. loader and feeder -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fake_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("inet"))
    inet.write_fake_imagenet(d, shards=2, per_shard=6)
    inet.write_fake_imagenet(d, shards=1, per_shard=6, is_training=False, seed=1)
    return d


def _loader(d, train, **kw):
    return inet.ImagenetLoader(d, 4, train, seed=2, num_threads=2, num_epochs=1, preprocessing="inception", **kw)


def test_loader_emits_valid_box_descriptors(fake_dir):
    for train, jit in ((True, 0.4), (True, 0.0), (False, 0.4)):
        ld = _loader(fake_dir, train, color_jitter=jit)
        n = 0
        for b, (packed, desc, labels) in enumerate(ld):
            assert desc.dtype == inet.BOX_DESC and desc.shape == (4,)
            rng = np.random.default_rng([2, 0, 99, b])
            off = 0
            for r in desc:
                H, W = int(r["H"]), int(r["W"])
                assert int(r["offset"]) == off
                assert 0 <= r["by"] and 0 <= r["bx"] and r["by"] + r["bh"] <= H and r["bx"] + r["bw"] <= W
                box = inet.draw_box(H, W, train, rng) + inet.draw_jitter(jit if train else 0.0, rng)
                assert tuple(r[k] for k in ("by", "bx", "bh", "bw", "flip", "order")) == box[:6]
                assert (float(r["ab"]), float(r["ac"]), float(r["as"])) == box[6:]
                if not (train and jit):
                    assert (r["order"], r["ab"], r["ac"], r["as"]) == (inet.ORDER_IDENTITY, 1.0, 1.0, 1.0)
                off += H * W * 3
            assert off == packed.size
            n += 1
        ld.close()
        assert n == (3 if train else 1)
    with pytest.raises(ValueError):
        inet.ImagenetLoader(fake_dir, 4, True, preprocessing="resnet")
    with pytest.raises(ValueError):
        inet.ImagenetLoader(fake_dir, 4, True, color_jitter=0.4)
    with pytest.raises(ValueError):
        inet.ImagenetLoader(fake_dir, 4, True, preprocessing="inception", scale_min=0.0)


@pytest.mark.parametrize("train,jit", [(True, 0.4), (True, 0.0), (False, 0.0)])
def test_ref_backend_feeder_produces_the_reference(fake_dir, train, jit):
    ref_ld = _loader(fake_dir, train, color_jitter=jit)
    batches = [tuple(np.array(x, copy=True) for x in item) for item in ref_ld]
    ref_ld.close()
    ex = Executor(imagenet_resnet_v2(18), 4, RefBackend(), "cpu")
    f = ImagenetFeeder(ex, _loader(fake_dir, train, color_jitter=jit), train)
    for packed, desc, labels in batches:
        assert f.next()
        assert torch.equal(ex.labels, torch.from_numpy(labels))
        assert not ex.images[..., 3:].any()
        for i, r in enumerate(desc):
            o, H, W = int(r["offset"]), int(r["H"]), int(r["W"])
            want = inet.box_preprocess_np(packed[o:o + H * W * 3].reshape(H, W, 3), r, jitter=jit > 0)
            err = np.abs(ex.images[i, :, :, :3].double().numpy() - want).max()
            assert err < 1e-5, (i, err)   # the executor's fp32 image buffer
    assert not f.next()
    f.close()


# -- 5. flags, .meta, evaluator -----------------------------------------------------------------------------
def test_flag_validation():
    F_ = cli.entry_flags("imagenet_main", [])
    assert (F_.imagenet_preprocessing, F_.rrc_scale_min, F_.color_jitter) == ("vgg", 0.08, 0.0)
    F_ = cli.entry_flags("imagenet_main", ["--imagenet_preprocessing=inception", "--color_jitter=0.4",
                                           "--rrc_scale_min=0.35"])
    assert (F_.imagenet_preprocessing, F_.rrc_scale_min, F_.color_jitter) == ("inception", 0.35, 0.4)
    bad = [("imagenet_main", ["--imagenet_preprocessing=resnet"]),
           ("imagenet_main", ["--color_jitter=0.4"]),
           ("imagenet_main", ["--imagenet_preprocessing=inception", "--color_jitter=1.0"]),
           ("imagenet_main", ["--imagenet_preprocessing=inception", "--color_jitter=-0.1"]),
           ("imagenet_main", ["--imagenet_preprocessing=inception", "--rrc_scale_min=0"]),
           ("imagenet_main", ["--imagenet_preprocessing=inception", "--rrc_scale_min=1.5"]),
           ("imagenet_main", ["--imagenet_preprocessing=inception", "--model=lrnet"]),
           ("cifar_main", ["--imagenet_preprocessing=inception"]),
           ("cifar_main", ["--color_jitter=0.2"]),
           ("cifar_main", ["--dataset=cifar100", "--imagenet_preprocessing=inception", "--color_jitter=0.2"])]
    for entry, args in bad:
        with pytest.raises(FlagsError):
            cli.entry_flags(entry, args)


def test_meta_round_trip_and_evaluator_choice(tmp_path):
    from distributed_resnet_tensorflow_amd.train.evaluator import checkpoint_preprocessing
    from distributed_resnet_tensorflow_amd.train.trainer import _meta, model_spec_from_flags
    F_ = cli.entry_flags("imagenet_main", ["--imagenet_preprocessing=inception", "--color_jitter=0.4",
                                           "--rrc_scale_min=0.25", "--resnet_size=18"])
    meta = _meta(F_, model_spec_from_flags(F_))
    s = Saver(str(tmp_path))
    new = s.save(1, {"global_step": np.array(1)}, meta)
    old = s.save(2, {"global_step": np.array(2)}, {"optimizer": "lars"})      # (written before the keys)
    got = Saver.restore_meta(new)
    assert (got["imagenet_preprocessing"], got["rrc_scale_min"], got["color_jitter"]) == ("inception", 0.25, 0.4)
    for prefix in (old, new + "-missing"):
        got = Saver.restore_meta(prefix)
        assert (got["imagenet_preprocessing"], got["rrc_scale_min"], got["color_jitter"]) == ("vgg", 0.08, 0.0)
    # no flag: the .meta decides; an agreeing flag is fine; a contradicting one is an error that says so
    E0 = cli.entry_flags("imagenet_eval_main", [])
    assert checkpoint_preprocessing(E0, new) == "inception" and checkpoint_preprocessing(E0, old) == "vgg"
    assert checkpoint_preprocessing(cli.entry_flags("imagenet_eval_main", ["--imagenet_preprocessing=inception"]),
                                    new) == "inception"
    for flag, prefix in (("vgg", new), ("inception", old)):
        with pytest.raises(FlagsError, match=r"contradicts checkpoint .*\.meta"):
            checkpoint_preprocessing(cli.entry_flags("imagenet_eval_main", [f"--imagenet_preprocessing={flag}"]), prefix)


# -- 6. command line ----------------------------------------------------------------------------------------
def _run(args):
    env = dict(os.environ)
    env.setdefault("PYTHONPATH", REPO)
    return subprocess.run([sys.executable] + args, cwd=REPO, capture_output=True, text=True, timeout=600, env=env)


def test_cli_cpu_train_then_eval(fake_dir, tmp_path):
    ck, ev = str(tmp_path / "ck"), str(tmp_path / "ev")
    common = ["--resnet_size=18", "--batch_size=2", "--input_workers=thread", f"--log_root={ck}",
              "--imagenet_preprocessing=inception", "--color_jitter=0.4"]
    r = _run(["resnet_imagenet_main.py", f"--train_data_path={fake_dir}", "--train_steps=2", "--log_every_n_steps=1"]
             + common)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    meta = json.load(open(os.path.join(ck, "model.ckpt-2.meta")))
    assert (meta["imagenet_preprocessing"], meta["color_jitter"], meta["rrc_scale_min"]) == ("inception", 0.4, 0.08)
    r = _run(["resnet_imagenet_eval.py", "--mode=eval", "--eval_once=True", f"--eval_data_path={fake_dir}",
              f"--eval_dir={ev}", "--eval_batch_count=2"] + common)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "best precision" in r.stdout + r.stderr
    # the evaluator refuses a pipeline other than the checkpoint's
    r = _run(["resnet_imagenet_eval.py", "--mode=eval", "--eval_once=True", f"--eval_data_path={fake_dir}",
              f"--log_root={ck}", "--resnet_size=18", "--batch_size=2", "--input_workers=thread",
              "--imagenet_preprocessing=vgg"])
    assert r.returncode != 0 and "contradicts checkpoint" in r.stdout + r.stderr
