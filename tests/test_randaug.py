"""RandAugment on the host (data/randaug.py): the counter-based draws, the integer reference on cases worked out
by hand, the flag refusals and the checkpoint .meta keys."""
import numpy as np
import pytest

from distributed_resnet_tensorflow_amd import cli
from distributed_resnet_tensorflow_amd.data import randaug as ra
from distributed_resnet_tensorflow_amd.flags import FlagsError

O = 7


def _image(seed=0, side=O):
    return np.random.default_rng(seed).integers(0, 256, (side, side, 3)).astype(np.int64)


def _one(q, op, magnitude=0, negate=False):
    return ra.randaug_np(q, ra.make_desc([[(op, magnitude, negate)]], q.shape[0])[0])


def test_draws_are_a_pure_function_of_their_key():
    a, b = (ra.RandAugSampler(8, 224, 3, 9, seed=5, rank=1) for _ in range(2))
    assert ra.RA_DESC.itemsize == 144
    assert a.draw(4).tobytes() == b.draw(4).tobytes() and a.draw(4).tobytes() != a.draw(5).tobytes()
    assert a.draw(4).tobytes() != ra.RandAugSampler(8, 224, 3, 9, seed=5, rank=0).draw(4).tobytes()
    # sample n's chain does not depend on the batch size; every record holds `layers` valid operations
    assert a.draw(4)[:4].tobytes() == ra.RandAugSampler(4, 224, 3, 9, seed=5, rank=1).draw(4).tobytes()
    d = np.concatenate([a.draw(i) for i in range(40)])
    assert (d["nops"] == 3).all() and set(d["op"]["id"][:, :3].reshape(-1)) == set(range(14))
    assert (d["op"]["id"][:, 3] == 0).all()
    with pytest.raises(ValueError):
        ra.RandAugSampler(8, 256, 2)


@pytest.mark.parametrize("op", sorted(ra.SIGNED | {ra.POSTERIZE, ra.SOLARIZE}), ids=lambda o: ra.OPS[o])
@pytest.mark.parametrize("negate", [False, True])
def test_magnitude_zero_is_the_identity(op, negate):
    q = _image(op)
    got = _one(q, op, 0, negate)
    if op == ra.SOLARIZE:   # t = 255 and p >= t inverts: PIL's and torchvision's Solarize at M = 0 too
        assert (got[q == 255] == 0).all()
        got, q = got[q < 255], q[q < 255]
    assert np.array_equal(got, q)


def test_constant_and_flat_images():
    q = np.broadcast_to(np.array([3, 200, 255], dtype=np.int64), (O, O, 3)).copy()
    assert np.array_equal(_one(q, ra.EQUALIZE), q)        # step == 0
    assert np.array_equal(_one(q, ra.AUTOCONTRAST), q)    # hi == lo
    # two levels: AutoContrast stretches them to 0 and 255; Equalize has step (49 - 16) // 255 = 0
    q[::2, ::2] = 100
    got = _one(q, ra.AUTOCONTRAST)
    assert set(got[..., 0].reshape(-1)) == {0, 255} and np.array_equal(got[..., 2] == 0, q[..., 2] == 100)
    assert np.array_equal(_one(q, ra.EQUALIZE), q)


def test_equalize_by_hand():
    # 32 x 32 with h = 4 per level: step = (1024 - 4) // 255 = 4, lut[i] = min(255, (2 + 4 i) // 4) = i
    q = np.repeat(np.arange(256, dtype=np.int64), 4).reshape(32, 32, 1).repeat(3, axis=2)
    assert np.array_equal(ra.equalize_np(q), q)
    # only levels 0 and 10, 512 each: step = 512 // 255 = 2, lut[0] = 1 // 2 = 0, lut[10] = min(255, 513 // 2) = 255
    q = np.where(q < 128, 0, 10)
    assert np.array_equal(ra.equalize_np(q), np.where(q == 0, 0, 255))


def test_affine_identities_and_quarter_turn():
    q = _image(3)
    for op in (ra.ROTATE, ra.TRANSLATE_X, ra.TRANSLATE_Y):
        assert np.array_equal(_one(q, op, 0), q)
    # the fixed-point centre convention: a quarter turn of an odd-sized image is np.rot90, no pixel filled
    assert np.array_equal(ra.affine_np(q, ra.affine_entries(ra.rotation(90.0))), np.rot90(q))
    assert np.array_equal(ra.affine_np(q, ra.affine_entries(ra.rotation(-90.0))), np.rot90(q, -1))
    # a forward translation by (+2, -1) pixels: out[y, x] = in[y + 1, x - 2], the rest filled with 128
    got = ra.affine_np(q, ra.affine_entries(((1.0, 0.0), (0.0, 1.0)), (2.0, -1.0)))
    assert np.array_equal(got[:-1, 2:], q[1:, :-2]) and (got[-1] == 128).all() and (got[:, :2] == 128).all()


def test_blend_sharpness_posterize_solarize_by_hand():
    q = np.full((3, 3, 3), 10, dtype=np.int64)
    q[1, 1] = 140
    # Sharpness, f = 486 (factor 1.9): s = (8 * 10 + 5 * 140 + 6) // 13 = 60,
    # (486 * 140 - 230 * 60 + 128) >> 8 = 212; the border keeps its level
    got = _one(q, ra.SHARPNESS, 30)
    assert got[1, 1, 0] == 212 and (np.delete(got.reshape(9, 3), 4, axis=0) == 10).all()
    assert (_one(q, ra.BRIGHTNESS, 30)[1, 1] == 255).all() and (_one(q, ra.BRIGHTNESS, 30, True)[1, 1] == 14).all()
    assert (_one(q, ra.POSTERIZE, 30)[1, 1] == 128).all() and (_one(q, ra.POSTERIZE, 9)[1, 1] == 140).all()
    assert (_one(q, ra.SOLARIZE, 30) == 255 - q).all()
    assert (_one(q, ra.SOLARIZE, 15)[1, 1] == 115).all() and (_one(q, ra.SOLARIZE, 15)[0, 0] == 10).all()
    assert ra.quantize_np(np.arange(256, dtype=np.float32) / np.float32(255)).tolist() == list(range(256))


@pytest.mark.parametrize("entry,args", [
    ("imagenet_main", ["--rand_augment_layers=2"]),                                          # needs inception
    ("imagenet_main", ["--imagenet_preprocessing=inception", "--rand_augment_layers=2", "--color_jitter=0.4"]),
    ("cifar_main", ["--rand_augment_layers=2"]),
    ("imagenet_main", ["--imagenet_preprocessing=inception", "--rand_augment_layers=5"]),
    ("imagenet_main", ["--imagenet_preprocessing=inception", "--rand_augment_layers=2",
                       "--rand_augment_magnitude=31"])])
def test_flag_refusals(entry, args):
    with pytest.raises(FlagsError):
        cli.entry_flags(entry, args)


def test_meta_records_the_flags_only_when_on(tmp_path):
    from distributed_resnet_tensorflow_amd.ckpt.saver import Saver
    from distributed_resnet_tensorflow_amd.train.trainer import _meta, model_spec_from_flags
    on = cli.entry_flags("imagenet_main", ["--imagenet_preprocessing=inception", "--rand_augment_layers=2",
                                           "--rand_augment_magnitude=15", "--resnet_size=18"])
    off = cli.entry_flags("imagenet_main", ["--resnet_size=18"])
    assert "rand_augment_layers" not in _meta(off, model_spec_from_flags(off))
    prefix = Saver(str(tmp_path)).save(1, {"global_step": np.array(1)}, _meta(on, model_spec_from_flags(on)))
    got = Saver.restore_meta(prefix)
    assert (got["rand_augment_layers"], got["rand_augment_magnitude"]) == (2, 15)
    assert Saver.restore_meta(prefix + "-missing")["rand_augment_layers"] == 0
