"""CPU: the joint transform (``--crop_size`` / ``--rotate_angle``: random flip, rotation and crop of image and label map together,
joint_transforms.py:248-255 of the reference).  The numpy restatement (tests/joint_ref.py) equals the vectors recorded from Pillow and
from the reference's own ``get_joint_transform`` (tests/golden/joint_augment_small.npz) and the installed Pillow; the product's host
side (``mcdseg.augment``: the draw and the parameter tables) reproduces the reference's recorded draws; the flags reach the pipeline.
No kernel is launched here."""
import argparse
import random

import numpy as np
import pytest

import joint_ref as J


@pytest.fixture(scope="module")
def fx(golden):
    return golden.npz("joint_augment_small.npz")


def _inputs(fx, shape, cs=3):
    si = J.SHAPES.index(tuple(shape))
    img = fx["img_s%d" % si]
    return (img if cs == 3 else img[..., :1]), fx["lbl_s%d" % si]


def _ref_resize():
    from oracle import ref_io
    return ref_io.resize_bilinear_u8, ref_io.resize_nearest_u8


def test_restatement_equals_the_recorded_pillow_outputs(fx):
    cases = J.direct_cases()
    assert len(cases) == 180 and {c[6] for c in cases} == {1, 3}
    for tag, shape, angle, flip, off, size, cs in cases:
        img, lbl = _inputs(fx, shape, cs)
        got = J.flip_rotate_crop(img, flip, angle, off[0], off[1], size[0], size[1])
        assert got.dtype == np.uint8 and np.array_equal(got, fx["dimg_" + tag]), tag
        if cs == 3:
            assert np.array_equal(J.flip_rotate_crop(lbl, flip, angle, off[0], off[1], size[0], size[1], nearest=True), fx["dlbl_" + tag]), tag
    for i, (angle, flip, off) in enumerate(J.BATCH_SAMPLES):
        tw, th = J.BATCH_CROP
        assert np.array_equal(J.flip_rotate_crop(fx["bimg"][i], flip, angle, off[0], off[1], tw, th), fx["bimg_out"][i])
        assert np.array_equal(J.flip_rotate_crop(fx["blbl"][i], flip, angle, off[0], off[1], tw, th, nearest=True), fx["blbl_out"][i])


def test_fixture_covers_what_it_should(fx):
    """the cases the vectors are meant to hold: every mode, both flips, both corners, fill pixels (also in label maps, where the fill
    is class 0) and label maps with the background id"""
    modes = {J.rotate_matrix(c[2], c[1][1], c[1][0])[0] for c in J.direct_cases()}
    assert modes == {J.AFFINE, J.ROT180, J.ROT90, J.ROT270}
    assert J.rotate_matrix(90.0, 23, 17)[0] == J.AFFINE and J.rotate_matrix(90.0, 24, 24)[0] == J.ROT90
    assert J.rotate_matrix(-0.0, 23, 17)[0] == J.COPY
    assert {J.draw(random.Random(k), s[1], s[0], crop, deg)[4] for _, s, crop, deg, k in J.CHAIN_CASES} == {"crop", "same", "resize"}
    assert {J.draw(random.Random(k), s[1], s[0], crop, deg)[0] for _, s, crop, deg, k in J.CHAIN_CASES} == {True, False}
    for si in range(len(J.SHAPES)):
        lbl = fx["lbl_s%d" % si]
        assert (lbl == 255).any() and lbl[lbl != 255].max() == 40 and lbl.min() == 0
    assert str(fx["pillow_version"])


def test_restatement_equals_the_installed_pillow():
    """the same grid against the Pillow that is installed (the vectors were recorded from one version of it)"""
    Image = pytest.importorskip("PIL.Image")
    for si, (h, w) in enumerate(J.SHAPES):
        img, lbl = J.seeded_inputs(77 + si, h, w)
        for angle in J.ANGLES + [-1e-4, 0.0]:
            for flip in (0, 1):
                a, b = Image.fromarray(img), Image.fromarray(lbl)
                if flip:
                    a, b = a.transpose(Image.FLIP_LEFT_RIGHT), b.transpose(Image.FLIP_LEFT_RIGHT)
                a, b = a.rotate(angle, Image.BILINEAR), b.rotate(angle, Image.NEAREST)
                assert np.array_equal(J.flip_rotate_crop(img, flip, angle, 0, 0, w, h), np.asarray(a)), (h, w, angle, flip)
                assert np.array_equal(J.flip_rotate_crop(lbl, flip, angle, 0, 0, w, h, nearest=True), np.asarray(b)), (h, w, angle, flip)
        one = Image.fromarray(img[..., 0]).rotate(7.3, Image.BILINEAR)
        assert np.array_equal(J.flip_rotate_crop(img[..., :1], 0, 7.3, 0, 0, w, h)[..., 0], np.asarray(one))


def test_seeded_draws_reproduce_the_reference_chain(fx):
    """``random.Random(k)`` in the reference's order gives the crops ``get_joint_transform`` produced after ``random.seed(k)`` -- for
    the restatement's draw AND for the product's (``mcdseg.augment.JointTransform``), including the no-draw and the resize cases"""
    from mcdseg import augment
    rb, rn = _ref_resize()
    for tag, shape, crop, degree, k in J.CHAIN_CASES:
        img, lbl = _inputs(fx, shape)
        got_img, got_lbl = J.joint_transform(img, lbl, random.Random(k), crop, degree, rb, rn)
        assert np.array_equal(got_img, fx["cimg_" + tag]) and np.array_equal(got_lbl, fx["clbl_" + tag]), tag
        h, w = shape
        drawn = augment.JointTransform(crop, degree, seed=k).draw_sample(w, h)
        assert drawn == J.draw(random.Random(k), w, h, crop, degree), tag
        # ... and the generator is left where the reference's is: the next sample's draws agree too
        jt, rng = augment.JointTransform(crop, degree, seed=k), random.Random(k)
        for _ in range(3):
            assert jt.draw_sample(w, h) == J.draw(rng, w, h, crop, degree)
        assert jt.rng.random() == rng.random()


def test_parameter_tables_are_pillows_numbers():
    from mcdseg import augment
    for h, w in J.SHAPES:
        for angle in J.ANGLES + [-1e-4, 0.0, -0.0, 360.0, 1e-14, 180.00000000000003]:
            mode, m = J.rotate_matrix(angle, w, h)
            a, g = augment.sample_params(True, angle, 3, 2, w, h)
            assert g[1:4] == [1, 3, 2]
            if mode == J.AFFINE and not (m[1] == 0 and m[3] == 0):
                assert g[0] == augment.MODE_AFFINE and a == m and g[4:] == J.fixed_matrix(m), (h, w, angle)
            elif mode == J.AFFINE:  # the sine rounded away: a copy / ROTATE_180 in effect
                assert g[0] == (augment.MODE_COPY if m[0] > 0 else augment.MODE_ROT180)
                img, lbl = J.seeded_inputs(5, h, w)
                want = img if m[0] > 0 else img[::-1, ::-1]
                assert np.array_equal(J.rotate_bilinear(img, angle), want)
            else:
                assert g[0] == mode and g[4:] == [0] * 6
    p = augment.JointTransform(12, 10, seed=3).draw(4, 24, 24)
    assert p.affine.shape == (4, 6) and p.affine.dtype == np.float64 and p.geom.shape == (4, 10) and p.geom.dtype == np.int32
    assert p.out_hw == (12, 12) and p.resize_to is None and len(p) == 4
    assert (p.geom[:, 2] <= 12).all() and (p.geom[:, 3] <= 12).all() and (p.geom[:, 2:4] >= 0).all()
    p = augment.JointTransform(32, 10, seed=3).draw(2, 24, 24)
    assert p.out_hw == (24, 24) and p.resize_to == (32, 32) and (p.geom[:, 2:4] == 0).all()
    p = augment.JointTransform(24, 0, seed=3).draw(2, 24, 24)
    assert p.out_hw == (24, 24) and p.resize_to is None and (p.geom[:, 0] == augment.MODE_COPY).all()
    with pytest.raises(ValueError):
        augment.sample_params(False, 7.3, 0, 0, 40000, 16)


def test_flags_reach_the_pipeline_only_with_a_crop_size():
    """``--crop_size <= 0``: no joint transform object at all, also with ``--rotate_angle`` set (adapt_trainer.py:101-102)"""
    import argmyparse
    import trainer_common
    from mcdseg import augment
    assert augment.get_joint_transform(-1, 10) is None and augment.get_joint_transform(0, 0) is None
    jt = augment.get_joint_transform(64, 10, seed=5)
    assert isinstance(jt, augment.JointTransform) and (jt.crop_size, jt.rotate_angle) == (64, 10)
    import torch
    from datasets import DeviceInputPipeline
    cpu = torch.device("cpu")  # (construction launches nothing)
    plain = DeviceInputPipeline(6, 41, cpu, img_shape=(32, 24), crop_size=-1, rotate_angle=10)
    assert plain.joint_transform is None and plain.img_shape == (32, 24) and plain.draw(2, 24, 32) is None
    cropped = DeviceInputPipeline(6, 41, cpu, img_shape=(32, 24), crop_size=16, rotate_angle=10, seed=9)
    assert cropped.joint_transform is not None and cropped.img_shape is None  # use_crop: no Scale
    assert cropped.draw(2, 24, 32).out_hw == (16, 16)

    class _Run(trainer_common.Run):
        def __init__(self):
            self.rank = 0

    base = ["suncg", "nyu", "--train_img_shape", "96", "64"]
    parse = lambda extra: argmyparse.get_da_mcd_training_parser().parse_args(base + extra)  # noqa: E731
    run = _Run()
    assert run.joint_transform_args(parse([])) == (-1, 0)
    assert run.joint_transform_args(parse(["--rotate_angle", "10", "--synthetic_raw"])) == (-1, 0)
    assert run.joint_transform_args(parse(["--crop_size", "64", "--rotate_angle", "10", "--synthetic_raw"])) == (64, 10)
    assert run.joint_transform_args(parse(["--crop_size", "64", "--src_file_list", "a.txt"])) == (64, 0)


def test_flags_without_raw_batches_say_that_they_have_no_effect(capsys):
    import argmyparse
    import trainer_common

    class _Run(trainer_common.Run):
        def __init__(self):
            self.rank = 0

    args = argmyparse.get_da_mcd_training_parser().parse_args(["suncg", "nyu", "--crop_size", "64", "--rotate_angle", "10", "--synthetic"])
    assert _Run().joint_transform_args(args) == (-1, 0)
    assert "have no effect" in capsys.readouterr().out
    args = argmyparse.get_da_mcd_training_parser().parse_args(["suncg", "nyu", "--crop_size", "64", "--synthetic_raw", "--input_ch", "6"])
    triple = argparse.Namespace(src_input_ch=7)
    assert _Run().joint_transform_args(args, triple) == (-1, 0)
    assert "no raw form" in capsys.readouterr().out
