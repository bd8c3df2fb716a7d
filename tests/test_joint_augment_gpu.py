"""GPU: the joint transform's kernels (csrc/augment.hip) against the vectors recorded from Pillow and from the reference's own
``get_joint_transform`` (tests/golden/joint_augment_small.npz) -- by equality: the kernels do Pillow's arithmetic.  Neither Pillow nor
the reference is needed here."""
import os

import numpy as np
import pytest
import torch

import joint_ref as J

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden):
    return golden.npz("joint_augment_small.npz")


def _params(samples, w, h, out_hw):
    """JointParams of [(flip, angle, x1, y1)] on w x h images"""
    from mcdseg import augment
    rows = [augment.sample_params(f, a, x1, y1, w, h) for f, a, x1, y1 in samples]
    return augment.JointParams([r[0] for r in rows], [r[1] for r in rows], (h, w), out_hw)


def _groups():
    """the direct cases of one (shape, channel count) form ONE batch: every sample of a launch is transformed differently"""
    groups = {}
    for case in J.direct_cases():
        groups.setdefault((case[1], case[6]), []).append(case)
    return groups


@pytest.mark.parametrize("shape_cs", sorted(_groups()))
def test_uint8_outputs_equal_pillow(device, fx, shape_cs):
    from mcdseg import ops
    (h, w), cs = shape_cs
    cases = _groups()[shape_cs]
    si = J.SHAPES.index((h, w))
    tw, th = J.CROP_WH[(h, w)]
    img = torch.from_numpy(fx["img_s%d" % si][..., :cs].copy()).to(device)
    lbl = torch.from_numpy(fx["lbl_s%d" % si]).to(device)
    n = len(cases)
    params = _params([(c[3], c[2], c[4][0], c[4][1]) for c in cases], w, h, (th, tw))
    got = ops.joint_augment_u8(img[None].expand(n, h, w, cs).contiguous(), params, (th, tw))
    assert got.shape == (n, th, tw, cs) and got.dtype == torch.uint8
    got = got.cpu().numpy()
    for i, c in enumerate(cases):
        assert np.array_equal(got[i], fx["dimg_" + c[0]]), (c[0], int((got[i] != fx["dimg_" + c[0]]).sum()))
    if cs == 3:
        got = ops.joint_augment_u8(lbl[None].expand(n, h, w).contiguous(), params, (th, tw), nearest=True)
        assert got.shape == (n, th, tw) and got.dtype == torch.uint8
        got = got.cpu().numpy()
        for i, c in enumerate(cases):
            assert np.array_equal(got[i], fx["dlbl_" + c[0]]), (c[0], int((got[i] != fx["dlbl_" + c[0]]).sum()))


def _batch(fx, device):
    h, w = J.BATCH_SHAPE
    params = _params([(f, a, off[0], off[1]) for a, f, off in J.BATCH_SAMPLES], w, h, J.BATCH_CROP)
    return params, torch.from_numpy(fx["bimg"]).to(device), torch.from_numpy(fx["phha"]).to(device), torch.from_numpy(fx["blbl"]).to(device)


def test_mixed_batch_indexes_the_tables_per_sample(device, fx):
    """three samples that differ in mode (ROTATE_90, affine, ROTATE_180), flip and crop corner, in one launch"""
    from mcdseg import ops
    params, rgb, _, lbl = _batch(fx, device)
    assert sorted(params.geom[:, 0]) == [1, 2, 3] and set(params.geom[:, 1]) == {0, 1}
    assert np.array_equal(ops.joint_augment_u8(rgb, params, J.BATCH_CROP).cpu().numpy(), fx["bimg_out"])
    assert np.array_equal(ops.joint_augment_u8(lbl, params, J.BATCH_CROP, nearest=True).cpu().numpy(), fx["blbl_out"])
    # the tables as plain device tensors
    tables = params.tables(device)
    assert torch.equal(ops.joint_augment_u8(rgb, tables, J.BATCH_CROP), torch.from_numpy(fx["bimg_out"]).to(device))


def test_fused_outputs_equal_the_two_step_ones(device, fx):
    """ToTensor+Normalize / ToLabel+ReLabel fused behind the gather == normalize_u8_ / relabel_u8 of the uint8 output, bit for bit; RGB and
    HHA written into one 6-channel batch at c_off 0 and 3; a fill pixel is the normalised byte 0"""
    from datasets import IMAGENET_MEAN, IMAGENET_STD
    from mcdseg import ops
    params, rgb, hha, lbl = _batch(fx, device)
    mean, std = torch.tensor(IMAGENET_MEAN, device=device), torch.tensor(IMAGENET_STD, device=device)
    oh, ow = J.BATCH_CROP
    fused = torch.full((3, 6, oh, ow), float("nan"), device=device)
    want = torch.full((3, 6, oh, ow), float("nan"), device=device)
    for part, off in ((rgb, 0), (hha, 3)):
        ops.joint_augment_normalize_u8_(fused, part, params, mean[off:off + 3], std[off:off + 3], c_off=off)
        ops.normalize_u8_(want, ops.joint_augment_u8(part, params, (oh, ow)), mean[off:off + 3], std[off:off + 3], c_off=off)
    assert torch.equal(fused, want) and bool(torch.isfinite(fused).all())
    u8 = ops.joint_augment_u8(rgb, params, (oh, ow))
    assert torch.equal(want[:, :3], ops.normalize_u8_(torch.empty_like(want[:, :3].contiguous()), torch.from_numpy(fx["bimg_out"]).to(device), mean[:3], std[:3]))
    fillpix = (u8 == 0).all(dim=3)  # (holds the rotation's fill pixels)
    assert bool(fillpix.any())
    zero = ((0.0 - mean[:3]) / std[:3]).view(1, 3, 1, 1).expand(3, 3, oh, ow)
    assert torch.equal(fused[:, :3].permute(0, 2, 3, 1)[fillpix], zero.permute(0, 2, 3, 1)[fillpix])
    # one channel, and a six-channel source in one pass (the generic-channel kernel)
    one = ops.joint_augment_normalize_u8_(torch.empty((3, 1, oh, ow), device=device), rgb[..., 1:2].contiguous(), params, mean[1:2], std[1:2])
    assert torch.equal(one[:, 0], want[:, 1])
    six = ops.joint_augment_normalize_u8_(torch.empty((3, 6, oh, ow), device=device), torch.cat([rgb, hha], dim=3), params, mean, std)
    assert torch.equal(six, want)
    # labels
    got = ops.joint_augment_relabel_u8(lbl, params, (oh, ow), 255, 40)
    assert got.dtype == torch.int64 and torch.equal(got, ops.relabel_u8(ops.joint_augment_u8(lbl, params, (oh, ow), nearest=True), 255, 40))
    assert torch.equal(got, ops.relabel_u8(torch.from_numpy(fx["blbl_out"]).to(device), 255, 40))
    assert int(got.max()) == 40 and int(got.min()) == 0


def test_arguments_are_validated(device, fx):
    from mcdseg import ops
    params, rgb, _, lbl = _batch(fx, device)
    with pytest.raises(RuntimeError):
        ops.joint_augment_u8(rgb.cpu(), params, J.BATCH_CROP)
    with pytest.raises(TypeError):
        ops.joint_augment_u8(rgb, params, J.BATCH_CROP, nearest=True)
    with pytest.raises(TypeError):
        ops.joint_augment_u8(lbl, params, J.BATCH_CROP)
    with pytest.raises(ValueError):
        ops.joint_augment_u8(rgb[:2].contiguous(), params, J.BATCH_CROP)  # three table rows, two samples
    with pytest.raises(ValueError):
        ops.joint_augment_u8(rgb, params, (0, 12))
    with pytest.raises(TypeError):
        ops.joint_augment_normalize_u8_(torch.empty((3, 3, 12, 12), device=device, dtype=torch.float64), rgb, params, torch.zeros(3), torch.ones(3))
    with pytest.raises(TypeError):
        a, g = params.tables(device)
        ops.joint_augment_u8(rgb, (a.float(), g), J.BATCH_CROP)


def test_pipeline_under_a_crop_agrees_with_the_reference_chain(device, fx):
    """DeviceInputPipeline(crop_size=...) == the reference's get_joint_transform after random.seed(k), followed by ToTensor+Normalize /
    ToLabel+ReLabel: RGB, HHA and the label map of a sample under one draw, the samples of a batch drawn one after another"""
    from datasets import DeviceInputPipeline
    from mcdseg import ops
    pipe = DeviceInputPipeline(6, 41, device, crop_size=J.PIPE_CROP, rotate_angle=J.PIPE_DEGREE, seed=J.PIPE_SEED)
    rgb, hha, lbl = torch.from_numpy(fx["bimg"]), torch.from_numpy(fx["phha"]), torch.from_numpy(fx["blbl"])
    images, labels = pipe.joint([rgb, hha], lbl)
    c = J.PIPE_CROP
    assert images.shape == (3, 6, c, c) and images.dtype == torch.float32 and labels.shape == (3, c, c) and labels.dtype == torch.int64
    want = torch.empty((3, 6, c, c), device=device)
    ops.normalize_u8_(want, torch.from_numpy(fx["prgb_out"]).to(device), pipe.mean[:3], pipe.std[:3], c_off=0)
    ops.normalize_u8_(want, torch.from_numpy(fx["phha_out"]).to(device), pipe.mean[3:], pipe.std[3:], c_off=3)
    assert torch.equal(images, want)
    assert torch.equal(labels, ops.relabel_u8(torch.from_numpy(fx["plbl_out"]).to(device), 255, 40))
    # the chain cases one by one, among them the sample that already has the crop's size and the one RandomCrop resizes
    for tag, shape, crop, degree, k in J.CHAIN_CASES:
        si = J.SHAPES.index(shape)
        pipe = DeviceInputPipeline(3, 41, device, crop_size=crop, rotate_angle=degree, seed=k)
        images, labels = pipe.joint(torch.from_numpy(fx["img_s%d" % si])[None], torch.from_numpy(fx["lbl_s%d" % si])[None])
        want_u8 = torch.from_numpy(fx["cimg_" + tag])[None].to(device)
        want = ops.normalize_u8_(torch.empty((1, 3) + tuple(want_u8.shape[1:3]), device=device), want_u8, pipe.mean, pipe.std)
        assert images.shape == want.shape and torch.equal(images, want), tag
        assert torch.equal(labels, ops.relabel_u8(torch.from_numpy(fx["clbl_" + tag])[None].to(device), 255, 40)), tag
    # without a crop size the pipeline is what it was
    plain = DeviceInputPipeline(6, 41, device, rotate_angle=10)
    both = torch.cat([rgb, hha], dim=3)
    a, b = plain.joint(both, lbl)
    assert torch.equal(a, plain.images(both)) and torch.equal(b, plain.labels(lbl)) and a.shape == (3, 6, 24, 24)


def test_adapt_trainer_with_crop_and_rotation(tmp_path, device):
    """``adapt_trainer.py --synthetic_raw --crop_size 64 --rotate_angle 10`` end to end: 96 x 64 samples are flipped, rotated and cropped
    to 64 x 64 on the device, the run ends and its checkpoint is finite"""
    import adapt_trainer
    import util
    out = str(tmp_path / "out")
    flags = ["--input_ch", "6", "-b", "2", "--train_img_shape", "96", "64", "--synthetic_raw", "--synthetic_len", "4", "--no_pretrained",
             "--no_tflog", "--epochs", "1", "--max_iter", "10", "--crop_size", "64", "--rotate_angle", "10"]
    assert adapt_trainer.main(["suncg", "nyu", "--base_outdir", out] + flags) == 0
    ck = util.load_checkpoint(os.path.join(out, "suncg-train2nyu-train_6ch", "pth", "MCD-normal-drn_d_38-1.pth.tar"))
    assert ck["args"].crop_size == 64 and ck["args"].rotate_angle == 10
    for key in ("g_state_dict", "f1_state_dict", "f2_state_dict"):
        assert all(torch.isfinite(v.float()).all() for v in ck[key].values()), key
    assert int(ck["g_state_dict"]["base.0.1.num_batches_tracked"]) == 14  # 2 iterations x 7 forwards
