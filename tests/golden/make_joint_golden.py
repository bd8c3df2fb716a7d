#!/usr/bin/env python3
"""Golden vectors for the joint transform (flip + rotate + crop of image and label map together): produced by the REAL thing -- the
installed Pillow (version recorded in the file) for the direct transpose / rotate / crop cases, and the reference's own
``get_joint_transform`` (joint_transforms.py:248-255, imported from the reference tree at generation time) after ``random.seed(k)`` for
the chain cases -- on seeded uint8 images and label maps.  The numpy restatement (tests/joint_ref.py) is asserted against every
recorded output while generating, and the affine cases are checked to reach both border branches (``check_border_branches``).
Only data is written: tests/golden/joint_augment_small.npz.

    python tests/golden/make_joint_golden.py <directory of the reference>     (or MCDSEG_REFERENCE=<directory>)
"""
import os
import random
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import joint_ref as J  # noqa: E402


def pil_direct(a, flip, angle, off, size, nearest):
    im = Image.fromarray(a if a.ndim == 2 or a.shape[2] == 3 else a[..., 0])
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    im = im.rotate(angle, Image.NEAREST if nearest else Image.BILINEAR)
    im = im.crop((off[0], off[1], off[0] + size[0], off[1] + size[1]))
    return np.asarray(im).reshape((size[1], size[0]) + (() if a.ndim == 2 else (a.shape[2],)))


def resize_bilinear(a, wh):
    return np.asarray(Image.fromarray(a).resize(wh, Image.BILINEAR))


def resize_nearest(a, wh):
    return np.asarray(Image.fromarray(a).resize(wh, Image.NEAREST))


def check_border_branches():
    """neither border branch goes untested: every affine angle has, on some shape, pixels whose taps are clipped at a border and, on
    some shape, fill pixels; every affine (shape, angle) has one of the two, and fill pixels from 7 degrees on.  (Not every case can have
    both: below a degree no pixel centre of the three small shapes moves by the half pixel that makes a fill pixel -- the 6 x 200 strip
    is there for those -- and at 45 degrees on 24 x 24 the source positions, 12 + k / sqrt(2), step over the half-pixel border strip.)"""
    seen = {}
    for h, w in J.SHAPES:
        for angle in J.ANGLES:
            mode, m = J.rotate_matrix(angle, w, h)
            if mode != J.AFFINE:
                continue
            inside, x0, y0, _, _ = J.bilinear_geometry(m, w, h)
            clipped = bool((inside & ((x0 < 0) | (x0 + 1 > w - 1) | (y0 < 0) | (y0 + 1 > h - 1))).any())
            fill = bool((~inside).any())
            assert clipped or fill, ("neither a clipped tap nor a fill pixel", (h, w), angle)
            if 7.0 <= angle % 360.0 <= 353.0:
                assert fill, ("no fill pixel", (h, w), angle)
            was = seen.get(angle, (False, False))
            seen[angle] = (was[0] or clipped, was[1] or fill)
    assert len(seen) >= 8 and all(c and f for c, f in seen.values()), seen


def main():
    ref_dir = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MCDSEG_REFERENCE")
    if not ref_dir or not os.path.exists(os.path.join(ref_dir, "joint_transforms.py")):
        raise SystemExit("give the directory of the reference (its joint_transforms.py is imported)")
    sys.path.insert(0, ref_dir)
    from joint_transforms import get_joint_transform
    check_border_branches()
    out = {"pillow_version": np.array(PIL.__version__)}
    inputs = {}
    for si, (h, w) in enumerate(J.SHAPES):
        img, lbl = J.seeded_inputs(1000 + si, h, w)
        inputs[(h, w)] = (img, lbl)
        out["img_s%d" % si], out["lbl_s%d" % si] = img, lbl

    # 1. direct Image.transpose / rotate / crop
    for tag, shape, angle, flip, off, size, cs in J.direct_cases():
        img, lbl = inputs[shape]
        img = img if cs == 3 else img[..., :1]
        ref_img, ref_lbl = pil_direct(img, flip, angle, off, size, False), pil_direct(lbl, flip, angle, off, size, True)
        got_img = J.flip_rotate_crop(img, flip, angle, off[0], off[1], size[0], size[1])
        got_lbl = J.flip_rotate_crop(lbl, flip, angle, off[0], off[1], size[0], size[1], nearest=True)
        assert np.array_equal(got_img, ref_img), (tag, "bilinear", int((got_img != ref_img).sum()))
        assert np.array_equal(got_lbl, ref_lbl), (tag, "nearest", int((got_lbl != ref_lbl).sum()))
        out["dimg_" + tag] = ref_img
        if cs == 3:
            out["dlbl_" + tag] = ref_lbl
    print("  %d direct cases ok" % len(J.direct_cases()))

    # 2. the reference's get_joint_transform after random.seed(k)
    kinds = set()
    for tag, shape, crop, degree, k in J.CHAIN_CASES:
        img, lbl = inputs[shape]
        random.seed(k)
        ref_img, ref_lbl = get_joint_transform(crop_size=crop, rotate_angle=degree)(Image.fromarray(img), Image.fromarray(lbl))
        ref_img, ref_lbl = np.asarray(ref_img), np.asarray(ref_lbl)
        kinds.add(J.draw(random.Random(k), shape[1], shape[0], crop, degree)[4])
        got_img, got_lbl = J.joint_transform(img, lbl, random.Random(k), crop, degree, resize_bilinear, resize_nearest)
        assert np.array_equal(got_img, ref_img) and np.array_equal(got_lbl, ref_lbl), tag
        out["cimg_" + tag], out["clbl_" + tag] = ref_img, ref_lbl
    assert kinds == {"crop", "same", "resize"}, kinds
    print("  %d chain cases ok" % len(J.CHAIN_CASES))

    # 3. a batch of three samples that differ in mode, flip and offset
    h, w = J.BATCH_SHAPE
    bimg, blbl = J.seeded_inputs(2000, h, w, n=3)
    out["bimg"], out["blbl"] = bimg, blbl
    out["bimg_out"] = np.stack([pil_direct(bimg[i], f, a, off, J.BATCH_CROP, False) for i, (a, f, off) in enumerate(J.BATCH_SAMPLES)])
    out["blbl_out"] = np.stack([pil_direct(blbl[i], f, a, off, J.BATCH_CROP, True) for i, (a, f, off) in enumerate(J.BATCH_SAMPLES)])
    assert len({J.rotate_matrix(a, w, h)[0] for a, _, _ in J.BATCH_SAMPLES}) == 3

    # 4. DeviceInputPipeline's chain: RGB, HHA and label map of a sample under ONE draw, the samples of a batch drawn one after another
    hha, _ = J.seeded_inputs(3000, h, w, n=3)
    out["phha"] = hha
    random.seed(J.PIPE_SEED)
    jt = get_joint_transform(crop_size=J.PIPE_CROP, rotate_angle=J.PIPE_DEGREE)
    rgb_o, hha_o, lbl_o = [], [], []
    for i in range(3):
        state = random.getstate()
        a, l = jt(Image.fromarray(bimg[i]), Image.fromarray(blbl[i]))
        random.setstate(state)  # the HHA image of the sample: the same draw
        b, l2 = jt(Image.fromarray(hha[i]), Image.fromarray(blbl[i]))
        assert np.array_equal(np.asarray(l), np.asarray(l2))
        rgb_o.append(np.asarray(a)), hha_o.append(np.asarray(b)), lbl_o.append(np.asarray(l))
    out["prgb_out"], out["phha_out"], out["plbl_out"] = np.stack(rgb_o), np.stack(hha_o), np.stack(lbl_o)
    rng = random.Random(J.PIPE_SEED)
    for i in range(3):
        state = rng.getstate()
        a, l = J.joint_transform(bimg[i], blbl[i], rng, J.PIPE_CROP, J.PIPE_DEGREE)
        rng.setstate(state)
        b, _ = J.joint_transform(hha[i], blbl[i], rng, J.PIPE_CROP, J.PIPE_DEGREE)
        assert np.array_equal(a, rgb_o[i]) and np.array_equal(b, hha_o[i]) and np.array_equal(l, lbl_o[i]), i

    path = os.path.join(HERE, "joint_augment_small.npz")
    np.savez_compressed(path, **out)
    print("joint_augment_small.npz written (Pillow %s, %d arrays, %d bytes)" % (PIL.__version__, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
