"""The joint transform of the reference's trainers (joint_transforms.py:248-255: RandomHorizontallyFlip, RandomRotate, RandomCrop on an
image and its label map together) restated in numpy: Pillow's own arithmetic (Image.rotate -> Image.transform -> Geometry.c), so that
the results are Pillow's bytes.  The kernels of csrc/augment.hip are held to it (tests/test_joint_augment_gpu.py, through the vectors
of tests/golden/joint_augment_small.npz) after tests/test_joint_augment_host.py has shown it equal to those vectors and to the
installed Pillow.  Nothing here imports the product.

Images are uint8 [H, W, C], label maps uint8 [H, W]; sizes are (w, h) where Pillow's are."""
import math
import random

import numpy as np

# the grid both the fixture's generator and the live-Pillow test walk: shapes (H, W) and angles.  The 6 x 200 strip is there for the
# small angles: at 0.37 and 359.2 degrees no pixel centre of the three small shapes moves by the half pixel that makes a fill pixel.
SHAPES = [(17, 23), (24, 24), (31, 16), (6, 200)]
ANGLES = [7.3, -10.0, 0.37, 45.0, 123.456, 359.2, 180.0, 90.0, 270.0]
CROP_WH = {(17, 23): (13, 11), (24, 24): (12, 12), (31, 16): (9, 14), (6, 200): (64, 5)}  # (tw, th) of the direct cases

COPY, AFFINE, ROT180, ROT90, ROT270 = 0, 1, 2, 3, 4


def rotate_matrix(angle, w, h):
    """(mode, matrix) of PIL.Image.rotate(angle) without expand / center / translate: its fast paths, else the destination -> source
    affine matrix with the rounding and the order of additions of Image.py"""
    angle = angle % 360.0
    if angle == 0:
        return COPY, None
    if angle == 180:
        return ROT180, None
    if angle in (90, 270) and w == h:
        return (ROT90 if angle == 90 else ROT270), None
    cx, cy = w / 2, h / 2
    rad = -math.radians(angle)
    m = [round(math.cos(rad), 15), round(math.sin(rad), 15), 0.0, round(-math.sin(rad), 15), round(math.cos(rad), 15), 0.0]
    x, y = -cx - 0, -cy - 0
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return AFFINE, m


def fixed_matrix(m):
    """affine_fixed's six 16.16 integers (Geometry.c): FIX(v) = floor(v * 65536 + 0.5)"""
    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def _exact(a, mode):
    if mode == COPY:
        return a.copy()
    if mode == ROT180:
        return a[::-1, ::-1].copy()
    return np.rot90(a, 1 if mode == ROT90 else 3).copy()  # Image.ROTATE_90 is counter-clockwise, like numpy's


def bilinear_geometry(m, w, h):
    """what ImagingGenericTransform + bilinear_filter8 derive per output pixel of a w x h image, as [h, w] arrays: inside (else the pixel
    is fill), the integer corner (x0, y0) BEFORE clipping and the weights (dx, dy)"""
    X, Y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    xin = m[0] * (X + 0.5) + m[1] * (Y + 0.5) + m[2]
    yin = m[3] * (X + 0.5) + m[4] * (Y + 0.5) + m[5]
    inside = ~((xin < 0.0) | (xin >= w) | (yin < 0.0) | (yin >= h))
    xin, yin = xin - 0.5, yin - 0.5
    x0, y0 = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    return inside, x0, y0, xin - x0, yin - y0


def rotate_bilinear(img, angle):
    """Image.fromarray(img).rotate(angle, Image.BILINEAR)"""
    h, w = img.shape[:2]
    mode, m = rotate_matrix(angle, w, h)
    if mode != AFFINE:
        return _exact(img, mode)
    inside, x0, y0, dx, dy = bilinear_geometry(m, w, h)
    c0, c1 = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    r0 = np.clip(y0, 0, h - 1)
    lower = (y0 + 1 >= 0) & (y0 + 1 < h)
    r1 = np.where(lower, y0 + 1, r0)
    src = img.astype(np.int64).reshape(h, w, -1)
    dx, dy = dx[..., None], dy[..., None]
    v1 = src[r0, c0] + (src[r0, c1] - src[r0, c0]).astype(np.float64) * dx
    v2 = src[r1, c0] + (src[r1, c1] - src[r1, c0]).astype(np.float64) * dx
    v2 = np.where(lower[..., None], v2, v1)
    v = v1 + (v2 - v1) * dy
    out = np.where(inside[..., None], v, 0.0).astype(np.uint8)  # (UINT8)v: truncation
    return out.reshape(img.shape)


def rotate_nearest(lbl, angle):
    """Image.fromarray(lbl).rotate(angle, Image.NEAREST): Pillow's 16.16 fixed-point path (h, w < 32768); the fill is 0"""
    h, w = lbl.shape
    assert h < 32768 and w < 32768
    mode, m = rotate_matrix(angle, w, h)
    if mode != AFFINE:
        return _exact(lbl, mode)
    f = fixed_matrix(m)
    X, Y = np.meshgrid(np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64))
    xi = (f[2] + Y * f[1] + X * f[0]) >> 16
    yi = (f[5] + Y * f[4] + X * f[3]) >> 16
    inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
    return np.where(inside, lbl[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)], 0).astype(np.uint8)


def flip_rotate_crop(a, flip, angle, x1, y1, tw, th, nearest=False):
    """a.transpose(FLIP_LEFT_RIGHT) if flip, .rotate(angle, NEAREST if nearest else BILINEAR), .crop((x1, y1, x1 + tw, y1 + th))"""
    a = a[:, ::-1] if flip else a
    a = rotate_nearest(np.ascontiguousarray(a), angle) if nearest else rotate_bilinear(np.ascontiguousarray(a), angle)
    return np.ascontiguousarray(a[y1:y1 + th, x1:x1 + tw])


def draw(rng, w, h, crop_size, degree):
    """the draws ``get_joint_transform(crop_size, degree)`` makes on one w x h sample, in its order, from ``rng`` (a random.Random, or the
    ``random`` module): (flip, angle, x1, y1, kind), kind = "same" (already the crop's size: nothing drawn), "resize" (smaller than the
    crop: RandomCrop resizes to it, nothing drawn) or "crop" """
    flip = rng.random() < 0.5
    angle = rng.random() * 2 * degree - degree
    th = tw = int(crop_size)
    if w == tw and h == th:
        return flip, angle, 0, 0, "same"
    if w < tw or h < th:
        return flip, angle, 0, 0, "resize"
    x1 = rng.randint(0, w - tw)
    y1 = rng.randint(0, h - th)
    return flip, angle, x1, y1, "crop"


def joint_transform(img, lbl, rng, crop_size, degree, resize_bilinear=None, resize_nearest=None):
    """get_joint_transform(crop_size, degree)(img, lbl) with the draws taken from ``rng``; the two resize functions (array, (w, h)) ->
    array serve RandomCrop's branch for samples smaller than the crop"""
    h, w = lbl.shape
    flip, angle, x1, y1, kind = draw(rng, w, h, crop_size, degree)
    if kind == "crop":
        return (flip_rotate_crop(img, flip, angle, x1, y1, crop_size, crop_size),
                flip_rotate_crop(lbl, flip, angle, x1, y1, crop_size, crop_size, nearest=True))
    img, lbl = flip_rotate_crop(img, flip, angle, 0, 0, w, h), flip_rotate_crop(lbl, flip, angle, 0, 0, w, h, nearest=True)
    if kind == "resize":
        img, lbl = resize_bilinear(img, (crop_size, crop_size)), resize_nearest(lbl, (crop_size, crop_size))
    return img, lbl


def seeded_inputs(seed, h, w, n=None):
    """seeded uint8 image(s) [.., h, w, 3] with saturated corners and label map(s) [.., h, w] holding 0..40 plus 10 % 255"""
    rng = np.random.RandomState(seed)
    lead = () if n is None else (n,)
    img = rng.randint(0, 256, size=lead + (h, w, 3)).astype(np.uint8)
    img[..., :2, :2, :] = 255
    img[..., -2:, -2:, :] = 0
    lbl = rng.randint(0, 41, size=lead + (h, w)).astype(np.uint8)
    lbl[rng.rand(*(lead + (h, w))) < 0.1] = 255
    return img, lbl


def direct_cases():
    """[(tag, (H, W), angle, flip, (x1, y1), (tw, th), cs)] of the direct Image.transpose / rotate / crop cases: every shape x angle x
    flip x {origin, far corner} with three channels, and the flipped far-corner one again with a single channel"""
    out = []
    for si, (h, w) in enumerate(SHAPES):
        tw, th = CROP_WH[(h, w)]
        for ai, angle in enumerate(ANGLES):
            for flip in (0, 1):
                for far in (0, 1):
                    off = (w - tw, h - th) if far else (0, 0)
                    out.append(("s%da%df%do%dc3" % (si, ai, flip, far), (h, w), angle, flip, off, (tw, th), 3))
            out.append(("s%da%df1o1c1" % (si, ai), (h, w), angle, 1, (w - tw, h - th), (tw, th), 1))
    return out


# (tag, shape, crop_size, degree, seed) of the cases run through the reference's own get_joint_transform after random.seed(seed)
CHAIN_CASES = ([("crop_s%d_k%d" % (si, k), SHAPES[si], 12 if si < 3 else 5, 10, k) for si in range(4) for k in range(4)] +
               [("deg0_k%d" % k, (17, 23), 12, 0, k) for k in (4, 5)] +
               [("same_k%d" % k, (24, 24), 24, 10, k) for k in (6, 7)] +        # w == tw and h == th: no crop drawn
               [("resize_k%d" % k, (31, 16), 20, 10, k) for k in (8, 9)])       # w < tw: RandomCrop resizes

# the batch of N = 3 whose samples differ in mode, flip and offset: (angle, flip, (x1, y1)) on 24 x 24 images, crop 12 x 12
BATCH_SAMPLES = [(90.0, 0, (0, 0)), (7.3, 1, (12, 12)), (180.0, 1, (5, 3))]
BATCH_SHAPE, BATCH_CROP = (24, 24), (12, 12)
# DeviceInputPipeline's chain: N = 3 RGB + HHA + label samples of 24 x 24, get_joint_transform(12, 10) after random.seed(PIPE_SEED)
PIPE_SEED, PIPE_CROP, PIPE_DEGREE = 21, 12, 10
