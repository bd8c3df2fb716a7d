"""Host side of the joint transform (joint_transforms.py:248-255 of the reference): the random draw per sample and the parameter
tables the kernels of csrc/augment.hip read.  Pure Python + numpy: nothing here touches the GPU.

``get_joint_transform(crop_size, rotate_angle)`` of the reference is Compose([RandomHorizontallyFlip(), RandomRotate(rotate_angle),
RandomCrop(crop_size)]); ``JointTransform.draw`` consumes a ``random.Random`` in exactly that order, and ``rotate_matrix`` computes the
affine matrix exactly as ``PIL.Image.rotate`` does (same rounding, same order of additions), so the doubles are Pillow's."""
import math
import random

import numpy as np

MODE_COPY, MODE_AFFINE, MODE_ROT180, MODE_ROT90, MODE_ROT270 = 0, 1, 2, 3, 4
GEOM_COLUMNS = 10  # {mode, flip, x1, y1, fa0..fa5}
FIXED_LIMIT = 32768  # Pillow takes its 16.16 fixed-point nearest path (affine_fixed) while every source coordinate stays below this


def rotate_matrix(angle, w, h):
    """(mode, [a0..a5]) of ``Image.rotate(angle)`` on a w x h image (PIL/Image.py ``rotate``, no expand / center / translate): the
    fast paths it takes (copy, ROTATE_180, and ROTATE_90 / ROTATE_270 on a square image) or the destination -> source matrix."""
    angle = angle % 360.0
    if angle == 0:
        return MODE_COPY, [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    if angle == 180:
        return MODE_ROT180, [-1.0, 0.0, float(w), 0.0, -1.0, float(h)]
    if angle in (90, 270) and w == h:
        return (MODE_ROT90 if angle == 90 else MODE_ROT270), [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    center = (w / 2, h / 2)
    angle = -math.radians(angle)
    matrix = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]

    def transform(x, y, matrix):
        a, b, c, d, e, f = matrix
        return a * x + b * y + c, d * x + e * y + f

    matrix[2], matrix[5] = transform(-center[0] - 0, -center[1] - 0, matrix)
    matrix[2] += center[0]
    matrix[5] += center[1]
    if matrix[1] == 0 and matrix[3] == 0:
        # an angle so close to 0 or 180 that the sine rounds to nothing at 15 decimals: every source position is then a pixel centre
        # exactly (bilinear weights 0), and Pillow's nearest path (ImagingScaleAffine here) lands on the same pixels -- the copy / ROTATE_180
        return (MODE_COPY if matrix[0] > 0 else MODE_ROT180), matrix
    return MODE_AFFINE, matrix


def fixed_point(matrix):
    """the six 16.16 integers of Pillow's ``affine_fixed`` (Geometry.c): FIX(v) = floor(v * 65536 + 0.5), the offsets taken at the centre
    of pixel (0, 0)"""
    a0, a1, a2, a3, a4, a5 = matrix

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))

    return [fix(a0), fix(a1), fix(a2 + a0 * 0.5 + a1 * 0.5), fix(a3), fix(a4), fix(a5 + a3 * 0.5 + a4 * 0.5)]


def _fixed_ok(matrix, w, h):
    """Pillow's ``check_fixed`` at the four corners of the output (ImagingTransformAffine)"""
    a0, a1, a2, a3, a4, a5 = matrix
    return all(abs(x * a0 + y * a1 + a2) < 32768.0 and abs(x * a3 + y * a4 + a5) < 32768.0 for x, y in ((0, 0), (w, h), (0, h), (w, 0)))


class JointParams(object):
    """The parameter tables of one batch.  ``affine`` float64 [N,6] and ``geom`` int32 [N,10] (numpy); ``in_hw`` the loader's size,
    ``out_hw`` the size the kernel writes -- the crop, or the full image when the reference's RandomCrop resizes instead
    (``resize_to`` = (tw, th) then, else None)."""

    def __init__(self, affine, geom, in_hw, out_hw, resize_to=None):
        self.affine = np.ascontiguousarray(affine, dtype=np.float64).reshape(-1, 6)
        self.geom = np.ascontiguousarray(geom, dtype=np.int32).reshape(-1, GEOM_COLUMNS)
        assert len(self.affine) == len(self.geom)
        self.in_hw, self.out_hw, self.resize_to = tuple(in_hw), tuple(out_hw), resize_to
        self._device = {}

    def __len__(self):
        return len(self.geom)

    def tables(self, device):
        """(affine, geom) as device tensors (made once per device)"""
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = (torch.from_numpy(self.affine).to(device), torch.from_numpy(self.geom).to(device))
        return self._device[key]


def sample_params(flip, angle, x1, y1, w, h):
    """one row of each table: (affine[6], geom[10]) for a w x h image"""
    if not (0 < w < FIXED_LIMIT and 0 < h < FIXED_LIMIT):
        raise ValueError("mcdseg: the joint transform takes images below %d x %d, got %d x %d" % (FIXED_LIMIT, FIXED_LIMIT, w, h))
    mode, matrix = rotate_matrix(angle, w, h)
    if mode == MODE_AFFINE and not _fixed_ok(matrix, w, h):
        raise ValueError("mcdseg: a %d x %d image rotated by %r leaves the fixed-point range of Pillow's nearest path" % (w, h, angle))
    fixed = fixed_point(matrix) if mode == MODE_AFFINE else [0] * 6
    return matrix, [mode, int(bool(flip)), int(x1), int(y1)] + fixed


class JointTransform(object):
    """``get_joint_transform(crop_size, rotate_angle)``: owns the generator and draws, per sample and in the reference's order, the flip
    (``random() < 0.5``), the angle (``random() * 2 * deg - deg`` -- consumed also when deg == 0: the angle is then +-0.0, a copy) and
    the crop corner (``randint(0, w - tw)`` then ``randint(0, h - th)``; nothing is drawn when the image already has the crop's
    size, nor when it is smaller -- the reference's RandomCrop resizes to the crop's size then)."""

    def __init__(self, crop_size, rotate_angle=0, seed=None):
        if crop_size <= 0:
            raise ValueError("mcdseg: the joint transform needs a crop size > 0 (get_joint_transform returns None without one)")
        self.crop_size, self.rotate_angle = int(crop_size), rotate_angle
        self.rng = random.Random(seed)

    def draw_sample(self, w, h):
        """(flip, angle, x1, y1, kind) with kind in {"same", "resize", "crop"}"""
        flip = self.rng.random() < 0.5
        angle = self.rng.random() * 2 * self.rotate_angle - self.rotate_angle
        th = tw = self.crop_size
        if w == tw and h == th:
            return flip, angle, 0, 0, "same"
        if w < tw or h < th:
            return flip, angle, 0, 0, "resize"
        x1 = self.rng.randint(0, w - tw)
        y1 = self.rng.randint(0, h - th)
        return flip, angle, x1, y1, "crop"

    def draw(self, n, h, w):
        """the tables of a batch of ``n`` samples of h x w pixels"""
        affine, geom, kind = [], [], "same"
        for _ in range(n):
            flip, angle, x1, y1, kind = self.draw_sample(w, h)
            a, g = sample_params(flip, angle, x1, y1, w, h)
            affine.append(a), geom.append(g)
        if kind == "crop":
            return JointParams(affine, geom, (h, w), (self.crop_size, self.crop_size))
        return JointParams(affine, geom, (h, w), (h, w), resize_to=(self.crop_size, self.crop_size) if kind == "resize" else None)


def get_joint_transform(crop_size=-1, rotate_angle=0, seed=None):
    """the trainers' ``get_joint_transform(...) if use_crop else None`` (adapt_trainer.py:101-102): no crop size, no joint transform
    at all -- also with a rotation angle set"""
    return JointTransform(crop_size, rotate_angle, seed) if crop_size > 0 else None
