"""The numpy / Pillow oracle of the ensembling tool: ``ensemble_predict`` of the reference's tools/ensemble_predict_from_npy.py:17-56
restated -- ``sum(probs) / len(probs)`` or ``np.max(probs, 0)``, ``prob[:n_used].argmax(0)``, ``Image.fromarray(..).resize(.., NEAREST)`` of
the label image AND of the palette image (the reference's two resizes), ``Colorize.__call__`` (transform.py:155-165) -- with what the
reference fixes (19 classes, its palette, its output sizes) as arguments.  Everything here runs on the CPU and is exact.

``canon`` is the one liberty: IEEE 754 leaves the payload (and sign) of a NaN that an operation makes to the implementation, and numpy
hands out the host's -- inf - inf is 0xFFC00000 on x86 and 0x7FC00000 elsewhere -- so the oracle's bits at a NaN are not a definition.
The device writes 0x7FC00000 for every NaN -- under "nms" too, where numpy would hand an input NaN's own payload through: input payloads
are not preserved, and the cases here use the canonical ``np.nan`` only --; a comparison "bit for bit" is one of ``canon(oracle)`` with the device's bits."""
import numpy as np
from PIL import Image

METHODS = ("averaging", "nms")

# the 21 colours of the PASCAL-VOC development kit's colour map (labels 0..20), as published
VOC21 = ((0, 0, 0), (128, 0, 0), (0, 128, 0), (128, 128, 0), (0, 0, 128), (128, 0, 128), (0, 128, 128), (128, 128, 128), (64, 0, 0),
         (192, 0, 0), (64, 128, 0), (192, 128, 0), (64, 0, 128), (192, 0, 128), (64, 128, 128), (192, 128, 128), (0, 64, 0), (128, 64, 0),
         (0, 192, 0), (128, 192, 0), (0, 64, 128))


def voc_colour(label):
    """the rule behind VOC21 for one label < 256, bit by bit: r takes label bits 0, 3, 6 into bits 7, 6, 5; g bits 1, 4, 7; b bits 2, 5"""
    bit = lambda k: (label >> k) & 1  # noqa: E731
    return ((bit(0) << 7) | (bit(3) << 6) | (bit(6) << 5), (bit(1) << 7) | (bit(4) << 6) | (bit(7) << 5), (bit(2) << 7) | (bit(5) << 6))


def voc_palette(n):
    return np.array([voc_colour(label) for label in range(n)], dtype=np.uint8).reshape(n, 3)


def combine(probs, method):
    """:23-26, on a list of fp32 arrays of one shape"""
    with np.errstate(invalid="ignore", over="ignore"):
        if method == "averaging":
            return sum(probs) / len(probs)
        if method == "nms":
            return np.max(probs, 0)
    raise ValueError(method)


def canon(a):
    """``a`` with every NaN replaced by the canonical quiet NaN 0x7FC00000 (see the module's docstring)"""
    a = np.array(a, dtype=np.float32, copy=True)
    a.view(np.uint32)[np.isnan(a)] = 0x7FC00000
    return a


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def labels_of(prob, n_used):
    """:32-33 for [C,H,W] (or [N,C,H,W]: the class axis is the third from the end)"""
    return np.uint8(prob[..., :n_used, :, :].argmax(-3))


def resize_nearest(img_u8, out_wh):
    """:34 / :55 -- uint8 [H,W] or [H,W,3]"""
    return np.asarray(Image.fromarray(img_u8).resize((int(out_wh[0]), int(out_wh[1])), Image.NEAREST))


def colorize(label_u8, palette):
    """Colorize.__call__: black, then one mask per palette entry -- a label beyond the palette stays black"""
    out = np.zeros(label_u8.shape + (3,), dtype=np.uint8)
    for label in range(len(palette)):
        out[label_u8 == label] = palette[label]
    return out


def ensemble_predict(probs, method="averaging", n_used=None, out_wh=None, palette=None):
    """one image: ``probs`` a list of [C,H,W] fp32 -> (prob [C,H,W], label uint8 [OH,OW], vis uint8 [OH,OW,3]); the palette defaults to
    the VOC colours of n_used + 1 labels.  vis is coloured at the maps' size and resized afterwards, as the reference does (:50-55)."""
    prob = combine(probs, method)
    c, h, w = prob.shape
    n_used = c if n_used is None else n_used
    out_wh = (w, h) if out_wh is None else out_wh
    palette = voc_palette(min(n_used + 1, 256)) if palette is None else palette
    pred = labels_of(prob, n_used)
    return prob, resize_nearest(pred, out_wh), resize_nearest(colorize(pred, palette), out_wh)


def nearest_indices_pillow(in_size, out_size):
    """the source index of every output position of Pillow's NEAREST resize along one axis, read off a resize of arange(in_size)
    (in_size <= 256: the positions fit a uint8 row)"""
    row = np.arange(in_size, dtype=np.uint8)[None, :]
    return np.asarray(Image.fromarray(row).resize((out_size, 1), Image.NEAREST))[0].astype(np.int64)


def make_maps(kind, k, n, c, h, w, seed=0):
    """K maps [N,C,H,W] fp32 of the kinds the tests name"""
    rng = np.random.RandomState(seed)
    shape = (k, n, c, h, w)
    if kind == "random":
        z = rng.standard_normal(shape) * 4
    elif kind == "saturated":  # +-1e30 overflows a sum of a few to +-inf; +-inf meet as inf - inf
        z = rng.choice(np.array([1e30, -1e30, np.inf, -np.inf, 3e38, -3e38, 1.0, 0.0]), size=shape)
    elif kind == "equal":      # every pixel a C-way tie, in every map and in the combination
        z = np.broadcast_to(rng.standard_normal((k, n, 1, h, w)), shape)
    elif kind == "zeros":      # signed zeros, alone and beside tiny values of both signs
        z = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1e-45, -1e-45]), size=shape)
    elif kind == "nan":        # NaN sprinkled at 5 %
        z = rng.standard_normal(shape)
        z[rng.random_sample(shape) < 0.05] = np.nan
    else:
        raise ValueError(kind)
    return [np.ascontiguousarray(z[i], dtype=np.float32) for i in range(k)]


KINDS = ("random", "saturated", "equal", "zeros", "nan")
