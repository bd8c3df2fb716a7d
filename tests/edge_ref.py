"""The integer oracle of the edge maps (csrc/edge.hip): OpenCV's published 8-bit algorithm for the luma plane,
``cv2.Laplacian(Y, CV_64F) + 128``, the Sobel magnitude and ``cv2.Canny`` (aperture 3, L1 gradient), restated with numpy and scipy.

A different construction from the kernels on purpose: whole-image correlations (``scipy.ndimage.correlate`` with ``mode="mirror"`` for
BORDER_REFLECT_101 and ``mode="nearest"`` for BORDER_REPLICATE), a zero-padded magnitude array for the non-maximum suppression and
``scipy.ndimage.label`` with a 3 x 3 structure for the hysteresis.  No OpenCV build was at hand: equality with one is not claimed."""
import numpy as np
from scipy import ndimage

KINDS = ("luma", "laplacian", "sobel", "canny_cls", "canny")
KX = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=np.int64)  # applied as a correlation; dy uses the transpose
LAP = np.array([[0, 1, 0], [1, -4, 1], [0, 1, 0]], dtype=np.int64)
EIGHT = np.ones((3, 3), dtype=np.int64)

# the shapes, contents and thresholds the GPU test runs (tests/test_edge_gpu.py) and whose coverage the host test asserts
SHAPES = ((1, 1), (1, 7), (5, 1), (2, 2), (3, 3), (31, 33), (33, 65), (64, 96))
CONTENTS = ("smooth", "blocks", "alphabet")
THRESHOLDS = ((100, 200), (6, 100), (200, 100), (0, 0))
BATCH = 3


def luma(rgb):
    """uint8 [...,3] in R, G, B order -> uint8 [...]: cv2.cvtColor(BGR2YUV)[:, :, 0]"""
    c = rgb.astype(np.int64)
    return ((4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14).astype(np.uint8)


def laplacian(y):
    v = ndimage.correlate(y.astype(np.int64), LAP, mode="mirror")
    return np.clip(v + 128, 0, 255).astype(np.uint8)


def gradients(y, mode):
    y = y.astype(np.int64)
    return ndimage.correlate(y, KX, mode=mode), ndimage.correlate(y, KX.T, mode=mode)


def isqrt(s):
    """exact floor(sqrt(s)) of a non-negative int64 array"""
    r = np.floor(np.sqrt(s.astype(np.float64))).astype(np.int64)
    r -= (r * r > s)
    r += ((r + 1) * (r + 1) <= s)
    return r


def sobel(y):
    dx, dy = gradients(y, "mirror")
    return np.minimum(isqrt(dx * dx + dy * dy), 255).astype(np.uint8)


def canny_branches(y, low, high):
    """(classes uint8 [H,W]: 0 / weak 1 / strong 2, branch int8 [H,W]: which rule of the non-maximum suppression decided a pixel with
    mag > low -- 0 horizontal, 1 vertical, 2 diagonal -- and -1 elsewhere)"""
    if low > high:
        low, high = high, low
    dx, dy = gradients(y, "nearest")
    mag = np.abs(dx) + np.abs(dy)
    h, w = mag.shape
    pad = np.zeros((h + 2, w + 2), dtype=np.int64)  # magnitudes outside the image are 0
    pad[1:-1, 1:-1] = mag

    def at(oy, ox):
        return pad[1 + oy:1 + oy + h, 1 + ox:1 + ox + w]

    x, yy = np.abs(dx), np.abs(dy) << 15
    t22 = x * 13573
    t67 = t22 + (x << 16)
    horizontal, vertical = yy < t22, (yy >= t22) & (yy > t67)
    keep_h = (mag > at(0, -1)) & (mag >= at(0, 1))
    keep_v = (mag > at(-1, 0)) & (mag >= at(1, 0))
    neg = (dx ^ dy) < 0
    keep_d = np.where(neg, (mag > at(-1, 1)) & (mag > at(1, -1)), (mag > at(-1, -1)) & (mag > at(1, 1)))
    keep = np.where(horizontal, keep_h, np.where(vertical, keep_v, keep_d)) & (mag > low)
    cls = np.where(keep, np.where(mag > high, 2, 1), 0).astype(np.uint8)
    branch = np.where(mag > low, np.where(horizontal, 0, np.where(vertical, 1, 2)), -1).astype(np.int8)
    return cls, branch


def canny_classes(y, low, high):
    return canny_branches(y, low, high)[0]


def components(cls):
    """(labels int [H,W] of the 8-connected components of the candidates (cls in {1, 2}), 0 elsewhere; their number; bool [n + 1]:
    component k holds a strong pixel)"""
    cand = (cls == 1) | (cls == 2)
    lab, n = ndimage.label(cand, structure=EIGHT)
    strong = np.zeros(n + 1, dtype=bool)
    strong[lab[cls == 2]] = True
    strong[0] = False
    return lab, n, strong


def hysteresis(cls):
    lab, _, strong = components(cls)
    return np.where(strong[lab], 255, 0).astype(np.uint8)


def edge_maps(rgb, low=100, high=200):
    """uint8 [H,W,3] or [N,H,W,3] -> {kind: uint8 [H,W] or [N,H,W]} for all five kinds"""
    if rgb.ndim == 4:
        per = [edge_maps(one, low, high) for one in rgb]
        return {k: np.stack([p[k] for p in per]) for k in KINDS}
    y = luma(rgb)
    cls = canny_classes(y, low, high)
    return {"luma": y, "laplacian": laplacian(y), "sobel": sobel(y), "canny_cls": cls, "canny": hysteresis(cls)}


def grey(y):
    """a grey RGB image of the luma plane ``y`` (a grey pixel maps to itself)"""
    return np.repeat(np.asarray(y, dtype=np.uint8)[..., None], 3, axis=-1)


def make_rgb(content, n, h, w, seed=0):
    """uint8 [n,h,w,3] test images.  "smooth": per channel a Gaussian-filtered (sigma 2) noise field stretched to 0..255 -- gradients of
    every direction, weak and strong ridges; "blocks": 8 x 8 on / off blocks per channel -- magnitude ties along every edge, zero
    gradients inside; "alphabet": every pixel one of four grey-ish levels -- ties and plateaus at pixel scale"""
    rng = np.random.RandomState(seed)
    if content == "smooth":
        f = ndimage.gaussian_filter(rng.rand(n, h, w, 3), sigma=(0, 2, 2, 0), mode="nearest")
        lo, hi = f.min(axis=(1, 2), keepdims=True), f.max(axis=(1, 2), keepdims=True)
        return np.round((f - lo) / np.maximum(hi - lo, 1e-12) * 255).astype(np.uint8)
    if content == "blocks":
        on = rng.randint(0, 2, size=(n, (h + 7) // 8, (w + 7) // 8, 3))
        return (np.kron(on, np.ones((1, 8, 8, 1), dtype=np.int64))[:, :h, :w] * 255).astype(np.uint8)
    if content == "alphabet":
        levels = np.array([0, 60, 130, 255], dtype=np.uint8)
        return np.repeat(levels[rng.randint(0, 4, size=(n, h, w))][..., None], 3, axis=-1)
    raise ValueError(content)


def coverage(rgb, low, high):
    """what one image holds under the oracle: components, kept components, kept components with weak pixels, weak-only components,
    edge pixels, strong pixels, and the pixels above ``low`` per branch of the non-maximum suppression"""
    y = luma(rgb)
    cls, branch = canny_branches(y, low, high)
    lab, n, strong = components(cls)
    weak_in = np.zeros(n + 1, dtype=bool)
    weak_in[lab[cls == 1]] = True
    return {"components": n, "kept": int(strong.sum()), "kept_with_weak": int((strong & weak_in).sum()),
            "weak_only": int((~strong[1:]).sum()), "edges": int((hysteresis(cls) == 255).sum()), "strong": int((cls == 2).sum()),
            "branches": tuple(int((branch == b).sum()) for b in range(3))}


def serpentine(h, w):
    """uint8 [h,w]: a one-pixel path of 1s that runs along every other row and turns at alternating ends, first pixel (0, 0); returns
    (map, (y, x) of its last pixel)"""
    m = np.zeros((h, w), dtype=np.uint8)
    last = (0, 0)
    for k, y in enumerate(range(0, h, 2)):
        m[y, :] = 1
        end = (w - 1) if k % 2 == 0 else 0  # row y is walked towards this end
        last = (y, end)
        if y + 2 < h:
            m[y + 1, end] = 1
    return m, last
