"""Pure-numpy restatement of the boundary refinement contract ("Refinement by predicted boundaries"), written from the
contract, for the tests: flood fill under the stated adjacency, the frame rule, canonical ids, strict thresholds and the
first-occurrence tie-break.  Also the patterns the host and the GPU tests share.  Slow and obvious on purpose."""
import numpy as np


def mask_of(boundary, thre):
    return np.asarray(boundary) > thre  # strictly


def regions(boundary, thre):
    """int32 [H,W]: -1 for the frame object, else the smallest row-major index of the pixel's component.  p ~ q iff m[p] == m[q] and
    (4-adjacent, or diagonal neighbours with m == 1)."""
    m = mask_of(boundary, thre)
    h, w = m.shape
    out = np.full((h, w), -2, dtype=np.int64)
    four = ((-1, 0), (1, 0), (0, -1), (0, 1))
    eight = four + ((-1, -1), (-1, 1), (1, -1), (1, 1))
    for y0 in range(h):
        for x0 in range(w):
            if out[y0, x0] != -2:
                continue
            # scanning in row-major order, the seed is the smallest index of its component
            rid, bit = y0 * w + x0, m[y0, x0]
            steps = eight if bit else four
            stack, members, frame = [(y0, x0)], [], False
            out[y0, x0] = rid
            while stack:
                y, x = stack.pop()
                members.append((y, x))
                if bit and (y == 0 or y == h - 1 or x == 0 or x == w - 1):
                    frame = True
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and out[yy, xx] == -2 and m[yy, xx] == bit:
                        out[yy, xx] = rid
                        stack.append((yy, xx))
            if frame:
                for y, x in members:
                    out[y, x] = -1
    return out.astype(np.int32)


def refine(seg, region_map, min_thre, max_thre):
    """uint8 [H,W]: regions with id >= 0 and min_thre < pixels < max_thre take their most common value of ``seg``; ties go to the value
    whose first pixel in row-major order comes earliest"""
    seg = np.asarray(seg, dtype=np.uint8)
    flat_seg, flat_reg = seg.reshape(-1), np.asarray(region_map).reshape(-1)
    out = flat_seg.copy()
    order = np.argsort(flat_reg, kind="stable")  # pixels grouped by id, in row-major order inside a group
    cuts = np.flatnonzero(np.diff(flat_reg[order])) + 1
    for idx in np.split(order, cuts):
        if flat_reg[idx[0]] < 0 or not (min_thre < idx.size < max_thre):
            continue
        vals = flat_seg[idx]
        best, best_count, best_first = None, -1, None
        for v in np.unique(vals):
            where = np.flatnonzero(vals == v)
            count, first = where.size, where[0]
            if count > best_count or (count == best_count and first < best_first):
                best, best_count, best_first = v, count, first
        out[idx] = best
    return out.reshape(seg.shape)


def refine_by_boundary(seg, boundary, thre=50, min_thre=500, max_thre=79333):
    return refine(seg, regions(boundary, thre), min_thre, max_thre)


# ---- patterns (uint8 boundary images; the mask is ``> THRE``) ----------------------------------------------------------------------

THRE = 50


def checkerboard(h, w, inset=0):
    b = np.zeros((h, w), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    on = (yy + xx) % 2 == 0
    if inset:
        on &= (yy >= inset) & (yy < h - inset) & (xx >= inset) & (xx < w - inset)
    b[on] = 255
    return b


def spiral(h, w):
    """one-pixel corridors of zeros between one-pixel walls: rings of wall at every even distance from the border, each ring cut by a
    one-pixel door, doors alternating between the ring's top-left and bottom-right, so the zeros form ONE winding corridor"""
    b = np.zeros((h, w), np.uint8)
    k, ring = 0, 0
    while 2 * k < min(h, w):
        y0, y1, x0, x1 = k, h - 1 - k, k, w - 1 - k
        b[y0, x0:x1 + 1] = 255
        b[y1, x0:x1 + 1] = 255
        b[y0:y1 + 1, x0] = 255
        b[y0:y1 + 1, x1] = 255
        if ring > 0 and y1 - y0 >= 2 and x1 - x0 >= 2:
            if ring % 2:
                b[y0, x0 + 1] = 0  # a door next to the top-left corner
            else:
                b[y1, x1 - 1] = 0  # a door next to the bottom-right corner
        k += 2
        ring += 1
    return b


def comb(h, w):
    """a serpentine: horizontal walls every second row, open alternately at the right and at the left end, inside a border of zeros"""
    b = np.zeros((h, w), np.uint8)
    for i, y in enumerate(range(2, h - 2, 2)):
        if i % 2:
            b[y, 3:w - 1] = 255
        else:
            b[y, 1:w - 3] = 255
    return b


def diagonal(h, w, short=0):
    """the mask line from the top-left corner to the bottom-right one of the image inset by ``short`` pixels: one step along the longer
    side per pixel, so it is 8-connected and no 4-connected path of zeros crosses it"""
    b = np.zeros((h, w), np.uint8)
    hh, ww = h - 2 * short, w - 2 * short
    if hh <= 0 or ww <= 0:
        return b
    n = max(hh, ww)
    for i in range(n):
        b[short + i * (hh - 1) // max(n - 1, 1), short + i * (ww - 1) // max(n - 1, 1)] = 255
    return b


def bernoulli(h, w, density, seed):
    rng = np.random.RandomState(seed)
    return np.where(rng.rand(h, w) < density, 255, 0).astype(np.uint8)


def threshold_pair(h, w):
    """columns alternately exactly THRE (outside the mask) and THRE + 1 (inside)"""
    b = np.full((h, w), THRE, np.uint8)
    b[:, 1::2] = THRE + 1
    return b


def seeded_seg(h, w, seed, n_values=5, block=3):
    """a blocky label image, so that regions hold clear majorities as well as ties"""
    rng = np.random.RandomState(seed)
    small = rng.randint(0, n_values, size=((h + block - 1) // block, (w + block - 1) // block))
    seg = np.kron(small, np.ones((block, block), dtype=np.int64))[:h, :w]
    seg[rng.rand(h, w) < 0.1] = 255
    return seg.astype(np.uint8)


SHAPES = ((1, 1), (1, 97), (97, 1), (33, 65), (64, 64), (130, 200))


def patterns(h, w):
    """{name: boundary image} of every pattern the GPU test runs at a shape"""
    out = {"zeros": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8), "threshold": threshold_pair(h, w),
           "checker": checkerboard(h, w), "checker_inset": checkerboard(h, w, 1), "spiral": spiral(h, w), "comb": comb(h, w),
           "diagonal": diagonal(h, w), "diagonal_short": diagonal(h, w, 1)}
    for d in (0.3, 0.5, 0.6):
        out["bernoulli_%d" % int(d * 10)] = bernoulli(h, w, d, seed=int(d * 10) + h * 1000 + w)
    return out


GOLDEN_SHAPE = (33, 65)
GOLDEN_THRESHOLDS = (4, 600)  # (min_thre, max_thre) of the committed cases


def golden_cases():
    """[(name, boundary, seg, thre, min_thre, max_thre)] of tests/golden/refine_small.npz: every pattern at 33 x 65, and the spiral at
    130 x 200 (structured, so it compresses to little)"""
    h, w = GOLDEN_SHAPE
    cases = [(name, b, seeded_seg(h, w, seed=100 + i), THRE) + GOLDEN_THRESHOLDS for i, (name, b) in enumerate(sorted(patterns(h, w).items()))]
    cases.append(("spiral_130x200", spiral(130, 200), seeded_seg(130, 200, seed=7, block=8), THRE, 4, 20000))
    return cases
