"""The fp64 numpy/scipy statement of the colorization depth inpainting: the yardstick of ``ops.fill_depth``
(csrc/fill.hip).  Nothing is claimed about byte equality with the NYU toolbox's ``fill_depth_colorization``; this file IS the definition.

Per image: ``rgb`` uint8 [H,W,3], ``Z`` fp32 [H,W] centimetres.  A pixel is known iff Z is finite, > 0 and (with ``max_valid_cm``)
< max_valid_cm.  ``system`` states steps 1-4 (luma, scale, weights, the sparse system M x = b), ``solve_direct`` is the sparse LU,
``solve_iter`` the BiCGSTAB iteration of step 5 with its true-residual stopping rule, ``minv_norm`` = ||M^-1 1||_inf, the constant of the
error bound  ||x - x*||_inf <= minv_norm (||b - M x||_inf + ||b - M x*||_inf)  (M is a non-singular M-matrix, so M^-1 >= 0).

The seeded case builders at the end are the scenes of tests/test_fill_depth_gpu.py; tests/test_fill_ref_host.py holds each of them to
the honesty conditions on the CPU."""
import functools
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import hha_ref

RUNNING, CONVERGED, EMPTY, NOT_CONVERGED, BREAKDOWN = 0, 1, 2, 3, 4
DIRS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))  # (dy, dx), row-major: the order of every sum
SIGMA_FLOOR = 2e-6
LN100 = math.log(100.0)


def known_mask(Z, max_valid_cm=None):
    Z = np.asarray(Z, np.float32)
    k = np.isfinite(Z) & (Z > 0)
    if max_valid_cm is not None:
        k &= Z.astype(np.float64) < float(max_valid_cm)
    return k


def luma(rgb):
    c = np.asarray(rgb).astype(np.float64)
    return ((0.299 * c[..., 0] + 0.587 * c[..., 1]) + 0.114 * c[..., 2]) / 255.0


def _shifted(a, dy, dx, fill):
    """a[v + dy, u + dx] where that lies inside the image, else ``fill``"""
    h, w = a.shape
    out = np.full((h, w), fill, a.dtype)
    v0, v1, u0, u1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if v1 > v0 and u1 > u0:
        out[v0:v1, u0:u1] = a[v0 + dy:v1 + dy, u0 + dx:u1 + dx]
    return out


def weights(rgb):
    """(w fp64 [8,H,W], inside bool [8,H,W]): the normalised weight of each 3 x 3 neighbour in ``DIRS`` order, 0 outside the image"""
    g = luma(rgb)
    h, w = g.shape
    if h * w < 2:
        raise ValueError("fill_depth needs H*W >= 2")
    inside = np.stack([_shifted(np.ones((h, w), bool), dy, dx, False) for dy, dx in DIRS])
    gq = np.stack([_shifted(g, dy, dx, 0.0) for dy, dx in DIRS])
    total, count = g.copy(), np.ones((h, w))
    for k in range(8):
        total = np.where(inside[k], total + gq[k], total)
        count = count + inside[k]
    mu = total / count
    var = (g - mu) * (g - mu)
    nearest = np.full((h, w), np.inf)
    d2 = np.zeros((8, h, w))
    for k in range(8):
        var = np.where(inside[k], var + (gq[k] - mu) * (gq[k] - mu), var)
        d = gq[k] - g
        d2[k] = d * d
        nearest = np.where(inside[k], np.minimum(nearest, d2[k]), nearest)
    var = var / count
    sigma = np.maximum(np.maximum(0.6 * var, nearest / LN100), SIGMA_FLOOR)
    wk = np.where(inside, np.exp(-d2 / sigma), 0.0)
    wsum = np.zeros((h, w))
    for k in range(8):
        wsum = np.where(inside[k], wsum + wk[k], wsum)
    return np.where(inside, wk / wsum, 0.0), inside


def system(rgb, Z, alpha=1.0, max_valid_cm=None):
    """(M scipy CSR [P,P], b [P], D [P], zmax): steps 1-4.  zmax is 0.0 for an image without a known pixel (then b = 0)."""
    Z = np.asarray(Z, np.float32)
    h, w = Z.shape
    known = known_mask(Z, max_valid_cm)
    zmax = float(Z[known].max()) if known.any() else 0.0
    z = np.where(known, Z.astype(np.float64) / (zmax if zmax > 0 else 1.0), 0.0)
    wk, inside = weights(rgb)
    alpha = float(alpha)
    D = np.where(known, 1.0 + alpha, 1.0).reshape(-1)
    b = np.where(known, alpha * z, 0.0).reshape(-1)
    idx = np.arange(h * w).reshape(h, w)
    rows, cols, vals = [idx.reshape(-1)], [idx.reshape(-1)], [D]
    for k, (dy, dx) in enumerate(DIRS):
        m = inside[k]
        rows.append(idx[m])
        cols.append(idx[m] + dy * w + dx)
        vals.append(-wk[k][m])
    M = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(h * w, h * w))
    M.sort_indices()
    return M, b, D, zmax


def solve_direct(M, b):
    return spla.spsolve(M.tocsc(), b)


def minv_norm(M):
    return float(np.max(spla.spsolve(M.tocsc(), np.ones(M.shape[0]))))


def _bad(v):
    return v == 0.0 or not np.isfinite(v)


def solve_iter(M, b, D, rtol=1e-10, max_iter=4000, check_every=8):
    """step 5 -> (x, status, iterations, ||b - M x||_2 / ||b||_2 of the last check)"""
    bn = np.sqrt(np.dot(b, b))
    x = b / D
    r = b - M @ x
    rhat = r.copy()
    rho = a = omega = 1.0
    v = np.zeros_like(b)
    p = np.zeros_like(b)

    def check():
        t = b - M @ x
        rn = np.sqrt(np.dot(t, t))
        return rn <= rtol * bn, rn / bn

    done, res = check()
    if done:
        return x, CONVERGED, 0, res
    it = 0
    with np.errstate(all="ignore"):
        while it < max_iter:
            rho_new = np.dot(rhat, r)
            if _bad(rho_new):
                return x, BREAKDOWN, it, res
            beta = (rho_new / rho) * (a / omega)
            p = r + beta * (p - omega * v)
            v = M @ (p / D)
            rv = np.dot(rhat, v)
            if _bad(rv):
                return x, BREAKDOWN, it, res
            a = rho_new / rv
            s = r - a * v
            t = M @ (s / D)
            tt = np.dot(t, t)
            if _bad(tt):
                return x, BREAKDOWN, it, res
            omega = np.dot(t, s) / tt
            x = x + (a * (p / D) + omega * (s / D))
            r = s - omega * t
            rho = rho_new
            it += 1
            if it % check_every == 0:
                done, res = check()
                if done:
                    return x, CONVERGED, it, res
    return x, NOT_CONVERGED, it, res


def fill(rgb, Z, alpha=1.0, rtol=1e-10, max_iter=4000, check_every=8, max_valid_cm=None, keep_known=False):
    """the whole procedure for one image -> dict(filled fp32, x, zmax, status, iterations, residual)"""
    Z = np.asarray(Z, np.float32)
    M, b, D, zmax = system(rgb, Z, alpha, max_valid_cm)
    if zmax == 0.0:
        return dict(filled=np.zeros(Z.shape, np.float32), x=np.zeros(Z.shape), zmax=0.0, status=EMPTY, iterations=0, residual=0.0)
    x, status, it, res = solve_iter(M, b, D, rtol, max_iter, check_every)
    filled = (x * zmax).astype(np.float32).reshape(Z.shape)
    if keep_known:
        k = known_mask(Z, max_valid_cm)
        filled[k] = Z[k]
    return dict(filled=filled, x=x.reshape(Z.shape), zmax=zmax, status=status, iterations=it, residual=res)


# ------------------------------------------------------------------------------------------------ the scenes
def _room(h, w, seed, **kw):
    """(rgb uint8 [H,W,3], depth fp32 [H,W] cm, complete): a box room (tests/hha_ref.room) painted by plane, shaded with depth, with
    pixel noise"""
    depth, truth = hha_ref.room(h, w, noise=0.2, seed=seed, **kw)
    rs = np.random.RandomState(1000 + seed)
    base = np.array([[150, 120, 90], [230, 230, 220], [120, 150, 180], [200, 170, 120], [90, 140, 110]], np.float64)
    shade = 1.0 - 0.45 * (depth - depth.min()) / max(depth.max() - depth.min(), 1e-9)
    rgb = base[truth["plane"]] * shade[..., None] + rs.normal(0, 4.0, (h, w, 3))
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8), depth.astype(np.float32)


def _band(depth, cols):
    depth[:, :cols] = 0  # the sensor's blind band at one border


def _discs(depth, rs, count, rmax):
    h, w = depth.shape
    vv, uu = np.mgrid[:h, :w]
    for _ in range(count):
        cv, cu, r = rs.randint(0, h), rs.randint(0, w), rs.randint(max(2, rmax // 3), rmax + 1)
        depth[(vv - cv) ** 2 + (uu - cu) ** 2 <= r * r] = 0


def _speckle(depth, rs, share):
    depth[rs.rand(*depth.shape) < share] = 0


def _clipped_8x12():
    rgb, d = _room(8, 12, 1, pitch=35.0)
    _speckle(d, np.random.RandomState(11), 0.40)
    return rgb[None], d[None]


def _odd_37x53():
    rgb, d = _room(37, 53, 3)
    rs = np.random.RandomState(12)
    _band(d, 4)
    _speckle(d, rs, 0.02)
    return rgb[None], d[None]


def _two_48x64():
    # image 0: a few specks; image 1: a farther room (another zmax) with a wide band and large holes: many more iterations
    rgb0, d0 = _room(48, 64, 0)
    _speckle(d0, np.random.RandomState(13), 0.02)
    rgb1, d1 = _room(48, 64, 5, cam_height=150.0, pitch=20.0, roll=-8.0, yaw=-30.0, ceiling=300.0, front=420.0, right=150.0)
    rs = np.random.RandomState(14)
    _band(d1, 8)
    _discs(d1, rs, 4, 9)
    _speckle(d1, rs, 0.02)
    return np.stack([rgb0, rgb1]), np.stack([d0, d1])


def _holes_96x128():
    rgb, d = _room(96, 128, 1)
    rs = np.random.RandomState(15)
    _band(d, 6)
    _discs(d, rs, 6, 12)
    _speckle(d, rs, 0.02)
    return rgb[None], d[None]


def _one_known_16x16():
    rgb, d = _room(16, 16, 2)
    z = np.zeros_like(d)
    z[5, 9] = d[5, 9]
    return rgb[None], z[None]


def _flat_gray_16x16():
    _, d = _room(16, 16, 4)
    rs = np.random.RandomState(16)
    _discs(d, rs, 2, 3)
    _speckle(d, rs, 0.05)
    return np.full((1, 16, 16, 3), 128, np.uint8), d[None]


def _island_32x32():
    _, d = _room(32, 32, 6)
    rgb = np.full((32, 32, 3), 20, np.uint8)
    rgb[8:24, 8:24] = 240
    d[12:20, 12:20] = 0  # missing inside the bright square: its value comes from the square's own rim, almost nothing crosses the edge
    return rgb[None], d[None]


def _row_1x40():
    rgb, d = _room(1, 40, 7)
    d[0, 10:17] = 0
    d[0, 30] = 0
    d[0, 39] = 0
    return rgb[None], d[None]


def _missing_beside_valid():
    rgb, d = _odd_37x53()
    return np.concatenate([rgb, rgb]), np.concatenate([np.zeros_like(d), d])


CASES = {
    "clipped_8x12": _clipped_8x12, "odd_37x53": _odd_37x53, "two_48x64": _two_48x64, "holes_96x128": _holes_96x128,
    "one_known_16x16": _one_known_16x16, "flat_gray_16x16": _flat_gray_16x16, "island_32x32": _island_32x32, "row_1x40": _row_1x40,
    "missing_beside_valid": _missing_beside_valid,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(rgb uint8 [N,H,W,3], depth fp32 [N,H,W] centimetres, 0 = missing), read-only"""
    rgb, depth = CASES[name]()
    rgb, depth = np.ascontiguousarray(rgb), np.ascontiguousarray(depth, dtype=np.float32)
    rgb.setflags(write=False)
    depth.setflags(write=False)
    return rgb, depth


@functools.lru_cache(maxsize=None)
def truth(name, k, alpha=1.0, max_valid_cm=None):
    """image k of a case: dict(M, b, D, zmax, weights, x_star, minv, it: solve_iter's (x, status, iterations, residual)); x_star,
    minv and it are None for an image without a known pixel.  Computed once, never changed."""
    rgb, depth = case(name)
    M, b, D, zmax = system(rgb[k], depth[k], alpha, max_valid_cm)
    out = dict(M=M, b=b, D=D, zmax=zmax, weights=weights(rgb[k])[0], x_star=None, minv=None, it=None)
    if zmax > 0:
        out.update(x_star=solve_direct(M, b), minv=minv_norm(M), it=solve_iter(M, b, D))
    return out
