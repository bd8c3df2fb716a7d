"""The depth-to-HHA encoding in numpy: the yardstick of csrc/hha.hip, and the scenes its tests use.

HHA is the three-channel depth encoding of Gupta, Girshick, Arbelaez and Malik (ECCV 2014): horizontal disparity, height above
ground, angle of the surface normal with gravity.  ``hha`` restates the published pipeline (saveHHA, processDepthImage,
computeNormalsSquareSupport, getYDir) for one image; it is the DEFINITION here -- no output of the MATLAB release is at hand, and
nothing is claimed about byte equality with it.  fp64 by default; ``dtype=np.float32`` runs every step in fp32, which gives the unit
the device results are measured in (``rel_to_max`` of the fp32 run against the fp64 run).

``room`` renders the depth of a box room (floor, ceiling, three walls) analytically, with optional Gaussian depth noise and
rectangular holes; ``CASES`` are the scenes of tests/test_hha_gpu.py, whose honesty conditions tests/test_hha_ref_host.py asserts.
"""
import numpy as np

R_SMALL, R_LARGE = 3, 10
THRESHOLDS_DEG = (45.0,) * 5 + (15.0,) * 5
ANGLE_OFFSET = 38.0
MIN_WINDOW_PIXELS = 3
# "|n| is 0" in floating point: a window whose valid pixels lie on one line has adj(M) t = 0 exactly, and fp64 evaluates it to
# ~1e-16 of the terms it is made of -- a direction of pure rounding noise.  |n| counts as 0 up to DEGENERATE x max(sum a^2, sum b^2,
# count)^2 x max|t|.  A window that spans two pixels each way lies (1/fx)^4-ish above that scale's 1e-16: 1e-9 and more on the scenes
# here, 1e-13 for three adjacent pixels at fx = 520.
# The constant is meant for fx, fy up to about 1000 pixels (VGA and HD depth cameras).  The smallest ratio of a window whose valid
# pixels do NOT lie on one line, measured on a room with 93 % of the pixels missing (three-pixel windows): 2e-12 at fx = 365, 6e-13 at 520,
# 3e-13 at 600, 3e-14 at 1050, 1e-14 at 1400 -- the collinear ones stay below 1e-15 at every fx.  Beyond fx ~ 1400 a window of three
# adjacent pixels counts as degenerate too; windows of six and more pixels were never dropped.
DEGENERATE = 1e-14
CLEARANCE = 1e-5  # no |g.N| of a test scene comes closer to a threshold, in any iteration


def rel_to_max(x, truth):
    """max |x - truth| relative to the truth's largest magnitude (the project's per-tensor error measure)"""
    truth = np.asarray(truth, np.float64)
    den = float(np.abs(truth).max()) if truth.size else 0.0
    if truth.size == 0:
        return 0.0
    return float(np.abs(np.asarray(x, np.float64) - truth).max()) / (den if den > 0 else 1.0)


def box_sum(x, r):
    """sum over the window [v-r, v+r] x [u-r, u+r] clipped to the image: 2r+1 shifted adds along the rows, then along the columns"""
    h, w = x.shape
    p = np.zeros((h, w + 2 * r), x.dtype)
    p[:, r:r + w] = x
    rows = np.zeros_like(x)
    for k in range(2 * r + 1):
        rows += p[:, k:k + w]
    p = np.zeros((h + 2 * r, w), x.dtype)
    p[r:r + h] = rows
    out = np.zeros_like(x)
    for k in range(2 * r + 1):
        out += p[k:k + h]
    return out


def normals(a, b, q, valid, r):
    """step 2: N [H,W,3] (zeros where invalid) and the validity mask"""
    dt = q.dtype
    v = valid.astype(dt)
    A, B = np.broadcast_to(a, q.shape) * v, np.broadcast_to(b, q.shape) * v
    with np.errstate(all="ignore"):
        s = [box_sum(np.ascontiguousarray(m.astype(dt)), r) for m in (A * a, A * b, A, B * b, B, v, A * q, B * q, q * v)]
        aa, ab, a1, bb, b1, n1, ta, tb, tq = s
        # adj(M) t, M = [[aa ab a1] [ab bb b1] [a1 b1 n1]]
        nx = (bb * n1 - b1 * b1) * ta + (a1 * b1 - ab * n1) * tb + (ab * b1 - a1 * bb) * tq
        ny = (a1 * b1 - ab * n1) * ta + (aa * n1 - a1 * a1) * tb + (ab * a1 - aa * b1) * tq
        nz = (ab * b1 - bb * a1) * ta + (ab * a1 - aa * b1) * tb + (aa * bb - ab * ab) * tq
        mag = np.sqrt(nx * nx + ny * ny + nz * nz)
        scale = np.maximum(np.maximum(aa, bb), n1) ** 2 * np.maximum(np.maximum(np.abs(ta), np.abs(tb)), np.abs(tq))
        ok = (n1 >= MIN_WINDOW_PIXELS) & np.isfinite(mag) & (mag > 0) & (mag > dt.type(DEGENERATE) * scale)
        n = np.stack([nx, ny, nz], -1) / np.where(ok, mag, 1)[..., None]
    n = np.where(ok[..., None], n, 0).astype(dt)
    n = np.where((n[..., 2] < 0)[..., None], -n, n)
    return n + 0, ok  # (+ 0: no negative zeros)


def gravity(n10, ok, trace=None):
    """step 3: the unit gravity direction from the R = 10 normals; ``trace`` (a list) receives per iteration
    (eigen-gap / largest |eigenvalue|, smallest distance of an |s| to a threshold)"""
    dt = n10.dtype
    nv = n10[ok].reshape(-1, 3)
    g = np.array([0, 1, 0], dt)
    for deg in THRESHOLDS_DEG:
        s = nv @ g
        hi, lo = dt.type(np.cos(np.deg2rad(deg))), dt.type(np.sin(np.deg2rad(deg)))
        f, w = np.abs(s) > hi, np.abs(s) < lo
        if trace is not None:
            near = float(min(np.abs(np.abs(s) - hi).min(), np.abs(np.abs(s) - lo).min())) if s.size else np.inf
        if not (f.any() or w.any()):
            if trace is not None:
                trace.append((np.inf, near))
            continue
        A = nv[w].T @ nv[w] - nv[f].T @ nv[f]
        ev, vec = np.linalg.eigh(A)
        if trace is not None:
            trace.append((float((ev[1] - ev[0]) / max(np.abs(ev).max(), 1e-300)), near))
        g2 = vec[:, 0].astype(dt)
        g2 = g2 / np.sqrt((g2 * g2).sum())
        g = g2 if g @ g2 >= 0 else -g2
    return g + 0


def round_u8(x):
    """half away from zero, saturated to [0, 255]"""
    x = np.asarray(x, np.float64)
    return np.clip(np.sign(x) * np.floor(np.abs(x) + 0.5), 0, 255).astype(np.uint8)


def hha(depth_cm, camera, dtype=np.float64, trace=None, gravity_mask=None):
    """one image: depth [H,W] in centimetres (<= 0 or non-finite: missing), camera (fx, fy, cx, cy) -> dict of
    bytes uint8 [H,W,3], pre (the three channels before rounding), normals3, normals10, gravity [3], height [H,W] (0 at missing
    pixels), y_min, valid.  ``gravity_mask`` [H,W] keeps only these R = 10 normals for step 3.  It is NOT part of the definition and the
    device code has no counterpart to it (``mcdseg_depth_to_hha`` lets every valid normal vote): it exists for the oracle's own tests on the
    noiseless room, where it shows that the ten iterations find the true direction once the windows that straddle two planes are left out."""
    dt = np.dtype(dtype)
    z = np.asarray(depth_cm)
    h, w = z.shape
    valid = np.isfinite(z) & (z > 0)
    z = np.where(valid, z, 1).astype(dt)
    fx, fy, cx, cy = (dt.type(np.float32(c)) for c in camera)
    a = ((np.arange(w, dtype=dt) - cx) / fx)[None, :]
    b = ((np.arange(h, dtype=dt) - cy) / fy)[:, None]
    q = np.where(valid, dt.type(100) / z, 0).astype(dt)
    n3, ok3 = normals(a, b, q, valid, R_SMALL)
    n10, ok10 = normals(a, b, q, valid, R_LARGE)
    g = gravity(n10, ok10 if gravity_mask is None else ok10 & gravity_mask, trace)
    hgt = -(g[0] * (a * z) + g[1] * (b * z) + g[2] * z)
    y_min = hgt[valid].min() if valid.any() else dt.type(np.inf)
    if y_min > -90:
        y_min = dt.type(-130)
    hgt = np.where(valid, hgt - y_min, 0).astype(dt)
    dot = np.clip(n3 @ g, -1, 1)
    pre = np.zeros((h, w, 3), dt)
    pre[..., 0] = dt.type(31000) / np.maximum(z, dt.type(100))
    pre[..., 1] = hgt
    pre[..., 2] = np.where(ok3, np.degrees(np.arccos(dot)) + dt.type(ANGLE_OFFSET), 0)
    pre = np.where(valid[..., None], pre, 0).astype(dt)
    return dict(bytes=round_u8(pre), pre=pre, normals3=n3, normals10=n10, ok3=ok3, ok10=ok10, gravity=g, height=hgt, y_min=y_min, valid=valid)


# ------------------------------------------------------------------------------------------------ scenes
def default_camera(h, w):
    return (0.9 * w, 0.9 * w, (w - 1) / 2.0, (h - 1) / 2.0)


def room(h, w, camera=None, cam_height=120.0, pitch=12.0, roll=5.0, yaw=20.0, ceiling=270.0, front=350.0, right=220.0, left=180.0,
         noise=0.0, holes=(), seed=0):
    """depth (fp64, centimetres) of a box room seen from a camera ``cam_height`` above the floor, pitched down by ``pitch`` and rolled by
    ``roll`` degrees, the walls turned by ``yaw`` about the vertical.  ``noise``: standard deviation of Gaussian depth noise (cm);
    ``holes``: (v0, u0, rows, cols) rectangles of missing depth (0).  Returns (depth, truth) with truth = dict(gravity, plane [H,W] in
    0..4 = floor, ceiling, front, right, left, normal [5,3] with z >= 0, interior [H,W]: the 7 x 7 window sees one plane)"""
    camera = camera or default_camera(h, w)
    fx, fy, cx, cy = (float(np.float32(c)) for c in camera)
    p, r, y = np.deg2rad([pitch, roll, yaw])
    g = np.array([-np.sin(r) * np.cos(p), np.cos(r) * np.cos(p), np.sin(p)])
    f = np.array([0.0, 0.0, 1.0]) - g[2] * g
    f /= np.linalg.norm(f)
    s = np.cross(g, f)
    f, s = np.cos(y) * f + np.sin(y) * s, -np.sin(y) * f + np.cos(y) * s
    planes = [(g, cam_height), (-g, ceiling - cam_height), (f, front), (s, right), (-s, left)]
    a = ((np.arange(w) - cx) / fx)[None, :] + np.zeros((h, 1))
    b = ((np.arange(h) - cy) / fy)[:, None] + np.zeros((1, w))
    ray = np.stack([a, b, np.ones_like(a)], -1)
    t = np.full((5, h, w), np.inf)
    for k, (n, d) in enumerate(planes):
        den = ray @ n
        t[k] = np.where(den > 1e-12, d / np.where(den > 1e-12, den, 1), np.inf)
    plane = t.argmin(0)
    depth = t.min(0)
    if noise > 0:
        depth = depth + np.random.RandomState(seed).normal(0, noise, depth.shape)
    for v0, u0, rows, cols in holes:
        depth[v0:v0 + rows, u0:u0 + cols] = 0
    normal = np.stack([n if n[2] >= 0 else -n for n, _ in planes])
    return depth, dict(gravity=g, plane=plane, normal=normal, interior=single_plane(plane, R_SMALL), camera=(fx, fy, cx, cy))


def single_plane(plane, r):
    """[H,W]: the window of radius ``r`` (clipped to the image) lies on one plane"""
    h, w = plane.shape
    same = np.ones((h, w), bool)
    pad = np.pad(plane, r, mode="edge")
    for dv in range(2 * r + 1):
        for du in range(2 * r + 1):
            same &= pad[dv:dv + h, du:du + w] == plane
    return same


# the scenes of tests/test_hha_gpu.py: name -> list of room() keyword sets, one per image of the batch.  Every scene carries depth noise,
# and its ``seed`` is the first for which the honesty conditions hold (``first_honest_seed``; tests/test_hha_ref_host.py asserts that the
# recorded seeds satisfy them).
CASES = {
    "clipped_8x12": [dict(h=8, w=12, pitch=35.0, noise=0.2, seed=1)],
    "odd_37x53": [dict(h=37, w=53, noise=0.2, seed=3)],
    "two_rooms_48x64": [dict(h=48, w=64, noise=0.2, seed=0),
                        dict(h=48, w=64, cam_height=150.0, pitch=20.0, roll=-8.0, yaw=-30.0, ceiling=300.0, front=420.0, right=150.0, noise=0.2, seed=0)],
    "noise_holes_96x128": [dict(h=96, w=128, noise=0.3, holes=((40, 50, 9, 9), (0, 100, 12, 7), (70, 20, 5, 11)), seed=1)],
}


def case_depth(name):
    """the fp32 depth batch [N,H,W] and cameras [N,4] of a case"""
    rooms = [room(**kw) for kw in CASES[name]]
    depth = np.stack([d for d, _ in rooms]).astype(np.float32)
    cams = np.array([t["camera"] for _, t in rooms], np.float32)
    return depth, cams


# The bounds of a comparison with a device result (tests/test_hha_gpu.py).  A float tensor may lie
# max(FLOOR, min(2 x the fp32 run's own distance, CAP)) from the fp64 oracle, by ``rel_to_max``:
#   2 x the fp32 unit  the project's rule for the loss kernels;
#   CAP     a tenth of CLEARANCE: a normal and a g within CAP (x sqrt 3 for the three components, twice) move no |g.N| by CLEARANCE, so
#           the device's sets F and W are the oracle's -- without the cap the fp32 unit of the normals (the adjugate cancels ~10 digits;
#           the fp32 run is off by 5e-6 ... 2.0) would allow results whose gravity iteration took another path;
#   FLOOR   2^-23, for tensors the fp32 run reproduces exactly (an all-missing image: g = (0,1,0), heights 0): the outputs are fp32,
#           rounded once (2^-24 of the value), the project's factor 2 on top.
FLOOR = 2.0 ** -23
CAP = 1e-6  # CLEARANCE / 10


def float_bounds(r64, r32):
    return {k: max(FLOOR, min(2 * rel_to_max(r32[k], r64[k]), CAP)) for k in ("normals3", "gravity", "height")}


def byte_margins(r64, bounds):
    """[H,W,3]: how far a device value before rounding may lie from the oracle's, in byte units, given the float bounds: the disparity
    is one fp64 division of the fp32 depth (FLOOR of its largest value); the height's bound is the float bound of ``height``; the angle's
    follows from d = sqrt(3) (bound of normals3 + bound of gravity) on the cosine, through acosd on [cos - d, cos + d]"""
    pre = r64["pre"].astype(np.float64)
    m = np.zeros(pre.shape)
    m[..., 0] = FLOOR * max(float(pre[..., 0].max()), 1.0)
    m[..., 1] = bounds["height"] * max(float(np.abs(r64["height"]).max()), 1.0)
    d = np.sqrt(3.0) * (bounds["normals3"] * max(float(np.abs(r64["normals3"]).max()), 1.0) + bounds["gravity"])
    dot = np.clip(r64["normals3"].astype(np.float64) @ r64["gravity"].astype(np.float64), -1, 1)
    ang = np.degrees(np.arccos(dot))
    m[..., 2] = np.maximum(np.abs(np.degrees(np.arccos(np.clip(dot - d, -1, 1))) - ang), np.abs(np.degrees(np.arccos(np.clip(dot + d, -1, 1))) - ang))
    return m


def near_rounding(r64, margins):
    """[H,W,3] bool: the value before rounding lies within its margin of a .5 boundary"""
    pre = r64["pre"].astype(np.float64)
    return np.abs(pre - np.floor(pre) - 0.5) <= margins


def byte_margin_share(r64, margins):
    """share of the pixels with a channel within its margin of a rounding boundary"""
    return float(near_rounding(r64, margins).any(-1).mean())


def honesty(depth, camera):
    """the conditions that keep a comparison with a device result honest, of one fp32 depth image: (smallest eigen-gap of A relative to
    its largest eigenvalue, smallest distance of a |g.N| to a threshold, distance of the raw y_min from -90, share of the pixels within
    the byte margin of a rounding boundary, the fp64 result, the float bounds, the margins)"""
    trace = []
    r64 = hha(depth, camera, trace=trace)
    bounds = float_bounds(r64, hha(depth, camera, dtype=np.float32))
    margins = byte_margins(r64, bounds)
    raw_min = float(r64["height"][r64["valid"]].min() + r64["y_min"]) if r64["valid"].any() else -np.inf
    return min(t[0] for t in trace), min(t[1] for t in trace), abs(raw_min + 90.0), byte_margin_share(r64, margins), r64, bounds, margins


def is_honest(gap, near, ymin_gap, share):
    return gap >= 1e-3 and near >= CLEARANCE and ymin_gap >= 1.0 and share <= 0.02


def first_honest_seed(kw, limit=256):
    """the first noise seed of a scene for which ``is_honest`` holds"""
    for seed in range(limit):
        d, t = room(**dict(kw, seed=seed))
        if is_honest(*honesty(d.astype(np.float32), t["camera"])[:4]):
            return seed
    raise AssertionError("no honest seed below %d" % limit)
