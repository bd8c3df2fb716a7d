#!/usr/bin/env python3
"""Milliseconds per image of the colorization depth inpainting in three forms:

    kernels   ``ops.fill_depth``: the kernels of csrc/fill.hip, host read-backs of the status records included
    composed  the same right-preconditioned BiCGSTAB, with the same stopping rule and the same freeze of finished images, from torch fp64
              operations on the device: shifted slices for the 8-neighbour stencil, ``sum`` for the dot products, a status read-back
              every ``check_every`` iterations
    spsolve   ``scipy.sparse.linalg.spsolve`` on the CPU, of the first image's system only (built from the device's weights; the
              time is the solve's alone, wall clock)

480 x 640 with ``-b 16`` by default, on synthetic rooms with a blind border band, six round holes of up to 60 pixels radius and 2 % of
speckle.  Device calls are bracketed by device events after ``--warmup`` calls; the forms alternate.  Prints one JSON line.

    python tools/time_fill_depth.py --reps 5 --warmup 2
"""
import argparse
import json
import os
import statistics
import sys
import time

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, PKG)

DIRS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def shifted(a, dy, dx, fill=0.0):
    """[N,H,W] -> a[:, v + dy, u + dx] inside the image, ``fill`` outside"""
    import torch.nn.functional as F
    h, w = a.shape[1:]
    return F.pad(a, (1, 1, 1, 1), value=fill)[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


def composed_system(rgb, z, alpha):
    """(weights [8][N,H,W], D, b, zmax) of the definition, from torch operations in fp64"""
    import torch
    dt = torch.float64
    c = rgb.to(dt)
    g = ((0.299 * c[..., 0] + 0.587 * c[..., 1]) + 0.114 * c[..., 2]) / 255.0
    inside = [shifted(torch.ones_like(g), dy, dx) > 0 for dy, dx in DIRS]
    gq = [shifted(g, dy, dx) for dy, dx in DIRS]
    count = 1 + sum(m.to(dt) for m in inside)
    mu = (g + sum(torch.where(m, q, torch.zeros_like(q)) for m, q in zip(inside, gq))) / count
    var = ((g - mu) ** 2 + sum(torch.where(m, (q - mu) ** 2, torch.zeros_like(q)) for m, q in zip(inside, gq))) / count
    d2 = [(q - g) ** 2 for q in gq]
    nearest = torch.stack([torch.where(m, d, torch.full_like(d, float("inf"))) for m, d in zip(inside, d2)]).amin(0)
    sigma = torch.maximum(torch.maximum(0.6 * var, nearest / 4.605170185988092), torch.full_like(var, 2e-6))
    wk = [torch.where(m, torch.exp(-d / sigma), torch.zeros_like(d)) for m, d in zip(inside, d2)]
    wsum = sum(wk)
    wk = [k / wsum for k in wk]
    known = torch.isfinite(z) & (z > 0)
    zmax = torch.where(known, z, torch.zeros_like(z)).amax(dim=(1, 2)).to(dt)
    zn = torch.where(known, z.to(dt) / zmax.clamp(min=1e-300)[:, None, None], torch.zeros_like(g))
    return wk, torch.where(known, 1.0 + alpha, 1.0).to(dt), alpha * zn, zmax


def composed(rgb, z, alpha=1.0, rtol=1e-10, max_iter=4000, check_every=8):
    """-> (filled fp32 [N,H,W], iterations [N])"""
    import torch
    wk, D, b, zmax = composed_system(rgb, z, alpha)
    n = z.shape[0]

    def M(x):
        out = D * x
        for k, (dy, dx) in enumerate(DIRS):
            out = out - wk[k] * shifted(x, dy, dx)
        return out

    def dot(u, v):
        return (u * v).sum(dim=(1, 2))[:, None, None]

    bn = dot(b, b).sqrt()
    x = b / D
    r = b - M(x)
    rhat = r.clone()
    one = torch.ones((n, 1, 1), dtype=torch.float64, device=z.device)
    rho, a, omega = one.clone(), one.clone(), one.clone()
    v, p = torch.zeros_like(b), torch.zeros_like(b)
    running = (zmax > 0)[:, None, None]
    iters = torch.zeros(n, dtype=torch.int64, device=z.device)

    def check(running):
        t = b - M(x)
        return running & ~(dot(t, t).sqrt() <= rtol * bn)

    running = check(running)
    done = 0
    while done < max_iter and bool(running.any().cpu()):
        for _ in range(min(check_every, max_iter - done)):
            rho_new = dot(rhat, r)
            beta = (rho_new / rho) * (a / omega)
            p_new = r + beta * (p - omega * v)
            v_new = M(p_new / D)
            a_new = rho_new / dot(rhat, v_new)
            s = r - a_new * v_new
            t = M(s / D)
            omega_new = dot(t, s) / dot(t, t)
            x_new = x + (a_new * (p_new / D) + omega_new * (s / D))
            r_new = s - omega_new * t
            keep = lambda new, old: torch.where(running, new, old)  # noqa: E731  (a finished image is frozen)
            x, r, p, v, rho, a, omega = (keep(x_new, x), keep(r_new, r), keep(p_new, p), keep(v_new, v), keep(rho_new, rho),
                                         keep(a_new, a), keep(omega_new, omega))
            iters += running.reshape(n).to(torch.int64)
            done += 1
        running = check(running)
    return (x * zmax[:, None, None]).float(), iters


def synthetic_scenes(n, h, w, seed):
    """(rgb uint8 [N,H,W,3], depth fp32 [N,H,W] cm): a floor, a front wall and a side wall, painted by plane and shaded with depth, with
    pixel noise; missing: a blind band at the left border, six round holes (radius up to 60 pixels at 480 x 640), 2 % of speckle"""
    import numpy as np
    rs = np.random.RandomState(seed)
    fx = 0.9 * w
    a = ((np.arange(w) - (w - 1) / 2) / fx)[None, None, :]
    b = ((np.arange(h) - (h - 1) / 2) / fx)[None, :, None]
    pitch = np.deg2rad(10 + 5 * rs.rand(n))[:, None, None]
    gy, gz = np.cos(pitch), np.sin(pitch)
    floor = 120.0 / np.maximum(gy * b + gz, 1e-9) + 0 * a
    den = -gz * b + gy
    front = np.where(den > 1e-9, 350.0 / np.maximum(den, 1e-9), np.inf) + 0 * a
    side = np.where(a > 1e-9, 220.0 / np.maximum(a, 1e-9), np.inf) + 0 * b + 0 * pitch
    planes = np.stack([floor, front, side])
    depth, plane = planes.min(0) + rs.normal(0, 0.3, (n, h, w)), planes.argmin(0)
    base = np.array([[150, 120, 90], [120, 150, 180], [200, 170, 120]], np.float64)
    shade = 1.0 - 0.45 * (depth - depth.min()) / (depth.max() - depth.min())
    rgb = np.clip(np.rint(base[plane] * shade[..., None] + rs.normal(0, 4.0, (n, h, w, 3))), 0, 255).astype(np.uint8)
    vv, uu = np.mgrid[:h, :w]
    rmax = max(2, h // 8)
    for k in range(n):
        depth[k, :, :max(1, w // 64)] = 0
        for _ in range(6):
            cv, cu, r = rs.randint(0, h), rs.randint(0, w), rs.randint(max(1, rmax // 3), rmax + 1)
            depth[k][(vv - cv) ** 2 + (uu - cu) ** 2 <= r * r] = 0
    depth[rs.rand(n, h, w) < 0.02] = 0
    return rgb, depth.astype(np.float32)


def spsolve_first(weights, depth, alpha, zmax):
    """the first image's system from the device's weights [8,H,W] -> (x [H,W], seconds of the solve alone)"""
    import numpy as np
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    h, w = depth.shape
    known = np.isfinite(depth) & (depth > 0)
    idx = np.arange(h * w).reshape(h, w)
    rows, cols, vals = [idx.reshape(-1)], [idx.reshape(-1)], [np.where(known, 1.0 + alpha, 1.0).reshape(-1)]
    for k, (dy, dx) in enumerate(DIRS):
        m = weights[k] > 0
        rows.append(idx[m]), cols.append(idx[m] + dy * w + dx), vals.append(-weights[k][m])
    M = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(h * w, h * w))
    b = np.where(known, alpha * depth.astype(np.float64) / zmax, 0.0).reshape(-1)
    t0 = time.perf_counter()
    x = spla.spsolve(M, b)
    return x.reshape(h, w), time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", type=int, nargs=2, default=(640, 480), metavar=("W", "H"))
    ap.add_argument("-b", "--batch_size", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--forms", nargs="+", default=("kernels", "composed", "spsolve"), choices=("kernels", "composed", "spsolve"))
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this measurement runs on an MI355X: there is no CPU fallback")
    from mcdseg import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    w, h = args.shape
    n = args.batch_size
    rgb_np, depth_np = synthetic_scenes(n, h, w, args.seed)
    rgb, depth = torch.from_numpy(rgb_np).to(dev), torch.from_numpy(depth_np).to(dev)

    def call(form):
        if form == "kernels":
            out, parts = ops.fill_depth(rgb, depth, return_parts=True)
            return out, parts["iterations"], parts
        with torch.no_grad():
            out, iters = composed(rgb, depth)
            return out, iters.cpu(), None

    device_forms = [f for f in args.forms if f != "spsolve"]
    times = {f: [] for f in device_forms}
    out = {}
    for rep in range(args.warmup + args.reps):
        for form in device_forms:
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out[form] = call(form)
            e.record()
            torch.cuda.synchronize()
            print("%s %s: %.3f ms" % ("warmup" if rep < args.warmup else "rep %d" % (rep - args.warmup), form, s.elapsed_time(e)),
                  file=sys.stderr, flush=True)
            if rep >= args.warmup:
                times[form].append(s.elapsed_time(e) / n)
    result = {"shape_wh": [w, h], "batch": n, "warmup": args.warmup, "missing_share": round(float((depth_np <= 0).mean()), 4)}
    for form in device_forms:
        t = times[form]
        its = out[form][1].tolist()
        result[form] = {"reps": len(t), "ms_per_image_median": round(statistics.median(t), 4),
                        "ms_per_image_min_max": [round(min(t), 4), round(max(t), 4)], "iterations_min_max": [min(its), max(its)]}
    if "kernels" in out:
        parts = out["kernels"][2]
        result["kernels"]["statuses"] = sorted(set(ops.FILL_STATUS_NAMES[int(s)] for s in parts["status"]))
        result["kernels"]["largest_residual"] = float(parts["residual"].max())
    if len(device_forms) == 2:
        result["speedup_over_composed"] = round(statistics.median(times["composed"]) / statistics.median(times["kernels"]), 2)
        result["largest_difference_cm_kernels_composed"] = float((out["kernels"][0].double() - out["composed"][0].double()).abs().max())
    if "spsolve" in args.forms and "kernels" in out:
        parts = out["kernels"][2]
        zmax = float(parts["zmax"][0])
        x, seconds = spsolve_first(parts["weights"][0].cpu().numpy(), depth_np[0], 1.0, zmax)
        result["spsolve"] = {"images": 1, "ms_per_image": round(1000 * seconds, 1)}
        result["largest_difference_cm_kernels_spsolve"] = float(abs(parts["x"][0].cpu().numpy() - x).max() * zmax)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
