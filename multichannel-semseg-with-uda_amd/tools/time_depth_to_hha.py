#!/usr/bin/env python3
"""Milliseconds per image of the depth -> HHA encoding in two forms, on one GPU:

    fused     ``ops.depth_to_hha``: the kernels of csrc/hha.hip
    composed  the same procedure (tests/hha_ref.py line for line) from torch operations on the device, in fp64:
              shifted adds for the window sums, masked einsums and a batched ``torch.linalg.eigh`` for the gravity iteration

480 x 640 with ``-b 16`` by default, on a synthetic room-like depth batch with noise and holes.  Calls are bracketed by device events after
``--warmup`` calls; the two forms alternate.  Prints one JSON line.

    python tools/time_depth_to_hha.py --reps 5 --warmup 2
"""
import argparse
import json
import math
import os
import statistics
import sys

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, PKG)


def box_sum(x, r):
    """[N,H,W] -> sums over the clipped (2r+1)^2 windows: shifted adds along the rows, then along the columns"""
    import torch
    n, h, w = x.shape
    p = torch.zeros((n, h, w + 2 * r), dtype=x.dtype, device=x.device)
    p[:, :, r:r + w] = x
    rows = torch.zeros_like(x)
    for k in range(2 * r + 1):
        rows += p[:, :, k:k + w]
    p = torch.zeros((n, h + 2 * r, w), dtype=x.dtype, device=x.device)
    p[:, r:r + h] = rows
    out = torch.zeros_like(x)
    for k in range(2 * r + 1):
        out += p[:, k:k + h]
    return out


def composed(depth, camera):
    """the definition from torch operations: fp32 depth [N,H,W] (cm), camera [N,4] -> (uint8 [N,H,W,3], g [N,3] fp64)"""
    import torch
    dt = torch.float64
    n, h, w = depth.shape
    dev = depth.device
    valid = torch.isfinite(depth) & (depth > 0)
    z = torch.where(valid, depth, torch.ones_like(depth)).to(dt)
    cam = camera.to(dt)
    a = ((torch.arange(w, dtype=dt, device=dev)[None, :] - cam[:, 2:3]) / cam[:, 0:1])[:, None, :]
    b = ((torch.arange(h, dtype=dt, device=dev)[None, :] - cam[:, 3:4]) / cam[:, 1:2])[:, :, None]
    v = valid.to(dt)
    q = v * (100.0 / z)
    A, B = a * v, b * v
    moments = (A * a, A * b, A, B * b, B, v, A * q, B * q, q)

    def normals(r):
        aa, ab, a1, bb, b1, n1, ta, tb, tq = [box_sum(m.contiguous(), r) for m in moments]
        nx = (bb * n1 - b1 * b1) * ta + (a1 * b1 - ab * n1) * tb + (ab * b1 - a1 * bb) * tq
        ny = (a1 * b1 - ab * n1) * ta + (aa * n1 - a1 * a1) * tb + (ab * a1 - aa * b1) * tq
        nz = (ab * b1 - bb * a1) * ta + (ab * a1 - aa * b1) * tb + (aa * bb - ab * ab) * tq
        mag = torch.sqrt(nx * nx + ny * ny + nz * nz)
        scale = torch.maximum(torch.maximum(aa, bb), n1) ** 2 * torch.maximum(torch.maximum(ta.abs(), tb.abs()), tq.abs())
        ok = (n1 >= 3) & torch.isfinite(mag) & (mag > 0) & (mag > 1e-14 * scale)
        nrm = torch.stack([nx, ny, nz], -1) / torch.where(ok, mag, torch.ones_like(mag))[..., None]
        nrm = torch.where(ok[..., None], nrm, torch.zeros_like(nrm))
        return torch.where((nrm[..., 2] < 0)[..., None], -nrm, nrm), ok

    n3, ok3 = normals(3)
    n10, ok10 = normals(10)
    g = torch.tensor([0.0, 1.0, 0.0], dtype=dt, device=dev).repeat(n, 1)
    flat, okf = n10.reshape(n, -1, 3), ok10.reshape(n, -1)
    for deg in (45.0,) * 5 + (15.0,) * 5:
        s = torch.einsum("npk,nk->np", flat, g).abs()
        f = (okf & (s > math.cos(math.radians(deg)))).to(dt)
        wk = (okf & (s < math.sin(math.radians(deg)))).to(dt)
        A3 = torch.einsum("np,npi,npj->nij", wk - f, flat, flat)
        _, vec = torch.linalg.eigh(A3)
        g2 = vec[:, :, 0]
        g2 = g2 / g2.norm(dim=1, keepdim=True)
        g2 = torch.where(((g * g2).sum(1) >= 0)[:, None], g2, -g2)
        g = torch.where(((f + wk).sum(1) > 0)[:, None], g2, g)
    gx, gy, gz = g[:, 0, None, None], g[:, 1, None, None], g[:, 2, None, None]
    hgt = -(gx * (a * z) + gy * (b * z) + gz * z)
    y_min = torch.where(valid, hgt, torch.full_like(hgt, float("inf"))).amin(dim=(1, 2))
    y_min = torch.where(y_min > -90, torch.full_like(y_min, -130.0), y_min)
    hgt = hgt - y_min[:, None, None]
    dot = torch.einsum("nhwk,nk->nhw", n3, g).clamp(-1, 1)
    ang = torch.where(ok3, torch.rad2deg(torch.acos(dot)) + 38.0, torch.zeros_like(dot))
    pre = torch.stack([31000.0 / z.clamp(min=100.0), hgt, ang], -1) * v[..., None]
    return torch.floor(pre + 0.5).clamp(0, 255).to(torch.uint8), g


def synthetic_depth(n, h, w, dev, seed):
    """a floor, a front wall and a side wall seen from 1.2 m with a pitched camera, 0.3 cm of noise, 1 % missing pixels and one hole"""
    import torch
    gen = torch.Generator(device="cpu").manual_seed(seed)
    fx = 0.9 * w
    a = ((torch.arange(w, dtype=torch.float64) - (w - 1) / 2) / fx)[None, None, :]
    b = ((torch.arange(h, dtype=torch.float64) - (h - 1) / 2) / fx)[None, :, None]
    pitch = torch.deg2rad(10 + 5 * torch.rand(n, generator=gen, dtype=torch.float64))[:, None, None]
    gy, gz = torch.cos(pitch), torch.sin(pitch)
    inf = torch.full((n, h, w), float("inf"), dtype=torch.float64)
    floor = 120.0 / (gy * b + gz).clamp(min=1e-9)
    den = -gz * b + gy
    front = torch.where(den > 1e-9, 350.0 / den.clamp(min=1e-9), inf) + 0 * a
    side = torch.where(a > 1e-9, 220.0 / a.clamp(min=1e-9), inf) + 0 * b
    depth = torch.minimum(torch.minimum(floor + 0 * a, front), side)
    depth = depth + 0.3 * torch.randn(depth.shape, generator=gen, dtype=torch.float64)
    depth[torch.rand(depth.shape, generator=gen) < 0.01] = 0
    depth[:, h // 3:h // 3 + 40, w // 2:w // 2 + 60] = 0
    camera = torch.tensor([fx, fx, (w - 1) / 2, (h - 1) / 2], dtype=torch.float32).repeat(n, 1)
    return depth.float().to(dev), camera


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", type=int, nargs=2, default=(640, 480), metavar=("W", "H"))
    ap.add_argument("-b", "--batch_size", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--forms", nargs="+", default=("fused", "composed"), choices=("fused", "composed"))
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this measurement runs on an MI355X: there is no CPU fallback")
    from mcdseg import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    w, h = args.shape
    n = args.batch_size
    depth, camera = synthetic_depth(n, h, w, dev, args.seed)
    cam_dev = camera.to(dev)

    def call(form):
        if form == "fused":
            out, parts = ops.depth_to_hha(depth, camera, return_parts=True)
            return out, parts["gravity"].double()
        with torch.no_grad():
            return composed(depth, cam_dev)

    times = {f: [] for f in args.forms}
    out = {}
    for rep in range(args.warmup + args.reps):
        for form in args.forms:
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
    result = {"shape_wh": [w, h], "batch": n, "warmup": args.warmup}
    for form in args.forms:
        t = times[form]
        result[form] = {"reps": len(t), "ms_per_image_median": round(statistics.median(t), 4), "ms_per_image_min_max": [round(min(t), 4), round(max(t), 4)]}
    if len(times) == 2:
        result["speedup"] = round(statistics.median(times["composed"]) / statistics.median(times["fused"]), 2)
        diff = (out["fused"][0].int() - out["composed"][0].int()).abs()
        result["bytes_that_differ"] = int((diff > 0).sum())
        result["largest_byte_difference"] = int(diff.max())
        result["largest_gravity_difference"] = float((out["fused"][1] - out["composed"][1]).abs().max())
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
