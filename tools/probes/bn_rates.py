#!/usr/bin/env python3
"""development: achieved GB/s of the BatchNorm backward reduce / apply kernels per layer size of BASELINE config 2 (N = 16)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multichannel-semseg-with-uda_amd"))
import torch  # noqa: E402

from mcdseg import ops  # noqa: E402

dev = torch.device("cuda:0")


def timeit(fn, reps=30):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for c, h, w in ((16, 480, 640), (32, 240, 320), (64, 120, 160), (128, 60, 80), (256, 60, 80), (512, 60, 80)):
    n = 16
    dy = torch.randn(n, c, h, w, device=dev)
    z = torch.randn(n, c, h, w, device=dev)
    mean, rstd = torch.zeros(c, device=dev), torch.ones(c, device=dev)
    gamma, beta = torch.ones(c, device=dev), torch.zeros(c, device=dev)
    t = timeit(lambda: ops._channel_reduce(dy, ops.MASK_Z, None, z, mean, rstd, gamma, beta, want_bound=True, train=True))
    nbytes = 2 * dy.numel() * 4
    print("reduce (zmask)  C=%4d %3dx%3d: %7.1f us  %6.0f GB/s  (%d MB)" % (c, h, w, t * 1e3, nbytes / t / 1e6, nbytes >> 20))
