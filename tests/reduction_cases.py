"""The cases of tests/test_reduction_bits_gpu.py and tests/golden/make_reduction_bits.py: every public op that reduces to scalars, on
seeded CPU inputs, returning the bit patterns of those scalars.

Each reduced scalar of the library is a fixed-order sum (csrc/block_reduce.h: per thread, per wave, the waves of a block in tree or
chain order, then the blocks' partial rows in fp64), so its bits are a property of the build.  The shapes are the smallest that walk
every step: an element count that is no multiple of a block's span; per finalizer at least one case with more than 256 partial rows
(256 threads stride over them: 66 306 pixels for the one-pixel-per-thread kernels, 1.1 M elements for the ceil(n / 4096) grids, 600 001
labels for ceil(n / 2048)) -- except where the grid is capped at 256 rows or fewer (the up-sampling loss kernels, the uncertain loss);
single-block cases (ONE_BLOCK below); C in {5, 41}.  Values are +-2^u, u uniform in [-10, 10], with one row of -0.0, and labels hold ignored and
out-of-range entries, so that the partial sums differ in sign and magnitude and another combination order gives other bits."""
import re

import numpy as np
import torch

IGNORE = 255


def compiler_version(path):
    """the compiler's identification as the built library carries it (its .comment sections)"""
    with open(path, "rb") as f:
        m = re.search(rb"[ -~]*clang version [ -~]+", f.read())
    return m.group(0).decode() if m else "unknown"


def _vals(rng, *shape):
    v = (np.exp2(rng.uniform(-10.0, 10.0, shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    v.reshape(-1, shape[-1])[0, :64] = -0.0
    return v


def _labels(rng, c, *shape):
    y = rng.integers(0, c, shape).astype(np.int64)
    y[rng.random(shape) < 0.1] = IGNORE
    y[rng.random(shape) < 0.02] = -1
    return y


def _weights(rng, c):
    w = rng.uniform(0.25, 4.0, c).astype(np.float32)
    w[c - 1] = 0.0
    return w


def _up_w(rng, c):
    return (rng.standard_normal((c, 1, 16, 16)) * 0.25).astype(np.float32)


def _bits(*tensors):
    torch.cuda.synchronize()
    flat = np.concatenate([t.detach().float().cpu().numpy().reshape(-1) for t in tensors]).astype(np.float32)
    return [int(b) for b in flat.view(np.uint32)]


def _mcd(seed, n, c, h, w, two, dist):
    def run(dev, ops):
        rng = np.random.default_rng(seed)
        z1 = torch.from_numpy(_vals(rng, n, c, h, w)).to(dev)
        z2 = torch.from_numpy(_vals(rng, n, c, h, w)).to(dev) if two else None
        y = torch.from_numpy(_labels(rng, c, n, h, w)).to(dev)
        cw = torch.from_numpy(_weights(rng, c)).to(dev)
        losses, _, _ = ops.mcd_losses(z1, z2, y, cw, ignore_index=IGNORE, ce_coef=1.0, diff_coef=1.0 if two else 0.0, want_grad=False, dist=dist)
        return _bits(losses)
    return run


def _up8_mcd(seed, n, c, hi, wi, two, dist, dma):
    def run(dev, ops):
        rng = np.random.default_rng(seed)
        s1 = torch.from_numpy(_vals(rng, n, c, hi, wi)).to(dev)
        s2 = torch.from_numpy(_vals(rng, n, c, hi, wi)).to(dev) if two else None
        w1 = torch.from_numpy(_up_w(rng, c)).to(dev)
        w2 = torch.from_numpy(_up_w(rng, c)).to(dev) if two else None
        # labels at a 16-byte aligned base run the LDS-DMA kernel; a view that starts 8 bytes off such a base, the register-staged one
        off = 2 if dma else 1
        y = np.zeros(n * 64 * hi * wi + off, np.int64)
        y[off:] = _labels(rng, c, n * 64 * hi * wi)
        y = torch.from_numpy(y).to(dev)[off:].view(n, 8 * hi, 8 * wi)
        cw = torch.from_numpy(_weights(rng, c)).to(dev)
        name = ops.up8_loss_kernel_name(n, c, hi, wi, two, y, dist)
        assert ("_dma_kernel" in name) == dma, name
        losses, _, _ = ops.up8_mcd_losses(s1, w1, s2, w2, y, cw, ignore_index=IGNORE, ce_coef=1.0, diff_coef=1.0 if two else 0.0,
                                          want_grad=False, dist=dist)
        return _bits(losses)
    return run


def _wsum(seed, c, p):
    def run(dev, ops):
        rng = np.random.default_rng(seed)
        y = torch.from_numpy(_labels(rng, c, p)).to(dev)
        return _bits(ops.label_weight_sum(y, torch.from_numpy(_weights(rng, c)).to(dev), c, IGNORE))
    return run


def _predict(seed, n, c, h, w, two, used):
    def run(dev, ops):
        rng = np.random.default_rng(seed)
        z1 = torch.from_numpy(_vals(rng, n, c, h, w) / 64.0).to(dev)
        z2 = torch.from_numpy(_vals(rng, n, c, h, w) / 64.0).to(dev) if two else None
        return _bits(ops.predict_labels(z1, z2, used)[1])
    return run


def _predict_up(seed, n, c, hi, wi, learned, used):
    def run(dev, ops):
        rng = np.random.default_rng(seed)
        s = torch.from_numpy(_vals(rng, n, c, hi, wi) / 64.0).to(dev)
        if learned:
            return _bits(ops.predict_labels_up8(s, torch.from_numpy(_up_w(rng, c)).to(dev), used)[1])
        return _bits(ops.predict_labels_bilinear8(s, used)[1])
    return run


def _mse(seed, n):
    def run(dev, ops):
        rng = np.random.default_rng(seed)
        return _bits(ops.mse_loss(torch.from_numpy(_vals(rng, n)).to(dev), torch.from_numpy(_vals(rng, n)).to(dev)))
    return run


def _prob(rng, *shape):
    return (1.0 / (1.0 + np.exp2(rng.uniform(-10.0, 10.0, shape)))).astype(np.float32)


def _bce2d(seed, n, u8):
    def run(dev, ops):
        rng = np.random.default_rng(seed)
        p = torch.from_numpy(_prob(rng, n)).to(dev)
        t = (rng.random(n) < 0.2)
        t = torch.from_numpy(t.astype(np.uint8) if u8 else (t * rng.random(n)).astype(np.float32)).to(dev)
        return _bits(*ops.bce2d(p, t, return_beta=True))
    return run


class _Ctx:  # what an autograd Function's forward needs of its context: the saved tensors hold [loss, beta]
    def save_for_backward(self, *tensors):
        self.saved = tensors


def _head_bce(seed, n, h8, w8, c):
    def run(dev, ops):
        rng = np.random.default_rng(seed)
        s1, s2, s3 = (torch.from_numpy(_vals(rng, n, 1, k * h8, k * w8) / 64.0).to(dev) for k in (4, 2, 1))
        y = np.repeat(np.repeat(_labels(rng, c, n, h8, w8), 8, 1), 8, 2)  # (blocks of one label: boundaries on a tenth of the pixels)
        ctx = _Ctx()
        loss = ops._BoundaryHeadBCE.forward(ctx, s1, s2, s3, torch.from_numpy(np.ascontiguousarray(y)).to(dev))
        out = ctx.saved[-1]
        assert _bits(loss) == _bits(out[0])
        return _bits(out)
    return run


def _seg2bd(seed, n, c, hi, wi):
    def run(dev, ops):
        rng = np.random.default_rng(seed)
        z1, z2 = (torch.from_numpy(_vals(rng, n, c, hi, wi) / 256.0).to(dev) for _ in range(2))
        wt = torch.from_numpy((rng.standard_normal((1, c, 5, 5)) * 0.1).astype(np.float32)).to(dev).requires_grad_(True)
        b = torch.tensor([-0.3], dtype=torch.float32, device=dev, requires_grad=True)
        t = torch.from_numpy((rng.random((n, 1, 8 * hi, 8 * wi)) < 0.2).astype(np.uint8)).to(dev)
        l1, l2, beta = ops.seg2bd_bce(z1, z2, wt, b, t, return_beta=True)
        (l1 + 0.5 * l2).backward()
        return _bits(l1, l2, beta, b.grad)
    return run


def _uncertain(seed, n, c, hi, wi, t):
    def run(dev, ops):
        rng = np.random.default_rng(seed)
        s = torch.from_numpy(_vals(rng, n, c, hi, wi) / 64.0).to(dev)
        w_up, w_std = (torch.from_numpy(_up_w(rng, c)).to(dev) for _ in range(2))
        y = torch.from_numpy(_labels(rng, c, n, 8 * hi, 8 * wi)).to(dev)
        keep = torch.from_numpy((rng.random((t, n, c)) < 0.8).astype(np.uint8)).to(dev)
        r = torch.from_numpy(rng.random(t).astype(np.float32)).to(dev)
        base, unc = ops.up8_uncertain_loss(s, w_up, w_std, y, torch.from_numpy(_weights(rng, c)).to(dev), keep, r, ignore_index=IGNORE)
        return _bits(base, unc)
    return run


def _prob_nll(seed, n, c, h, w):
    def run(dev, ops):
        rng = np.random.default_rng(seed)
        p = _prob(rng, n, c, h, w)
        p = torch.from_numpy(p / p.sum(1, keepdims=True)).to(dev)
        y = torch.from_numpy(_labels(rng, c, n, h, w)).to(dev)
        return _bits(ops.prob_cross_entropy2d(p, y, torch.from_numpy(_weights(rng, c)).to(dev), IGNORE))
    return run


# name -> run(device, ops) -> [uint32 bit patterns]; the recorded scalars are named in the comments
CASES = {
    # losses[0:4] = CE1, CE2, discrepancy, sum w[y]
    "mcd_losses/diff-two-c41-260blocks": _mcd(1, 1, 41, 258, 257, True, "diff"),
    "mcd_losses/jsd-two-c5-260blocks": _mcd(3, 2, 5, 129, 257, True, "jsd"),
    "up8_mcd_losses/dma-diff-two-c41": _up8_mcd(4, 2, 41, 5, 9, True, "diff", True),
    "up8_mcd_losses/dma-diff-one-c5-340items": _up8_mcd(5, 4, 5, 16, 40, False, "diff", True),
    "up8_mcd_losses/dma-jsd-two-c5": _up8_mcd(6, 1, 5, 3, 9, True, "jsd", True),
    "up8_mcd_losses/staged-diff-two-c41": _up8_mcd(7, 2, 41, 5, 9, True, "diff", False),
    "up8_mcd_losses/staged-jsd-two-c5-340items": _up8_mcd(8, 4, 5, 16, 40, True, "jsd", False),
    "label_weight_sum/293blocks": _wsum(9, 41, 600001),
    # the entropy
    "predict_labels/two-c41-260blocks": _predict(11, 1, 41, 258, 257, True, 40),
    "predict_labels_up8/c5-273blocks": _predict_up(13, 3, 5, 90, 3, True, 4),
    "predict_labels_up8/c41": _predict_up(14, 1, 41, 4, 9, True, 40),
    "predict_labels_bilinear8/c5-273blocks": _predict_up(15, 3, 5, 90, 3, False, None),
    "predict_labels_bilinear8/c41": _predict_up(16, 1, 41, 4, 9, False, 40),
    "mse_loss/269blocks": _mse(17, 1100003),
    # loss, beta
    "bce2d/u8-269blocks": _bce2d(19, 1100003, True),
    "boundary_head_bce/261blocks": _head_bce(21, 1, 129, 129, 41),
    # loss of head 1, of head 2, beta, db after backward
    "seg2bd_bce/c5-261blocks": _seg2bd(23, 1, 5, 129, 129),
    # B, U_n
    "up8_uncertain_loss/c5": _uncertain(25, 2, 5, 3, 9, 3),
    "up8_uncertain_loss/c41": _uncertain(26, 3, 41, 16, 20, 4),
    "prob_cross_entropy2d/293blocks": _prob_nll(27, 1, 5, 300, 1000),
}
# One block: the scalar is that block's tail and nothing else, so the order in which the tail combines its four wave sums reaches the
# recorded bits -- in about every second scalar, by the rounding it happens to meet; hence four seeds each.  (Behind hundreds of
# partial rows summed in fp64 and rounded to fp32 once, one unit in the last place of a few partials is invisible: the large cases
# above hold the finalizers to every row, not to an order.)
ONE_BLOCK = {
    "mcd_losses/diff-one-c5-1block": lambda seed: _mcd(seed, 1, 5, 10, 20, False, "diff"),
    "mcd_losses/symkl-two-c5-1block": lambda seed: _mcd(seed, 1, 5, 10, 20, True, "symkl"),
    "label_weight_sum/1block": lambda seed: _wsum(seed, 5, 250),
    "predict_labels/one-c5-1block": lambda seed: _predict(seed, 1, 5, 10, 20, False, None),
    "mse_loss/1block": lambda seed: _mse(seed, 1000),
    "bce2d/soft-1block": lambda seed: _bce2d(seed, 777, False),
    "boundary_head_bce/1block": lambda seed: _head_bce(seed, 1, 2, 3, 5),
    "seg2bd_bce/c41-1block": lambda seed: _seg2bd(seed, 1, 41, 2, 3),
    "prob_cross_entropy2d/1block": lambda seed: _prob_nll(seed, 1, 41, 20, 25),
}
for _k, (_name, _make) in enumerate(ONE_BLOCK.items()):
    for _s in range(4):
        CASES["%s-seed%d" % (_name, _s)] = _make(100 + 10 * _k + _s)
