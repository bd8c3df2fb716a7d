"""The dense CRF of DESIGN.md section 4.12 in numpy, written from the definition: dense O(N^2), the whole kernel matrix of each term in
memory, every sum over ALL pixels (no window, no lattice).  ``dtype`` is the precision of every operation: float64 is the truth the
kernels are held to, float32 the unit -- "the reference's own fp32 distance from the truth".

    U = -log_softmax(z);  Q^0 = softmax(-U)
    k(i,j) = exp(-0.5 |f_i - f_j|^2), j = i included;  n_i = 1 / sqrt(sum_j k(i,j) + 1e-20);  M_i = n_i sum_j k(i,j) n_j Q_j
    Q^{t+1} = softmax(-U + w_g M_g(Q^t) + w_b M_b(Q^t));  the bilateral term only with an image
"""
import numpy as np

DEFAULTS = {"n_iters": 10, "sxy_gaussian": (1, 1), "compat_gaussian": 4, "sxy_bilateral": (49, 49), "compat_bilateral": 5,
            "srgb_bilateral": (13, 13, 13)}


def softmax(x, axis):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def log_softmax(x, axis):
    s = x - x.max(axis=axis, keepdims=True)
    return s - np.log(np.exp(s).sum(axis=axis, keepdims=True))


def kernel_matrix(f):
    """f [N, D] -> k [N, N] from the feature DIFFERENCES, one dimension at a time"""
    d2 = np.zeros((f.shape[0], f.shape[0]), f.dtype)
    for d in range(f.shape[1]):
        diff = f[:, None, d] - f[None, :, d]
        d2 += diff * diff
    return np.exp(f.dtype.type(-0.5) * d2)


def features(h, w, sxy, rgb=None, srgb=None, dtype=np.float64):
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    cols = [xs.reshape(-1).astype(dtype) / dtype(sxy[0]), ys.reshape(-1).astype(dtype) / dtype(sxy[1])]
    if rgb is not None:
        cols += [rgb.reshape(-1, 3)[:, k].astype(dtype) / dtype(srgb[k]) for k in range(3)]
    return np.stack(cols, 1)


def dense_crf(z, rgb=None, n_iters=10, sxy_gaussian=(1, 1), compat_gaussian=4, sxy_bilateral=(49, 49), compat_bilateral=5,
              srgb_bilateral=(13, 13, 13), dtype=np.float64, keep=()):
    """one image: logits z [C,H,W], rgb uint8 [H,W,3] or None -> Q^{n_iters} [C,H,W] in ``dtype``; with ``keep`` (iteration numbers) a
    dict {t: Q^t} of those iterations instead"""
    dtype = np.dtype(dtype).type
    c, h, w = z.shape
    n = h * w
    u = -log_softmax(z.reshape(c, n).T.astype(dtype), 1)
    terms = [(kernel_matrix(features(h, w, sxy_gaussian, dtype=dtype)), dtype(compat_gaussian))]
    if rgb is not None:
        terms.append((kernel_matrix(features(h, w, sxy_bilateral, rgb, srgb_bilateral, dtype)), dtype(compat_bilateral)))
    norms = [dtype(1) / np.sqrt(k.sum(1) + dtype(1e-20)) for k, _ in terms]
    q = softmax(-u, 1)
    kept = {0: q} if 0 in keep else {}
    for t in range(1, max([n_iters] + list(keep)) + 1):
        x = -u
        for (k, wt), nrm in zip(terms, norms):
            x = x + wt * (nrm[:, None] * (k @ (nrm[:, None] * q)))
        q = softmax(x, 1)
        if t in keep:
            kept[t] = q
    assert q.dtype == np.dtype(dtype)
    if keep:
        return {t: v.T.reshape(c, h, w) for t, v in kept.items()}
    return q.T.reshape(c, h, w)


def labels_of(q, c_used=None):
    """arg-max over the first c_used classes, first maximum on a tie (numpy's rule), uint8"""
    return np.argmax(q[:c_used], 0).astype(np.uint8)


def margin_of(q, c_used=None):
    """the distance of the largest from the second largest of the first c_used classes per pixel (inf with one class)"""
    q = q[:c_used]
    if q.shape[0] < 2:
        return np.full(q.shape[1:], np.inf)
    top = np.sort(q, 0)
    return top[-1] - top[-2]


def make_case(b, h, w, c, seed):
    """the inputs of the parity cases: label blobs of 4 x 4, a colour per label plus N(0, 12) noise, logits N(0, 1.5) plus 1.5 on the
    blob's class -> (logits fp32 [B,C,H,W], rgb uint8 [B,H,W,3])"""
    rng = np.random.RandomState(seed)
    palette = rng.randint(0, 256, size=(c, 3)).astype(np.float64)
    z = np.empty((b, c, h, w), np.float32)
    rgb = np.empty((b, h, w, 3), np.uint8)
    for k in range(b):
        blobs = rng.randint(0, c, size=((h + 3) // 4, (w + 3) // 4))
        lab = np.repeat(np.repeat(blobs, 4, 0), 4, 1)[:h, :w]
        rgb[k] = np.clip(np.rint(palette[lab] + rng.normal(0, 12, size=(h, w, 3))), 0, 255).astype(np.uint8)
        zz = rng.normal(0, 1.5, size=(c, h, w))
        zz[lab, np.arange(h)[:, None], np.arange(w)[None, :]] += 1.5
        z[k] = zz.astype(np.float32)
    return z, rgb
