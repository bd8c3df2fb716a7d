#!/usr/bin/env python3
"""Golden vectors for the depth image of the multitask tester: ``unnormalize`` of the reference (transform.py:285-294) applied to the
depth head's HWC float32 map (adapt_multitask_tester.py:148-155), then ``Image.resize(test_img_shape, Image.BILINEAR)``.

The reference's transform.py imports torchvision (absent here), so the one function is taken out of its source with ``ast`` and run
as it stands against the real numpy and Pillow (versions recorded in the file).  The maps are seeded float32 arrays with Cd = 3 and
Cd = 1 channels (numpy broadcasts (H,W,1) * (3,) into three channels), with values far outside [0, 1], beyond the int32 range of the
cast, NaN and +-inf.  Only data is written: tests/golden/depth_image_small.npz.

    python tests/golden/make_golden_depth_image.py [path of the reference checkout]
"""
import ast
import os
import sys
import warnings

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
SHAPES = [(40, 30), (21, 13)]  # test_img_shape (W, H): up and down from the 32 x 24 maps


def load_unnormalize():
    path = os.path.join(REF, "transform.py")
    tree = ast.parse(open(path).read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "unnormalize"]
    assert len(fn) == 1, "unnormalize not found in %s" % path
    ns = {"np": np, "Image": Image}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["unnormalize"]


def make_map(rng, cd):
    h, w = 24, 32
    x = (rng.randn(h, w, cd) * 1.5).astype(np.float32)     # the bulk: around [0,1] and across both ends of the byte
    x[rng.rand(h, w, cd) < 0.08] *= 40                      # far outside [0, 255] after scaling: wraps
    x[0, :6] = np.array([np.nan, np.inf, -np.inf, 4e7, -3.6e7, 3.6e7], np.float32)[:, None]  # NaN, inf, beyond int32 (0) and just inside it
    x[1, :4] = np.array([-2.1179, 2.2489, 1e-8, -1e-8], np.float32)[:, None]  # near the 0 / 255 edges of channel 0
    return x


def main():
    unnormalize = load_unnormalize()
    rng = np.random.RandomState(20261016)
    out = {"numpy_version": np.array(np.__version__), "pillow_version": np.array(PIL.__version__),
           "sizes": np.array(SHAPES, dtype=np.int64)}
    for cd in (3, 1):
        x = make_map(rng, cd)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # numpy warns on the invalid casts it performs
            img = unnormalize(x)
        u8 = np.asarray(img)
        assert u8.dtype == np.uint8 and u8.shape == (24, 32, 3), (u8.dtype, u8.shape)
        out["map_%dch" % cd] = x
        out["img_%dch" % cd] = u8
        for k, (ow, oh) in enumerate(SHAPES):
            out["resized%d_%dch" % (k, cd)] = np.asarray(img.resize((ow, oh), Image.BILINEAR))
        print("  Cd=%d: %d of %d bytes outside the plain [0,1] range" % (cd, int(((x < 0) | (x > 1)).sum()), x.size))
    np.savez_compressed(os.path.join(HERE, "depth_image_small.npz"), **out)
    print("depth_image_small.npz written (numpy %s, Pillow %s)" % (np.__version__, PIL.__version__))


if __name__ == "__main__":
    main()
