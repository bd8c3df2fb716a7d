"""Edge maps of RGB images -- the reference's tools/edge_detect.py:33-53 (OpenCV's Laplacian, Canny and Sobel of the luma plane), whose
``edges/canny`` its post-processing recipe refines label maps by (sample_scripts/refine_seg_by_boundary.sh:6) -- as device steps
(``ops.edge_maps``), and what ``tools/edge_detect.py`` and other callers share."""
import os

import numpy as np
import torch
from PIL import Image

from util import mkdir_if_not_exist
from mcdseg import ops

KINDS = ("laplacian", "canny", "sobel")                  # edge_detect.py:21-23: the three directories under edges/
DEFAULTS = {"min_canny_thre": 100, "max_canny_thre": 200}  # edge_detect.py:59-60


def check_kinds(kinds):
    kinds = tuple(kinds)
    unknown = [k for k in kinds if k not in KINDS]
    if unknown or not kinds:
        raise ValueError("edge kinds must be some of %s, got %s" % (", ".join(KINDS), ", ".join(map(str, kinds)) or "none"))
    return tuple(k for k in KINDS if k in kinds)


def read_rgb(path):
    """uint8 [H,W,3], R, G, B: ``Image.open(path).convert("RGB")``, the colour decode ``cv2.imread`` gives for a lossless file (in B, G, R
    order there).  An image deeper than 8 bits per channel is refused: ``convert`` would clip or rescale it, ``cv2.imread`` would not"""
    img = Image.open(path)
    if img.mode.startswith(("I", "F")):
        raise ValueError("%s holds a %s image: deeper than 8 bits per channel" % (path, img.mode))
    arr = np.array(img.convert("RGB"))
    if arr.ndim != 3 or arr.shape[2] != 3 or arr.dtype != np.uint8:
        raise ValueError("%s does not decode to an 8-bit RGB image" % path)
    return arr


class EdgeDetector(object):
    def __init__(self, low=DEFAULTS["min_canny_thre"], high=DEFAULTS["max_canny_thre"], kinds=KINDS, device=None):
        self.low, self.high, self.kinds, self.device = int(low), int(high), check_kinds(kinds), device

    def detect(self, rgb_u8):
        """uint8 [N,H,W,3] (a device tensor, or a host array that is uploaded) -> {kind: uint8 [N,H,W] device tensor}"""
        t = rgb_u8 if torch.is_tensor(rgb_u8) else torch.from_numpy(np.ascontiguousarray(rgb_u8))
        if self.device is not None:
            t = t.to(self.device)
        return ops.edge_maps(t, self.low, self.high, self.kinds)

    def save(self, maps, stems, edge_dir):
        """writes ``edge_dir/<kind>/<stem>.png`` for every kind and image of ``maps``"""
        for kind, t in maps.items():
            mkdir_if_not_exist(os.path.join(edge_dir, kind))
            arr = t.cpu().numpy()
            for k, stem in enumerate(stems):
                Image.fromarray(arr[k]).save(os.path.join(edge_dir, kind, stem + ".png"))


def batches(paths, batch_size):
    """[(stems, uint8 [n,H,W,3])] over the files in order: runs of at most ``batch_size`` images of equal size"""
    stems, imgs = [], []
    for path in paths:
        rgb = read_rgb(path)
        if imgs and (len(imgs) >= batch_size or imgs[0].shape != rgb.shape):
            yield stems, np.stack(imgs)
            stems, imgs = [], []
        stems.append(os.path.splitext(os.path.basename(path))[0])
        imgs.append(rgb)
    if imgs:
        yield stems, np.stack(imgs)
