"""Refinement of label maps by predicted boundaries -- the reference's "Postprocess using Boundary Detection output"
(sample_scripts/refine_seg_by_boundary.sh:15-17: tools/binalize_boundary.py, MATLAB's bwboundaries through tools/apply_bwboundary.m,
tools/refine_seg_by_bwboundary.py) -- as one device step (``ops.refine_labels_by_boundary``), and what its two users share: the
segbd / triple testers under ``--refine_by_boundary`` and ``tools/refine_seg_by_boundary.py``.

``refined_label/<name>`` is written next to ``label/``; with ground truth, ``eval_result_refined.json`` holds the summaries of the
unrefined and the refined label maps at the test shape as {"before": ..., "after": ...}."""
import os

import numpy as np
import torch
from PIL import Image

from eval import ConfusionMeter
from util import mkdir_if_not_exist, save_dic_to_json
from mcdseg import ops

DEFAULTS = {"thre": 50, "min_thre": 500, "max_thre": 79333}  # binalize_boundary.py:45, refine_seg_by_bwboundary.py:62-64 (425 * 560 / 3)


class BoundaryRefiner(object):
    def __init__(self, base_outdir, thre=DEFAULTS["thre"], min_thre=DEFAULTS["min_thre"], max_thre=DEFAULTS["max_thre"], n_class=None,
                 device=None):
        self.base_outdir, self.outdir = base_outdir, os.path.join(base_outdir, "refined_label")
        mkdir_if_not_exist(self.outdir)
        self.thre, self.min_thre, self.max_thre = int(thre), int(min_thre), int(max_thre)
        self.n_class, self.device = n_class, device
        self.before = self.after = None

    def refine(self, labels_u8, boundary_u8):
        """uint8 [N,H,W] label maps and boundary images (device tensors, or host arrays that are uploaded) -> refined uint8 [N,H,W]"""
        labels_u8, boundary_u8 = self._dev(labels_u8), self._dev(boundary_u8)
        return ops.refine_labels_by_boundary(labels_u8, boundary_u8, self.thre, self.min_thre, self.max_thre)

    def _dev(self, t):
        t = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
        return t.to(self.device) if self.device is not None else t

    def update(self, labels_u8, refined_u8, gt_u8):
        """ground truth uint8 [N,H,W] at the shape of the label maps, background 255 (as in label PNGs)"""
        if self.before is None:
            self.before = ConfusionMeter(self.n_class, background_id=255, device=self.device)
            self.after = ConfusionMeter(self.n_class, background_id=255, device=self.device)
        gt_u8 = self._dev(gt_u8)
        self.before.update(self._dev(labels_u8), gt_u8)
        self.after.update(refined_u8, gt_u8)

    def save(self, refined_u8, names):
        arr = refined_u8.cpu().numpy()
        for k, name in enumerate(names):
            Image.fromarray(arr[k]).save(os.path.join(self.outdir, name))

    def finish(self):
        """writes eval_result_refined.json when ground truth was seen; returns the summaries (or None)"""
        if self.before is None or int(self.before.hist.sum()) == 0:
            return None
        result = {"before": self.before.summary(), "after": self.after.summary()}
        save_dic_to_json(result, os.path.join(self.base_outdir, "eval_result_refined.json"), verbose=False)
        print("refined by boundary: mIoU %.2f -> %.2f  pixAcc %.2f -> %.2f" % (result["before"]["mIoU"], result["after"]["mIoU"],
                                                                              result["before"]["pixAcc"], result["after"]["pixAcc"]))
        return result


def tester_ground_truth(gts, labels, n_class, test_img_shape):
    """the testers' ground truth (int64 at the training shape, background n_class-1) as ``update_meter`` maps it (n_class-1 -> 255),
    as uint8 resized NEAREST to the test shape; None when the batch carries none"""
    if not (torch.is_tensor(gts) and gts.dim() == 3 and tuple(gts.shape) == tuple(labels.shape)):
        return None
    gts = gts.to(labels.device)
    gt_u8 = torch.where(gts == n_class - 1, torch.full_like(gts, 255), gts).to(torch.uint8)
    return ops.resize_u8(gt_u8, test_img_shape, nearest=True)
