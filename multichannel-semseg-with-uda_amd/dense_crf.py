"""The fully connected CRF over saved logits -- the reference's tools/crf.py (softmax of ``prob/<name>.npy``, mean-field with a
Gaussian and a bilateral Potts term, arg-max to PNG) -- as one device step (``ops.dense_crf``: exact pairwise sums, DESIGN.md
section 4.12) and what ``tools/dense_crf.py`` needs around it.

``<outdir>/<name>.png`` holds the labels, ``<prob_outdir>/<name>.npy`` the refined probabilities [C,H,W]; with ground truth,
``eval_result_crf.json`` beside ``outdir`` holds the summaries of the arg-max of the logits and of the CRF's labels, both at the
size of the logits, as {"before": ..., "after": ...}."""
import os

import numpy as np
import torch
from PIL import Image

from eval import ConfusionMeter
from util import mkdir_if_not_exist, save_dic_to_json
from mcdseg import ops

DEFAULTS = dict(ops.CRF_DEFAULTS)  # tools/crf.py:14-21


class DenseCRF(object):
    def __init__(self, outdir, prob_outdir=None, outimg_shape=None, n_used=None, n_class=None, device=None, **params):
        unknown = set(params) - set(DEFAULTS)
        if unknown:
            raise TypeError("DenseCRF: unknown parameters %s" % sorted(unknown))
        self.outdir, self.prob_outdir = outdir, prob_outdir
        self.base_outdir = os.path.split(os.path.normpath(outdir))[0]
        mkdir_if_not_exist(outdir)
        if prob_outdir:
            mkdir_if_not_exist(prob_outdir)
        self.outimg_shape = None if outimg_shape is None else (int(outimg_shape[0]), int(outimg_shape[1]))  # (W, H)
        self.n_used, self.n_class, self.device = n_used, n_class, device
        self.params = dict(DEFAULTS, **params)
        self.before = self.after = None

    def _dev(self, t):
        t = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
        return t.to(self.device) if self.device is not None else t

    def refine(self, logits, rgb=None):
        """fp32 logits [B,C,H,W] and uint8 RGB [B,H,W,3] or None (device tensors, or host arrays that are uploaded) ->
        (Q fp32 [B,C,H,W], labels uint8 [B,H,W])"""
        return ops.dense_crf(self._dev(logits), None if rgb is None else self._dev(rgb), c_used=self.n_used, **self.params)

    def plain_labels(self, logits):
        """the arg-max of softmax(logits) over the same classes, by the same tie rule: what the CRF started from"""
        return ops.dense_crf(self._dev(logits), None, c_used=self.n_used, **dict(self.params, n_iters=0))[1]

    def update(self, labels_u8, refined_u8, gt_u8):
        """ground truth uint8 [B,H,W] at the size of the logits, background 255 (as in label PNGs)"""
        if self.before is None:
            self.before = ConfusionMeter(self.n_class, background_id=255, device=self.device)
            self.after = ConfusionMeter(self.n_class, background_id=255, device=self.device)
        gt_u8 = self._dev(gt_u8)
        self.before.update(self._dev(labels_u8), gt_u8)
        self.after.update(self._dev(refined_u8), gt_u8)

    def save(self, labels_u8, names, q=None):
        """``names`` without extension; the PNG is resized NEAREST to ``outimg_shape`` (tools/crf.py:120-123) when that is set"""
        arr = labels_u8.cpu().numpy()
        probs = q.cpu().numpy() if (q is not None and self.prob_outdir) else None
        for k, name in enumerate(names):
            img = Image.fromarray(arr[k])
            if self.outimg_shape is not None:
                img = img.resize(self.outimg_shape, Image.NEAREST)
            img.save(os.path.join(self.outdir, name + ".png"))
            if probs is not None:
                np.save(os.path.join(self.prob_outdir, name + ".npy"), probs[k])  # crf.py:115-118, [C,H,W]

    def finish(self):
        """writes eval_result_crf.json when ground truth was seen; returns the summaries (or None)"""
        if self.before is None or int(self.before.hist.sum()) == 0:
            return None
        result = {"before": self.before.summary(), "after": self.after.summary()}
        save_dic_to_json(result, os.path.join(self.base_outdir, "eval_result_crf.json"), verbose=False)
        print("dense CRF: mIoU %.2f -> %.2f  pixAcc %.2f -> %.2f" % (result["before"]["mIoU"], result["after"]["mIoU"],
                                                                     result["before"]["pixAcc"], result["after"]["pixAcc"]))
        return result
