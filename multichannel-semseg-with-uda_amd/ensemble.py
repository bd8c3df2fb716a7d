"""Ensembling of saved predictions -- the reference's tools/ensemble_predict_from_npy.py (the ``prob/<name>.npy`` maps that several
testers wrote, combined by mean or by maximum, arg-max to a label PNG and a palette PNG) -- as two device steps (``ops.ensemble_probs``,
``ops.label_resize_colorize``: DESIGN.md section 4.14) and what ``tools/ensemble_predict_from_npy.py`` needs around them.

``<outdir>/label/<name>.png`` holds the labels, ``<outdir>/vis/<name>.png`` their palette image (RGB), ``<outdir>/prob/<name>.npy`` the
combined map [C,H,W] (ensemble_predict_from_npy.py:71-77); with ground truth, ``<outdir>/eval_result_ensemble.json`` holds the summaries of
every member's own arg-max and of the ensemble's labels, all at the size of the PNGs, as {"members": [...], "ensemble": ...}."""
import json
import os

import numpy as np
import torch
from PIL import Image

from util import mkdir_if_not_exist, save_dic_to_json
from mcdseg import ops

METHODS = tuple(ops.ENSEMBLE_METHODS)


def default_palette(n):
    """the PASCAL-VOC colour map of ``n`` <= 256 labels, uint8 [n,3]: the bits of a label are dealt out to r, g, b in turn, from the top
    bit of each colour down -- r takes label bits 0, 3, 6 into its bits 7, 6, 5, g bits 1, 4, 7, b bits 2, 5 into its bits 7, 6"""
    if not 1 <= int(n) <= 256:
        raise ValueError("a palette holds 1..256 colours, got %r" % (n,))
    label = np.arange(int(n), dtype=np.int64)
    pal = np.zeros((int(n), 3), dtype=np.int64)
    for channel in range(3):
        for j in range(3):  # the j-th label bit of this channel -> colour bit 7 - j
            pal[:, channel] |= ((label >> (3 * j + channel)) & 1) << (7 - j)
    return pal.astype(np.uint8)


def load_palette(fn):
    """a ``{"palette": [[r,g,b], ...]}`` file, what ``util.save_colorized_lbl`` of the reference reads (util.py:135-138)"""
    with open(fn) as f:
        pal = np.array(json.load(f)["palette"])
    if pal.ndim != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= 256 or pal.min() < 0 or pal.max() > 255:
        raise ValueError("%s: \"palette\" must be 1..256 [r,g,b] rows of 0..255" % fn)
    return pal.astype(np.uint8)


class Ensemble(object):
    def __init__(self, outdir, method="averaging", n_used=None, out_shape=None, palette=None, save_prob=True, n_class=None, device=None):
        if method not in METHODS:
            raise ValueError("Ensemble: method must be one of %s, got %r" % (sorted(METHODS), method))
        self.outdir, self.method, self.n_used, self.n_class, self.device = outdir, method, n_used, n_class, device
        self.label_dir, self.vis_dir = os.path.join(outdir, "label"), os.path.join(outdir, "vis")
        self.prob_dir = os.path.join(outdir, "prob") if save_prob else None
        for d in (self.label_dir, self.vis_dir, self.prob_dir):
            if d:
                mkdir_if_not_exist(d)
        self.out_shape = None if out_shape is None else (int(out_shape[0]), int(out_shape[1]))  # (W, H)
        self.palette = None if palette is None else np.ascontiguousarray(palette, dtype=np.uint8)
        self._palette_dev = None
        self.members = self.ensemble = None

    def _dev(self, t):
        t = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
        return t.to(self.device) if self.device is not None else t

    def _colours(self, n_used):
        """the palette on the device; the default has n_used + 1 colours (the reference's 20 for its 19 classes)"""
        if self._palette_dev is None:
            if self.palette is None:
                self.palette = default_palette(min(n_used + 1, 256))
            self._palette_dev = self._dev(self.palette)
        return self._palette_dev

    def _wh(self, labels):
        return self.out_shape if self.out_shape is not None else (labels.shape[2], labels.shape[1])

    def combine(self, maps):
        """``maps``: one fp32 [B,C,H,W] per member (device tensors, or host arrays that are uploaded) ->
        (the combined map fp32 [B,C,H,W], or None when it is not saved; labels uint8 [B,OH,OW]; palette image uint8 [B,OH,OW,3])"""
        maps = [self._dev(m) for m in maps]
        n_used = maps[0].shape[1] if self.n_used is None else self.n_used
        prob, labels = ops.ensemble_probs(maps, self.method, n_used, want_prob=self.prob_dir is not None)
        labels_out, vis = ops.label_resize_colorize(labels, self._wh(labels), self._colours(n_used))
        return prob, labels_out, vis

    def member_labels(self, one_map):
        """the arg-max of one member's own map over the same classes, by the same rule, at the size of the PNGs: max(m, m) is m"""
        m = self._dev(one_map)
        n_used = m.shape[1] if self.n_used is None else self.n_used
        labels = ops.ensemble_probs([m, m], "nms", n_used, want_prob=False)[1]
        return ops.label_resize_colorize(labels, self._wh(labels), None, want_vis=False)[0]

    def update(self, member_labels_u8, labels_u8, gt_u8):
        """ground truth uint8 [B,OH,OW] at the size of the PNGs, background 255 (as in label PNGs)"""
        from eval import ConfusionMeter
        if self.ensemble is None:
            self.members = [ConfusionMeter(self.n_class, background_id=255, device=self.device) for _ in member_labels_u8]
            self.ensemble = ConfusionMeter(self.n_class, background_id=255, device=self.device)
        gt_u8 = self._dev(gt_u8)
        for meter, lab in zip(self.members, member_labels_u8):
            meter.update(self._dev(lab), gt_u8)
        self.ensemble.update(self._dev(labels_u8), gt_u8)

    def save(self, names, labels_u8, vis_u8, prob=None):
        """``names`` without extension; host arrays (or tensors, which are downloaded)"""
        lab, vis = _host(labels_u8), _host(vis_u8)
        prob = _host(prob) if (prob is not None and self.prob_dir) else None
        for k, name in enumerate(names):
            if prob is not None:
                np.save(os.path.join(self.prob_dir, name + ".npy"), prob[k])           # :29
            Image.fromarray(lab[k]).save(os.path.join(self.label_dir, name + ".png"))   # :33-35
            Image.fromarray(vis[k]).save(os.path.join(self.vis_dir, name + ".png"))  # :54-56

    def finish(self):
        """writes eval_result_ensemble.json when ground truth was seen; returns the summaries (or None)"""
        if self.ensemble is None or int(self.ensemble.hist.sum()) == 0:
            return None
        result = {"members": [m.summary() for m in self.members], "ensemble": self.ensemble.summary()}
        save_dic_to_json(result, os.path.join(self.outdir, "eval_result_ensemble.json"), verbose=False)
        print("ensemble (%s): mIoU %s -> %.2f" % (self.method, " ".join("%.2f" % m["mIoU"] for m in result["members"]),
                                                  result["ensemble"]["mIoU"]))
        return result


def _host(t):
    return t.cpu().numpy() if torch.is_tensor(t) else t
