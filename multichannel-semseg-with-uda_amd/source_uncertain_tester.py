#!/usr/bin/env python3
"""Inference with the aleatoric-uncertainty model -- the reference's ``source_uncertain_tester.py`` (:27-174): load a
``source_uncertain_trainer`` checkpoint into ``get_full_uncertain_model`` (no ``module.`` prefix), run it in eval mode (no dropout)
and write per image

    label/<name>                        argmax over the non-background classes, resized NEAREST to the test shape
    prob/<name>.npy                     the full-resolution logits (only with ---saves_prob)
    aleatoric_uncertainty/<name>.png    sum over the classes of relu(up_std(scores)), resized (bilinear) to the test shape, then
                                        matplotlib's ``jet`` over the resized map's own range (what ``plt.imshow(.., cmap="jet")`` normalises to)
    aleatoric_uncertainty/<name>.npy    that map at full resolution, fp32 (only with ---saves_prob)
    vis/<name>                          the label PNG with a palette, mode P (only with --vis; ``--palette_json``, or the PASCAL-VOC colours)

plus ``ave_ent_<x>.txt`` and, when the data carry ground truth, ``eval_result.json``.  The reference's literal
``plt.imshow(std[0])`` (:162-166) takes the [C,H,W] array only for C = 3 or 4; the channel sum is what its own commented-out lines
(:163, models/dilated_fcn.py:160) were after.  Labels and entropy come from the fused up-sampling tail (``ops.predict_labels_up8``) and
the uncertainty map from ``ops.up8_std_sum``: neither C-channel full-resolution tensor is formed without ---saves_prob.

    python source_uncertain_tester.py nyu train_output/suncg-train_only_6ch_uncertain/pth/normal-drn_d_38-40.pth.tar --synthetic
"""
import os

import numpy as np
import torch
from PIL import Image

import source_tester
import tester_common
from argmyparse import add_additional_params_to_args
from loss import CrossEntropyLoss2d
from models.model_util import get_full_uncertain_model
from util import get_class_weight_from_file, mkdir_if_not_exist
from mcdseg import ops

get_parser = source_tester.get_parser  # the reference's flags are source_tester.py's (:27-36), three-dash ---saves_prob included

# matplotlib's "jet" (its _jet_data segments: piecewise linear in each channel), so that the tester needs no plotting library
_JET = {"r": ((0.0, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.0, 0.5)),
        "g": ((0.0, 0.0), (0.125, 0.0), (0.375, 1.0), (0.64, 1.0), (0.91, 0.0), (1.0, 0.0)),
        "b": ((0.0, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.0, 0.0))}


def jet_u8(a):
    """[H,W] array -> uint8 [H,W,3]: the range [min, max] of ``a`` through the jet colour map (a constant image maps to its low end)"""
    a = np.asarray(a, dtype=np.float64)
    lo, hi = float(a.min()), float(a.max())
    x = (a - lo) / (hi - lo) if hi > lo else np.zeros_like(a)
    rgb = [np.interp(x, [p[0] for p in _JET[ch]], [p[1] for p in _JET[ch]]) for ch in "rgb"]
    return np.uint8(np.clip(np.stack(rgb, axis=-1), 0.0, 1.0) * 255.0 + 0.5)


def main(argv=None):
    args = add_additional_params_to_args(get_parser().parse_args(argv))
    dev = tester_common.device()
    checkpoint = tester_common.load(args)
    if "args" not in checkpoint:
        raise SystemExit("%s holds no training arguments ('args'): the network and class count cannot be known" % args.trained_checkpoint)
    train_args = checkpoint["args"]

    os.environ["MCDSEG_PRETRAINED"] = "0"  # weights come from the checkpoint
    weight = get_class_weight_from_file(n_class=train_args.n_class, weight_filename=train_args.loss_weights_file,
                                        add_bg_loss=train_args.add_bg_loss)
    model = get_full_uncertain_model(net=train_args.net, res=train_args.res, n_class=train_args.n_class, input_ch=train_args.input_ch,
                                     n_dropout=getattr(train_args, "n_dropout", 10), criterion=CrossEntropyLoss2d(weight),
                                     is_data_parallel=False)
    model.load_state_dict(checkpoint["state_dict"] if "state_dict" in checkpoint else checkpoint)
    args.train_img_shape = train_args.train_img_shape
    base_outdir = tester_common.output_dir(args)
    tester_common.write_params(args, base_outdir)

    test_img_shape = tuple(int(x) for x in args.test_img_shape)
    train_img_shape = args.train_img_shape
    if getattr(train_args, "crop_size", -1) > 0:
        train_img_shape = test_img_shape
        print("train_img_shape was set to the same as test_img_shape")
    loader = tester_common.make_loader(args, train_args, train_img_shape)

    model.to(dev)
    model.eval()
    n_used = train_args.n_class if getattr(train_args, "add_bg_loss", False) else train_args.n_class - 1

    label_root = os.path.join(base_outdir, "label")
    uncertainty_root = os.path.join(base_outdir, "aleatoric_uncertainty")
    mkdir_if_not_exist(label_root)
    mkdir_if_not_exist(uncertainty_root)
    total_ent, images = 0.0, 0
    meter = tester_common.new_meter(train_args, dev)
    save_vis = tester_common.vis_saver(args, base_outdir, n_used)
    with torch.no_grad():
        for imgs, gts, paths in loader:
            imgs = imgs.to(dev, non_blocking=True)
            scores = model.seg(model.base(imgs))  # UncertainDRNSeg.forward up to its up-samplers; dropout is off in eval mode
            labels, ent = ops.predict_labels_up8(scores, model.up.weight, n_used)
            total_ent += float(ent) * len(paths)  # the reference's mean over images (it runs one image per batch)
            images += len(paths)
            tester_common.update_meter(meter, labels, gts, train_args.n_class)
            if args.saves_prob:
                tester_common.save_probs(base_outdir, paths, ops.up8(scores, model.up.weight))
            lab = ops.resize_u8(labels, test_img_shape, nearest=True).cpu().numpy()
            std = ops.up8_std_sum(scores, model.up_std.weight).cpu().numpy()
            for k, path in enumerate(paths):
                name = os.path.basename(path)
                Image.fromarray(lab[k]).save(os.path.join(label_root, name))
                if save_vis is not None:
                    save_vis(lab[k], name)
                resized = np.asarray(Image.fromarray(std[k], mode="F").resize(test_img_shape, Image.BILINEAR))  # the scalar map first,
                colour = Image.fromarray(jet_u8(resized))                                                       # then its colours
                colour.save(os.path.join(uncertainty_root, os.path.splitext(name)[0] + ".png"))
                if args.saves_prob:
                    np.save(os.path.join(uncertainty_root, os.path.splitext(name)[0] + ".npy"), std[k])
    return label_root, uncertainty_root, tester_common.finish(base_outdir, total_ent, images, meter)


if __name__ == "__main__":
    main()
