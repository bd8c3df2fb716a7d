#!/usr/bin/env python3
"""MCD inference -- the reference's ``adapt_tester.py`` (:17-146): load a trained checkpoint, eval-mode G -> F1
(optionally averaged with F2), argmax over the non-background classes, write uint8 label PNGs (resized NEAREST to the
test shape), report the mean prediction entropy.

On the HIP path eval-mode BatchNorm is folded into the convolution epilogue (``mcdseg_conv_fprop_affine``) and the
argmax / entropy tail is one kernel (``mcdseg_predict_labels``).  ``--vis`` adds ``vis/<name>``, the label PNG with a palette
(``--palette_json``, or the PASCAL-VOC colours); the ``eval.py`` run of the reference is outside this build.

    python adapt_tester.py nyu train_output/.../pth/MCD-normal-drn_d_38-1.pth.tar --synthetic
"""
import os

import torch
from PIL import Image

import tester_common
from argmyparse import add_additional_params_to_args, get_da_mcd_testing_parser
from models.model_util import get_models
from util import mkdir_if_not_exist
from mcdseg import ops


def main(argv=None, mfnet=False):
    """``mfnet=True`` is the two-encoder variant (adapt_mfnet_tester.py): checkpoints hold ``g_3ch_state_dict`` /
    ``g_1ch_state_dict``, the classifier takes both feature maps and only F1 is evaluated (:102-105)."""
    args = add_additional_params_to_args(get_da_mcd_testing_parser().parse_args(argv))
    t = tester_common.start(args, strip_tar=mfnet)
    train_args, checkpoint = t.train_args, t.checkpoint

    method = getattr(train_args, "method", "MCD")
    if mfnet:  # the trainer stores the full "MFNet-<fusion>" name in method_detail (adapt_mfnet_trainer.py:29)
        method = train_args.method_detail if "MFNet" in train_args.method_detail else method + "-" + train_args.method_detail
    if method == "DANN":  # dann_trainer.py's G and F are MCD's G and F1; its checkpoint holds no F2 (and a D, which inference does not use)
        method = "MCD"
    *encoders, F1, F2 = get_models(net_name=train_args.net, res=train_args.res, input_ch=train_args.input_ch, n_class=train_args.n_class,
                                   method=method, is_data_parallel=getattr(train_args, "is_data_parallel", False))
    for G, key in zip(encoders, ("g_3ch_state_dict", "g_1ch_state_dict") if mfnet else ("g_state_dict",)):
        G.load_state_dict(checkpoint[key])
    F1.load_state_dict(checkpoint["f1_state_dict"])
    if args.use_f2:
        F2.load_state_dict(checkpoint["f2_state_dict"])
    for m in encoders + [F1, F2]:
        m.eval()
        m.to(t.dev)

    label_outdir = os.path.join(t.base_outdir, "label")
    mkdir_if_not_exist(label_outdir)
    total_ent, batches = 0.0, 0
    save_vis = tester_common.vis_saver(args, t.base_outdir, t.n_used)
    with torch.no_grad():
        for imgs, gts, paths in t.loader:
            imgs = imgs.to(t.dev, non_blocking=True)
            if mfnet:
                out1 = F1(encoders[0](imgs[:, :3, :, :]), encoders[1](imgs[:, 3:, :, :]))
                out2 = None  # adapt_mfnet_tester.py:105 evaluates F1 alone, with or without --use_f2
            else:
                feature = encoders[0](imgs)
                out1 = F1(feature)
                out2 = F2(feature) if args.use_f2 else None
            labels, ent = ops.predict_labels(out1, out2, t.n_used)
            total_ent += float(ent)  # the mean over batches, as the reference's (it runs one image per batch)
            batches += 1
            tester_common.update_meter(t.meter, labels, gts, train_args.n_class)
            if args.saves_prob:
                tester_common.save_probs(t.base_outdir, paths, out1 if out2 is None else (out1 + out2) / 2)
            lab = labels.cpu().numpy()
            for k, path in enumerate(paths):
                img = Image.fromarray(lab[k]).resize(t.test_img_shape, Image.NEAREST)
                img.save(os.path.join(label_outdir, os.path.basename(path)))
                if save_vis is not None:
                    save_vis(img, os.path.basename(path))
    return label_outdir, tester_common.finish(t.base_outdir, total_ent, batches, t.meter)


if __name__ == "__main__":
    main()
