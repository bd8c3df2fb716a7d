#!/usr/bin/env python3
"""Multitask MCD inference -- the reference's ``adapt_multitask_tester.py`` (:1-166): load an ``adapt_multitask_trainer``
checkpoint (``enc_state_dict`` / ``dec_state_dict``), run the RGB encoder on ``imgs[:, :3]`` and the decoder in eval mode, and
write per image

    label/<name>       argmax of pred_semseg1 over the non-background classes, resized NEAREST to the test shape
    depth/<name>       the depth head as an RGB image (transform.unnormalize), resized BILINEAR to the test shape
    prob/<name>.npy    pred_semseg1 at full resolution (only with --saves_prob)

plus ``ave_ent_<x>.txt`` (mean entropy of pred_semseg1) and, when the data carry ground truth, ``eval_result.json``.

The decoder's heads run at 1/8 resolution; the x8 bilinear up-sampling is fused into the argmax / entropy kernel
(``mcdseg_predict_labels_up8``) and into the depth-image kernel (``mcdseg_depth_image_u8``), so neither full-resolution tensor is
stored.  pred_semseg2 is not evaluated: the reference computes it and drops it (its F2 average is commented out, :118-121), so
``--use_f2`` only renames the output directory, as there.  ``--vis`` adds ``vis/<name>``, the label PNG with a palette (``--palette_json``,
or the PASCAL-VOC colours); the ``eval.py`` run of the reference is outside this build.

    python adapt_multitask_tester.py nyu train_output/...MCDmultitask/pth/MCD-normal-drn_d_38-40.pth.tar --synthetic
"""
import os

import torch
from PIL import Image

import tester_common
from argmyparse import add_additional_params_to_args, get_da_mcd_testing_parser
from models.model_util import get_multitask_models
from trainer_common import criteria
from util import mkdir_if_not_exist
from mcdseg import ops


def main(argv=None):
    args = add_additional_params_to_args(get_da_mcd_testing_parser().parse_args(argv))
    t = tester_common.start(args)
    train_args = t.train_args

    # the criteria are not used here, but the decoder holds the class weights as a buffer (semseg_criterion.nll_loss.weight) and the
    # checkpoint carries it, so they are built as the trainer built them (adapt_multitask_tester.py:73-86)
    criterion, criterion_d = criteria(train_args)
    model_enc, model_dec = get_multitask_models(net_name=train_args.net, input_ch=train_args.input_ch, n_class=train_args.n_class,
                                                is_data_parallel=getattr(train_args, "is_data_parallel", False),
                                                semseg_criterion=criterion, discrepancy_criterion=criterion_d)
    model_enc.load_state_dict(t.checkpoint["enc_state_dict"])
    model_dec.load_state_dict(t.checkpoint["dec_state_dict"])
    dec = tester_common.unwrap(model_dec)
    print(dec.get_task_weights())
    for m in (model_enc, model_dec):
        m.eval()
        m.to(t.dev)

    label_outdir = os.path.join(t.base_outdir, "label")
    depth_outdir = os.path.join(t.base_outdir, "depth")
    mkdir_if_not_exist(label_outdir)
    mkdir_if_not_exist(depth_outdir)
    total_ent, images = 0.0, 0
    save_vis = tester_common.vis_saver(args, t.base_outdir, t.n_used)
    with torch.no_grad():
        for imgs, gts, paths in t.loader:
            imgs = imgs.to(t.dev, non_blocking=True)
            feature = model_enc(imgs[:, :3, :, :].contiguous())
            s1 = dec.semsegcls_dec1(feature)  # pred_semseg1 before the x8 up-sampling
            dep = dec.deprgr_dec(feature)     # pred_depth before the x8 up-sampling
            labels, ent = ops.predict_labels_bilinear8(s1, t.n_used)
            total_ent += float(ent) * len(paths)  # the reference's mean over images (it runs one image per batch)
            images += len(paths)
            tester_common.update_meter(t.meter, labels, gts, train_args.n_class)
            if args.saves_prob:
                tester_common.save_probs(t.base_outdir, paths, ops.bilinear8(s1))
            lab = ops.resize_u8(labels, t.test_img_shape, nearest=True).cpu().numpy()
            depth = ops.resize_u8(ops.depth_image_u8(dep), t.test_img_shape).cpu().numpy()
            for k, path in enumerate(paths):
                name = os.path.basename(path)
                Image.fromarray(lab[k]).save(os.path.join(label_outdir, name))
                if save_vis is not None:
                    save_vis(lab[k], name)
                Image.fromarray(depth[k]).save(os.path.join(depth_outdir, name))
    return label_outdir, depth_outdir, tester_common.finish(t.base_outdir, total_ent, images, t.meter)


if __name__ == "__main__":
    main()
