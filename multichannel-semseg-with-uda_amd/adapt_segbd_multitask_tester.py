#!/usr/bin/env python3
"""Segmentation + boundary multitask MCD inference -- the reference's ``adapt_segbd_multitask_tester.py`` (:1-176): load an
``adapt_segbd_multitask_trainer`` checkpoint (``enc_state_dict`` / ``dec_state_dict``), run the stage-tap RGB encoder on
``imgs[:, :3]`` and the decoder in eval mode, and write per image

    label/<name>       argmax of pred_semseg1 over the non-background classes, resized NEAREST to the test shape
    boundary/<name>    np.uint8(pred_boundary * 255) (numpy's own cast, on the host), resized BILINEAR to the test shape
    prob/<name>.npy    pred_semseg1 at full resolution (only with --saves_prob)

plus ``ave_ent_<x>.txt`` (mean entropy of pred_semseg1) and, when the data carry ground truth, ``eval_result.json``.

With ``--refine_by_boundary`` the reference's "Postprocess using Boundary Detection output" (sample_scripts/refine_seg_by_boundary.sh)
runs on the device while the batch is still there: ``refined_label/<name>`` = the label map with every region the boundary image
encloses (``--boundary_thre``, ``--min_thre``, ``--max_thre``) set to its majority class, and ``eval_result_refined.json``
({"before", "after"}, both at the test shape) when the data carry ground truth.

The segmentation heads run at 1/8 resolution; the x8 bilinear up-sampling is fused into the argmax / entropy kernel
(``mcdseg_predict_labels_up8``); the boundary map is one pass of ``mcdseg_boundary_head_fwd``.  pred_semseg2 is not evaluated: the reference computes it and drops it (its F2 average is commented out, :122-125), so
``--use_f2`` only renames the output directory, as there.  ``--vis`` adds ``vis/<name>``, the label PNG with a palette (``--palette_json``,
or the PASCAL-VOC colours); the ``eval.py`` run of the reference is outside this build, as in the other testers.

    python adapt_segbd_multitask_tester.py nyu train_output/...MCD_segbd_multitask/pth/MCD-normal-drn_d_38-40.pth.tar --synthetic
"""
import os

import numpy as np
import torch
from PIL import Image

import boundary_refine
import tester_common
from argmyparse import add_additional_params_to_args, get_da_mcd_testing_parser
from models.model_util import get_segbd_multitask_models
from trainer_common import criteria
from util import mkdir_if_not_exist
from mcdseg import ops


def get_parser():
    parser = get_da_mcd_testing_parser()
    g = parser.add_argument_group("refinement by the predicted boundaries (sample_scripts/refine_seg_by_boundary.sh)")
    g.add_argument("--refine_by_boundary", action="store_true", help="also write refined_label/ (and eval_result_refined.json)")
    g.add_argument("--boundary_thre", type=int, default=boundary_refine.DEFAULTS["thre"], help="threshold to binalize. Set from 0 to 255")
    g.add_argument("--min_thre", type=int, default=boundary_refine.DEFAULTS["min_thre"], help="the minimum number of pixel in a region")
    g.add_argument("--max_thre", type=int, default=boundary_refine.DEFAULTS["max_thre"], help="the maximum number of pixel in a region")
    return parser


def main(argv=None):
    args = add_additional_params_to_args(get_parser().parse_args(argv))
    refine = args.refine_by_boundary
    if not refine:  # param.json of a run without the step stays what it was
        for key in ("refine_by_boundary", "boundary_thre", "min_thre", "max_thre"):
            delattr(args, key)
    t = tester_common.start(args)
    train_args = t.train_args

    # the criteria are not used here, but the decoder holds the class weights as a buffer (semseg_criterion.nll_loss.weight) and the
    # checkpoint carries it, so they are built as the trainer built them (adapt_segbd_multitask_tester.py:76-93)
    criterion, criterion_d = criteria(train_args)
    model_enc, model_dec = get_segbd_multitask_models(
        net_name=train_args.net, input_ch=train_args.input_ch, n_class=train_args.n_class,
        is_data_parallel=getattr(train_args, "is_data_parallel", False), semseg_criterion=criterion, discrepancy_criterion=criterion_d,
        semseg_shortcut=getattr(train_args, "semseg_shortcut", False), depth_shortcut=getattr(train_args, "depth_shortcut", False),
        add_pred_seg_boundary_loss=getattr(train_args, "add_pred_seg_boundary_loss", False),
        use_seg2bd_conv=getattr(train_args, "use_seg2bd_conv", False))
    model_enc.load_state_dict(t.checkpoint["enc_state_dict"])
    model_dec.load_state_dict(t.checkpoint["dec_state_dict"])
    enc, dec = tester_common.unwrap(model_enc), tester_common.unwrap(model_dec)
    print(dec.get_task_weights())
    for m in (model_enc, model_dec):
        m.eval()
        m.to(t.dev)

    label_outdir = os.path.join(t.base_outdir, "label")
    boundary_outdir = os.path.join(t.base_outdir, "boundary")
    mkdir_if_not_exist(label_outdir)
    mkdir_if_not_exist(boundary_outdir)
    refiner = boundary_refine.BoundaryRefiner(t.base_outdir, args.boundary_thre, args.min_thre, args.max_thre, train_args.n_class,
                                              t.dev) if refine else None
    total_ent, images = 0.0, 0
    save_vis = tester_common.vis_saver(args, t.base_outdir, t.n_used)
    with torch.no_grad():
        for imgs, gts, paths in t.loader:
            imgs = imgs.to(t.dev, non_blocking=True)
            feature = enc(imgs[:, :3, :, :].contiguous())
            s1 = dec.semsegcls_dec1(feature["h8"])  # pred_semseg1 before the x8 up-sampling
            pred_boundary = dec.boundary_forward(feature)
            labels, ent = ops.predict_labels_bilinear8(s1, t.n_used)
            total_ent += float(ent) * len(paths)  # the reference's mean over images (it runs one image per batch)
            images += len(paths)
            tester_common.update_meter(t.meter, labels, gts, train_args.n_class)
            if args.saves_prob:
                tester_common.save_probs(t.base_outdir, paths, ops.bilinear8(s1))
            lab_dev = ops.resize_u8(labels, t.test_img_shape, nearest=True)
            lab = lab_dev.cpu().numpy()
            boundary = np.uint8(pred_boundary[:, 0].cpu().numpy() * 255)
            resized = []
            for k, path in enumerate(paths):
                name = os.path.basename(path)
                Image.fromarray(lab[k]).save(os.path.join(label_outdir, name))
                if save_vis is not None:
                    save_vis(lab[k], name)
                resized.append(Image.fromarray(boundary[k]).resize(t.test_img_shape, Image.BILINEAR))
                resized[k].save(os.path.join(boundary_outdir, name))
            if refiner is not None:  # on the bytes the boundary/ PNGs hold
                refined = refiner.refine(lab_dev, np.stack([np.asarray(im) for im in resized]))
                refiner.save(refined, [os.path.basename(path) for path in paths])
                gt_u8 = boundary_refine.tester_ground_truth(gts, labels, train_args.n_class, t.test_img_shape)
                if gt_u8 is not None:
                    refiner.update(lab_dev, refined, gt_u8)
    if refiner is not None:
        refiner.finish()
    return label_outdir, boundary_outdir, tester_common.finish(t.base_outdir, total_ent, images, t.meter)


if __name__ == "__main__":
    main()
