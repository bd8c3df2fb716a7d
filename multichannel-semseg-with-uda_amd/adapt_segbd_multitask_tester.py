#!/usr/bin/env python3
"""Segmentation + boundary multitask MCD inference -- the reference's ``adapt_segbd_multitask_tester.py`` (:1-176): load an
``adapt_segbd_multitask_trainer`` checkpoint (``enc_state_dict`` / ``dec_state_dict``), run the stage-tap RGB encoder on
``imgs[:, :3]`` and the decoder in eval mode, and write per image

    label/<name>       argmax of pred_semseg1 over the non-background classes, resized NEAREST to the test shape
    boundary/<name>    np.uint8(pred_boundary * 255) (numpy's own cast, on the host), resized BILINEAR to the test shape
    prob/<name>.npy    pred_semseg1 at full resolution (only with --saves_prob)

plus ``ave_ent_<x>.txt`` (mean entropy of pred_semseg1) and, when the data carry ground truth, ``eval_result.json``.

The segmentation heads run at 1/8 resolution; the x8 bilinear up-sampling is fused into the argmax / entropy kernel
(``mcdseg_predict_labels_up8``); the boundary map is one pass of ``mcdseg_boundary_head_fwd``.  pred_semseg2 is not evaluated: the reference computes it and drops it (its F2 average is commented out, :122-125), so
``--use_f2`` only renames the output directory, as there.  The palette visualisation (``vis/``) and ``eval.py`` run of the reference are
outside this build, as in the other testers.

    python adapt_segbd_multitask_tester.py nyu train_output/...MCD_segbd_multitask/pth/MCD-normal-drn_d_38-40.pth.tar --synthetic
"""
import os

import numpy as np
import torch
from PIL import Image

from argmyparse import add_additional_params_to_args, get_da_mcd_testing_parser
from datasets import get_dataset
from eval import ConfusionMeter
from loss import CrossEntropyLoss2d, get_prob_distance_criterion
from models.model_util import get_segbd_multitask_models
from util import check_if_done, get_class_weight_from_file, load_checkpoint, mkdir_if_not_exist, save_dic_to_json
from mcdseg import ops


def _unwrap(m):
    return m.module if isinstance(m, torch.nn.DataParallel) else m


def main(argv=None):
    args = get_da_mcd_testing_parser().parse_args(argv)
    args = add_additional_params_to_args(args)
    if not torch.cuda.is_available():
        raise SystemExit("this tester runs on an MI355X: the HIP kernels are the only implementation (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    indir, infn = os.path.split(args.trained_checkpoint)
    trained_mode = indir.split(os.path.sep)[-2]
    args.mode = "%s---%s-%s" % (trained_mode, args.tgt_dataset, args.split)
    model_name = infn.replace(".pth", "") + ("-use_f2" if args.use_f2 else "")
    if not os.path.exists(args.trained_checkpoint):
        raise OSError("%s does not exist!" % args.trained_checkpoint)
    checkpoint = load_checkpoint(args.trained_checkpoint)
    train_args = checkpoint["args"]
    args.start_epoch = checkpoint["epoch"]
    base_outdir = os.path.join(args.outdir, args.mode, model_name)
    mkdir_if_not_exist(base_outdir)
    json_fn = os.path.join(base_outdir, "param.json")
    check_if_done(json_fn)
    save_dic_to_json(dict(vars(args)), json_fn, verbose=False)

    train_img_shape = [int(x) for x in train_args.train_img_shape]
    test_img_shape = tuple(int(x) for x in args.test_img_shape)
    spec = dict(length=args.synthetic_len, img_shape=train_img_shape, n_class=train_args.n_class, seed=args.seed) if args.synthetic else None
    tgt_dataset = get_dataset(dataset_name=args.tgt_dataset, split=args.split, img_transform=None, label_transform=None, test=True,
                              input_ch=train_args.input_ch, synthetic=spec)
    loader = torch.utils.data.DataLoader(tgt_dataset, batch_size=args.batch_size, pin_memory=True)

    os.environ["MCDSEG_PRETRAINED"] = "0"  # weights come from the checkpoint
    # the criteria are not used here, but the decoder holds the class weights as a buffer (semseg_criterion.nll_loss.weight) and the
    # checkpoint carries it, so they are built as the trainer built them (adapt_segbd_multitask_tester.py:76-93)
    weight = get_class_weight_from_file(n_class=train_args.n_class, weight_filename=train_args.loss_weights_file,
                                        add_bg_loss=train_args.add_bg_loss)
    model_enc, model_dec = get_segbd_multitask_models(
        net_name=train_args.net, input_ch=train_args.input_ch, n_class=train_args.n_class,
        is_data_parallel=getattr(train_args, "is_data_parallel", False), semseg_criterion=CrossEntropyLoss2d(weight),
        discrepancy_criterion=get_prob_distance_criterion(train_args.d_loss, n_class=train_args.n_class),
        semseg_shortcut=getattr(train_args, "semseg_shortcut", False), depth_shortcut=getattr(train_args, "depth_shortcut", False),
        add_pred_seg_boundary_loss=getattr(train_args, "add_pred_seg_boundary_loss", False),
        use_seg2bd_conv=getattr(train_args, "use_seg2bd_conv", False))
    model_enc.load_state_dict(checkpoint["enc_state_dict"])
    model_dec.load_state_dict(checkpoint["dec_state_dict"])
    enc, dec = _unwrap(model_enc), _unwrap(model_dec)
    print(dec.get_task_weights())
    for m in (model_enc, model_dec):
        m.eval()
        m.to(dev)
    n_used = args.n_class if getattr(train_args, "add_bg_loss", False) else args.n_class - 1

    label_outdir = os.path.join(base_outdir, "label")
    boundary_outdir = os.path.join(base_outdir, "boundary")
    mkdir_if_not_exist(label_outdir)
    mkdir_if_not_exist(boundary_outdir)
    total_ent, images = 0.0, 0
    meter = ConfusionMeter(train_args.n_class, background_id=255, device=dev)
    with torch.no_grad():
        for imgs, gts, paths in loader:
            imgs = imgs.to(dev, non_blocking=True)
            feature = enc(imgs[:, :3, :, :].contiguous())
            s1 = dec.semsegcls_dec1(feature["h8"])  # pred_semseg1 before the x8 up-sampling
            pred_boundary = dec.boundary_forward(feature)
            labels, ent = ops.predict_labels_bilinear8(s1, n_used)
            total_ent += float(ent) * len(paths)  # the reference's mean over images (it runs one image per batch)
            images += len(paths)
            if torch.is_tensor(gts) and gts.dim() == 3 and tuple(gts.shape) == tuple(labels.shape):
                gts = gts.to(dev)
                meter.update(labels, torch.where(gts == train_args.n_class - 1, torch.full_like(gts, 255), gts))
            if args.saves_prob:
                prob_outdir = os.path.join(base_outdir, "prob")
                mkdir_if_not_exist(prob_outdir)
                full = ops.bilinear8(s1)
                for k, path in enumerate(paths):
                    np.save(os.path.join(prob_outdir, os.path.basename(path).replace("png", "npy")), full[k].cpu().numpy())
                del full
            lab = ops.resize_u8(labels, test_img_shape, nearest=True).cpu().numpy()
            boundary = np.uint8(pred_boundary[:, 0].cpu().numpy() * 255)
            for k, path in enumerate(paths):
                name = os.path.basename(path)
                Image.fromarray(lab[k]).save(os.path.join(label_outdir, name))
                Image.fromarray(boundary[k]).resize(test_img_shape, Image.BILINEAR).save(os.path.join(boundary_outdir, name))
    ave_ent = total_ent / max(images, 1)
    print("average entropy: %s" % ave_ent)
    with open(os.path.join(base_outdir, "ave_ent_%s.txt" % ave_ent), "w") as f:
        f.write(str(ave_ent))
    if int(meter.hist.sum()) > 0:
        summary = meter.summary()
        save_dic_to_json(summary, os.path.join(base_outdir, "eval_result.json"), verbose=False)
        print("pixAcc %.2f  mAcc %.2f  fwIoU %.2f  mIoU %.2f" % (summary["pixAcc"], summary["mAcc"], summary["fwIoU"], summary["mIoU"]))
    return label_outdir, boundary_outdir, ave_ent


if __name__ == "__main__":
    main()
