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
``--use_f2`` only renames the output directory, as there.  The palette visualisation and ``eval.py`` run of the reference are
outside this build.

    python adapt_multitask_tester.py nyu train_output/...MCDmultitask/pth/MCD-normal-drn_d_38-40.pth.tar --synthetic
"""
import os

import numpy as np
import torch
from PIL import Image

from argmyparse import add_additional_params_to_args, get_da_mcd_testing_parser
from datasets import get_dataset
from eval import ConfusionMeter
from loss import CrossEntropyLoss2d, get_prob_distance_criterion
from models.model_util import get_multitask_models
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
    # checkpoint carries it, so they are built as the trainer built them (adapt_multitask_tester.py:73-86)
    weight = get_class_weight_from_file(n_class=train_args.n_class, weight_filename=train_args.loss_weights_file,
                                        add_bg_loss=train_args.add_bg_loss)
    model_enc, model_dec = get_multitask_models(net_name=train_args.net, input_ch=train_args.input_ch, n_class=train_args.n_class,
                                                is_data_parallel=getattr(train_args, "is_data_parallel", False),
                                                semseg_criterion=CrossEntropyLoss2d(weight),
                                                discrepancy_criterion=get_prob_distance_criterion(train_args.d_loss, n_class=train_args.n_class))
    model_enc.load_state_dict(checkpoint["enc_state_dict"])
    model_dec.load_state_dict(checkpoint["dec_state_dict"])
    dec = _unwrap(model_dec)
    print(dec.get_task_weights())
    for m in (model_enc, model_dec):
        m.eval()
        m.to(dev)
    n_used = args.n_class if getattr(train_args, "add_bg_loss", False) else args.n_class - 1

    label_outdir = os.path.join(base_outdir, "label")
    depth_outdir = os.path.join(base_outdir, "depth")
    mkdir_if_not_exist(label_outdir)
    mkdir_if_not_exist(depth_outdir)
    total_ent, images = 0.0, 0
    meter = ConfusionMeter(train_args.n_class, background_id=255, device=dev)
    with torch.no_grad():
        for imgs, gts, paths in loader:
            imgs = imgs.to(dev, non_blocking=True)
            feature = model_enc(imgs[:, :3, :, :].contiguous())
            s1 = dec.semsegcls_dec1(feature)  # pred_semseg1 before the x8 up-sampling
            dep = dec.deprgr_dec(feature)     # pred_depth before the x8 up-sampling
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
            depth = ops.resize_u8(ops.depth_image_u8(dep), test_img_shape).cpu().numpy()
            for k, path in enumerate(paths):
                name = os.path.basename(path)
                Image.fromarray(lab[k]).save(os.path.join(label_outdir, name))
                Image.fromarray(depth[k]).save(os.path.join(depth_outdir, name))
    ave_ent = total_ent / max(images, 1)
    print("average entropy: %s" % ave_ent)
    with open(os.path.join(base_outdir, "ave_ent_%s.txt" % ave_ent), "w") as f:
        f.write(str(ave_ent))
    if int(meter.hist.sum()) > 0:
        summary = meter.summary()
        save_dic_to_json(summary, os.path.join(base_outdir, "eval_result.json"), verbose=False)
        print("pixAcc %.2f  mAcc %.2f  fwIoU %.2f  mIoU %.2f" % (summary["pixAcc"], summary["mAcc"], summary["fwIoU"], summary["mIoU"]))
    return label_outdir, depth_outdir, ave_ent


if __name__ == "__main__":
    main()
