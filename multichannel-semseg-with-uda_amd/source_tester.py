#!/usr/bin/env python3
"""Source-only inference -- the reference's ``source_tester.py`` (:1-167): load a ``source_trainer`` checkpoint into
``get_full_model`` (DRNSeg with DataParallel's ``module.`` keys), run it in eval mode and write per image

    label/<name>       argmax over the non-background classes, resized NEAREST to the test shape
    prob/<name>.npy    the full-resolution logits (only with ---saves_prob)
    vis/<name>         the label PNG with a palette, mode P (only with --vis)

plus ``ave_ent_<x>.txt``, an empty ``data_list.txt`` (as the reference leaves it) and, when the data carry ground truth,
``eval_result.json``.  For ``suncg`` the outputs go one directory deeper, into the image's own subdirectory, as there.

The model's last layer, the learned x8 up-sampler, is fused into the argmax / entropy kernel (``mcdseg_predict_labels_up8``): the
full-resolution logits are formed only with ---saves_prob.  ``--vis`` adds ``vis/<name>``, the label PNG with a palette (``--palette_json``,
or the PASCAL-VOC colours); the ``eval.py`` run of the reference is outside this build.

    python source_tester.py nyu train_output/suncg-train_only_6ch/pth/normal-drn_d_38-40.pth.tar --synthetic
"""
import argparse
import os

import numpy as np
import torch
from PIL import Image

import tester_common
from argmyparse import add_additional_params_to_args
from datasets import AVAILABLE_DATASET_LIST
from models.model_util import get_full_model
from util import mkdir_if_not_exist
from mcdseg import ops


def get_parser():
    """source_tester.py:22-32 of the reference (its three-dash ``---saves_prob`` kept, ``--saves_prob`` accepted too) + this
    build's synthetic-data switches"""
    parser = argparse.ArgumentParser(description="Adapt tester for validation data")
    parser.add_argument("tgt_dataset", type=str, choices=AVAILABLE_DATASET_LIST)
    parser.add_argument("--split", type=str, default="val", help="'val' or 'test')  is used")
    parser.add_argument("trained_checkpoint", type=str, metavar="PTH")
    parser.add_argument("--outdir", type=str, default="test_output", help="output directory")
    parser.add_argument("--test_img_shape", default=None, nargs=2, type=int, help="W H, FOR Valid(2048, 1024) Test(1280, 720)")
    parser.add_argument("---saves_prob", "--saves_prob", dest="saves_prob", action="store_true",
                        help="whether you save probability tensors")
    g = parser.add_argument_group("MI355X build")
    g.add_argument("--synthetic", action="store_true")
    g.add_argument("--synthetic_len", type=int, default=4)
    g.add_argument("--seed", type=int, default=4321)
    g.add_argument("-b", "--batch_size", type=int, default=1)
    g.add_argument("--vis", action="store_true", help="also write vis/<name>: the label PNG with a palette (mode P)")
    g.add_argument("--palette_json", type=str, default=None,
                   help='with --vis: a {"palette": [[r,g,b],...]} file (default: the PASCAL-VOC colours of the classes used + 1)')
    return parser


def add_subdir_if_necessary(outdir, subdir, tgt_dataset):
    if tgt_dataset == "suncg":
        outdir = os.path.join(outdir, subdir)
    return outdir


def main(argv=None):
    args = add_additional_params_to_args(get_parser().parse_args(argv))
    dev = tester_common.device()
    checkpoint = tester_common.load(args)
    if "args" not in checkpoint:
        raise SystemExit("%s holds no training arguments ('args'): the network and class count cannot be known" % args.trained_checkpoint)
    train_args = checkpoint["args"]

    os.environ["MCDSEG_PRETRAINED"] = "0"  # weights come from the checkpoint
    model = get_full_model(train_args.net, train_args.res, train_args.n_class, train_args.input_ch)
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
    net = tester_common.unwrap(model)
    n_used = train_args.n_class if getattr(train_args, "add_bg_loss", False) else train_args.n_class - 1

    with open(os.path.join(base_outdir, "data_list.txt"), "w"):
        pass
    label_root = os.path.join(base_outdir, "label")
    mkdir_if_not_exist(label_root)
    total_ent, images = 0.0, 0
    meter = tester_common.new_meter(train_args, dev)
    save_vis = tester_common.vis_saver(args, base_outdir, n_used)
    with torch.no_grad():
        for imgs, gts, paths in loader:
            imgs = imgs.to(dev, non_blocking=True)
            scores = net.seg(net.base(imgs))  # DRNSeg.forward up to its up-sampler
            labels, ent = ops.predict_labels_up8(scores, net.up.weight, n_used)
            total_ent += float(ent) * len(paths)  # the reference's mean over images (it runs one image per batch)
            images += len(paths)
            tester_common.update_meter(meter, labels, gts, train_args.n_class)
            full = ops.up8(scores, net.up.weight) if args.saves_prob else None
            lab = ops.resize_u8(labels, test_img_shape, nearest=True).cpu().numpy()
            for k, path in enumerate(paths):
                name, subdir = os.path.basename(path), os.path.basename(os.path.dirname(path))
                if full is not None:
                    prob_outdir = add_subdir_if_necessary(os.path.join(base_outdir, "prob"), subdir, args.tgt_dataset)
                    mkdir_if_not_exist(prob_outdir)
                    np.save(os.path.join(prob_outdir, name.replace("png", "npy")), full[k].cpu().numpy())
                label_outdir = add_subdir_if_necessary(label_root, subdir, args.tgt_dataset)
                mkdir_if_not_exist(label_outdir)
                Image.fromarray(lab[k]).save(os.path.join(label_outdir, name))
                if save_vis is not None:
                    save_vis(lab[k], name, subdir if args.tgt_dataset == "suncg" else None)
            del full
    return label_root, tester_common.finish(base_outdir, total_ent, images, meter)


if __name__ == "__main__":
    main()
