"""What the testers share: the prologue (the GPU check before any file is touched, checkpoint, output directory, ``param.json``, data
loader), the ground-truth update of the device-side confusion matrix, and the epilogue (``ave_ent_<x>.txt``, ``eval_result.json``).
``start`` is the whole prologue of the MCD testers; ``source_tester.py`` puts the same pieces around its own steps."""
import os
import types

import numpy as np
import torch

from datasets import get_dataset
from eval import ConfusionMeter
from util import check_if_done, load_checkpoint, mkdir_if_not_exist, save_colorized_lbl, save_dic_to_json


def unwrap(m):
    return m.module if isinstance(m, torch.nn.DataParallel) else m


def device():
    if not torch.cuda.is_available():
        raise SystemExit("this tester runs on an MI355X: the HIP kernels are the only implementation (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def load(args):
    if not os.path.exists(args.trained_checkpoint):
        raise OSError("%s does not exist!" % args.trained_checkpoint)
    return load_checkpoint(args.trained_checkpoint)


def output_dir(args, strip_tar=False):
    """<outdir>/<the training run's mode>---<dataset>-<split>/<checkpoint name without ".pth">[-use_f2]; sets ``args.mode``"""
    indir, infn = os.path.split(args.trained_checkpoint)
    args.mode = "%s---%s-%s" % (indir.split(os.path.sep)[-2], args.tgt_dataset, args.split)
    model_name = infn.replace(".pth", "").replace(".tar", "") if strip_tar else infn.replace(".pth", "")
    return os.path.join(args.outdir, args.mode, model_name + ("-use_f2" if getattr(args, "use_f2", False) else ""))


def write_params(args, base_outdir):
    mkdir_if_not_exist(base_outdir)
    json_fn = os.path.join(base_outdir, "param.json")
    check_if_done(json_fn)
    params = dict(vars(args))
    if not params.get("vis"):  # param.json of a run without --vis stays what it was
        params.pop("vis", None), params.pop("palette_json", None)
    save_dic_to_json(params, json_fn, verbose=False)


def make_loader(args, train_args, train_img_shape):
    spec = dict(length=args.synthetic_len, img_shape=[int(x) for x in train_img_shape], n_class=train_args.n_class,
                seed=args.seed) if args.synthetic else None
    tgt_dataset = get_dataset(dataset_name=args.tgt_dataset, split=args.split, img_transform=None, label_transform=None, test=True,
                              input_ch=train_args.input_ch, synthetic=spec)
    return torch.utils.data.DataLoader(tgt_dataset, batch_size=args.batch_size, pin_memory=True)


def new_meter(train_args, dev):
    """the reference shells out to eval.py over the written PNGs (util.py:36-41); here the confusion matrix is accumulated on the
    device while the label maps are still there"""
    return ConfusionMeter(train_args.n_class, background_id=255, device=dev)


def start(args, strip_tar=False):
    dev = device()
    base_outdir = output_dir(args, strip_tar)
    checkpoint = load(args)
    train_args = checkpoint["args"]
    args.start_epoch = checkpoint["epoch"]
    write_params(args, base_outdir)
    loader = make_loader(args, train_args, train_args.train_img_shape)
    os.environ["MCDSEG_PRETRAINED"] = "0"  # weights come from the checkpoint
    return types.SimpleNamespace(
        dev=dev, checkpoint=checkpoint, train_args=train_args, base_outdir=base_outdir, loader=loader,
        test_img_shape=tuple(int(x) for x in args.test_img_shape),
        n_used=args.n_class if getattr(train_args, "add_bg_loss", False) else args.n_class - 1,
        meter=new_meter(train_args, dev))


def update_meter(meter, labels, gts, n_class):
    """background is 255 in label PNGs, n_class-1 in training labels"""
    if torch.is_tensor(gts) and gts.dim() == 3 and tuple(gts.shape) == tuple(labels.shape):
        gts = gts.to(labels.device)
        meter.update(labels, torch.where(gts == n_class - 1, torch.full_like(gts, 255), gts))


def save_probs(base_outdir, paths, full):
    prob_outdir = os.path.join(base_outdir, "prob")
    mkdir_if_not_exist(prob_outdir)
    for k, path in enumerate(paths):
        np.save(os.path.join(prob_outdir, os.path.basename(path).replace("png", "npy")), full[k].cpu().numpy())


def vis_saver(args, base_outdir, n_used):
    """``--vis``: ``save(label, name, subdir=None)`` writes ``vis/[<subdir>/]<name>`` beside ``label/``: the label image (a uint8 array, or
    the PIL image that went into ``label/``) in mode "P" with the colours of ``--palette_json``, or with the PASCAL-VOC colours of
    ``n_used + 1`` labels (``ensemble.default_palette``).  None without the flag: no directory is made, nothing is written."""
    if not getattr(args, "vis", False):
        return None
    from PIL import Image
    import ensemble
    palette = ensemble.load_palette(args.palette_json) if getattr(args, "palette_json", None) else ensemble.default_palette(min(n_used + 1, 256))
    vis_root = os.path.join(base_outdir, "vis")
    mkdir_if_not_exist(vis_root)

    def save(label, name, subdir=None):
        outdir = vis_root if subdir is None else os.path.join(vis_root, subdir)
        mkdir_if_not_exist(outdir)
        img = label.copy() if isinstance(label, Image.Image) else Image.fromarray(label)  # (putpalette changes the image it is given)
        save_colorized_lbl(img, os.path.join(outdir, name), palette)
    return save


def finish(base_outdir, total_ent, count, meter):
    """``count``: what ``total_ent`` was summed over -- batches in adapt_tester.py, images in the others"""
    ave_ent = total_ent / max(count, 1)
    print("average entropy: %s" % ave_ent)
    with open(os.path.join(base_outdir, "ave_ent_%s.txt" % ave_ent), "w") as f:
        f.write(str(ave_ent))
    if int(meter.hist.sum()) > 0:
        summary = meter.summary()
        save_dic_to_json(summary, os.path.join(base_outdir, "eval_result.json"), verbose=False)
        print("pixAcc %.2f  mAcc %.2f  fwIoU %.2f  mIoU %.2f" % (summary["pixAcc"], summary["mAcc"], summary["fwIoU"], summary["mIoU"]))
    return ave_ent
