#!/usr/bin/env python3
"""Source-only trainer of the aleatoric-uncertainty model -- the reference's ``source_uncertain_trainer.py`` (:25-179):
``UncertainDRNSeg`` (DRNSeg + the ``up_std`` up-sampler), whose loss averages ``--n_dropout`` Monte-Carlo dropout passes.  The
reference runs the network that many times per step; here ``get_loss`` runs the trunk once and one HIP kernel loops over the draws
(models/dilated_fcn.py, csrc/uncertain.hip).  The checkpoint carries ``state_dict`` WITHOUT DataParallel's ``module.`` prefix (the
reference passes ``is_data_parallel=False``, :69-70) and ``optimizer``.

Two deliberate departures from the reference:
  * its ``loss = base_loss + uncertain_loss`` is a vector of one entry per sample, so its ``loss.backward()`` works at ``-b 1`` only
    (:138-140); the step here descends ``base_loss + uncertain_loss.mean()``, which is that loss at ``-b 1``;
  * its resume branch builds ``get_full_model`` -- a DRNSeg without ``up_std``, into which its own checkpoint does not load (:54-57);
    a resumed run here rebuilds ``UncertainDRNSeg``.

    python source_uncertain_trainer.py suncg --net drn_d_38 --input_ch 6 -b 2 --train_img_shape 320 240 --synthetic --no_pretrained
"""
import os

from argmyparse import get_src_only_training_parser
from loss import CrossEntropyLoss2d
from models.model_util import get_full_uncertain_model, get_optimizer
from trainer_common import Layout, Trainer, model_name, parse_args, train
from util import get_class_weight_from_file


def get_parser():
    parser = get_src_only_training_parser()
    parser.add_argument("--n_dropout", type=int, default=10, help="how many dropout passes one loss averages")  # (:26-27)
    return parser


def build(args):
    weight = get_class_weight_from_file(n_class=args.n_class, weight_filename=args.loss_weights_file, add_bg_loss=args.add_bg_loss)
    model = get_full_uncertain_model(net=args.net, res=args.res, n_class=args.n_class, input_ch=args.input_ch, n_dropout=args.n_dropout,
                                     criterion=CrossEntropyLoss2d(weight), is_data_parallel=False)
    model.seed_draws(getattr(args, "seed", 1234))
    optimizer = get_optimizer(model.parameters(), opt=args.opt, lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
    return {"state_dict": model}, {"optimizer": optimizer}


def layout(args, resumed):
    """the output directories travel in the checkpoint's arguments: a resumed run writes where the first one did"""
    name = model_name(args)
    if not resumed:
        args.outdir = os.path.join(args.base_outdir, "%s-%s_only_%sch_uncertain" % (args.src_dataset, args.split, args.input_ch))
        args.pth_dir = os.path.join(args.outdir, "pth")
        args.tflog_dir = os.path.join(args.outdir, "tflog", name)
    json_fn = "param_%s_resume.json" % args.savename if resumed else "param-%s.json" % name
    return Layout(args.pth_dir, args.tflog_dir, os.path.join(args.outdir, json_fn), name)


def make_step(args, run, modules, optimizers):
    model, optimizer = modules["state_dict"], optimizers["optimizer"]
    seen = {"epoch": None, "ind": 0}

    def step(imgs, lbls, epoch):
        if seen["epoch"] != epoch:
            seen.update(epoch=epoch, ind=0)
        optimizer.zero_grad()
        base_loss, uncertain_loss = model.get_loss(imgs, lbls, separately_returning=True)
        uncertain_loss = uncertain_loss.mean()
        loss = base_loss + uncertain_loss
        loss.backward()
        optimizer.step()
        if seen["ind"] % 100 == 0 and run.is_main:  # (:148-150; the only host read of the step besides the epoch sums)
            print("iter [%d] TotalLoss: %.4f (SegLoss: %.4f UncertainLoss: %.4f)" % (seen["ind"], float(loss.detach()), float(base_loss.detach()),
                                                                                       float(uncertain_loss.detach())))
        seen["ind"] += 1
        return loss.detach(), base_loss.detach(), uncertain_loss.detach()
    return step


def report(epoch, sums, modules):
    print("Epoch [%d] Loss: %.4f" % (epoch + 1, sums["loss"]))


TRAINER = Trainer(build=build, make_step=make_step, layout=layout, sums=("loss", "seg_loss", "uncertain_loss"), report=report,
                  backfill=("n_dropout",))


def main(argv=None):
    return train(TRAINER, parse_args(get_parser(), argv))


if __name__ == "__main__":
    main()
