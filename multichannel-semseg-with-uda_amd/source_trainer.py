#!/usr/bin/env python3
"""Source-only supervised trainer -- the reference's ``source_trainer.py`` (:21-165): DRNSeg wrapped so that
the checkpoint carries DataParallel's ``module.`` prefix, CE loss, SGD; BASELINE config 1 geometry is
``suncg --net drn_d_38 --input_ch 6 -b 2 --train_img_shape 320 240 --synthetic --no_pretrained``."""
import os

from argmyparse import get_src_only_training_parser
from loss import CrossEntropyLoss2d
from models.model_util import get_full_model, get_optimizer
from trainer_common import Layout, Trainer, model_name, parse_args, train
from util import get_class_weight_from_file


def build(args):
    model = get_full_model(net=args.net, res=args.res, n_class=args.n_class, input_ch=args.input_ch)
    optimizer = get_optimizer(model.parameters(), opt=args.opt, lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
    return {"state_dict": model}, {"optimizer": optimizer}


def layout(args, resumed):
    """the output directories travel in the checkpoint's arguments: a resumed run writes where the first one did"""
    name = model_name(args)
    if not resumed:
        args.outdir = os.path.join(args.base_outdir, "%s-%s_only_%sch" % (args.src_dataset, args.split, args.input_ch))
        args.pth_dir = os.path.join(args.outdir, "pth")
        args.tflog_dir = os.path.join(args.outdir, "tflog", name)
    json_fn = "param_%s_resume.json" % args.savename if resumed else "param-%s.json" % name
    return Layout(args.pth_dir, args.tflog_dir, os.path.join(args.outdir, json_fn), name)


def make_step(args, run, modules, optimizers):
    model, optimizer = modules["state_dict"], optimizers["optimizer"]
    weight = get_class_weight_from_file(n_class=args.n_class, weight_filename=args.loss_weights_file, add_bg_loss=args.add_bg_loss)
    criterion = CrossEntropyLoss2d(weight.to(run.device))

    def step(imgs, lbls, epoch):
        optimizer.zero_grad()
        loss = criterion(model(imgs), lbls)
        loss.backward()
        optimizer.step()
        return (loss,)
    return step


def report(epoch, sums, modules):
    print("Epoch [%d] Loss: %.4f" % (epoch + 1, sums["loss"]))


TRAINER = Trainer(build=build, make_step=make_step, layout=layout, sums=("loss",), report=report)


def main(argv=None):
    return train(TRAINER, parse_args(get_src_only_training_parser(), argv))


if __name__ == "__main__":
    main()
