#!/usr/bin/env python3
"""Trainer of the domain-adversarial baseline the reference compares MCD against -- its ``dann_trainer.py`` (:73-358): G
(``DRNSegBase``), F (``DRNSegPixelClassifier``) and the domain classifier D (``DRNSegDomainClassifier``, three fused HIP launches each
way: csrc/dann.hip).  The checkpoint carries ``g_state_dict``, ``f1_state_dict``, ``d_state_dict`` and ``optimizer_g`` / ``_f`` /
``_d``; ``adapt_tester.py`` evaluates it as it is.

One iteration is the reference's two updates (:273-326):
  1. zero G and F; loss = CrossEntropyLoss2d(F(G(src)), lbl) - CE(D(G(src)), 1) - CE(D(G(tgt)), 0); backward; step G and F.
     D receives this gradient too.  It is not stepped here AND NOT ZEROED.
  2. zero G and F; both G passes again with the new weights; loss_d = CE(D(G(src)), 1) + CE(D(G(tgt)), 0); backward; step D; zero D.
     D's step therefore descends update 2's gradient PLUS the leftover negative gradient of update 1 -- the two nearly cancel, and what
     remains is what D learns.  This is the reference's behaviour, kept on purpose and pinned by tests/golden/dann_small.npz ("step").
Two shortcuts that change no number: update 2 runs G without a tape (the gradient it would send into G is zeroed at the top of the
next iteration, never used), and both domains go through D's kernels in one ``forward_pair`` (BatchNorm1d statistics stay per domain).

Departures from the reference: D's ``fc1`` is sized from ``--train_img_shape`` (the reference's 1089 fits 1080 x 1080
only); a resumed run reloads D and ``optimizer_d`` too (the reference forgets both); ``d_loss`` is logged as ``loss_d`` (the reference
divides by ``args.num_k``, which its DANN parser does not define); ``-b 1`` is refused before the first step (BatchNorm1d needs two
rows per domain; the reference's default of 1 cannot run its own DRN path); one process only -- data-parallel DANN is not built yet.
``--adjust_lr`` adjusts ``optimizer_g`` and ``optimizer_f`` only, as the reference does (:340-342).

    python dann_trainer.py suncg nyu --net drn_d_38 --input_ch 6 -b 16 --synthetic --no_pretrained
"""
import os

import torch

from argmyparse import get_da_dann_training_parser
from loss import CrossEntropyLoss2d
from models.model_util import get_dann_models, get_optimizer
from trainer_common import Trainer, adapt_layout, mcd_report, parse_args, train
from util import get_class_weight_from_file


def check(args, world=None):
    """what this trainer cannot run, said before anything is built (and before the GPU is touched)"""
    world = int(os.environ.get("WORLD_SIZE", "1")) if world is None else world
    if world > 1:
        raise SystemExit("dann_trainer.py runs in one process: data-parallel DANN is not built yet (got WORLD_SIZE=%d)" % world)
    if args.batch_size < 2:
        raise SystemExit("dann_trainer.py needs -b 2 or more: the domain classifier's BatchNorm1d takes its statistics over the batch of "
                         "one domain, and one sample has none (got -b %d)" % args.batch_size)


def build(args):
    model_g, model_f, model_d = get_dann_models(net_name=args.net, res=args.res, input_ch=args.input_ch, n_class=args.n_class,
                                                img_shape=args.train_img_shape)
    optimizers = {key: get_optimizer(m.parameters(), opt=args.opt, lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
                  for key, m in (("optimizer_g", model_g), ("optimizer_f", model_f), ("optimizer_d", model_d))}
    return {"g_state_dict": model_g, "f1_state_dict": model_f, "d_state_dict": model_d}, optimizers


def update_g_f(model_g, model_f, model_d, optimizer_g, optimizer_f, criterion, src_imgs, src_lbls, tgt_imgs):
    """update 1 (:273-304); returns c_loss.  D's gradient of ``-loss_d`` stays in ``model_d``'s ``.grad``."""
    optimizer_g.zero_grad()
    optimizer_f.zero_grad()
    src_fet, tgt_fet = model_g(src_imgs), model_g(tgt_imgs)
    domain_ce, _ = model_d.forward_pair(src_fet, tgt_fet)
    loss = criterion(model_f(src_fet), src_lbls)
    c_loss = loss.detach()
    (loss - domain_ce.sum()).backward()
    optimizer_g.step()
    optimizer_f.step()
    return c_loss


def update_d(model_g, model_d, optimizer_g, optimizer_f, optimizer_d, src_imgs, tgt_imgs):
    """update 2 (:306-322); returns loss_d.  G runs without a tape: what this pass would send into it is never used."""
    optimizer_g.zero_grad()
    optimizer_f.zero_grad()
    with torch.no_grad():
        src_fet, tgt_fet = model_g(src_imgs), model_g(tgt_imgs)
    domain_ce, _ = model_d.forward_pair(src_fet, tgt_fet)
    loss_d = domain_ce.sum()
    loss_d.backward()
    optimizer_d.step()
    optimizer_d.zero_grad()
    return loss_d.detach()


def make_step(args, run, modules, optimizers):
    model_g, model_f, model_d = (modules[k] for k in ("g_state_dict", "f1_state_dict", "d_state_dict"))
    optimizer_g, optimizer_f, optimizer_d = (optimizers[k] for k in ("optimizer_g", "optimizer_f", "optimizer_d"))
    weight = get_class_weight_from_file(n_class=args.n_class, weight_filename=args.loss_weights_file, add_bg_loss=args.add_bg_loss)
    criterion = CrossEntropyLoss2d(weight.to(run.device))

    def step(src_imgs, src_lbls, tgt_imgs, epoch):
        c_loss = update_g_f(model_g, model_f, model_d, optimizer_g, optimizer_f, criterion, src_imgs, src_lbls, tgt_imgs)
        d_loss = update_d(model_g, model_d, optimizer_g, optimizer_f, optimizer_d, src_imgs, tgt_imgs)
        return d_loss, c_loss
    return step


def layout(args, resumed):
    return adapt_layout(args, resumed, method="DANN")


def on_resume(args, cli):
    if "savename" not in vars(args):
        args.savename = os.path.split(cli.resume)[1].split("-")[0]


TRAINER = Trainer(build=build, make_step=make_step, layout=layout, sums=("d_loss", "c_loss"), report=mcd_report, on_resume=on_resume,
                  announces_resume=True, lr_adjusted=("optimizer_g", "optimizer_f"))


def main(argv=None):
    args = parse_args(get_da_dann_training_parser(), argv)
    check(args)
    return train(TRAINER, args)


if __name__ == "__main__":
    main()
