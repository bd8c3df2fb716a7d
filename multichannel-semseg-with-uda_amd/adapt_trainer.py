#!/usr/bin/env python3
"""MCD early-fusion trainer -- entry point with the reference's CLI, output layout and checkpoint format
(adapt_trainer.py:21-245), running on the MI355X HIP kernels.

    python adapt_trainer.py suncg nyu --input_ch 6 -b 16 --synthetic --no_pretrained
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 adapt_trainer.py suncg nyu ... (data parallel)

Three-step update per iteration (adapt_trainer.py:155-220): ``--solver fused`` (default) uses
``solvers.solver.MCDSolver``; ``--solver dropin`` runs the reference's statements over the drop-in modules.
"""
import os

from argmyparse import get_da_mcd_training_parser
from models.model_util import get_models, get_optimizer
from solvers.solver import MCDSolver
from trainer_common import Trainer, adapt_layout, criteria, mcd_report, parse_args, train


def build(args):
    model_g, model_f1, model_f2 = get_models(net_name=args.net, res=args.res, input_ch=args.input_ch, n_class=args.n_class,
                                             method=args.method, is_data_parallel=args.is_data_parallel)
    optimizer_g = get_optimizer(model_g.parameters(), lr=args.lr, momentum=args.momentum, opt=args.opt,
                                weight_decay=args.weight_decay)
    optimizer_f = get_optimizer(list(model_f1.parameters()) + list(model_f2.parameters()), opt=args.opt, lr=args.lr,
                                momentum=args.momentum, weight_decay=args.weight_decay)
    return ({"g_state_dict": model_g, "f1_state_dict": model_f1, "f2_state_dict": model_f2},
            {"optimizer_g": optimizer_g, "optimizer_f": optimizer_f})


def dropin_step(model_g, model_f1, model_f2, optimizer_g, optimizer_f, criterion, criterion_d, src_imgs, src_lbls, tgt_imgs,
                num_k, num_multiply_d_loss):
    """adapt_trainer.py:163-214, statement for statement"""
    optimizer_g.zero_grad()
    optimizer_f.zero_grad()
    outputs = model_g(src_imgs)
    loss = criterion(model_f1(outputs), src_lbls) + criterion(model_f2(outputs), src_lbls)
    loss.backward()
    c_loss = loss.detach()
    optimizer_g.step()
    optimizer_f.step()
    optimizer_g.zero_grad()
    optimizer_f.zero_grad()
    outputs = model_g(src_imgs)
    loss = criterion(model_f1(outputs), src_lbls) + criterion(model_f2(outputs), src_lbls)
    outputs = model_g(tgt_imgs)
    loss = loss - criterion_d(model_f1(outputs), model_f2(outputs))
    loss.backward()
    optimizer_f.step()
    for _ in range(num_k):
        optimizer_g.zero_grad()
        outputs = model_g(tgt_imgs)
        loss = criterion_d(model_f1(outputs), model_f2(outputs)) * num_multiply_d_loss
        loss.backward()
        optimizer_g.step()
    return c_loss, loss.detach() / num_k


def make_step(args, run, modules, optimizers):
    if args.no_dropout:  # (said by this trainer alone)
        print("NO DROPOUT")
    models, optims = tuple(modules.values()), tuple(optimizers.values())
    criterion, criterion_d = criteria(args, run.device)
    if args.solver == "fused":  # whatever --d_loss: every distance is a kind of the fused loss kernels
        solver = MCDSolver(*models, *optims, criterion, criterion_d, num_k=args.num_k, num_multiply_d_loss=args.num_multiply_d_loss)
        return lambda src_imgs, src_lbls, tgt_imgs, epoch: solver.step(src_imgs, src_lbls, tgt_imgs)
    return lambda src_imgs, src_lbls, tgt_imgs, epoch: dropin_step(*models, *optims, criterion, criterion_d, src_imgs, src_lbls,
                                                                   tgt_imgs, args.num_k, args.num_multiply_d_loss)


def on_resume(args, cli):
    if "savename" not in vars(args):
        args.savename = os.path.split(cli.resume)[1].split("-")[0]


TRAINER = Trainer(build=build, make_step=make_step, layout=adapt_layout, sums=("c_loss", "d_loss"), report=mcd_report,
                  on_resume=on_resume, announces_resume=True)


def main(argv=None):
    return train(TRAINER, parse_args(get_da_mcd_training_parser(), argv))


if __name__ == "__main__":
    main()
