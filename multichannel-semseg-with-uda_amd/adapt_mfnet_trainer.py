#!/usr/bin/env python3
"""MCD trainer for the two-encoder MFNet (RGB encoder + HHA/depth encoder, fused classifiers) -- the reference's
``adapt_mfnet_trainer.py`` (:22-270) on the MI355X HIP kernels.

    python adapt_mfnet_trainer.py suncg nyu --input_ch 6 --method_detail MFNet-ScoreAddFusion -b 16 --synthetic --no_pretrained
"""
from argmyparse import get_da_mcd_training_parser
from loss import CrossEntropyLoss2d, ProbCrossEntropyLoss2d
from models.model_util import get_models, get_optimizer
from solvers.solver import MFNetMCDSolver
from trainer_common import Trainer, adapt_layout, criteria, mcd_report, parse_args, train


def get_parser():
    parser = get_da_mcd_training_parser()
    parser.add_argument("--method_detail", type=str, default="MFNet-AddFusion",
                        help="MFNet-{Add,Gate,Concat,ConcatConv}Fusion, MFNet-Score{Add,Gate}Fusion")
    return parser


def build(args):
    g3, g1, f1, f2 = get_models(net_name=args.net, res=args.res, input_ch=args.input_ch, n_class=args.n_class,
                                method=args.method_detail, is_data_parallel=args.is_data_parallel)
    optimizer_g = get_optimizer(list(g3.parameters()) + list(g1.parameters()), lr=args.lr, opt=args.opt,
                                momentum=args.momentum, weight_decay=args.weight_decay)
    optimizer_f = get_optimizer(list(f1.parameters()) + list(f2.parameters()), lr=args.lr, opt=args.opt,
                                momentum=args.momentum, weight_decay=args.weight_decay)
    return ({"g_3ch_state_dict": g3, "g_1ch_state_dict": g1, "f1_state_dict": f1, "f2_state_dict": f2},
            {"optimizer_g": optimizer_g, "optimizer_f": optimizer_f})


def make_step(args, run, modules, optimizers):
    # the gated fusions are paired with the probability-input criterion (adapt_mfnet_trainer.py:149)
    criterion, criterion_d = criteria(args, run.device, ProbCrossEntropyLoss2d if "Gate" in args.method_detail else CrossEntropyLoss2d)
    solver = MFNetMCDSolver(*modules.values(), *optimizers.values(), criterion, criterion_d, num_k=args.num_k)
    return lambda src_imgs, src_lbls, tgt_imgs, epoch: solver.step(src_imgs, src_lbls, tgt_imgs)


TRAINER = Trainer(build=build, make_step=make_step, sums=("c_loss", "d_loss"), report=mcd_report, backfill=("method_detail",),
                  layout=lambda args, resumed: adapt_layout(args, resumed, "_MFNet", args.method_detail))


def main(argv=None):
    return train(TRAINER, parse_args(get_parser(), argv))


if __name__ == "__main__":
    main()
