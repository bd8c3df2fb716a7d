#!/usr/bin/env python3
"""MCD + HHA-regression multitask trainer -- the reference's ``adapt_multitask_trainer.py`` (:21-273) on the
MI355X HIP kernels: RGB encoder, two segmentation decoders + one depth decoder, learned task weights.

    python adapt_multitask_trainer.py suncg nyu --input_ch 6 -b 8 --synthetic --no_pretrained
"""
from argmyparse import get_da_mcd_training_parser
from models.model_util import get_multitask_models, get_optimizer
from solvers.solver import MultiTaskMCDSolver
from trainer_common import Trainer, adapt_layout, criteria, mcd_report, parse_args, train


def build(args):
    criterion, criterion_d = criteria(args)  # built before the models, which keep them as buffers
    model_enc, model_dec = get_multitask_models(net_name=args.net, input_ch=args.input_ch, n_class=args.n_class,
                                                is_data_parallel=args.is_data_parallel, semseg_criterion=criterion,
                                                discrepancy_criterion=criterion_d)
    optimizer_enc = get_optimizer(model_enc.parameters(), lr=args.lr, momentum=args.momentum, opt=args.opt,
                                  weight_decay=args.weight_decay)
    optimizer_dec = get_optimizer(model_dec.parameters(), opt=args.opt, lr=args.lr, momentum=args.momentum,
                                  weight_decay=args.weight_decay)
    return ({"enc_state_dict": model_enc, "dec_state_dict": model_dec}, {"optimizer_enc": optimizer_enc, "optimizer_dec": optimizer_dec})


def make_step(args, run, modules, optimizers):
    solver = MultiTaskMCDSolver(*modules.values(), *optimizers.values(), num_k=args.num_k, num_multiply_d_loss=args.num_multiply_d_loss)

    def step(src_imgs, src_gt, tgt_imgs, epoch):
        c_loss, d_loss, parts = solver.step(src_imgs, src_gt, tgt_imgs)
        return c_loss, d_loss, parts[0], parts[1], parts[2]
    return step


def report(epoch, sums, modules):
    dec = modules["dec_state_dict"]
    std_semseg, std_depth = (dec.module if hasattr(dec, "module") else dec).get_task_weights()
    print("std_semseg: %.4f, std_depth: %.4f" % (float(std_semseg.reshape(-1)[0]), float(std_depth.reshape(-1)[0])))  # (1-element arrays, as the reference returns them)
    mcd_report(epoch, sums, modules)


TRAINER = Trainer(build=build, make_step=make_step, report=report,
                  sums=("c_loss", "d_loss", "src_semseg_loss", "src_depth_loss", "tgt_depth_loss"),
                  layout=lambda args, resumed: adapt_layout(args, resumed, "_MCDmultitask"))


def main(argv=None):
    args = parse_args(get_da_mcd_training_parser(), argv)
    if args.input_ch <= 3:
        raise SystemExit("the multitask trainer regresses the channels after RGB: --input_ch must be 4 or 6")
    return train(TRAINER, args)


if __name__ == "__main__":
    main()
