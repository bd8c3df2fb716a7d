#!/usr/bin/env python3
"""MCD + boundary-detection multitask trainer -- the reference's ``adapt_segbd_multitask_trainer.py`` (:24-291) on the
MI355X HIP kernels: stage-tap RGB encoder, two segmentation decoders + a HED-style boundary head trained on the boundaries of the
label map (no depth channel is needed), learned task weights.  Under data parallelism each rank balances its boundary loss with the
beta of its own batch, as the reference's local loss does.

    python adapt_segbd_multitask_trainer.py suncg nyu --input_ch 3 -b 8 --synthetic --no_pretrained
"""
from argmyparse import get_da_mcd_training_parser
from models.model_util import get_optimizer, get_segbd_multitask_models
from solvers.solver import SegBDMultiTaskMCDSolver
from trainer_common import Trainer, adapt_layout, criteria, mcd_report, parse_args, train


SEGBD_FLAGS = ("depth_shortcut", "semseg_shortcut", "add_pred_seg_boundary_loss", "use_seg2bd_conv", "boundary_loss_converging_epoch",
               "scale_bd_loss")


def get_parser():
    """the MCD training flags + the reference's six of this trainer (adapt_segbd_multitask_trainer.py:24-36)"""
    parser = get_da_mcd_training_parser()
    parser.add_argument('--depth_shortcut', action="store_true", help='whether you use depth shortcut')
    parser.add_argument('--semseg_shortcut', action="store_true", help='whether you use semseg shortcut')
    parser.add_argument('--add_pred_seg_boundary_loss', action="store_true", help='whether you use additional boundary loss')
    parser.add_argument('--use_seg2bd_conv', action="store_true", help='whether you use additional boundary loss')
    parser.add_argument('--boundary_loss_converging_epoch', type=int, default=5, help='epoch starting to include tgt boundary loss')
    parser.add_argument('--scale_bd_loss', type=int, default=1, help='epoch starting to include tgt boundary loss')
    return parser


def build(args):
    criterion, criterion_d = criteria(args)  # built before the models, which keep them as buffers
    model_enc, model_dec = get_segbd_multitask_models(net_name=args.net, input_ch=args.input_ch, n_class=args.n_class,
                                                      is_data_parallel=args.is_data_parallel, semseg_criterion=criterion,
                                                      discrepancy_criterion=criterion_d, depth_shortcut=args.depth_shortcut,
                                                      semseg_shortcut=args.semseg_shortcut,
                                                      add_pred_seg_boundary_loss=args.add_pred_seg_boundary_loss,
                                                      use_seg2bd_conv=args.use_seg2bd_conv)
    optimizer_enc = get_optimizer(model_enc.parameters(), lr=args.lr, momentum=args.momentum, opt=args.opt,
                                  weight_decay=args.weight_decay)
    optimizer_dec = get_optimizer(model_dec.parameters(), opt=args.opt, lr=args.lr, momentum=args.momentum,
                                  weight_decay=args.weight_decay)
    return ({"enc_state_dict": model_enc, "dec_state_dict": model_dec}, {"optimizer_enc": optimizer_enc, "optimizer_dec": optimizer_dec})


def make_step(args, run, modules, optimizers):
    enc, dec = (m.module if hasattr(m, "module") else m for m in modules.values())  # the solver takes the unwrapped modules
    solver = SegBDMultiTaskMCDSolver(enc, dec, *optimizers.values(), num_k=args.num_k, num_multiply_d_loss=args.num_multiply_d_loss,
                                     add_pred_seg_boundary_loss=args.add_pred_seg_boundary_loss,
                                     boundary_loss_converging_epoch=args.boundary_loss_converging_epoch, scale_bd_loss=args.scale_bd_loss)

    def step(src_imgs, src_gt, tgt_imgs, epoch):
        c_loss, d_loss, parts = solver.step(src_imgs, src_gt, tgt_imgs, epoch=epoch)
        return c_loss, d_loss, parts[0], parts[1], parts[2]
    return step


def report(epoch, sums, modules):
    mcd_report(epoch, sums, modules)
    print("SrcSemsegLoss: %.4f, SrcBoundaryLoss: %.4f  TgtPsuedoBoundaryLoss: %.4f"
          % (sums["src_semseg_loss"], sums["src_boundary_loss"], sums["tgt_psuedo_boundary_loss"]))


def on_resume(args, cli):
    args.epochs = cli.epochs  # (the pickled arguments replace the command line's, except the epoch count: :67-71)


TRAINER = Trainer(build=build, make_step=make_step, report=report, backfill=SEGBD_FLAGS, on_resume=on_resume,
                  sums=("c_loss", "d_loss", "src_semseg_loss", "src_boundary_loss", "tgt_psuedo_boundary_loss"),
                  layout=lambda args, resumed: adapt_layout(args, resumed, "_MCD_segbd_multitask"))


def main(argv=None):
    return train(TRAINER, parse_args(get_parser(), argv))


if __name__ == "__main__":
    main()
