#!/usr/bin/env python3
"""Ensemble saved predictions -- the reference's tools/ensemble_predict_from_npy.py with its command line, the arithmetic on the MI355X
(``ops.ensemble_probs`` + ``ops.label_resize_colorize``: DESIGN.md section 4.14).

    python tools/ensemble_predict_from_npy.py --npydirs D1 D2 [D3 ...] [--method {averaging,nms}] [-d OUT] [--mode {test,valid}]
                                              [--n_used K] [--out_shape W H] [--palette_json FILE] [--no_prob] [-b N]
                                              [--gt_dir DIR --n_class K]

reads ``<name>.npy`` (fp32 [C,H,W], what the testers write into ``prob/`` under ``--saves_prob``) from every directory -- the names are
those of the first one; a name missing elsewhere, or a map of another shape, is an error -- and writes ``OUT/prob/<name>.npy`` (the mean,
or the maximum for ``nms``), ``OUT/label/<name>.png`` (the arg-max) and ``OUT/vis/<name>.png`` (its palette image).  What the reference
fixes for its own data is an option here: ``--n_used`` takes the arg-max over all classes unless given (the reference over the first 19,
:14), ``--out_shape`` keeps the maps' size unless given -- ``--mode``, when it is passed, gives the reference's 1280 x 720 (test) or
2048 x 1024 (valid) (:69) -- and ``--palette_json`` names a ``{"palette": [[r,g,b],...]}`` file in place of the PASCAL-VOC colours of
``n_used + 1`` labels.  ``--no_prob`` leaves ``prob/`` out.  With ``--gt_dir`` (label PNGs of the same names at the size of the written
PNGs, background 255) ``OUT/eval_result_ensemble.json`` = {"members": [...], "ensemble": ...} is written.

The loop keeps the device and the disks busy together: the maps of batch i + 1 are read into pinned buffers and uploaded on a second
stream while the kernels of batch i run, and the PNG / npy files of batch i are written by a thread that waits for nothing but the
event behind that batch's download."""
import argparse
import os
import queue
import sys
import threading

import numpy as np

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if sys.path[:1] != [PKG]:  # in FRONT of this file's own directory: ``import ensemble`` below is the package's module
    sys.path.insert(0, PKG)

MODE_SHAPES = {"test": (1280, 720), "valid": (2048, 1024)}  # ensemble_predict_from_npy.py:69, (W, H)


def get_parser():
    parser = argparse.ArgumentParser(description="Ensemble predict")
    parser.add_argument("--npydirs", type=str, nargs="+", required=True, help="result directories that contain probability npys")
    parser.add_argument("--method", default="averaging", choices=["averaging", "nms"], help='"averaging" or "nms"')
    parser.add_argument("-d", "--out_directory", default="ensemble_results")
    parser.add_argument("--mode", default=None, choices=["test", "valid"], help="the reference's output sizes: 1280 x 720 / 2048 x 1024")
    parser.add_argument("--n_used", type=int, default=None, help="arg-max over the first K classes (default: all)")
    parser.add_argument("--out_shape", default=None, nargs=2, type=int, help="W H of the PNGs (default: the maps' size)")
    parser.add_argument("--palette_json", type=str, default=None, help='a {"palette": [[r,g,b],...]} file (default: PASCAL-VOC colours)')
    parser.add_argument("--no_prob", action="store_true", help="do not save the combined maps")
    parser.add_argument("-b", "--batch_size", type=int, default=1, help="images of equal size combined per call")
    parser.add_argument("--gt_dir", type=str, default=None, help="ground-truth label PNGs: also write eval_result_ensemble.json")
    parser.add_argument("--n_class", type=int, default=None, help="number of classes of the evaluation (with --gt_dir)")
    return parser


def check_args(args):
    """the refusals that need no file and no device"""
    if len(args.npydirs) < 2:
        raise SystemExit("--npydirs needs at least two directories")
    if len(args.npydirs) > 16:
        raise SystemExit("--npydirs takes at most 16 directories")
    if args.gt_dir is not None and (args.n_class is None or args.n_class <= 0):
        raise SystemExit("--gt_dir needs --n_class")
    if args.batch_size <= 0:
        raise SystemExit("--batch_size must be positive")
    if args.n_used is not None and not 1 <= args.n_used <= 256:
        raise SystemExit("--n_used must lie in 1..256")
    if args.out_shape is not None and min(args.out_shape) <= 0:
        raise SystemExit("--out_shape must be positive")
    if args.out_shape is not None and args.mode is not None:
        raise SystemExit("--out_shape and --mode both set the size of the PNGs: pass one")
    return MODE_SHAPES[args.mode] if args.mode is not None else (None if args.out_shape is None else tuple(args.out_shape))


def list_names(npydirs):
    """the names (without ".npy") of the first directory, sorted; each must exist in every other one"""
    names = sorted(f[:-4] for f in os.listdir(npydirs[0]) if f.endswith(".npy"))
    for d in npydirs[1:]:
        for name in names:
            if not os.path.isfile(os.path.join(d, name + ".npy")):
                raise FileNotFoundError("%s is missing: every directory must hold the maps of %s" % (os.path.join(d, name + ".npy"), npydirs[0]))
    return names


def load_member_maps(npydirs, name, n_used=None):
    """the K maps of one name as fp32 [C,H,W] arrays; a shape that differs from the first directory's is an error that names the file"""
    maps = []
    for d in npydirs:
        fn = os.path.join(d, name + ".npy")
        z = np.load(fn)
        if z.ndim != 3:
            raise ValueError("%s holds an array of shape %s, not a map [C,H,W]" % (fn, z.shape))
        if maps and z.shape != maps[0].shape:
            raise ValueError("%s holds a map of shape %s, %s one of shape %s" % (fn, z.shape, os.path.join(npydirs[0], name + ".npy"),
                                                                                 maps[0].shape))
        if n_used is not None and n_used > z.shape[0]:
            raise ValueError("--n_used %d exceeds the %d classes of %s" % (n_used, z.shape[0], fn))
        maps.append(np.ascontiguousarray(z, dtype=np.float32))
    return maps


class _Slot(object):
    """what one batch in flight owns: pinned staging and device buffers of the K maps, pinned buffers of the results, and the events
    that say when each may be touched again"""

    def __init__(self, torch, dev):
        self.torch, self.dev = torch, dev
        self.shape = None
        self.uploaded = self.consumed = self.downloaded = None
        self.written = threading.Event()
        self.written.set()

    def fit(self, k, shape, out_hw, want_prob, want_gt):
        """buffers for K maps [B,C,H,W]; called only when nothing of the slot is in flight.  True when device buffers were allocated:
        they come from the current stream's pool and may be blocks that stream has only just released, so whichever other stream
        writes them first has to wait for the current one"""
        torch = self.torch
        key = (k, tuple(shape), tuple(out_hw), want_prob, want_gt)
        if key == self.shape:
            return False
        self.shape = key
        self.host = [torch.empty(shape, dtype=torch.float32, pin_memory=True) for _ in range(k)]
        self.maps = [torch.empty(shape, dtype=torch.float32, device=self.dev) for _ in range(k)]
        b = shape[0]
        self.labels = torch.empty((b,) + tuple(out_hw), dtype=torch.uint8, pin_memory=True)
        self.vis = torch.empty((b,) + tuple(out_hw) + (3,), dtype=torch.uint8, pin_memory=True)
        self.prob = torch.empty(shape, dtype=torch.float32, pin_memory=True) if want_prob else None
        self.gt_host = torch.empty((b,) + tuple(out_hw), dtype=torch.uint8, pin_memory=True) if want_gt else None
        self.gt = torch.empty((b,) + tuple(out_hw), dtype=torch.uint8, device=self.dev) if want_gt else None
        return True


def main(argv=None):
    args = get_parser().parse_args(argv)
    out_shape = check_args(args)
    names = list_names(args.npydirs)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this tool runs on an MI355X: the HIP kernels are the only implementation (no CPU fallback)")
    from PIL import Image
    import ensemble
    dev = torch.device("cuda", torch.cuda.current_device())
    palette = ensemble.load_palette(args.palette_json) if args.palette_json else None
    ens = ensemble.Ensemble(args.out_directory, args.method, args.n_used, out_shape, palette, not args.no_prob, args.n_class, dev)
    print("- npy_directory_list\n%s\n- method\n%s\n- out_shape\n%s\n%d" % (args.npydirs, args.method, out_shape or "the maps'", len(names)))
    print("Ensembling ...")

    k = len(args.npydirs)
    main_stream, up_stream = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
    slots = [_Slot(torch, dev), _Slot(torch, dev)]
    jobs, failure = queue.Queue(), []

    def writer():
        while True:
            job = jobs.get()
            if job is None:
                return
            slot, batch_names = job
            try:
                if not failure:
                    slot.downloaded.synchronize()  # this batch's results are on the host; the device is already at the next batch
                    n = len(batch_names)
                    ens.save(batch_names, slot.labels.numpy()[:n], slot.vis.numpy()[:n], None if slot.prob is None else slot.prob.numpy()[:n])
            except BaseException as e:  # noqa: B902 -- handed to the main thread, which raises it
                failure.append(e)
            finally:
                slot.written.set()

    thread = threading.Thread(target=writer, name="ensemble-writer", daemon=True)
    thread.start()

    def run(slot, batch):
        """batch: [(name, [K maps], gt or None)] of one shape.  Host work first (it overlaps the previous batch on the device), then
        the upload (maps and ground truth, from pinned buffers) on the second stream, the kernels and the download on the main one.
        The host waits for the device only where this slot's own buffers are re-used, two batches back, or re-made for another shape;
        the second stream waits for the kernels that last read the device buffers it is about to overwrite and, when those buffers
        are new, for everything the main stream had queued when they were allocated (their memory may be a block it just released)."""
        slot.written.wait()
        if failure:
            return
        c, h, w = batch[0][1][0].shape
        out_hw = (h, w) if out_shape is None else (out_shape[1], out_shape[0])
        key = (k, (args.batch_size, c, h, w), out_hw, not args.no_prob, args.gt_dir is not None)
        if key != slot.shape and slot.consumed is not None:
            slot.consumed.synchronize()
        if slot.fit(*key):
            up_stream.wait_stream(main_stream)
        if slot.uploaded is not None:
            slot.uploaded.synchronize()  # the pinned staging buffers are free again (two batches back: long done)
        n = len(batch)
        for j in range(k):
            staged = slot.host[j].numpy()
            for i, item in enumerate(batch):
                staged[i] = item[1][j]
        if slot.gt is not None:
            staged = slot.gt_host.numpy()
            for i, item in enumerate(batch):
                staged[i] = item[2]
        with torch.cuda.stream(up_stream):
            if slot.consumed is not None:
                up_stream.wait_event(slot.consumed)  # the kernels that read these device buffers two batches back
            for j in range(k):
                slot.maps[j][:n].copy_(slot.host[j][:n], non_blocking=True)
            if slot.gt is not None:
                slot.gt[:n].copy_(slot.gt_host[:n], non_blocking=True)
            slot.uploaded = up_stream.record_event()
        main_stream.wait_event(slot.uploaded)
        maps = [m[:n] for m in slot.maps]
        prob, labels, vis = ens.combine(maps)
        if slot.gt is not None:
            ens.update([ens.member_labels(m) for m in maps], labels, slot.gt[:n])
        slot.consumed = main_stream.record_event()
        slot.labels[:n].copy_(labels, non_blocking=True)
        slot.vis[:n].copy_(vis, non_blocking=True)
        if prob is not None:
            slot.prob[:n].copy_(prob, non_blocking=True)
        slot.downloaded = main_stream.record_event()
        slot.written.clear()
        jobs.put((slot, [item[0] for item in batch]))

    batch, count = [], 0
    try:
        for name in names:
            maps = load_member_maps(args.npydirs, name, args.n_used)
            gt = None
            if args.gt_dir is not None:
                c, h, w = maps[0].shape
                ow, oh = out_shape or (w, h)
                gt = np.array(Image.open(os.path.join(args.gt_dir, name + ".png")))
                if gt.shape != (oh, ow) or gt.dtype != np.uint8:
                    raise ValueError("ground truth %s is not an 8-bit %d x %d label image" % (os.path.join(args.gt_dir, name + ".png"), ow, oh))
            if batch and (len(batch) >= args.batch_size or batch[0][1][0].shape != maps[0].shape):
                run(slots[count % 2], batch)
                count += 1
                batch = []
            batch.append((name, maps, gt))
            if failure:
                break
        if batch and not failure:
            run(slots[count % 2], batch)
    finally:
        jobs.put(None)
        thread.join()
    if failure:
        raise failure[0]
    ens.finish()
    print("Finished!!!")
    return args.out_directory


if __name__ == "__main__":
    main()
