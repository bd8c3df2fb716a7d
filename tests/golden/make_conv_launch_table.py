#!/usr/bin/env python3
"""Characterisation table of the layer of mcdseg/ops.py that turns one convolution into library launches: for every convolution of
drn_d_38 at BASELINE config 2 (N = 16, 6 x 480 x 640) and of drn_d_105 at config 5 (N = 16 and 32, 6 x 720 x 1280), the heads and a few
thin / stem / forced-cut geometries, under every arithmetic, ``MAX_CONV_BYTES`` at its default and at a small value that forces cuts,
and the library options WGRAD_TR64 / WGRAD_THIN_TR / WGRAD_PP_DEEP each off and on:

  pieces        ``_batch_pieces(desc)``, ``(desc, False)``, ``(desc, True)`` and ``_batch_pieces_half(desc)``
  wgrad         per ``have_cb``: ``_wgrad_split_plan``, and the kernel name of every launch as ``_conv_wgrad`` gives it to its timer
  thin_tr, reads_cb   ``_wgrad_thin_tr(desc)``, ``_wgrad_reads_cb(desc)``
  fprop, dgrad  per form (fp32 operands / pre-split companion / the 2-byte chain, where the form applies): every timed kernel of
                every launch as ``_split_launches`` brackets it -- [name, part handed to the entry point, FLOPs, bytes]

Host arithmetic and the library's plan queries only: the built library, no tensor, no GPU.  Only data is written
(tests/golden/conv_launch_table.json: geometries x settings -> a cell, a cell -> one index per part of the record into the list of that part's
distinct values);
tests/test_cabi_and_host.py recomputes every cell with ``record`` below and asserts equality.
Run once:  python tests/golden/make_conv_launch_table.py
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "multichannel-semseg-with-uda_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

MATHS = ("f16x3", "bf16x6", "f16x1", "f32")
SMALL_MAX_BYTES = 1 << 28
OPTIONS = ("WGRAD_TR64", "WGRAD_THIN_TR", "WGRAD_PP_DEEP")
FIELDS = ("N", "Cin", "H", "W", "Cout", "KH", "stride", "pad", "dil")
EXTRA = [  # (N, Cin, H, W, Cout, k, stride, dil): thin layers past one launch, the stem, the heads, a small layer the small limit cuts
    (40, 16, 720, 1280, 16, 3, 1, 1), (36, 16, 720, 1280, 16, 3, 1, 1), (35, 16, 720, 1280, 16, 3, 1, 1), (32, 16, 720, 1280, 32, 3, 2, 1),
    (64, 16, 720, 1280, 32, 1, 2, 1), (2, 6, 64, 96, 16, 7, 1, 1), (2, 16, 64, 96, 16, 3, 1, 1), (2, 16, 64, 96, 32, 3, 2, 1),
    (16, 512, 60, 80, 41, 1, 1, 1), (32, 512, 90, 160, 41, 1, 1, 1), (64, 2048, 90, 160, 512, 1, 1, 1), (5, 128, 32, 32, 128, 3, 1, 1),
    (5, 24, 33, 35, 40, 3, 1, 1), (3, 48, 17, 19, 256, 1, 1, 1),
]


def settings():
    """every (arithmetic, MAX_CONV_BYTES or None for the default, {option: value}) the table is taken under"""
    opts = [{}] + [{o: v} for o in OPTIONS for v in (0, 1)]
    return [dict(math=m, max_bytes=b, options=o) for m in MATHS for b in (None, SMALL_MAX_BYTES) for o in opts]


class applied:
    """``with applied(ops, setting):`` the module switches and library options of one setting, restored afterwards"""

    def __init__(self, ops, setting):
        self.ops, self.setting = ops, setting

    def __enter__(self):
        import mcdseg
        ops, s = self.ops, self.setting
        self.saved = (ops.CONV_MATH, ops.MAX_CONV_BYTES, ops.LAUNCH_TIMER)
        ops.CONV_MATH = s["math"]
        if s["max_bytes"] is not None:
            ops.MAX_CONV_BYTES = s["max_bytes"]
        self.prev = {k: mcdseg.set_option(k, v) for k, v in s["options"].items()}

    def __exit__(self, *exc):
        import mcdseg
        self.ops.CONV_MATH, self.ops.MAX_CONV_BYTES, self.ops.LAUNCH_TIMER = self.saved
        for k, v in self.prev.items():
            mcdseg.set_option(k, v)


class _Recorder:
    """a launch timer that times nothing: it writes down the name and the work of every kernel the drivers would bracket"""

    def __init__(self):
        self.seen = []

    def wants(self, name):
        self.seen.append(name)
        return False


def geometry(desc):
    return [getattr(desc, f) for f in FIELDS]


def make_desc(ops, g):
    n, cin, h, w, cout, k, stride, pad, dil = g
    return ops.conv_desc((n, cin, h, w), (cout, cin, k, k), stride, pad, dil)


def _runs(launches):
    """[[count, launch]] of a list of launches: the pieces of a cut batch are alike but for the last"""
    out = []
    for x in launches:
        if out and out[-1][1] == x:
            out[-1][0] += 1
        else:
            out.append([1, x])
    return out


def _launch_descs(ops, desc, pieces, ncb):
    return [(a, b, desc if (a, b) == (0, desc.N) else ops._sub_desc(desc, b - a, ncb)) for a, b in pieces]


def _timed_kernels(ops, d, presplit, dgrad, name, work=None):
    """[name, part, FLOPs, bytes] of every kernel ``_split_launches`` brackets for one launch"""
    rec, parts, works = ops.LAUNCH_TIMER, [], []
    first = len(rec.seen)
    real_timed = ops._timed

    class timed(real_timed):
        def __init__(self, name, work):
            real_timed.__init__(self, name, work)
            works.append(work)
    ops._timed = timed
    try:
        ops._split_launches(d, presplit, dgrad, name, parts.append, *(() if work is None else (work,)))
    finally:
        ops._timed = real_timed
    names = rec.seen[first:]
    assert len(names) == len(parts) == len(works)
    return [[n, p, w[0], w[1]] for n, p, w in zip(names, parts, works)]


def _conv_names(ops, desc, dgrad, presplit, half):
    """the timed kernels of one forward pass (data gradient) as ``_conv_fprop`` / ``_conv_fprop_half`` (``_conv_dgrad`` / ``_conv_dgrad_half``)
    launch it: per launch, the list of ``_timed_kernels`` -- or the one f32 kernel -- as ``_runs``"""
    L = ops.lib()
    m, k = (desc.Cin, desc.Cout) if dgrad else (desc.Cout, desc.Cin)
    direct = bool(not dgrad and ops.CONV_MATH in ops.MATH_ID and L.mcdseg_conv_split_direct_ok(ctypes.byref(desc)))
    split = ops._use_split(k) or direct
    out = []
    if half:
        for a, b, d in _launch_descs(ops, desc, ops._batch_pieces_half(desc), desc.N):
            pixels = d.N * (d.H * d.W if dgrad else d.Ho * d.Wo)
            out.append(_timed_kernels(ops, d, True, dgrad, ops.gemm_kernel_name(m, k, dgrad, True, True, False, pixels), ops.half_conv_work))
        return _runs(out)
    for a, b, d in _launch_descs(ops, desc, ops._batch_pieces(desc), desc.N if presplit else 0):
        pixels = d.N * (d.H * d.W if dgrad else d.Ho * d.Wo)
        name = (ops._window_name(d, presplit, dgrad) if split else None) or ops.gemm_kernel_name(m, k, dgrad, split, presplit, direct, pixels)
        out.append(_timed_kernels(ops, d, presplit, dgrad, name) if split else [[name, None] + list(ops.conv_work(d))])
    return _runs(out)


def _wgrad_names(ops, desc, have_cb):
    """the kernel name of every launch of ``_conv_wgrad``, as ``_runs``"""
    pieces = ops._batch_pieces(desc, wgrad_cb=have_cb)
    if have_cb and len(pieces) > 1 and desc.Cin <= 16:  # (the thin window kernel takes whole batches only)
        have_cb, pieces = False, ops._batch_pieces(desc, wgrad_cb=False)
    split = bool(ops._wgrad_split_plan(desc, have_cb))
    return _runs([ops.wgrad_split_kernel_name(d, have_cb) if split else ops.wgrad_kernel_name(desc.Cout, desc.Cin, desc.KH * desc.KW)
                  for a, b, d in _launch_descs(ops, desc, pieces, desc.N if have_cb else 0)])


def record(ops, desc):
    """every recorded value of one geometry under the module's current switches (``applied``)"""
    L = ops.lib()
    ops.LAUNCH_TIMER = _Recorder()
    lists = lambda pieces: [list(p) for p in pieces]  # noqa: E731  (as JSON gives them back)
    math = ops.MATH_ID.get(ops.CONV_MATH, 0)
    both8 = desc.Cin % 8 == 0 and desc.Cout % 8 == 0
    out = {"pieces": {"conv": lists(ops._batch_pieces(desc)), "wgrad": lists(ops._batch_pieces(desc, False)),
                      "wgrad_cb": lists(ops._batch_pieces(desc, True)), "half": lists(ops._batch_pieces_half(desc))},
           "thin_tr": bool(ops._wgrad_thin_tr(desc)), "reads_cb": bool(ops._wgrad_reads_cb(desc)), "wgrad": {}, "fprop": {}, "dgrad": {}}
    for have_cb in (False, True):
        if have_cb and not (math and (both8 or desc.Cin <= 16)):  # (companions exist in the split arithmetics; the stem's input is padded)
            continue
        out["wgrad"]["cb" if have_cb else "fp32"] = {"split_plan": bool(ops._wgrad_split_plan(desc, have_cb)), "names": _wgrad_names(ops, desc, have_cb)}
    for dgrad, key in ((False, "fprop"), (True, "dgrad")):
        out[key]["fp32"] = _conv_names(ops, desc, dgrad, False, False)
        if ops._cb_wanted(desc.Cout if dgrad else desc.Cin):
            out[key]["cb"] = _conv_names(ops, desc, dgrad, True, False)
        if math and L.mcdseg_conv_split_half_ok(ctypes.byref(desc), math, int(dgrad)):
            out[key]["half"] = _conv_names(ops, desc, dgrad, True, True)
    return out


KEYS = ("pieces", "wgrad", "fprop", "dgrad")


def split_record(rec):
    """a record as the table stores it: one part per key of KEYS (the weight gradient's three predicates in one part)"""
    return {"pieces": rec["pieces"], "wgrad": [rec["thin_tr"], rec["reads_cb"], rec["wgrad"]], "fprop": rec["fprop"], "dgrad": rec["dgrad"]}


def lookup(table, gi, si):
    """the stored record of geometry ``gi`` under setting ``si``, in ``split_record``'s form"""
    return {k: table["pools"][k][i] for k, i in zip(table["keys"], table["cells"][table["table"][gi][si]])}


def network_geometries():
    """descriptor fields of every convolution of the two trunks (walked on meta tensors with a shape-only ``conv_bn_act``), the heads
    and EXTRA: distinct ones, in order of appearance"""
    import torch
    from mcdseg import ops
    from models import drn
    from models.dilated_fcn import Trunk
    seen = []

    def group(x, conv, bn, relu=True, residual=None, **kw):
        desc = ops.conv_desc(x.shape, conv.weight.shape, conv.stride[0], conv.padding[0], conv.dilation[0])
        seen.append(geometry(desc))
        return torch.empty((desc.N, desc.Cout, desc.Ho, desc.Wo), device="meta", requires_grad=True)
    real, ops.conv_bn_act = ops.conv_bn_act, group
    try:
        for net, n, h, w in (("drn_d_38", 16, 480, 640), ("drn_d_105", 16, 720, 1280), ("drn_d_105", 32, 720, 1280)):
            Trunk(*getattr(drn, net)(input_ch=6, num_classes=0).trunk()).train()(torch.empty((n, 6, h, w), device="meta"))
    finally:
        ops.conv_bn_act = real
    for n, cin, h, w, cout, k, stride, dil in EXTRA:
        seen.append([n, cin, h, w, cout, k, stride, dil * (k // 2), dil])
    return [g for i, g in enumerate(seen) if g not in seen[:i]]


def main():
    os.environ.setdefault("MCDSEG_PRETRAINED", "0")
    import mcdseg
    from mcdseg import ops
    mcdseg.build()
    geos, sets = network_geometries(), settings()
    pools, index, cells, cell_index, table = {k: [] for k in KEYS}, {k: {} for k in KEYS}, [], {}, []
    for g in geos:
        row = []
        for s in sets:
            with applied(ops, s):
                rec = split_record(record(ops, make_desc(ops, g)))
            cell = []
            for k in KEYS:  # each part of a record is stored once: most settings leave most parts as they are
                text = json.dumps(rec[k], sort_keys=True)
                if text not in index[k]:
                    index[k][text] = len(pools[k])
                    pools[k].append(json.loads(text))
                cell.append(index[k][text])
            row.append(cell_index.setdefault(tuple(cell), len(cell_index)))
            if row[-1] == len(cells):
                cells.append(cell)
        table.append(row)
    path = os.path.join(HERE, "conv_launch_table.json")
    with open(path, "w") as fh:
        json.dump({"fields": list(FIELDS), "geometries": geos, "settings": sets, "keys": list(KEYS), "pools": pools, "cells": cells, "table": table},
                  fh, separators=(",", ":"), sort_keys=True)
    print("conv_launch_table.json: %d geometries x %d settings, %d distinct cells, %s distinct parts, %d bytes"
          % (len(geos), len(sets), len(cells), {k: len(v) for k, v in pools.items()}, os.path.getsize(path)))


if __name__ == "__main__":
    main()
