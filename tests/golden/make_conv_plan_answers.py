#!/usr/bin/env python3
"""Characterisation table of the library's convolution plan queries (include/mcdseg.h), taken before the routes of a convolution pass
were gathered into one place per pass: for every geometry of make_conv_launch_table.py -- at its batch N, at 2 N, and as a half-batch
slice of a companion written for N images (``Ncb`` = N) -- under every ``math`` (0 / F16X3 / F16X1 / BF16X6), ``presplit`` and
``dgrad``, with the library options at their defaults and each value of OPTIONS alone:

  rows    mcdseg_conv_stat_rows, mcdseg_conv_split_stat_rows, _direct_ok; per math and presplit: _stat_rows_for, and per dgrad _window_ok
  tiles   mcdseg_conv_split_tile_config of the forward and the data-gradient GEMM, per presplit
  pp      per math: per presplit and dgrad mcdseg_conv_split_parts, _rest_pingpong, _wide_pingpong; per dgrad _pp_deep, _half_ok
  wgrad   mcdseg_conv_wgrad_workspace_bytes, _thin_tr_config; per math and presplit mcdseg_conv_wgrad_variant, _fits

Host arithmetic only: the built library, no tensor, no GPU (off the GPU the library plans for the MI355X's 256 CUs, so the table is the
same on both).  Only data is written (tests/golden/conv_plan_answers.json: (geometry, form) x setting -> a cell, a cell -> one index per
part of the record into the list of that part's distinct values); tests/test_cabi_and_host.py recomputes every cell with ``record``
below and asserts equality.
Run once:  python tests/golden/make_conv_plan_answers.py   (MCDSEG_LIB=<libmcdseg.so of another build> answers with that build)
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, ROOT, os.path.join(ROOT, "multichannel-semseg-with-uda_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

MATHS = (0, 3, 1, 6)  # mcdseg_conv_wgrad's f32 plans, MCDSEG_MATH_F16X3, _F16X1, _BF16X6
FORMS = ("N", "2N", "half")
OPTIONS = (("PINGPONG", (0, 1, 2, 4)), ("PP_CUS", (16, 64)), ("PP_MIN_ROUNDS", (1,)), ("PP_WIDE_FILL", (101,)), ("PP_WIDE128", (0,)),
           ("THIN_WINDOW", (0,)), ("BIGTILE_MIN_SLOTS", (1,)), ("WIDETILE_MIN_SLOTS", (1,)), ("WGRAD_PP", (0, 1)), ("WGRAD_PP3", (0,)),
           ("WGRAD_TR64", (0,)), ("WGRAD_THIN_TR", (0,)), ("WGRAD_BIG", (0,)), ("WGRAD_PP_CUS", (16,)))
KEYS = ("rows", "tiles", "pp", "wgrad")


def settings():
    """every {option: value} the table is taken under: the defaults, then each value of OPTIONS alone"""
    return [{}] + [{o: v} for o, values in OPTIONS for v in values]


def forms(ops, g):
    """the descriptors of one geometry: its batch, twice its batch, and the first half of its batch with the companions of the whole"""
    import make_conv_launch_table as table
    d = table.make_desc(ops, g)
    return [d, ops._sub_desc(d, 2 * d.N), ops._sub_desc(d, max(1, d.N // 2), d.N)]


def record(L, d):
    """every recorded answer for one descriptor under the library's current options"""
    r, both = ctypes.byref(d), ((0, 0), (0, 1), (1, 0), (1, 1))  # (presplit, dgrad)
    return {
        "rows": [L.mcdseg_conv_stat_rows(r), L.mcdseg_conv_split_stat_rows(r), L.mcdseg_conv_split_direct_ok(r),
                 [[[L.mcdseg_conv_split_stat_rows_for(r, m, p), L.mcdseg_conv_split_window_ok(r, m, p, 0), L.mcdseg_conv_split_window_ok(r, m, p, 1)]
                   for p in (0, 1)] for m in MATHS]],
        "tiles": [[L.mcdseg_conv_split_tile_config(d.Cout, d.N * d.Ho * d.Wo, p), L.mcdseg_conv_split_tile_config(d.Cin, d.N * d.H * d.W, p)]
                  for p in (0, 1)],
        "pp": [[[[L.mcdseg_conv_split_parts(r, m, p, g), L.mcdseg_conv_split_rest_pingpong(r, m, p, g), L.mcdseg_conv_split_wide_pingpong(r, m, p, g)]
                 for p, g in both], [[L.mcdseg_conv_split_pp_deep(r, m, g), L.mcdseg_conv_split_half_ok(r, m, g)] for g in (0, 1)]] for m in MATHS],
        "wgrad": [L.mcdseg_conv_wgrad_workspace_bytes(r), L.mcdseg_conv_wgrad_thin_tr_config(r),
                  [[[L.mcdseg_conv_wgrad_variant(r, m, p), L.mcdseg_conv_wgrad_fits(r, m, p)] for p in (0, 1)] for m in MATHS]],
    }


def lookup(table, row, si):
    """the stored record of row ``row`` (geometry * len(FORMS) + form) under setting ``si``"""
    return {k: table["pools"][k][i] for k, i in zip(table["keys"], table["cells"][table["table"][row][si]])}


def main():
    os.environ.setdefault("MCDSEG_PRETRAINED", "0")
    import mcdseg
    import make_conv_launch_table as launch_table
    from mcdseg import ops
    if not os.environ.get("MCDSEG_LIB"):
        mcdseg.build()
    L = ops.lib()
    geos, sets = launch_table.network_geometries(), settings()
    pools, index, cells, cell_index, table = {k: [] for k in KEYS}, {k: {} for k in KEYS}, [], {}, []
    for g in geos:
        for d in forms(ops, g):
            row = []
            for s in sets:
                with mcdseg.options(**s):
                    rec = record(L, d)
                cell = []
                for k in KEYS:  # each part of a record is stored once: most settings leave most parts as they are
                    text = json.dumps(rec[k])
                    if text not in index[k]:
                        index[k][text] = len(pools[k])
                        pools[k].append(rec[k])
                    cell.append(index[k][text])
                row.append(cell_index.setdefault(tuple(cell), len(cell_index)))
                if row[-1] == len(cells):
                    cells.append(cell)
            table.append(row)
    path = os.path.join(HERE, "conv_plan_answers.json")
    with open(path, "w") as fh:
        json.dump({"fields": list(launch_table.FIELDS), "geometries": geos, "forms": list(FORMS), "maths": list(MATHS), "settings": sets,
                   "keys": list(KEYS), "pools": pools, "cells": cells, "table": table}, fh, separators=(",", ":"), sort_keys=True)
    print("conv_plan_answers.json: %d geometries x %d forms x %d settings, %d distinct cells, %s distinct parts, %d bytes"
          % (len(geos), len(FORMS), len(sets), len(cells), {k: len(v) for k, v in pools.items()}, os.path.getsize(path)))


if __name__ == "__main__":
    main()
