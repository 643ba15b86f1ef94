#!/usr/bin/env python3
"""Two builds of csrc/yy_tower_g.hip (tools/tg_variants.py build DIR parent=OLD.hip: libtg_base.so = this tree, libtg_parent.so =
the parent revision) on the headline launch of the 8x8 evaluator, 128x10, two boards per workgroup, 2x2 wave grid, head
convolutions fused, interleaved in ONE process: the dense 4096-board launch and a compacted launch of 1 883 gathered rows.
    python tools/tower_edge_ab.py DIR [out.json]        bits of both launches, then 10 samples of 20 launches per build and shape,
                                                        rounds alternate the order of the builds
    python tools/tower_edge_ab.py DIR --one NAME N      N dense launches of libtg_NAME.so (for a rocprofv3 --pmc pass)"""
import ctypes as ct
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from tower_grid_ab import G, LIVE, setup, timed

VP = ct.c_void_p


def load(lib_dir, name):
    L = ct.CDLL(os.path.join(lib_dir, "libtg_%s.so" % name))
    L.yy_nn_tower_g.argtypes = [VP] * 9 + [ct.c_int] * 13 + [VP]
    return L


def launcher(L, ev, planes, out, rows=None, n=None):
    p = lambda t: None if t is None else VP(t.data_ptr())
    args = (p(planes), p(ev.g_w), p(ev.g_hw), p(ev.g_b), p(ev.g_hb), None, p(out), p(rows), p(n), G, 8, 8, 128, ev.h3_layers,
            int(ev.g_exps[0]), int(ev.g_exps[1]), int(ev.g_exps[2]), 8, 2, -1, 0x7FFFFFFF, 0)

    def fn():
        assert L.yy_nn_tower_g(*args, VP(torch.cuda.current_stream().cuda_stream)) == 0
    return fn


def main():
    lib_dir = sys.argv[1]
    ev, planes, rows, n, out = setup()
    if sys.argv[2:3] == ["--one"]:
        fn = launcher(load(lib_dir, sys.argv[3]), ev, planes, out)
        print(json.dumps({"build": sys.argv[3], "us_per_launch": timed(fn, int(sys.argv[4]))}))
        return
    builds = ("parent", "base")
    libs = {b: load(lib_dir, b) for b in builds}
    shapes = {"dense_4096": (), "compacted_1883": (rows, n)}
    res = {"board": "8x8", "net": "128x10", "form": [8, 2], "kernel": "k_tower_g22<3>", "rounds": 10, "launches_per_sample": 20,
           "same_bits": {}, "us": {}}
    for shape, extra in shapes.items():
        outs = {}
        for b in builds:
            o = torch.full_like(out, -7.0)
            launcher(libs[b], ev, planes, o, *extra)()
            torch.cuda.synchronize()
            outs[b] = o[:LIVE] if extra else o
        res["same_bits"][shape] = bool(torch.equal(outs["parent"].view(torch.int32), outs["base"].view(torch.int32)))
    cases = {(shape, b): launcher(libs[b], ev, planes, out, *extra) for shape, extra in shapes.items() for b in builds}
    ts = {k: [] for k in cases}
    for rnd in range(10):
        for shape in shapes:
            for b in (builds if rnd % 2 == 0 else builds[::-1]):
                ts[(shape, b)].append(timed(cases[(shape, b)], 20))
    for shape in shapes:
        rec = {b: {"median": float(np.median(ts[(shape, b)])), "min": float(np.min(ts[(shape, b)])), "max": float(np.max(ts[(shape, b)])),
                   "samples": [round(x, 1) for x in ts[(shape, b)]]} for b in builds}
        rec["speedup_median"] = rec["parent"]["median"] / rec["base"]["median"]
        rec["base_median_below_parent_min"] = rec["base"]["median"] < rec["parent"]["min"]
        res["us"][shape] = rec
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 2:
        json.dump(res, open(sys.argv[2], "w"), indent=1)


if __name__ == "__main__":
    main()
