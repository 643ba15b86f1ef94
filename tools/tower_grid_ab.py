#!/usr/bin/env python3
"""The split-f16 tower at 8x8, 128x10, large form (8 row-aligned column blocks, two boards): the 2x2 wave grid (k_tower_g22, the
kernel's own choice) against one wave per 32-channel slice (k_tower_g<4,8,9,true>, engine.tower_g(..., wave_grid=False)),
interleaved in ONE process.  Times the dense 4096-board launch and a compacted launch of 1 883 gathered rows (one lane's rows per
simulation step of the headline), head convolutions fused, as the evaluator launches them.
    python tools/tower_grid_ab.py [out.json]              A/B timing, rounds alternate the order of the two kernels
    python tools/tower_grid_ab.py --one grid|slices N     N dense launches of one kernel (for a rocprofv3 --pmc pass)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import yinyang_game_alphazero_amd as pkg
from yinyang_game_alphazero_amd import engine as E

G, LIVE = 4096, 1883


def setup():
    torch.manual_seed(0)
    net = pkg.YinYangNeuralNetwork(pkg.YinYangGame(8, 8), 128, 10).cuda().eval()
    ev = pkg.BatchedEvaluator(net, "f16x3")
    assert ev.g_big == (8, 2)
    rng = np.random.default_rng(0)
    planes = E.encode_planes(torch.from_numpy(rng.integers(-1, 2, size=(G, 8, 8)).astype(np.int8)).cuda())
    flags = torch.zeros(G, dtype=torch.uint8, device="cuda")
    flags[torch.from_numpy(rng.choice(G, LIVE, replace=False)).cuda()] = 1
    rows, n = E.compact_rows(flags)
    assert int(n) == LIVE
    out = torch.empty((G, 2, 2048), dtype=torch.float32, device="cuda")
    return ev, planes, rows, n, out


def launcher(ev, planes, out, grid, rows=None, n=None):
    return lambda: E.tower_g(planes, ev.g_w, ev.g_b, ev.h3_layers, ev.g_exps, 8, 2, ev.g_hw, ev.g_hb, rows, n, out,
                             wave_grid=grid)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps * 1e3          # us per launch


def main():
    ev, planes, rows, n, out = setup()
    if sys.argv[1:2] == ["--one"]:
        fn = launcher(ev, planes, out, sys.argv[2] == "grid")
        print(json.dumps({"kernel": sys.argv[2], "us_per_launch": timed(fn, int(sys.argv[3]))}))
        return
    cases = {(shape, kern): launcher(ev, planes, out, kern == "grid", *((rows, n) if shape == "compacted_1883" else ()))
             for shape in ("dense_4096", "compacted_1883") for kern in ("grid", "slices")}
    ts = {k: [] for k in cases}
    for rnd in range(10):
        for shape in ("dense_4096", "compacted_1883"):
            order = ("grid", "slices") if rnd % 2 == 0 else ("slices", "grid")
            for kern in order:
                ts[(shape, kern)].append(timed(cases[(shape, kern)], 20))
    res = {"board": "8x8", "net": "128x10", "form": [8, 2], "rounds": 10, "launches_per_sample": 20, "us": {}}
    for shape in ("dense_4096", "compacted_1883"):
        rec = {kern: {"median": float(np.median(ts[(shape, kern)])), "min": float(np.min(ts[(shape, kern)])),
                      "max": float(np.max(ts[(shape, kern)])), "samples": [round(x, 1) for x in ts[(shape, kern)]]}
               for kern in ("grid", "slices")}
        rec["speedup_median"] = rec["slices"]["median"] / rec["grid"]["median"]
        res["us"][shape] = rec
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        json.dump(res, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
