"""The cost of symmetry-randomised evaluation (evaluation_symmetry="random"), whole self-play runs played to completion on one
GPU -> profiles/evaluation_symmetry.json.

Default workload: config 2 -- 8x8, 800 simulations, f16x3, 128x10 net, 4 096 games in two lockstep lanes.  Legs: the engine
defaults (evaluation reuse on) and evaluation reuse off; in each the option off and on alternate inside one process, and every
figure is the median of --repeats runs.  Reported per leg and setting: positions/s over the whole run and evaluator rows per
move (rows the evaluator was asked for / positions searched).  The games differ between off and on (the network is not
equivariant), so the rows per move differ a little too; no claim about playing strength is made.

    python tools/evaluation_symmetry.py                                  # both legs (many minutes)
    python tools/evaluation_symmetry.py --legs reuse_off --out profiles/evaluation_symmetry.reuse_off.json
    python tools/evaluation_symmetry.py --merge a.json b.json --out profiles/evaluation_symmetry.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def merge(paths, out):
    docs = [json.load(open(p)) for p in paths]
    doc = dict(workload=docs[0]["workload"], median={}, runs={})
    for d in docs:
        assert d["workload"] == doc["workload"], "the parts were measured on different workloads"
        doc["median"].update(d["median"])
        doc["runs"].update(d["runs"])
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc["median"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--cols", type=int, default=8)
    ap.add_argument("--simulations", type=int, default=800)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--legs", default="defaults,reuse_off")
    ap.add_argument("--merge", nargs="+", default=None, help="join the files of runs made leg by leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluation_symmetry.json"))
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    import torch
    import yinyang_game_alphazero_amd as pkg

    torch.cuda.set_device(0)
    game = pkg.YinYangGame(args.rows, args.cols)
    torch.manual_seed(0)
    ev = pkg.BatchedEvaluator(pkg.YinYangNeuralNetwork(game, args.channels, args.blocks).cuda().eval(), "f16x3")
    legs = {"defaults": {}, "reuse_off": dict(reuse_pass_value=False, reuse_transpositions=False, keep_evaluations=False)}
    runs = {}
    for rep in range(args.repeats):
        for name in args.legs.split(","):
            for mode in ("off", "random"):
                eng = pkg.SelfPlayLanes(game, ev, num_simulations=args.simulations, concurrent_games=args.games, lanes=args.lanes,
                                        seed=1000 + rep, **legs[name], **(dict(evaluation_symmetry=mode) if mode != "off" else {}))
                eng.ctx.reset_counters()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.run(args.games)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                ctr = eng.ctx.status()
                rec = dict(seconds=dt, positions=eng.positions, games=eng.games_finished, positions_per_s=eng.positions / dt,
                           evaluator_rows=ctr["evals"], rows_per_move=ctr["evals"] / max(1, eng.positions),
                           cache_and_book_hits=ctr["transposition_hits"])
                runs.setdefault(f"{name}/{mode}", []).append(rec)
                print(name, mode, json.dumps(rec), flush=True)
                eng.close()
    median = {k: {f: statistics.median(r[f] for r in v) for f in v[0]} for k, v in runs.items()}
    out = dict(workload=dict(board=f"{args.rows}x{args.cols}", games=args.games, lanes=args.lanes, simulations=args.simulations,
                             net=f"{args.channels}x{args.blocks}", nn="f16x3", repeats=args.repeats,
                             device=torch.cuda.get_device_name(0)), median=median, runs=runs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(median, indent=1))


if __name__ == "__main__":
    main()
