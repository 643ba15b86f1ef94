"""The cost of the Gumbel search options in the tree step -- with everything off against the parent commit, with gumbel_root
and with gumbel_root + gumbel_interior -> profiles/gumbel_interior.json.

Per-step timing.  2 048 slots, hash evaluator: the fused yy_mcts_step on the live trees of a search, a pair of events around
every launch, the mean over the launches after the first few, with the selection levels walked per descent beside it.  For every
board of --boards (8x8: one edge word; 9x12: two, where the tree kernel's occupancy differs from the parent's) and every budget
of --budgets (800 and 100 simulations), four legs:

    parent          a built checkout of the parent commit (--parent DIR), everything off
    tree_off        this tree, everything off
    gumbel_root     this tree, gumbel_root=16
    gumbel_interior this tree, gumbel_root=16, gumbel_interior=True

EVERY RUN IN A PROCESS OF ITS OWN, the processes alternating over the legs, --rounds times (3).  The parent's runs among
themselves give its range; the file records whether the median of tree_off lies inside it (`off_inside_parent_runs`) and the
difference of the medians.  The two Gumbel legs are other searches -- other trees, other depths -- so their figures get no
threshold; levels_per_descent says how deep they walk.  Nothing here says anything about playing strength.

    python tools/gumbel_interior.py --parent ../parent
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LEGS = ("parent", "tree_off", "gumbel_root", "gumbel_interior")
M = 16


def run_micro(args):
    sys.path.insert(0, args.root or ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import yinyang_game_alphazero_amd as pkg
    from hash_eval import hash_eval_torch
    torch.cuda.set_device(0)
    G, sims, A = args.slots, args.simulations, args.rows * args.cols
    kw = {}
    if args.leg in ("gumbel_root", "gumbel_interior"):
        kw["gumbel_root"] = M
    if args.leg == "gumbel_interior":
        kw["gumbel_interior"] = True
    ctx = pkg.engine.BatchedMCTS(G, args.rows, args.cols, sims, **kw)
    if kw:
        ctx.set_gumbel(pkg.engine.gumbel_rows(1000, torch.arange(G, dtype=torch.int64, device="cuda"),
                                              torch.zeros(G, dtype=torch.int32, device="cuda"), A))
        ctx.set_num_sims(sims)
    boards = torch.zeros((G, args.rows, args.cols), dtype=torch.int8, device="cuda")
    players = torch.ones(G, dtype=torch.int8, device="cuda")
    ctx.begin(boards, players, None)
    p, v = hash_eval_torch(ctx.planes, 10, 11)
    if args.leg == "gumbel_interior":
        ctx.expand_root(p, None, 0.25, value=v)
    else:
        ctx.expand_root(p, None, 0.25)
    ctx.select()
    skip = min(20, sims // 4)
    total, n = 0.0, 0
    for s in range(sims - 1):
        p, v = hash_eval_torch(ctx.planes, 10, 11)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ctx.step(p, v)
        b.record()
        torch.cuda.synchronize()
        if s > skip:
            total += a.elapsed_time(b)
            n += 1
    levels = ctx.status()["levels"]
    ctx.close()
    print("RESULT " + json.dumps(dict(step_us=total / n * 1e3, step_launches=n, levels_per_descent=levels / (G * sims))), flush=True)


def child(extra, limit):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, capture_output=True, text=True, timeout=limit)
    lines = [line for line in out.stdout.splitlines() if line.startswith("RESULT ")]
    if out.returncode != 0 or not lines:
        sys.exit(f"{' '.join(extra)}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    return json.loads(lines[-1][7:])


def summary(runs):
    med = {k: statistics.median(x["step_us"] for x in v) for k, v in runs.items()}
    out = dict(median_step_us=med, median_levels_per_descent={k: statistics.median(x["levels_per_descent"] for x in v)
                                                              for k, v in runs.items()})
    if "parent" in runs and "tree_off" in runs:
        us = [x["step_us"] for x in runs["parent"]]
        out.update(parent_runs=len(us), parent_min_us=min(us), parent_max_us=max(us), off_minus_parent_us=med["tree_off"] - med["parent"],
                   off_inside_parent_runs=bool(min(us) <= med["tree_off"] <= max(us)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", default="8x8,9x12")
    ap.add_argument("--budgets", default="800,100")
    ap.add_argument("--slots", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gumbel_interior.json"))
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)           # child: one per-step timing
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--rows", type=int, default=8, help=argparse.SUPPRESS)
    ap.add_argument("--cols", type=int, default=8, help=argparse.SUPPRESS)
    ap.add_argument("--simulations", type=int, default=800, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return run_micro(args)
    doc = dict(workload=dict(slots=args.slots, evaluator="hash", gumbel_root=M, rounds=args.rounds, boards=args.boards, budgets=args.budgets),
               skipped=[] if args.parent else ["the parent commit's runs (no --parent)"], per_step_us={}, summary={})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)

    for board in args.boards.split(","):
        rows, cols = (int(x) for x in board.split("x"))
        for sims in (int(x) for x in args.budgets.split(",")):
            key = f"{board}/{sims}"
            runs = doc["per_step_us"].setdefault(key, {})
            for _ in range(args.rounds):
                for leg in LEGS:
                    root = args.parent if leg == "parent" else ROOT
                    if root is None:
                        continue
                    rec = child(["--leg", "tree_off" if leg == "parent" else leg, "--root", os.path.abspath(root), "--rows", str(rows),
                                 "--cols", str(cols), "--simulations", str(sims), "--slots", str(args.slots)], 300)
                    runs.setdefault(leg, []).append(rec)
                    print(key, leg, json.dumps(rec), flush=True)
                    doc["summary"][key] = summary(runs)
                    save()
    print(json.dumps(doc["summary"], indent=1))


if __name__ == "__main__":
    main()
