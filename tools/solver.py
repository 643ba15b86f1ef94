"""The cost of the MCTS solver (solver=True) in the tree step with the option off, and what it does with the option on
-> profiles/solver.json.

Per-step timing.  2 048 slots, 8x8, hash evaluator: the fused yy_mcts_step on the live trees of an 800-simulation search, a
pair of events around every launch, the mean over the launches after the first 20.  EVERY RUN IN A PROCESS OF ITS OWN, the
processes alternating parent, tree (option off), parent, tree (solver on), --micro-repeats times.  --parent DIR names a built
checkout of the parent commit; its runs among themselves give the run-to-run spread (max - min), and the file records whether
the median of the tree's option-off runs exceeds the median of the parent's by more than that spread (`off_within_spread`).

Self-play legs.  Config 2 -- 8x8, 800 simulations, f16x3, 128x10 net with random weights, 4 096 games in two lockstep lanes,
played to completion -- with the engine's defaults ("defaults") and with evaluation reuse off ("reuse_off"), each once with
the option off and once on (--repeats for more), each run in a process of its own: positions/s, evaluator rows per move and the
three solver counters.  The games differ between off and on: no speed threshold applies, and nothing here says anything about
playing strength.

By ply.  --ply-games games (512) of the same board, budget and network are searched move by move in lockstep on one context
with the option on, all games at the same ply, the move drawn from the T = 1 root distribution (no root noise): per ply the
share of the descents that ended on a proven node below the root, the share of roots that are proven, and the evaluator rows
per descent.

    python tools/solver.py --parent ../parent          # everything
    python tools/solver.py --legs '' --no-ply --micro-repeats 5 --parent ../parent
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _imports(root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import yinyang_game_alphazero_amd as pkg
    torch.cuda.set_device(0)
    return torch, pkg


class HashEval:
    row_independent = True

    def __call__(self, planes):
        from hash_eval import hash_eval_torch
        return hash_eval_torch(planes, 10, 11)


def _net(torch, pkg, game, args):
    torch.manual_seed(0)
    return pkg.BatchedEvaluator(pkg.YinYangNeuralNetwork(game, args.channels, args.blocks).cuda().eval(), "f16x3")


def run_leg(args):
    torch, pkg = _imports(ROOT)
    game = pkg.YinYangGame(args.rows, args.cols)
    kw = dict(solver=True) if args.solver else {}
    if args.leg == "reuse_off":
        kw.update(reuse_pass_value=False, reuse_transpositions=False, keep_evaluations=False)
    eng = pkg.SelfPlayLanes(game, _net(torch, pkg, game, args), num_simulations=args.simulations, concurrent_games=args.games,
                            lanes=args.lanes, seed=args.seed, **kw)
    eng.ctx.reset_counters()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.run(args.games)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ctr = eng.ctx.status()
    sv = eng.ctx.solver_counters() if args.solver else dict(proven_nodes=0, proven_descents=0, proven_roots=0)
    rec = dict(seconds=dt, positions=eng.positions, games=eng.games_finished, positions_per_s=eng.positions / dt,
               evaluator_rows=ctr["evals"], rows_per_move=ctr["evals"] / max(1, eng.positions),
               terminal_revisits=ctr["terminal_revisits"], **sv)
    eng.close()
    print("RESULT " + json.dumps(rec), flush=True)


def run_ply(args):
    """All games at the same ply: one search per ply on one context, the counters read between two searches."""
    torch, pkg = _imports(ROOT)
    G, R, C, sims = args.ply_games, args.rows, args.cols, args.simulations
    game = pkg.YinYangGame(R, C)
    ctx = pkg.engine.BatchedMCTS(G, R, C, sims, solver=True)
    search = pkg.arena.LockstepSearch(ctx, _net(torch, pkg, game, args), use_graph=True)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    boards = torch.zeros((G, R, C), dtype=torch.int8, device="cuda")
    players = torch.ones(G, dtype=torch.int8, device="cuda")
    alive = torch.ones(G, dtype=torch.bool, device="cuda")
    rows = []
    for ply in range(4 * R * C):
        if not bool(alive.any()):
            break
        has = pkg.engine.valid_mask(boards, players).bool().any(1)
        players = torch.where(alive & ~has, -players, players).contiguous()          # a side without a move passes
        movers = alive & pkg.engine.valid_mask(boards, players).bool().any(1)
        if bool(movers.any()):
            ctx.reset_counters()
            search.run(boards, players, sims, noise=None, active=movers.to(torch.uint8).contiguous())
            ctr, sv = ctx.status(), ctx.solver_counters()
            root, _ = ctx.root_proven()
            n = int(movers.sum())
            rows.append(dict(ply=ply, games=n, descents=n * sims, proven_descents=sv["proven_descents"],
                             share_proven=sv["proven_descents"] / (n * sims), terminal_revisits=ctr["terminal_revisits"],
                             rows_per_descent=ctr["evals"] / (n * sims), proven_nodes=sv["proven_nodes"],
                             roots_proven=int((root[movers] != 0).sum())))
            pick = torch.multinomial(ctx.root_policy().float().clamp_min(0) + (~movers)[:, None].float(), 1, generator=gen).reshape(-1)
            action = torch.where(movers, pick.to(torch.int32), torch.full((G,), -1, dtype=torch.int32, device="cuda"))
            old = players.clone()
            pkg.engine.step_(boards, players, action.contiguous())
            players = torch.where(movers, players, old).contiguous()
        alive &= pkg.engine.game_ended(boards, players) == 0
    ctx.close()
    print("RESULT " + json.dumps(rows), flush=True)


def run_micro(args):
    torch, pkg = _imports(args.root or ROOT)
    G, sims = args.slots, args.simulations
    ev = HashEval()
    ctx = pkg.engine.BatchedMCTS(G, args.rows, args.cols, sims, **(dict(solver=True) if args.solver else {}))
    boards = torch.zeros((G, args.rows, args.cols), dtype=torch.int8, device="cuda")
    players = torch.ones(G, dtype=torch.int8, device="cuda")
    ctx.begin(boards, players, None)
    p, _ = ev(ctx.planes)
    ctx.expand_root(p, None, 0.25)
    ctx.select()
    total, n = 0.0, 0
    for s in range(sims - 1):
        p, v = ev(ctx.planes)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ctx.step(p, v)
        b.record()
        torch.cuda.synchronize()
        if s > 20:
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--cols", type=int, default=8)
    ap.add_argument("--simulations", type=int, default=800)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--micro-repeats", type=int, default=3)
    ap.add_argument("--slots", type=int, default=2048)
    ap.add_argument("--ply-games", type=int, default=512)
    ap.add_argument("--legs", default="defaults,reuse_off", help="'' = no self-play leg")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the per-step timing")
    ap.add_argument("--no-micro", action="store_true")
    ap.add_argument("--no-ply", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solver.json"))
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)          # child: one self-play run
    ap.add_argument("--micro", action="store_true", help=argparse.SUPPRESS)  # child: one per-step timing
    ap.add_argument("--ply", action="store_true", help=argparse.SUPPRESS)    # child: the by-ply run
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--solver", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--seed", type=int, default=1000, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    if args.micro:
        return run_micro(args)
    if args.ply:
        return run_ply(args)
    size = ["--games", args.games, "--lanes", args.lanes, "--rows", args.rows, "--cols", args.cols, "--simulations",
            args.simulations, "--channels", args.channels, "--blocks", args.blocks, "--slots", args.slots, "--ply-games", args.ply_games]
    size = [str(x) for x in size]
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc["workload"] = dict(board=f"{args.rows}x{args.cols}", games=args.games, lanes=args.lanes, simulations=args.simulations,
                           net=f"{args.channels}x{args.blocks}", nn="f16x3", micro_slots=args.slots, ply_games=args.ply_games)
    doc.setdefault("skipped", [])

    def save():
        runs = doc.get("runs", {})
        doc["median"] = {k: {f: statistics.median(r[f] for r in v) for f in v[0]} for k, v in runs.items()}
        doc["workload"]["runs_per_leg"] = {k: len(v) for k, v in runs.items()}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)

    if not args.no_micro:
        micro = doc.setdefault("per_step_us", {})
        for _ in range(args.micro_repeats):
            for name, root, on in (("parent", args.parent, 0), ("tree_off", ROOT, 0), ("parent", args.parent, 0), ("tree_on", ROOT, 1)):
                if root is None:
                    continue
                rec = child(size + ["--micro", "--root", os.path.abspath(root), "--solver", str(on)], 300)
                micro.setdefault(name, []).append(rec)
                print("micro", name, json.dumps(rec), flush=True)
                save()
        med = {k: statistics.median(x["step_us"] for x in v) for k, v in micro.items()}
        doc["per_step_summary"] = dict(median_step_us=med)
        if "parent" in micro:
            us = [x["step_us"] for x in micro["parent"]]
            spread = max(us) - min(us)
            doc["per_step_summary"].update(parent_runs=len(us), parent_min_us=min(us), parent_max_us=max(us), parent_spread_us=spread,
                                           off_minus_parent_us=med["tree_off"] - med["parent"],
                                           off_inside_parent_runs=bool(min(us) <= med["tree_off"] <= max(us)),
                                           off_within_spread=bool(med["tree_off"] <= med["parent"] + spread))
        else:
            doc["skipped"].append("per-step timing of the parent commit (no --parent)")
        save()
    doc.setdefault("runs", {})
    for rep in range(args.repeats):
        for leg in [x for x in args.legs.split(",") if x]:
            for on in (0, 1):
                rec = child(size + ["--leg", leg, "--solver", str(on), "--seed", str(1000 + rep)], 1200)
                doc["runs"].setdefault(f"{leg}/{'on' if on else 'off'}", []).append(rec)
                print(leg, on, json.dumps(rec), flush=True)
                save()
    if not args.no_ply:
        doc["by_ply"] = child(size + ["--ply", "--seed", "1000"], 1200)
        save()
    print(json.dumps(dict(per_step=doc.get("per_step_summary"), median=doc.get("median")), indent=1))


if __name__ == "__main__":
    main()
