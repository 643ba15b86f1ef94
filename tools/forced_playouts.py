"""The cost and the effect of forced playouts with policy target pruning (forced_playouts=k) -> profiles/forced_playouts.json.

Self-play legs.  Config 2 -- 8x8, 800 simulations, f16x3, 128x10 net with random weights, 4 096 games in two lockstep lanes,
played to completion -- with the engine defaults and with evaluation reuse off; the option off and k = 2 alternate, EVERY RUN IN
A PROCESS OF ITS OWN, --repeats times; all runs are in the file, the medians and the number of runs per leg next to them (a
second call with the same --out adds its runs to the file's).  Per run: positions/s, evaluator rows
per move, and with the option on a probe on the run's own positions: --probe positions drawn from its examples are searched once
more (same net, Dirichlet(0.3) noise, eps 0.25) on a context of their own, which gives the share of root descents that took a
forced edge (yy_mcts_forced_descents / simulations) and the mean pruned-away share of the visits behind pi (1 - sum N' / sum N,
sum N' = N(c*) / pi(c*): the most visited edge keeps its count).  The games differ between off and on: no speed threshold
applies and no claim about playing strength is made.

Per-step timing (--micro-only / part of the default run).  2 048 slots, hash evaluator: the fused yy_mcts_step on the live trees
of an 800-simulation search (events around every launch, mean) and 400 back-to-back yy_mcts_step_selfplay launches with every
slot idle (tools/free_running.py's launch timing).  --parent DIR names a built checkout of the parent commit: the processes
alternate parent, tree (option off), parent, tree (k = 2), so the parent's two runs give its own run-to-run spread.

    python tools/forced_playouts.py --parent ../parent                    # everything (about 20 minutes)
    python tools/forced_playouts.py --legs defaults --repeats 1
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


# ------------------------------------------------------------------------------------------------ one self-play run
def probe(torch, pkg, ev, states, args, k):
    """-> (share of root descents that were forced, mean pruned-away visit share) on `states` int8 [n, R, C]"""
    n = states.shape[0]
    stones_b, stones_w = (states == 1).flatten(1).sum(1), (states == -1).flatten(1).sum(1)
    players = torch.where(stones_b == stones_w, 1, -1).to(torch.int8)
    mask = pkg.engine.valid_mask(states, players).bool()
    keep = mask.any(1)
    states, players, mask = states[keep][:args.probe].contiguous(), players[keep][:args.probe].contiguous(), mask[keep][:args.probe]
    n = states.shape[0]
    g = torch.distributions.Gamma(torch.full(mask.shape, 0.3, dtype=torch.float64, device=mask.device), 1.0).sample()
    g = torch.where(mask, g, torch.zeros_like(g))
    noise = (g / g.sum(1, keepdim=True).clamp_min(1e-300)).contiguous()
    mc = pkg.engine.BatchedMCTS(n, args.rows, args.cols, args.simulations, forced_playouts=k)
    try:
        mc.search(states, players, ev, args.simulations, noise=noise, eps=0.25)
        counts = mc.root_counts().cpu().numpy().astype("float64")
        pi = mc.root_policy().cpu().numpy()
        forced = mc.forced_descents()
        mc.status()
    finally:
        mc.close()
    star = counts.argmax(1)
    rows = range(n)
    pruned_sum = counts[rows, star] / pi[rows, star]
    return forced / float(counts.sum()), float((1.0 - pruned_sum / counts.sum(1)).mean()), n


def run_leg(args):
    torch, pkg = _imports(ROOT)
    game = pkg.YinYangGame(args.rows, args.cols)
    torch.manual_seed(0)
    ev = pkg.BatchedEvaluator(pkg.YinYangNeuralNetwork(game, args.channels, args.blocks).cuda().eval(), "f16x3")
    legs = {"defaults": {}, "reuse_off": dict(reuse_pass_value=False, reuse_transpositions=False, keep_evaluations=False)}
    k = float(args.k)
    eng = pkg.SelfPlayLanes(game, ev, num_simulations=args.simulations, concurrent_games=args.games, lanes=args.lanes,
                            seed=args.seed, **legs[args.leg], **(dict(forced_playouts=k) if k else {}))
    eng.ctx.reset_counters()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ex = eng.run(args.games)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ctr = eng.ctx.status()
    rec = dict(seconds=dt, positions=eng.positions, games=eng.games_finished, positions_per_s=eng.positions / dt,
               evaluator_rows=ctr["evals"], rows_per_move=ctr["evals"] / max(1, eng.positions))
    states = ex["states"]
    eng.close()
    if k:
        pick = torch.randperm(states.shape[0], generator=torch.Generator().manual_seed(args.seed))[:2 * args.probe]
        rec["forced_descent_share"], rec["pruned_visit_share"], rec["probe_positions"] = probe(
            torch, pkg, ev, states[pick.to(states.device)].to(torch.int8).cuda(), args, k)
    print("RESULT " + json.dumps(rec), flush=True)


# ------------------------------------------------------------------------------------------------ per-step timing
def run_micro(args):
    torch, pkg = _imports(args.root or ROOT)
    G, sims, k = args.slots, args.simulations, float(args.k)
    kw = dict(forced_playouts=k) if k else {}
    ev = HashEval()
    ctx = pkg.engine.BatchedMCTS(G, args.rows, args.cols, sims, **kw)
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
    ctx.status()
    ctx.close()
    rec = dict(step_us=total / n * 1e3, step_launches=n)
    eng = pkg.SelfPlayEngine(pkg.YinYangGame(args.rows, args.cols), ev, num_simulations=8, concurrent_games=G, seed=1,
                             free_running=True, **kw)
    eng.run(G)
    c, run = eng.ctx, eng.run_state
    policy = torch.zeros((c.rows, c.A), dtype=torch.float32, device=c.device)
    value = torch.zeros(c.rows, dtype=torch.float32, device=c.device)
    for _ in range(20):
        run.step(policy, value)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.move_launches):
        run.step(policy, value)
    b.record()
    b.synchronize()
    rec["step_selfplay_idle_us"] = a.elapsed_time(b) * 1000.0 / args.move_launches
    eng.close()
    print("RESULT " + json.dumps(rec), flush=True)


# ------------------------------------------------------------------------------------------------ the whole measurement
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--probe", type=int, default=512)
    ap.add_argument("--slots", type=int, default=2048)
    ap.add_argument("--move-launches", type=int, default=400)
    ap.add_argument("--legs", default="defaults,reuse_off", help="'' = none")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the per-step timing")
    ap.add_argument("--no-micro", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forced_playouts.json"))
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)          # child: one self-play run
    ap.add_argument("--micro", action="store_true", help=argparse.SUPPRESS)  # child: one per-step timing
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--k", type=float, default=0.0, help=argparse.SUPPRESS)
    ap.add_argument("--seed", type=int, default=1000, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    if args.micro:
        return run_micro(args)
    size = ["--games", args.games, "--lanes", args.lanes, "--rows", args.rows, "--cols", args.cols, "--simulations",
            args.simulations, "--channels", args.channels, "--blocks", args.blocks, "--probe", args.probe, "--slots", args.slots,
            "--move-launches", args.move_launches]
    size = [str(x) for x in size]
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc["workload"] = dict(board=f"{args.rows}x{args.cols}", games=args.games, lanes=args.lanes, simulations=args.simulations,
                           net=f"{args.channels}x{args.blocks}", nn="f16x3", k=2.0, probe=args.probe, micro_slots=args.slots)

    def save():
        runs = doc.get("runs", {})
        doc["median"] = {k: {f: statistics.median(r[f] for r in v) for f in v[0]} for k, v in runs.items()}
        doc["workload"]["runs_per_leg"] = {k: len(v) for k, v in runs.items()}
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)

    if not args.no_micro:
        order = [("parent", args.parent, 0.0), ("tree_off", ROOT, 0.0), ("parent", args.parent, 0.0), ("tree_k2", ROOT, 2.0)]
        micro = {}
        for name, root, k in order:
            if root is None:
                continue
            rec = child(size + ["--micro", "--root", os.path.abspath(root), "--k", str(k)], 300)
            micro.setdefault(name, []).append(rec)
            print("micro", name, json.dumps(rec), flush=True)
        doc["per_step_us"] = micro
        save()
    doc.setdefault("runs", {})
    for rep in range(args.repeats):
        for leg in [x for x in args.legs.split(",") if x]:
            for k in (0.0, 2.0):
                rec = child(size + ["--leg", leg, "--k", str(k), "--seed", str(1000 + rep)], 900)
                doc["runs"].setdefault(f"{leg}/{'off' if not k else 'k=2'}", []).append(rec)
                print(leg, k, json.dumps(rec), flush=True)
                save()
    print(json.dumps(doc.get("median"), indent=1))


if __name__ == "__main__":
    main()
