"""What the shared evaluation table (shared_evaluations=) buys in self-play, and what the option costs in the tree step when it
is off -> profiles/shared_evaluations.json.

Self-play legs, played to completion on one MI355X, EVERY RUN IN A PROCESS OF ITS OWN, the legs alternating inside a repeat
(--repeats, default 3); all runs are kept in the file, the medians next to them.
  8x8 at config-2 size (800 simulations, f16x3, 128x10 net with random weights, 4 096 games in two lockstep lanes):
    defaults            cache + 8-stone book          defaults+shared      the same + a table per lane
    cache+shared        cache + table, no book        reuse-off            the network asked for every leaf
    reuse-off+shared    the table alone
  12x12 (config 4: 1 600 simulations, 1 024 games; no book exists there):   12x12, 12x12+shared
  free-running with the playout cap (0.25, fast 100) at the 8x8 size:          free-cap, free-cap+shared
A leg with the table plays the games of the leg without it, so positions/s compare directly; the tool asserts equal position
counts inside every such pair.  Per run: positions/s, evaluator rows per move, shared hits per move, fill of the tables at
the end, dropped inserts, table memory, seconds.

Per-step timing (the option off must cost nothing).  2 048 slots, 8x8, hash evaluator: the fused yy_mcts_step on the live trees
of an 800-simulation search, a pair of events around every launch, the mean over the launches after the first 20; the
processes alternate parent, tree (off), parent, tree (on), --micro-repeats times.  --parent DIR names a built checkout of the
parent commit; its runs among themselves give the run-to-run spread (max - min), and the file records whether the median of
the tree's option-off runs lies within it (`off_within_spread`).

The replacing table (shared_evaluations_replace=; --out profiles/shared_evaluations_replace.json):
  legs defaults+replace, free-cap+replace, 12x12+replace play the games of their base legs with a replacing table per lane;
  their records add duplicates, evicted, live at the end and the time of a sweep call (two events around 20 extra sweeps at
  the end of the run, which evict nothing new).  --high-water F sets the tables' high-water mark (default: the package's),
  --table-slots N their size (default: the package's 2^23), so a table smaller than the run shows eviction at work;
  the per-step timing adds parent_on (the parent with an insert-only table) and tree_replace (this tree, replacing table).
  Its 2 048 games are identical (one root, no noise, no per-game cache), so with a table it is the worst case by
  construction: every game inserts the same position in the same launch;
  --sweep-slots N times the two passes of a sweep alone on a table of N slots, half of them live (below the mark: the counting
  pass and an evicting pass that returns at once; above: both passes in full), against the bytes they move.

    python tools/shared_evaluations.py --parent ../parent                       # everything
    python tools/shared_evaluations.py --legs defaults,defaults+shared --no-micro
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

SMALL = dict(rows=8, cols=8, simulations=800, games=4096, lanes=2)
BIG = dict(rows=12, cols=12, simulations=1600, games=1024, lanes=2)
CAP = dict(free_running=True, fast_simulations=100, full_search_probability=0.25)
OFF = dict(reuse_pass_value=False, reuse_transpositions=False, keep_evaluations=False)
# leg -> (size, engine keywords, the leg whose games it plays)
LEGS = {
    "defaults": (SMALL, dict(opening_book=8), None),
    "defaults+shared": (SMALL, dict(opening_book=8, shared_evaluations=True), "defaults"),
    "cache+shared": (SMALL, dict(opening_book=0, shared_evaluations=True), "defaults"),
    "reuse-off": (SMALL, dict(opening_book=0, **OFF), "defaults"),
    "reuse-off+shared": (SMALL, dict(opening_book=0, shared_evaluations=True, **OFF), "defaults"),
    "12x12": (BIG, dict(opening_book=0), None),
    "12x12+shared": (BIG, dict(opening_book=0, shared_evaluations=True), "12x12"),
    "free-cap": (SMALL, dict(opening_book=8, **CAP), None),
    "free-cap+shared": (SMALL, dict(opening_book=8, shared_evaluations=True, **CAP), "free-cap"),
    "defaults+replace": (SMALL, dict(opening_book=8, shared_evaluations=True, shared_evaluations_replace=True), "defaults"),
    "free-cap+replace": (SMALL, dict(opening_book=8, shared_evaluations=True, shared_evaluations_replace=True, **CAP), "free-cap"),
    "12x12+replace": (BIG, dict(opening_book=0, shared_evaluations=True, shared_evaluations_replace=True), "12x12"),
}
HBM_PEAK_BYTES_PER_S = 8.0e12      # MI355X HBM3E, the data sheet's figure


def timed(torch, fn, n):
    """Mean milliseconds of fn() over n calls on the current stream, one pair of events around all of them."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


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


def run_leg(args):
    torch, pkg = _imports(ROOT)
    size, kw, _ = LEGS[args.leg]
    kw = dict(kw)
    if args.table_slots and kw.get("shared_evaluations"):
        kw["shared_evaluations"] = args.table_slots
    games = args.games or size["games"]
    game = pkg.YinYangGame(size["rows"], size["cols"])
    torch.manual_seed(0)
    ev = pkg.BatchedEvaluator(pkg.YinYangNeuralNetwork(game, args.channels, args.blocks).cuda().eval(), "f16x3")
    eng = pkg.SelfPlayLanes(game, ev, num_simulations=size["simulations"], concurrent_games=games, lanes=size["lanes"],
                            seed=args.seed, **kw)
    eng.ctx.reset_counters()
    replacing = [l.shared for l in eng.lanes if l.shared is not None and l.shared.replace]
    for t in replacing:
        if args.high_water is not None:
            t.high_water = args.high_water
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.run(games)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ctr, sh = eng.ctx.status(), eng.ctx.shared_counters()
    tables = [l.shared for l in eng.lanes if l.shared is not None]
    moves = max(1, eng.positions)
    rec = dict(seconds=dt, positions=eng.positions, games=eng.games_finished, positions_per_s=eng.positions / dt,
               evaluator_rows=ctr["evals"], rows_per_move=ctr["evals"] / moves, table_hits=ctr["transposition_hits"],
               shared_hits=sh["hits"], shared_hits_per_move=sh["hits"] / moves, shared_inserts=sh["inserts"],
               dropped_inserts=sh["dropped"], slots=sum(t.slots for t in tables), fill=sum(t.fill() for t in tables),
               memory_bytes=eng.memory_bytes())
    if replacing:
        ex = eng.ctx.shared_counters_ex()
        rec.update(duplicates=ex["duplicates"], evicted=ex["evicted"], live_at_last_sweep=ex["live"], high_water=replacing[0].high_water)
        sweep_ms = []
        for ln in eng.lanes:                      # after the run: the sweep of a lane's table as the run left it, on the lane's stream
            with ln._on_stream():
                sweep_ms.append(timed(torch, ln.shared.sweep, 20))
        rec.update(sweep_us_per_call=1e3 * statistics.mean(sweep_ms))
    eng.close()
    print("RESULT " + json.dumps(rec), flush=True)


def run_micro(args):
    torch, pkg = _imports(args.root or ROOT)
    G, sims = args.slots, 800
    ev = HashEval()
    ctx = pkg.engine.BatchedMCTS(G, 8, 8, sims)
    if args.shared:
        table = pkg.engine.SharedEvaluations(8, 8, 1 << 20, **(dict(replace=True) if args.replace else {}))
        ctx.set_shared_evaluations(table)
    boards = torch.zeros((G, 8, 8), dtype=torch.int8, device="cuda")
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
    c = ctx.status()
    rec = dict(step_us=total / n * 1e3, step_launches=n, evaluator_rows=c["evals"])
    if args.shared:
        rec.update(table.counters(), fill=table.fill())
    ctx.close()
    print("RESULT " + json.dumps(rec), flush=True)


def run_sweep(args):
    """The two passes of a sweep alone: a table of --sweep-slots slots of which every second one is live and old."""
    torch, pkg = _imports(ROOT)
    n = args.sweep_slots
    ctx = pkg.engine.BatchedMCTS(2, 8, 8, 8)
    table = pkg.engine.SharedEvaluations(8, 8, n, replace=True)
    ctx.set_shared_evaluations(table)
    rec = dict(slots=n, live=n // 2)

    def fill():
        table.claim.zero_()
        table.claim[::2] = (7 << 32) | 1          # tag 7, insert stamp 1
        table.last_hit.fill_(1)
        table.sweep_state.zero_()

    fill()
    table.stamp.fill_(5)
    # below the mark: the counting pass in full, the evicting pass returns at once in every workgroup
    table.high_water = 1.0
    table.sweep()
    ms = timed(torch, table.sweep, 50)
    moved = 8 * n
    rec.update(below_mark_us=1e3 * ms, below_mark_bytes=moved, below_mark_fraction_of_hbm_peak=moved / (ms * 1e-3) / HBM_PEAK_BYTES_PER_S)
    # above the mark, nothing to evict (every live entry carries the cutoff's stamp or a newer one): both passes read, no store
    table.high_water = 0.0
    table.sweep()                                  # records the stamp
    table.claim[::2] = (7 << 32) | 5
    table.last_hit.fill_(5)
    ms = timed(torch, table.sweep, 50)
    moved = 8 * n + 12 * n
    c = table.counters()
    assert c["evicted"] == 0 and c["live"] == n // 2, c
    rec.update(above_mark_us=1e3 * ms, above_mark_bytes=moved, above_mark_fraction_of_hbm_peak=moved / (ms * 1e-3) / HBM_PEAK_BYTES_PER_S)
    # above the mark, every live entry goes: one sweep (the stores of n / 2 claim words on top)
    fill()
    table.sweep()                                  # records stamp 5
    table.stamp.fill_(9)
    ms = timed(torch, table.sweep, 1)
    c = table.counters()
    assert c["evicted"] == n // 2 and c["live"] == 0, c
    rec.update(evict_all_us=1e3 * ms, evict_all_bytes=moved + 8 * (n // 2), note="three launches a sweep: count, evict, close; the "
               "times are per sweep() call, launches included, events around 50 calls (1 for evict_all)")
    ctx.close()
    print("RESULT " + json.dumps(rec), flush=True)


def child(extra, limit):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, capture_output=True, text=True, timeout=limit)
    lines = [line for line in out.stdout.splitlines() if line.startswith("RESULT ")]
    if out.returncode != 0 or not lines:
        sys.exit(f"{' '.join(extra)}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--micro-repeats", type=int, default=3)
    ap.add_argument("--slots", type=int, default=2048, help="games of the per-step timing")
    ap.add_argument("--legs", default=",".join(LEGS), help="'' = no self-play leg")
    ap.add_argument("--games", type=int, default=0, help="games per leg (0: the leg's own size)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the per-step timing")
    ap.add_argument("--no-micro", action="store_true")
    ap.add_argument("--leg-timeout", type=int, default=1100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_evaluations.json"))
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)          # child: one self-play run
    ap.add_argument("--micro", action="store_true", help=argparse.SUPPRESS)  # child: one per-step timing
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--shared", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--seed", type=int, default=1000, help=argparse.SUPPRESS)
    ap.add_argument("--high-water", type=float, default=None, help="replacing tables: the high-water mark (default: the package's)")
    ap.add_argument("--table-slots", type=int, default=0, help="slots of every leg's table (0: the package's default)")
    ap.add_argument("--sweep-slots", type=int, default=0, help="time the sweep passes alone on a table of this many slots")
    ap.add_argument("--replace", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--sweep-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    if args.micro:
        return run_micro(args)
    if args.sweep_child:
        return run_sweep(args)
    common = [str(x) for x in ("--channels", args.channels, "--blocks", args.blocks, "--slots", args.slots, "--games", args.games,
                               "--table-slots", args.table_slots)]
    if args.high_water is not None:
        common += ["--high-water", str(args.high_water)]
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc["workload"] = dict(net=f"{args.channels}x{args.blocks}", nn="f16x3", micro_slots=args.slots,
                           legs={k: dict(v[0], **v[1]) for k, v in LEGS.items()}, games_override=args.games or None)

    def save():
        runs = doc.get("runs", {})
        doc["median"] = {k: {f: statistics.median(r[f] for r in v) for f in v[0] if f != "memory_bytes"} for k, v in runs.items()}
        doc["workload"]["runs_per_leg"] = {k: len(v) for k, v in runs.items()}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)

    if not args.no_micro:
        micro = doc.setdefault("per_step_us", {})
        for _ in range(args.micro_repeats):
            for name, root, shared in (("parent", args.parent, False), ("tree_off", ROOT, False), ("parent_on", args.parent, True),
                                       ("tree_on", ROOT, True), ("parent", args.parent, False), ("tree_replace", ROOT, "replace")):
                if root is None:
                    continue
                rec = child(common + ["--micro", "--root", os.path.abspath(root)] + (["--shared"] if shared else [])
                            + (["--replace"] if shared == "replace" else []), 300)
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
                                           off_within_spread=bool(min(us) <= med["tree_off"] <= max(us)))
        if "parent_on" in micro:
            us = [x["step_us"] for x in micro["parent_on"]]
            doc["per_step_summary"].update(parent_on_min_us=min(us), parent_on_max_us=max(us),
                                           on_within_spread=bool(min(us) <= med["tree_on"] <= max(us)))
        save()
    if args.sweep_slots:
        rec = child(common + ["--sweep-child", "--sweep-slots", str(args.sweep_slots)], 300)
        doc.setdefault("sweep_passes", []).append(rec)
        print("sweep", json.dumps(rec), flush=True)
        save()
    doc.setdefault("runs", {})
    legs = [x for x in args.legs.split(",") if x]
    for rep in range(args.repeats):
        for leg in legs:
            rec = child(common + ["--leg", leg, "--seed", str(1000 + rep)], args.leg_timeout)
            rec["seed"] = 1000 + rep
            doc["runs"].setdefault(leg, []).append(rec)
            print(leg, json.dumps(rec), flush=True)
            save()
            base = LEGS[leg][2]
            for other in doc["runs"].get(base, []) if base else []:
                if other.get("seed") == rec["seed"]:     # the same games: the same number of positions
                    assert other["positions"] == rec["positions"] and other["games"] == rec["games"], (leg, base, other, rec)
    print(json.dumps(dict(per_step=doc.get("per_step_summary"), median=doc.get("median")), indent=1))


if __name__ == "__main__":
    main()
