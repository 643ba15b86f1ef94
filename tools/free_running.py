"""Lockstep against free-running self-play, whole runs played to completion, on one GPU -> profiles/free_running.json.

Default workload: config 2 -- 8x8, 800 simulations, f16x3, 128x10 net, 4 096 games in two lanes.  Configurations compared,
each lockstep and free-running: engine defaults, evaluation reuse off, playout cap (0.25, 100) with reuse on and off.  The
configurations alternate inside one process; every figure is the median of --repeats runs.  Reported per leg and engine:
positions/s and recorded examples/s over the whole run; steps issued (free-running: the device steps the host replayed;
lockstep: moves x (simulations + 1) evaluator launches per lane, summed over the lanes); the histogram, the sum and the mean of
the evaluator rows per launch; and the time of one k_selfplay_move launch.

Rows per launch are counted on the device, inside the captured step, by the search's `timer` hook (it runs between the
evaluator and the tree kernel): three small torch kernels per step that add needs_eval.sum() to a histogram -- the same
overhead for both engines.  Lockstep's root call and last evaluation of a move are issued outside that hook (2 of
simulations + 1 launches per move) and are not in its histogram; the free-running root rows travel in ordinary steps and are.
The move launch is timed after a run, when every slot is idle (every wavefront takes the early-out, the common case during
a run): `--move-launches` steps of yy_mcts_step_selfplay (k_mcts + k_selfplay_move) against as many of yy_mcts_step (k_mcts
alone) between events; the difference per step is the launch.

    python tools/free_running.py                                  # config 2, all legs (many minutes)
    python tools/free_running.py --legs reuse_off --out profiles/free_running.reuse_off.json
    python tools/free_running.py --merge a.json b.json --out profiles/free_running.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EDGES = [1, 2, 17, 65, 129, 257, 513, 1025, 1537, 2049]      # bins: 0, 1, 2-16, 17-64, 65-128, 129-256, ..., > 2048
BINS = ["0", "1", "2-16", "17-64", "65-128", "129-256", "257-512", "513-1024", "1025-1536", "1537-2048", ">2048"]


class RowCounter:
    """search.timer hook: start() runs inside every step, captured or eager, after the evaluator and before the tree kernel."""

    def __init__(self, torch, ctx):
        dev = ctx.device
        self.torch, self.flags = torch, ctx.needs_eval
        self.edges = torch.tensor(EDGES, dtype=torch.int64, device=dev)
        self.hist = torch.zeros(len(BINS), dtype=torch.int64, device=dev)
        self.rows = torch.zeros(1, dtype=torch.int64, device=dev)
        self.one = torch.ones(1, dtype=torch.int64, device=dev)

    def start(self):
        n = self.flags.sum(dtype=self.torch.int64).reshape(1)
        self.rows.add_(n)
        self.hist.index_add_(0, self.torch.bucketize(n, self.edges, right=True), self.one)

    def stop(self):
        pass


def move_launch_us(torch, lane, n):
    """One k_selfplay_move launch with every slot idle, in microseconds: (k_mcts + move) - (k_mcts) per step."""
    ctx, run = lane.ctx, lane.run_state
    policy = torch.zeros((ctx.rows, ctx.A), dtype=torch.float32, device=ctx.device)
    value = torch.zeros(ctx.rows, dtype=torch.float32, device=ctx.device)
    out = []
    for fn in (lambda: run.step(policy, value), lambda: ctx.step(policy, value)):
        for _ in range(20):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / n)
    return out[0] - out[1], out[0], out[1]


def merge(paths, out):
    docs = [json.load(open(p)) for p in paths]
    doc = dict(workload=docs[0]["workload"], bins=BINS, median={}, runs={})
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
    ap.add_argument("--slots", type=int, default=0, help="concurrent games (default: --games)")
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--simulations", type=int, default=800)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--move-launches", type=int, default=400)
    ap.add_argument("--legs", default="defaults,reuse_off,cap,cap_reuse_off")
    ap.add_argument("--merge", nargs="+", default=None, help="join the files of runs made leg by leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "free_running.json"))
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    import torch
    import yinyang_game_alphazero_amd as pkg
    from yinyang_game_alphazero_amd.self_play import shard_games

    torch.cuda.set_device(0)
    game = pkg.YinYangGame(8, 8)
    torch.manual_seed(0)
    ev = pkg.BatchedEvaluator(pkg.YinYangNeuralNetwork(game, args.channels, args.blocks).cuda().eval(), "f16x3")
    off = dict(reuse_pass_value=False, reuse_transpositions=False, keep_evaluations=False)
    cap = dict(fast_simulations=min(100, args.simulations), full_search_probability=0.25)
    legs = {"defaults": {}, "reuse_off": off, "cap": cap, "cap_reuse_off": dict(cap, **off)}
    slots = args.slots or args.games
    runs = {}
    for rep in range(args.repeats):
        for name in args.legs.split(","):
            for free in (False, True):
                eng = pkg.SelfPlayLanes(game, ev, num_simulations=args.simulations, concurrent_games=slots, lanes=args.lanes,
                                        seed=1000 + rep, **legs[name], **(dict(free_running=True) if free else {}))
                K = len(eng.lanes)
                eng.ctx.reset_counters()
                moves = [0]
                if not free:
                    play_move = eng.play_move

                    def counted():
                        moves[0] += sum(1 for l in eng.lanes if l.n_alive > 0)      # lane-moves: one search each
                        return play_move()
                    eng.play_move = counted
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k, l in enumerate(eng.lanes):
                    l.begin_run(shard_games(args.games, k, K)[0])
                counters = []
                for l in eng.lanes:
                    with l._on_stream():
                        counters.append(RowCounter(torch, l.ctx))
                    (l.free_search if free else l.search).timer = counters[-1]
                eng.play_to_completion()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                ctr = eng.ctx.status()
                hist = sum(c.hist for c in counters).tolist()
                rows, launches = int(sum(int(c.rows) for c in counters)), int(sum(hist))
                steps = eng.steps_issued if free else moves[0] * (args.simulations + 1)
                rec = dict(seconds=dt, positions=eng.positions, recorded=eng.recorded, games=eng.games_finished,
                           positions_per_s=eng.positions / dt, recorded_per_s=eng.recorded / dt, steps_issued=steps,
                           launches_counted=launches, rows_counted=rows, rows_per_launch=rows / max(1, launches),
                           evaluator_rows=ctr["evals"], rows_histogram=hist)
                if free:
                    with eng.lanes[0]._on_stream():
                        rec["move_launch_us"], rec["step_selfplay_us"], rec["step_us"] = move_launch_us(torch, eng.lanes[0],
                                                                                                         args.move_launches)
                runs.setdefault(f"{name}/{'free_running' if free else 'lockstep'}", []).append(rec)
                print(name, "free" if free else "lock", json.dumps(rec), flush=True)
                eng.close()

    def med(v, f):
        if isinstance(v[0][f], list):
            return [statistics.median(r[f][i] for r in v) for i in range(len(v[0][f]))]
        return statistics.median(r[f] for r in v)

    median = {k: {f: med(v, f) for f in v[0]} for k, v in runs.items()}
    out = dict(workload=dict(board="8x8", games=args.games, slots=slots, lanes=args.lanes, simulations=args.simulations,
                             net=f"{args.channels}x{args.blocks}", nn="f16x3", repeats=args.repeats,
                             device=torch.cuda.get_device_name(0)), bins=BINS, median=median, runs=runs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(median, indent=1))


if __name__ == "__main__":
    main()
