"""Self-play throughput with tree reuse across moves (tree_reuse=True): one JSON line per configuration, all written to --out.

G games advance --moves lockstep moves per round through G slots (SelfPlayLanes, lanes as SelfPlayManager picks them), 8x8
board, 800 simulations, the split-f16 evaluator (f16x3) on the seeded 128x10 network, tree_reuse off / on, each with evaluation
reuse off and with the engine's defaults, ALTERNATING inside this one process; median of --reps rounds.  Every round of a
configuration goes on with the same engine: the first round starts the games from the empty board, the later ones continue
them, so the captured steps are reused.  positions/s = searched positions / wall seconds; rows per move = evaluator rows the
tree asked for / moves; kept visits = the visits the re-rooted trees carry into the next search, mean over all slots and moves;
advance ms = device time between two events around the yy_mcts_advance launch of a lane, mean over lanes and moves (the other
lane's kernels run beside it).  The tree_reuse=False lines of the same run are the yardstick; nothing here says anything about
playing strength."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import yinyang_game_alphazero_amd as pkg  # noqa: E402


def timed_advance(lane, log):
    """Wrap the lane's ctx.advance: events around the launch, and the kept visits it returns."""
    inner = lane.ctx.advance

    def advance(actions):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        kept = inner(actions)
        t1.record()
        log.append((t0, t1, kept))
        return kept

    lane.ctx.advance = advance


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--moves", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--cols", type=int, default=8)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_reuse.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    game = pkg.YinYangGame(a.rows, a.cols)
    ev = pkg.BatchedEvaluator(pkg.YinYangNeuralNetwork(game, a.channels, a.blocks).cuda().eval(), "f16x3")
    G, lanes = a.games, 2 if a.games >= 512 else 1
    engines, runs, logs = {}, {}, {}
    for reuse in (False, None):                                          # evaluation reuse off; the engine's defaults
        for tree in (False, True):
            eng = pkg.SelfPlayLanes(game, ev, num_simulations=a.sims, concurrent_games=G, lanes=lanes, seed=1, reuse_pass_value=reuse,
                                    reuse_transpositions=reuse, keep_evaluations=reuse, tree_reuse=tree)
            engines[reuse, tree], runs[reuse, tree], logs[reuse, tree] = eng, [], []
            if tree:
                for ln in eng.lanes:
                    timed_advance(ln, logs[reuse, tree])
    for rep in range(a.reps):
        for cfg, eng in engines.items():                                # alternating: every configuration once per round
            if rep == 0:
                for ln in eng.lanes:
                    ln.begin_run(10 ** 9)                               # more games than any run plays: the slots stay full
                eng.play_move()                                         # the captures and warm-up of this engine's steps
            eng.ctx.reset_counters()
            del logs[cfg][:]
            pos = eng.positions
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.moves):
                eng.play_move()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            n = eng.positions - pos
            rec = dict(seconds=dt, positions=n, positions_per_s=n / dt, rows_per_move=eng.ctx.status()["evals"] / a.moves)
            if logs[cfg]:
                rec["advance_ms"] = statistics.mean(t0e.elapsed_time(t1e) for t0e, t1e, _ in logs[cfg])
                rec["kept_visits"] = statistics.mean(float(k.float().mean()) for _, _, k in logs[cfg])
            runs[cfg].append(rec)
    lines = []
    for (reuse, tree), eng in engines.items():
        r = runs[reuse, tree]
        med = lambda k: statistics.median(x[k] for x in r) if k in r[0] else None
        lines.append(dict(what=f"SelfPlayLanes.play_move x {a.moves}", board=f"{a.rows}x{a.cols}", net=f"{a.channels}x{a.blocks}",
                          nn="f16x3", sims=a.sims, concurrent_games=G, lanes=lanes, tree_reuse=tree,
                          evaluation_reuse=bool(eng.reuse_pass_value), median_positions_per_s=med("positions_per_s"),
                          median_rows_per_move=med("rows_per_move"), median_kept_visits=med("kept_visits"),
                          median_advance_ms=med("advance_ms"), runs=r, device=torch.cuda.get_device_name(0)))
        print(json.dumps(lines[-1]), flush=True)
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
