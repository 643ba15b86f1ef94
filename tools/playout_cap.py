"""Self-play throughput with playout-cap randomisation (fast_simulations / full_search_probability): one JSON line per
configuration, all of them written to --out.

G games advance --moves lockstep moves through G slots (SelfPlayLanes, lanes as SelfPlayManager picks them), 8x8 board, 800
simulations, the split-f16 evaluator (f16x3) on the seeded 128x10 network, for (P, fast) = (1, -), (0.25, 100), (0.25, 200),
each with evaluation reuse off and with the engine's defaults, ALTERNATING inside this one process; median of --reps rounds.
Every round of a configuration goes on with the same engine: the first round starts the games, the later ones continue them
(and refill the slots of finished games), so the captured steps are reused.  positions/s = searched positions / wall seconds,
examples/s = the positions recorded as training examples (the fully searched ones), rows per move = evaluator rows the tree
asked for / moves.  The (1, -) lines of the same run are the yardstick; nothing here says anything about playing strength."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--moves", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--caps", default="1:0,0.25:100,0.25:200", help="P:fast pairs; fast 0 = no playout cap")
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--cols", type=int, default=8)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "playout_cap.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    game = pkg.YinYangGame(a.rows, a.cols)
    ev = pkg.BatchedEvaluator(pkg.YinYangNeuralNetwork(game, a.channels, a.blocks).cuda().eval(), "f16x3")
    G, lanes = a.games, 2 if a.games >= 512 else 1
    caps = [(float(p), int(f)) for p, f in (c.split(":") for c in a.caps.split(","))]
    engines, runs = {}, {}
    for reuse in (False, None):                                          # off; the engine's defaults
        for p, fast in caps:
            engines[p, fast, reuse] = pkg.SelfPlayLanes(game, ev, num_simulations=a.sims, concurrent_games=G, lanes=lanes, seed=1,
                                                        reuse_pass_value=reuse, reuse_transpositions=reuse, keep_evaluations=reuse,
                                                        fast_simulations=fast or None, full_search_probability=p)
            runs[p, fast, reuse] = []
    for rep in range(a.reps):
        for cfg, eng in engines.items():                                # alternating: every configuration once per round
            if rep == 0:
                for k, ln in enumerate(eng.lanes):
                    ln.begin_run(10 ** 9)                               # more games than any run plays: the slots stay full
                eng.play_move()                                         # the captures and warm-up of this engine's steps
            eng.ctx.reset_counters()
            pos, rec = eng.positions, eng.recorded
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.moves):
                eng.play_move()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            n, m = eng.positions - pos, eng.recorded - rec
            runs[cfg].append(dict(seconds=dt, positions=n, examples=m, positions_per_s=n / dt, examples_per_s=m / dt,
                                  rows_per_move=eng.ctx.status()["evals"] / a.moves))
    lines = []
    for (p, fast, reuse), eng in engines.items():
        r = runs[p, fast, reuse]
        med = lambda k: statistics.median(x[k] for x in r)
        lines.append(dict(what=f"SelfPlayLanes.play_move x {a.moves}", board=f"{a.rows}x{a.cols}", net=f"{a.channels}x{a.blocks}",
                          nn="f16x3", sims=a.sims, concurrent_games=G, lanes=lanes, full_search_probability=p,
                          fast_simulations=fast or None, evaluation_reuse=bool(eng.reuse_pass_value),
                          median_positions_per_s=med("positions_per_s"), median_examples_per_s=med("examples_per_s"),
                          median_rows_per_move=med("rows_per_move"), recorded_share=sum(x["examples"] for x in r) / sum(x["positions"] for x in r),
                          runs=r, device=torch.cuda.get_device_name(0)))
        print(json.dumps(lines[-1]), flush=True)
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
