"""Self-play throughput with leaf-parallel searches (leaves_per_step K) at few concurrent games: one JSON line per measurement.

G games are played to completion through G slots by SelfPlayLanes (lanes as SelfPlayManager picks them: 2 from 512 slots on),
8x8 board, 800 simulations, the split-f16 evaluator (f16x3) on the seeded 128x10 network, for each G of --games and, ALTERNATING
inside this one process, each K of --ks with evaluation reuse off (what K > 1 resolves to) and, at K = 1, a second line with
the engine's defaults (evaluation reuse on; no book below 1024 games), so that the record shows where K loses to reuse.
positions/s = searched positions / wall seconds of the run, the draining tail included; median of --reps runs.  Every run of
a configuration plays new games of the same engine (the game indices go on), so its captured steps are reused after run 1.
The K = 1 lines of the same run are the yardstick; nothing is compared with numbers from another process or box."""
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
    ap.add_argument("--games", default="40,100,512")
    ap.add_argument("--ks", default="1,4,8,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--cols", type=int, default=8)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the lines to this file (rewritten after every G)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    game = pkg.YinYangGame(a.rows, a.cols)
    ev = pkg.BatchedEvaluator(pkg.YinYangNeuralNetwork(game, a.channels, a.blocks).cuda().eval(), "f16x3")
    lines = []

    def emit(rec):
        rec["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                for r in lines:
                    f.write(json.dumps(r) + "\n")

    for G in [int(g) for g in a.games.split(",")]:
        lanes = 2 if G >= 512 else 1
        configs = [(K, False) for K in [int(k) for k in a.ks.split(",")]] + [(1, None)]      # (K, the three reuse options)
        engines, runs = {}, {}
        for K, reuse in configs:
            engines[K, reuse] = pkg.SelfPlayLanes(game, ev, num_simulations=a.sims, concurrent_games=G, lanes=lanes, seed=1,
                                                  leaves_per_step=K, reuse_pass_value=reuse, reuse_transpositions=reuse,
                                                  keep_evaluations=reuse)
            runs[K, reuse] = []
        for _ in range(a.reps):
            for cfg, eng in engines.items():                            # alternating: every configuration once per round
                eng.ctx.reset_counters()
                before = eng.positions
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ex = eng.run(G)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                n = eng.positions - before
                assert int(ex["states"].shape[0]) == n
                runs[cfg].append(dict(seconds=dt, positions=n, positions_per_s=n / dt, evals=eng.ctx.status()["evals"]))
        for (K, reuse), eng in engines.items():
            r = runs[K, reuse]
            emit(dict(what="SelfPlayLanes.run to completion", board=f"{a.rows}x{a.cols}", net=f"{a.channels}x{a.blocks}", nn="f16x3",
                      sims=a.sims, games=G, concurrent_games=G, lanes=lanes, leaves_per_step=K,
                      evaluation_reuse=bool(eng.reuse_pass_value), steps_per_move=-(-a.sims // K) + 1,
                      median_positions_per_s=statistics.median(x["positions_per_s"] for x in r),
                      median_seconds=statistics.median(x["seconds"] for x in r), runs=r))
            eng.close()


if __name__ == "__main__":
    main()
