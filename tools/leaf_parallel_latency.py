"""Latency of leaf-parallel search (leaves_per_step K) at small batches: one JSON line per measurement.

  search: wall time of MCTS.search on one 8x8 board, 800 simulations, the split-f16 evaluator (f16x3) on the seeded 128x10
          network, hipGraph replay on, for each K of --ks (median of --reps after one warm-up search).
  arena:  a --games-game, 800-simulation Arena of that network against itself, K = 1 and K = --arena-k alternating in the same
          process, median of --arena-reps runs each.
Run under `rocprofv3 --kernel-trace --stats -- python tools/leaf_parallel_latency.py --only search --ks K --reps 3` (one K per
process) to get the tree kernel's time per launch (k_mcts for K = 1, k_mcts_multi for K > 1)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import yinyang_game_alphazero_amd as pkg  # noqa: E402
from yinyang_game_alphazero_amd.game import YinYangLogic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["search", "arena", "all"], default="all")
    ap.add_argument("--ks", default="1,4,8,16,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--games", type=int, default=40)
    ap.add_argument("--arena-k", type=int, default=8)
    ap.add_argument("--arena-reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    game = pkg.YinYangGame(8, 8)
    ev = pkg.BatchedEvaluator(pkg.YinYangNeuralNetwork(game, 128, 10).cuda().eval(), "f16x3")
    lines = []

    def emit(rec):
        rec["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    if a.only in ("search", "all"):
        board = YinYangLogic(8, 8)
        rng = np.random.default_rng(0)
        player = 1
        for _ in range(6):                                         # a few random plies: a typical early position
            m = game.getValidMoves(board, player)
            board.board.flat[rng.choice(np.flatnonzero(m))] = player
            player = -player
        for K in [int(k) for k in a.ks.split(",")]:
            m = pkg.MCTS(game, ev, num_simulations=a.sims, board_semantics="copied", leaves_per_step=K)
            m.search(board, player)                                # warm-up: graph capture
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pi, root = m.search(board, player)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            assert root.visits == a.sims
            emit(dict(what="MCTS.search", board="8x8", net="128x10", nn="f16x3", sims=a.sims, leaves_per_step=K,
                      steps=-(-a.sims // K), median_ms=1e3 * statistics.median(ts), all_ms=[1e3 * t for t in ts]))
            m.close()
    if a.only in ("arena", "all"):
        ts = {1: [], a.arena_k: []}
        res = {}
        for _ in range(a.arena_reps):
            for K in (1, a.arena_k):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[K] = pkg.arena.Arena(game, ev, ev, num_simulations=a.sims, leaves_per_step=K).play(a.games)
                torch.cuda.synchronize()
                ts[K].append(time.perf_counter() - t0)
        for K in (1, a.arena_k):
            emit(dict(what="Arena.play", board="8x8", net="128x10", nn="f16x3", games=a.games, sims=a.sims, leaves_per_step=K,
                      median_s=statistics.median(ts[K]), all_s=ts[K], result=res[K]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
