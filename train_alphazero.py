#!/usr/bin/env python3
"""Same-flag entry point as the reference's train_alphazero.py (train_alphazero.py:30-61), running
`--mode self-play` on the MI355X engine.

    python train_alphazero.py --mode self-play --rows 8 --cols 8 --simulations 800 --episodes 4096
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train_alphazero.py --mode self-play ...

Flags added to the reference's set: --concurrent-games, --lanes, --board-semantics {copied,aliased}, --reference-quirks,
--nn {auto,f16x3,bf16,fp32,fp32t}, --evaluation-reuse, --opening-book-stones, --seed, --arena-games, --channels, --blocks, --fresh,
--dist-backend, --reference-format, --leaves-per-step, --fast-simulations, --full-search-probability, --tree-reuse, --free-running,
--evaluation-symmetry, --symmetry-seed, --forced-playouts, --fpu-reduction, --fpu-reduction-root, --shared-evaluations, --shared-evaluations-replace,
--solver.
`--mode train` runs
the iteration loop (GPU self-play -> PyTorch-ROCm training -> batched arena -> promote at 0.6) and
`--mode evaluate` plays 10 games against RandomPlayer, like the reference's modes.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Yin-Yang AlphaZero self-play on MI355X")
    p.add_argument("--rows", type=int, default=8)
    p.add_argument("--cols", type=int, default=8)
    p.add_argument("--iterations", type=int, default=100)
    p.add_argument("--episodes", type=int, default=100)
    p.add_argument("--simulations", type=int, default=800)
    p.add_argument("--epochs", type=int, default=10)
    p.add_argument("--batch-size", type=int, default=64)
    p.add_argument("--lr", type=float, default=0.001)
    p.add_argument("--workers", type=int, default=1)
    p.add_argument("--mcts-threads", type=int, default=1)
    p.add_argument("--model-dir", type=str, default="models")
    p.add_argument("--data-dir", type=str, default="data")
    p.add_argument("--resume", action="store_true",
                   help="accepted for compatibility and inert, like the reference's (train_alphazero.py:55 parses it, nothing reads it): "
                        "models and checkpoint_<n> files found in --model-dir are ALWAYS continued from (alphazero.py:66-73, "
                        "training_pipeline.py:171-190); use --fresh to start over")
    p.add_argument("--fresh", action="store_true",
                   help="train: remove current_model / best_model / checkpoint_<n> from --model-dir first (start from a new random network)")
    p.add_argument("--mode", choices=["train", "self-play", "evaluate"], default="train")
    p.add_argument("--output-model", type=str, default="best_model.pth.tar")
    # engine flags
    p.add_argument("--concurrent-games", type=int, default=4096)
    p.add_argument("--board-semantics", choices=["copied", "aliased"], default="copied")
    p.add_argument("--reference-quirks", action="store_true", help="reproduce Q4/Q5 of the reference's play_game")
    p.add_argument("--nn", choices=["auto", "f16x3", "bf16", "fp32", "fp32t"], default="auto",
                   help="evaluator: auto = float32-accurate (f16x3 split-f16 tower where the kernels cover the shape, else the fp32 module; the "
                        "reference evaluates in float32); bf16 = reduced-precision fast tower; fp32t exact-f32 tower (8x8, 128 channels)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--evaluation-reuse", choices=["auto", "off"], default="auto",
                   help="auto: the network is asked once per position of a game (pass values + per-game evaluation cache; "
                        "identical games); off: once per leaf, like the reference")
    p.add_argument("--reference-format", action="store_true",
                   help="self-play: also store the reference's pickled board objects so its own training pipeline reads the file")
    p.add_argument("--opening-book-stones", type=int, default=None,
                   help="shared opening book: every position reachable with at most N stones is evaluated once before play "
                        "(default: 8 when evaluation reuse is on, the board has at most 64 cells and the rank plays >= 1024 games; 0 = none)")
    p.add_argument("--dist-backend", choices=["nccl", "gloo"], default="nccl",
                   help="collectives of a multi-rank launch: nccl = RCCL over xGMI (one rank per GPU); gloo = over the host, "
                        "which also allows several ranks to share one GPU (rehearsals on a 1-GPU box)")
    p.add_argument("--lanes", type=int, default=0,
                   help="self-play: HIP streams the rank's concurrent games are cut over (0 = automatic: 2 from 512 games on); a lane's "
                        "evaluator launch fills the compute units the other lane's last round of workgroups leaves idle; same games")
    p.add_argument("--arena-games", type=int, default=40)
    p.add_argument("--channels", type=int, default=128)
    p.add_argument("--blocks", type=int, default=10)
    p.add_argument("--leaves-per-step", type=int, default=1,
                   help="K descents per game per search step with virtual visits, evaluated in one batch (a search then takes "
                        "ceil(simulations / K) evaluator calls; 1 = the reference's search; changes which moves are picked): the "
                        "searches of --mode evaluate, of --mode self-play and of --mode train (self-play and arena).  In "
                        "self-play K > 1 turns --evaluation-reuse auto off and builds no opening book (--opening-book-stones is "
                        "ignored); not with --board-semantics aliased or --reference-quirks.  --mcts-threads stays inert")
    p.add_argument("--fast-simulations", type=int, default=None,
                   help="self-play and train: playout-cap randomisation -- a move is searched with --simulations with probability "
                        "--full-search-probability and with N simulations otherwise; only the fully searched moves become "
                        "training examples (default: every move is searched in full)")
    p.add_argument("--full-search-probability", type=float, default=1.0,
                   help="share P in (0, 1] of the moves searched in full when --fast-simulations is given (default 1 = all)")
    p.add_argument("--tree-reuse", action="store_true",
                   help="self-play, train and evaluate: every search continues from the subtree under the move played and tops its "
                        "root up to the move's simulations, instead of starting from a fresh root (default off; changes which "
                        "moves are picked; not with --leaves-per-step > 1 or --board-semantics aliased)")
    p.add_argument("--free-running", action="store_true",
                   help="self-play and train: the games play their moves on the device, inside the search step, each as soon as its "
                        "own search is complete, instead of in lockstep (default off; the same games; not with --leaves-per-step "
                        "> 1, --board-semantics aliased, --reference-quirks or --tree-reuse)")
    p.add_argument("--evaluation-symmetry", choices=["off", "random"], default="off",
                   help="self-play and train: random = every position is shown to the network under a board symmetry drawn for it "
                        "(a pure function of --symmetry-seed and the position) and the policy is mapped back (default off; changes "
                        "which moves are picked; not with --board-semantics aliased or --reference-quirks)")
    p.add_argument("--symmetry-seed", type=int, default=None,
                   help="seed of the symmetry draw of --evaluation-symmetry random (default: the engine's seed)")
    p.add_argument("--forced-playouts", type=float, default=None, metavar="K",
                   help="self-play and train: forced playouts with policy target pruning at the search root -- a visited root child "
                        "is visited again while N*N < K*P*S, and the recorded policy is computed from the pruned counts (KataGo: 2; "
                        "default off; changes which moves are picked; not with --leaves-per-step > 1, --board-semantics aliased or "
                        "--reference-quirks)")
    p.add_argument("--fpu-reduction", type=float, default=None, metavar="R",
                   help="self-play, train (self-play and arena) and evaluate: first-play urgency reduction -- a child that has not been "
                        "visited is scored with the mean value of its visited siblings less R * sqrt(their share of the prior) "
                        "instead of 0 (KataGo: 0.2; default off; changes which moves are picked; not with --reference-quirks)")
    p.add_argument("--fpu-reduction-root", type=float, default=None, metavar="R",
                   help="the R of --fpu-reduction at the search root (default: the same R; KataGo uses 0 at a noised root)")
    p.add_argument("--shared-evaluations", type=int, nargs="?", const=True, default=None, metavar="SLOTS",
                   help="self-play and train: the games of a lane share their evaluations through a table they fill while they play "
                        "-- a position any of them has had evaluated needs no evaluator row again (SLOTS: table slots per lane, "
                        "rounded up to a power of two; without a number 2^23, which at 8x8 costs what the 8-stone book costs; "
                        "default off; the same games; not with --leaves-per-step > 1, --board-semantics aliased or --reference-quirks)")
    p.add_argument("--shared-evaluations-replace", action="store_true",
                   help="self-play and train, with --shared-evaluations: the table keeps one slot per position and sheds what is no "
                        "longer used (a sweep per move, or per poll with --free-running), so it serves a run of any length from "
                        "its fixed size (default off; the same games)")
    p.add_argument("--solver", action="store_true",
                   help="self-play, train (self-play and arena) and evaluate: MCTS-Solver -- wins, losses and draws proven from "
                        "terminal positions are propagated up the tree, a descent stops at a proven node below the root without "
                        "asking the network, and the arena plays a proven winning move when the root has one (default off; changes "
                        "which moves are picked; not with --leaves-per-step > 1, --board-semantics aliased or --reference-quirks)")
    p.add_argument("--gumbel-root", type=int, default=None, metavar="M",
                   help="self-play and train: Gumbel root search -- every root draws Gumbel noise, spends its simulations by "
                        "sequential halving over its M best actions, records the completed-Q policy target and plays the "
                        "Gumbel winner at every ply (2 .. 64; the paper: 16; default off; changes which moves are picked; "
                        "not with --leaves-per-step > 1, --board-semantics aliased, --reference-quirks, --forced-playouts, "
                        "--tree-reuse or --solver)")
    p.add_argument("--gumbel-c-visit", type=float, default=None, metavar="X",
                   help="c_visit of --gumbel-root's sigma (default 50)")
    p.add_argument("--gumbel-c-scale", type=float, default=None, metavar="Y",
                   help="c_scale of --gumbel-root's sigma (default 1.0)")
    p.add_argument("--gumbel-interior", action="store_true",
                   help="self-play and train, with --gumbel-root: the rest of Gumbel AlphaZero -- the root keeps its network value, "
                        "unvisited children are completed with v_mix in the policy target, and a descent below the root takes the "
                        "child of largest improved-policy share less visit share instead of the PUCT choice (default off; changes "
                        "which moves are picked; not with --fpu-reduction)")
    return p.parse_args(argv)


# What each mode hands to the options resolver (the package's options.resolve: the one copy of the rules), one call per tuple.
# train's self-play always runs on copied boards without the quirks, so --tree-reuse and --free-running do not look at those two
# flags there; --leaves-per-step > 1 has always refused them in train mode too and still does: the second call.
_SEARCH = ("num_simulations", "leaves_per_step", "fast_simulations", "full_search_probability", "tree_reuse", "free_running",
           "evaluation_symmetry", "forced_playouts", "fpu_reduction", "fpu_reduction_root", "shared_evaluations",
           "shared_evaluations_replace", "solver", "gumbel_root", "gumbel_c_visit", "gumbel_c_scale",
           "gumbel_interior")
HANDED = {"self-play": [_SEARCH + ("board_semantics", "reference_quirks")],
          "train": [_SEARCH, ("leaves_per_step", "board_semantics", "reference_quirks")],
          "evaluate": [("leaves_per_step", "tree_reuse", "fpu_reduction", "fpu_reduction_root", "solver")]}


def _handed(args, names):
    """The flags' values under the option names `names`."""
    return {n: getattr(args, "simulations" if n == "num_simulations" else n) for n in names}


def _flag(args, name):
    """An option's name as its flag, with the value it was given."""
    attr = "simulations" if name == "num_simulations" else name
    flag, value = "--" + attr.replace("_", "-"), getattr(args, attr)
    return flag if value is True else f"{flag} {value}"


def refused(args):
    """The flag combinations no search runs with, as a one-line message (None: none), from the parsed flags alone: the
    resolver's verdict, its option names rendered as flags."""
    from yinyang_game_alphazero_amd import options       # imports neither torch nor numpy
    for names in HANDED[args.mode]:
        try:
            options.resolve(**_handed(args, names))
        except options.OptionConflict as e:
            others = ", ".join(_flag(args, n) for n in e.conflicts)
            return f"train_alphazero.py: {_flag(args, e.option)}: {'not with ' + others if others else 'out of range'} ({e})"
    return None


def main(argv=None):
    args = parse_args(argv)
    if refused(args):
        sys.exit(refused(args))
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    rank = int(os.environ.get("RANK", "0"))
    if not torch.cuda.is_available():
        sys.exit("train_alphazero.py: no ROCm device -- the self-play engine has no CPU fallback")
    if args.dist_backend == "gloo":
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    if world > 1:
        import torch.distributed as dist
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo")
    import yinyang_game_alphazero_amd as pkg
    game = pkg.YinYangGame(args.rows, args.cols)
    for d in (args.model_dir, args.data_dir):
        os.makedirs(d, exist_ok=True)
    if args.mode == "train" and args.fresh:
        import glob
        if rank == 0:
            for f in glob.glob(os.path.join(args.model_dir, "checkpoint*.pth.tar")) + [os.path.join(args.model_dir, n) for n in
                                                                                     ("current_model.pth.tar", "best_model.pth.tar")]:
                if os.path.exists(f):
                    os.remove(f)
        if world > 1:
            dist.barrier()
    if args.mode == "train":                     # train_alphazero.py:84-101
        az = pkg.AlphaZero(game, args.model_dir, args.data_dir, num_iterations=args.iterations, num_episodes=args.episodes,
                           num_epochs=args.epochs, num_workers=args.workers,
                           mcts_threads=args.mcts_threads, nn_mode=args.nn, concurrent_games=args.concurrent_games,
                           arena_games=args.arena_games, num_channels=args.channels, num_res_blocks=args.blocks,
                           lr=args.lr, batch_size=args.batch_size, **_handed(args, _SEARCH + ("symmetry_seed",)))
        hist = az.run()
        if rank == 0:
            print(json.dumps({"iterations": hist}))
        if world > 1:
            dist.destroy_process_group()
        return
    model_path = os.path.join(args.model_dir, args.output_model)
    if args.mode == "evaluate":                  # train_alphazero.py:124-243: 10 games against RandomPlayer
        if not os.path.exists(model_path):
            sys.exit(f"Model file not found: {model_path}")
        res = pkg.evaluate_vs_random(game, model_path, num_games=10, num_simulations=args.simulations, nn_mode=args.nn,
                                     num_channels=args.channels, num_res_blocks=args.blocks, **_handed(args, HANDED["evaluate"][0]))
        print(json.dumps(res))
        return
    if not os.path.exists(model_path):           # same contract as the reference (train_alphazero.py:107-109)
        sys.exit(f"Model file not found: {model_path}")
    path = pkg.generate_self_play_data(game, model_path, args.data_dir, num_games=args.episodes, num_workers=args.workers,
                                       concurrent_games=args.concurrent_games, nn_mode=args.nn, seed=args.seed,
                                       num_channels=args.channels, num_res_blocks=args.blocks,
                                       reference_format=args.reference_format,
                                       evaluation_reuse=None if args.evaluation_reuse == "auto" else False,
                                       opening_book_stones=0 if args.leaves_per_step > 1 else args.opening_book_stones,
                                       lanes=args.lanes or None,
                                       **_handed(args, HANDED["self-play"][0] + ("symmetry_seed",)))
    if rank == 0:
        st = pkg.generate_self_play_data.last_stats
        st = dict(st, positions_per_s=st["positions"] / st["seconds"], expansions_per_s=st["evals"] / st["seconds"])
        print(json.dumps({"data_file": path, "rank0_stats": st}))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
