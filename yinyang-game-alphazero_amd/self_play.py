"""Self-play: the batched lockstep engine (throughput path) and the reference's self-play API.

Reference: src/yin_yang/ai/self_play.py -- SelfPlayWorker.play_game :72-192, generate_games
:194-216, SelfPlayManager :218-335, generate_self_play_data :337-387.

`SelfPlayEngine` is the MI355X design: G games advance in lockstep on one GPU; per move every
game runs `num_simulations` simulations, each simulation being ONE fused HIP kernel
(expand+backup of the previous leaves, PUCT select + rules + plane encode of the next) and ONE
batched CNN forward over all G leaves, replayed from a hipGraph.  Finished games are replaced in
their slot so the batch stays full.  Episodes shard across ranks (one process per GPU) and the
(state, pi, z) examples are collected with one all-gather at the end (`gather_examples`).

`SelfPlayWorker` / `SelfPlayManager` / `generate_self_play_data` keep the reference's names and
signatures.  `reference_quirks=True` reproduces Q4/Q5 of SURVEY.md (always search and mask as
player +1, never alternate the value labels); `board_semantics="aliased"` reproduces Q2.
"""
import contextlib
import os
import time

import numpy as np
import torch

from . import engine, options
from ._lib import YY_E_ARENA, YYError
from .game import YinYangLogic
from .mcts import MCTS
from .network import BatchedEvaluator, YinYangNeuralNetwork
from .search import FreeRunningSearch, LockstepSearch

DRAW = 1e-4


def _opening_book(opening_book, game, evaluator, device, symmetry=("off", None)):
    """An engine.OpeningBook as it is; a stone count N -> the book of every position with <= N stones, None for N <= 0, built
    under `symmetry` = (evaluation_symmetry, symmetry_seed) of the contexts that will read it."""
    if not isinstance(opening_book, int):
        return opening_book
    R, C = game.getBoardSize()
    return (engine.OpeningBook(R, C, evaluator, opening_book, rowcol=bool(getattr(game, "rowcol_rule", False)), device=device,
                               evaluation_symmetry=symmetry[0], symmetry_seed=symmetry[1])
            if opening_book > 0 else None)


def free_running_step_bound(num_games, slots, actions, num_simulations):
    """Steps a free-running run of num_games games on `slots` slots can need at most.  A game is at most A + 2 moves of
    num_simulations + 1 steps each = L steps; a free slot takes the next game at once (greedy list scheduling), so the last
    game starts no later than the mean load num_games * L / slots and the run ends within (ceil(num_games / slots) + 1) * L.
    The host stops with an error there instead of spinning: beyond it something is wrong."""
    return (-(-int(num_games) // max(1, int(slots))) + 1) * (int(actions) + 2) * (int(num_simulations) + 1)


def sort_examples(ex):
    """The examples ordered by (game_id, ply), on their device: the order free-running runs return, whatever order the games
    finished in."""
    if ex["game_id"].numel() == 0:
        return ex
    span = int(ex["ply"].max()) + 1
    order = torch.argsort(ex["game_id"] * span + ex["ply"], stable=True)
    return {k: v.index_select(0, order) for k, v in ex.items()}


def _play_lockstep(eng, progress=None):
    """play_move() until no game of `eng` (LockstepEngine or lockstep SelfPlayLanes, armed by begin_run) is alive; returns the
    examples."""
    moves = 0
    while eng.n_alive > 0:
        eng.play_move()
        moves += 1
        if moves % 8 == 0:
            eng.ctx.status()     # a failed search (NaN from the evaluator, arena overflow) stops the run now, not at its end
        if progress and moves % 10 == 0:
            progress(eng)
    eng.ctx.status()             # per-game search errors are sticky on the device: any failure of any move raises here
    return eng.collect()


# =============================================================================== batched engine
class _Engine:
    """What the lockstep and the free-running engine share: the options, the geometry, the tree context with its reuse
    defaults resolved, the book, the counters, and run / collect / close."""
    free_running = False

    def __init__(self, game, evaluator, num_simulations=800, concurrent_games=4096, cpuct=1.0,
                 dirichlet_alpha=0.3, dirichlet_epsilon=0.25, temperature_threshold=10,
                 board_semantics="copied", reference_quirks=False, use_graph=True, seed=0,
                 device=None, first_game_index=0, game_index_stride=1,
                 reuse_pass_value=None, reuse_transpositions=None, keep_evaluations=None,
                 opening_book=None, stream=None, rng="philox", leaves_per_step=1,
                 fast_simulations=None, full_search_probability=1.0, tree_reuse=False, evaluation_symmetry="off",
                 symmetry_seed=None, forced_playouts=None, fpu_reduction=None, fpu_reduction_root=None, shared_evaluations=None,
                 shared_evaluations_replace=False, solver=False, gumbel_root=None, gumbel_c_visit=None, gumbel_c_scale=None, gumbel_interior=False):
        """gumbel_root m (default off) with gumbel_c_visit / gumbel_c_scale: the Gumbel root search in every search, fast and full
        alike (options.SearchOptions) -- every root draws its Gumbel variables from the game's own counter stream (keyed by seed,
        game index and ply), spends its budget by sequential halving, records the completed-Q policy target as pi and plays
        the Gumbel winner at every ply: the temperature rule and the move draw are not consulted.  dirichlet_epsilon = 0 is
        recommended with it (the Gumbel variables are the root's exploration).
        solver (default off): the MCTS-Solver in every search, fast and full alike (options.SearchOptions) -- descents stop
        at proven nodes below the root and ask for no evaluator row; the move draw and the recorded pi are computed from the
        visit counts as without it and do not look at proofs.
        shared_evaluations_replace (needs shared_evaluations): the table in its replacing form (engine.SharedEvaluations
        replace=True): one slot per position, and the engine sweeps it -- the lockstep engine once per move, after the move and
        the re-rooting of tree_reuse, the free-running engine at every poll, between two graph replays -- so that it sheds what
        is no longer used; `self.shared.high_water` may be set between sweeps.  The same games.
        shared_evaluations (None / False: off; True: the default size; an int: slots, rounded up to a power of two): the games
        of this engine share their evaluations through an engine.SharedEvaluations table of the engine's own (`self.shared`),
        tied to its evaluator and (evaluation_symmetry, symmetry_seed); same games, fewer evaluator rows.  Needs an evaluator
        that declares `row_independent` (ValueError otherwise).
        leaves_per_step, fast_simulations / full_search_probability, tree_reuse, evaluation_symmetry / symmetry_seed (None: `seed`),
        forced_playouts (the recorded pi and the move draw use the pruned counts; fast and full searches alike),
        fpu_reduction / fpu_reduction_root (first-play urgency reduction in every search, fast and full alike)
        and the mode (free_running): options.SearchOptions; a refused combination raises ValueError before anything touches the
        device.  An opening_book built under another (evaluation_symmetry, symmetry_seed) is refused (ValueError).
        reuse_pass_value / reuse_transpositions / keep_evaluations: None = on when the boards are copied and the evaluator
        declares `row_independent` (the split-f16 evaluator does); off at leaves_per_step > 1.  The reference asks the network
        for every leaf: a node without legal moves again on every visit (ai/mcts.py:93-95, 371-397), a position another move
        order of the same search already reached (:385-397), a position the previous move's search evaluated -- and gets the
        same numbers each time.  With these options the search takes them from the tree / from a per-game evaluation cache in
        HBM instead (YY_FLAG_REUSE_PASS_VALUE, YY_FLAG_REUSE_TRANSPOSITIONS, YY_FLAG_KEEP_EVALUATIONS in include/yy_engine.h).
        The games played are the same, move for move; the evaluator sees a fraction of the rows.  The engine owns ONE evaluator
        for its lifetime, which is what keep_evaluations needs.
        opening_book: an engine.OpeningBook built with THIS evaluator, or a stone count N to build one here (every position
        reachable with <= N stones is evaluated once, in large batches, before play; all games start from the empty board, so
        the first plies of every game search the same positions), or None.
        rng: "philox" (default) = the per-game counter streams of csrc/yy_selfplay.hip, drawn on the device; "numpy"
        (LockstepEngine) = the reference's generator."""
        assert board_semantics in ("aliased", "copied")
        assert rng in ("philox", "numpy")
        opts = options.resolve(num_simulations, leaves_per_step, board_semantics, reference_quirks, rng,
                               (reuse_pass_value, reuse_transpositions, keep_evaluations), opening_book, fast_simulations,
                               full_search_probability, tree_reuse, self.free_running, evaluation_symmetry, symmetry_seed,
                               forced_playouts, fpu_reduction, fpu_reduction_root, shared_evaluations, shared_evaluations_replace,
                               solver, gumbel_root=gumbel_root, gumbel_c_visit=gumbel_c_visit, gumbel_c_scale=gumbel_c_scale, gumbel_interior=gumbel_interior)
        if opts.shared_evaluations and not getattr(evaluator, "row_independent", False):
            raise ValueError("shared_evaluations: a stored row stands in for the evaluator's, so the evaluator must declare "
                             "`row_independent` (a row's result does not depend on the rest of the batch); this one does not")
        self.options = opts
        self.K, self.tree_reuse, self.forced_playouts, self.solver = opts.leaves_per_step, opts.tree_reuse, opts.forced_playouts, opts.solver
        self.symmetry = engine.symmetry_key(opts.evaluation_symmetry, seed if opts.symmetry_seed is None else opts.symmetry_seed)
        self.fast_sims, self.p_full = opts.fast_simulations, opts.full_search_probability
        self.game = game
        self.R, self.C = game.getBoardSize()
        self.A = self.R * self.C
        self.G = int(concurrent_games)
        self.sims = int(num_simulations)
        self.alpha, self.eps = float(dirichlet_alpha), float(dirichlet_epsilon)
        self.thr = int(temperature_threshold)
        self.aliased = board_semantics == "aliased"
        self.quirks = bool(reference_quirks)
        self.rowcol = bool(getattr(game, "rowcol_rule", False))
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.evaluator, self.use_graph = evaluator, use_graph
        self.stream = stream                       # HIP stream every launch of this engine goes to (None: the caller's current one)
        auto = self.K == 1 and (not self.aliased) and bool(getattr(evaluator, "row_independent", False))
        self.reuse_pass_value, self.reuse_transpositions, self.keep_evaluations = (
            bool(auto if x is None else x) for x in (reuse_pass_value, reuse_transpositions, keep_evaluations))
        self.ctx = engine.BatchedMCTS(self.G, self.R, self.C, self.sims, cpuct=cpuct, aliased=self.aliased,
                                      rowcol=self.rowcol, device=self.device, reuse_pass_value=self.reuse_pass_value,
                                      reuse_transpositions=self.reuse_transpositions, keep_evaluations=self.keep_evaluations,
                                      **opts.tree_keywords(seed))
        self.book = _opening_book(opening_book, game, evaluator, self.device, self.symmetry)
        if self.book is not None:
            self.ctx.set_book(self.book)
        # one table per context: the kernel boundary of the context's own stream is what publishes its entries
        self.shared = (engine.SharedEvaluations(self.R, self.C, opts.shared_evaluations, self.device, *self.symmetry,
                                                replace=opts.shared_evaluations_replace)
                       if opts.shared_evaluations else None)
        if self.shared is not None:
            with self._on_stream():
                self.ctx.set_shared_evaluations(self.shared)
        self.seed = int(seed)                     # key of the per-game counter streams (csrc/yy_selfplay.hip)
        self.rng = rng
        self.first_game_index, self.stride = int(first_game_index), int(game_index_stride)
        # a game has at most A placements; passes never add examples.  Literal quirk mode can make
        # no-op moves (illegal placements), so leave generous room there.
        self.T = self.A + 2 if not self.quirks else 4 * self.A + 8
        self.n_alive = 0       # live games, tracked on the host (no device read needed)
        self.positions = 0
        self.recorded = 0      # examples recorded so far (== positions without playout cap)
        self.games_started = self.games_finished = self.games_target = 0
        self.steps_issued = 0  # free-running: steps put on the stream so far
        self.out = []          # finished examples: dicts of device tensors (states, policies, values, game_id, ply)

    def _on_stream(self):
        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def run(self, num_games, progress=None):
        """Play `num_games` games to completion; returns the examples (device tensors)."""
        self.begin_run(num_games)
        return self.play_to_completion(progress)

    def collect(self):
        """The examples finished since the last collect(); a free-running engine's sorted by (game_id, ply)."""
        out, self.out = self.out, []
        if not out:
            e = torch.empty
            return dict(states=e((0, self.R, self.C), dtype=torch.int8, device=self.device),
                        policies=e((0, self.A), dtype=torch.float32, device=self.device),
                        values=e((0,), dtype=torch.float32, device=self.device),
                        game_id=e((0,), dtype=torch.int64, device=self.device),
                        ply=e((0,), dtype=torch.int64, device=self.device))
        ex = {k: torch.cat([o[k] for o in out]) for k in out[0]}
        return sort_examples(ex) if self.free_running else ex

    def memory_bytes(self):
        """HBM of the search state: the tree context (arenas and the per-game evaluation cache), the opening book and the
        shared evaluation table."""
        return dict(context=self.ctx.memory_bytes(), book=self.book.bytes if self.book is not None else 0,
                    shared_evaluations=self.shared.memory_bytes if self.shared is not None else 0)

    def close(self):
        self.ctx.close()
        self.shared = None


class LockstepEngine(_Engine):
    """G games advance in lockstep: one search and one move of every live game per play_move(), finished games replaced in
    their slot (the module docstring)."""

    def __init__(self, *args, compact_tail=True, row_tiers=None, numpy_seeds=None, **kwargs):
        """The other arguments are _Engine's.  rng="numpy" = the REFERENCE's generator and call sequence, per game: a host numpy RandomState(numpy_seeds[game index],
        default seed + index) draws np.random.dirichlet at the game's first search (ai/mcts.py:305) and np.random.choice for
        every move (ai/self_play.py:146, 160) exactly where SelfPlayWorker.play_game draws from the global stream after
        np.random.seed(s) -- a batch of games then replays the reference's transcripts move for move (tests: episodes_*.npz).
        One host round trip of (pi, legal mask) per move: a parity mode, not the throughput path."""
        super().__init__(*args, **kwargs)
        self.search = LockstepSearch(self.ctx, self.evaluator, use_graph=self.use_graph)
        self.numpy_seeds, self._rs = numpy_seeds, {}
        self._pending = None                       # a move enqueued by enqueue_move() and not yet finished
        self._evals_seen = 0                       # tree-context counter at the end of the last move (rows_hint)
        self._stats_host = None                    # pinned record of the move's one host read, made at the first move
        dev, G, T = self.device, self.G, self.T
        self.boards = torch.zeros((G, self.R, self.C), dtype=torch.int8, device=dev)
        self.players = torch.ones(G, dtype=torch.int8, device=dev)
        self.ply = torch.zeros(G, dtype=torch.int32, device=dev)
        self.n_ex = torch.zeros(G, dtype=torch.int64, device=dev)
        self.alive = torch.zeros(G, dtype=torch.bool, device=dev)
        self.game_id = torch.full((G,), -1, dtype=torch.int64, device=dev)
        self.hist_state = torch.zeros((G, T, self.R, self.C), dtype=torch.int8, device=dev)
        self.hist_pi = torch.zeros((G, T, self.A), dtype=torch.float32, device=dev)
        self.hist_player = torch.zeros((G, T), dtype=torch.int8, device=dev)
        # playout cap: the examples of a game are its fully searched moves only, so an example's index is not its ply
        self.hist_ply = torch.zeros((G, T), dtype=torch.int64, device=dev) if self.fast_sims is not None else None
        self._ar = torch.arange(G, device=dev)
        # Gumbel root search: the rows the root expansions read, redrawn in place before every search (captured steps hold
        # the pointer); the free-running run has rows of its own (engine.SelfPlayRun)
        self.gumbel_rows = torch.zeros((G, self.A), dtype=torch.float32, device=dev) if self.options.gumbel_root else None
        if self.options.gumbel_root:
            self.ctx.set_gumbel(self.gumbel_rows)
        self._ones = torch.ones(G, dtype=torch.int8, device=dev)
        # draining batch: once no new game will start, live games are packed to the front and only the leaf rows of the first
        # `rows` GAMES are evaluated (rows = the smallest tier that holds them; one captured step per tier).  rows and the tiers
        # count games at any leaves_per_step: LockstepSearch turns them into rows * K evaluator rows
        self.compact_tail = bool(compact_tail)
        self.rows = G
        self.tiers = sorted({G} | ({m for m in range(1024, G, 1024)} | {m for m in (512, 256) if m < G}
                                   if row_tiers is None else {int(t) for t in row_tiers if 0 < int(t) < G}))

    def _pack_live_games(self):
        """Once per tier change: stable permutation of every per-slot tensor, live games first (the Gumbel rows are redrawn
        per move from (game id, ply) and stay in place)."""
        perm = torch.argsort((~self.alive).to(torch.int8), stable=True)
        for name in ("boards", "players", "ply", "n_ex", "alive", "game_id", "hist_state", "hist_pi", "hist_player") + (
                ("hist_ply",) if self.hist_ply is not None else ()):
            setattr(self, name, getattr(self, name).index_select(0, perm).contiguous())

    # ---- slots
    def _start_games(self, slots):
        n = int(slots.numel())
        if n == 0:
            return
        ids = self.first_game_index + (self.games_started + torch.arange(n, device=self.device)) * self.stride
        self.games_started += n
        self.n_alive += n
        self.rows = self.G                            # new games may sit anywhere
        self.boards[slots] = 0
        self.players[slots] = 1                       # black starts (self_play.py:81)
        self.ply[slots] = 0
        self.n_ex[slots] = 0
        self.alive[slots] = True
        self.game_id[slots] = ids

    def _finalize(self, over, result, final_player):
        """Label and emit the examples of the games in `over` (self_play.py:114-121, 170-188), then
        refill their slots."""
        idx = over.nonzero(as_tuple=True)[0]
        if idx.numel() == 0:
            return
        n = self.n_ex[idx]
        sel = torch.arange(self.T, device=self.device)[None, :] < n[:, None]          # [k,T]
        res = result[idx].to(torch.float64)
        if self.quirks:
            z = res[:, None].expand(-1, self.T)                                          # Q5: never alternates
        else:
            same = self.hist_player[idx] == final_player[idx][:, None]
            z = torch.where(same, res[:, None], -res[:, None])
        states = self.hist_state[idx]
        if self.quirks and self.aliased:
            states = self.boards[idx][:, None].expand(-1, self.T, -1, -1)               # Q5: all alias the final board
        gid = self.game_id[idx][:, None].expand(-1, self.T)
        plyi = (torch.arange(self.T, device=self.device)[None, :].expand(idx.numel(), -1) if self.hist_ply is None
                else self.hist_ply[idx])
        self.out.append(dict(states=states[sel], policies=self.hist_pi[idx][sel], values=z[sel].to(torch.float32),
                             game_id=gid[sel], ply=plyi[sel]))
        self.games_finished += int(idx.numel())
        self.n_alive -= int(idx.numel())
        self.alive[idx] = False
        self.game_id[idx] = -1
        room = max(0, self.games_target - self.games_started)
        self._start_games(idx[:room])

    # ---- one lockstep move for every live game (self_play.py:91-192)
    # ---- rng="numpy": the reference's generator, one RandomState per game
    def _numpy_stream(self, gid):
        rs = self._rs.get(gid)
        if rs is None:
            seed = self.seed + gid if self.numpy_seeds is None else int(self.numpy_seeds[gid])
            rs = self._rs[gid] = np.random.RandomState(seed)
        return rs

    def _numpy_actions(self, searching, pi, mask_u8):
        """self_play.py:143-160 on the host, game by game, from each game's own RandomState."""
        idx = searching.nonzero(as_tuple=True)[0]
        action = torch.full((self.G,), -1, dtype=torch.int32, device=self.device)
        if idx.numel() == 0:
            return action
        pi_h, m_h = pi[idx].cpu().numpy(), mask_u8[idx].cpu().numpy().astype(np.float64)
        gid_h, ply_h = self.game_id[idx].cpu().numpy(), self.ply[idx].cpu().numpy()
        out = np.zeros(len(gid_h), np.int32)
        for j, gid in enumerate(gid_h):
            rs, p, valid = self._numpy_stream(int(gid)), pi_h[j], m_h[j]
            if ply_h[j] >= self.thr:                                           # temperature 0: random among the most visited
                out[j] = rs.choice(np.where(p == np.max(p))[0])
            else:
                probs = p * valid
                if np.sum(probs) > 0:
                    probs = probs / np.sum(probs)
                else:
                    vi = np.flatnonzero(valid)
                    probs = np.zeros_like(valid)
                    probs[vi] = 1.0 / len(vi)
                out[j] = rs.choice(len(probs), p=probs)
        action[idx] = torch.from_numpy(out).to(self.device)
        return action

    def play_move(self):
        """One lockstep move of every live game: enqueue_move() + finish_move()."""
        self.enqueue_move()
        return self.finish_move()

    def finish_move(self):
        """Waits for the move enqueue_move() put on the engine's stream, reads its one small statistics record (positions
        searched, games finished) and, when games finished, labels their examples and refills their slots."""
        assert self._pending is not None, "finish_move() without enqueue_move()"
        host, event, fin, fin_res, fin_player = self._pending
        self._pending = None
        event.synchronize()
        if hasattr(self.evaluator, "rows_hint"):
            # the stream is idle here: rows the evaluator was asked for per step of this move (also surfaces a failed search now)
            evals = self.ctx.status()["evals"]
            if evals >= self._evals_seen:
                self.evaluator.rows_hint(id(self.search), (evals - self._evals_seen) / float(self.ctx.steps(self.sims) + 1))
            self._evals_seen = evals
        n_pos, n_fin = int(host[0]), int(host[1])
        self.positions += n_pos
        self.recorded += int(host[2]) if self.fast_sims is not None else n_pos
        if n_fin:
            with self._on_stream():
                self._finalize(fin, fin_res, fin_player)
        return n_pos

    def enqueue_move(self):
        """Every per-move decision is taken on the device with fixed-shape masked operations and ENQUEUED on the engine's
        stream without waiting: the host reads ONE small statistics record per move, in finish_move().  Random draws come from the
        per-game counter streams of csrc/yy_selfplay.hip, so a game's noise and moves depend only on (seed, global game index,
        ply).  Between the two calls the host is free to enqueue the moves of other engines on other streams
        (SelfPlayLanes): their kernels fill the compute units this engine's partly empty last round of workgroups leaves idle."""
        assert self._pending is None, "enqueue_move() twice without finish_move()"
        with self._on_stream():
            self._enqueue_move()

    def _enqueue_move(self):
        dev, G = self.device, self.G
        if self.compact_tail and self.games_started >= self.games_target:      # the batch is draining
            need = next(t for t in self.tiers if t >= self.n_alive)
            if need < self.rows:
                self._pack_live_games()
                self.rows = need
                if self.tree_reuse:                                            # the kept trees stayed in the old slots
                    self.ctx.advance(torch.full((G,), -1, dtype=torch.int32, device=dev))
        ones = self._ones
        pending = self.alive.clone()
        searching = torch.zeros(G, dtype=torch.bool, device=dev)
        passes = torch.zeros(G, dtype=torch.int32, device=dev)
        fin = torch.zeros(G, dtype=torch.bool, device=dev)                     # games that end in this move
        fin_res = torch.zeros(G, dtype=torch.float64, device=dev)
        fin_player = self.players.clone()
        for _ in range(2):                                                     # pass handling :103-125
            rp = ones if self.quirks else self.players                         # Q4
            has = engine.valid_mask(self.boards, rp.contiguous(), self.rowcol).bool().any(1)
            go = pending & has
            searching |= go
            pending &= ~go
            nomove = pending & ~has
            passes += nomove.to(torch.int32)
            over = nomove & (passes >= 2)
            r = engine.game_ended(self.boards, self.players, self.rowcol)
            r = torch.where(r == 0, torch.full_like(r, DRAW), r)               # :110-112
            fin |= over
            fin_res = torch.where(over, r, fin_res)
            fin_player = torch.where(over, self.players, fin_player)
            pending &= ~over
            flip = nomove & ~over
            self.players = torch.where(flip, -self.players, self.players)
        searching &= self.alive
        rp = (ones if self.quirks else self.players).contiguous()
        mask_u8 = engine.valid_mask(self.boards, rp, self.rowcol)
        s_u8 = searching.to(torch.uint8)
        noise = None
        if self.eps > 0 and self.rng == "numpy":                               # the reference's own draw, game by game (mcts.py:298-312)
            first = (searching & (self.ply == 0)).nonzero(as_tuple=True)[0]
            noise = torch.zeros((G, self.A), dtype=torch.float64, device=dev)
            if first.numel():
                m_host, gid_host = mask_u8[first].cpu().numpy(), self.game_id[first].cpu().numpy()
                rows = np.zeros((len(gid_host), self.A), np.float64)
                for j, gid in enumerate(gid_host):
                    idx = np.flatnonzero(m_host[j])
                    rows[j, idx] = self._numpy_stream(int(gid)).dirichlet([self.alpha] * len(idx))
                noise[first] = torch.from_numpy(rows).to(dev)
        elif self.eps > 0:                                                     # add_noise = (step == 0), :131
            first = (searching & (self.ply == 0)).to(torch.uint8)
            noise = engine.root_noise(self.seed, self.game_id, self.ply, first, mask_u8, self.alpha)
        if self.options.gumbel_root:                                                        # every root, every ply: the game's own stream
            engine.gumbel_rows(self.seed, self.game_id, self.ply, self.A, out=self.gumbel_rows)
        record = searching                                                     # the games whose move becomes an example
        if self.fast_sims is None:
            self.search.run(self.boards, rp, self.sims, noise=noise, eps=self.eps, active=s_u8, rows=self.rows)
        else:                                                                  # playout cap: a full or a fast search, game by game
            budgets, is_full = engine.draw_budgets(self.seed, self.game_id, self.ply, s_u8, self.p_full, self.sims, self.fast_sims)
            self.search.run(self.boards, rp, budgets, noise=noise, eps=self.eps, active=s_u8, rows=self.rows,
                            num_sims_bound=self.sims)
            record = searching & is_full.bool()
        pi = self.ctx.root_policy()                                            # T == 1 distribution, :329
        # ---- record the example before the move (:140): fixed-shape scatter, rows of idle games rewrite themselves
        ar, slot = self._ar, self.n_ex.clamp_max(self.T - 1)
        self.hist_state[ar, slot] = torch.where(record[:, None, None], self.boards, self.hist_state[ar, slot])
        self.hist_pi[ar, slot] = torch.where(record[:, None], pi.to(torch.float32), self.hist_pi[ar, slot])
        self.hist_player[ar, slot] = torch.where(record, self.players, self.hist_player[ar, slot])
        if self.hist_ply is not None:
            self.hist_ply[ar, slot] = torch.where(record, self.ply.to(torch.int64), self.hist_ply[ar, slot])
        self.n_ex += record.to(torch.int64)
        # ---- choose the action (:143-160) from the game's own stream
        if self.options.gumbel_root:                                                        # the Gumbel winner, at every ply (no draw)
            action = torch.where(searching, self.ctx.root_gumbel_action(), torch.full((G,), -1, dtype=torch.int32, device=dev))
        elif self.rng == "numpy":
            action = self._numpy_actions(searching, pi, mask_u8)
        else:
            action = engine.sample_actions(self.seed, self.game_id, self.ply, s_u8, pi, mask_u8, self.thr)
        # ---- make the move (:163); aliased: the search has mutated the game's board (Q2)
        if self.aliased:
            self.boards = torch.where(searching[:, None, None], self.ctx.boards(), self.boards)
        old_players = self.players
        self.players = self.players.clone()
        engine.step_(self.boards, self.players, action, self.rowcol)
        self.players = torch.where(searching, self.players, old_players)
        self.ply += searching.to(torch.int32)
        ended = engine.game_ended(self.boards, self.players, self.rowcol)      # :167
        done = searching & (ended != 0)
        fin |= done
        fin_res = torch.where(done, ended, fin_res)
        fin_player = torch.where(done, self.players, fin_player)
        if self.tree_reuse:
            # re-root every tree at the move played; a game that ended (its slot may be refilled) or did not search keeps nothing
            self.kept_visits = self.ctx.advance(torch.where(fin, torch.full_like(action, -1), action))
        if self.shared is not None and self.shared.replace:
            self.shared.sweep()                                                # once per move: no select is pending here
        counts = [searching.sum(), fin.sum()] + ([record.sum()] if self.fast_sims is not None else [])
        stats = torch.stack(counts)                                            # the move's one host read, taken in finish_move()
        if self._stats_host is None:
            self._stats_host = torch.zeros(len(counts), dtype=stats.dtype).pin_memory()
        self._stats_host.copy_(stats, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        self._pending = (self._stats_host, event, fin, fin_res, fin_player)

    def begin_run(self, num_games):
        """Arm the engine for `num_games` more games: the first ones start in the free slots, the others as slots free up."""
        with self._on_stream():
            self.games_target = self.games_started + int(num_games)
            free = (~self.alive).nonzero(as_tuple=True)[0]
            self._start_games(free[: int(num_games)])

    play_to_completion = _play_lockstep


class FreeRunningEngine(_Engine):
    """The games play their moves on the device, inside the search step (options.SearchOptions free_running); the host replays
    steps and polls the counters of the run's device state (engine.SelfPlayRun, made by begin_run for the run's game count)."""
    free_running = True

    def __init__(self, *args, poll_steps=None, compact_tail=None, row_tiers=None, numpy_seeds=None, **kwargs):
        """poll_steps: steps between two polls of the run's counters (default: four unrolled graphs).  compact_tail, row_tiers and
        numpy_seeds are the lockstep engine's and do not apply; the other arguments are _Engine's."""
        super().__init__(*args, **kwargs)
        self.poll_steps = poll_steps
        # the steps are FreeRunningSearch's, made with the run's device state by begin_run
        self.run_state = self.free_search = self._run_open = self._tick = None
        self._example_capacity = None      # rows of the example buffer; None: num_games * (A + 2), which always fits

    def play_move(self, *args):
        raise RuntimeError("free_running=True: the games play their moves on the device, there is no lockstep move "
                           "(play_move / enqueue_move / finish_move) -- use run() or begin_run() + play_to_completion()")

    enqueue_move = finish_move = play_move

    def begin_run(self, num_games):
        """Make (or reuse) the run's device state, sized for num_games games, and put every slot's first root on the stream."""
        n = int(num_games)
        if self._run_open is not None:
            raise RuntimeError("begin_run() while a free-running run is in progress: play_to_completion() first")
        cap = max(1, n * (self.A + 2)) if self._example_capacity is None else int(self._example_capacity)
        with self._on_stream():
            if self.run_state is None or (self.run_state.capacity < cap if self._example_capacity is None
                                          else self.run_state.capacity != cap):
                if self.run_state is not None:
                    self.run_state.close()
                self.run_state = engine.SelfPlayRun(self.ctx, self.seed, self.sims, cap, self.alpha, self.eps, self.thr,
                                                    self.fast_sims, self.p_full)
                self.free_search = FreeRunningSearch(self.ctx, self.evaluator, self.run_state, use_graph=self.use_graph)
            self.run_state.arm(n, self.first_game_index + self.games_started * self.stride, self.stride)
        self.games_target = self.games_started + n
        self.n_alive = n
        self._run_open = n

    def play_to_completion(self, progress=None):
        """Replay steps on the engine's stream until the run begin_run() armed is over; returns the examples.  Every poll_steps
        steps the counter copy is enqueued with an event and the PREVIOUS poll's record is read, so the host never waits on the
        stream it is feeding; the run is over when finished + failed == its games.  Raises YYError when a search failed (the
        other games' examples stay collectable), when the example buffer overflowed, or when the run is not over after
        free_running_step_bound() steps."""
        while not self.tick():
            if progress:
                progress(self)
        return self.finish()

    def tick(self):
        """One batch of poll_steps steps and the poll behind it; reads the previous poll's record.  True: the run is over (or
        there is none)."""
        n = self._run_open
        if not n:
            return True
        if not isinstance(self._tick, dict):
            poll = max(1, int(self.poll_steps) if self.poll_steps else 4 * self.free_search.unroll)
            self._tick = dict(poll=poll, steps=0, prev=None, cur=None, bound=free_running_step_bound(n, self.G, self.A, self.sims))
        t, run = self._tick, self.run_state
        with self._on_stream():
            self.free_search.issue(t["poll"])
            if self.shared is not None and self.shared.replace:
                # between two graph replays, never captured: legal with selects pending (csrc/yy_shared_table.hip)
                self.shared.sweep()
            t["steps"] += t["poll"]
            self.steps_issued += t["poll"]
            t["prev"], t["cur"] = t["cur"], run.poll_counters() + (t["steps"],)
        if t["prev"] is None:
            return False
        event, record, steps_then = t["prev"]
        event.synchronize()                                # a whole batch of steps is queued behind it
        c = run.counters(record)
        if c["finished"] + c["failed"] >= n:
            return True
        if steps_then >= t["bound"]:
            self._run_open, self._tick, self.n_alive = None, None, 0
            raise YYError(-5, f"free-running self-play: {c['finished'] + c['failed']} of {n} games over after {steps_then} steps "
                              f"(bound {t['bound']}): something is wrong")
        return False

    def finish(self):
        """The run is over: its final counters, its examples; raises for failed searches and an overflowed example buffer."""
        n, t, run = self._run_open, self._tick, self.run_state
        self._run_open, self._tick, self.n_alive = None, None, 0
        if not n:
            return self.collect()
        t["cur"][0].synchronize()                          # issued after the poll that showed the end: the final counters
        c = run.counters(t["cur"][1])
        self.games_started += n
        self.positions += c["positions"]
        self.recorded += c["recorded"]
        self.games_finished += c["finished"]
        if c["overflow"]:
            raise YYError(-3, f"free-running self-play: the example buffer ({run.capacity} rows) is too small: the examples of "
                              f"{c['overflow']} games did not fit ({c['rows']} rows asked for)")
        with self._on_stream():
            self.out.append(run.examples(c["rows"]))
        if c["failed"]:
            try:
                self.ctx.status()                          # clears the sticky per-game flags that the count below reports
            except YYError:
                pass
            raise YYError(YY_E_ARENA, f"free-running self-play: {c['failed']} of {n} games failed (tree arena overflow or "
                                      f"non-finite evaluator output) and were abandoned, their examples dropped")
        self.ctx.status()
        return self.collect()

    def close(self):
        if self.run_state is not None:
            self.run_state.close()                 # before the context its kernels read
            self.run_state = self.free_search = None
        super().close()


def SelfPlayEngine(game, evaluator, *args, free_running=False, **kwargs):
    """The engine of one batch of games on one GPU: FreeRunningEngine with free_running=True, else LockstepEngine; the other
    arguments are the class's."""
    return (FreeRunningEngine if free_running else LockstepEngine)(game, evaluator, *args, **kwargs)


class _LaneCounters:
    """ctx-like view over the lanes' tree contexts: reset_counters() / status() summed over the lanes."""

    def __init__(self, lanes):
        self.lanes = lanes

    def reset_counters(self):
        for ln in self.lanes:
            with ln._on_stream():
                ln.ctx.reset_counters()

    def _summed(self, method_name):
        tot = {}
        for ln in self.lanes:
            for k, v in getattr(ln.ctx, method_name)().items():
                tot[k] = tot.get(k, 0) + v
        return tot

    def status(self):
        return self._summed("status")

    def shared_counters(self):
        return self._summed("shared_counters")

    def shared_counters_ex(self):
        return self._summed("shared_counters_ex")

    def solver_counters(self):
        return self._summed("solver_counters")


class SelfPlayLanes:
    """K independent SelfPlayEngine lanes of G / K games each on K HIP streams of ONE GPU, their moves enqueued back to back.

    Why: a lockstep step's evaluator launch holds only the leaves that need an evaluation -- ~3 800 of 4 096 without evaluation
    reuse, ~800 with it -- and a tower workgroup occupies a whole compute unit for the ~0.2-0.4 ms its boards take, so the last
    round of workgroups of every launch leaves compute units idle until the launch ends (402 two-board workgroups on 256 CUs =
    1.57 rounds = 2).  Games are independent, so the batch is cut into lanes whose steps are enqueued on separate streams: while
    one lane's launch drains, the other lane's workgroups take the free compute units -- the chip sees one continuous flow of
    workgroups instead of rounds.  A game's transcript depends only on (seed, global game index), never on its lane or slot,
    so the games played are the same as a single engine's (tests/test_gpu_selfplay.py::test_lanes_play_the_same_games).
    Lane k of K plays the games first_game_index + (k + j*K) * game_index_stride, j = 0, 1, ..."""

    def __init__(self, game, evaluator, num_simulations=800, concurrent_games=4096, lanes=2, seed=0, device=None,
                 first_game_index=0, game_index_stride=1, opening_book=None, board_semantics="copied", reference_quirks=False,
                 reuse_pass_value=None, reuse_transpositions=None, keep_evaluations=None, rng="philox", leaves_per_step=1,
                 fast_simulations=None, full_search_probability=1.0, tree_reuse=False, free_running=False, evaluation_symmetry="off",
                 symmetry_seed=None, forced_playouts=None, fpu_reduction=None, fpu_reduction_root=None, shared_evaluations=None,
                 shared_evaluations_replace=False, solver=False, gumbel_root=None, gumbel_c_visit=None, gumbel_c_scale=None, gumbel_interior=False, **engine_kwargs):
        """gumbel_root / gumbel_c_visit / gumbel_c_scale / gumbel_interior: the Gumbel root search in every lane (options.SearchOptions).
        solver: the MCTS-Solver in every lane (options.SearchOptions).
        shared_evaluations: every lane gets a shared evaluation table of its own (one per context and stream), each of the
        size asked for; memory_bytes() reports their sum.  shared_evaluations_replace: every lane's table is a replacing one,
        swept by its lane on the lane's stream.
        leaves_per_step, fast_simulations / full_search_probability, tree_reuse, free_running, evaluation_symmetry / symmetry_seed
        (None: `seed`, the same in every lane), forced_playouts, fpu_reduction / fpu_reduction_root: options.SearchOptions, in every lane; resolved here once, before the book or any
        lane is built.  Free-running lanes each run on their own stream and the host alternates their batches of graph replays.
        The other keywords are SelfPlayEngine's."""
        opts = options.resolve(num_simulations, leaves_per_step, board_semantics, reference_quirks, rng,
                               (reuse_pass_value, reuse_transpositions, keep_evaluations), opening_book, fast_simulations,
                               full_search_probability, tree_reuse, free_running, evaluation_symmetry, symmetry_seed,
                               forced_playouts, fpu_reduction, fpu_reduction_root, shared_evaluations, shared_evaluations_replace,
                               solver, gumbel_root=gumbel_root, gumbel_c_visit=gumbel_c_visit, gumbel_c_scale=gumbel_c_scale, gumbel_interior=gumbel_interior)
        self.free_running, self.leaves_per_step = opts.free_running, opts.leaves_per_step
        symmetry = engine.symmetry_key(opts.evaluation_symmetry, seed if opts.symmetry_seed is None else opts.symmetry_seed)
        engine_kwargs.update(board_semantics=board_semantics, reference_quirks=reference_quirks, rng=rng,
                             reuse_pass_value=reuse_pass_value, reuse_transpositions=reuse_transpositions,
                             keep_evaluations=keep_evaluations, **opts.keywords())
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        K = max(1, min(int(lanes), int(concurrent_games)))
        self.game, self.evaluator, self.sims = game, evaluator, int(num_simulations)
        self.book = _opening_book(opening_book, game, evaluator, self.device, symmetry)      # one book, shared read-only by every lane
        self.lanes = []
        for k in range(K):
            g_k = concurrent_games // K + (1 if k < concurrent_games % K else 0)
            with torch.cuda.device(self.device):
                st = torch.cuda.Stream(device=self.device) if K > 1 else None
            # the lane's tensors are allocated under its own stream, so the caching allocator never recycles one of them
            # for another stream while this stream still uses it
            with (torch.cuda.stream(st) if st is not None else contextlib.nullcontext()):
                self.lanes.append(SelfPlayEngine(game, evaluator, num_simulations=num_simulations, concurrent_games=g_k, seed=seed,
                                                 device=self.device, first_game_index=first_game_index + k * game_index_stride,
                                                 game_index_stride=K * game_index_stride, opening_book=self.book, stream=st,
                                                 **engine_kwargs))
        torch.cuda.synchronize(self.device)      # evaluator weights / the book were written on the caller's stream
        ln = self.lanes[0]
        self.G = sum(l.G for l in self.lanes)
        self.R, self.C, self.A, self.T = ln.R, ln.C, ln.A, ln.T
        self.reuse_pass_value, self.reuse_transpositions, self.keep_evaluations = ln.reuse_pass_value, ln.reuse_transpositions, ln.keep_evaluations
        self.ctx = _LaneCounters(self.lanes)

    positions = property(lambda self: sum(l.positions for l in self.lanes))
    recorded = property(lambda self: sum(l.recorded for l in self.lanes))
    games_finished = property(lambda self: sum(l.games_finished for l in self.lanes))
    n_alive = property(lambda self: sum(l.n_alive for l in self.lanes))
    steps_issued = property(lambda self: sum(l.steps_issued for l in self.lanes))

    def play_to_completion(self, progress=None):
        """Free-running lanes: every lane's batch of steps and its poll are enqueued in turn, so the lanes' graph replays
        alternate on their streams; a lane whose run is over drops out.  Then every lane's run is closed: the first error is
        raised after all lanes have handed over their examples."""
        if not self.free_running:
            return _play_lockstep(self, progress)
        live = list(self.lanes)
        while live:
            live = [l for l in live if not l.tick()]
            if progress:
                progress(self)
        parts, err = [], None
        for l in self.lanes:
            try:
                parts.append(l.finish())
            except YYError as e:
                err = err or e
                parts.append(l.collect())
        if err is not None:
            for l, p in zip(self.lanes, parts):
                l.out.append(p)                            # stay collectable
            raise err
        return sort_examples({k: torch.cat([p[k] for p in parts]) for k in parts[0]})

    def play_move(self):
        """One lockstep move of every lane: all lanes' moves are enqueued on their streams, then finished in turn."""
        live = [l for l in self.lanes if l.n_alive > 0]
        for l in live:
            l.enqueue_move()
        return sum(l.finish_move() for l in live)

    def run(self, num_games, progress=None):
        """Play `num_games` games to completion; returns the examples.  The lanes start every move TOGETHER (play_move): with
        evaluation reuse the rows per evaluator launch rise from a dozen to hundreds inside each search, and two lanes in the
        same phase fill the compute units together in the heavy half, while a lane left to run free (its next move enqueued as
        soon as its last one was read back) drifts out of phase and spends its heavy half alone on the chip -- config 2 played
        to completion, same box: 32.8 s in step against 44.0 s free-running with the reuse on, 128.7 s against 132.2 s without."""
        K = len(self.lanes)
        for k, l in enumerate(self.lanes):
            l.begin_run(shard_games(int(num_games), k, K)[0])
        return self.play_to_completion(progress)

    def memory_bytes(self):
        """The lanes' _Engine.memory_bytes() summed; the one book the lanes share counted once."""
        per = [l.memory_bytes() for l in self.lanes]
        return dict(context=sum(m["context"] for m in per), book=self.book.bytes if self.book is not None else 0,
                    shared_evaluations=sum(m["shared_evaluations"] for m in per))

    def collect(self):
        torch.cuda.synchronize(self.device)
        parts = [l.collect() for l in self.lanes]
        ex = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
        return sort_examples(ex) if self.free_running else ex

    def close(self):
        torch.cuda.synchronize(self.device)
        for l in self.lanes:
            l.close()


# =============================================================================== multi-GPU sharding + gather
def shard_games(total, rank, world):
    """Episode sharding (replaces `games_per_worker` processes, self_play.py:299-304): rank r of `world` plays the
    games with global index r, r + world, r + 2*world, ... < total.  Returns (count, first_index, stride); the
    union over ranks is exactly range(total) for any world size, so per-game ids do not depend on it."""
    count = total // world + (1 if rank < total % world else 0)
    return count, rank, world


def example_capacity(total_games, world, rows_per_game):
    """Upper bound of the examples one rank can produce: its share of the games (shard_games) times the most examples a
    game can hold.  Every rank computes the same number, so the exchange needs no size negotiation."""
    return (total_games // world + (1 if total_games % world else 0)) * rows_per_game


def gather_examples(ex, group=None, capacity=None):
    """The ONE exchange of the path (north_star: a single all-gather of the (state, pi, z) examples at iteration end; the
    reference's return_queue.get loop, self_play.py:311-315).  Every rank packs its examples row-wise into one byte buffer
    [header: row count | rows: state int8 R*C, pi f32 A, z f32, game id i64, ply i64] and ONE all_gather_into_tensor
    (RCCL over xGMI on GPUs; gloo on CPU tensors in the tests) delivers all buffers to every rank, which returns the
    concatenation in rank order.  capacity = rows each rank's buffer holds (`example_capacity`; the same on every rank);
    without it a second, 8-byte all-gather of the counts sizes the buffers first."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return ex
    world = dist.get_world_size(group)
    keys = sorted(ex)
    if dist.get_backend(group) == "gloo" and ex[keys[0]].is_cuda:      # gloo gathers host buffers: stage the examples there
        ex = {k: v.cpu() for k, v in ex.items()}
    dev = ex[keys[0]].device
    n = int(ex[keys[0]].shape[0])
    widths = [int(np.prod(ex[k].shape[1:], dtype=np.int64)) * ex[k].element_size() for k in keys]      # bytes per row and key
    cols = [ex[k].contiguous().reshape(n, -1).view(torch.uint8) for k in keys] if n else []
    rb = sum(widths)
    if capacity is None:
        mine = torch.tensor([n], dtype=torch.int64, device=dev)
        every = torch.empty(world, dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(every, mine, group=group)
        capacity = max(int(every.max()), 1)
    if n > capacity:
        raise ValueError(f"gather_examples: {n} examples exceed the agreed capacity {capacity}")
    HDR = 16
    buf = torch.zeros(HDR + capacity * rb, dtype=torch.uint8, device=dev)
    buf[:HDR].view(torch.int64).copy_(torch.tensor([n, rb], dtype=torch.int64))
    if n:
        buf[HDR:HDR + n * rb].view(n, rb).copy_(torch.cat(cols, dim=1))
    out = torch.empty(world * buf.numel(), dtype=torch.uint8, device=dev)
    dist.all_gather_into_tensor(out, buf, group=group)                      # <- the single data-path collective
    out = out.view(world, -1)
    hdr = out[:, :HDR].contiguous().view(torch.int64).reshape(world, 2).cpu()
    assert bool((hdr[:, 1] == rb).all()), "ranks disagree on the example row layout"
    rows = torch.cat([out[r, HDR:HDR + int(hdr[r, 0]) * rb].view(-1, rb) for r in range(world)])
    res, off = {}, 0
    for k, w in zip(keys, widths):
        col = rows[:, off:off + w].contiguous()
        res[k] = col.view(ex[k].dtype).reshape((rows.shape[0],) + tuple(ex[k].shape[1:]))
        off += w
    return res


def publish_examples_file(ex, output_dir, reference_format=False):
    """Rank 0 writes self_play_data_<unix_ts>.npz (self_play.py:374-384) to a temporary name and renames it into place, every
    rank waits at a barrier until the file is complete, and all ranks return the SAME path (rank 0's, broadcast): a rank that
    went on to load_data() could otherwise miss the file or open a half-written zip, and a per-rank time stamp could name
    different files."""
    import torch.distributed as dist
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    rank = dist.get_rank() if multi else 0
    os.makedirs(output_dir, exist_ok=True)
    filename = os.path.join(output_dir, f"self_play_data_{int(time.time())}.npz")
    n = 1
    while os.path.exists(filename):                    # two publications within one second: never overwrite
        filename = os.path.join(output_dir, f"self_play_data_{int(time.time())}_{n}.npz")
        n += 1
    if multi:
        names = [filename]
        dist.broadcast_object_list(names, src=0)
        filename = names[0]
    if rank == 0:
        # temporary name that the loaders' glob (self_play_data_*.npz) cannot match: a crash before the rename leaves no
        # half-written file that would be picked up as training data
        tmp = f"{filename}.{os.getpid()}.partial"
        states = ex["states"].cpu().numpy()
        with open(tmp, "wb") as fh:
            if reference_format:
                # `boards` = pickled board objects of the reference's own class, readable by ITS TrainingDataQueue.push_file
                from .training import save_examples_reference_format
                save_examples_reference_format(fh, states, ex["policies"].cpu().numpy(), ex["values"].cpu().numpy())
            else:
                np.savez(fh, boards=states, states=states, policies=ex["policies"].cpu().numpy().astype(np.float64),
                         values=ex["values"].cpu().numpy().astype(np.float64), game_id=ex["game_id"].cpu().numpy(),
                         ply=ex["ply"].cpu().numpy())
        os.replace(tmp, filename)
    if multi:
        dist.barrier()
    return filename


# =============================================================================== reference API
class SelfPlayWorker:
    """self_play.py:22-216 with the same constructor; plays games one at a time through MCTS (G == 1)
    drawing from the global numpy stream exactly where the reference does, so identical seeds give
    identical transcripts.  Defaults reproduce the literal reference (aliased boards, quirks)."""

    def __init__(self, game, model_path, num_simulations=800, num_games=1, temperature_threshold=10,
                 dirichlet_alpha=0.3, dirichlet_epsilon=0.25, cpuct=1.0, num_parallel=1,
                 board_semantics="aliased", reference_quirks=True, neural_net=None, device=None, leaves_per_step=1,
                 fast_simulations=None, full_search_probability=1.0, tree_reuse=False, free_running=False,
                 evaluation_symmetry="off", symmetry_seed=None, forced_playouts=None, fpu_reduction=None, fpu_reduction_root=None,
                 shared_evaluations=None, shared_evaluations_replace=False, solver=False, gumbel_root=None, gumbel_c_visit=None, gumbel_c_scale=None, gumbel_interior=False):
        """gumbel_root / gumbel_c_visit / gumbel_c_scale / gumbel_interior: MCTS's (needs board_semantics="copied" and reference_quirks=False, which
        are not this class's defaults); every search draws its Gumbel rows in MCTS and the move played is the Gumbel winner at
        every ply (MCTS.gumbel_action), so numpy's stream is not asked for the move.
        solver: MCTS's (needs board_semantics="copied" and reference_quirks=False, which are not this class's defaults).
        shared_evaluations: MCTS's (a table shared by the one game's searches; needs board_semantics="copied",
        reference_quirks=False and a network whose evaluator is row-independent).  shared_evaluations_replace: MCTS's too.
        leaves_per_step, fast_simulations / full_search_probability, tree_reuse, evaluation_symmetry / symmetry_seed (None: 0; this
        class has no seed of its own), forced_playouts, fpu_reduction / fpu_reduction_root (needs reference_quirks=False):
        options.SearchOptions, through MCTS; K > 1, tree_reuse, evaluation_symmetry
        and forced_playouts need board_semantics="copied", K > 1, evaluation_symmetry and forced_playouts also
        reference_quirks=False, which are not this class's defaults.
        free_running: refused (ValueError).  This class plays ONE game at a time through MCTS, drawing from numpy's global
        stream: there is no batch whose games could be freed from each other; the mode is SelfPlayEngine's."""
        if free_running:
            raise ValueError("free_running=True: SelfPlayWorker plays one game at a time through MCTS (numpy's global stream): "
                             "there is no batch to free -- use SelfPlayEngine / SelfPlayManager")
        opts = options.resolve(num_simulations, leaves_per_step, board_semantics, reference_quirks, fast_simulations=fast_simulations,
                               full_search_probability=full_search_probability, tree_reuse=tree_reuse,
                               evaluation_symmetry=evaluation_symmetry, symmetry_seed=symmetry_seed,
                               forced_playouts=forced_playouts, fpu_reduction=fpu_reduction,
                               fpu_reduction_root=fpu_reduction_root, shared_evaluations=shared_evaluations,
                               shared_evaluations_replace=shared_evaluations_replace, solver=solver, gumbel_root=gumbel_root, gumbel_c_visit=gumbel_c_visit, gumbel_c_scale=gumbel_c_scale, gumbel_interior=gumbel_interior)
        self.gumbel_root = opts.gumbel_root
        self.tree_reuse, self.leaves_per_step, self.playout_cap = opts.tree_reuse, opts.leaves_per_step, opts.playout_cap
        self.game, self.model_path = game, model_path
        self.num_simulations, self.num_games = num_simulations, num_games
        self.temperature_threshold = temperature_threshold
        self.dirichlet_alpha, self.dirichlet_epsilon, self.cpuct = dirichlet_alpha, dirichlet_epsilon, cpuct
        self.num_parallel = num_parallel
        self.board_semantics, self.reference_quirks = board_semantics, reference_quirks
        if neural_net is None:
            neural_net = YinYangNeuralNetwork(game)
            if os.path.exists(model_path):
                neural_net.load_model(model_path)
            dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            neural_net = neural_net.to(dev).eval()    # the reference keeps self-play inference on the CPU (:54-59)
        self.neural_net = neural_net
        self.mcts = MCTS(game, neural_net, num_simulations=num_simulations, cpuct=cpuct,
                         dirichlet_alpha=dirichlet_alpha, dirichlet_epsilon=dirichlet_epsilon,
                         num_threads=num_parallel, board_semantics=board_semantics, device=device,
                         **{k: v for k, v in opts.keywords().items() if k not in opts.playout_cap})   # the cap is drawn in play_game

    def play_game(self):
        game, examples = self.game, []
        board = game.getInitBoard()
        player, step, passes = 1, 0, 0
        copied = self.board_semantics == "copied"

        def label(result):
            out, value = [], result
            for i, (b, pi, pl) in enumerate(examples):
                if self.reference_quirks:
                    out.append((b, pi, value if i % 2 == 0 else -value))      # :116-118 (nets out to +result)
                    value = -value
                else:
                    out.append((b, pi, result if pl == player else -result))
            return out

        while True:
            temperature = 1.0 if step < self.temperature_threshold else 0
            root_player = 1 if self.reference_quirks else player               # Q4
            valid_moves = game.getValidMoves(board, root_player)
            valid_idx = np.where(valid_moves == 1)[0]
            if len(valid_idx) == 0:
                passes += 1
                if passes >= 2:
                    result = game.getGameEnded(board, player)
                    if result == 0:
                        result = DRAW
                    return label(result)
                player = -player
                continue
            passes = 0
            if self.playout_cap:
                full = np.random.random() < self.playout_cap["full_search_probability"]
                pi, root = self.mcts.search(board, root_player, add_exploration_noise=(step == 0),
                                            num_simulations=None if full else self.playout_cap["fast_simulations"])
                if full:
                    examples.append((board, pi, player))
            else:
                pi, root = self.mcts.search(board, root_player, add_exploration_noise=(step == 0))
                examples.append((board, pi, player))
            if self.gumbel_root:
                action = self.mcts.gumbel_action()
            elif temperature == 0:
                action = np.random.choice(np.where(pi == np.max(pi))[0])
            else:
                probs = pi * valid_moves
                if np.sum(probs) > 0:
                    probs = probs / np.sum(probs)
                else:
                    probs = np.zeros_like(valid_moves)
                    probs[valid_idx] = 1.0 / len(valid_idx)
                action = np.random.choice(len(probs), p=probs)
            if copied:                                                         # examples keep the pre-move board
                nb = YinYangLogic(board.n, board.m, getattr(board, "rowcol_rule", False))
                nb.board = board.board.copy()
                board = nb
            board, player = game.getNextState(board, player, action)
            if self.tree_reuse:
                self.mcts.reuse_tree(root, board, player, int(action))                 # self_play.py:192
            step += 1
            result = game.getGameEnded(board, player)
            if result != 0:
                return label(result)

    def generate_games(self):
        all_examples = []
        for _ in range(self.num_games):
            all_examples.extend(self.play_game())
        return all_examples


class SelfPlayManager:
    """self_play.py:218-335.  The reference forks `num_workers` CPU processes and pickles lists back
    through a queue; here `num_workers * games_per_worker` episodes are sharded over the ranks of the
    running job (one process per GPU, `torchrun`), each rank plays its shard on the batched engine,
    and one all-gather collects the examples."""

    def __init__(self, game, model_path, num_workers=1, num_simulations=800, games_per_worker=1,
                 temperature_threshold=10, dirichlet_alpha=0.3, dirichlet_epsilon=0.25, cpuct=1.0,
                 mcts_parallel=1, concurrent_games=4096, board_semantics="copied", reference_quirks=False,
                 nn_mode="auto", seed=0, num_channels=128, num_res_blocks=10, evaluation_reuse=None,
                 opening_book_stones=None, lanes=None, leaves_per_step=1, fast_simulations=None, full_search_probability=1.0,
                 tree_reuse=False, free_running=False, evaluation_symmetry="off", symmetry_seed=None, forced_playouts=None,
                 fpu_reduction=None, fpu_reduction_root=None, shared_evaluations=None, shared_evaluations_replace=False,
                 solver=False, gumbel_root=None, gumbel_c_visit=None, gumbel_c_scale=None, gumbel_interior=False):
        """gumbel_root / gumbel_c_visit / gumbel_c_scale / gumbel_interior: the Gumbel root search (options.SearchOptions),
        solver (its three counters go into `stats` as solver_*, in lockstep runs: a free-running context stays armed, and
        the counters are read after a finished search),
        leaves_per_step, fast_simulations / full_search_probability, tree_reuse, free_running, evaluation_symmetry / symmetry_seed
        (None: the engine's seed, 1000 + seed, on every rank), forced_playouts, fpu_reduction / fpu_reduction_root,
        shared_evaluations (a table per lane; its counters, fill and memory go into `stats`), shared_evaluations_replace (the
        replacing table; `stats` then holds its six counters): options.SearchOptions.
        evaluation_reuse: None = the engine's default (on for copied boards with the float32-accurate evaluator: pass values +
        per-game evaluation cache, SelfPlayEngine; off at leaves_per_step > 1, where opening_book_stones=None also means no
        book); False = the network is asked for every leaf like the reference."""
        self.options = options.resolve(num_simulations, leaves_per_step, board_semantics, reference_quirks, "philox",
                                       (evaluation_reuse,), opening_book_stones, fast_simulations, full_search_probability,
                                       tree_reuse, free_running, evaluation_symmetry, symmetry_seed, forced_playouts,
                                       fpu_reduction, fpu_reduction_root, shared_evaluations, shared_evaluations_replace, solver, gumbel_root=gumbel_root, gumbel_c_visit=gumbel_c_visit, gumbel_c_scale=gumbel_c_scale, gumbel_interior=gumbel_interior)
        self.evaluation_reuse = evaluation_reuse
        self.lanes = lanes                 # HIP streams the rank's games are cut over (SelfPlayLanes); None = 2 from 512 slots on
        # None = 8 stones when it pays: evaluation reuse on, a board of at most 64 cells (770 k positions at 8x8: ~1.5 s to build)
        # and at least 1024 games for this rank; 0 = no book
        self.opening_book_stones = opening_book_stones
        self.game, self.model_path = game, model_path
        self.num_workers, self.games_per_worker = num_workers, games_per_worker
        self.num_simulations, self.temperature_threshold = num_simulations, temperature_threshold
        self.dirichlet_alpha, self.dirichlet_epsilon, self.cpuct = dirichlet_alpha, dirichlet_epsilon, cpuct
        self.mcts_parallel = mcts_parallel
        self.concurrent_games, self.board_semantics, self.reference_quirks = concurrent_games, board_semantics, reference_quirks
        self.nn_mode, self.seed = nn_mode, seed
        self.num_channels, self.num_res_blocks = num_channels, num_res_blocks
        self.stats = {}

    def generate_games_parallel(self):
        import torch.distributed as dist
        rank, world = (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else (0, 1)
        total = self.num_workers * self.games_per_worker
        mine, first, stride = shard_games(total, rank, world)
        dev = torch.device("cuda", torch.cuda.current_device())
        net = YinYangNeuralNetwork(self.game, self.num_channels, self.num_res_blocks)
        if os.path.exists(self.model_path):
            net.load_model(self.model_path)       # every rank reads the same file: no broadcast needed
        net = net.to(dev).eval()
        evaluator = BatchedEvaluator(net, self.nn_mode)
        book = self.opening_book_stones
        if book is None:
            auto = (self.options.leaves_per_step == 1 and self.evaluation_reuse is not False and self.board_semantics == "copied" and mine >= 1024
                    and self.game.getActionSize() <= 64 and getattr(evaluator, "row_independent", False))
            book = 8 if auto else 0
        slots = max(1, min(self.concurrent_games, mine))
        eng = SelfPlayLanes(self.game, evaluator, num_simulations=self.num_simulations, opening_book=int(book),
                            lanes=self.lanes if self.lanes else (2 if slots >= 512 else 1),
                             concurrent_games=slots, cpuct=self.cpuct,
                             dirichlet_alpha=self.dirichlet_alpha, dirichlet_epsilon=self.dirichlet_epsilon,
                             temperature_threshold=self.temperature_threshold, board_semantics=self.board_semantics,
                             reference_quirks=self.reference_quirks, seed=1000 + self.seed,   # key of the per-game streams: the same on every rank
                             first_game_index=first, game_index_stride=stride, device=dev,
                             reuse_pass_value=self.evaluation_reuse, reuse_transpositions=self.evaluation_reuse,
                             keep_evaluations=self.evaluation_reuse, **self.options.keywords())
        t0 = time.perf_counter()
        ex = eng.run(mine) if mine > 0 else eng.collect()
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        counters = eng.ctx.status()
        if self.options.shared_evaluations:
            shc = eng.ctx.shared_counters_ex() if self.options.shared_evaluations_replace else eng.ctx.shared_counters()
            counters.update({f"shared_{k}": v for k, v in shc.items()},
                            shared_fill=sum(l.shared.fill() for l in eng.lanes), shared_slots=sum(l.shared.slots for l in eng.lanes),
                            memory_bytes=eng.memory_bytes())
        if self.options.solver and not self.options.free_running:
            counters.update({f"solver_{k}": v for k, v in eng.ctx.solver_counters().items()})
        ex = gather_examples(ex, capacity=example_capacity(total, world, eng.T))
        self.stats = dict(seconds=t1 - t0, positions=eng.positions, games=eng.games_finished, **counters,
                          **(dict(steps_issued=eng.steps_issued) if self.options.free_running else {}))
        eng.close()
        return ex


def generate_self_play_data(game, model_path, output_dir, num_games=100, num_workers=1, num_simulations=800,
                            reference_format=False, leaves_per_step=1, fast_simulations=None, full_search_probability=1.0,
                            **engine_kwargs):
    """self_play.py:337-387: same arguments and the same file name pattern.  The .npz holds plain
    tensors (`states` int8 [N,R,C], `policies` float64 [N,A], `values` float64 [N]; `boards` is an
    alias of `states`) instead of pickled board objects; `reference_format=True` writes the reference's pickled-object
    layout as well (training.save_examples_reference_format) so that the reference's training pipeline can read the file.
    leaves_per_step, fast_simulations, full_search_probability: SelfPlayManager's, checked here before anything is written;
    the other keywords (tree_reuse, free_running, forced_playouts, fpu_reduction / fpu_reduction_root, shared_evaluations,
    shared_evaluations_replace, solver and gumbel_root / gumbel_c_visit / gumbel_c_scale / gumbel_interior among them) are SelfPlayManager's too."""
    opts = options.resolve(num_simulations, leaves_per_step, fast_simulations=fast_simulations,
                           full_search_probability=full_search_probability)
    os.makedirs(output_dir, exist_ok=True)
    games_per_worker = max(1, num_games // num_workers)               # :355 (remainder dropped)
    manager = SelfPlayManager(game, model_path, num_workers=num_workers, games_per_worker=games_per_worker,
                              num_simulations=num_simulations, **opts.keywords(), **engine_kwargs)
    ex = manager.generate_games_parallel()
    filename = publish_examples_file(ex, output_dir, reference_format)
    generate_self_play_data.last_stats = manager.stats
    return filename
