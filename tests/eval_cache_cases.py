"""The configurations on which the evaluation cache is held against tests/eval_cache_model.py, and what the host test
(tests/test_eval_cache_model_host.py: CPU oracle) and the device test (tests/test_gpu_eval_cache_trace.py) share: the start
positions, the schedule of searches, restarts and clears, and the rule that picks the move between two searches.  Everything
here is computed on the host with the CPU oracle's rules, so both tests walk the same positions."""
import functools

import numpy as np

import oracle_lib as O
from eval_cache_model import BOOK, HIT, HIT_CLASSES, MISS, STORE_CLASSES, cache_slots, pack_keys, replay

PBITS, VBITS = 6, 4          # the hash evaluator of every run: hash_eval_torch(planes, 6, 4) / the oracle's yyo_hash_eval

# flags: the cached context; base: the context whose flagged rows are exactly the cached context's lookups (option-off, or
# reuse_pass_value alone for a cached context with it: a K_REUSE revisit consults nothing).  searches: consecutive searches of
# one context, a move played in between.  restart: the searches in front of which every third game is put back on the empty
# board; clear_before: the searches in front of which the cache is cleared.  small: the cache overflows (every store class is
# required); book_stones: an opening book of that many stones is set on the cached context.  jump: {search: plies}, the searches
# in front of which every game is put on a fresh position of that many plies (never the empty board: the epoch stays).
TT = dict(reuse_transpositions=True)
CONFIGS = {
    "8x8-tt": dict(shape=(8, 8), G=48, sims=100, max_ply=60, seed=11, flags=TT, base={}, searches=2),
    "8x8-pass+tt": dict(shape=(8, 8), G=48, sims=100, max_ply=60, seed=11, flags=dict(reuse_pass_value=True, **TT),
                        base=dict(reuse_pass_value=True), searches=2),
    "9x12-tt": dict(shape=(9, 12), G=32, sims=60, min_ply=51, max_ply=86, seed=12, flags=TT, base={}, searches=2,
                    nodes_per_game=64),
    "12x12-tt": dict(shape=(12, 12), G=32, sims=60, min_ply=69, max_ply=115, seed=13, flags=TT, base={}, searches=2,
                     nodes_per_game=64),
    "12x16-tt": dict(shape=(12, 16), G=32, sims=60, min_ply=92, max_ply=153, seed=14, flags=TT, base={}, searches=2,
                     nodes_per_game=64),
    # 128 slots a game.  Searches 0 .. 10 advance move by move (every third game restarts twice, one clear); the most visited
    # child leads into the part of the tree the cache already holds, so these searches alone never fill a window.  Searches
    # 11 .. 15 therefore jump to unrelated positions of FEWER stones each time -- nothing stored becomes "cannot recur", the
    # table fills with live entries -- and searches 16 .. 19 advance again, with hits and live replacements side by side
    "8x8-keep": dict(shape=(8, 8), G=48, sims=30, max_ply=40, seed=4, searches=20, nodes_per_game=32, small=True,
                     flags=dict(reuse_pass_value=True, keep_evaluations=True, **TT), base=dict(reuse_pass_value=True),
                     restart=(3, 6), clear_before=(9,), jump={11: 36, 12: 30, 13: 24, 14: 18, 15: 10}),
    # the same pressure on three bitboard words: here the slot of an entry, and so the hash of the third word, decides hits
    "12x12-keep": dict(shape=(12, 12), G=32, sims=30, min_ply=60, max_ply=110, seed=16, searches=12, nodes_per_game=32,
                       flags=dict(reuse_pass_value=True, keep_evaluations=True, **TT), base=dict(reuse_pass_value=True),
                       jump={4: 100, 5: 90, 6: 80, 7: 70}),
    "6x6-book": dict(shape=(6, 6), G=32, sims=60, max_ply=6, seed=15, flags=dict(keep_evaluations=True, **TT), base={},
                     searches=2, book_stones=3),
    "8x8-aliased-tt": dict(shape=(8, 8), G=32, sims=60, max_ply=56, seed=2, flags=TT, base={}, searches=2, aliased=True),
}
MIN_EVENTS = 20              # how often a configuration must exercise each rule it is there for


def late_positions(G, R, C, max_ply, seed, min_ply=0):
    """Game g after min_ply .. max_ply plies (spread evenly over the games) of random legal play from the empty board; a side
    without a move passes.  -> (boards int8 [G, R, C], players int8 [G])"""
    rng = np.random.default_rng(seed)
    boards, players = np.zeros((G, R, C), np.int8), np.ones(G, np.int8)
    target = min_ply + (np.arange(G) * (max_ply - min_ply)) // G
    for ply in range(max_ply):
        mask = O.valid_mask(boards, players)
        for g in np.flatnonzero(ply < target):
            legal = np.flatnonzero(mask[g])
            if len(legal):
                boards[g].reshape(-1)[rng.choice(legal)] = players[g]
            players[g] = -players[g]
    return boards, players


def pick_moves(counts):
    """The most visited root child, the lowest action on ties; -1 (a pass) where the root has no visited child."""
    counts = np.asarray(counts)
    return np.where(counts.sum(1) > 0, counts.argmax(1), -1)


def play(boards, players, actions):
    boards, players = boards.copy(), players.copy()
    for g, a in enumerate(actions):
        if a >= 0:
            assert boards[g].reshape(-1)[a] == 0
            boards[g].reshape(-1)[a] = players[g]
        players[g] = -players[g]
    return boards, players


def restart_games(G):
    return np.arange(G) % 3 == 0


def run_config(cfg, search):
    """The schedule of one configuration.  search(s, boards, players) -> root visit counts int [G, A] of search s."""
    R, C = cfg["shape"]
    boards, players = late_positions(cfg["G"], R, C, cfg["max_ply"], cfg["seed"], cfg.get("min_ply", 0))
    for s in range(cfg["searches"]):
        if s in cfg.get("restart", ()):
            again = restart_games(cfg["G"])
            boards[again], players[again] = 0, 1
        if s in cfg.get("jump", {}):
            ply = cfg["jump"][s]
            boards, players = late_positions(cfg["G"], R, C, ply, cfg["seed"] + 100 + s, ply)
        counts = search(s, boards.copy(), players.copy())
        boards, players = play(boards, players, pick_moves(counts))


def lookups_of(leaf_boards):
    """int8 [n, R, C] leaf positions -> (keys uint64 [n, 2 * NW], stones [n])"""
    b = np.asarray(leaf_boards, np.int8)
    return pack_keys(b), np.count_nonzero(b, axis=(1, 2))


@functools.lru_cache(maxsize=None)
def oracle_searches(name):
    """The configuration searched by the CPU oracle: per game the list of (root stones, keys, stones) of its searches.  The
    oracle's leaf log holds the evaluator calls of the simulations in order (the root call of mcts.py:295 is not logged), which
    are the leaves a context with reuse_transpositions and without reuse_pass_value consults the cache with."""
    cfg = CONFIGS[name]
    games = [[] for _ in range(cfg["G"])]

    def search(s, boards, players):
        counts = []
        for g in range(cfg["G"]):
            r = O.search_hash(boards[g], int(players[g]), cfg["sims"], 0 if cfg.get("aliased") else 1, PBITS, VBITS,
                              leaf_cap=cfg["sims"])
            assert len(r.leaves) == r.n_evals <= cfg["sims"]
            games[g].append((int(np.count_nonzero(boards[g])), *lookups_of(r.leaves)))
            counts.append(r.counts)
        return np.stack(counts)

    run_config(cfg, search)
    return games


def slots_of(cfg):
    R, C = cfg["shape"]
    return cache_slots(cfg.get("nodes_per_game") or cfg["sims"] + 2, cfg["G"], R * C)


@functools.lru_cache(maxsize=None)
def book_positions(R, C, stones):
    """The positions an OpeningBook of `stones` stones holds: what alternating legal play, black first, reaches from the empty
    board with 1 .. stones stones.  -> a frozenset of key tuples"""
    b, player, keys = np.zeros((1, R, C), np.int8), 1, set()
    for _ in range(stones):
        m = O.valid_mask(b, np.full(len(b), player, np.int8))
        bi, a = np.nonzero(m)
        c = b[bi].reshape(len(bi), -1).copy()
        c[np.arange(len(bi)), a] = player
        b = np.unique(c, axis=0).reshape(-1, R, C)
        keys.update(map(tuple, pack_keys(b).tolist()))
        player = -player
    return frozenset(keys)


def model_replay(name, searches, mutant=None, book=None):
    """One game's searches through the model, with the configuration's cache size, flags, book and clears."""
    cfg = CONFIGS[name]
    if cfg.get("book_stones") and book is None:
        book = book_positions(*cfg["shape"], cfg["book_stones"])
    return replay(searches, slots_of(cfg), bool(cfg["flags"].get("keep_evaluations")), mutant, book,
                  cfg.get("book_stones", 0), cfg.get("clear_before", ()))


def sum_counts(dicts):
    out = {}
    for d in dicts:
        for k, v in d.items():
            out[k] = out.get(k, 0) + int(v)
    return out


def coverage_shortfalls(name, c):
    """The rules a configuration is there for, each exercised at least MIN_EVENTS times (window wraps: once) -> the list of
    conditions the classification counts `c` miss."""
    cfg = CONFIGS[name]
    need = {"hit_current": MIN_EVENTS, "wraps": 1}
    if cfg.get("small"):
        need.update(dict.fromkeys(STORE_CLASSES, MIN_EVENTS))
    if cfg["flags"].get("keep_evaluations") and cfg.get("restart"):
        need["hit_older"] = MIN_EVENTS
    if cfg.get("book_stones"):
        need["book"] = MIN_EVENTS
    return ["%s: %s %d < %d" % (name, k, c.get(k, 0), n) for k, n in need.items() if c.get(k, 0) < n]


# ---- the device side: what an evaluator callable records (torch is imported by the GPU tests only)
class Recorder:
    """The hash evaluator as a callable that records m.needs_eval at every call, and with `positions` the black and white stones
    of every row as planes 1 and 2 hold them."""

    def __init__(self, m, positions):
        self.m, self.positions, self.ne, self.bits = m, positions, [], []

    def __call__(self, planes):
        import torch
        from hash_eval import hash_eval_torch
        self.ne.append(self.m.needs_eval.clone())
        if self.positions:
            self.bits.append((planes[:, 1] - planes[:, 2]).to(torch.int8))
        return hash_eval_torch(planes, PBITS, VBITS)

    def take(self):
        """-> (needs_eval uint8 [calls, G], boards int8 [calls, G, R, C] or None) of the calls since the last take, the root
        call (call 0: every root is evaluated, nothing is looked up) dropped."""
        import torch
        ne = torch.stack(self.ne).cpu().numpy()[1:]
        b = torch.stack(self.bits).cpu().numpy()[1:] if self.positions else None
        self.ne, self.bits = [], []
        return ne, b


def game_lookups(ne, boards, g):
    """Game g's lookups of one base search -> (the calls that looked something up, keys, stones)"""
    calls = np.flatnonzero(ne[:, g])
    return calls, *lookups_of(boards[calls, g])


def expected_needs_eval(n_calls, calls, outcome):
    """The cached context's needs_eval column of one game and search: 1 where the model predicts a miss."""
    want = np.zeros(n_calls, np.uint8)
    want[calls] = outcome == MISS
    return want
