"""Plain-numpy restatement of the first-play urgency reduction (include/yy_engine.h YY_FLAG_FPU_REDUCTION).

TEST INFRASTRUCTURE.  One game: the search of tests/tree_model.py with r / r_root, which asks select() below wherever r > 0,
and the exact hash evaluator of hash_eval.py (its priors times PSCALE, as in forced_playouts_model: sqrt(SP) is then not
negligible next to the values).

  search(root_or_board, player, budget, r, r_root, K, forced, aliased)
        the search of leaf_parallel_model (K descents per step with virtual visits; K = 1: the reference's search) from a
        board or from a kept Tree (tree_reuse_model), with forced playouts at the root (K = 1) and, with aliased=True, on
        ONE board that every expansion plays its move on (K = 1, fresh roots; the reference's literal semantics, checked
        against the C oracle at r = 0).  r == 0: the option is off and every selection is leaf_parallel_model._select.
        r > 0: select() below; the root is scored with r_root (None: r), every other node with r.
  fixed_sums(children)  SN, SW, SP over the (n, w, P) of the children with n > 0, as integers: SW in units of 2^-32 and SP in
                        units of 2^-40, every term truncated toward zero -- so the order of the children does not matter.
  fpu_q(r, SN, SW, SP)  f32(f32(SW / SN) - f32(r * f32(sqrt(SP)))) in np.float32 steps; 0 when SN == 0.

`mutant=` (MUTANTS) breaks one rule on purpose; tests/test_fpu_model.py asserts that the fixtures of the GPU tests (CASES
below, tests/test_gpu_fpu.py) tell each from the true model."""
import functools
import math

import numpy as np

import oracle_lib as O
import tree_model
from forced_playouts_model import PSCALE
from tree_model import advance, dirichlet_noise, random_root  # noqa: F401  (re-exported for the callers of this model)

f32 = np.float32

MUTANTS = {
    "sp_all": "SP sums the priors of all children, not only of the visited ones",
    "prior_raw": "at a noised root SP reads the priors from before the noise",
    "r_everywhere": "the root is scored with r where r_root belongs",
    "no_parent": "the SW / SN term is dropped: q_fpu = -f32(r * f32(sqrt(SP)))",
    "reduce_visited": "the reduction is also taken off the q of the visited children",
    "sn0": "SN == 0 is not special-cased: 0 / 0 is NaN, no child of a fresh node is selectable and the game stops searching",
}


def fixed_sums(children):
    """children: iterable of (n, w, P) -> (SN, SW, SP), python integers"""
    SN = SW = SP = 0
    for n, w, P in children:
        if n > 0:
            SN += int(n)
            SW += int(float(w) * 4294967296.0)                     # exact product, truncated toward zero
            SP += int(float(P) * 1099511627776.0)
    return SN, SW, SP


def fpu_q(r, SN, SW, SP, mutant=None):
    if SN == 0 and mutant != "sn0":
        return f32(0.0)
    sp = f32(float(SP) * 2.0 ** -40)
    red = f32(f32(r) * np.sqrt(sp))
    if mutant == "no_parent":
        return f32(f32(0.0) - red)
    sw = f32(float(SW) * 2.0 ** -32)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = f32(sw / f32(SN))
    return f32(mean - red)


def select(node, vc, cpuct, r, mutant=None, raw=None):
    """leaf_parallel_model._select with the first-play urgency of `node` for its unvisited children.  r: the node's reduction
    (0 at a root with r_root = 0: the visited children's mean itself).  raw: {id(edge): prior before the noise} of a noised
    root (the prior_raw mutant).  -> the edge, or None when no child is selectable (NaN scores)."""
    stat = []
    for e in node.edges:
        v = vc.get(id(e), 0)
        stat.append((e.N + v, f32(e.W - f32(v)) if v > 0 else e.W))
    S = sum(n for n, _ in stat)
    sq = f32(math.sqrt(S))

    def prior(e):
        return raw[id(e)] if (mutant == "prior_raw" and raw and id(e) in raw) else e.P

    SN, SW, SP = fixed_sums((n, w, prior(e)) for (n, w), e in zip(stat, node.edges))
    if mutant == "sp_all":
        SP = sum(int(float(e.P) * 1099511627776.0) for e in node.edges)
    q0 = fpu_q(r, SN, SW, SP, mutant)
    red = f32(f32(r) * np.sqrt(f32(float(SP) * 2.0 ** -40)))
    best, best_ucb = None, -math.inf
    for (n, w), e in zip(stat, node.edges):
        u = f32(f32(f32(cpuct * e.P) * sq) / f32(1 + n))
        q = f32(w / f32(n)) if n > 0 else q0
        if n > 0 and mutant == "reduce_visited":
            q = f32(q - red)
        ucb = f32(q + u)
        if ucb > best_ucb:                                          # strict >: the lowest action wins ties; NaN never wins
            best, best_ucb = e, ucb
    return best


def search(root_or_board, player, budget, r=0.0, r_root=None, K=1, pbits=10, vbits=11, mutant=None, pscale=PSCALE, **options):
    """tree_model.search with the reduction r (the root: r_root; None: r) -> Result; forced, aliased: its keywords."""
    assert mutant is None or mutant in MUTANTS
    return tree_model.search(root_or_board, player, budget, K, pbits, vbits, r=r, r_root=r_root, pscale=pscale,
                             mutant=mutant and "fpu." + mutant, **options)


# ------------------------------------------------------------------------------------------------ the fixtures of the GPU tests
# GAMES games per case; game g starts g % 5 random plies into a game (1x6 and 7x1: g plies, so that roots without a move,
# finished games and childless nodes below a root turn up), root noise as numpy Dirichlet(0.3) draws over the root's moves.  A case is searched over `moves` moves:
# after each, every game whose tree advance() keeps under the most visited move -- and whose game goes on -- searches on.
GAMES = 8
R, R_ROOT0 = 0.25, 0.0
#         name                 rows cols sims  keywords of search()                                 eps   moves
CASES = {
    "4x4":            (4, 4, 32, dict(r=R), 0.0, 1),
    "5x7":            (5, 7, 48, dict(r=R), 0.0, 1),
    "1x6":            (1, 6, 16, dict(r=R), 0.0, 1),
    "7x1":            (7, 1, 16, dict(r=R), 0.0, 1),
    "9x12":           (9, 12, 16, dict(r=R), 0.0, 1),
    "12x12":          (12, 12, 16, dict(r=R), 0.0, 1),
    "4x4-noise":      (4, 4, 32, dict(r=R), 0.25, 1),
    "5x7-noise":      (5, 7, 48, dict(r=R), 0.25, 1),
    "4x4-root0":      (4, 4, 32, dict(r=R, r_root=R_ROOT0), 0.25, 1),
    "5x7-root0":      (5, 7, 48, dict(r=R, r_root=R_ROOT0), 0.25, 1),
    "12x12-root0":    (12, 12, 16, dict(r=R, r_root=R_ROOT0), 0.25, 1),
    "4x4-K4":         (4, 4, 32, dict(r=R, K=4), 0.0, 1),
    "5x7-K4":         (5, 7, 48, dict(r=R, K=4), 0.25, 1),
    "12x12-K4":       (12, 12, 16, dict(r=R, K=4), 0.0, 1),
    "4x4-reuse":      (4, 4, 32, dict(r=R), 0.25, 3),
    "5x7-reuse":      (5, 7, 48, dict(r=R, r_root=R_ROOT0), 0.25, 3),
    "4x4-forced":     (4, 4, 32, dict(r=R, forced=2.0), 0.25, 1),
    "5x7-forced":     (5, 7, 48, dict(r=R, forced=2.0), 0.0, 1),
    "4x4-aliased":    (4, 4, 32, dict(r=R, aliased=True), 0.0, 1),
    "5x7-aliased":    (5, 7, 48, dict(r=R, aliased=True), 0.25, 1),
    "9x12-aliased":   (9, 12, 16, dict(r=R, aliased=True), 0.0, 1),
}


class Move:
    """One move of a case: what the device test feeds in (boards, players, active, noise; actions: the move every game's tree
    was advanced by BEFORE this search, -1 at the first) and the model's Result per game (None: the game sat out)."""


@functools.lru_cache(maxsize=None)
def fixture(name, mutant=None, off=False):
    """-> list of Move, one per move of case `name`.  off: the same case searched with r = 0 (the option off)."""
    rows, cols, sims, kw, eps, moves = CASES[name]
    kw = dict(kw, r=0.0, r_root=None) if off else kw
    seed = sorted(CASES).index(name)
    roots = [random_root(rows, cols, g if min(rows, cols) == 1 else g % 5, [seed, g]) for g in range(GAMES)]
    boards = [b for b, _ in roots]
    players = [p for _, p in roots]
    trees = [None] * GAMES
    alive = [True] * GAMES
    actions = np.full(GAMES, -1, np.int32)
    out = []
    for t in range(moves):
        m = Move()
        m.boards, m.players = np.stack(boards), np.array(players, np.int8)
        m.active, m.actions = np.array(alive, np.uint8), actions.copy()
        m.noise = np.zeros((GAMES, rows * cols))
        m.results = [None] * GAMES
        actions = np.full(GAMES, -1, np.int32)
        for g in range(GAMES):
            if not alive[g]:
                continue
            if eps:
                m.noise[g] = dirichlet_noise(boards[g], players[g], [seed, g, t])
            res = search(trees[g] if trees[g] is not None else boards[g], players[g], sims, noise=m.noise[g] if eps else None,
                         eps=eps, mutant=mutant, **kw)
            m.results[g] = res
            a = int(np.argmax(res.counts))
            alive[g] = False
            if t + 1 < moves and res.counts[a] > 0 and not res.failed:
                tree, kept = advance(res.tree, a)
                b = boards[g].copy()
                b.flat[a] = players[g]
                if tree is not None and kept < sims and float(O.game_ended(b[None], [-players[g]])[0]) == 0.0:
                    trees[g], boards[g], players[g], actions[g], alive[g] = tree, b, -players[g], a, True
        out.append(m)
    return out


def observables(moves):
    """What a device run is compared on, as one nested tuple (for telling a mutant from the true model)."""
    return tuple((r.counts.tobytes(), r.child_w.tobytes(), r.child_p.tobytes(), r.root_visits, r.root_w)
                 for m in moves for r in m.results if r is not None)
