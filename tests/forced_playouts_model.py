"""Plain-numpy restatement of forced playouts with policy target pruning (include/yy_engine.h YY_FLAG_FORCED_PLAYOUTS, DESIGN.md
section 3).

TEST INFRASTRUCTURE.  One game, copied boards, K = 1: the search of tests/tree_model.py with forced=k, which asks is_forced()
below at the root, and the exact hash evaluator of hash_eval.py.

  search(root_or_board, player, budget, k)   tree_reuse_model.search with one change: at depth 0 of every descent, with S the sum
                                             of the root's child visits, an edge with N >= 1 and f64(N)*f64(N) < (k*f64(P))*f64(S)
                                             is forced (P the stored prior: the noised one at a noised root), and the descent takes
                                             the forced edge of the lowest action; else the PUCT choice.  k = 0: no change at all.
  prune(edges, k, cpuct)                     -> N' int [len(edges)]: c* = the most visited edge (lowest action on ties) keeps N;
                                             every other edge with N > 0 gives back, one visit at a time and at most n_f =
                                             min{m >= 0: f64(m)*f64(m) >= (k*f64(P))*f64(S)} of them, every visit without which its
                                             float32 PUCT score (N' - 1 in the exploration term, W / N unchanged) stays below c*'s
                                             at the final S; N' == 1 becomes 0.
  distribution(counts, tzero)                Node.get_children_distribution on pruned counts: N' / sum(N') in float64 (uniform 1 / A
                                             when the sum is 0), or uniform over the arg-max set.

The Result carries, next to tree_reuse_model's fields, forced (descents that took a forced edge), pruned int32 [A] (N') and
pi / pi0 (the T = 1 and T = 0 distributions of the pruned counts).

`mutant=` (MUTANTS) breaks one rule on purpose; tests/test_forced_playouts_model.py asserts that the GPU fixtures tell each from
the true model."""
import math

import numpy as np

import tree_model
from tree_model import Tree, advance  # noqa: F401  (advance: re-exported for the callers of this model)

f32 = np.float32

MUTANTS = {
    "forced_le": "an edge is forced while N*N <= k*P*S (not <)",
    "prior_raw": "the forcing test and n_f read the prior from before the root noise",
    "s_root_n": "S is the root's visit count, also on a kept root (whose children hold one less)",
    "keep_one": "pruning leaves an edge with N' == 1 as it is",
    "prune_star": "the most visited edge is pruned like every other, against the highest score among the visited edges",
    "forced_high": "the forced edge of the HIGHEST action is taken",
}


def bound(k, P, S):
    """(k * f64(P)) * f64(S): two float64 products, in this order"""
    return (float(k) * float(P)) * float(S)


def is_forced(k, P, n, S, mutant=None):
    lhs = float(n) * float(n)
    return n >= 1 and (lhs <= bound(k, P, S) if mutant == "forced_le" else lhs < bound(k, P, S))


def score(cpuct, sq, P, nu, nq, w):
    """_select's float32 score, the exploration term with nu visits and the mean value over nq"""
    u = f32(f32(f32(cpuct * P) * sq) / f32(1 + nu))
    q = f32(w / f32(nq)) if nq > 0 else f32(0.0)
    return f32(q + u)


def prune(edges, k, cpuct=1.0, mutant=None, raw=None, S=None):
    """-> list of N' in edge order.  raw: {id(edge): prior before noise} (the prior_raw mutant); S: override (s_root_n)."""
    cpuct = f32(cpuct)
    n = [e.N for e in edges]
    if not edges or max(n) == 0 or not k:
        return n
    S = sum(n) if S is None else S
    sq = f32(math.sqrt(S))
    star = n.index(max(n))                                         # lowest index == lowest action
    es = edges[star]
    best = score(cpuct, sq, es.P, es.N, es.N, es.W)
    if mutant == "prune_star":
        best = max(score(cpuct, sq, e.P, e.N, e.N, e.W) for e in edges if e.N > 0)
    out = []
    for i, e in enumerate(edges):
        if e.N == 0 or (i == star and mutant != "prune_star"):
            out.append(e.N)
            continue
        P = raw[id(e)] if mutant == "prior_raw" else e.P
        b = bound(k, P, S)
        np_, m = e.N, 0
        while np_ >= 1 and float(m) * float(m) < b:                # m < n_f
            if score(cpuct, sq, e.P, np_ - 1, e.N, e.W) < best:
                np_ -= 1
            else:
                break
            m += 1
        out.append(0 if np_ == 1 and mutant != "keep_one" else np_)
    return out


def distribution(counts, tzero):
    counts = np.asarray(counts, np.int64)
    A = counts.size
    if tzero:
        hit = counts == counts.max()
        return hit / float(hit.sum())
    s = int(counts.sum())
    return counts / float(s) if s > 0 else np.full(A, 1.0 / A)


PSCALE = 32.0   # the hash evaluator's priors lie in (0, 1/64]: k * P * S then stays below 1 for every budget here.  The fixtures'
                # evaluator returns them times 32 (a power of two: still exact in float32), priors in (0, 1/2]


def search(root_or_board, player, budget, k, pbits=10, vbits=11, cpuct=1.0, mutant=None, pscale=PSCALE, **options):
    """tree_model.search at K = 1 with forced=k -> Result, with pruned, pi, pi0 (module docstring)."""
    assert mutant is None or mutant in MUTANTS
    s = tree_model.Search(root_or_board, player, budget, 1, pbits, vbits, cpuct=cpuct, forced=k, pscale=pscale,
                          mutant=mutant and "forced_playouts." + mutant, **options).run()
    r = s.result()
    edges = s.root.edges
    r.pruned = np.zeros(s.A, np.int32)
    S = s.tree.n if (mutant == "s_root_n" and edges) else None
    for e, npr in zip(edges, prune(edges, k, cpuct, mutant, s.raw, S)):
        r.pruned[e.action] = npr
    r.pi, r.pi0 = distribution(r.pruned, False), distribution(r.pruned, True)
    return r


# ------------------------------------------------------------------------------------------------ the fixtures of the GPU tests
# 8 games per board, root noise as numpy Dirichlet(0.3) draws.  Games 0 .. 2 start 0 .. 3 plies into a game: wide roots (at 9x12
# more than 64 children, so the edges span two 64-lane chunks), where a prior is far too small for a budget of 8 to force anything.
# Games 3 .. 7 start late in a game, at a position with 2 .. 4 legal moves: priors of 0.25 .. 0.5, which k * P * S lifts above 1 within
# a budget of 8 even for k = 0.5 and without noise.  SEEDS were picked so that, for every (board, budget, eps, k), at least half of
# the games show a forced descent and at least half a pruned edge (tests/test_forced_playouts_model.py asserts it).
SHAPES = {"4x4": (4, 4), "5x7": (5, 7), "8x8": (8, 8), "9x12": (9, 12)}
BUDGETS = (8, 24, 64)
EPSILONS = (0.25, 0.0)
KS = (2.0, 0.5)
GAMES = 8
LATE = (2, 2, 3, 3, 4)                                               # legal moves at the roots of games 3 .. 7, at most
# The hash evaluator as it is (priors at most 1/64, so at most 1 in sum on 8x8): k * P * S reaches 1 only for a large k.  One
# fixture of realistic prior magnitudes: (board, budget, eps, k), searched with pscale = 1.
UNSCALED = ("8x8", 64, 0.0, 64.0)
SEEDS = {"4x4": 9, "5x7": 6, "8x8": 3, "9x12": 1}


def roots(name, seed=None):
    """-> boards int8 [GAMES, R, C], players int8 [GAMES], noise float64 [GAMES, A], noise2 (for the kept root of the next move)"""
    import oracle_lib as O
    R, C = SHAPES[name]
    rng = np.random.default_rng([SEEDS[name] if seed is None else seed, R, C])
    boards = np.zeros((GAMES, R, C), np.int8)
    players = np.ones(GAMES, np.int8)
    for g in range(GAMES):
        while True:
            b, p = np.zeros((R, C), np.int8), 1
            want = LATE[g - 3] if g >= 3 else None
            plies = int(rng.integers(0, 4))
            ok = False
            for t in range(R * C):
                if float(O.game_ended(b[None], [p])[0]) != 0.0:
                    break
                legal = np.flatnonzero(O.valid_mask(b[None], [p])[0])
                if (want is None and t == plies) or (want is not None and 2 <= len(legal) <= want):
                    ok = True
                    break
                if len(legal) == 0:
                    break
                b.flat[rng.choice(legal)] = p
                p = -p
            if ok:
                boards[g], players[g] = b, p
                break
    noise = np.zeros((2, GAMES, R * C))
    for n in noise:
        for g in range(GAMES):
            n[g] = rng.dirichlet(np.full(R * C, 0.3))              # over all cells: a root reads its own moves' entries
    return boards, players, noise[0], noise[1]


_CACHE = {}


def fixture(name, budget, eps, k, mutant=None, pscale=PSCALE):
    """-> (first, second): per game the Result of the search from the fixture root and of the search that follows the most
    visited move on the tree advance() keeps (None where nothing is kept or the game is over: the device test skips those)."""
    import oracle_lib as O
    key = (name, budget, eps, k, mutant, pscale)
    if key in _CACHE:
        return _CACHE[key]
    boards, players, noise, noise2 = roots(name)
    first, second = [], []
    for g in range(GAMES):
        r = search(boards[g], players[g], budget, k, noise=noise[g] if eps else None, eps=eps, mutant=mutant, pscale=pscale)
        snap = (r.counts.copy(), r.child_w.copy(), r.child_p.copy(), r.pruned.copy(), r.pi.copy(), r.pi0.copy(), r.forced)
        a = int(np.argmax(r.counts))
        r2 = None
        if r.counts[a] > 0:
            tree, kept = advance(r.tree, a)
            b = boards[g].copy()
            b.flat[a] = players[g]
            if tree is not None and kept < budget and float(O.game_ended(b[None], [-players[g]])[0]) == 0.0:
                r2 = search(tree, -players[g], budget, k, noise=noise2[g] if eps else None, eps=eps, mutant=mutant, pscale=pscale)
                r2.board, r2.action = b, a
        r.counts, r.child_w, r.child_p, r.pruned, r.pi, r.pi0, r.forced = snap
        first.append(r)
        second.append(r2)
    _CACHE[key] = (first, second)
    return first, second
