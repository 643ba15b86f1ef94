"""Plain-numpy restatement of the Gumbel root search (include/yy_engine.h YY_FLAG_GUMBEL_ROOT).

TEST INFRASTRUCTURE.  One game, copied boards, K = 1: the search of tests/tree_model.py with m > 0, which asks select_root()
below at the root, and the exact hash evaluator of hash_eval.py.  Below the root the search is plain PUCT; the root differs:

  seq(m, n)                 the considered-visit sequence, mctx's table; seq_at(m, n, S) the device's closed form of seq(m, n)[S]
  gumbel(seed, gid, ply, a) the draw: f32(-log(-log(u))) over tests/philox_ref.py, purpose 4
  score(s0, N, W, maxN)     f32(s0 + sigma), sigma = f32(f32(f32(c_visit + maxN) * c_scale) * q), q = f32(W / N) or 0
  Search(...)               the search, one simulation per step(): at the root, with S the children's visits and v = seq[S], the
                            child with N == v (any child when there is none) of the largest score, the lowest edge on ties
  winner(), policy()        the move and pi' = softmax(log P + sigma64(completed q)) in float64

The base scores s0 = f32(f64(g) + log(f64(P))) are an INPUT (set_s0: the device's own, read with root_gumbel()), so that no
comparison of a selection depends on a libm; host_s0() computes them with numpy's log for the CPU-only tests."""
import math

import numpy as np

import philox_ref as P
import tree_model

f32 = np.float32
PURPOSE = 4


def seq(m, n):
    """mctx's considered-visit table for m considered actions and n simulations"""
    if m <= 1:
        return list(range(n))
    L = int(math.ceil(math.log2(m)))
    visits, c, out = [0] * m, m, []
    while len(out) < n:
        extra = max(1, n // (L * c))
        for _ in range(extra):
            out += visits[:c]
            for i in range(c):
                visits[i] += 1
        c = max(2, c // 2)
    return out[:n]


def seq_at(m, n, S):
    """the device's form: inside a phase the c considered actions all hold v visits at its start"""
    if m <= 1:
        return S
    L = (m - 1).bit_length()
    c, v, pos = m, 0, 0
    while True:
        extra = max(1, n // (L * c))
        if S < pos + extra * c:
            return v + (S - pos) // c
        pos, v, c = pos + extra * c, v + extra, max(2, c // 2)


def gumbel(seed, gid, ply, a):
    """-> (f32 g, float64 value before the rounding)"""
    r = P.draw(seed, gid, ply, PURPOSE, a)
    u = P.u01(r[0], r[1])
    if u == 0.0:
        u = 2.0 ** -54
    g = -math.log(-math.log(u))
    return f32(g), g


def gumbel_rows(seed, gids, plies, A):
    return np.array([[gumbel(seed, int(g), int(p), a)[0] for a in range(A)] for g, p in zip(gids, plies)], np.float32)


def score(s0, N, W, maxN, c_visit, c_scale):
    with np.errstate(all="ignore"):
        q = f32(f32(W) / f32(N)) if N > 0 else f32(0.0)
        sg = f32(f32(f32(f32(c_visit) + f32(maxN)) * f32(c_scale)) * q)
        return f32(f32(s0) + sg)


def best_of(edges, idx, s0, maxN, c_visit, c_scale):
    """the index in idx of the largest score, the lowest on ties (-inf ties included); a NaN score is never taken"""
    best, bs = None, None
    for i in idx:
        sc = score(s0[i], edges[i].N, edges[i].W, maxN, c_visit, c_scale)
        if sc != sc:
            continue
        if best is None or sc > bs:
            best, bs = i, sc
    return best


def select_root(edges, s0, n, m, c_visit, c_scale):
    """-> the edge a descent takes at the root; n: the budget, s0: the base scores in edge order"""
    S = sum(e.N for e in edges)
    v = seq(min(m, len(edges)), n)[S]
    maxN = max(e.N for e in edges)
    cand = [i for i, e in enumerate(edges) if e.N == v] or list(range(len(edges)))
    return edges[best_of(edges, cand, s0, maxN, c_visit, c_scale)]


class Search(tree_model.Search):
    def __init__(self, board, player, n, m, c_visit=50.0, c_scale=1.0, **options):
        """tree_model.Search at K = 1 with the root rule; zero_prior: an action whose root prior is set to exactly 0 (s0 = -inf)"""
        super().__init__(board, player, n, 1, m=m, c_visit=c_visit, c_scale=c_scale, **options)

    def host_s0(self, g_row):
        with np.errstate(divide="ignore"):
            self.set_s0({e.action: f32(float(g_row[e.action]) + np.log(np.float64(e.P))) for e in self.root.edges})

    def set_s0(self, by_action):
        """by_action: array [A] or dict of the root children's base scores"""
        self.s0 = [f32(by_action[e.action]) for e in self.root.edges]

    # ---- read-outs, by action
    def counts(self):
        return self.result().counts

    def child_w(self):
        return self.result().child_w

    def child_p(self):
        return self.result().child_p

    def winner(self):
        edges = self.root.edges
        if not edges:
            return -1
        mx = max(e.N for e in edges)
        cand = [i for i, e in enumerate(edges) if e.N == mx]
        i = best_of(edges, cand, self.s0, mx, self.cv, self.cs)
        return edges[cand[0] if i is None else i].action

    def policy(self):
        """pi' float64 [A]"""
        edges = self.root.edges
        if not edges:
            return np.full(self.A, 1.0 / self.A)
        mx = max(e.N for e in edges)
        sn = sum(e.N for e in edges)
        sw = sum(int(float(e.W) * 4294967296.0) for e in edges if e.N > 0)      # int(): toward zero
        cq0 = (float(sw) * 2.0 ** -32) / float(sn) if sn else 0.0
        scale = (float(self.cv) + float(mx)) * float(self.cs)
        with np.errstate(divide="ignore"):
            logit = np.array([np.log(np.float64(e.P)) + scale * (float(e.W) / float(e.N) if e.N > 0 else cq0) for e in edges])
        lm = logit.max()
        x = np.exp(logit - lm) if lm > -np.inf else np.ones(len(edges))
        out = np.zeros(self.A)
        for e, xi in zip(edges, x / x.sum()):
            out[e.action] = xi
        return out


# ------------------------------------------------------------------------------------------------ the shapes of the GPU tests
# (board, n, m): the issue's table.  1x6: k < m and passes; 9x12: two edge words, n < m'; 12x12: three words, odd m
CASES = [("4x4", (4, 4), 16, 4), ("5x7", (5, 7), 24, 16), ("1x6", (1, 6), 8, 16), ("9x12", (9, 12), 8, 16), ("12x12", (12, 12), 8, 3)]
GAMES = 4
SEED = 20240


def roots(shape, games=GAMES, seed=5):
    """-> boards int8 [games, R, C], players int8 [games]: game g starts g plies (random legal moves) into a game"""
    import oracle_lib as O
    R, C = shape
    rng = np.random.default_rng([seed, R, C])
    boards, players = np.zeros((games, R, C), np.int8), np.ones(games, np.int8)
    for g in range(games):
        b, p = np.zeros((R, C), np.int8), 1
        for _ in range(g):
            legal = np.flatnonzero(O.valid_mask(b[None], [p])[0])
            if float(O.game_ended(b[None], [p])[0]) != 0.0 or len(legal) == 0:
                break
            nb = b.copy()
            nb.flat[rng.choice(legal)] = p
            if float(O.game_ended(nb[None], [-p])[0]) != 0.0 or not O.valid_mask(nb[None], [-p])[0].any():
                break                                               # keep a root that is not over and has a move
            b, p = nb, -p
        boards[g], players[g] = b, p
    return boards, players
