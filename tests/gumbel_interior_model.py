"""Plain-numpy restatement of Gumbel search below the root (include/yy_engine.h YY_FLAG_GUMBEL_INTERIOR).

TEST INFRASTRUCTURE.  The search of tests/gumbel_model.py with interior=True: the root keeps the evaluator's value of its
position, an unvisited child is completed with v_mix, and below the root a descent takes the child of the largest
pi'(a) - N(a) / (1 + S).  Every operation is the device's, one rounding each, in the same order -- python floats are IEEE
float64 with round-to-nearest and never contracted -- so the comparison with the device is equality:

  E(x)                        exp(x) for x <= 0 from correctly rounded products and sums and an exact scaling
  improved(edges, vhat, ..)   (t per edge, Z, S, v_mix): pi'(a) = t(a) / Z
  select_interior(...)        the edge a descent takes below the root
  Search(..., interior=True)  the search; policy() is pi' completed with v_mix, winner() the Gumbel winner as before

A node's own evaluator value is what the evaluator returned for its board (nodes own their boards: copied boards only), kept
by position as the rows are evaluated.  interior=False is gumbel_model.Search, tally for tally."""
import math

import numpy as np

import gumbel_model as G

f32 = np.float32
LOG2E, LN2_HI, LN2_LO = float.fromhex("0x1.71547652b82fep+0"), float.fromhex("0x1.62e42feep-1"), float.fromhex("0x1.a39ef35793c76p-33")
FACT = [1.0 / float(math.factorial(i)) for i in range(14)]           # the float64 quotients 1.0 / i!
NAN_TERM = -1                                                        # the term of an edge whose sigma is a NaN against the maximum
# one deliberately broken rule each: completion by the visited children's SW / SN instead of v_mix; N / S instead of N / (1 + S);
# the highest edge on ties; the root's own value left at 0
MUTANTS = ("cq_mean", "n_over_s", "tie_high", "root_vhat_zero")


def E(x):
    x = float(x)
    if x < -708.0:
        return 0.0
    n = float(np.rint(x * LOG2E))
    r = (x + (-(n * LN2_HI))) + (-(n * LN2_LO))
    p = FACT[13]
    for i in range(12, -1, -1):
        p = p * r + FACT[i]                                          # two roundings: python does not contract
    return math.ldexp(p, int(n))


def prior(e):
    x = float(e.P) * 1099511627776.0
    return int(x) if x > 0.0 else 0                                   # units of 2^-40, truncated; negative or NaN: 0


def improved(edges, vhat, c_visit, c_scale, mutant=None):
    """-> (t [k], Z, S, v_mix)"""
    S = sum(e.N for e in edges)
    mx = max(e.N for e in edges)
    p = [prior(e) for e in edges]
    q = [float(e.W) / float(e.N) if e.N > 0 else None for e in edges]
    spv = sum(pi for pi, e in zip(p, edges) if e.N > 0)
    pq = [float(pi) * qi for pi, qi, e in zip(p, q, edges) if e.N > 0]
    spq = sum(int(x) for x in pq if abs(x) < 2.0 ** 62)              # int(): toward zero; a NaN or infinite product adds nothing
    vmix = float(vhat)
    if S > 0:
        wq = float(spq) / float(spv) if spv else 0.0
        vmix = (float(vhat) + float(S) * wq) / float(1 + S)
    if mutant == "cq_mean":
        sw = sum(int(float(e.W) * 4294967296.0) for e in edges if e.N > 0)
        vmix = (float(sw) * 2.0 ** -32) / float(S) if S else 0.0
    scale = (float(c_visit) + float(mx)) * float(c_scale)
    x = [scale * (qi if qi is not None else vmix) for qi in q]
    live = [xi for xi, pi in zip(x, p) if pi and xi == xi]
    xm = max(live) if live else -math.inf
    t = []
    for xi, pi in zip(x, p):
        if not any(p):
            t.append(1)
        elif not pi:
            t.append(0)
        else:
            a = xi + (-xm)
            t.append(NAN_TERM if a != a else int((float(pi) * E(a)) * 4096.0))
    return t, sum(ti for ti in t if ti != NAN_TERM), S, vmix


def pi_prime(edges, vhat, c_visit, c_scale, mutant=None):
    t, Z, _, _ = improved(edges, vhat, c_visit, c_scale, mutant)
    return [math.nan if ti == NAN_TERM or Z == 0 else float(ti) / float(Z) for ti in t]     # Z == 0: the device's 0 / 0


def select_interior(edges, vhat, c_visit, c_scale, mutant=None):
    """-> the edge of the largest pi'(a) - N(a) / (1 + S), the lowest on ties; None when every score is a NaN"""
    t, Z, S, _ = improved(edges, vhat, c_visit, c_scale, mutant)
    best, bs = None, None
    for e, ti in zip(edges, t):
        if ti == NAN_TERM or Z == 0:
            continue
        den = float(S) if mutant == "n_over_s" else float(1 + S)
        sc = float(ti) / float(Z) + (-(float(e.N) / den if den else 0.0))
        if sc != sc:
            continue
        if best is None or sc > bs or (mutant == "tie_high" and sc == bs):
            best, bs = e, sc
    return best


class Search(G.Search):
    def __init__(self, board, player, n, m, interior=True, mutant=None, evaluator=None, **options):
        """gumbel_model.Search with interior: the rule above below the root and v_mix in policy().  mutant: a name of MUTANTS."""
        self.interior, self.values = bool(interior), {}
        inner = evaluator

        def recording(boards):
            if inner is None:
                from hash_eval import hash_eval_batch
                pol, val = hash_eval_batch(boards, options.get("pbits", 10), options.get("vbits", 11))
                pol = pol * f32(options.get("pscale", 1.0))
            else:
                pol, val = inner(boards)
            for b, v in zip(boards, val):
                self.values[np.asarray(b, np.int8).tobytes()] = f32(v)
            return pol, val

        super().__init__(board, player, n, m, evaluator=recording,
                         mutant=None if mutant is None else "gumbel_interior." + mutant, **options)
        if self.root.board.tobytes() not in self.values:           # a root expanded from a given row: its value is still the evaluator's
            recording(self.root.board[None])

    def vhat(self, node):
        if node is self.root and self.own("gumbel_interior") == "root_vhat_zero":
            return f32(0.0)
        return self.values[node.board.tobytes()]

    def choose(self, node, vc, s_parent):
        if self.interior and node is not self.root:
            return select_interior(node.edges, self.vhat(node), self.cv, self.cs, self.own("gumbel_interior"))
        return super().choose(node, vc, s_parent)

    def policy(self):
        """pi' float64 [A]"""
        if not self.interior or not self.root.edges:
            return super().policy()
        out = np.zeros(self.A)
        for e, x in zip(self.root.edges, pi_prime(self.root.edges, self.vhat(self.root), self.cv, self.cs, self.own("gumbel_interior"))):
            out[e.action] = x
        return out


# ------------------------------------------------------------------------------------------------ the shapes of the tests
# (name, board, budgets, m): the issue's table.  4x4: small k, deep trees; 5x7: non-square, one word; 1x6: nodes with 1 - 2
# children, passes; 9x12: 108 edges, two words; 12x12: 144 edges, three words
CASES = [("4x4-16", (4, 4), 16, 4), ("4x4-48", (4, 4), 48, 4), ("5x7", (5, 7), 32, 8), ("1x6", (1, 6), 12, 16),
         ("9x12", (9, 12), 24, 4), ("12x12", (12, 12), 24, 3)]
GAMES = 8
SEED = 4711


def fixture(shape, n, m, g, boards, players, interior=True, mutant=None, **options):
    """The model search of game g of a case on host base scores (the CPU tests); the GPU tests set the device's own."""
    s = Search(boards[g], players[g], n, m, interior=interior, mutant=mutant, **options)
    s.host_s0(G.gumbel_rows(SEED, [g], [0], shape[0] * shape[1])[0])
    return s


def walk(s):
    """every node of the model's tree, root first, following the edges in order: (path of actions, node)"""
    out, stack = [], [((), s.root)]
    while stack:
        path, node = stack.pop()
        out.append((path, node))
        stack += [(path + (e.action,), e.child) for e in reversed(node.edges) if e.child is not None]
    return out


def tally(s):
    """what the GPU tests compare after a search: every node's edges (action, N, W bits), the winner and pi' (bits)"""
    tree = [(path, [(e.action, e.N, int(f32(e.W).view(np.uint32))) for e in node.edges]) for path, node in walk(s)]
    return tree, s.winner(), s.policy().view(np.uint64).tolist()
