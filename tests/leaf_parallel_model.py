"""Plain-numpy float32 restatement of the leaf-parallel search (leaves_per_step K, include/yy_engine.h and DESIGN.md).

TEST INFRASTRUCTURE.  One game, copied boards, the rules of the CPU oracle (oracle_lib) and the exact hash evaluator of
hash_eval.py.  Every step runs K_eff = min(K, simulations not yet started) descents on the tree as it stands; descent j sees
on every edge the virtual count v of the descents 0 .. j-1 of this step that walked it, and scores a child with n = N + v,
w = v > 0 ? f32(W - f32(v)) : W, S = sum of the children's n.  A descent that ends on the leaf of an earlier one (same
unexpanded edge, same childless node) takes no evaluation and shares the earlier one's.  Then, in descent order, the first
occurrence of a leaf expands it and every descent backs its value up.  At K = 1 this is the reference's search
(oracle_lib.search_hash), which tests/test_leaf_parallel_model.py checks.

The device counters (BatchedMCTS.COUNTERS, GameState.ctr in csrc/yy_engine.hip) are counted where the kernels count them:
  levels             every edge a descent walks (one select_child call), so at the end the sum of N over all edges;
  children_scanned   the children of the node of every such call;
  children_created   the edges of every node expanded WITH children -- the root's own expansion included (the root call goes
                     through the same expand_leaf), a terminal or childless node adds 0, and so does a re-expansion;
  nodes              the nodes a search adds below the root, one per `expand` leaf -- the root itself is NOT counted;
  terminal_revisits  the descents that ended on a terminal node, a terminal root's included;
  evals              the evaluator rows asked for after the root call (the root call is not counted).
evals + terminal descents + duplicate descents == root_visits.  A failed game (NaN value or prior, full arena, path too deep)
is outside this model: it has no arena and no NaN.  On the device such a game keeps what it counted up to the failure -- levels,
children_scanned and terminal_revisits of the descents walked, evals of every step whose selection completed (the step whose
expansion then fails included), nodes and children_created of the expansions done before the failing one -- and counts nothing
afterwards.

`mutant=` (MUTANTS) breaks one rule on purpose; tests/test_leaf_parallel_model.py asserts that the GPU cases tell each from the
true model."""
import math

import numpy as np

import oracle_lib as O
from hash_eval import hash_eval_batch

f32 = np.float32
TERMINAL, EXPAND, REEXPAND, ROOTPASS = "terminal", "expand", "reexpand", "rootpass"

MUTANTS = {
    "keep_w": "the virtual visits are not subtracted from W (w = W, n = N + v)",
    "s_parent": "S is N(node) - 1 (the root: its completed simulations), not the sum of the children's N + v",
    "dup_row": "a duplicate leaf takes an evaluator row of its own",
    "tie_high": "ties go to the highest action",
    "full_last": "the last step runs K descents, not K_eff",
    "reverse_backup": "the expansion + backup phase runs in reverse descent order",
    "terminal_f32": "a terminal value is backed up as float32 where the python-float rule applies (terminal root)",
    "v_low64": "virtual counts are dropped for the children of index >= 64 of a node",
}


class Descent(tuple):
    """One descent of a step in the trace: unpacks as (kind, actions on the path, dup index or -1); needs_eval says whether
    its evaluator row g*K + j is flagged, and then board int8 [R, C] / player are the position that row holds (else None)."""

    def __new__(cls, kind, actions, dup, needs_eval, board, player):
        self = super().__new__(cls, (kind, actions, dup))
        self.kind, self.actions, self.dup = kind, actions, dup
        self.needs_eval, self.board, self.player = needs_eval, board, player
        return self


class Edge:
    __slots__ = ("action", "P", "N", "W", "child")

    def __init__(self, action, P):
        self.action, self.P, self.N, self.W, self.child = action, f32(P), 0, f32(0.0), None


class Node:
    __slots__ = ("board", "player", "edges", "terminal", "tv")

    def __init__(self, board, player):
        self.board, self.player, self.edges, self.terminal, self.tv = board, player, [], False, 0.0


class Result:
    pass


def _expand(node, policy, flags, noise=None, eps=0.25):
    """-> the number of children created"""
    ended = float(O.game_ended(node.board[None], [node.player], flags)[0])
    node.edges = []
    if ended != 0.0:
        node.terminal, node.tv = True, ended                      # python number: 1, -1 or 0.0001
        return 0
    mask = O.valid_mask(node.board[None], [node.player], flags)[0]
    legal = np.flatnonzero(mask)
    mix = noise is not None and bool(np.any(np.asarray(noise)[legal] != 0.0))
    keep = f32(1.0 - eps)
    for a in legal:
        p = f32(policy[a])
        if mix:
            p = f32(float(f32(keep * p)) + eps * float(noise[a]))
        node.edges.append(Edge(int(a), p))
    return len(node.edges)


def _select(node, vc, cpuct, mutant=None, s_parent=0):
    def virt(i, e):
        return 0 if (mutant == "v_low64" and i >= 64) else vc.get(id(e), 0)

    S = s_parent if mutant == "s_parent" else sum(e.N + virt(i, e) for i, e in enumerate(node.edges))
    sq = f32(math.sqrt(S))
    best, best_ucb = None, -math.inf
    for i, e in enumerate(node.edges):
        v = virt(i, e)
        n = e.N + v
        w = f32(e.W - f32(v)) if v > 0 and mutant != "keep_w" else e.W
        u = f32(f32(f32(cpuct * e.P) * sq) / f32(1 + n))
        q = f32(w / f32(n)) if n > 0 else f32(0.0)
        ucb = f32(q + u)
        if ucb > best_ucb or (mutant == "tie_high" and ucb == best_ucb):    # strict >: the lowest action wins ties
            best, best_ucb = e, ucb
    return best


def search(board, player, sims, K, pbits=10, vbits=11, noise=None, eps=0.25, cpuct=1.0, flags=0, trace=None, mutant=None,
           evaluator=None):
    """-> Result with counts int32 [A], child_w f32 [A], child_p f32 [A], root_visits, root_w (float), evals, steps, the
    counters levels, children_scanned, children_created, terminal_revisits, nodes (module docstring), duplicates, and root (the
    final tree).  trace: optional list; every step appends one Descent per descent.  evaluator(boards int8 [n, R, C]) ->
    (policy f32 [n, A], value f32 [n]) replaces the hash evaluator.  mutant: one of MUTANTS, or None for the true search."""
    assert mutant is None or mutant in MUTANTS
    if evaluator is None:
        evaluator = lambda b: hash_eval_batch(b, pbits, vbits)
    board = np.array(board, np.int8)
    R, C = board.shape
    A = R * C
    cpuct = f32(cpuct)
    root = Node(board, int(player))
    pol, _ = evaluator(board[None])                               # root call, value discarded (mcts.py:295)
    created = _expand(root, pol[0], flags, noise, eps)
    root_n, root_w_py, root_is_py, root_wf = 0, 0.0, True, f32(0.0)
    evals = steps = levels = scanned = revisits = nodes = duplicates = 0
    while root_n < sims:
        keff = K if mutant == "full_last" else min(K, sims - root_n)
        steps += 1
        vc, desc, first_of = {}, [], {}
        for j in range(keff):                                      # selection phase: the tree does not change
            node, path, parent, s_parent = root, [], None, root_n
            while True:
                if node.terminal:
                    kind = TERMINAL
                    break
                if not node.edges:
                    kind = ROOTPASS if node is root else REEXPAND
                    break
                e = _select(node, vc, cpuct, mutant, s_parent)
                levels += 1
                scanned += len(node.edges)
                path.append(e)
                parent, s_parent = node, e.N - 1
                if e.child is None:
                    kind = EXPAND
                    break
                node = e.child
            for e in path:
                vc[id(e)] = vc.get(id(e), 0) + 1
            key = id(path[-1]) if kind == EXPAND else id(node)
            dup = first_of.setdefault(key, j) if kind != TERMINAL else j
            desc.append(dict(kind=kind, path=path, node=node, parent=parent, dup=dup if dup != j else -1))
        for d in desc:
            d["need"] = d["kind"] != TERMINAL and (d["dup"] < 0 or mutant == "dup_row")
            if d["kind"] == TERMINAL:
                d["board"] = d["player"] = None
            elif d["kind"] == EXPAND:
                par, e = d["parent"], d["path"][-1]
                b = par.board.copy()
                b.flat[e.action] = par.player                    # a legal move of the parent always places (copied boards)
                d["board"], d["player"] = b, -par.player
            else:
                d["board"], d["player"] = d["node"].board, d["node"].player
        rows = [d for d in desc if d["need"]]
        if rows:
            P, V = evaluator(np.stack([d["board"] for d in rows]))
            for i, d in enumerate(rows):
                d["policy"], d["value"] = P[i], f32(V[i])
        evals += len(rows)
        revisits += sum(d["kind"] == TERMINAL for d in desc)
        duplicates += sum(d["dup"] >= 0 for d in desc)
        if trace is not None:
            trace.append([Descent(d["kind"], [e.action for e in d["path"]], d["dup"], d["need"],
                                  d["board"] if d["need"] else None, d["player"] if d["need"] else None) for d in desc])
        for d in (reversed(desc) if mutant == "reverse_backup" else desc):   # expansion + backup phase, in descent order
            if d["kind"] == TERMINAL:
                v, v_is_py = d["node"].tv, mutant != "terminal_f32"
            elif d["dup"] >= 0:
                v, v_is_py = desc[d["dup"]]["value"], False
            else:
                v, v_is_py = d["value"], False
                if d["kind"] == EXPAND:
                    child = Node(d["board"], d["player"])
                    d["path"][-1].child = child
                    created += _expand(child, d["policy"], flags)
                    nodes += 1
                else:
                    created += _expand(d["node"], d["policy"], flags)
            depth = len(d["path"])
            v32 = f32(v)
            for i, e in enumerate(d["path"]):
                sv = -v32 if (depth - (i + 1)) & 1 else v32
                e.N += 1
                e.W = f32(e.W + sv)
            root_n += 1
            if root_is_py and v_is_py and depth == 0:
                root_w_py += -v if depth & 1 else v
            else:
                sv = -v32 if depth & 1 else v32
                base = f32(root_w_py) if root_is_py else root_wf
                root_wf = f32(base + sv)
                root_is_py = False
    r = Result()
    r.counts = np.zeros(A, np.int32)
    r.child_w = np.zeros(A, np.float32)
    r.child_p = np.zeros(A, np.float32)
    for e in root.edges:
        r.counts[e.action], r.child_w[e.action], r.child_p[e.action] = e.N, e.W, e.P
    r.root_visits = root_n
    r.root_w = root_w_py if root_is_py else float(root_wf)
    r.evals, r.steps = evals, steps
    r.levels, r.children_scanned, r.children_created, r.terminal_revisits, r.nodes = levels, scanned, created, revisits, nodes
    r.duplicates, r.root = duplicates, root
    return r
