"""Plain-numpy float32 restatement of the leaf-parallel search (leaves_per_step K, include/yy_engine.h and DESIGN.md).

TEST INFRASTRUCTURE.  One game, copied boards, the rules of the CPU oracle (oracle_lib) and the exact hash evaluator of
hash_eval.py.  Every step runs K_eff = min(K, simulations not yet started) descents on the tree as it stands; descent j sees
on every edge the virtual count v of the descents 0 .. j-1 of this step that walked it, and scores a child with n = N + v,
w = v > 0 ? f32(W - f32(v)) : W, S = sum of the children's n.  A descent that ends on the leaf of an earlier one (same
unexpanded edge, same childless node) takes no evaluation and shares the earlier one's.  Then, in descent order, the first
occurrence of a leaf expands it and every descent backs its value up.  At K = 1 this is the reference's search
(oracle_lib.search_hash), which tests/test_leaf_parallel_model.py checks."""
import math

import numpy as np

import oracle_lib as O
from hash_eval import hash_eval_batch

f32 = np.float32
TERMINAL, EXPAND, REEXPAND, ROOTPASS = "terminal", "expand", "reexpand", "rootpass"


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
    ended = float(O.game_ended(node.board[None], [node.player], flags)[0])
    node.edges = []
    if ended != 0.0:
        node.terminal, node.tv = True, ended                      # python number: 1, -1 or 0.0001
        return
    mask = O.valid_mask(node.board[None], [node.player], flags)[0]
    legal = np.flatnonzero(mask)
    mix = noise is not None and bool(np.any(np.asarray(noise)[legal] != 0.0))
    keep = f32(1.0 - eps)
    for a in legal:
        p = f32(policy[a])
        if mix:
            p = f32(float(f32(keep * p)) + eps * float(noise[a]))
        node.edges.append(Edge(int(a), p))


def _select(node, vc, cpuct):
    S = sum(e.N + vc.get(id(e), 0) for e in node.edges)
    sq = f32(math.sqrt(S))
    best, best_ucb = None, -math.inf
    for e in node.edges:
        v = vc.get(id(e), 0)
        n = e.N + v
        w = f32(e.W - f32(v)) if v > 0 else e.W
        u = f32(f32(f32(cpuct * e.P) * sq) / f32(1 + n))
        q = f32(w / f32(n)) if n > 0 else f32(0.0)
        ucb = f32(q + u)
        if ucb > best_ucb:                                         # strict >: the lowest action wins ties
            best, best_ucb = e, ucb
    return best


def search(board, player, sims, K, pbits=10, vbits=11, noise=None, eps=0.25, cpuct=1.0, flags=0, trace=None):
    """-> Result with counts int32 [A], child_w f32 [A], child_p f32 [A], root_visits, root_w (float), evals, steps.
    trace: optional list; every step appends [(kind, actions on the path, dup index or -1)] per descent."""
    board = np.array(board, np.int8)
    R, C = board.shape
    A = R * C
    cpuct = f32(cpuct)
    root = Node(board, int(player))
    pol, _ = hash_eval_batch(board[None], pbits, vbits)           # root call, value discarded (mcts.py:295)
    _expand(root, pol[0], flags, noise, eps)
    root_n, root_w_py, root_is_py, root_wf = 0, 0.0, True, f32(0.0)
    evals = steps = 0
    while root_n < sims:
        keff = min(K, sims - root_n)
        steps += 1
        vc, desc, first_of = {}, [], {}
        for j in range(keff):                                      # selection phase: the tree does not change
            node, path, parent = root, [], None
            while True:
                if node.terminal:
                    kind = TERMINAL
                    break
                if not node.edges:
                    kind = ROOTPASS if node is root else REEXPAND
                    break
                e = _select(node, vc, cpuct)
                path.append(e)
                parent = node
                if e.child is None:
                    kind = EXPAND
                    break
                node = e.child
            for e in path:
                vc[id(e)] = vc.get(id(e), 0) + 1
            key = id(path[-1]) if kind == EXPAND else id(node)
            dup = first_of.setdefault(key, j) if kind != TERMINAL else j
            desc.append(dict(kind=kind, path=path, node=node, parent=parent, dup=dup if dup != j else -1))
        rows = [d for d in desc if d["kind"] != TERMINAL and d["dup"] < 0]
        boards = []
        for d in rows:
            if d["kind"] == EXPAND:
                par, e = d["parent"], d["path"][-1]
                b = par.board.copy()
                b.flat[e.action] = par.player                    # a legal move of the parent always places (copied boards)
                d["board"], d["player"] = b, -par.player
            else:
                d["board"], d["player"] = d["node"].board, d["node"].player
            boards.append(d["board"])
        if boards:
            P, V = hash_eval_batch(np.stack(boards), pbits, vbits)
            for i, d in enumerate(rows):
                d["policy"], d["value"] = P[i], f32(V[i])
        evals += len(rows)
        if trace is not None:
            trace.append([(d["kind"], [e.action for e in d["path"]], d["dup"]) for d in desc])
        for d in desc:                                             # expansion + backup phase, in descent order
            if d["kind"] == TERMINAL:
                v, v_is_py = d["node"].tv, True
            elif d["dup"] >= 0:
                v, v_is_py = desc[d["dup"]]["value"], False
            else:
                v, v_is_py = d["value"], False
                if d["kind"] == EXPAND:
                    child = Node(d["board"], d["player"])
                    d["path"][-1].child = child
                    _expand(child, d["policy"], flags)
                else:
                    _expand(d["node"], d["policy"], flags)
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
    return r
