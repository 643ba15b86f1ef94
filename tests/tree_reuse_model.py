"""Plain-numpy float32 restatement of tree reuse across moves (include/yy_engine.h yy_mcts_advance).

TEST INFRASTRUCTURE.  One game, copied boards, K = 1, on the Node / Edge / _expand / _select of leaf_parallel_model.py and the
exact hash evaluator of hash_eval.py.

  search(root_or_board, player, budget)  a board: the reference's search from a fresh root (oracle_lib.search_hash, and
                                         leaf_parallel_model.search at K = 1).  A Tree (what advance() returns): the search
                                         tops the kept root up -- it stops when root.visits == budget, so a root that already
                                         holds its budget runs nothing.  The root call is made either way; on a kept root its
                                         policy row is ignored and a noise row that is non-zero over the root's moves is mixed
                                         into the STORED priors, p = f32(f64(f32(1-eps)*P) + eps*noise).
  advance(tree, action)                  -> (Tree or None, kept_visits).  The child under `action` becomes the root when the
                                         root has an edge with that action whose child is a node that is not terminal and has
                                         children; its visits are the edge's N, its value sum the edge's W (float32).

Counters are counted per search() call the way leaf_parallel_model counts them (its module docstring); a kept root adds no
children_created of its own (it is not expanded again).

`mutant=` (MUTANTS) breaks one rule on purpose; tests/test_tree_reuse_model.py asserts that the GPU cases' inputs tell each from
the true model."""
import numpy as np

from hash_eval import hash_eval_batch
from leaf_parallel_model import EXPAND, REEXPAND, ROOTPASS, TERMINAL, Node, Result, _expand, _select

f32 = np.float32

MUTANTS = {
    "root_sum": "the kept root's visits are the sum of its children's N (one less than the edge's N)",
    "budget_additional": "the budget of a kept root counts additional simulations, not the root's visits",
    "noise_policy": "noise on a kept root is mixed into the root call's policy row, not into the stored priors",
    "keep_terminal": "a terminal child is kept",
    "edge_order": "the kept nodes' edges do not keep their order (descending action)",
}


class Tree:
    """A search tree with the root statistics the device keeps next to it (GameState root_N / root_W / root_w_is_py)."""

    def __init__(self, root, n=0, w_py=0.0, is_py=True, wf=f32(0.0), kept=False):
        self.root, self.n, self.w_py, self.is_py, self.wf, self.kept = root, n, w_py, is_py, wf, kept

    @property
    def w(self):
        return self.w_py if self.is_py else float(self.wf)


def _reverse_edges(node):
    node.edges.reverse()
    for e in node.edges:
        if e.child is not None:
            _reverse_edges(e.child)


def advance(tree, action, mutant=None):
    """-> (the tree re-rooted at the child under `action`, or None when nothing is kept; kept_visits)"""
    assert mutant is None or mutant in MUTANTS
    if tree is None or action is None or action < 0:
        return None, 0
    e = next((e for e in tree.root.edges if e.action == action), None)
    if e is None or e.child is None:
        return None, 0
    ch = e.child
    if ch.terminal and mutant != "keep_terminal":
        return None, 0
    if not ch.terminal and not ch.edges:
        return None, 0
    n = sum(x.N for x in ch.edges) if mutant == "root_sum" else e.N
    if mutant == "edge_order":
        _reverse_edges(ch)
    return Tree(ch, n=n, is_py=False, wf=f32(e.W), kept=True), n


def search(root_or_board, player, budget, pbits=10, vbits=11, noise=None, eps=0.25, cpuct=1.0, flags=0, trace=None,
           mutant=None, root_policy=None):
    """-> Result with counts int32 [A], child_w f32 [A], child_p f32 [A], root_visits, root_w, evals, the counters levels,
    children_scanned, children_created, terminal_revisits, nodes, needs (one bool per simulation run: did it take an evaluator
    row), kept (the search continued a kept tree) and tree (the Tree after the search, for advance()).  trace: optional list;
    every simulation that takes a row appends its board int8 [R, C].  root_policy: the row handed to the root expansion in
    place of the evaluator's (what yy_mcts_expand_root is given); a kept root does not read it."""
    assert mutant is None or mutant in MUTANTS
    evaluator = lambda b: hash_eval_batch(b, pbits, vbits)
    cpuct = f32(cpuct)
    created = 0
    if isinstance(root_or_board, Tree):
        tree = root_or_board
        root = tree.root
        assert root.player == int(player)
        pol = evaluator(root.board[None])[0][0] if root_policy is None else np.asarray(root_policy, np.float32)
        if noise is not None and any(float(noise[e.action]) != 0.0 for e in root.edges):
            keep = f32(1.0 - eps)
            for e in root.edges:
                p = f32(pol[e.action]) if mutant == "noise_policy" else e.P
                e.P = f32(float(f32(keep * p)) + eps * float(noise[e.action]))
        goal = tree.n + budget if mutant == "budget_additional" else budget
    else:
        board = np.array(root_or_board, np.int8)
        root = Node(board, int(player))
        pol = evaluator(board[None])[0][0] if root_policy is None else np.asarray(root_policy, np.float32)
        created = _expand(root, pol, flags, noise, eps)           # root call, value discarded (mcts.py:295)
        tree = Tree(root)
        goal = budget
    A = root.board.size
    kept = tree.kept
    evals = levels = scanned = revisits = nodes = 0
    needs = []
    while tree.n < goal:
        node, path, parent = root, [], None
        while True:
            if node.terminal:
                kind = TERMINAL
                break
            if not node.edges:
                kind = ROOTPASS if node is root else REEXPAND
                break
            e = _select(node, {}, cpuct)
            levels += 1
            scanned += len(node.edges)
            path.append(e)
            parent = node
            if e.child is None:
                kind = EXPAND
                break
            node = e.child
        needs.append(kind != TERMINAL)
        if kind == TERMINAL:
            v, v_is_py = node.tv, True
            revisits += 1
        else:
            if kind == EXPAND:
                b = parent.board.copy()
                b.flat[path[-1].action] = parent.player           # a legal move of the parent always places (copied boards)
                child = Node(b, -parent.player)
                path[-1].child = child
                node = child
                nodes += 1
            P, V = evaluator(node.board[None])
            evals += 1
            if trace is not None:
                trace.append(node.board.copy())
            created += _expand(node, P[0], flags)
            v, v_is_py = f32(V[0]), False
        depth = len(path)
        v32 = f32(v)
        for i, e in enumerate(path):
            sv = -v32 if (depth - (i + 1)) & 1 else v32
            e.N += 1
            e.W = f32(e.W + sv)
        tree.n += 1
        if tree.is_py and v_is_py and depth == 0:
            tree.w_py += v
        else:
            sv = -v32 if depth & 1 else v32
            base = f32(tree.w_py) if tree.is_py else tree.wf
            tree.wf = f32(base + sv)
            tree.is_py = False
    r = Result()
    r.counts = np.zeros(A, np.int32)
    r.child_w = np.zeros(A, np.float32)
    r.child_p = np.zeros(A, np.float32)
    for e in root.edges:
        r.counts[e.action], r.child_w[e.action], r.child_p[e.action] = e.N, e.W, e.P
    r.root_visits, r.root_w = tree.n, tree.w
    r.evals, r.levels, r.children_scanned, r.children_created = evals, levels, scanned, created
    r.terminal_revisits, r.nodes, r.needs, r.kept, r.tree = revisits, nodes, needs, kept, tree
    return r
