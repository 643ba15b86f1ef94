"""The one plain-numpy float32 tree search that every option model restates its rule on (TEST INFRASTRUCTURE).

One game, the rules of the CPU oracle (oracle_lib) and the exact hash evaluator of hash_eval.py.  Search is the search sequence
of include/yy_engine.h, stated once: a step runs K_eff = min(K, budget - root visits) descents on the tree as it stands
(selection phase; descent j sees the virtual counts of descents 0 .. j-1, leaf_parallel_model.py), asks the evaluator for one
row per leaf that needs one, and then, in descent order, expands the leaves and backs the values up.  What an option changes
is a keyword, and the option's own arithmetic stays in its own file, imported where the loop calls it:

  K                      descents per step (leaf_parallel_model.py: virtual visits, duplicates, the device counters)
  a Tree for a board     the search tops a kept root up to its budget (tree_reuse_model.py; advance() re-roots)
  forced                 forced playouts at the root (forced_playouts_model.py: is_forced)
  r, r_root              first-play urgency reduction (fpu_model.py: select)
  aliased                one board that every expansion plays its move on (fpu_model.py)
  solver                 proven nodes end a descent, proofs walk up the path (solver_model.py: status, propagate)
  m, c_visit, c_scale    the Gumbel root rule on base scores s0 set from outside (gumbel_model.py: select_root)

The model is no wider than the device: forced, solver, Gumbel, a kept Tree or the aliased board at K > 1, the aliased board
with any of them, and Gumbel with forced, solver or a kept Tree are refused.

mutant: "<owner>.<name>", a key of <owner>_model.MUTANTS -- one deliberately broken rule.  The ones that break the sequence
itself are single branches below, each commented with its owner; the others are handed to their owner's rule functions."""
import importlib
import math
from types import SimpleNamespace

import numpy as np

import oracle_lib as O
from hash_eval import hash_eval_batch

f32 = np.float32
TERMINAL, EXPAND, REEXPAND, ROOTPASS = "terminal", "expand", "reexpand", "rootpass"
PROVEN = 8                                                         # the kind of a descent that ended on a proven node


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


class Tree:
    """A search tree with the root statistics the device keeps next to it (GameState root_N / root_W / root_w_is_py), and the
    solver's proofs: proven {id(node): (node, status)} and log [(node, status, children)] of every node proven by propagation."""

    def __init__(self, root, n=0, w_py=0.0, is_py=True, wf=f32(0.0), kept=False):
        self.root, self.n, self.w_py, self.is_py, self.wf, self.kept = root, n, w_py, is_py, wf, kept
        self.proven, self.log = {}, []

    @property
    def w(self):
        return self.w_py if self.is_py else float(self.wf)


def _reverse_edges(node):
    node.edges.reverse()
    for e in node.edges:
        if e.child is not None:
            _reverse_edges(e.child)


def advance(tree, action, mutant=None):
    """-> (the tree re-rooted at the child under `action`, or None when nothing is kept; kept_visits).  mutant: a name of
    tree_reuse_model.MUTANTS (root_sum, keep_terminal, edge_order are broken here)."""
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


def random_root(R, C, plies, seed, flags=0):
    """A position after `plies` random legal moves from the empty board (fewer when the game ends first), side to move."""
    rng = np.random.default_rng(seed)
    board, player = np.zeros((1, R, C), np.int8), np.ones(1, np.int8)
    for _ in range(plies):
        m = O.valid_mask(board, player, flags)[0]
        if not m.any() or O.game_ended(board, player, flags)[0] != 0:
            break
        board, player, _ = O.next_state(board, player, np.array([rng.choice(np.flatnonzero(m))], np.int32), flags)
    return board[0], int(player[0])


def dirichlet_noise(board, player, seed, alpha=0.3, flags=0):
    legal = np.flatnonzero(O.valid_mask(board[None], [player], flags)[0])
    nz = np.zeros(board.size)
    if len(legal):
        nz[legal] = np.random.default_rng(seed).dirichlet([alpha] * len(legal))
    return nz


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
    """Plain PUCT over n = N + v, w = W - v.  mutant: a name of leaf_parallel_model.MUTANTS (keep_w, s_parent, tie_high and
    v_low64 are broken here)."""
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


class Search:
    """The search of one game, step by step.  root_or_board: a board (the root call is made and the root expanded, with
    root_policy in place of the evaluator's row when given, zero_prior an action whose root prior is set to exactly 0) or a
    kept Tree (the root call's row is ignored; a noise row that is non-zero over the root's moves is mixed into the STORED
    priors).  evaluator(boards int8 [n, R, C]) -> (policy f32 [n, A], value f32 [n]) replaces the hash evaluator with its
    priors times pscale.  trace: optional list; every step appends one Descent per descent.  s0: the Gumbel base scores of
    the root's edges, set from outside (gumbel_model.py)."""

    def __init__(self, root_or_board, player, budget, K=1, pbits=10, vbits=11, noise=None, eps=0.25, cpuct=1.0, flags=0,
                 trace=None, mutant=None, evaluator=None, pscale=1.0, aliased=False, forced=0.0, r=0.0, r_root=None,
                 solver=False, m=0, c_visit=50.0, c_scale=1.0, root_policy=None, zero_prior=None):
        kept = isinstance(root_or_board, Tree)
        assert K == 1 or not (forced or solver or m or aliased or kept)      # what the device refuses
        assert not (aliased and (forced or solver or m or kept))
        assert not (m and (forced or solver or kept))
        owner, _, name = (mutant or ".").partition(".")
        assert mutant is None or name in importlib.import_module(owner + "_model").MUTANTS, mutant
        self.mutant, self._owner, self._name = mutant, owner, name
        if evaluator is None:
            def evaluator(b):
                pol, val = hash_eval_batch(b, pbits, vbits)
                return pol * f32(pscale), val
        self.evaluator, self.K, self.flags, self.trace, self.cpuct = evaluator, K, flags, trace, f32(cpuct)
        self.aliased, self.forced, self.solver = aliased, forced, solver
        self.r = float(r)
        self.r_root = self.r if r_root is None or mutant == "fpu.r_everywhere" else float(r_root)
        self.budget, self.m, self.cv, self.cs, self.s0 = int(budget), int(m), f32(c_visit), f32(c_scale), None
        self.created = 0
        if kept:
            self.tree, self.root = root_or_board, root_or_board.root
            assert self.root.player == int(player)
            self.raw = {id(e): e.P for e in self.root.edges}       # the priors from before the noise (the prior_raw mutants)
            if noise is not None and any(float(noise[e.action]) != 0.0 for e in self.root.edges):
                keep = f32(1.0 - eps)
                if mutant == "tree_reuse.noise_policy":            # tree_reuse: the root call's row, not the stored priors
                    pol = evaluator(self.root.board[None])[0][0] if root_policy is None else np.asarray(root_policy, np.float32)
                for e in self.root.edges:
                    p = f32(pol[e.action]) if mutant == "tree_reuse.noise_policy" else e.P
                    e.P = f32(float(f32(keep * p)) + eps * float(noise[e.action]))
        else:
            board = np.array(root_or_board, np.int8)
            self.root = Node(board, int(player))
            pol = evaluator(board[None])[0][0] if root_policy is None else np.asarray(root_policy, np.float32)
            if zero_prior is not None:
                pol = pol.copy()
                pol[zero_prior] = 0.0
            self.created = _expand(self.root, pol, flags, noise, eps)        # root call, value discarded (mcts.py:295)
            self.raw = {id(e): f32(pol[e.action]) for e in self.root.edges}
            self.tree = Tree(self.root)
        # tree_reuse: budget_additional counts the simulations of this call, not the root's visits
        self.goal = self.tree.n + self.budget if mutant == "tree_reuse.budget_additional" else self.budget
        self.A = self.root.board.size
        self.kept = self.tree.kept
        self.shared = self.root.board.copy()                       # aliased: the one board of the search
        self.failed = False
        self.ended = []                                            # the kind of every descent
        self.evals = self.steps = self.levels = self.scanned = self.revisits = self.nodes = self.duplicates = 0
        self.forced_descents = self.proven_nodes = self.proven_descents = self.proven_roots = 0

    def own(self, owner):
        """the mutant's name for the rule functions of `owner`_model, None for everybody else's"""
        return self._name if self._owner == owner else None

    @property
    def sims(self):
        return self.tree.n

    def choose(self, node, vc, s_parent):
        """-> the edge a descent takes out of `node`, or None when no child is selectable (NaN scores)"""
        import forced_playouts_model as FP
        import fpu_model as F
        import gumbel_model as G
        at_root, edges = node is self.root, node.edges
        if self.m and at_root:
            return G.select_root(edges, self.s0, self.budget, self.m, self.cv, self.cs)
        if self.forced and at_root:
            fm = self.own("forced_playouts")
            S = self.tree.n if fm == "s_root_n" else sum(e.N for e in edges)             # forced_playouts: s_root_n
            owed = [x for x in edges if FP.is_forced(self.forced, self.raw[id(x)] if fm == "prior_raw" else x.P, x.N, S, fm)]
            if owed:
                self.forced_descents += 1
                return owed[-1] if fm == "forced_high" else owed[0]   # ascending action; forced_playouts: forced_high
        if not self.r:
            return _select(node, vc, self.cpuct, self.own("leaf_parallel"), s_parent)
        return F.select(node, vc, self.cpuct, self.r_root if at_root else self.r, self.own("fpu"), self.raw if at_root else None)

    def step(self):
        """One step of K_eff descents; False once the budget is spent or the game failed (a descent found no selectable
        child: the game stops there, as on the device)."""
        import solver_model as S
        tree, root, mutant, flags = self.tree, self.root, self.mutant, self.flags
        if tree.n >= self.goal or self.failed:
            return False
        keff = self.K if mutant == "leaf_parallel.full_last" else min(self.K, self.goal - tree.n)    # leaf_parallel: full_last
        self.steps += 1
        vc, desc, first_of = {}, [], {}
        for j in range(keff):                                      # selection phase: the tree does not change
            node, path, nodes, s_parent = root, [], [], tree.n     # leaf_parallel: s_parent reads N(node) - 1 for S
            while True:
                if node.terminal:
                    kind = TERMINAL
                    break
                if self.solver and S.status(tree, node) != S.NONE and (node is not root or mutant == "solver.root_terminal"):
                    kind = PROVEN                                  # solver: root_terminal ends a descent on a proven root
                    break
                if not node.edges:
                    kind = ROOTPASS if node is root else REEXPAND
                    break
                e = self.choose(node, vc, s_parent)
                if e is None:
                    self.failed = True
                    return False
                self.levels += 1
                self.scanned += len(node.edges)
                path.append(e)
                nodes.append(node)
                s_parent = e.N - 1
                if e.child is None:
                    kind = EXPAND
                    break
                node = e.child
            for e in path:
                vc[id(e)] = vc.get(id(e), 0) + 1
            key = id(path[-1]) if kind == EXPAND else id(node)
            dup = first_of.setdefault(key, j) if kind not in (TERMINAL, PROVEN) else j
            desc.append(SimpleNamespace(kind=kind, path=path, nodes=nodes, node=node, dup=dup if dup != j else -1))
        for d in desc:                                             # the evaluator rows
            d.need = d.kind not in (TERMINAL, PROVEN) and (d.dup < 0 or mutant == "leaf_parallel.dup_row")   # leaf_parallel: dup_row
            d.board = d.player = None
            if not d.need:
                continue
            if self.aliased:                                       # the shared board: place the move iff it is legal on it now
                if d.kind != ROOTPASS:
                    par, e = d.nodes[-1], d.path[-1]
                    if O.valid_mask(self.shared[None], [par.player], flags)[0][e.action]:
                        self.shared.flat[e.action] = par.player
                    d.player = -par.player
                else:
                    d.player = root.player
                d.board = self.shared.copy()
            elif d.kind == EXPAND:
                par, e = d.nodes[-1], d.path[-1]
                d.board = par.board.copy()
                d.board.flat[e.action] = par.player                # a legal move of the parent always places (copied boards)
                d.player = -par.player
            else:
                d.board, d.player = d.node.board, d.node.player
        rows = [d for d in desc if d.need]
        if rows:
            P, V = self.evaluator(np.stack([d.board for d in rows]))
            for i, d in enumerate(rows):
                d.policy, d.value = P[i], f32(V[i])
        self.evals += len(rows)
        self.revisits += sum(d.kind == TERMINAL for d in desc)
        self.proven_descents += sum(d.kind == PROVEN for d in desc)
        self.duplicates += sum(d.dup >= 0 for d in desc)
        self.ended += [d.kind for d in desc]
        if self.trace is not None:
            self.trace.append([Descent(d.kind, [e.action for e in d.path], d.dup, d.need, d.board, d.player) for d in desc])
        # expansion + backup phase, in descent order (leaf_parallel: reverse_backup)
        for d in (reversed(desc) if mutant == "leaf_parallel.reverse_backup" else desc):
            exact = d.kind in (TERMINAL, PROVEN)                   # solver: the leaf's value is a game value
            if d.kind == TERMINAL:
                v, v_is_py = d.node.tv, mutant != "leaf_parallel.terminal_f32"           # leaf_parallel: terminal_f32
            elif d.kind == PROVEN:
                v, v_is_py = S.VALUE[S.status(tree, d.node)], True
            elif d.dup >= 0:
                v, v_is_py = desc[d.dup].value, False
            else:
                v, v_is_py = d.value, False
                if d.kind == EXPAND:
                    d.node = d.path[-1].child = Node(d.board, d.player)
                    self.nodes += 1
                else:
                    d.node.board = d.board                         # aliased: the node is expanded on the board as it is now
                self.created += _expand(d.node, d.policy, flags)
                exact = d.kind == EXPAND and d.node.terminal
            depth = len(d.path)
            v32 = f32(v)
            for i, e in enumerate(d.path):
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
            if self.solver and exact:
                a, b = S.propagate(tree, d.nodes, self.own("solver"))
                self.proven_nodes += a
                self.proven_roots += b
        return True

    def run(self):
        while self.step():
            pass
        return self

    def result(self):
        """-> Result: by action counts int32 [A], child_w f32 [A], child_p f32 [A], child_proven int8 [A] (0 where the child
        does not exist or the solver is off); root_visits, root_w, root_proven; of this Search evals, steps, the device counters
        levels, children_scanned, children_created, terminal_revisits, nodes (leaf_parallel_model.py), duplicates, forced
        (descents that took a forced edge), proven_nodes, proven_descents, proven_roots and ended (the kind of every descent);
        tree (for advance()), root, kept (the search continued a kept tree), final_board (aliased: the one board after the
        search) and failed."""
        import solver_model as S
        tree, root = self.tree, self.root
        r = Result()
        r.counts = np.zeros(self.A, np.int32)
        r.child_w = np.zeros(self.A, np.float32)
        r.child_p = np.zeros(self.A, np.float32)
        r.child_proven = np.zeros(self.A, np.int8)
        for e in root.edges:
            r.counts[e.action], r.child_w[e.action], r.child_p[e.action] = e.N, e.W, e.P
            if self.solver and e.child is not None:
                r.child_proven[e.action] = S.status(tree, e.child)
        r.root_visits, r.root_w, r.root_proven = tree.n, tree.w, S.status(tree, root) if self.solver else S.NONE
        r.evals, r.steps, r.levels, r.children_scanned, r.children_created = self.evals, self.steps, self.levels, self.scanned, self.created
        r.terminal_revisits, r.nodes, r.duplicates, r.forced = self.revisits, self.nodes, self.duplicates, self.forced_descents
        r.proven_nodes, r.proven_descents, r.proven_roots, r.ended = self.proven_nodes, self.proven_descents, self.proven_roots, self.ended
        r.tree, r.root, r.kept, r.final_board, r.failed = tree, root, self.kept, self.shared, self.failed
        return r


def search(root_or_board, player, budget, K=1, pbits=10, vbits=11, **options):
    """Search(...) run to its end -> Result"""
    return Search(root_or_board, player, budget, K, pbits, vbits, **options).run().result()
