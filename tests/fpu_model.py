"""Plain-numpy restatement of the first-play urgency reduction (include/yy_engine.h YY_FLAG_FPU_REDUCTION).

TEST INFRASTRUCTURE.  One game, on the Node / Edge / _expand / _select of leaf_parallel_model.py, the Tree and advance() of
tree_reuse_model.py, the forcing test of forced_playouts_model.py and the exact hash evaluator of hash_eval.py (its priors
times PSCALE, as in forced_playouts_model: sqrt(SP) is then not negligible next to the values).

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
from forced_playouts_model import PSCALE, is_forced
from hash_eval import hash_eval_batch
from leaf_parallel_model import EXPAND, REEXPAND, ROOTPASS, TERMINAL, Node, Result, _expand, _select
from tree_reuse_model import Tree, advance

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


def search(root_or_board, player, budget, r=0.0, r_root=None, K=1, forced=0.0, aliased=False, pbits=10, vbits=11, noise=None,
           eps=0.25, cpuct=1.0, flags=0, mutant=None, pscale=PSCALE):
    """-> Result with counts int32 [A], child_w f32 [A], child_p f32 [A], root_visits, root_w, evals, tree (the Tree after
    the search, for advance()), final_board (aliased: the one board after the search) and failed (a descent found no
    selectable child: the game stopped there, as on the device)."""
    assert mutant is None or mutant in MUTANTS
    assert K == 1 or not (forced or aliased or isinstance(root_or_board, Tree))
    assert not (aliased and (forced or isinstance(root_or_board, Tree)))
    r = float(r)
    r_root = r if r_root is None else float(r_root)
    if mutant == "r_everywhere":
        r_root = r

    def evaluator(b):
        pol, val = hash_eval_batch(b, pbits, vbits)
        return pol * f32(pscale), val

    cpuct = f32(cpuct)
    raw = {}
    if isinstance(root_or_board, Tree):
        tree = root_or_board
        root = tree.root
        assert root.player == int(player)
        if noise is not None and any(float(noise[e.action]) != 0.0 for e in root.edges):
            raw = {id(e): e.P for e in root.edges}
            keep = f32(1.0 - eps)
            for e in root.edges:
                e.P = f32(float(f32(keep * e.P)) + eps * float(noise[e.action]))
    else:
        board = np.array(root_or_board, np.int8)
        root = Node(board, int(player))
        pol = evaluator(board[None])[0][0]
        _expand(root, pol, flags, noise, eps)                      # root call, value discarded (mcts.py:295)
        if noise is not None and any(float(noise[e.action]) != 0.0 for e in root.edges):
            raw = {id(e): f32(pol[e.action]) for e in root.edges}
        tree = Tree(root)
    shared = root.board.copy()                                     # aliased: the one board of the search
    A = root.board.size
    evals = 0
    failed = False

    def choose(node, vc):
        if forced and node is root:
            S = sum(e.N for e in root.edges)
            owed = [x for x in root.edges if is_forced(forced, x.P, x.N, S)]
            if owed:
                return owed[0]
        if not r:
            return _select(node, vc, cpuct)
        return select(node, vc, cpuct, r_root if node is root else r, mutant, raw if node is root else None)

    while tree.n < budget and not failed:
        keff = min(K, budget - tree.n)
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
                e = choose(node, vc)
                if e is None:
                    failed = True
                    break
                path.append(e)
                parent = node
                if e.child is None:
                    kind = EXPAND
                    break
                node = e.child
            if failed:
                break
            for e in path:
                vc[id(e)] = vc.get(id(e), 0) + 1
            key = id(path[-1]) if kind == EXPAND else id(node)
            dup = first_of.setdefault(key, j) if kind != TERMINAL else j
            desc.append(dict(kind=kind, path=path, node=node, parent=parent, dup=dup if dup != j else -1))
        if failed:
            break
        for d in desc:
            d["need"] = d["kind"] != TERMINAL and d["dup"] < 0
            if not d["need"]:
                continue
            if aliased:                                            # the shared board: place the move iff it is legal on it now
                if d["kind"] != ROOTPASS:
                    par, e = d["parent"], d["path"][-1]
                    if O.valid_mask(shared[None], [par.player], flags)[0][e.action]:
                        shared.flat[e.action] = par.player
                    d["player"] = -par.player
                else:
                    d["player"] = root.player
                d["board"] = shared.copy()
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
                    d["node"].board = d["board"]                   # aliased: the node is expanded on the board as it is now
                    _expand(d["node"], d["policy"], flags)
            depth = len(d["path"])
            v32 = f32(v)
            for i, e in enumerate(d["path"]):
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
    res = Result()
    res.counts = np.zeros(A, np.int32)
    res.child_w = np.zeros(A, np.float32)
    res.child_p = np.zeros(A, np.float32)
    for e in root.edges:
        res.counts[e.action], res.child_w[e.action], res.child_p[e.action] = e.N, e.W, e.P
    res.root_visits, res.root_w, res.evals, res.tree, res.final_board, res.failed = tree.n, tree.w, evals, tree, shared, failed
    return res


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


def random_root(rows, cols, plies, seed):
    """A position after `plies` random legal moves from the empty board (fewer when the game ends first), side to move."""
    rng = np.random.default_rng(seed)
    board, player = np.zeros((1, rows, cols), np.int8), np.ones(1, np.int8)
    for _ in range(plies):
        m = O.valid_mask(board, player)[0]
        if not m.any() or O.game_ended(board, player)[0] != 0:
            break
        board, player, _ = O.next_state(board, player, np.array([rng.choice(np.flatnonzero(m))], np.int32))
    return board[0], int(player[0])


def dirichlet_noise(board, player, seed, alpha=0.3):
    legal = np.flatnonzero(O.valid_mask(board[None], [player])[0])
    nz = np.zeros(board.size)
    if len(legal):
        nz[legal] = np.random.default_rng(seed).dirichlet([alpha] * len(legal))
    return nz


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
