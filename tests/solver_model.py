"""Plain-numpy restatement of the MCTS solver (include/yy_engine.h YY_FLAG_SOLVER).

TEST INFRASTRUCTURE.  One game, copied boards, one descent per step: the search of tests/tree_model.py with solver=True, which
asks status() and propagate() below, and the exact hash evaluator with its priors times PSCALE.

  search(root_or_board, player, budget, solver, r, r_root, forced)
        fpu_model.search at K = 1 on copied boards, from a board or a kept Tree, with the proofs.  solver=False: that search,
        observable for observable (tests/test_solver_model.py).
  status(tree, node)   0 none, WIN, LOSS or DRAW for the node's side to move: a terminal node's is the class of its terminal
                       value; every other node's is kept in tree.proven, {id(node): (node, status)} -- Node has __slots__, and
                       the entry keeps the node alive, so that no id is ever met twice.  advance_proven() carries it to the
                       re-rooted Tree as the device carries the flags with the node records.

The rules: a node without children (the mover has no move, the game is not over) is never proven.  After the backup of a
descent that ended on a terminal node (a revisit, or the expansion that found it terminal) or on a proven node, the path is
walked upwards from the leaf's parent: a node becomes WIN if a child that exists is LOSS, else -- all children exist and are
proven -- DRAW if one is DRAW, else LOSS; the walk stops at the first node whose status does not change.  A proven node below
the root ends a descent: no evaluator row, its exact value (1, -1, 1e-4: python numbers, like a terminal value) is backed up.
The root is never treated as terminal.  Statistics are not rewritten.

`mutant=` (MUTANTS) breaks one rule on purpose; tests/test_solver_model.py asserts that the fixtures of the GPU tests (CASES
below, tests/test_gpu_solver.py) tell each from the true model."""
import functools

import numpy as np

import fpu_model as F
import oracle_lib as O
import tree_model
from forced_playouts_model import PSCALE, distribution, prune
from tree_model import PROVEN, advance  # noqa: F401  (PROVEN: the kind of a descent that ended on a proven node)

NONE, WIN, LOSS, DRAW = 0, 1, 2, 3
VALUE = {WIN: 1, LOSS: -1, DRAW: 0.0001}                           # python numbers, as Node.tv

MUTANTS = {
    "loss_partial": "LOSS (or DRAW) without all children: children that do not exist yet are not waited for",
    "draw_ignored": "DRAW ignored: a node all of whose children are proven and none LOSS is a LOSS even when one is a DRAW",
    "root_terminal": "the root is treated as terminal: a descent ends on a proven root",
    "stop_early": "propagation stops one level early: the walk never reaches the root",
}


def value_class(tv):
    return WIN if tv == 1 else LOSS if tv == -1 else DRAW


def status(tree, node):
    if node.terminal:
        return value_class(node.tv)
    hit = tree.proven.get(id(node))
    return hit[1] if hit else NONE


def advance_proven(tree, action):
    """tree_reuse_model.advance with the statuses carried along -> (Tree or None, kept_visits)"""
    new, kept = advance(tree, action)
    if new is not None:
        new.proven = getattr(tree, "proven", {})
    return new, kept


def propagate(tree, nodes, mutant=None):
    """nodes: the nodes of the path, root first, leaf's parent last -> (nodes proven, 1 if the root became proven)"""
    proven = root = 0
    top = 1 if mutant == "stop_early" else 0
    for lvl in range(len(nodes) - 1, top - 1, -1):
        n = nodes[lvl]
        if not n.edges or status(tree, n) != NONE:
            break
        st = [status(tree, e.child) if e.child is not None else None for e in n.edges]
        if mutant == "loss_partial":
            st = [s for s in st if s is not None]
        if LOSS in st:
            s = WIN
        elif None in st or NONE in st:
            s = NONE
        elif DRAW in st and mutant != "draw_ignored":
            s = DRAW
        else:
            s = LOSS
        if s == NONE:
            break
        tree.proven[id(n)] = (n, s)
        tree.log.append((n, s, len(n.edges)))
        proven += 1
        root += n is tree.root
    return proven, root


def search(root_or_board, player, budget, solver=True, pbits=10, vbits=11, mutant=None, pscale=PSCALE, **options):
    """tree_model.search at K = 1 with the proofs -> Result; r, r_root, forced: its keywords."""
    assert mutant is None or mutant in MUTANTS
    return tree_model.search(root_or_board, player, budget, 1, pbits, vbits, solver=solver, pscale=pscale,
                             mutant=mutant and "solver." + mutant, **options)


def root_policy(res, forced=0.0, tzero=False):
    """The distribution of the root's children (mcts.py:183-215) for T == 1 or T == 0, float64 [A]; with forced playouts on
    the pruned counts (forced_playouts_model.prune)."""
    counts = np.zeros(res.counts.size, np.int64)
    edges = res.tree.root.edges
    for e, n in zip(edges, prune(edges, forced)):
        counts[e.action] = n
    return distribution(counts, tzero)


def winning_move(res):
    """The arena's rule: the most visited root child that is proven LOSS for its mover, the lowest action among ties; -1: none"""
    wins = np.flatnonzero(res.child_proven == LOSS)
    if not len(wins):
        return -1
    return int(wins[np.argmax(res.counts[wins])])


def late_root(rows, cols, back, seed):
    """A position `back` moves before the end of a random game played to its end under the real rules -- a side without a move
    passes -- so that terminal positions are within reach of a short search; side to move, which has a move."""
    rng = np.random.default_rng(seed)
    board, player = np.zeros((1, rows, cols), np.int8), np.ones(1, np.int8)
    seen = []
    while float(O.game_ended(board, player)[0]) == 0.0:
        m = O.valid_mask(board, player)[0]
        if not m.any():
            player = -player
            continue
        seen.append((board[0].copy(), int(player[0])))
        board, player, _ = O.next_state(board, player, np.array([rng.choice(np.flatnonzero(m))], np.int32))
    return seen[max(0, len(seen) - back)]


# ------------------------------------------------------------------------------------------------ the fixtures of the GPU tests
# GAMES games per case; game g starts plies(g) random plies into a game (fpu_model.random_root), or, plies(g) < 0, that many
# moves before the end of a random game (late_root).  A case is searched over `moves`
# moves: after each, every game whose tree advance() keeps under the most visited move -- and whose game goes on -- searches on.
# budgets: one simulation budget per game in place of `sims` (yy_mcts_set_sim_budgets).
GAMES = 8
#         name            rows cols sims  plies of game g       keywords of search()  eps moves budgets            seed
CASES = {
    "3x3":         (3, 3, 64, lambda g: 4 + g % 4,    dict(), 0.0, 1, None, 100),
    "2x2":         (2, 2, 64, lambda g: g % 3,        dict(), 0.0, 1, None, 101),
    "2x4":         (2, 4, 64, lambda g: 2 + g % 3,    dict(), 0.0, 1, None, 301),
    "4x4":         (4, 4, 48, lambda g: 6 + g % 5,    dict(), 0.0, 1, None, 102),
    "1x6":         (1, 6, 16, lambda g: g,            dict(), 0.0, 1, None, 103),
    "7x1":         (7, 1, 16, lambda g: g,            dict(), 0.0, 1, None, 104),
    "5x7":         (5, 7, 32, lambda g: -3 - g % 4,   dict(), 0.0, 1, None, 105),
    "9x12":        (9, 12, 16, lambda g: -1 - g % 3,  dict(), 0.0, 1, None, 204),
    "4x4-noise":   (4, 4, 48, lambda g: 6 + g % 5,    dict(), 0.25, 1, None, 107),
    "4x4-fpu":     (4, 4, 48, lambda g: 6 + g % 5,    dict(r=0.2), 0.0, 1, None, 108),
    "4x4-forced":  (4, 4, 48, lambda g: 6 + g % 5,    dict(forced=2.0), 0.25, 1, None, 109),
    "4x4-budgets": (4, 4, 16, lambda g: 6 + g % 5,    dict(), 0.0, 1, (4, 16, 4, 16, 16, 4, 16, 4), 110),
    "4x4-reuse":   (4, 4, 48, lambda g: 4 + g % 5,    dict(), 0.25, 3, None, 111),
    "3x3-reuse":   (3, 3, 24, lambda g: g % 3,        dict(), 0.0, 3, None, 112),
}


class Move:
    """One move of a case: what the device test feeds in (boards, players, active, noise, budgets; actions: the move every
    game's tree was advanced by BEFORE this search, -1 at the first) and the model's Result per game (None: the game sat out)."""


@functools.lru_cache(maxsize=None)
def fixture(name, mutant=None, solver=True):
    """-> list of Move, one per move of case `name`.  solver=False: the same case searched without the option."""
    rows, cols, sims, plies, kw, eps, moves, budgets, seed = CASES[name]
    roots = [F.random_root(rows, cols, plies(g), [seed, g]) if plies(g) >= 0 else late_root(rows, cols, -plies(g), [seed, g])
             for g in range(GAMES)]
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
        m.budgets = np.array(budgets if budgets else [sims] * GAMES, np.int32)
        m.results = [None] * GAMES
        actions = np.full(GAMES, -1, np.int32)
        for g in range(GAMES):
            if not alive[g]:
                continue
            if eps:
                m.noise[g] = F.dirichlet_noise(boards[g], players[g], [seed, g, t])
            res = search(trees[g] if trees[g] is not None else boards[g], players[g], int(m.budgets[g]), solver=solver,
                         noise=m.noise[g] if eps else None, eps=eps, mutant=mutant, **kw)
            m.results[g] = res
            a = int(np.argmax(res.counts))
            alive[g] = False
            if t + 1 < moves and res.counts[a] > 0 and not res.failed:
                tree, kept = advance_proven(res.tree, a)
                b = boards[g].copy()
                b.flat[a] = players[g]
                if tree is not None and kept < sims and float(O.game_ended(b[None], [-players[g]])[0]) == 0.0:
                    trees[g], boards[g], players[g], actions[g], alive[g] = tree, b, -players[g], a, True
        out.append(m)
    return out


def observables(moves):
    """What a device run is compared on, as one nested tuple (for telling a mutant from the true model)."""
    return tuple((r.counts.tobytes(), r.child_w.tobytes(), r.child_p.tobytes(), r.root_visits, r.root_w, r.root_proven,
                  r.child_proven.tobytes(), r.proven_nodes, r.proven_descents, r.proven_roots)
                 for m in moves for r in m.results if r is not None)
