"""The multi-move cases of tests/test_gpu_tree_reuse.py and their replay on tests/tree_reuse_model.py (TEST INFRASTRUCTURE).

A case is a batch of G games on one board size and a plan: one entry per ply saying, game by game, which child of the searched
root the tree is advanced by ("choice"), the budgets, the active flags, whether the root gets noise and whether the ply advances
twice (own move, then the reply).  replay() plays the plan on the model, one game at a time, and returns per ply everything
the device test feeds in (boards, players, active, budgets, noise, the actions of the advances) and everything it compares
(root statistics, the per-simulation needs_eval flags, the evaluated positions, counters, kept visits).  The CPU test checks on
these records that the cases exercise kept trees and fallbacks at all, and that every mutant of the model shows on them.

Choices:  best = the most visited child (lowest action on ties); once = a child visited exactly once; unvisited = a child never
visited (nothing kept); none = action -1; oob = an action beyond the board; terminal = a visited child that ended the game (not
kept); swap = advance by the best child but PLAY another move, so that the next begin sees a board the kept tree was not built
for.  A choice that the root does not offer falls back to best; a root without children advances by -1 and the game idles from
then on (active = 0)."""
import functools

import numpy as np

import oracle_lib as O
import tree_reuse_model as T
from tree_model import dirichlet_noise, random_root

KINDS8 = ("best", "best", "best", "once", "unvisited", "none", "oob", "terminal")


def _plan(G, sims, long=False):
    """The per-board plan: one advance of every kind then budget = kept visits (nothing selected), a top-up with the scalar
    budget and noise on the kept roots, a double advance, a top-up with a foreign policy row at the root."""
    k = [KINDS8[g % 8] for g in range(G)]
    plan = [dict(choice=k, budget="sims", noise=True),
            dict(choice=["best"] * G, budget="kept"),
            dict(choice=["best"] * G, budget="sims", noise=True, bad_policy=True, double=True),
            dict(choice=["best"] * G, budget="sims"),
            dict(choice=["best"] * G, budget="sims", bad_policy=True)]
    if long:        # six to ten plies, games going different ways, inactive games, small budgets, forced fresh roots
        kinds = ("best", "once", "best", "swap", "best", "none", "best", "best")
        plan = []
        for t in range(8):
            plan.append(dict(choice=[kinds[(g + t) % 8] for g in range(G)],
                             budget=[(2 if (g + t) % 4 == 1 else sims - (g % 3)) for g in range(G)] if t % 2 else "sims",
                             active=[0 if (g + 2 * t) % 7 == 3 else 1 for g in range(G)], noise=(t in (0, 3)),
                             double=(t == 5)))
    return plan


#        name      R   C  sims G  opening plies, seed, pbits
CASES = {
    "3x3": (3, 3, 40, 8, 1, 11, 10),
    "4x4": (4, 4, 60, 8, 3, 12, 2),
    "1x6": (1, 6, 40, 8, 0, 13, 10),
    "7x1": (7, 1, 40, 8, 1, 14, 10),
    "5x7": (5, 7, 100, 8, 6, 15, 10),
    "2x9": (2, 9, 60, 8, 3, 16, 2),
    "9x12": (9, 12, 48, 8, 20, 17, 10),
    "12x16": (12, 16, 40, 8, 30, 18, 10),
    "4x4-long": (4, 4, 48, 8, 2, 19, 10),
    "5x5-long": (5, 5, 64, 8, 4, 20, 2),
}
VB = 11


class Ply:
    pass


def _pick(kind, res, tree, A):
    """-> (the action the tree is advanced by, the action played or None)"""
    edges = tree.root.edges
    if not edges:
        return -1, None
    best = int(np.argmax(res.counts))
    if kind == "none":
        return -1, None
    if kind == "oob":
        return A + 5, None
    if kind == "once":
        a = next((e.action for e in edges if e.N == 1 and e.child is not None and not e.child.terminal and e.child.edges), best)
        return a, a
    if kind == "unvisited":
        a = next((e.action for e in edges if e.N == 0), best)
        return a, a
    if kind == "terminal":
        a = next((e.action for e in edges if e.child is not None and e.child.terminal), best)
        return a, a
    if kind == "swap":
        other = next((e.action for e in sorted(edges, key=lambda e: -e.N) if e.action != best), best)
        return best, other
    return best, best


def _snapshot(tree, A):
    """-> (counts, child_w, child_p, root visits, root value sum) of the root of `tree` as root_counts / root_stats report it"""
    counts, w, pr = np.zeros(A, np.int32), np.zeros(A, np.float32), np.zeros(A, np.float32)
    if tree is None:
        return counts, w, pr, 0, 0.0
    for e in tree.root.edges:
        counts[e.action], w[e.action], pr[e.action] = e.N, e.W, e.P
    return counts, w, pr, tree.n, tree.w


@functools.lru_cache(maxsize=None)
def replay(name, mutant=None):
    """-> list of Ply records (module docstring), one per ply of case `name`, played on the model (mutant: tree_reuse_model's)."""
    R, C, sims, G, opening, seed, pb = CASES[name]
    A = R * C
    plan = _plan(G, sims, long=name.endswith("-long"))
    roots = [random_root(R, C, opening + g % 3, seed * 131 + g) for g in range(G)]
    boards = [np.array(b, np.int8) for b, _ in roots]
    players = [int(p) for _, p in roots]
    trees = [None] * G
    keptv = [0] * G
    alive = [True] * G
    out = []
    for t, spec in enumerate(plan):
        p = Ply()
        p.boards, p.players = np.stack(boards), np.array(players, np.int8)
        p.active = np.array([int(alive[g] and (spec.get("active") or [1] * G)[g]) for g in range(G)], np.uint8)
        b = spec["budget"]
        if b == "sims":
            p.budgets, p.bound = None, sims
        else:
            p.budgets = np.array([(keptv[g] if keptv[g] > 0 else sims // 2) if b == "kept" else b[g] for g in range(G)], np.int64)
            p.bound = int(p.budgets.max())
        p.noise = np.zeros((G, A))
        if spec.get("noise"):
            for g in range(G):
                if g % 3 != 2:                                   # every third game draws nothing: an all-zero row
                    p.noise[g] = dirichlet_noise(boards[g], players[g], 100 * t + g)
        p.bad_policy = bool(spec.get("bad_policy"))
        p.double = bool(spec.get("double"))
        p.results, p.used_kept, p.kept_in = [None] * G, [False] * G, [0] * G
        p.actions, p.kept1 = np.full(G, -1, np.int32), np.zeros(G, np.int32)
        p.actions2, p.kept2 = np.full(G, -1, np.int32), np.zeros(G, np.int32)
        p.after = [_snapshot(None, A)] * G                        # the root the advances of this ply leave (an empty tree: zeros)
        for g in range(G):
            tree, trees[g] = trees[g], None                       # begin consumes the mark whatever follows
            kin, keptv[g] = keptv[g], 0
            if not p.active[g]:
                continue
            same = tree is not None and np.array_equal(tree.root.board, boards[g]) and tree.root.player == players[g]
            budget = sims if p.budgets is None else int(p.budgets[g])
            rp = None
            if p.bad_policy:                                      # the row the root expansion is handed: not this position's
                rp = np.roll(T.hash_eval_batch(boards[g][None], pb, VB)[0][0], 1)
            trace = []
            res = T.search(tree if same else boards[g], players[g], budget, pb, VB, noise=p.noise[g] if p.noise[g].any() else None,
                           trace=trace, mutant=mutant, root_policy=rp)
            res.trace = trace
            p.results[g], p.used_kept[g], p.kept_in[g] = res, same, (kin if same else 0)
            a, played = _pick(spec["choice"][g], res, res.tree, A)
            p.actions[g] = a
            new, kv = T.advance(res.tree, a if 0 <= a < A else -1, mutant=mutant)
            p.kept1[g] = kv
            if played is not None:
                nb, npl, _ = O.next_state(boards[g][None], [players[g]], np.array([played], np.int32))
                boards[g], players[g] = nb[0], int(npl[0])
            if p.double:
                a2 = -1
                if new is not None:
                    n2 = [e.N for e in new.root.edges]
                    if max(n2) > 0:
                        a2 = new.root.edges[int(np.argmax(n2))].action
                p.actions2[g] = a2
                new, kv = T.advance(new, a2, mutant=mutant)
                p.kept2[g] = kv
                if a2 >= 0:
                    nb, npl, _ = O.next_state(boards[g][None], [players[g]], np.array([a2], np.int32))
                    boards[g], players[g] = nb[0], int(npl[0])
            trees[g], keptv[g] = new, kv
            p.after[g] = _snapshot(new, A)
            ended = O.game_ended(boards[g][None], [players[g]])[0] != 0
            if ended or not O.valid_mask(boards[g][None], [players[g]])[0].any() or not res.tree.root.edges:
                alive[g] = False
        out.append(p)
    return out


def observables(plies):
    """What a device run is compared on, as one nested tuple (for telling a mutant from the true model)."""
    obs = []
    for p in plies:
        for g, r in enumerate(p.results):
            if r is not None:
                obs.append((r.counts.tobytes(), r.child_w.tobytes(), r.child_p.tobytes(), r.root_visits, r.root_w, tuple(r.needs)))
        obs.append((p.kept1.tobytes(), p.kept2.tobytes(), p.actions.tobytes()))
    return tuple(obs)
