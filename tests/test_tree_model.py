"""What only the one search of tests/tree_model.py can state and the device already does: the device counters of a search
with an option on, and the descents of an option model with its option off.  CPU only; 4x4 and 1x6, at most 32 simulations."""
import numpy as np
import pytest

import gumbel_model as G
import solver_model as S
import tree_model as M
from forced_playouts_model import PSCALE
from test_leaf_parallel_model import tree_recount

ROOTS = [(4, 4, 3, 32), (4, 4, 9, 32), (4, 4, 12, 24), (1, 6, 0, 16), (1, 6, 2, 16), (1, 6, 4, 16)]     # R, C, plies, sims


@pytest.mark.parametrize("kw", [dict(r=0.25), dict(r=0.25, r_root=0.0), dict(forced=2.0), dict(solver=True),
                                dict(solver=True, r=0.2, forced=2.0)], ids=str)
def test_counter_identities_with_an_option_on(kw):
    """test_leaf_parallel_model.test_counter_identities at K = 1.  A descent that ends on a proven node takes no row and is no
    terminal revisit (the device counts it as proven_descents alone), so it is the fourth term of the visit sum; it is 0
    without the solver."""
    fired = 0
    for (R, C, plies, sims) in ROOTS:
        for seed in range(3):
            board, player = M.random_root(R, C, plies, seed)
            trace = []
            r = M.search(board, player, sims, trace=trace, pscale=PSCALE, **kw)
            assert not r.failed and r.steps == sims
            levels, created, nodes = tree_recount(r.root)
            kinds = [d for step in trace for d in step]
            assert len(kinds) == sims and [d.kind for d in kinds] == r.ended
            assert r.levels == levels == sum(len(d.actions) for d in kinds)
            assert r.children_created == created                      # every node with children, the root included
            assert r.nodes == nodes                                   # the root is not counted
            assert r.terminal_revisits == sum(d.kind == M.TERMINAL for d in kinds)
            assert r.proven_descents == sum(d.kind == M.PROVEN for d in kinds)
            assert r.duplicates == sum(d.dup >= 0 for d in kinds) == 0
            assert r.evals + r.terminal_revisits + r.duplicates + r.proven_descents == r.root_visits == sims
            assert r.evals == sum(d.needs_eval for d in kinds)
            assert r.children_scanned >= r.levels and (r.levels == 0) == (r.children_scanned == 0)
            if not kw.get("solver"):
                assert r.proven_descents == r.proven_nodes == r.proven_roots == 0
            if not kw.get("forced"):
                assert r.forced == 0
            fired += r.forced if kw.get("forced") else r.proven_descents if kw.get("solver") else r.levels
    assert fired > 0                                                  # the option did something on these roots


def same_descents(a, b):
    assert len(a) == len(b) > 0
    for x, y in zip((d for step in a for d in step), (d for step in b for d in step)):
        assert tuple(x) == tuple(y) and x.needs_eval == y.needs_eval and x.player == y.player
        assert (x.board is None) == (y.board is None) and (x.board is None or np.array_equal(x.board, y.board))


@pytest.mark.parametrize("R,C,plies,sims", ROOTS)
def test_the_descents_of_an_option_off_are_the_plain_search(R, C, plies, sims):
    for seed in range(3):
        board, player = M.random_root(R, C, plies, seed)
        noise = M.dirichlet_noise(board, player, 50 + seed) if seed else None
        plain, off = [], []
        M.search(board, player, sims, noise=noise, trace=plain, pscale=PSCALE)
        r = S.search(board, player, sims, solver=False, noise=noise, trace=off)
        same_descents(off, plain)
        assert M.PROVEN not in r.ended and not r.tree.proven
        plain, off = [], []
        M.search(board, player, sims, noise=noise, trace=plain)
        s = G.Search(board, player, sims, 0, noise=noise, trace=off).run()      # m = 0: the root rule is off, no s0 is read
        same_descents(off, plain)
        assert s.s0 is None and s.sims == sims
