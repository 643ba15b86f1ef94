"""CPU checks of tests/tree_reuse_model.py and of the inputs of tests/test_gpu_tree_reuse.py (tests/tree_reuse_cases.py).

With no advance the model is the reference's search: equal to the C oracle (oracle_lib.search_hash) and to the K = 1
leaf-parallel model.  The GPU cases must exercise what they are for -- a test that only ever sees fresh roots proves nothing --
so for every case, replayed on the model: at least half of its searched moves continue a kept tree of at least 2 visits, and at
least one searched move after an advance falls back to a fresh root.  Every mutant of the model differs from the true model on
at least one case."""
import numpy as np
import pytest

import leaf_parallel_model as L
import oracle_lib as O
import tree_reuse_cases as Cs
import tree_reuse_model as T
from tree_model import dirichlet_noise, random_root


@pytest.mark.parametrize("R,C,plies,sims", [(3, 3, 2, 40), (1, 6, 1, 30), (5, 7, 6, 80), (9, 12, 10, 40)])
@pytest.mark.parametrize("with_noise", [False, True])
def test_without_advance_the_model_is_the_reference_search(R, C, plies, sims, with_noise):
    for seed in range(2):
        board, player = random_root(R, C, plies, 50 + seed)
        noise = dirichlet_noise(board, player, seed) if with_noise else None
        want = O.search_hash(board, player, sims, 1, 10, 11, noise=noise)
        lp = L.search(board, player, sims, 1, noise=noise)
        got = T.search(board, player, sims, noise=noise)
        assert np.array_equal(got.counts, want.counts) and np.array_equal(got.counts, lp.counts)
        assert np.array_equal(got.child_w.astype(np.float64), want.child_w) and np.array_equal(got.child_w, lp.child_w)
        assert np.array_equal(got.child_p, want.child_p) and np.array_equal(got.child_p, lp.child_p)
        assert (got.root_visits, got.root_w) == (want.root_visits, want.root_w) == (lp.root_visits, lp.root_w)
        assert got.evals == want.n_evals == lp.evals
        for k in ("levels", "children_scanned", "children_created", "terminal_revisits", "nodes"):
            assert getattr(got, k) == getattr(lp, k), k


def test_a_kept_root_is_topped_up_not_searched_again():
    board, player = random_root(5, 7, 6, 3)
    first = T.search(board, player, 80)
    a = int(np.argmax(first.counts))
    tree, kept = T.advance(first.tree, a)
    assert kept == first.counts[a] >= 2 and tree.n == kept and tree.w == float(first.child_w[a])
    again = T.search(tree, -player, kept)
    assert again.needs == [] and again.root_visits == kept and again.counts.sum() == kept - 1
    more = T.search(tree, -player, 80)
    assert len(more.needs) == 80 - kept and more.root_visits == 80 and more.counts.sum() == 79
    assert T.advance(first.tree, -1) == (None, 0) and T.advance(first.tree, 35 + 5) == (None, 0)


@pytest.mark.parametrize("name", list(Cs.CASES))
def test_every_gpu_case_keeps_trees_and_falls_back(name):
    plies = Cs.replay(name)
    searched = [(t, g) for t, p in enumerate(plies) for g in range(len(p.results)) if p.results[g] is not None]
    kept2 = [(t, g) for t, g in searched if plies[t].used_kept[g] and plies[t].kept_in[g] >= 2]
    fallback = [(t, g) for t, g in searched if t > 0 and not plies[t].used_kept[g]]
    assert 2 * len(kept2) >= len(searched), (len(kept2), len(searched))
    assert fallback
    # a kept root that already holds its budget, and one that is topped up
    assert any(plies[t].used_kept[g] and not plies[t].results[g].needs for t, g in searched)
    assert any(plies[t].used_kept[g] and plies[t].results[g].needs for t, g in searched)


def test_the_cases_cover_terminal_children_and_two_advances():
    seen = set()
    for name in Cs.CASES:
        for p in Cs.replay(name):
            for g, r in enumerate(p.results):
                if r is None:
                    continue
                e = next((e for e in r.tree.root.edges if e.action == p.actions[g]), None)
                if e is not None and e.child is not None and e.child.terminal:
                    seen.add("terminal")
                if e is not None and e.N == 1 and p.kept1[g] == 1:
                    seen.add("once")
                if p.double and p.kept2[g] >= 1:
                    seen.add("double")
                if p.noise[g].any() and p.used_kept[g]:
                    seen.add("noise on a kept root")
    assert seen == {"terminal", "once", "double", "noise on a kept root"}, seen


@pytest.mark.parametrize("mutant", sorted(T.MUTANTS))
def test_every_mutant_shows_on_the_gpu_cases(mutant):
    for name in Cs.CASES:
        if name in ("9x12", "12x16"):
            continue                                               # the small boards tell them apart; these cost seconds each
        if Cs.observables(Cs.replay(name, mutant)) != Cs.observables(Cs.replay(name)):
            return
    pytest.fail(f"no case tells mutant {mutant!r} from the model")
