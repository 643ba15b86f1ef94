"""The numpy restatement of Gumbel search below the root (tests/gumbel_interior_model.py) against its own laws (no GPU): the
exponential against math.exp, pi' as a distribution, its two limits, the option off as gumbel_model's search, and the fixtures
of the GPU tests: every mutant and the option itself change what those tests compare."""
import functools
import math

import numpy as np
import pytest

import gumbel_interior_model as M
import gumbel_model as G
from tree_model import Edge

f32 = np.float32


def test_the_exponential_is_within_1e14_of_math_exp():
    rng = np.random.default_rng(7)
    xs = list(-708.0 * rng.random(100000)) + [0.0, -708.0] + [-math.log(2.0) * n for n in range(1, 1022)]
    worst = max(abs(M.E(x) - math.exp(x)) / math.exp(x) for x in xs)
    print("largest relative difference", worst)
    assert worst <= 1e-14
    assert M.E(0.0) == 1.0 and M.E(math.nextafter(-708.0, -math.inf)) == 0.0 and M.E(-1e300) == 0.0 and M.E(-708.0) > 0.0


def edges_of(P, N, W):
    out = []
    for a, (p, n, w) in enumerate(zip(P, N, W)):
        e = Edge(a, p)
        e.N, e.W = int(n), f32(w)
        out.append(e)
    return out


def random_node(rng, k, visited):
    P = rng.random(k).astype(np.float32)
    P /= P.sum()
    N = np.where(rng.random(k) < visited, rng.integers(1, 9, k), 0)
    W = (N * (2 * rng.random(k) - 1)).astype(np.float32)
    return edges_of(P, N, W), f32(2 * rng.random() - 1)


@pytest.mark.parametrize("k", [1, 2, 16, 35, 108, 144])
def test_pi_prime_is_a_distribution(k):
    rng = np.random.default_rng(k)
    for visited in (0.0, 0.3, 1.0):
        for _ in range(20):
            edges, vhat = random_node(rng, k, visited)
            pi = M.pi_prime(edges, vhat, 50.0, 1.0)
            assert all(x >= 0.0 for x in pi) and abs(sum(pi) - 1.0) <= 1e-15 * k


def test_without_visits_pi_prime_is_the_prior_row_and_v_mix_the_nodes_value():
    rng = np.random.default_rng(3)
    for k in (1, 5, 144):
        edges, vhat = random_node(rng, k, 0.0)
        t, Z, S, vmix = M.improved(edges, vhat, 50.0, 1.0)
        assert S == 0 and vmix == float(vhat)
        p = [M.prior(e) for e in edges]                             # E(0) == 1: the terms are the fixed-point priors, exactly
        assert t == [pi * 4096 for pi in p] and Z == 4096 * sum(p)
        assert M.pi_prime(edges, vhat, 50.0, 1.0) == [float(ti) / float(Z) for ti in t]
    zero = edges_of([0.0, 0.0, 0.0], [0, 0, 0], [0.0, 0.0, 0.0])     # every prior 0: the uniform row
    assert M.pi_prime(zero, f32(0.5), 50.0, 1.0) == [1.0 / 3.0] * 3


def test_with_every_child_visited_the_nodes_value_drops_out_of_pi_prime_but_not_of_v_mix():
    rng = np.random.default_rng(4)
    edges, _ = random_node(rng, 20, 1.0)
    a, b = M.improved(edges, f32(0.75), 50.0, 1.0), M.improved(edges, f32(-0.25), 50.0, 1.0)
    assert a[:3] == b[:3] and a[3] != b[3]
    unvisited, _ = random_node(rng, 20, 0.5)
    # a flat sigma (small c_visit, c_scale), so that the terms of the unvisited children do not all truncate to 0
    assert M.improved(unvisited, f32(0.75), 1.0, 0.1)[0] != M.improved(unvisited, f32(-0.25), 1.0, 0.1)[0]


def test_the_interior_rule_takes_the_lowest_edge_on_ties_and_passes_a_nan_over():
    tie = edges_of([0.25, 0.25, 0.25, 0.25], [0, 0, 0, 0], [0, 0, 0, 0])
    assert M.select_interior(tie, f32(0.0), 50.0, 1.0).action == 0
    assert M.select_interior(tie, f32(0.0), 50.0, 1.0, "tie_high").action == 3
    tie[0].N, tie[0].W = 1, f32(math.nan)
    assert M.select_interior(tie, f32(0.0), 50.0, 1.0).action == 1
    for e in tie:
        e.N, e.W = 1, f32(math.nan)
    assert M.select_interior(tie, f32(0.0), 50.0, 1.0) is None


@functools.lru_cache(maxsize=None)
def run(case, g, interior=True, mutant=None):
    name, shape, n, m = next(c for c in M.CASES if c[0] == case)
    boards, players = G.roots(shape, M.GAMES)
    s = M.fixture(shape, n, m, g, boards, players, interior=interior, mutant=mutant).run()
    assert not s.failed and s.sims == n
    return s


@pytest.mark.parametrize("case", [c[0] for c in M.CASES])
def test_the_option_off_is_gumbel_models_search(case):
    name, shape, n, m = next(c for c in M.CASES if c[0] == case)
    boards, players = G.roots(shape, M.GAMES)
    for g in range(M.GAMES):
        want = G.Search(boards[g], players[g], n, m)
        want.host_s0(G.gumbel_rows(M.SEED, [g], [0], shape[0] * shape[1])[0])
        want.run()
        got = run(case, g, interior=False)
        assert np.array_equal(got.counts(), want.counts()) and np.array_equal(got.child_w().view(np.uint32), want.child_w().view(np.uint32))
        assert got.winner() == want.winner() and np.array_equal(got.policy(), want.policy())
        assert (got.levels, got.evals, got.nodes) == (want.levels, want.evals, want.nodes)


@pytest.mark.parametrize("case", [c[0] for c in M.CASES])
def test_the_option_changes_every_fixture(case):
    """a device that takes the flag and ignores it fails the GPU tests of every case"""
    assert any(M.tally(run(case, g)) != M.tally(run(case, g, interior=False)) for g in range(M.GAMES))
    assert any(M.tally(run(case, g))[0] != M.tally(run(case, g, interior=False))[0] for g in range(M.GAMES))     # the trees themselves


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_changes_a_tally_of_a_fixture(mutant):
    hit = [c[0] for c in M.CASES if any(M.tally(run(c[0], g, mutant=mutant)) != M.tally(run(c[0], g)) for g in range(M.GAMES))]
    print(mutant, "changes", hit)
    assert hit
