"""Gumbel root search: the numpy model (tests/gumbel_model.py) against its own laws, and the host rules of the option.  Every
test here fails without the feature: neither the module's subject nor the keyword exists."""
import numpy as np
import pytest

import gumbel_model as M


@pytest.fixture(scope="module")
def options():
    import yinyang_game_alphazero_amd.options as o
    return o


@pytest.mark.parametrize("m", (1, 2, 3, 4, 16))
@pytest.mark.parametrize("n", (1, 5, 8, 16, 25))
def test_seq_has_length_n_and_the_closed_form_is_the_table(m, n):
    s = M.seq(m, n)
    assert len(s) == n
    assert s == [M.seq_at(m, n, S) for S in range(n)]
    assert s[:min(m, n)] == [0] * min(m, n)                     # the first m descents open m children


def test_the_closed_form_is_the_table_everywhere():
    for m in range(1, 65):
        for n in (1, 2, 3, 7, 8, 16, 24, 25, 50, 100, 200, 800):
            assert M.seq(m, n) == [M.seq_at(m, n, S) for S in range(n)], (m, n)


def tallies(m, k, n):
    """the children's visit counts that seq implies, sorted: entry S of the sequence is a visit to a child that holds seq[S]"""
    mp = min(m, k)
    counts = [0] * mp
    for v in M.seq(mp, n):
        counts[counts.index(v)] += 1                            # some child with exactly v visits gets one more
    return sorted(counts, reverse=True)


@pytest.mark.parametrize("name,shape,n,m", M.CASES, ids=[c[0] for c in M.CASES])
def test_a_search_visits_min_m_k_n_children_with_the_tallies_of_seq(name, shape, n, m):
    boards, players = M.roots(shape)
    for g in range(M.GAMES):
        s = M.Search(boards[g], players[g], n, m)
        s.host_s0(M.gumbel_rows(M.SEED, [g], [0], s.A)[0])
        k = len(s.root.edges)
        top = sorted(range(k), key=lambda i: (-float(s.s0[i]), i))[:min(m, k, n)]
        s.run()
        c = np.array([e.N for e in s.root.edges])
        assert int((c > 0).sum()) == min(m, k, n), (name, g, c)
        assert sorted(np.flatnonzero(c > 0)) == sorted(top), (name, g)          # the top-m' children by g + log P
        assert sorted(c[c > 0], reverse=True) == [t for t in tallies(m, k, n) if t > 0], (name, g, c)
        assert int(c.sum()) == n
        pi = s.policy()
        assert abs(pi.sum() - 1.0) < 1e-12 and (pi >= 0).all()
        assert s.counts()[s.winner()] == c.max()


def test_pi_is_the_prior_softmax_when_every_q_is_equal():
    boards, players = M.roots((5, 7))
    s = M.Search(boards[1], players[1], 8, 4)
    s.host_s0(M.gumbel_rows(M.SEED, [1], [0], s.A)[0])
    want = np.zeros(s.A)
    p = np.array([float(e.P) for e in s.root.edges])
    for e, x in zip(s.root.edges, p / p.sum()):
        want[e.action] = x
    assert np.allclose(s.policy(), want, rtol=1e-13, atol=0)                    # nothing visited: every completed q is 0
    for i, e in enumerate(s.root.edges):                                        # every child the same mean value
        e.N, e.W = i % 3 + 1, np.float32(0.25 * (i % 3 + 1))
    assert np.allclose(s.policy(), want, rtol=1e-12, atol=0)
    for e in s.root.edges[::2]:                                                 # the unvisited ones are completed with it
        e.N, e.W = 0, np.float32(0.0)
    assert np.allclose(s.policy(), want, rtol=1e-12, atol=0)


def test_a_zero_prior_child_scores_minus_infinity_and_gets_no_mass():
    boards, players = M.roots((4, 4))
    s = M.Search(boards[0], players[0], 16, 16, zero_prior=5)
    s.host_s0(M.gumbel_rows(M.SEED, [0], [0], s.A)[0])
    i = [e.action for e in s.root.edges].index(5)
    assert s.s0[i] == -np.inf
    s.run()
    assert s.root.edges[i].N >= 1                                               # k <= m: every child is considered, -inf included
    assert s.policy()[5] == 0.0 and abs(s.policy().sum() - 1.0) < 1e-12
    assert s.winner() != 5


def test_gumbel_draws_are_finite_and_keyed():
    a = M.gumbel_rows(3, [0, 1, 0], [0, 0, 1], 16)
    assert np.isfinite(a).all() and not np.array_equal(a[0], a[1]) and not np.array_equal(a[0], a[2])
    assert np.array_equal(a, M.gumbel_rows(3, [0, 1, 0], [0, 0, 1], 16))
    assert abs(float(a.mean()) - 0.5772) < 0.6                                  # Gumbel(0, 1): mean 0.5772, sd 1.28 over 48 draws


# ------------------------------------------------------------------------------------------------ the option rules
REFUSALS = [dict(leaves_per_step=2), dict(board_semantics="aliased"), dict(reference_quirks=True), dict(rng="numpy"),
            dict(forced_playouts=2.0), dict(tree_reuse=True), dict(solver=True)]


@pytest.mark.parametrize("kw", REFUSALS, ids=[next(iter(k)) for k in REFUSALS])
def test_every_refusal_names_gumbel_root(options, kw):
    with pytest.raises(options.OptionConflict) as e:
        options.resolve(num_simulations=16, gumbel_root=4, **kw)
    assert e.value.option == "gumbel_root" and next(iter(kw)) in e.value.conflicts


@pytest.mark.parametrize("kw", [dict(gumbel_root=1), dict(gumbel_root=65), dict(gumbel_root=-3), dict(gumbel_root=2.5),
                                dict(gumbel_root="x"), dict(gumbel_root=True), dict(gumbel_root=4, gumbel_c_visit=-1.0),
                                dict(gumbel_root=4, gumbel_c_visit=float("inf")), dict(gumbel_root=4, gumbel_c_scale=0.0),
                                dict(gumbel_root=4, gumbel_c_scale=float("nan")), dict(gumbel_c_visit=50.0),
                                dict(gumbel_root=0, gumbel_c_scale=1.0)])
def test_values_outside_the_ranges_are_refused(options, kw):
    with pytest.raises(options.OptionConflict) as e:
        options.resolve(**kw)
    assert e.value.option == "gumbel_root" and e.value.conflicts == ()


def test_the_option_resolves_and_is_forwarded(options):
    off = options.resolve(num_simulations=16)
    assert off.gumbel_root == 0 and "gumbel_root" not in off.keywords()
    assert options.resolve(gumbel_root=None).keywords() == options.resolve(gumbel_root=0).keywords() == off.keywords()
    on = options.resolve(num_simulations=16, gumbel_root=16)
    assert (on.gumbel_root, on.gumbel_c_visit, on.gumbel_c_scale) == (16, 50.0, 1.0)
    assert on.keywords()["gumbel_root"] == 16 and on.keywords()["gumbel_c_visit"] == 50.0
    # it goes with the playout cap, free-running, evaluation symmetry, the shared tables and fpu_reduction
    o = options.resolve(num_simulations=16, gumbel_root=2, gumbel_c_visit=0, gumbel_c_scale=0.1, fast_simulations=4,
                        full_search_probability=0.5, free_running=True, evaluation_symmetry="random", fpu_reduction=0.2,
                        shared_evaluations=64, shared_evaluations_replace=True)
    assert (o.gumbel_root, o.gumbel_c_visit, o.gumbel_c_scale) == (2, 0.0, 0.1) and o.free_running


def test_the_cli_flags_resolve():
    import train_alphazero as T
    for mode in ("self-play", "train"):
        a = T.parse_args(["--mode", mode, "--gumbel-root", "16", "--gumbel-c-visit", "40", "--gumbel-c-scale", "0.5"])
        assert (a.gumbel_root, a.gumbel_c_visit, a.gumbel_c_scale) == (16, 40.0, 0.5)
        assert T.refused(a) is None
        msg = T.refused(T.parse_args(["--mode", mode, "--gumbel-root", "16", "--solver"]))
        assert msg and "--gumbel-root 16" in msg and "--solver" in msg
        assert "out of range" in T.refused(T.parse_args(["--mode", mode, "--gumbel-root", "1"]))
    assert T.refused(T.parse_args(["--mode", "self-play", "--gumbel-root", "4", "--board-semantics", "aliased"]))
    assert "gumbel_root" not in sum(T.HANDED["evaluate"], ())                   # the arena does not take it
