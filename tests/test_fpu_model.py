"""First-play urgency reduction: the numpy model (tests/fpu_model.py) against the models it is built on and the C oracle at
r = 0, its own laws and its mutants, on the fixtures the GPU tests (tests/test_gpu_fpu.py) run."""
import itertools

import numpy as np
import pytest

import forced_playouts_model as F
import fpu_model as M
import leaf_parallel_model as L
import oracle_lib as O
from hash_eval import hash_eval_batch

f32 = np.float32


def scaled(b):
    p, v = hash_eval_batch(b, 10, 11)
    return p * f32(M.PSCALE), v


def same(a, w):
    assert np.array_equal(a.counts, w.counts)
    assert np.array_equal(a.child_w.view(np.uint32), np.asarray(w.child_w, np.float32).view(np.uint32))
    assert np.array_equal(a.child_p.view(np.uint32), w.child_p.view(np.uint32))
    assert a.root_visits == w.root_visits and a.root_w == w.root_w


SHAPES = [(4, 4, 2, 32), (5, 7, 3, 48), (1, 6, 1, 16), (7, 1, 2, 16), (9, 12, 2, 16), (12, 12, 3, 16)]


@pytest.mark.parametrize("R,C,plies,sims", SHAPES)
@pytest.mark.parametrize("K", [1, 4])
def test_r_zero_is_the_leaf_parallel_model(R, C, plies, sims, K):
    for seed in range(3):
        board, player = M.random_root(R, C, plies, seed)
        noise = M.dirichlet_noise(board, player, 50 + seed) if seed else None
        for kw in (dict(), dict(r=0.0, r_root=0.0)):
            same(M.search(board, player, sims, K=K, noise=noise, **kw), L.search(board, player, sims, K, noise=noise, evaluator=scaled))


@pytest.mark.parametrize("name", ["4x4", "5x7", "9x12"])
@pytest.mark.parametrize("k", [0.0, 2.0])
def test_r_zero_is_the_tree_reuse_and_forced_playouts_model(name, k):
    """Three moves on kept roots with root noise: forced_playouts_model.search (k = 0: tree_reuse_model's search) move by move."""
    boards, players, noise, noise2 = F.roots(name)
    n = 0
    for g in range(F.GAMES):
        a, w = M.search(boards[g], players[g], 24, forced=k, noise=noise[g]), F.search(boards[g], players[g], 24, k, noise=noise[g])
        same(a, w)
        for nz in (noise2[g], noise[g]):
            act = int(np.argmax(w.counts))
            ta, ka = M.advance(a.tree, act)
            tw, kw = M.advance(w.tree, act)
            assert ka == kw and (ta is None) == (tw is None)
            if ta is None or ka >= 24 or ta.root.terminal:
                break
            p = ta.root.player
            a, w = M.search(ta, p, 24, forced=k, noise=nz), F.search(tw, p, 24, k, noise=nz)
            same(a, w)
            n += 1
    assert n >= F.GAMES


@pytest.mark.parametrize("R,C,plies,sims", SHAPES)
def test_r_zero_on_the_aliased_board_is_the_oracle(R, C, plies, sims):
    """The model's aliased search is new here: at r = 0 it is the C oracle's literal search, final board included."""
    for seed in range(6):
        board, player = M.random_root(R, C, seed % 5, seed)
        noise = M.dirichlet_noise(board, player, 70 + seed) if seed % 2 else None
        a, w = M.search(board, player, sims, aliased=True, noise=noise, pscale=1.0), O.search_hash(board, player, sims, 0, 10, 11, noise=noise)
        same(a, w)
        assert np.array_equal(a.final_board, w.final_board)


def test_the_fixed_point_sums_do_not_depend_on_the_order_of_the_children():
    rng = np.random.default_rng(0)
    for _ in range(50):
        k = int(rng.integers(1, 150))
        ch = [(int(n), f32(w), f32(p)) for n, w, p in zip(rng.integers(0, 4, k), rng.normal(0, 3, k), rng.random(k))]
        want = M.fixed_sums(ch)
        for _ in range(5):
            perm = rng.permutation(k)
            assert M.fixed_sums([ch[i] for i in perm]) == want
        # lane order on the device: child i*64 + lane is lane's i-th term, the lanes are reduced as a tree
        lanes = [M.fixed_sums(ch[l::64]) for l in range(64)]
        assert tuple(sum(x[i] for x in lanes) for i in range(3)) == want
        assert all(abs(x) < 2 ** 63 for x in want)
    # a float32 sum of the same terms does depend on the order: the reason for the fixed point
    w = [f32(1e8), f32(1.0), f32(-1e8)]
    assert f32(f32(w[0] + w[1]) + w[2]) != f32(f32(w[0] + w[2]) + w[1])
    # truncation toward zero, and the units
    assert M.fixed_sums([(1, f32(-0.75), f32(0.5)), (0, f32(9.0), f32(0.25))]) == (1, -3 * 2 ** 30, 2 ** 39)
    assert M.fixed_sums([(2, f32(-2.0 ** -33), f32(2.0 ** -41))]) == (2, 0, 0)


def test_the_formula_in_its_order():
    assert M.fpu_q(0.25, 0, 0, 0) == 0.0
    SN, SW, SP = M.fixed_sums([(3, f32(1.5), f32(0.25)), (1, f32(-0.25), f32(0.0625))])
    want = f32(f32(f32(1.25) / f32(4)) - f32(f32(0.25) * np.sqrt(f32(0.3125))))
    assert M.fpu_q(0.25, SN, SW, SP) == want
    assert M.fpu_q(0.0, SN, SW, SP) == f32(f32(1.25) / f32(4))         # r_root = 0: the visited children's mean itself


def test_every_case_differs_from_the_search_without_the_option():
    for name in M.CASES:
        assert M.observables(M.fixture(name)) != M.observables(M.fixture(name, off=True)), name


def test_the_cases_cover_what_they_are_for():
    for name, (R, C, sims, kw, eps, moves) in M.CASES.items():
        fx = M.fixture(name)
        assert len(fx) == moves and all(r is not None and not r.failed and r.root_visits == sims for r in fx[0].results), name
        if moves > 1:                                              # kept roots: at least half of the games search on, twice
            assert all(sum(r is not None for r in m.results) >= M.GAMES // 2 for m in fx[1:]), name
            assert all(r.tree.kept for m in fx[1:] for r in m.results if r is not None), name
    for name in ("1x6", "7x1"):                                    # pass roots and childless nodes below a root
        fx = M.fixture(name)[0]
        assert any(not r.tree.root.edges and not r.tree.root.terminal for r in fx.results), name

        def childless(node):
            return any(e.child is not None and (not e.child.terminal and not e.child.edges or childless(e.child)) for e in node.edges)
        assert any(childless(r.tree.root) for r in fx.results), name
    for name in ("9x12", "12x12"):                                 # more than 64 / more than 128 children at a root
        assert max(len(r.tree.root.edges) for r in M.fixture(name)[0].results) > (64 if name == "9x12" else 128), name


@pytest.mark.parametrize("mutant", sorted(M.MUTANTS))
def test_the_fixtures_tell_every_mutant_from_the_model(mutant):
    hit = [name for name in M.CASES if M.observables(M.fixture(name, mutant)) != M.observables(M.fixture(name))]
    assert hit, mutant
    if mutant == "r_everywhere":
        assert all("root0" in n or "reuse" in n for n in hit), hit
    if mutant == "prior_raw":
        assert all(M.CASES[n][4] for n in hit), hit                 # only a noised root has another prior to read
    if mutant not in ("r_everywhere", "prior_raw"):                 # the others show on copied, K > 1, kept, forced and aliased searches
        for kind in ("", "-K4", "-reuse", "-forced", "-aliased"):
            assert any(n.endswith(kind) if kind else "-" not in n for n in hit), (mutant, kind, hit)


def test_forcing_and_pruning_do_not_read_the_urgency():
    """edge_forced looks at visited edges only and pruning scores visited edges only: on the final tree of a search with the
    option, the forcing test and the pruned counts are those of forced_playouts_model on the same edges."""
    for m in M.fixture("4x4-forced") + M.fixture("5x7-forced"):
        for r in m.results:
            edges = r.tree.root.edges
            S = sum(e.N for e in edges)
            assert all(e.N > 0 for e in edges if F.is_forced(2.0, e.P, e.N, S))
            pruned = F.prune(edges, 2.0)
            assert all(p == 0 for p, e in zip(pruned, edges) if e.N == 0)
