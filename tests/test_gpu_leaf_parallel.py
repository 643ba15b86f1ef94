"""Leaf-parallel MCTS (leaves_per_step K, include/yy_engine.h) on the MI355X: the HIP search against the plain-numpy
restatement (tests/leaf_parallel_model.py) with tolerance 0, the step machinery (fused / unfused, graph replay / eager, a
rows limit, inactive games), the sticky error, the refused combinations, and the public interface (MCTS, Arena)."""
import numpy as np
import pytest

import tree_model as M
from hash_eval import hash_eval_batch, hash_eval_torch, planes_to_boards
from tree_model import dirichlet_noise, random_root

pytestmark = pytest.mark.gpu
PB, VB = 10, 11


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    import yinyang_game_alphazero_amd as p
    return p


def host_eval(planes):
    import torch
    p, v = hash_eval_batch(planes_to_boards(planes.cpu().numpy()), PB, VB)
    return torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda()


def roots(R, C, G, plies, seed):
    bs, ps = zip(*[random_root(R, C, plies + (g % 3), seed * 101 + g) for g in range(G)])
    return np.stack(bs), np.array(ps, np.int8)


def check_against_model(ctx, boards, players, sims, K, noise=None, games=None):
    counts, cw, cp = (t.cpu().numpy() for t in ctx.root_counts(with_children=True))
    visits, wsum = (t.cpu().numpy() for t in ctx.root_stats())
    evals = 0
    for g in (range(len(boards)) if games is None else games):
        want = M.search(boards[g], int(players[g]), sims, K, PB, VB, noise=None if noise is None else noise[g])
        assert np.array_equal(counts[g], want.counts), (g, K)
        assert np.array_equal(cw[g], want.child_w), (g, K)
        assert np.array_equal(cp[g], want.child_p), (g, K)
        assert int(visits[g]) == want.root_visits == sims
        assert float(wsum[g]) == want.root_w
        evals += want.evals
    return evals


SHAPES = [(3, 3, 0, 40, 6), (3, 3, 3, 25, 6), (8, 8, 4, 800, 2), (16, 12, 6, 60, 3)]


@pytest.mark.parametrize("R,C,plies,sims,G", SHAPES)
@pytest.mark.parametrize("K", [1, 2, 3, 8, 32])
def test_search_equals_restatement(pkg, R, C, plies, sims, G, K):
    import torch
    boards, players = roots(R, C, G, plies, seed=K)
    noise = np.stack([dirichlet_noise(boards[g], int(players[g]), 7 + g) if g % 2 else np.zeros(R * C) for g in range(G)])
    mc = pkg.engine.BatchedMCTS(G, R, C, sims, leaves_per_step=K)
    try:
        assert mc.planes.shape[0] == G * K and mc.needs_eval.shape[0] == G * K
        mc.search(torch.from_numpy(boards).cuda(), torch.from_numpy(players).cuda(), host_eval, sims,
                  noise=torch.from_numpy(noise).cuda())
        evals = check_against_model(mc, boards, players, sims, K, noise=[None if not g % 2 else noise[g] for g in range(G)])
        assert mc.status()["evals"] == evals
    finally:
        mc.close()


def test_k1_through_the_parameter_is_the_default_context(pkg):
    import torch
    R, C, G, sims = 6, 6, 4, 90
    boards, players = roots(R, C, G, 3, seed=3)
    out = []
    for kw in ({}, dict(leaves_per_step=1), dict(leaves_per_step=0)):
        mc = pkg.engine.BatchedMCTS(G, R, C, sims, **kw)
        mc.search(torch.from_numpy(boards).cuda(), torch.from_numpy(players).cuda(), host_eval, sims)
        out.append([t.cpu().numpy() for t in mc.root_counts(with_children=True) + mc.root_stats()] + [mc.status()])
        mc.close()
    for o in out[1:]:
        for a, b in zip(out[0][:-1], o[:-1]):
            assert np.array_equal(a, b)
        assert o[-1] == out[0][-1]


def test_memory_grows_with_k(pkg):
    a = pkg.engine.BatchedMCTS(4, 8, 8, 100)
    b = pkg.engine.BatchedMCTS(4, 8, 8, 100, leaves_per_step=8)
    assert b.memory_bytes() > a.memory_bytes()
    a.close()
    b.close()


def test_fused_equals_unfused(pkg):
    import torch
    R, C, G, sims, K = 8, 8, 4, 150, 8
    boards, players = roots(R, C, G, 5, seed=11)
    res = []
    for fused in (True, False):
        mc = pkg.engine.BatchedMCTS(G, R, C, sims, leaves_per_step=K)
        mc.search(torch.from_numpy(boards).cuda(), torch.from_numpy(players).cuda(), host_eval, sims, fused=fused)
        res.append([t.cpu().numpy() for t in mc.root_counts(with_children=True) + mc.root_stats()] + [mc.status()])
        mc.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


def test_lockstep_graph_equals_eager_with_rows_limit_and_inactive_games(pkg):
    import torch
    from yinyang_game_alphazero_amd.self_play import LockstepSearch
    R, C, G, sims, K, rows = 8, 8, 8, 200, 8, 5
    boards, players = roots(R, C, G, 4, seed=5)
    active = np.array([1, 1, 0, 1, 1, 0, 0, 0], np.uint8)            # rows limit 5: every active game sits below it
    ev = lambda planes, **kw: hash_eval_torch(planes, PB, VB)
    res = []
    for use_graph in (True, False):
        mc = pkg.engine.BatchedMCTS(G, R, C, sims, leaves_per_step=K)
        ls = LockstepSearch(mc, ev, use_graph=use_graph, unroll=4)
        for _ in range(2):                                            # the second search replays the captured steps
            ls.run(torch.from_numpy(boards).cuda(), torch.from_numpy(players).cuda(), sims,
                   active=torch.from_numpy(active).cuda(), rows=rows)
        if use_graph:
            assert ls.graphs
        res.append([t.cpu().numpy() for t in mc.root_counts(with_children=True) + mc.root_stats()] + [mc.status()])
        evals = check_against_model(mc, boards, players, sims, K, games=np.flatnonzero(active))
        assert res[-1][-1]["evals"] == 2 * evals
        assert (res[-1][0][active == 0] == 0).all()
        mc.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


@pytest.mark.parametrize("S,n_graphs", [(1, 0), (2, 0), (4, 0), (5, 1), (12, 2), (13, 2)])
@pytest.mark.parametrize("K", [1, 3])
def test_every_driver_agrees_on_short_searches(pkg, K, S, n_graphs):
    """S steps of K descents around LockstepSearch's thresholds (eager_sims = 3, unroll = 4): S - 1 = 3 middle steps capture
    nothing, 4 the one-step graph, 11 leave 8 = 2 * unroll after the warm-up and capture both, 12 replay the unrolled graph twice
    and the one-step graph besides.  search() fused and unfused, LockstepSearch eager and replayed: one result."""
    import torch
    from yinyang_game_alphazero_amd.search import LockstepSearch
    R, C, G, sims = 6, 6, 4, K * S
    boards, players = (torch.from_numpy(a).cuda() for a in roots(R, C, G, 3, seed=7))
    ev = lambda planes, **kw: hash_eval_torch(planes, PB, VB)

    def lockstep(use_graph, searches):
        def drive(mc):
            ls = LockstepSearch(mc, ev, use_graph=use_graph, eager_sims=3, unroll=4)
            for _ in range(searches):                                 # the second search is pure replay
                ls.run(boards, players, sims)
            assert len(ls.graphs) == (n_graphs if use_graph else 0)
        return drive, searches

    res = []
    for drive, searches in ((lambda mc: mc.search(boards, players, ev, sims, fused=True), 1),
                            (lambda mc: mc.search(boards, players, ev, sims, fused=False), 1), lockstep(False, 1), lockstep(True, 2)):
        mc = pkg.engine.BatchedMCTS(G, R, C, sims, leaves_per_step=K)
        try:
            drive(mc)
            counters = mc.status()
            assert all(v % searches == 0 for v in counters.values())
            res.append([t.cpu().numpy() for t in mc.root_counts(with_children=True) + mc.root_stats()]
                       + [{k: v // searches for k, v in counters.items()}])
        finally:
            mc.close()
    if n_graphs:                                                      # unroll = 1: the one-step graph only, same result
        mc = pkg.engine.BatchedMCTS(G, R, C, sims, leaves_per_step=K)
        try:
            ls = LockstepSearch(mc, ev, use_graph=True, eager_sims=3, unroll=1)
            ls.run(boards, players, sims)
            assert len(ls.graphs) == 1
            res.append([t.cpu().numpy() for t in mc.root_counts(with_children=True) + mc.root_stats()] + [mc.status()])
        finally:
            mc.close()
    assert (res[0][3] == sims).all()
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


def test_nan_in_a_later_row_stops_only_that_game(pkg):
    import torch
    R, C, G, sims, K = 6, 6, 3, 40, 4
    boards, players = roots(R, C, G, 2, seed=9)
    calls = [0]

    def ev(planes):
        p, v = host_eval(planes)
        calls[0] += 1
        if calls[0] == 3:                                             # the second simulation step
            need = mc.needs_eval.cpu().numpy()
            rows = [j for j in range(1, K) if need[1 * K + j]]
            assert rows, "game 1 asks for a row j > 0"
            v[1 * K + rows[0]] = float("nan")
        return p, v

    mc = pkg.engine.BatchedMCTS(G, R, C, sims, leaves_per_step=K)
    mc.search(torch.from_numpy(boards).cuda(), torch.from_numpy(players).cuda(), ev, sims)
    visits, _ = mc.root_stats()
    with pytest.raises(pkg._lib.YYError) as e:
        mc.status()
    assert e.value.code == pkg._lib.YY_E_ARENA
    assert int(visits[1]) < sims
    check_against_model(mc, boards, players, sims, K, games=[0, 2])
    mc.close()


@pytest.mark.parametrize("kw", [dict(aliased=True), dict(reuse_pass_value=True), dict(reuse_transpositions=True),
                                dict(keep_evaluations=True)])
def test_create_refuses_k_with_aliased_boards_and_reuse(pkg, kw):
    with pytest.raises(pkg._lib.YYError) as e:
        pkg.engine.BatchedMCTS(2, 6, 6, 50, leaves_per_step=4, **kw)
    assert e.value.code == -2 and "leaves_per_step" in str(e.value)
    pkg.engine.BatchedMCTS(2, 6, 6, 50, leaves_per_step=1, **kw).close()     # K = 1 still takes them


@pytest.fixture(scope="module")
def net800(pkg):
    import torch
    torch.manual_seed(0)
    game = pkg.YinYangGame(8, 8)
    ev = pkg.BatchedEvaluator(pkg.YinYangNeuralNetwork(game).cuda().eval(), "f16x3")
    return game, ev


def test_mcts_search_f16x3_k8(pkg, net800):
    game, ev = net800
    board, player = random_root(8, 8, 6, 1)
    from yinyang_game_alphazero_amd.game import YinYangLogic
    lb = YinYangLogic(8, 8)
    lb.board = board.copy()
    pis = []
    for use_graph in (True, True, False):
        m = pkg.MCTS(game, ev, num_simulations=800, board_semantics="copied", leaves_per_step=8)
        m.use_graph = use_graph
        pi, root = m.search(lb, player)
        assert root.visits == 800 and sum(c.visits for c in root.children.values()) == 800
        pis.append(pi)
        m.close()
    assert np.array_equal(pis[0], pis[1]) and np.array_equal(pis[0], pis[2])


def test_arena_k8_deterministic_and_equals_eager(pkg, monkeypatch):
    from yinyang_game_alphazero_amd import arena as A
    game6 = pkg.YinYangGame(6, 6)
    import torch
    torch.manual_seed(1)
    ev6 = pkg.BatchedEvaluator(pkg.YinYangNeuralNetwork(game6, 32, 2).cuda().eval(), "f16x3")
    out = []
    for _ in range(2):
        a = A.Arena(game6, ev6, ev6, num_simulations=64, leaves_per_step=8)
        out.append((a.play(4, record=True), a.transcript))
    real = A.LockstepSearch
    monkeypatch.setattr(A, "LockstepSearch", lambda ctx, dual, use_graph=True: real(ctx, dual, use_graph=False))
    a = A.Arena(game6, ev6, ev6, num_simulations=64, leaves_per_step=8)
    out.append((a.play(4, record=True), a.transcript))
    for res, tr in out[1:]:
        assert res == out[0][0]
        for k in tr:
            assert np.array_equal(tr[k], out[0][1][k])
