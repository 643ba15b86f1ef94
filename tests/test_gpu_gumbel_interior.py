"""Gumbel search below the root on the device (include/yy_engine.h YY_FLAG_GUMBEL_INTERIOR) against tests/gumbel_interior_model.py.

Search pin: after EVERY simulation the root children's N and W (raw bits) and the Gumbel winner equal the model's; after the
search every node's record -- its edges' prior, N, W and child, its own evaluator value, the root's included -- and pi' equal
the model's, bit for bit: the model takes the device's base scores s0 as its input (the root's rule is unchanged) and restates
everything below operation for operation.  Engines: free-running equals lockstep, two lanes equal one, evaluation reuse and both
shared tables play the same games, and the option changes the games.  Every test here fails without the feature: the keyword
and the flag do not exist."""
import ctypes
import functools

import numpy as np
import pytest

import gumbel_interior_model as M
import gumbel_model as G
import tree_model
from hash_eval import hash_eval_torch

pytestmark = pytest.mark.gpu
KEYS = ("states", "policies", "values", "game_id", "ply")
NONE = 0xFFFFFF


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    import yinyang_game_alphazero_amd as p
    return p


class HashEval:
    """The exact hash evaluator: a pure function of the row.  zero: (row, action) whose prior the FIRST call returns as exactly 0."""
    row_independent = True

    def __init__(self, zero=None):
        self.zero = zero

    def __call__(self, planes):
        p, v = hash_eval_torch(planes, 10, 11)
        if self.zero is not None:
            p = p.clone()
            p[self.zero[0], self.zero[1]] = 0.0
            self.zero = None
        return p, v


def same_tree(s, nodes, edges, where):
    """the device's records of one game against the model's tree, walked together from the root"""
    stack, seen = [(0, s.root)], 0
    while stack:
        i, node = stack.pop()
        first, y, z, w = (int(x) for x in nodes[i])
        k = y & 0xFFFF
        seen += 1
        assert k == len(node.edges) and bool((y >> 16) & 1) == node.terminal, (where, i)
        if node.terminal:
            assert np.uint32(z).view(np.float32) == np.float32(node.tv), (where, i)
        assert w == int(np.float32(s.vhat(node)).view(np.uint32)), (where, "the node's own value", i)
        for j, e in enumerate(node.edges):
            p, n, wsum, cw = (int(x) for x in edges[first + j])
            assert (cw >> 24, p, n, wsum) == (e.action, int(e.P.view(np.uint32)), e.N, int(np.float32(e.W).view(np.uint32))), (where, i, j)
            assert ((cw & NONE) == NONE) == (e.child is None), (where, i, j)
            if e.child is not None:
                stack.append((cw & NONE, e.child))
    return seen


def pin(pkg, shape, n, m, budgets=None, zero=None, eps=0.0, games=M.GAMES):
    import torch
    R, C = shape
    A = R * C
    boards, players = G.roots(shape, games)
    ev = HashEval(zero)
    mc = pkg.engine.BatchedMCTS(games, R, C, n, gumbel_root=m, gumbel_interior=True)
    try:
        rows = pkg.engine.gumbel_rows(M.SEED, torch.arange(games, dtype=torch.int64).cuda(), torch.zeros(games, dtype=torch.int32).cuda(), A)
        mc.set_gumbel(rows)
        if budgets is None:
            mc.set_num_sims(n)
        else:
            mc.set_sim_budgets(torch.tensor(budgets, dtype=torch.int32).cuda())
        noise = np.stack([tree_model.dirichlet_noise(boards[g], players[g], 100 + g) for g in range(games)]) if eps else None
        mc.begin(torch.from_numpy(boards).cuda(), torch.from_numpy(players).cuda())
        policy, value = ev(mc.planes)
        with pytest.raises(pkg._lib.YYError):                                   # the root keeps its value: the form without it is refused
            mc.expand_root(policy)
        mc.expand_root(policy, None if noise is None else torch.from_numpy(noise).cuda(), eps, value=value)
        s0 = mc.root_gumbel().cpu().numpy()
        model = []
        for g in range(games):
            s = M.Search(boards[g], players[g], n if budgets is None else budgets[g], m, noise=None if noise is None else noise[g],
                         eps=eps, zero_prior=zero[1] if zero is not None and zero[0] == g else None)
            s.set_s0(s0[g])
            model.append(s)
        for step in range(n):
            mc.select()
            mc.expand_backup(*ev(mc.planes))
            counts, cw, _ = (t.cpu().numpy() for t in mc.root_counts(with_children=True))
            act = mc.root_gumbel_action().cpu().numpy()
            for g, s in enumerate(model):
                s.step()
                where = (shape, n, m, "game", g, "after simulation", step + 1)
                assert np.array_equal(counts[g], s.counts()), (where, counts[g], s.counts())
                assert np.array_equal(cw[g].view(np.uint32), s.child_w().view(np.uint32)), where
                assert act[g] == s.winner(), (where, act[g], s.winner())
        pi = mc.root_policy().cpu().numpy()
        pi0 = mc.root_policy(temperature_zero=True).cpu().numpy()
        nodes, edges, sizes = (t.cpu().numpy().view(np.uint32) for t in mc.tree())
        for g, s in enumerate(model):
            assert not s.failed
            assert np.array_equal(pi[g].view(np.uint64), s.policy().view(np.uint64)), (shape, g, pi[g], s.policy())
            assert np.array_equal(pi[g].view(np.uint64), pi0[g].view(np.uint64))
            assert same_tree(s, nodes[g], edges[g], (shape, n, m, "game", g)) == int(sizes[g, 0]) == s.nodes + 1
        assert np.array_equal(mc.root_stats()[0].cpu().numpy(), [s.sims for s in model])
        mc.status()
    finally:
        mc.close()
    return model


@pytest.mark.parametrize("name,shape,n,m", M.CASES, ids=[c[0] for c in M.CASES])
def test_every_simulation_and_every_node_equal_the_model(pkg, name, shape, n, m):
    model = pin(pkg, shape, n, m)
    # the device did not ignore the flag: the plain Gumbel root search builds other trees on these roots (checked on the CPU too)
    boards, players = G.roots(shape, M.GAMES)
    differs = False
    for g, s in enumerate(model):
        off = M.Search(boards[g], players[g], n, m, interior=False)
        off.s0 = s.s0
        differs |= M.tally(off.run())[0] != M.tally(s)[0]
    assert differs


def test_per_game_budgets_in_one_batch(pkg):
    model = pin(pkg, (4, 4), 48, 4, budgets=[4, 48, 16, 48, 0, 12, 48, 7])
    assert [s.sims for s in model] == [4, 48, 16, 48, 0, 12, 48, 7]


def test_a_child_with_prior_zero(pkg):
    model = pin(pkg, (4, 4), 16, 16, zero=(0, 5))
    assert model[0].policy()[5] == 0.0 and model[0].root.edges[[e.action for e in model[0].root.edges].index(5)].N >= 1


def test_a_noised_root(pkg):
    pin(pkg, (5, 7), 32, 8, eps=0.25)


def test_the_fused_search_is_the_stepwise_one(pkg):
    import torch
    shape, n, m = (5, 7), 32, 8
    model = pin(pkg, shape, n, m)
    boards, players = G.roots(shape, M.GAMES)
    mc = pkg.engine.BatchedMCTS(M.GAMES, *shape, n, gumbel_root=m, gumbel_interior=True)
    try:
        mc.set_gumbel(pkg.engine.gumbel_rows(M.SEED, torch.arange(M.GAMES, dtype=torch.int64).cuda(),
                                             torch.zeros(M.GAMES, dtype=torch.int32).cuda(), shape[0] * shape[1]))
        counts = mc.search(torch.from_numpy(boards).cuda(), torch.from_numpy(players).cuda(), HashEval(), n).cpu().numpy()
        pi = mc.root_policy().cpu().numpy()
        for g, s in enumerate(model):
            assert np.array_equal(counts[g], s.counts()) and np.array_equal(pi[g].view(np.uint64), s.policy().view(np.uint64))
        with pytest.raises(pkg._lib.YYError) as e:                              # tree reuse is refused, as on a Gumbel context
            mc.advance(mc.root_gumbel_action())
        assert e.value.code == -2
    finally:
        mc.close()


def test_the_c_abi_refuses_the_flag_without_the_root_flag(pkg):
    L = pkg._lib
    for flags, want in ((L.FLAG_GUMBEL_INTERIOR, -2), (L.FLAG_GUMBEL_INTERIOR | L.FLAG_GUMBEL_ROOT | L.FLAG_FPU_REDUCTION, -2)):
        cfg = L.MctsConfig(2, 4, 4, 8, 1.0, flags, 0, 0, 1, 0, 0.0, 0.2, 0.2, 4, 50.0, 1.0)
        h = ctypes.c_void_p()
        assert L.lib().yy_mcts_create(ctypes.byref(cfg), ctypes.byref(h)) == want          # YY_E_UNSUPPORTED
    assert L.FLAG_GUMBEL_INTERIOR == 1024
    with pytest.raises(ValueError):
        pkg.engine.BatchedMCTS(2, 4, 4, 8, gumbel_interior=True)


# ------------------------------------------------------------------------------------------------ self-play
ENGINE_CASES = {"4x4": ((4, 4), 8, 16, 16), "5x7": ((5, 7), 8, 8, 16)}           # board, slots, games, simulations
CAP = dict(fast_simulations=4, full_search_probability=0.5)
SP_M, SP_SEED = 4, 11


def play(pkg, case, free=False, lanes=0, interior=True, **kw):
    shape, slots, games, sims = ENGINE_CASES[case]
    game = pkg.YinYangGame(*shape)
    kw = dict(num_simulations=sims, concurrent_games=slots, seed=SP_SEED, gumbel_root=SP_M, gumbel_interior=interior,
              dirichlet_epsilon=0.0, **kw)
    if free:
        kw["free_running"] = True
    eng = pkg.SelfPlayLanes(game, HashEval(), lanes=lanes, **kw) if lanes else pkg.SelfPlayEngine(game, HashEval(), **kw)
    try:
        ex = pkg.self_play.sort_examples(eng.run(games))
        assert eng.games_finished == games
    finally:
        eng.close()
    return {k: ex[k].cpu().numpy() for k in KEYS}


@functools.lru_cache(maxsize=None)
def lockstep(pkg, case, cap=False):
    ex = play(pkg, case, **(CAP if cap else {}))
    for a in ex.values():
        a.setflags(write=False)
    return ex


def same(a, b):
    assert a["game_id"].shape == b["game_id"].shape, (a["game_id"].shape, b["game_id"].shape)
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.mark.parametrize("cap", [False, True], ids=["plain", "playout-cap"])
def test_free_running_plays_the_lockstep_games(pkg, cap):
    same(play(pkg, "4x4", free=True, **(CAP if cap else {})), lockstep(pkg, "4x4", cap))


def test_the_option_changes_the_games(pkg):
    want, off = lockstep(pkg, "4x4"), play(pkg, "4x4", interior=False)
    assert want["policies"].shape != off["policies"].shape or not np.array_equal(want["policies"], off["policies"])


def test_the_recorded_pi_is_the_models(pkg):
    """the first position of every game (the empty board, black to move) searched by the model on the device's base scores"""
    import torch
    shape, slots, games, sims = ENGINE_CASES["5x7"]
    A = shape[0] * shape[1]
    ex = lockstep(pkg, "5x7")
    first = np.flatnonzero(ex["ply"] == 0)
    assert len(first) == games
    mc = pkg.engine.BatchedMCTS(games, *shape, sims, gumbel_root=SP_M, gumbel_interior=True)
    try:
        mc.set_gumbel(pkg.engine.gumbel_rows(SP_SEED, torch.from_numpy(ex["game_id"][first].copy()).cuda(),
                                             torch.zeros(games, dtype=torch.int32).cuda(), A))
        mc.set_num_sims(sims)
        mc.begin(torch.zeros((games, *shape), dtype=torch.int8).cuda(), torch.ones(games, dtype=torch.int8).cuda())
        policy, value = HashEval()(mc.planes)
        mc.expand_root(policy, value=value)
        s0 = mc.root_gumbel().cpu().numpy()
    finally:
        mc.close()
    for j, i in enumerate(first):
        s = M.Search(np.zeros(shape, np.int8), 1, sims, SP_M)
        s.set_s0(s0[j])
        s.run()
        assert np.array_equal(ex["policies"][i].view(np.uint32), s.policy().astype(np.float32).view(np.uint32)), i


@pytest.mark.parametrize("free", [False, True], ids=["lockstep", "free-running"])
def test_two_lanes_reuse_and_the_shared_tables_play_the_same_games(pkg, free):
    want = lockstep(pkg, "5x7")
    same(play(pkg, "5x7", free=free, lanes=2), want)
    same(play(pkg, "5x7", free=free, reuse_pass_value=False, reuse_transpositions=False, keep_evaluations=False), want)
    same(play(pkg, "5x7", free=free, shared_evaluations=4096), want)
    same(play(pkg, "5x7", free=free, shared_evaluations=4096, shared_evaluations_replace=True), want)
