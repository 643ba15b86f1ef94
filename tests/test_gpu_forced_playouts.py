"""Forced playouts with policy target pruning on the device (include/yy_engine.h YY_FLAG_FORCED_PLAYOUTS), tolerance 0: integers,
bits of float32 and float64.

(a) / (b): the fixtures of tests/forced_playouts_model.py -- 4x4, 5x7, 8x8 (one bitboard word) and 9x12 (two: the wide roots have
more than 64 children), 8 games, budgets 8 / 24 / 64, root noise eps 0.25 and 0, k = 2 and k = 0.5 -- searched on one BatchedMCTS
per fixture and compared with the numpy model: raw root counts, child W, stored priors, and root_policy() for T = 1 and T = 0; then
the same on the root advance() keeps under the most visited move.  tests/test_forced_playouts_model.py asserts on the CPU that
at least half of the games of every fixture show a forced descent and a pruned edge.  The evaluator is the exact hash evaluator
with its priors times 32 (forced_playouts_model.PSCALE: its own priors, at most 1/64, never reach the forcing bound).
(c) / (d): SelfPlayEngine(forced_playouts=2) lockstep, free-running, in lanes and without graphs plays the same games.
(e): k = 0 is a context created without the option.  Every test here fails without the feature: the keyword does not exist."""
import functools

import numpy as np
import pytest

import forced_playouts_model as M
from hash_eval import hash_eval_torch

pytestmark = pytest.mark.gpu
KEYS = ("states", "policies", "values", "game_id", "ply")
FIXTURES = [(n, b, e) for n in M.SHAPES for b in M.BUDGETS for e in M.EPSILONS]
IDS = [f"{n}-{b}-eps{e}" for n, b, e in FIXTURES]


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    import yinyang_game_alphazero_amd as p
    return p


class HashEval:
    """The exact hash evaluator with its priors scaled by a power of two: a pure function of the row."""
    row_independent = True

    def __init__(self, pscale=M.PSCALE):
        self.pscale = pscale

    def __call__(self, planes):
        p, v = hash_eval_torch(planes, 10, 11)
        return p * self.pscale, v


def root_obs(mc):
    counts, cw, cp = (t.cpu().numpy() for t in mc.root_counts(with_children=True))
    return counts, cw, cp, mc.root_policy().cpu().numpy(), mc.root_policy(temperature_zero=True).cpu().numpy()


def same_root(got, g, r, where):
    counts, cw, cp, pi, pi0 = got[:5]
    assert np.array_equal(counts[g], r.counts), where
    assert np.array_equal(cw[g].view(np.uint32), r.child_w.view(np.uint32)), where
    assert np.array_equal(cp[g].view(np.uint32), r.child_p.view(np.uint32)), where
    assert np.array_equal(pi[g].view(np.uint64), r.pi.view(np.uint64)), (where, pi[g], r.pi)
    assert np.array_equal(pi0[g].view(np.uint64), r.pi0.view(np.uint64)), (where, pi0[g], r.pi0)


@functools.lru_cache(maxsize=None)
def device_run(name, budget, eps, k, pscale=M.PSCALE):
    """-> (root_obs after the fixture search, root_obs after the search on the kept roots)"""
    import torch
    import yinyang_game_alphazero_amd as pkg
    R, C = M.SHAPES[name]
    boards, players, noise, noise2 = M.roots(name)
    _, second = M.fixture(name, budget, eps, k, pscale=pscale)
    mc = pkg.engine.BatchedMCTS(M.GAMES, R, C, budget, forced_playouts=k)
    ev = HashEval(pscale)
    try:
        mc.search(torch.from_numpy(boards).cuda(), torch.from_numpy(players).cuda(), ev, budget,
                  noise=torch.from_numpy(noise).cuda() if eps else None, eps=eps)
        a = root_obs(mc) + (mc.forced_descents(),)
        go = np.array([r is not None for r in second])
        b2, p2 = boards.copy(), (-players).astype(np.int8)
        for g, r in enumerate(second):
            if r is not None:
                b2[g] = r.board
        actions = np.array([r.action if r is not None else -1 for r in second], np.int32)
        kept = mc.advance(torch.from_numpy(actions).cuda()).cpu().numpy()
        b = None
        if go.any():
            mc.search(torch.from_numpy(b2).cuda(), torch.from_numpy(p2).cuda(), ev, budget,
                      noise=torch.from_numpy(noise2).cuda() if eps else None, eps=eps,
                      active=torch.from_numpy(go.astype(np.uint8)).cuda())
            b = root_obs(mc)
        mc.status()
    finally:
        mc.close()
    return a, b, kept


@pytest.mark.parametrize("name,budget,eps", FIXTURES, ids=IDS)
@pytest.mark.parametrize("k", M.KS)
def test_the_search_and_the_pruned_policy_equal_the_model(name, budget, eps, k):
    first, _ = M.fixture(name, budget, eps, k)
    got, _, _ = device_run(name, budget, eps, k)
    for g, r in enumerate(first):
        same_root(got, g, r, (name, budget, eps, k, g, "forced descents", r.forced))


@pytest.mark.parametrize("name,budget,eps", FIXTURES, ids=IDS)
@pytest.mark.parametrize("k", M.KS)
def test_a_kept_root_equals_the_model(name, budget, eps, k):
    _, second = M.fixture(name, budget, eps, k)
    _, got, kept = device_run(name, budget, eps, k)
    n = 0
    for g, r in enumerate(second):
        if r is not None:
            assert r.kept and kept[g] > 0, (name, g)
            same_root(got, g, r, (name, budget, eps, k, g, "kept root"))
            n += 1
    assert n >= M.GAMES // 2, n


def test_the_hash_evaluator_as_it_is():
    """One fixture with the evaluator's own priors (at most 1/64 each) and k = 64: fresh and kept roots equal the model."""
    name, budget, eps, k = M.UNSCALED
    first, second = M.fixture(name, budget, eps, k, pscale=1.0)
    got, got2, _ = device_run(name, budget, eps, k, pscale=1.0)
    for g, r in enumerate(first):
        same_root(got, g, r, (g, "unscaled"))
    for g, r in enumerate(second):
        if r is not None:
            same_root(got2, g, r, (g, "unscaled, kept root"))


def test_the_forced_descent_counter_is_the_models():
    name, budget, eps, k = "5x7", 64, 0.25, 2.0
    first, _ = M.fixture(name, budget, eps, k)
    assert device_run(name, budget, eps, k)[0][5] == sum(r.forced for r in first) > 0
    assert device_run(name, budget, eps, 0.5)[0][5] == sum(r.forced for r in M.fixture(name, budget, eps, 0.5)[0])


def test_mcts_and_the_worker_take_the_option(pkg):
    """MCTS(forced_playouts=2) returns the pruned distribution of its context; another temperature than 0 / 1 is refused;
    SelfPlayWorker hands the option to its MCTS and plays a game."""
    game = pkg.YinYangGame(4, 4)
    ev = HashEval()
    m = pkg.MCTS(game, ev, num_simulations=24, board_semantics="copied", forced_playouts=2.0, dirichlet_noise=False, verbose=0)
    try:
        board = game.getInitBoard()
        pi, root = m.search(board, 1)
        r = M.search(np.zeros((4, 4), np.int8), 1, 24, 2.0)
        assert np.array_equal(pi, r.pi) and (r.pruned < r.counts).any()
        assert root.children and all(root.children[a].visits == r.counts[a] for a in root.children)
        m.temperature = 0.5
        with pytest.raises(ValueError):
            m.search(board, 1)
    finally:
        m.close()
    with pytest.raises(ValueError):
        pkg.MCTS(game, ev, forced_playouts=2.0)                     # the default board semantics are the reference's: aliased
    w = pkg.SelfPlayWorker(game, None, num_simulations=16, board_semantics="copied", reference_quirks=False, neural_net=ev,
                           forced_playouts=2.0)
    try:
        assert w.mcts.forced_playouts == 2.0 and w.mcts._context(1).forced_playouts == 2.0
        assert len(w.play_game()) > 0
    finally:
        w.mcts.close()


def test_the_c_abi_refuses_what_it_does_not_support(pkg):
    for kw in (dict(aliased=True), dict(leaves_per_step=2)):
        with pytest.raises(pkg._lib.YYError) as e:
            pkg.engine.BatchedMCTS(2, 4, 4, 8, forced_playouts=2.0, **kw)
        assert e.value.code == -2, e.value                       # YY_E_UNSUPPORTED


def test_k_zero_is_a_context_without_the_option(pkg):
    import torch
    name, budget = "9x12", 24
    R, C = M.SHAPES[name]
    boards, players, noise, _ = M.roots(name)
    out = []
    for kw in (dict(), dict(forced_playouts=0.0), dict(forced_playouts=None)):
        mc = pkg.engine.BatchedMCTS(M.GAMES, R, C, budget, **kw)
        try:
            mc.search(torch.from_numpy(boards).cuda(), torch.from_numpy(players).cuda(), HashEval(), budget,
                      noise=torch.from_numpy(noise).cuda())
            visits, wsum = (t.cpu().numpy() for t in mc.root_stats())
            out.append(root_obs(mc) + (visits, wsum, np.array(list(mc.status().values()))))
        finally:
            mc.close()
    for o in out[1:]:
        for x, y in zip(out[0], o):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    counts, pi = out[0][0], out[0][3]
    assert np.array_equal(pi, counts / counts.sum(1, keepdims=True).astype(np.float64))   # unpruned


# ------------------------------------------------------------------------------------------------ self-play
def play(pkg, shape, free=False, lanes=0, games=12, sims=24, **kw):
    game = pkg.YinYangGame(*shape)
    kw = dict(num_simulations=sims, concurrent_games=8, seed=11, **kw)
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
def lockstep(pkg, shape, cap, k=2.0):
    kw = dict(fast_simulations=8, full_search_probability=0.5) if cap else {}
    if k is not None:
        kw["forced_playouts"] = k
    ex = play(pkg, shape, **kw)
    for a in ex.values():
        a.setflags(write=False)
    return ex


def same(a, b):
    assert a["game_id"].shape == b["game_id"].shape, (a["game_id"].shape, b["game_id"].shape)
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def openings(shape, games, sims, seed=11, alpha=0.3, eps=0.25):
    """The model's search of every game's first move: the empty board, the game's own noise row (tests/philox_ref.py)."""
    import oracle_lib as O
    import philox_ref
    R, C = shape
    empty = np.zeros((R, C), np.int8)
    mask = np.repeat(O.valid_mask(empty[None], [1]), games, 0)
    noise = philox_ref.root_noise(seed, np.arange(games), np.zeros(games, np.int64), np.ones(games), mask, alpha)
    return [M.search(empty, 1, sims, 2.0, noise=noise[g], eps=eps) for g in range(games)]


@pytest.mark.parametrize("shape", [(4, 4), (5, 7)], ids=["4x4", "5x7"])
@pytest.mark.parametrize("cap", [False, True], ids=["full", "playout-cap"])
def test_free_running_plays_the_lockstep_games(pkg, shape, cap):
    """12 games on 8 slots (slots refill).  The feature fires in these games: the model's search of every opening shows a forced
    descent and a pruned edge in at least half of them, and without the cap (every move recorded) the engines' first pi is the
    model's pruned distribution."""
    model = openings(shape, 12, 24)
    assert sum(r.forced > 0 for r in model) >= 6 and sum(bool((r.pruned < r.counts).any()) for r in model) >= 6
    want = lockstep(pkg, shape, cap)
    kw = dict(fast_simulations=8, full_search_probability=0.5) if cap else {}
    same(play(pkg, shape, free=True, forced_playouts=2.0, **kw), want)
    assert len(np.unique(want["game_id"])) == 12
    if not cap:
        first = want["ply"] == 0
        assert first.sum() == 12
        for g, pi in zip(want["game_id"][first], want["policies"][first]):
            assert np.array_equal(pi.astype(np.float32), model[int(g)].pi.astype(np.float32)), g
    plain = lockstep(pkg, shape, cap, k=None)                     # the option changes the games
    assert plain["policies"].shape != want["policies"].shape or not np.array_equal(plain["policies"], want["policies"])


@pytest.mark.parametrize("free", [False, True], ids=["lockstep", "free-running"])
def test_lanes_and_eager_play_the_same_games(pkg, free):
    want = lockstep(pkg, (4, 4), False)
    same(play(pkg, (4, 4), free=free, lanes=2, forced_playouts=2.0), want)
    same(play(pkg, (4, 4), free=free, use_graph=False, forced_playouts=2.0), want)


def test_k_zero_plays_the_games_of_an_engine_without_the_option(pkg):
    want = lockstep(pkg, (4, 4), False, k=None)
    same(play(pkg, (4, 4), forced_playouts=0.0), want)
    same(play(pkg, (4, 4), free=True, forced_playouts=0), want)
