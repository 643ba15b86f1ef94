"""The MCTS solver on the device (include/yy_engine.h YY_FLAG_SOLVER), tolerance 0: integers and the bits of float32 / float64.

(a) the cases of tests/solver_model.py -- 3x3 / 64 simulations (roots get proven), 2x2, 2x4 (a LOSS that needed every child),
    4x4 / 48 from 6-10 stones, 1x6 and 7x1 (pass nodes are never proven), 5x7 / 32 and 9x12 / 16 (two bitboard words) from late
    positions; with root noise, fpu_reduction = 0.2, forced_playouts = 2, per-game budgets of 4 and 16, and tree reuse over
    three moves -- searched on one BatchedMCTS per case and compared with the numpy model: root counts, child W, child priors,
    root visits and W, root_policy, root_proven and the three counters.  tests/test_solver_model.py asserts on the CPU what the
    cases show and that they tell every mutant of the model from it.
(b) the option off: root_proven all zero, the counters zero, the search fpu_model's.
(c) SelfPlayEngine(solver=True): free-running and lockstep return the same examples, with and without the playout cap.
(d) the arena rule: a proven winning root child is played although it is not the most visited one.
(e) the C ABI refuses the flag with K > 1 and on aliased boards, and the readers with a select pending.
Every test here fails without the feature: the keyword does not exist."""
import ctypes
import functools

import numpy as np
import pytest

import fpu_model as F
import solver_model as S
from test_gpu_fpu import KEYS, HashEval, play, root_obs, same
from test_solver_model import ARENA_ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    import yinyang_game_alphazero_amd as p
    return p


def context_keywords(kw):
    out = dict(solver=True)
    if kw.get("r"):
        out["fpu_reduction"] = kw["r"]
    if kw.get("forced"):
        out["forced_playouts"] = kw["forced"]
    return out


@functools.lru_cache(maxsize=None)
def device_run(name):
    """-> per move of case `name`: root_obs, root_policy for T = 1 and T = 0, root_proven and the counters of that search"""
    import torch
    import yinyang_game_alphazero_amd as pkg
    rows, cols, sims, _, kw, eps, moves, budgets, _ = S.CASES[name]
    mc = pkg.engine.BatchedMCTS(S.GAMES, rows, cols, sims, **context_keywords(kw))
    ev = HashEval()
    out = []
    try:
        for t, m in enumerate(S.fixture(name)):
            if t:
                kept = mc.advance(torch.from_numpy(m.actions).cuda()).cpu().numpy()
                assert (kept[m.active != 0] > 0).all(), (name, t, kept, m.active)
            mc.reset_counters()
            mc.search(torch.from_numpy(m.boards).cuda(), torch.from_numpy(m.players).cuda(), ev, m.budgets if budgets else sims,
                      noise=torch.from_numpy(m.noise).cuda() if eps else None, eps=eps,
                      active=torch.from_numpy(m.active).cuda() if t else None)
            root, child = (x.cpu().numpy() for x in mc.root_proven())
            out.append(root_obs(mc) + (mc.root_policy().cpu().numpy(), mc.root_policy(temperature_zero=True).cpu().numpy(), root, child,
                                       mc.solver_counters(), mc.status()["evals"]))
    finally:
        mc.close()
    return out


@pytest.mark.parametrize("name", list(S.CASES))
def test_the_search_equals_the_model(name):
    got, want = device_run(name), S.fixture(name)
    forced = S.CASES[name][4].get("forced", 0.0)
    assert len(got) == len(want)
    for t, (o, m) in enumerate(zip(got, want)):
        counts, cw, cp, visits, wsum, pi, pi0, root, child, ctr, evals = o
        rs = [r for r in m.results if r is not None]
        for g, r in enumerate(m.results):
            where = (name, "move", t, "game", g)
            if r is None:
                assert root[g] == 0 and not child[g].any(), where
                continue
            assert np.array_equal(counts[g], r.counts), (where, counts[g], r.counts)
            assert np.array_equal(cw[g].view(np.uint32), r.child_w.view(np.uint32)), where
            assert np.array_equal(cp[g].view(np.uint32), r.child_p.view(np.uint32)), where
            assert visits[g] == r.root_visits, where
            assert np.float64(wsum[g]).tobytes() == np.float64(r.root_w).tobytes(), (where, wsum[g], r.root_w)
            assert pi[g].tobytes() == S.root_policy(r, forced).tobytes(), where      # forced playouts: on the pruned counts
            assert pi0[g].tobytes() == S.root_policy(r, forced, tzero=True).tobytes(), where
            assert root[g] == r.root_proven, (where, root[g], r.root_proven)
            assert child.dtype == np.int8 and np.array_equal(child[g], r.child_proven), (where, child[g], r.child_proven)
        assert ctr == dict(proven_nodes=sum(r.proven_nodes for r in rs), proven_descents=sum(r.proven_descents for r in rs),
                           proven_roots=sum(r.proven_roots for r in rs)), (name, t, ctr)
        assert evals == sum(r.evals for r in rs), (name, t)         # a descent that ended on a proven node asked for no row


def test_the_option_off_is_todays_search(pkg):
    import torch
    rows, cols, sims = 3, 3, 64
    m = S.fixture("3x3")[0]
    out = []
    for kw in (dict(), dict(solver=False)):
        mc = pkg.engine.BatchedMCTS(S.GAMES, rows, cols, sims, **kw)
        try:
            mc.search(torch.from_numpy(m.boards).cuda(), torch.from_numpy(m.players).cuda(), HashEval(), sims)
            root, child = (x.cpu().numpy() for x in mc.root_proven())
            assert not root.any() and not child.any() and root.shape == (S.GAMES,) and child.shape == (S.GAMES, rows * cols)
            assert mc.solver_counters() == dict(proven_nodes=0, proven_descents=0, proven_roots=0)
            out.append(root_obs(mc) + (mc.root_policy().cpu().numpy(), np.array(list(mc.status().values()))))
        finally:
            mc.close()
    for x, y in zip(*out):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for g in range(S.GAMES):
        r = F.search(m.boards[g], m.players[g], sims)
        assert np.array_equal(out[0][0][g], r.counts) and np.array_equal(out[0][1][g].view(np.uint32), r.child_w.view(np.uint32))
        assert out[0][3][g] == r.root_visits and np.float64(out[0][4][g]).tobytes() == np.float64(r.root_w).tobytes()


@pytest.mark.parametrize("cap", [dict(), dict(fast_simulations=4, full_search_probability=0.5)], ids=["full", "playout-cap"])
def test_free_running_plays_the_lockstep_games(pkg, cap):
    want, wstats = play(pkg, (4, 4), 8, 20, 16, False, solver=True, **cap)
    got, gstats = play(pkg, (4, 4), 8, 20, 16, True, solver=True, **cap)
    assert len(np.unique(want["game_id"])) == 20
    same(got, want)
    for k in ("positions", "recorded", "games_finished"):
        assert gstats[k] == wstats[k], (k, gstats[k], wstats[k])
    plain, pstats = play(pkg, (4, 4), 8, 20, 16, False, **cap)
    if not cap:                                                     # full searches: the option changes the games
        assert plain["policies"].shape != want["policies"].shape or not np.array_equal(plain["policies"], want["policies"])
    same(play(pkg, (4, 4), 8, 20, 16, True, solver=False, **cap)[0], plain)


def test_the_engine_counts_its_proofs(pkg):
    game = pkg.YinYangGame(4, 4)
    eng = pkg.SelfPlayEngine(game, HashEval(), num_simulations=16, concurrent_games=8, seed=11, solver=True)
    try:
        eng.run(20)
        ctr = eng.ctx.solver_counters()
        assert ctr["proven_nodes"] > 0 and ctr["proven_descents"] > 0, ctr
    finally:
        eng.close()


def test_the_player_and_the_arena_play_the_proven_win(pkg):
    rows, cols, plies, seed = ARENA_ROOT
    board, player = F.random_root(rows, cols, plies, seed)
    on, off = S.search(board, player, 64), S.search(board, player, 64, solver=False)
    win, most = S.winning_move(on), int(np.argmax(on.counts))
    assert win >= 0 and win != most
    game = pkg.YinYangGame(rows, cols)
    for solver, want in ((True, win), (False, int(np.argmax(off.counts)))):
        m = pkg.MCTS(game, HashEval(), num_simulations=64, board_semantics="copied", dirichlet_noise=False, verbose=0, solver=solver)
        try:
            b = game.getInitBoard()
            b.board[...] = board
            pi, _ = m.search(b, player)
            r = on if solver else off
            assert np.array_equal(pi, S.root_policy(r)), solver
            ctx = m._ctx[1]
            picked = int(pkg.arena.proven_winning_move(ctx)[0]) if solver else -1
            assert picked == (win if solver else -1)
            # the player's rule: the proven win when there is one, else the most visited move
            assert (picked if picked >= 0 else int(np.argmax(pi))) == want
            if solver:
                a = pkg.Arena(game, HashEval(), HashEval(), num_simulations=64, solver=True)
                assert a.solver and int(a._move(ctx)[0]) == win
                assert int(pkg.Arena(game, HashEval(), HashEval(), num_simulations=64)._move(ctx)[0]) == most
        finally:
            m.close()
    # AlphaZeroPlayer.play itself, its network replaced by the model's evaluator: the proven win with the option, the most
    # visited move without, and with tree_reuse the re-rooting that follows the move does not disturb it
    for kw, want in ((dict(solver=True), win), (dict(solver=True, tree_reuse=True), win), (dict(), int(np.argmax(off.counts)))):
        player_ = pkg.AlphaZeroPlayer(game, "no-such-model.pth.tar", num_simulations=64, **kw)
        try:
            player_.mcts.neural_net = HashEval()
            player_.mcts.use_dirichlet = False
            b = game.getInitBoard()
            b.board[...] = board
            assert player_.play(b, player) == want, kw
        finally:
            player_.mcts.close()
    res = pkg.Arena(game, HashEval(), HashEval(), num_simulations=32, solver=True, tree_reuse=True).play(4)
    assert res["games"] == 4
    with pytest.raises(ValueError):
        pkg.Arena(game, HashEval(), HashEval(), num_simulations=32, solver=True, leaves_per_step=4)
    with pytest.raises(ValueError):
        pkg.Arena(game, HashEval(), HashEval(), num_simulations=32, solver=True, literal=True)


def test_the_c_abi_refuses_what_the_option_does_not_go_with(pkg):
    L = pkg._lib
    for flags, K in ((L.FLAG_SOLVER, 4), (L.FLAG_SOLVER | L.FLAG_ALIASED, 1)):
        cfg = L.MctsConfig(2, 4, 4, 8, 1.0, flags, 0, 0, K, 0, 0.0, 0.0, 0.0)
        h = ctypes.c_void_p()
        assert L.lib().yy_mcts_create(ctypes.byref(cfg), ctypes.byref(h)) == -2     # YY_E_UNSUPPORTED
        assert b"SOLVER" in L.lib().yy_last_error()
    for kw in (dict(leaves_per_step=4), dict(aliased=True)):
        with pytest.raises(L.YYError) as e:
            pkg.engine.BatchedMCTS(2, 4, 4, 8, solver=True, **kw)
        assert e.value.code == -2
    import torch
    mc = pkg.engine.BatchedMCTS(2, 4, 4, 8, solver=True)
    try:
        mc.begin(torch.zeros((2, 4, 4), dtype=torch.int8).cuda(), torch.ones(2, dtype=torch.int8).cuda())
        for call in (mc.root_proven, mc.solver_counters):             # a root expansion is pending
            with pytest.raises(L.YYError) as e:
                call()
            assert e.value.code == -5                                 # YY_E_STATE
        pol, _ = HashEval()(mc.planes)
        mc.expand_root(pol)
        assert not mc.root_proven()[0].cpu().numpy().any()
        mc.select()
        with pytest.raises(L.YYError):                                # a select is pending
            mc.root_proven()
    finally:
        mc.close()
