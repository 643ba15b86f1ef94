"""Gumbel root search on the device (include/yy_engine.h YY_FLAG_GUMBEL_ROOT) against tests/gumbel_model.py.

Draw: engine.gumbel_rows against the float64 formula over tests/philox_ref.py.  Search pin: after EVERY simulation of a search
the root children's N and W (raw bits), root_gumbel() and root_gumbel_action() equal the model's, bit for bit; the model takes
the device's base scores s0 as its input, so no selection depends on a libm.  pi': root_policy() (float64) against the model's
softmax, which differs through the device's exp / log only.  Engines: free-running self-play equals lockstep example for example,
two lanes equal one, evaluation reuse off equals on, every recorded pi row is the model's and every move played the Gumbel winner.
Every test here fails without the feature: the keyword does not exist."""
import functools

import numpy as np
import pytest

import gumbel_model as M
from hash_eval import hash_eval_torch

pytestmark = pytest.mark.gpu
KEYS = ("states", "policies", "values", "game_id", "ply")
# pi' against the model: the largest relative difference measured over every case of this file on an MI355X (the first run, kept
# in profiles/gumbel_root.json) was PI_MEASURED; the bound is 16 times that, and never looser than 1e-12
PI_MEASURED = 8.04e-16
PI_BOUND = min(16 * PI_MEASURED, 1e-12)
_seen = {"pi_rel": 0.0}


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    import yinyang_game_alphazero_amd as p
    return p


class HashEval:
    """The exact hash evaluator: a pure function of the row.  zero: (row, action) whose prior is returned as exactly 0 by the
    FIRST call (the root call of an eager search), and by no later one."""
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


# ------------------------------------------------------------------------------------------------ the draw
def test_gumbel_rows_are_the_formula_over_philox(pkg):
    """The device rounds -log(-log(u)) of ITS float64 log to float32.  The existing root-noise test allows the device's log 1e-13
    relative; here the same 1e-13 (of max(1, |g|): g passes through 0) plus the float32 rounding of the result, half an ulp."""
    import torch
    gid = torch.tensor([0, 1, 7, 123456789012, 1], dtype=torch.int64).cuda()
    ply = torch.tensor([0, 0, 3, 200, 9], dtype=torch.int32).cuda()
    A = 144
    got = pkg.engine.gumbel_rows(77, gid, ply, A).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (5, A) and np.isfinite(got).all()
    worst = 0.0
    for i, (g, p) in enumerate(zip(gid.tolist(), ply.tolist())):
        for a in range(A):
            want = M.gumbel(77, g, p, a)[1]
            err = abs(float(got[i, a]) - want)
            tol = 1e-13 * max(1.0, abs(want)) + 0.5 * float(np.spacing(np.float32(abs(want))))
            worst = max(worst, err / tol)
            assert err <= tol, (g, p, a, got[i, a], want)
    print("gumbel rows: worst error / tolerance", worst)
    # a game's row does not depend on its slot or batch
    perm = torch.tensor([4, 2, 0, 3, 1]).cuda()
    again = pkg.engine.gumbel_rows(77, gid[perm].contiguous(), ply[perm].contiguous(), A).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), got[perm.cpu().numpy()].view(np.uint32))
    one = pkg.engine.gumbel_rows(77, gid[2:3].contiguous(), ply[2:3].contiguous(), A).cpu().numpy()
    assert np.array_equal(one[0].view(np.uint32), got[2].view(np.uint32))
    assert not np.array_equal(got[1], got[4]) and not np.array_equal(got[0], got[1])


# ------------------------------------------------------------------------------------------------ the search, step by step
def pin(pkg, shape, n, m, budgets=None, zero=None, games=M.GAMES):
    """One search of `games` roots, one simulation at a time (select / expand_backup, the kernels of the fused step), compared
    with the model after every simulation.  -> the largest relative difference of pi' seen"""
    import torch
    R, C = shape
    A = R * C
    boards, players = M.roots(shape, games)
    ev = HashEval(zero)
    mc = pkg.engine.BatchedMCTS(games, R, C, n, gumbel_root=m)
    worst = 0.0
    try:
        rows = pkg.engine.gumbel_rows(M.SEED, torch.arange(games, dtype=torch.int64).cuda(),
                                      torch.zeros(games, dtype=torch.int32).cuda(), A)
        mc.set_gumbel(rows)
        if budgets is None:
            mc.set_num_sims(n)
        else:
            mc.set_sim_budgets(torch.tensor(budgets, dtype=torch.int32).cuda())
        mc.begin(torch.from_numpy(boards).cuda(), torch.from_numpy(players).cuda())
        mc.expand_root(ev(mc.planes)[0])
        s0 = mc.root_gumbel().cpu().numpy()
        model = []
        for g in range(games):
            s = M.Search(boards[g], players[g], n if budgets is None else budgets[g], m,
                         zero_prior=zero[1] if zero is not None and zero[0] == g else None)
            legal = np.zeros(A, bool)
            legal[[e.action for e in s.root.edges]] = True
            assert np.isnan(s0[g][~legal]).all() and not np.isnan(s0[g][legal]).any(), g
            # the device's s0 is f32(g + log P) up to its own log: one float32 ulp of the host's
            s.host_s0(rows[g].cpu().numpy())
            host = np.array(s.s0)
            dev = s0[g][legal]
            fin = np.isfinite(host)
            assert np.array_equal(np.isneginf(host), np.isneginf(dev)), g
            assert (np.abs(dev[fin] - host[fin]) <= np.spacing(np.abs(host[fin]))).all(), g
            s.set_s0(s0[g])
            model.append(s)
        for step in range(n):
            mc.select()
            mc.expand_backup(*ev(mc.planes))
            counts, cw, _ = (t.cpu().numpy() for t in mc.root_counts(with_children=True))
            act = mc.root_gumbel_action().cpu().numpy()
            pi = mc.root_policy().cpu().numpy()
            pi0 = mc.root_policy(temperature_zero=True).cpu().numpy()
            assert np.array_equal(mc.root_gumbel().cpu().numpy().view(np.uint32), s0.view(np.uint32))
            for g, s in enumerate(model):
                s.step()
                where = (shape, n, m, "game", g, "after simulation", step + 1)
                assert np.array_equal(counts[g], s.counts()), (where, counts[g], s.counts())
                assert np.array_equal(cw[g].view(np.uint32), s.child_w().view(np.uint32)), where
                assert act[g] == s.winner(), (where, act[g], s.winner())
                want = s.policy()
                assert np.array_equal(pi[g].view(np.uint64), pi0[g].view(np.uint64)), where     # both temperatures
                assert np.array_equal(want == 0.0, pi[g] == 0.0), where
                nz = want > 0
                rel = float(np.max(np.abs(pi[g][nz] - want[nz]) / want[nz]))
                worst = max(worst, rel)
                assert rel <= PI_BOUND, (where, rel)
                assert abs(pi[g].sum() - 1.0) < 1e-12
        visits = mc.root_stats()[0].cpu().numpy()
        assert np.array_equal(visits, [s.sims for s in model])
        mc.status()
    finally:
        mc.close()
    _seen["pi_rel"] = max(_seen["pi_rel"], worst)
    print("pi' largest relative difference", shape, n, m, worst, "so far", _seen["pi_rel"])
    return model


@pytest.mark.parametrize("name,shape,n,m", M.CASES, ids=[c[0] for c in M.CASES])
def test_every_simulation_equals_the_model(pkg, name, shape, n, m):
    model = pin(pkg, shape, n, m)
    for s in model:
        k = len(s.root.edges)
        assert int((s.counts() > 0).sum()) == min(m, k, n)


def test_per_game_budgets_in_one_batch(pkg):
    """budgets 4 and 16 side by side: every game halves over ITS budget, and a game whose budget is spent stands still"""
    model = pin(pkg, (4, 4), 16, 4, budgets=[4, 16, 16, 4])
    assert [s.sims for s in model] == [4, 16, 16, 4]


def test_a_child_with_prior_zero(pkg):
    """The evaluator returns exactly 0 for action 5 of game 0's root: s0 = -inf on the device, the child is still considered
    (k <= m), visited in its turn, gets no mass in pi' and is never the move."""
    model = pin(pkg, (4, 4), 16, 16, zero=(0, 5))
    s = model[0]
    i = [e.action for e in s.root.edges].index(5)
    assert s.s0[i] == -np.inf and s.root.edges[i].N >= 1 and s.policy()[5] == 0.0


def test_the_fused_search_is_the_stepwise_one(pkg):
    """BatchedMCTS.search (fused steps; run_search hands the budget to the context) ends where the stepwise search ends"""
    import torch
    shape, n, m = (5, 7), 24, 16
    model = pin(pkg, shape, n, m)
    boards, players = M.roots(shape)
    mc = pkg.engine.BatchedMCTS(M.GAMES, *shape, n, gumbel_root=m)
    try:
        with pytest.raises(pkg._lib.YYError):                                   # no rows set: YY_E_STATE, not a wild read
            mc.search(torch.from_numpy(boards).cuda(), torch.from_numpy(players).cuda(), HashEval(), n)
        mc.set_gumbel(pkg.engine.gumbel_rows(M.SEED, torch.arange(M.GAMES, dtype=torch.int64).cuda(),
                                             torch.zeros(M.GAMES, dtype=torch.int32).cuda(), shape[0] * shape[1]))
        mc.search(torch.from_numpy(boards).cuda(), torch.from_numpy(players).cuda(), HashEval(), n)
        counts = mc.root_counts().cpu().numpy()
        act = mc.root_gumbel_action().cpu().numpy()
        for g, s in enumerate(model):
            assert np.array_equal(counts[g], s.counts()) and act[g] == s.winner()
        with pytest.raises(pkg._lib.YYError) as e:                              # tree reuse is refused on such a context
            mc.advance(torch.from_numpy(act).cuda())
        assert e.value.code == -2
    finally:
        mc.close()


def test_the_c_abi_refuses_what_it_does_not_support(pkg):
    for kw in (dict(leaves_per_step=2), dict(aliased=True), dict(forced_playouts=2.0), dict(solver=True)):
        with pytest.raises(pkg._lib.YYError) as e:
            pkg.engine.BatchedMCTS(2, 4, 4, 8, gumbel_root=4, **kw)
        assert e.value.code == -2, e.value                                      # YY_E_UNSUPPORTED
    L = pkg._lib
    for m, cv, cs in ((1, 50.0, 1.0), (65, 50.0, 1.0), (4, -1.0, 1.0), (4, 50.0, 0.0)):
        cfg = L.MctsConfig(2, 4, 4, 8, 1.0, L.FLAG_GUMBEL_ROOT, 0, 0, 1, 0, 0.0, 0.0, 0.0, m, cv, cs)
        import ctypes
        h = ctypes.c_void_p()
        assert L.lib().yy_mcts_create(ctypes.byref(cfg), ctypes.byref(h)) == -1          # YY_E_INVALID
    mc = pkg.engine.BatchedMCTS(2, 4, 4, 8)
    try:
        with pytest.raises(pkg._lib.YYError):
            mc.root_gumbel()
        with pytest.raises(pkg._lib.YYError):
            mc.root_gumbel_action()
    finally:
        mc.close()


# ------------------------------------------------------------------------------------------------ self-play
ENGINE_CASES = {"4x4": ((4, 4), 8, 20, 16), "1x6": ((1, 6), 4, 6, 8)}         # board, slots, games, simulations
VARIANTS = {"plain": {}, "playout-cap": dict(fast_simulations=4, full_search_probability=0.5),
            "symmetry": dict(evaluation_symmetry="random")}
SP_M, SP_SEED = 4, 11


def play(pkg, case, free=False, lanes=0, **kw):
    shape, slots, games, sims = ENGINE_CASES[case]
    game = pkg.YinYangGame(*shape)
    kw = dict(num_simulations=sims, concurrent_games=slots, seed=SP_SEED, gumbel_root=SP_M, dirichlet_epsilon=0.0, **kw)
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
def lockstep(pkg, case, variant):
    ex = play(pkg, case, **VARIANTS[variant])
    for a in ex.values():
        a.setflags(write=False)
    return ex


def same(a, b):
    assert a["game_id"].shape == b["game_id"].shape, (a["game_id"].shape, b["game_id"].shape)
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_free_running_plays_the_lockstep_games(pkg, case, variant):
    want = lockstep(pkg, case, variant)
    assert len(np.unique(want["game_id"])) == ENGINE_CASES[case][2]
    same(play(pkg, case, free=True, **VARIANTS[variant]), want)


def test_the_option_changes_the_games_and_off_is_the_engine_without_it(pkg):
    shape, slots, games, sims = ENGINE_CASES["4x4"]
    out = []
    for kw in (dict(), dict(gumbel_root=None), dict(gumbel_root=0)):
        eng = pkg.SelfPlayEngine(pkg.YinYangGame(*shape), HashEval(), num_simulations=sims, concurrent_games=slots, seed=SP_SEED,
                                 dirichlet_epsilon=0.0, **kw)
        try:
            ex = pkg.self_play.sort_examples(eng.run(games))
        finally:
            eng.close()
        out.append({k: ex[k].cpu().numpy() for k in KEYS})
    same(out[1], out[0])
    same(out[2], out[0])
    want = lockstep(pkg, "4x4", "plain")
    assert want["policies"].shape != out[0]["policies"].shape or not np.array_equal(want["policies"], out[0]["policies"])


@pytest.mark.parametrize("free", [False, True], ids=["lockstep", "free-running"])
def test_two_lanes_equal_one_and_reuse_off_equals_on(pkg, free):
    want = lockstep(pkg, "4x4", "plain")
    same(play(pkg, "4x4", free=free, lanes=2), want)
    same(play(pkg, "4x4", free=free, reuse_pass_value=False, reuse_transpositions=False, keep_evaluations=False), want)
    same(play(pkg, "4x4", free=free, use_graph=False), want)


@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_every_recorded_pi_is_the_models_and_every_move_the_winner(pkg, case):
    """The games of the plain lockstep run are replayed on the host (the side to move follows from the pass rule), every
    recorded position is searched by the model on the device's own base scores for (game, ply), and the model's pi' -- rounded
    to float32 like the record, so one float32 ulp -- and its winner are what the engine recorded and played."""
    import oracle_lib as O
    import torch
    shape, slots, games, sims = ENGINE_CASES[case]
    A = shape[0] * shape[1]
    ex = lockstep(pkg, case, "plain")
    n = len(ex["ply"])
    players = np.zeros(n, np.int8)
    moves = np.full(n, -1)
    for gid in np.unique(ex["game_id"]):
        idx = np.flatnonzero(ex["game_id"] == gid)
        assert np.array_equal(ex["ply"][idx], np.arange(len(idx)))
        p = 1
        for j, i in enumerate(idx):
            b = ex["states"][i]
            if not O.valid_mask(b[None], [p])[0].any():
                p = -p                                                          # a pass: the other side searches this position
            players[i] = p
            if j + 1 < len(idx):
                d = np.flatnonzero((ex["states"][idx[j + 1]] != b).ravel())
                assert len(d) == 1 and ex["states"][idx[j + 1]].flat[d[0]] == p
                moves[i] = d[0]
            p = -p
    mc = pkg.engine.BatchedMCTS(n, *shape, sims, gumbel_root=SP_M)
    try:
        mc.set_gumbel(pkg.engine.gumbel_rows(SP_SEED, torch.from_numpy(ex["game_id"].copy()).cuda(),
                                             torch.from_numpy(ex["ply"].astype(np.int32)).cuda(), A))
        mc.set_num_sims(sims)
        mc.begin(torch.from_numpy(ex["states"].copy()).cuda(), torch.from_numpy(players).cuda())
        mc.expand_root(HashEval()(mc.planes)[0])
        s0 = mc.root_gumbel().cpu().numpy()
    finally:
        mc.close()
    checked = 0
    for i in range(n):
        s = M.Search(ex["states"][i], players[i], sims, SP_M)
        s.set_s0(s0[i])
        s.run()
        want = s.policy().astype(np.float32)
        got = ex["policies"][i]
        assert np.array_equal(want == 0, got == 0), i
        assert (np.abs(got - want) <= np.spacing(want)).all(), (i, got, want)
        if moves[i] >= 0:
            assert s.winner() == moves[i], (i, s.winner(), moves[i])
            checked += 1
    assert checked >= n - games


def test_mcts_and_the_worker_take_the_option(pkg):
    """MCTS(gumbel_root=m) draws its own rows per search, returns pi' and the winner; SelfPlayWorker plays the winner"""
    game = pkg.YinYangGame(4, 4)
    ev = HashEval()
    m = pkg.MCTS(game, ev, num_simulations=16, board_semantics="copied", gumbel_root=4, dirichlet_noise=False, verbose=0,
                 gumbel_seed=3)
    try:
        board = game.getInitBoard()
        pi, root = m.search(board, 1)
        ctx = m._context(1)
        s = M.Search(np.zeros((4, 4), np.int8), 1, 16, 4)
        s.set_s0(ctx.root_gumbel().cpu().numpy()[0])
        s.run()
        assert all(root.children[a].visits == s.counts()[a] for a in root.children)
        assert m.gumbel_action() == s.winner() and np.allclose(pi, s.policy(), rtol=PI_BOUND, atol=0)
        first = ctx._gumbel.cpu().numpy().copy()
        m.search(board, 1)
        assert not np.array_equal(first, ctx._gumbel.cpu().numpy())             # the per-search counter keys the rows
        m.temperature = 0.5
        with pytest.raises(ValueError):
            m.search(board, 1)
    finally:
        m.close()
    with pytest.raises(ValueError):
        pkg.MCTS(game, ev, gumbel_root=4)                                       # the default board semantics: aliased
    w = pkg.SelfPlayWorker(game, None, num_simulations=8, board_semantics="copied", reference_quirks=False, neural_net=ev,
                           gumbel_root=4, dirichlet_epsilon=0.0)
    try:
        assert w.mcts._context(1).gumbel_root == 4 and len(w.play_game()) > 0
    finally:
        w.mcts.close()
