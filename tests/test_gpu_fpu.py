"""First-play urgency reduction on the device (include/yy_engine.h YY_FLAG_FPU_REDUCTION), tolerance 0: integers and the bits
of float32 / float64.

(a) the cases of tests/fpu_model.py -- 4x4 / 32 simulations, 5x7 / 48, 1x6 and 7x1 (pass roots, finished games, childless
    nodes), 9x12 / 16 (two bitboard words) and 12x12 / 16 (three; up to 144 children, so the wave reductions run over three
    64-lane strides); with root noise, with fpu_reduction_root = 0, with K = 4 (virtual visits), with tree reuse over three
    moves, with forced playouts k = 2 and on aliased boards -- searched on one BatchedMCTS per case and compared with the numpy
    model: root counts, child W, child priors, root visits and root W.  tests/test_fpu_model.py asserts on the CPU that every
    case differs from the search without the option and that the cases tell every mutant of the model from it.  The evaluator
    is the exact hash evaluator with its priors times 32 (forced_playouts_model.PSCALE).
(b) r = 0 / None is a context created without the keyword.
(c) SelfPlayEngine(fpu_reduction=0.25): free-running and lockstep return the same examples; evaluation reuse on and off and
    the two-stone book play the same games (the cache and the book hold evaluator outputs only).
(d) Arena and evaluate_vs_random take the keyword, and the first move of a match is the model's with and without it.
Every test here fails without the feature: the keyword does not exist."""
import functools

import numpy as np
import pytest

import fpu_model as M
from hash_eval import hash_eval_torch

pytestmark = pytest.mark.gpu
KEYS = ("states", "policies", "values", "game_id", "ply")


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
    visits, wsum = (t.cpu().numpy() for t in mc.root_stats())
    return counts, cw, cp, visits, wsum


def context_keywords(kw):
    out = dict(fpu_reduction=kw["r"], leaves_per_step=kw.get("K", 1), aliased=kw.get("aliased", False))
    if "r_root" in kw:
        out["fpu_reduction_root"] = kw["r_root"]
    if kw.get("forced"):
        out["forced_playouts"] = kw["forced"]
    return out


@functools.lru_cache(maxsize=None)
def device_run(name):
    """-> per move of case `name`: root_obs after the search (and the aliased board where there is one)"""
    import torch
    import yinyang_game_alphazero_amd as pkg
    rows, cols, sims, kw, eps, moves = M.CASES[name]
    mc = pkg.engine.BatchedMCTS(M.GAMES, rows, cols, sims, **context_keywords(kw))
    ev = HashEval()
    out = []
    try:
        for t, m in enumerate(M.fixture(name)):
            if t:
                kept = mc.advance(torch.from_numpy(m.actions).cuda()).cpu().numpy()
                assert (kept[m.active != 0] > 0).all(), (name, t, kept, m.active)
            mc.search(torch.from_numpy(m.boards).cuda(), torch.from_numpy(m.players).cuda(), ev, sims,
                      noise=torch.from_numpy(m.noise).cuda() if eps else None, eps=eps,
                      active=torch.from_numpy(m.active).cuda() if t else None)
            out.append(root_obs(mc) + ((mc.boards().cpu().numpy(),) if kw.get("aliased") else ()))
        mc.status()
    finally:
        mc.close()
    return out


@pytest.mark.parametrize("name", list(M.CASES))
def test_the_search_equals_the_model(name):
    got, want = device_run(name), M.fixture(name)
    assert len(got) == len(want)
    for t, (o, m) in enumerate(zip(got, want)):
        counts, cw, cp, visits, wsum = o[:5]
        for g, r in enumerate(m.results):
            if r is None:
                continue
            where = (name, "move", t, "game", g)
            assert np.array_equal(counts[g], r.counts), (where, counts[g], r.counts)
            assert np.array_equal(cw[g].view(np.uint32), r.child_w.view(np.uint32)), where
            assert np.array_equal(cp[g].view(np.uint32), r.child_p.view(np.uint32)), where
            assert visits[g] == r.root_visits, where
            assert np.float64(wsum[g]).tobytes() == np.float64(r.root_w).tobytes(), (where, wsum[g], r.root_w)
            if len(o) > 5:
                assert np.array_equal(o[5][g], r.final_board), where


@pytest.mark.parametrize("kw", [dict(), dict(leaves_per_step=4), dict(aliased=True)], ids=["copied", "K4", "aliased"])
def test_r_zero_is_a_context_without_the_option(pkg, kw):
    import torch
    rows, cols, sims = 9, 12, 16
    m = M.fixture("9x12")[0]
    noise = np.stack([M.dirichlet_noise(b, p, [7, g]) for g, (b, p) in enumerate(zip(m.boards, m.players))])
    out = []
    for fk in (dict(), dict(fpu_reduction=0.0), dict(fpu_reduction=None), dict(fpu_reduction=0, fpu_reduction_root=0.0)):
        mc = pkg.engine.BatchedMCTS(M.GAMES, rows, cols, sims, **kw, **fk)
        try:
            mc.search(torch.from_numpy(m.boards).cuda(), torch.from_numpy(m.players).cuda(), HashEval(), sims,
                      noise=torch.from_numpy(noise).cuda())
            out.append(root_obs(mc) + (mc.root_policy().cpu().numpy(), np.array(list(mc.status().values()))))
        finally:
            mc.close()
    for o in out[1:]:
        for x, y in zip(out[0], o):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # and that search is the model's without the option
    for g in range(M.GAMES):
        r = M.search(m.boards[g], m.players[g], sims, noise=noise[g], K=kw.get("leaves_per_step", 1), aliased=kw.get("aliased", False))
        assert np.array_equal(out[0][0][g], r.counts) and np.array_equal(out[0][1][g].view(np.uint32), r.child_w.view(np.uint32))


def test_the_c_abi_checks_the_two_values(pkg):
    for fk in (dict(fpu_reduction=float("inf")), dict(fpu_reduction=-0.5), dict(fpu_reduction=0.2, fpu_reduction_root=-1.0),
               dict(fpu_reduction=0.0, fpu_reduction_root=0.2), dict(fpu_reduction=float("nan"))):
        with pytest.raises(ValueError) as e:
            pkg.engine.BatchedMCTS(2, 4, 4, 8, **fk)
        assert e.value.option == "fpu_reduction"
    cfg = pkg._lib.MctsConfig(2, 4, 4, 8, 1.0, pkg._lib.FLAG_FPU_REDUCTION, 0, 0, 1, 0, 0.0, 0.0, 0.0)
    import ctypes
    h = ctypes.c_void_p()
    assert pkg._lib.lib().yy_mcts_create(ctypes.byref(cfg), ctypes.byref(h)) == -1     # YY_E_INVALID: the flag with r == 0
    mc = pkg.engine.BatchedMCTS(2, 4, 4, 8, fpu_reduction=0.2)
    assert (mc.fpu_reduction, mc.fpu_reduction_root) == (0.2, 0.2)
    mc.close()


# ------------------------------------------------------------------------------------------------ self-play
def play(pkg, shape, G, games, sims, free, lanes=0, ev=None, **kw):
    """One run -> (examples sorted by (game_id, ply) as numpy arrays, the engine's counters)."""
    game = pkg.YinYangGame(*shape)
    ev = HashEval() if ev is None else ev
    kw = dict(num_simulations=sims, concurrent_games=G, seed=11, **kw)
    if free:
        kw["free_running"] = True
    eng = pkg.SelfPlayLanes(game, ev, lanes=lanes, **kw) if lanes else pkg.SelfPlayEngine(game, ev, **kw)
    try:
        ex = pkg.self_play.sort_examples(eng.run(games))
        stats = dict(positions=eng.positions, recorded=eng.recorded, games_finished=eng.games_finished, evals=eng.ctx.status()["evals"])
    finally:
        eng.close()
    return {k: ex[k].cpu().numpy() for k in KEYS}, stats


@functools.lru_cache(maxsize=None)
def lockstep(pkg, r, **kw):
    """The reference run -- 4x4, 8 slots, 20 games, 16 simulations -- computed once per configuration and left unchanged."""
    ex, stats = play(pkg, (4, 4), 8, 20, 16, False, **(dict(fpu_reduction=r) if r is not None else {}), **kw)
    for a in ex.values():
        a.setflags(write=False)
    return ex, stats


def same(a, b):
    assert a["game_id"].shape == b["game_id"].shape, (a["game_id"].shape, b["game_id"].shape)
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def test_free_running_plays_the_lockstep_games(pkg):
    want, wstats = lockstep(pkg, 0.25)
    got, gstats = play(pkg, (4, 4), 8, 20, 16, True, fpu_reduction=0.25)
    assert len(np.unique(want["game_id"])) == 20
    same(got, want)
    for k in ("positions", "recorded", "games_finished"):
        assert gstats[k] == wstats[k], (k, gstats[k], wstats[k])
    plain, _ = lockstep(pkg, None)                                  # the option changes the games
    assert plain["policies"].shape != want["policies"].shape or not np.array_equal(plain["policies"], want["policies"])
    same(play(pkg, (4, 4), 8, 20, 16, False, fpu_reduction=0.0)[0], plain)
    same(play(pkg, (4, 4), 8, 20, 16, True, fpu_reduction=None, fpu_reduction_root=None)[0], plain)


def test_the_first_recorded_policy_is_the_models(pkg):
    """Every game's first search: the empty board, the game's own noise row (tests/philox_ref.py), r at the root too."""
    import oracle_lib as O
    import philox_ref
    want, _ = lockstep(pkg, 0.25)
    empty = np.zeros((4, 4), np.int8)
    mask = np.repeat(O.valid_mask(empty[None], [1]), 20, 0)
    noise = philox_ref.root_noise(11, np.arange(20), np.zeros(20, np.int64), np.ones(20), mask, 0.3)
    first = want["ply"] == 0
    assert first.sum() == 20
    for g, pi in zip(want["game_id"][first], want["policies"][first]):
        r = M.search(empty, 1, 16, r=0.25, noise=noise[int(g)], pscale=M.PSCALE)
        assert np.array_equal(pi, r.counts / np.float64(r.counts.sum())), g


@pytest.mark.parametrize("free", [False, True], ids=["lockstep", "free-running"])
def test_evaluation_reuse_and_the_book_hold_nothing_of_the_option(pkg, free):
    """The evaluation cache and the book hold evaluator outputs, which the option does not touch: the games with reuse off,
    with reuse on (the engine's default with a row-independent evaluator) and with a two-stone book are the same games; reuse
    and the book only save evaluator rows."""
    want, wstats = lockstep(pkg, 0.25)
    off, ostats = play(pkg, (4, 4), 8, 20, 16, free, fpu_reduction=0.25, reuse_pass_value=False, reuse_transpositions=False,
                       keep_evaluations=False)
    same(off, want)
    book, bstats = play(pkg, (4, 4), 8, 20, 16, free, fpu_reduction=0.25, opening_book=2)
    same(book, want)
    assert bstats["evals"] <= wstats["evals"] <= ostats["evals"], (bstats, wstats, ostats)


def test_a_book_and_a_cache_serve_contexts_with_and_without_the_option(pkg):
    """One OpeningBook object, built once, handed to an engine with the option and to one without: each plays the games it
    plays without a book."""
    ev = HashEval()
    book = pkg.engine.OpeningBook(4, 4, ev, 2)
    for r in (0.25, None):
        want, _ = lockstep(pkg, r)
        same(play(pkg, (4, 4), 8, 20, 16, False, ev=ev, opening_book=book, **(dict(fpu_reduction=r) if r else {}))[0], want)


def test_lanes_k4_and_the_playout_cap_take_the_option(pkg):
    want, _ = lockstep(pkg, 0.25)
    same(play(pkg, (4, 4), 8, 20, 16, False, lanes=2, fpu_reduction=0.25)[0], want)
    same(play(pkg, (4, 4), 8, 20, 16, True, lanes=2, fpu_reduction=0.25, fpu_reduction_root=0.25)[0], want)
    k4, s4 = play(pkg, (4, 4), 8, 20, 16, False, leaves_per_step=4, fpu_reduction=0.25, fpu_reduction_root=0.0)
    assert s4["games_finished"] == 20
    cap = dict(fast_simulations=4, full_search_probability=0.5, tree_reuse=True)
    a, sa = play(pkg, (4, 4), 8, 20, 16, False, fpu_reduction=0.25, **cap)
    b, sb = play(pkg, (4, 4), 8, 20, 16, False, **cap)
    assert sa["games_finished"] == sb["games_finished"] == 20
    assert a["policies"].shape != b["policies"].shape or not np.array_equal(a["policies"], b["policies"])


# ------------------------------------------------------------------------------------------------ matches
def first_moves(r, sims=32):
    e = np.zeros((4, 4), np.int8)
    return int(np.argmax(M.search(e, 1, sims, r=r).counts))


def test_the_arena_takes_the_option(pkg):
    """4x4, 32 simulations, no noise, temperature 0: the model's first move from the empty board is another with r = 0.25
    than without, and game 0 of a match (A plays black) opens with it."""
    assert first_moves(0.25) != first_moves(0.0)
    game = pkg.YinYangGame(4, 4)
    seen = {}
    for r in (0.25, 0.0, None):
        a = pkg.Arena(game, HashEval(), HashEval(), num_simulations=32, fpu_reduction=r)
        res = a.play(4, record=True)
        assert res["games"] == 4
        seen[r] = a.transcript["actions"].copy()
        assert seen[r][0, 0] == first_moves(r or 0.0), (r, seen[r][0])
    assert np.array_equal(seen[0.0], seen[None]) and not np.array_equal(seen[0.25], seen[None])
    with pytest.raises(ValueError):
        pkg.Arena(game, HashEval(), HashEval(), num_simulations=32, fpu_reduction=-1.0)
    t = pkg.Arena(game, HashEval(), HashEval(), num_simulations=32, fpu_reduction=0.25, fpu_reduction_root=0.0, tree_reuse=True)
    assert t.play(4)["games"] == 4


def test_evaluate_vs_random_takes_the_option(pkg, tmp_path, monkeypatch):
    """The model file's network is replaced by the hash evaluator, and the match is recorded: game 0 opens with the model's
    first move, another with the option than without."""
    arena = pkg.arena
    game = pkg.YinYangGame(4, 4)
    path = str(tmp_path / "m.pth.tar")
    pkg.YinYangNeuralNetwork(game, 16, 1).save_model(path)
    made = []

    class Recording(arena.Arena):
        def play(self, n, record=False):
            made.append(self)
            return super().play(n, record=True)

    monkeypatch.setattr(arena, "_load_evaluator", lambda *a, **k: HashEval())
    monkeypatch.setattr(arena, "Arena", Recording)
    for r in (0.25, None):
        res = pkg.evaluate_vs_random(game, path, num_games=4, num_simulations=32, nn_mode="fp32", num_channels=16, num_res_blocks=1,
                                     **(dict(fpu_reduction=r) if r else {}))
        assert res["alphazero_wins"] + res["random_wins"] + res["draws"] == 4
        assert made[-1].transcript["actions"][0, 0] == first_moves(r or 0.0)
    assert made[0].fpu == dict(fpu_reduction=0.25, fpu_reduction_root=0.25) and made[1].fpu == {}


def test_mcts_the_player_and_the_worker_take_the_option(pkg):
    game = pkg.YinYangGame(4, 4)
    ev = HashEval()
    for sem in ("copied", "aliased"):
        m = pkg.MCTS(game, ev, num_simulations=32, board_semantics=sem, fpu_reduction=0.25, dirichlet_noise=False, verbose=0)
        try:
            pi, _ = m.search(game.getInitBoard(), 1)
            r = M.search(np.zeros((4, 4), np.int8), 1, 32, r=0.25, aliased=sem == "aliased")
            assert np.array_equal(pi, r.counts / np.float64(r.counts.sum())), sem
        finally:
            m.close()
    w = pkg.SelfPlayWorker(game, None, num_simulations=16, board_semantics="copied", reference_quirks=False, neural_net=ev,
                           fpu_reduction=0.25, fpu_reduction_root=0.0)
    try:
        ctx = w.mcts._context(1)
        assert (ctx.fpu_reduction, ctx.fpu_reduction_root) == (0.25, 0.0)
        assert len(w.play_game()) > 0
    finally:
        w.mcts.close()
    with pytest.raises(ValueError):
        pkg.SelfPlayWorker(game, None, num_simulations=16, neural_net=ev, fpu_reduction=0.25)   # reference_quirks is its default
