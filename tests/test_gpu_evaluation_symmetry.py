"""Symmetry-randomised evaluation (evaluation_symmetry="random"): every position is shown to the evaluator under a board
symmetry drawn from (symmetry_seed, position), and the policy row is mapped back.

The exact reference is a host-wrapped evaluator (tests/symmetry_model.py, Wrapped): planes of the original position -> board
-> s from the numpy restatement of the draw -> T_s(board) with numpy -> the existing encode_planes -> the inner evaluator ->
the policy row permuted back.  The unchanged engine (option off) driven by the wrapper must equal the engine with the option on
driven by the bare inner evaluator, bit for bit.  The inner evaluator is the hash of tests/hash_eval.py: a hash of the row, so
maximally non-equivariant -- a wrong cell, a wrong inverse or a missed call site changes the searches and the games.
Every test here fails on the parent: the keyword and the ABI calls do not exist."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import symmetry_model as sm
from hash_eval import hash_eval_torch

pytestmark = pytest.mark.gpu
KEYS = ("states", "policies", "values", "game_id", "ply")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11                         # the engines' seed, and so their symmetry seed


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    import yinyang_game_alphazero_amd as p
    return p


class HashEval:
    row_independent = True

    def __call__(self, planes):
        return hash_eval_torch(planes, 10, 11)


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 1. the draw
@pytest.mark.parametrize("shape", sm.DRAW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_draw_is_the_numpy_restatement(pkg, shape):
    boards = sm.positions(shape)
    want = sm.draw(boards, sm.DRAW_SEED)
    n = sm.group_size(*shape)
    counts = np.bincount(want, minlength=n)
    assert len(counts) == n and counts.min() > 0 and counts.max() <= 512 // (4 if n == 8 else 2), counts
    got = pkg.engine.evaluation_symmetry(on_device(boards), sm.DRAW_SEED).cpu().numpy()
    assert got.dtype == np.int8 and got.min() >= 0 and got.max() < n
    assert np.array_equal(got, want)
    other = pkg.engine.evaluation_symmetry(on_device(boards), sm.DRAW_SEED + 1).cpu().numpy()
    assert np.array_equal(other, sm.draw(boards, sm.DRAW_SEED + 1)) and not np.array_equal(other, got)
    # seeds beyond 32 bits reach the key whole
    big = (1 << 63) + 12345
    assert np.array_equal(pkg.engine.evaluation_symmetry(on_device(boards[:64]), big).cpu().numpy(), sm.draw(boards[:64], big))


# ------------------------------------------------------------------------------------------------ 2. the encoder
@pytest.mark.parametrize("shape", sm.DRAW_SHAPES + ((1, 6), (7, 1)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_encoder_is_the_plain_encoder_of_the_transformed_board(pkg, shape):
    boards = sm.positions(shape, 64)
    s = sm.draw(boards, sm.DRAW_SEED)
    assert len(np.unique(s)) > 1
    want = pkg.engine.encode_planes(on_device(sm.transform_boards(boards, s))).cpu().numpy()
    got = pkg.engine.encode_planes(on_device(boards), symmetry_seed=sm.DRAW_SEED).cpu().numpy()
    assert got.shape == (64, 5) + shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    plain = pkg.engine.encode_planes(on_device(boards)).cpu().numpy()
    assert not np.array_equal(got, plain)


# ------------------------------------------------------------------------------------------------ 3. the search
def root_positions(pkg, shape, G):
    """Game g after g % 5 random legal moves from the empty board (black starts): boards int8 [G,R,C], players int8 [G]."""
    import torch
    rng = np.random.RandomState(17)
    boards = torch.zeros((G,) + shape, dtype=torch.int8, device="cuda")
    players = torch.ones(G, dtype=torch.int8, device="cuda")
    for ply in range(4):
        mask = pkg.engine.valid_mask(boards, players).cpu().numpy()
        action = np.full(G, -1, np.int32)
        for g in range(G):
            legal = np.flatnonzero(mask[g])
            if g % 5 > ply and len(legal):
                action[g] = rng.choice(legal)
        move = on_device(action >= 0)
        before = players.clone()
        pkg.engine.step_(boards, players, on_device(action))
        players = torch.where(move, players, before)
    return boards, players


def searched(pkg, shape, G, sims, K, evaluator, **kw):
    boards, players = root_positions(pkg, shape, G)
    ctx = pkg.engine.BatchedMCTS(G, shape[0], shape[1], sims, leaves_per_step=K, **kw)
    try:
        counts = ctx.search(boards, players, evaluator, sims)
        _, cw, cp = ctx.root_counts(with_children=True)
        visits, wsum = ctx.root_stats()
        ctx.status()
        return [t.cpu().numpy() for t in (counts, cp, cw, visits, wsum)]
    finally:
        ctx.close()


@pytest.mark.parametrize("shape,G,sims,K", [((4, 4), 8, 16, 1), ((4, 4), 8, 16, 2), ((5, 7), 8, 24, 1), ((9, 12), 4, 8, 1),
                                            ((12, 12), 2, 8, 1)],
                         ids=["4x4-one-word", "4x4-K2", "5x7-non-square", "9x12-two-words", "12x12-three-words"])
def test_search_equals_the_wrapped_evaluator(pkg, shape, G, sims, K):
    ev = HashEval()
    want = searched(pkg, shape, G, sims, K, sm.Wrapped(pkg, ev, SEED))
    got = searched(pkg, shape, G, sims, K, ev, evaluation_symmetry="random", symmetry_seed=SEED)
    plain = searched(pkg, shape, G, sims, K, ev)
    for name, a, b in zip(("counts", "priors", "W", "root visits", "root W"), got, want):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    assert got[0].sum() == G * sims and (got[0] > 0).sum() > G           # child order: per-action arrays, several children each
    assert not np.array_equal(got[1], plain[1])                          # and the option does something


def test_search_with_the_evaluation_cache(pkg):
    """The per-game cache stores the evaluator's row (the transformed frame) and is read through the same map."""
    ev, kw = HashEval(), dict(reuse_pass_value=True, reuse_transpositions=True, keep_evaluations=True)
    want = searched(pkg, (4, 4), 8, 48, 1, sm.Wrapped(pkg, ev, SEED), **kw)
    got = searched(pkg, (4, 4), 8, 48, 1, ev, evaluation_symmetry="random", symmetry_seed=SEED, **kw)
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ 4. self-play
def play(pkg, shape, G, games, sims, ev, free=False, **kw):
    eng = pkg.SelfPlayEngine(pkg.YinYangGame(*shape), ev, num_simulations=sims, concurrent_games=G, seed=SEED, free_running=free, **kw)
    try:
        ex = pkg.self_play.sort_examples(eng.run(games))
    finally:
        eng.close()
    return {k: ex[k].cpu().numpy() for k in KEYS}


@functools.lru_cache(maxsize=None)
def _wrapped_lockstep(pkg, shape, G, games, sims, kw):
    ex = play(pkg, shape, G, games, sims, sm.Wrapped(pkg, HashEval(), SEED), use_graph=False, **dict(kw))
    for a in ex.values():
        a.setflags(write=False)
    return ex


def wrapped_lockstep(pkg, shape, G, games, sims, **kw):
    """The reference run (option off, wrapped evaluator, lockstep), computed once per configuration and left unchanged."""
    return _wrapped_lockstep(pkg, shape, G, games, sims, tuple(sorted(kw.items())))


def same(a, b):
    assert a["game_id"].shape == b["game_id"].shape, (a["game_id"].shape, b["game_id"].shape)
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


REUSE_OFF = dict(reuse_pass_value=False, reuse_transpositions=False, keep_evaluations=False)


@pytest.mark.parametrize("shape,G,games,sims,kw,free_too", [
    ((4, 4), 8, 20, 16, {}, True), ((4, 4), 8, 20, 16, dict(opening_book=2), True), ((4, 4), 8, 20, 16, REUSE_OFF, True),
    ((4, 4), 8, 20, 16, dict(fast_simulations=4, full_search_probability=0.5), True),
    ((4, 4), 8, 20, 16, dict(tree_reuse=True), False), ((5, 7), 8, 12, 24, {}, True)],
    ids=["4x4-defaults", "book-2-stones", "reuse-off", "playout-cap", "tree-reuse-lockstep-only", "5x7"])
def test_self_play_equals_the_wrapped_evaluator(pkg, shape, G, games, sims, kw, free_too):
    want = wrapped_lockstep(pkg, shape, G, games, sims, **kw)
    assert len(np.unique(want["game_id"])) == games
    on = dict(kw, evaluation_symmetry="random")                          # symmetry_seed: the engine's seed
    same(play(pkg, shape, G, games, sims, HashEval(), **on), want)
    if free_too:
        same(play(pkg, shape, G, games, sims, HashEval(), free=True, **on), want)
    plain = play(pkg, shape, G, games, sims, HashEval(), **kw)
    assert plain["states"].shape != want["states"].shape or not np.array_equal(plain["states"], want["states"])


def test_symmetry_seed_is_its_own_seed(pkg):
    """symmetry_seed given: the games' own draws keep the engine's seed, the symmetry takes the other one."""
    want = play(pkg, (4, 4), 8, 20, 16, sm.Wrapped(pkg, HashEval(), 5), use_graph=False)
    same(play(pkg, (4, 4), 8, 20, 16, HashEval(), free=True, evaluation_symmetry="random", symmetry_seed=5), want)
    lanes = pkg.SelfPlayLanes(pkg.YinYangGame(4, 4), HashEval(), num_simulations=16, concurrent_games=8, lanes=2, seed=SEED,
                              opening_book=2, evaluation_symmetry="random", symmetry_seed=5)
    try:
        assert lanes.book.symmetry == ("random", 5)
        ex = pkg.self_play.sort_examples(lanes.run(20))
    finally:
        lanes.close()
    same({k: ex[k].cpu().numpy() for k in KEYS}, want)


# ------------------------------------------------------------------------------------------------ 5. the book's frame
def test_a_book_of_another_frame_is_refused(pkg):
    game, ev = pkg.YinYangGame(4, 4), HashEval()
    plain = pkg.engine.OpeningBook(4, 4, ev, 2)
    other = pkg.engine.OpeningBook(4, 4, ev, 2, evaluation_symmetry="random", symmetry_seed=SEED + 1)
    right = pkg.engine.OpeningBook(4, 4, ev, 2, evaluation_symmetry="random", symmetry_seed=SEED)
    assert plain.symmetry == ("off", None) and right.symmetry == ("random", SEED)
    assert not np.array_equal(plain.policy.cpu().numpy(), right.policy.cpu().numpy())
    for free in (False, True):
        for book in (plain, other):
            with pytest.raises(ValueError, match="book"):
                pkg.SelfPlayEngine(game, ev, num_simulations=8, concurrent_games=4, seed=SEED, opening_book=book,
                                   evaluation_symmetry="random", free_running=free)
        with pytest.raises(ValueError, match="book"):
            pkg.SelfPlayEngine(game, ev, num_simulations=8, concurrent_games=4, seed=SEED, opening_book=right, free_running=free)
    eng = pkg.SelfPlayEngine(game, ev, num_simulations=8, concurrent_games=4, seed=SEED, opening_book=right, evaluation_symmetry="random")
    assert eng.ctx.book is right
    eng.close()


def test_unsupported_combinations_raise(pkg):
    game, ev = pkg.YinYangGame(4, 4), HashEval()
    for kw in (dict(board_semantics="aliased"), dict(reference_quirks=True), dict(rng="numpy")):
        with pytest.raises(ValueError, match="evaluation_symmetry"):
            pkg.SelfPlayEngine(game, ev, num_simulations=8, concurrent_games=4, evaluation_symmetry="random", **kw)
    with pytest.raises(pkg.YYError) as e:                               # the C ABI refuses what it cannot play
        pkg.engine.BatchedMCTS(4, 4, 4, 8, aliased=True, evaluation_symmetry="random")
    assert e.value.code == -2


# ------------------------------------------------------------------------------------------------ 6. the command line
def test_cli_lockstep_and_free_running_write_the_same_file(tmp_path):
    import torch
    import yinyang_game_alphazero_amd as pkg
    mdir, ddir = tmp_path / "models", tmp_path / "data"
    os.makedirs(mdir)
    torch.manual_seed(0)
    pkg.YinYangNeuralNetwork(pkg.YinYangGame(6, 6)).save_model(str(mdir / "best_model.pth.tar"))
    cmd = [sys.executable, os.path.join(ROOT, "train_alphazero.py"), "--mode", "self-play", "--rows", "6", "--cols", "6",
           "--simulations", "25", "--episodes", "4", "--workers", "1", "--model-dir", str(mdir), "--data-dir", str(ddir),
           "--evaluation-symmetry", "random"]
    files = []
    for extra in ([], ["--free-running"]):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        info = json.loads(r.stdout.strip().splitlines()[-1])
        z = np.load(info["data_file"])
        order = np.lexsort((z["ply"], z["game_id"]))
        files.append({k: z[k][order] for k in z.files})
        os.remove(info["data_file"])
    assert len(np.unique(files[0]["game_id"])) == 4
    for k in files[0]:
        assert np.array_equal(files[0][k], files[1][k]), k
