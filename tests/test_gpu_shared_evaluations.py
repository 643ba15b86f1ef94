"""The shared evaluation table (shared_evaluations=, engine.SharedEvaluations, yy_mcts_set_shared_evaluations): the games of a
context share what the evaluator has told any of them.

The reference is always the SAME engine with the option off: the option on plays its games bit for bit (examples sorted by
(game_id, ply), byte compare, tolerance 0) -- a stored row is the row the evaluator would return (the exact hash evaluator of
tests/hash_eval.py is a pure function of the row; the split-f16 evaluator in one case).  The counters pin the device code: the
table serves leaves (hits > 0, fewer evaluator rows, the same leaves accounted for) and trusts nothing of the launch in flight
(twin games that insert every position in the same launch never hit).  Every test here fails on the parent: the keyword, the
class and the ABI call do not exist."""
import functools

import numpy as np
import pytest

from hash_eval import hash_eval_torch

pytestmark = pytest.mark.gpu
KEYS = ("states", "policies", "values", "game_id", "ply")
SLOTS = 4096
REUSE_OFF = dict(reuse_pass_value=False, reuse_transpositions=False, keep_evaluations=False)


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


def counters(eng):
    c = dict(eng.ctx.status())
    c.update(eng.ctx.shared_counters())
    return c


def play(pkg, shape, G, games, sims, lanes=0, rowcol=False, ev=None, **kw):
    """One run -> (examples sorted by (game_id, ply) as numpy arrays, the engine's counters)."""
    game = pkg.YinYangGame(*shape, rowcol_rule=rowcol)
    kw = dict(num_simulations=sims, concurrent_games=G, seed=11, **kw)
    eng = pkg.SelfPlayLanes(game, HashEval() if ev is None else ev, lanes=lanes, **kw) if lanes else \
        pkg.SelfPlayEngine(game, HashEval() if ev is None else ev, **kw)
    try:
        ex = pkg.self_play.sort_examples(eng.run(games))
        stats = dict(positions=eng.positions, recorded=eng.recorded, games_finished=eng.games_finished, **counters(eng))
        if kw.get("shared_evaluations"):
            tables = [l.shared for l in eng.lanes] if lanes else [eng.shared]
            stats.update(fill=sum(t.fill() for t in tables), slots=sum(t.slots for t in tables))
            assert eng.memory_bytes()["shared_evaluations"] == sum(t.memory_bytes for t in tables) > 0
    finally:
        eng.close()
    return {k: ex[k].cpu().numpy() for k in KEYS}, stats


@functools.lru_cache(maxsize=None)
def _off(pkg, shape, G, games, sims, kw):
    ex, stats = play(pkg, shape, G, games, sims, **dict(kw))
    for a in ex.values():
        a.setflags(write=False)
    return ex, stats


def option_off(pkg, shape, G, games, sims, **kw):
    """The reference run, computed once per configuration and left unchanged."""
    return _off(pkg, shape, G, games, sims, tuple(sorted(kw.items())))


def same(a, b):
    assert a["game_id"].shape == b["game_id"].shape, (a["game_id"].shape, b["game_id"].shape)
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def check(pkg, shape, G, games, sims, slots=SLOTS, **kw):
    want, wstats = option_off(pkg, shape, G, games, sims, **kw)
    got, gstats = play(pkg, shape, G, games, sims, shared_evaluations=slots, **kw)
    assert len(np.unique(want["game_id"])) == games
    same(got, want)
    for k in ("positions", "recorded", "games_finished"):
        assert gstats[k] == wstats[k], (k, gstats[k], wstats[k])
    assert wstats["hits"] == wstats["inserts"] == wstats["dropped"] == 0
    print({k: gstats[k] for k in ("evals", "transposition_hits", "hits", "inserts", "dropped", "fill")}, "off: evals", wstats["evals"])
    return gstats, wstats


# ---- 1. the same games
@pytest.mark.parametrize("shape,G,games,sims", [((4, 4), 8, 24, 16), ((5, 7), 8, 20, 24), ((1, 6), 4, 6, 8), ((7, 1), 4, 6, 8),
                                                ((9, 12), 4, 4, 8), ((12, 12), 2, 2, 8)],
                         ids=["4x4-refill-twice", "5x7", "1x6-passes", "7x1-passes", "9x12-two-words", "12x12-three-words"])
def test_same_games_lockstep(pkg, shape, G, games, sims):
    check(pkg, shape, G, games, sims)


def test_same_games_free_running(pkg):
    check(pkg, (4, 4), 8, 24, 16, free_running=True)


def test_same_games_two_lanes(pkg):
    """Every lane has a table of its own."""
    g, _ = check(pkg, (4, 4), 8, 24, 16, lanes=2)
    assert g["slots"] == 2 * SLOTS


@pytest.mark.parametrize("kw", [dict(fast_simulations=4, full_search_probability=0.5), dict(tree_reuse=True, compact_tail=False),
                                dict(evaluation_symmetry="random"), dict(forced_playouts=2), dict(fpu_reduction=0.2),
                                dict(opening_book=2), REUSE_OFF, dict(rowcol=True), dict(dirichlet_epsilon=0)],
                         ids=["playout-cap", "tree-reuse", "evaluation-symmetry", "forced-playouts", "fpu-reduction", "book-2-stones",
                              "reuse-off", "rowcol-rule", "no-noise"])
def test_same_games_with_options(pkg, kw):
    check(pkg, (4, 4), 8, 24, 16, **kw)


# ---- 2. it shares
def test_it_shares(pkg):
    """The refilled games' first leaves are children of the empty board, which earlier launches inserted long before: hits by
    construction.  Hits and evaluator rows together account for the leaves of the option-off run (the games are the same, so
    are their trees)."""
    g, w = check(pkg, (4, 4), 8, 24, 16)
    assert g["hits"] > 0
    assert g["evals"] < w["evals"]
    assert g["evals"] + g["transposition_hits"] == w["evals"] + w["transposition_hits"]      # transposition_hits counts every table
    assert g["transposition_hits"] - g["hits"] <= w["transposition_hits"]                    # what the shared table served first
    assert g["inserts"] + g["dropped"] == g["evals"] and g["fill"] == g["inserts"]            # every fresh row is offered; insert-only


# ---- 3. nothing of the current launch is read
def midgame_4x4(pkg):
    """A 4x4 position after four plies of the first legal move each (host rules), and its side to move."""
    game = pkg.YinYangGame(4, 4)
    board, player = game.getInitBoard(), 1
    for _ in range(4):
        a = int(np.flatnonzero(game.getValidMoves(board, player))[0])
        board, player = game.getNextState(board, player, a)
    return np.asarray(board.board, np.int8), player


def twin_search(pkg, reuse, slots):
    import torch
    b, player = midgame_4x4(pkg)
    boards = torch.from_numpy(np.stack([b, b])).cuda()
    players = torch.full((2,), player, dtype=torch.int8, device="cuda")
    ctx = pkg.engine.BatchedMCTS(2, 4, 4, 32, reuse_pass_value=reuse, reuse_transpositions=reuse, keep_evaluations=reuse)
    table = None
    if slots:
        table = pkg.engine.SharedEvaluations(4, 4, slots)
        ctx.set_shared_evaluations(table)
    counts = ctx.search(boards, players, lambda planes: hash_eval_torch(planes, 10, 11), 32).cpu().numpy()
    c = dict(ctx.status(), **ctx.shared_counters())
    ctx.close()
    assert np.array_equal(counts[0], counts[1]) and counts[0].sum() == 32
    return counts, c


def test_twin_games_never_read_the_launch_in_flight(pkg):
    """Two games on the same root, no noise: their searches are identical step for step, so every position is inserted by both
    in the same launch, and a game meets a position again first in its own cache.  A hit here could only be an entry of the
    launch in flight or one skipped wrongly."""
    want, wc = twin_search(pkg, True, 0)
    got, gc = twin_search(pkg, True, SLOTS)
    assert gc["hits"] == 0
    assert gc["evals"] == wc["evals"] and gc["inserts"] == gc["evals"]
    assert np.array_equal(got, want)


def test_twin_games_hit_entries_of_earlier_launches(pkg):
    """The same without the per-game reuse: a transposition (or a childless node visited again) inside the search finds the entry
    an earlier launch inserted."""
    want, wc = twin_search(pkg, False, 0)
    got, gc = twin_search(pkg, False, SLOTS)
    assert gc["hits"] > 0 and gc["evals"] + gc["hits"] == wc["evals"]
    assert np.array_equal(got, want)


# ---- 4. a table that fills up
def test_a_full_table_drops_inserts(pkg):
    g, _ = check(pkg, (4, 4), 8, 24, 16, slots=64)
    assert g["dropped"] > 0 and g["fill"] <= 64 and g["fill"] == g["inserts"]


# ---- 5. clear()
def test_clear(pkg):
    game = pkg.YinYangGame(4, 4)
    runs = {}
    for on in (False, True):
        eng = pkg.SelfPlayEngine(game, HashEval(), num_simulations=16, concurrent_games=8, seed=11,
                                 **(dict(shared_evaluations=SLOTS) if on else {}))
        try:
            first = pkg.self_play.sort_examples(eng.run(12))
            c1 = counters(eng)
            if on:
                assert eng.shared.fill() == c1["inserts"] > 0
                eng.shared.clear()
                assert eng.shared.fill() == 0
            eng.ctx.reset_counters()
            second = pkg.self_play.sort_examples(eng.run(12))
            c2 = counters(eng)
            if on:
                assert eng.shared.fill() == c2["inserts"] > 0      # the table holds what was inserted since the clear, nothing else
            runs[on] = ([{k: e[k].cpu().numpy() for k in KEYS} for e in (first, second)], c2)
        finally:
            eng.close()
    for a, b in zip(runs[True][0], runs[False][0]):
        same(a, b)
    assert sorted(np.unique(runs[True][0][1]["game_id"])) == list(range(12, 24))               # the indices go on
    on, off = runs[True][1], runs[False][1]
    assert on["hits"] > 0 and on["evals"] + on["transposition_hits"] == off["evals"] + off["transposition_hits"]


# ---- 6. the split-f16 evaluator
def test_split_f16_evaluator(pkg):
    import torch
    game = pkg.YinYangGame(6, 6)
    torch.manual_seed(0)
    ev = pkg.BatchedEvaluator(pkg.YinYangNeuralNetwork(game, 32, 1).cuda().eval())
    assert ev.mode == "f16x3" and ev.row_independent
    want, wstats = play(pkg, (6, 6), 8, 12, 16, ev=ev)
    got, gstats = play(pkg, (6, 6), 8, 12, 16, ev=ev, shared_evaluations=1 << 14)
    same(got, want)
    assert gstats["positions"] == wstats["positions"] and gstats["hits"] > 0 and gstats["evals"] < wstats["evals"]


# ---- 7. refusals
def test_c_abi_refuses_aliased_boards_and_leaf_parallel_steps(pkg):
    table = pkg.engine.SharedEvaluations(4, 4, 64)
    for kw in (dict(aliased=True), dict(leaves_per_step=2)):
        ctx = pkg.engine.BatchedMCTS(4, 4, 4, 8, **kw)
        with pytest.raises(pkg.YYError) as e:
            ctx.set_shared_evaluations(table)
        assert e.value.code == -2 and ctx.shared is None and table.ctx is None
        ctx.close()


def test_python_refusals(pkg):
    game = pkg.YinYangGame(4, 4)

    class Dependent(HashEval):
        row_independent = False

    with pytest.raises(ValueError, match="row_independent"):
        pkg.SelfPlayEngine(game, Dependent(), num_simulations=8, concurrent_games=4, shared_evaluations=64)
    a = pkg.engine.BatchedMCTS(2, 4, 4, 8)
    b = pkg.engine.BatchedMCTS(2, 4, 4, 8, evaluation_symmetry="random", symmetry_seed=3)
    table = pkg.engine.SharedEvaluations(4, 4, 100)
    assert table.slots == 128 and table.memory_bytes == 128 * (4 + 16 + 4 + 64) + 4
    with pytest.raises(ValueError, match="symmetry"):
        b.set_shared_evaluations(table)
    with pytest.raises(ValueError, match="board size"):
        a.set_shared_evaluations(pkg.engine.SharedEvaluations(4, 5, 64))
    a.set_shared_evaluations(table)
    c = pkg.engine.BatchedMCTS(2, 4, 4, 8)
    with pytest.raises(ValueError, match="another context"):
        c.set_shared_evaluations(table)
    a.set_shared_evaluations(None)
    c.set_shared_evaluations(table)                # free again
    for ctx in (a, b, c):
        ctx.close()


def test_clear_is_refused_while_a_select_is_pending(pkg):
    """A pending leaf may name a slot of the table: the table is emptied through its context, which refuses in that state."""
    import torch
    ctx = pkg.engine.BatchedMCTS(2, 4, 4, 8)
    table = pkg.engine.SharedEvaluations(4, 4, 64)
    ctx.set_shared_evaluations(table)
    boards = torch.zeros((2, 4, 4), dtype=torch.int8, device="cuda")
    players = torch.ones(2, dtype=torch.int8, device="cuda")
    ctx.begin(boards, players)
    for call in (table.clear, lambda: ctx.set_shared_evaluations(None)):
        with pytest.raises(pkg.YYError) as e:
            call()
        assert e.value.code == -5
    p, _ = hash_eval_torch(ctx.planes, 10, 11)
    ctx.expand_root(p)
    ctx.select()
    with pytest.raises(pkg.YYError) as e:
        table.clear()
    assert e.value.code == -5
    ctx.expand_backup(*hash_eval_torch(ctx.planes, 10, 11))
    table.clear()                                  # between searches
    assert table.fill() == 0
    ctx.close()
    assert table.ctx is None and ctx.shared is None          # close() lets go of the table


def test_mcts_takes_the_option_and_checks_the_evaluator(pkg):
    import torch
    game = pkg.YinYangGame(4, 4)
    b, player = midgame_4x4(pkg)
    boards = torch.from_numpy(np.stack([b, b, b])).cuda()
    players = torch.full((3,), player, dtype=torch.int8, device="cuda")
    out = {}
    for on in (False, True):
        m = pkg.MCTS(game, HashEval(), num_simulations=24, board_semantics="copied", dirichlet_noise=False,
                     **(dict(shared_evaluations=256) if on else {}))
        pi, ctx = m.search_batch(boards, players)
        pi2, _ = m.search_batch(boards, players)                      # the second search finds the first one's rows
        out[on] = (pi.cpu().numpy(), pi2.cpu().numpy(), ctx.status()["evals"], ctx.shared_counters()["hits"])
        m.close()
    assert np.array_equal(out[True][0], out[False][0]) and np.array_equal(out[True][1], out[False][1])
    assert out[True][3] > 0 and out[True][2] < out[False][2] and out[False][3] == 0
    m = pkg.MCTS(game, lambda planes: hash_eval_torch(planes, 10, 11), num_simulations=8, board_semantics="copied",
                 shared_evaluations=256)
    with pytest.raises(ValueError, match="row_independent"):
        m.search_batch(boards, players)
    m.close()
