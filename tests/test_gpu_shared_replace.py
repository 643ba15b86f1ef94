"""The replacing shared evaluation table (shared_evaluations_replace=, engine.SharedEvaluations(replace=True),
yy_mcts_set_shared_evaluations_replacing, yy_mcts_shared_evaluations_sweep): one slot per position and launch, hit marks, and
eviction by sweeps between tree steps.

The reference is always the SAME engine WITHOUT any table: a table only ever returns the evaluator's own row for a position, so
no duplicate or eviction decision may change a game -- examples sorted by (game_id, ply), byte compare, tolerance 0, with a
table of 64 slots that is far smaller than what the games visit (windows overflow, sweeps evict).  The counters pin the device
code.  Every test here fails on the parent: the keyword, the class argument and the ABI calls do not exist."""
import functools

import numpy as np
import pytest

from hash_eval import hash_eval_torch

pytestmark = pytest.mark.gpu
KEYS = ("states", "policies", "values", "game_id", "ply")
SMALL = 64
REUSE_OFF = dict(reuse_pass_value=False, reuse_transpositions=False, keep_evaluations=False)
BASE = ((4, 4), 8, 24, 16)                           # shape, slots of the batch, games, simulations


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


def snapshot(table):
    """The table's arrays on the host, and what must hold of them whatever was played (no torn entry)."""
    return dict(claim=table.claim.cpu().numpy().view(np.uint64), last_hit=table.last_hit.cpu().numpy().view(np.uint32),
                keys=table.keys.cpu().numpy().copy(), value=table.value.cpu().numpy().copy(), policy=table.policy.cpu().numpy().copy())


def play(pkg, shape, G, games, sims, high_water=None, **kw):
    """One run -> (examples sorted by (game_id, ply) as numpy arrays, the engine's counters, the table's arrays or None)."""
    game = pkg.YinYangGame(*shape)
    eng = pkg.SelfPlayEngine(game, HashEval(), num_simulations=sims, concurrent_games=G, seed=11, **kw)
    try:
        if high_water is not None:
            eng.shared.high_water = high_water
        ex = pkg.self_play.sort_examples(eng.run(games))
        stats = dict(positions=eng.positions, recorded=eng.recorded, games_finished=eng.games_finished, **eng.ctx.status())
        snap = None
        if eng.shared is not None:
            stats.update(eng.shared.counters(), fill=eng.shared.fill())
            snap = snapshot(eng.shared) if eng.shared.replace else None
    finally:
        eng.close()
    return {k: ex[k].cpu().numpy() for k in KEYS}, stats, snap


@functools.lru_cache(maxsize=None)
def _no_table(pkg, shape, G, games, sims, kw):
    ex, stats, _ = play(pkg, shape, G, games, sims, **dict(kw))
    for a in ex.values():
        a.setflags(write=False)
    return ex, stats


def no_table(pkg, shape, G, games, sims, **kw):
    """The reference run, computed once per configuration and left unchanged."""
    return _no_table(pkg, shape, G, games, sims, tuple(sorted(kw.items())))


def same(a, b):
    assert a["game_id"].shape == b["game_id"].shape, (a["game_id"].shape, b["game_id"].shape)
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def check(pkg, shape, G, games, sims, high_water=None, **kw):
    want, wstats = no_table(pkg, shape, G, games, sims, **kw)
    got, gstats, snap = play(pkg, shape, G, games, sims, high_water=high_water, shared_evaluations=SMALL,
                             shared_evaluations_replace=True, **kw)
    print({k: gstats[k] for k in ("evals", "hits", "inserts", "dropped", "duplicates", "evicted", "live", "fill")},
          "no table: evals", wstats["evals"])
    assert len(np.unique(want["game_id"])) == games
    same(got, want)
    for k in ("positions", "recorded", "games_finished"):
        assert gstats[k] == wstats[k], (k, gstats[k], wstats[k])
    assert gstats["fill"] == gstats["inserts"] - gstats["evicted"]          # every slot taken was counted, every slot freed too
    return gstats, wstats, snap


# ---- 1. the same games
@pytest.mark.parametrize("free_running", [False, True], ids=["lockstep", "free-running"])
def test_same_games(pkg, free_running):
    g, w, _ = check(pkg, *BASE, free_running=free_running)
    assert g["evicted"] > 0 and g["hits"] > 0                               # not an idle table
    assert g["evals"] < w["evals"]
    if not free_running:                                                    # `evals` counts leaf rows, not the root calls:
        assert g["inserts"] + g["dropped"] + g["duplicates"] == g["evals"]  # every fresh non-root row is offered to the table


@pytest.mark.parametrize("kw", [dict(evaluation_symmetry="random"), dict(fast_simulations=4, full_search_probability=0.5),
                                dict(tree_reuse=True, compact_tail=False), dict(forced_playouts=2), dict(fpu_reduction=0.2), REUSE_OFF],
                         ids=["evaluation-symmetry", "playout-cap", "tree-reuse", "forced-playouts", "fpu-reduction", "reuse-off"])
def test_same_games_with_options(pkg, kw):
    check(pkg, *BASE, **kw)


@pytest.mark.parametrize("shape,G,games,sims", [((9, 12), 4, 4, 8), ((12, 12), 2, 2, 8)], ids=["9x12-two-words", "12x12-three-words"])
def test_same_games_on_larger_boards(pkg, shape, G, games, sims):
    check(pkg, shape, G, games, sims)


# ---- 2. one slot per position
def identical_games(pkg, replace):
    import torch
    boards = torch.zeros((8, 4, 4), dtype=torch.int8, device="cuda")
    players = torch.ones(8, dtype=torch.int8, device="cuda")
    ctx = pkg.engine.BatchedMCTS(8, 4, 4, 16, **REUSE_OFF)
    table = pkg.engine.SharedEvaluations(4, 4, 4096, replace=replace)
    ctx.set_shared_evaluations(table)
    counts = ctx.search(boards, players, lambda planes: hash_eval_torch(planes, 10, 11), 16).cpu().numpy()
    c = dict(ctx.status(), **table.counters(), fill=table.fill())
    ctx.close()
    assert all(np.array_equal(counts[0], counts[g]) for g in range(8)) and counts[0].sum() == 16
    return c


def test_one_slot_per_position(pkg):
    """Eight identical games insert every position in the same launch: one of them takes a slot, seven count a duplicate."""
    c = identical_games(pkg, True)
    assert c["evals"] % 8 == 0
    rows = c["evals"] // 8              # game 0's evaluator rows less its root call: `evals` counts leaf rows only, no root call
    print(c)
    assert rows > 0 and c["inserts"] == rows and c["duplicates"] == 7 * rows and c["dropped"] == 0 and c["fill"] == rows
    plain = identical_games(pkg, False)
    print(plain)
    assert plain["evals"] == c["evals"] and plain["hits"] == c["hits"]
    assert plain["inserts"] == 8 * rows and set(plain) == set(c) - {"duplicates", "evicted", "live"}      # what changed


# ---- 3. a full window comes back
def midgame_4x4(pkg):
    game = pkg.YinYangGame(4, 4)
    board, player = game.getInitBoard(), 1
    for _ in range(4):
        a = int(np.flatnonzero(game.getValidMoves(board, player))[0])
        board, player = game.getNextState(board, player, a)
    return np.asarray(board.board, np.int8), player


@pytest.mark.parametrize("replace", [True, False], ids=["replacing", "insert-only"])
def test_a_full_window_comes_back(pkg, replace):
    import torch
    sims = 512                                        # far more positions than slots: every window of the 64 slots overflows
    ctx = pkg.engine.BatchedMCTS(1, 4, 4, sims, **REUSE_OFF)
    table = pkg.engine.SharedEvaluations(4, 4, SMALL, replace=replace, high_water=0.0)
    ctx.set_shared_evaluations(table)
    ev = lambda planes: hash_eval_torch(planes, 10, 11)
    ctx.search(torch.zeros((1, 4, 4), dtype=torch.int8, device="cuda"), torch.ones(1, dtype=torch.int8, device="cuda"), ev, sims)
    before = table.counters()
    print(before, table.fill())
    assert before["dropped"] > 0
    assert table.fill() == SMALL                      # the whole table is full: the control below rests on it
    for _ in range(2):                                # the first sweep above the mark records the stamp, the second evicts
        if replace:
            table.sweep()
        else:
            with pytest.raises(RuntimeError):
                table.sweep()
    b, player = midgame_4x4(pkg)
    ctx.search(torch.from_numpy(b[None]).cuda(), torch.full((1,), player, dtype=torch.int8, device="cuda"), ev, sims)
    after = table.counters()
    print(after, table.fill())
    ctx.status()
    ctx.close()
    if replace:
        assert after["inserts"] > before["inserts"] and after["evicted"] > 0
    else:
        assert after["inserts"] == before["inserts"] and after["dropped"] > before["dropped"]


# ---- 4. no torn entry
def test_no_torn_entry(pkg):
    """After the same-games run: every live entry holds the evaluator's row of its own key, no position sits twice under one
    insert stamp, and the live entries are the inserted ones less the evicted ones."""
    import torch
    g, _, snap = check(pkg, *BASE)
    stamp = (snap["claim"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    live = np.flatnonzero((stamp != 0) & (stamp != 0xFFFFFFFF))
    assert len(live) == g["inserts"] - g["evicted"] > 0
    keys = torch.from_numpy(snap["keys"][live]).cuda()                    # [n, 2]: black word, white word
    boards = pkg.engine.unpack_boards(keys[:, :1].t().contiguous(), keys[:, 1:].t().contiguous(), 4, 4)
    policy, value = hash_eval_torch(pkg.engine.encode_planes(boards), 10, 11)
    assert np.array_equal(snap["policy"][live].view(np.uint32), policy.cpu().numpy().view(np.uint32))
    assert np.array_equal(snap["value"][live].view(np.uint32), value.cpu().numpy().view(np.uint32))
    entries = {(int(stamp[s]), snap["keys"][s].tobytes()) for s in live}
    assert len(entries) == len(live)                                      # one slot per (insert stamp, position)
    # a last-hit stamp is never older than the insert stamp (no wrap in a run this short: plain numbers)
    assert (snap["last_hit"][live].astype(np.int64) >= stamp[live]).all()


# ---- 5. pending leaves are safe
def test_a_sweep_between_every_two_steps_with_selects_pending(pkg):
    """Free-running, a poll and with it a sweep after every single step, high_water 0: every sweep evicts whatever the latest
    launch neither inserted nor served, while every game has a select pending."""
    g, w, _ = check(pkg, *BASE, high_water=0.0, free_running=True, poll_steps=1)
    assert g["games_finished"] == w["games_finished"] == BASE[2] and g["evicted"] > 0


# ---- 6. the C ABI's refusals
def test_c_abi_refuses_aliased_boards_and_leaf_parallel_steps(pkg):
    table = pkg.engine.SharedEvaluations(4, 4, 64, replace=True)
    for kw in (dict(aliased=True), dict(leaves_per_step=2)):
        ctx = pkg.engine.BatchedMCTS(4, 4, 4, 8, **kw)
        with pytest.raises(pkg.YYError) as e:
            ctx.set_shared_evaluations(table)
        assert e.value.code == -2 and ctx.shared is None and table.ctx is None
        ctx.close()


def test_sweep_without_a_replacing_table_is_an_error_code(pkg):
    L = pkg._lib.lib()
    ctx = pkg.engine.BatchedMCTS(2, 4, 4, 8)
    assert L.yy_mcts_shared_evaluations_sweep(ctx._h, 0, None) == -5 and b"replacing" in L.yy_last_error()
    ctx.set_shared_evaluations(pkg.engine.SharedEvaluations(4, 4, 64))
    assert L.yy_mcts_shared_evaluations_sweep(ctx._h, 0, None) == -5
    assert L.yy_mcts_shared_evaluations_sweep(None, 0, None) == -1
    table = pkg.engine.SharedEvaluations(4, 4, 64, replace=True)
    ctx.set_shared_evaluations(table)
    assert L.yy_mcts_shared_evaluations_sweep(ctx._h, -1, None) == -1
    table.sweep()
    assert table.counters() == dict(hits=0, inserts=0, dropped=0, duplicates=0, evicted=0, live=0)
    ctx.close()
