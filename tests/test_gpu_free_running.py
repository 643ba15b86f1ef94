"""Free-running self-play (SelfPlayEngine(free_running=True), csrc/yy_selfplay_move.hip): the games play their moves on the
device, inside the search step.

The reference is the LOCKSTEP engine: with the same seed and the same game indices the free-running engine returns the same
examples bit for bit after sorting both by (game_id, ply) -- states, pi, z, game_id, ply; tolerance 0.  That holds because every
draw is keyed by (seed, game index, ply) and the evaluator is row-independent (the exact hash evaluator of tests/hash_eval.py;
the split-f16 evaluator in one case).  Every test here fails on the parent: the keyword does not exist."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hash_eval import hash_eval_torch

pytestmark = pytest.mark.gpu
KEYS = ("states", "policies", "values", "game_id", "ply")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    import yinyang_game_alphazero_amd as p
    return p


class HashEval:
    """The exact hash evaluator as an evaluator object: a pure function of the row, so the engines may reuse its evaluations.
    poison: a board int8 [R,C] whose value comes out NaN (a failed search for every game that evaluates it as a leaf)."""

    def __init__(self, row_independent=True, poison=None):
        self.row_independent = row_independent
        self.poison = None if poison is None else poison.cuda()     # on the device before any step is captured

    def __call__(self, planes):
        import torch
        p, v = hash_eval_torch(planes, 10, 11)
        if self.poison is not None:
            b = (planes[:, 1] - planes[:, 2]).to(torch.int8)
            hit = (b == self.poison[None]).flatten(1).all(1)
            v = torch.where(hit, torch.full_like(v, float("nan")), v)
        return p, v


def play(pkg, shape, G, games, sims, free, lanes=0, rowcol=False, ev=None, **kw):
    """One run -> (examples sorted by (game_id, ply) as numpy arrays, the engine's counters)."""
    game = pkg.YinYangGame(*shape, rowcol_rule=rowcol)
    row_independent = kw.pop("row_independent", True)
    ev = HashEval(row_independent) if ev is None else ev
    kw = dict(num_simulations=sims, concurrent_games=G, seed=11, **kw)
    if free:
        kw["free_running"] = True
    eng = pkg.SelfPlayLanes(game, ev, lanes=lanes, **kw) if lanes else pkg.SelfPlayEngine(game, ev, **kw)
    try:
        ex = pkg.self_play.sort_examples(eng.run(games))
        stats = dict(positions=eng.positions, recorded=eng.recorded, games_finished=eng.games_finished,
                     steps_issued=eng.steps_issued if free else None)
    finally:
        eng.close()
    return {k: ex[k].cpu().numpy() for k in KEYS}, stats


@functools.lru_cache(maxsize=None)
def lockstep(pkg, shape, G, games, sims, **kw):
    """The reference run, computed once per configuration and left unchanged."""
    ex, stats = play(pkg, shape, G, games, sims, False, **kw)
    for a in ex.values():
        a.setflags(write=False)
    return ex, stats


def lockstep_of(pkg, shape, G, games, sims, **kw):
    return lockstep(pkg, shape, G, games, sims, **dict(sorted(kw.items())))


def same(a, b):
    assert a["game_id"].shape == b["game_id"].shape, (a["game_id"].shape, b["game_id"].shape)
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def check(pkg, shape, G, games, sims, **kw):
    want, wstats = lockstep_of(pkg, shape, G, games, sims, **kw)
    got, gstats = play(pkg, shape, G, games, sims, True, **kw)
    assert len(np.unique(want["game_id"])) == games
    same(got, want)
    for k in ("positions", "recorded", "games_finished"):
        assert gstats[k] == wstats[k], (k, gstats[k], wstats[k])
    # the host sees the end one poll late: at most two polls of steps beyond the bound (poll = four unrolled graphs by default)
    poll = 4 * max(1, int(os.environ.get("YY_GRAPH_UNROLL", "8")))
    assert 0 < gstats["steps_issued"] <= pkg.self_play.free_running_step_bound(games, G, shape[0] * shape[1], sims) + 2 * poll
    return got, gstats


@pytest.mark.parametrize("shape,G,games,sims", [((4, 4), 8, 24, 16), ((5, 7), 8, 20, 24), ((1, 6), 4, 6, 8), ((7, 1), 4, 6, 8),
                                                ((9, 12), 4, 4, 8), ((12, 12), 2, 2, 8)],
                         ids=["4x4-refill-twice", "5x7", "1x6-passes", "7x1-passes", "9x12-two-words", "12x12-three-words"])
def test_same_examples_as_lockstep(pkg, shape, G, games, sims):
    check(pkg, shape, G, games, sims)


@pytest.mark.parametrize("G,games", [(1, 3), (8, 13), (8, 3)], ids=["one-slot", "not-a-multiple", "idle-slots"])
def test_slot_and_game_counts(pkg, G, games):
    check(pkg, (4, 4), G, games, 8)


@pytest.mark.parametrize("kw", [dict(dirichlet_epsilon=0.0), dict(reuse_pass_value=False, reuse_transpositions=False, keep_evaluations=False),
                                dict(opening_book=2), dict(rowcol=True), dict(temperature_threshold=3)],
                         ids=["no-noise", "reuse-off", "book-2-stones", "rowcol-rule", "temperature-0-from-ply-3"])
def test_options(pkg, kw):
    """The default cases above run with noise (epsilon 0.25) and evaluation reuse on (the evaluator is row-independent)."""
    check(pkg, (4, 4), 8, 20, 16, **kw)


def test_playout_cap(pkg):
    got, stats = check(pkg, (4, 4), 8, 24, 16, fast_simulations=4, full_search_probability=0.5)
    assert 0 < stats["recorded"] < stats["positions"] and got["game_id"].shape[0] == stats["recorded"]
    print("playout cap (0.5, fast 4, full 16), 24 games on 8 slots: steps issued", stats["steps_issued"])


def test_two_lanes_play_the_same_games(pkg):
    want, _ = lockstep_of(pkg, (4, 4), 8, 20, 16)
    got, stats = play(pkg, (4, 4), 8, 20, 16, True, lanes=2)
    same(got, want)
    assert stats["games_finished"] == 20


def test_two_ranks_union_is_the_one_rank_run(pkg):
    want, _ = lockstep_of(pkg, (4, 4), 8, 20, 16)
    parts = [play(pkg, (4, 4), 4, 10, 16, True, first_game_index=r, game_index_stride=2)[0] for r in range(2)]
    both = {k: np.concatenate([p[k] for p in parts]) for k in KEYS}
    order = np.lexsort((both["ply"], both["game_id"]))
    same({k: v[order] for k, v in both.items()}, want)


def test_graph_and_eager_steps_agree(pkg):
    want, _ = lockstep_of(pkg, (4, 4), 8, 20, 16)
    same(play(pkg, (4, 4), 8, 20, 16, True, use_graph=False)[0], want)
    same(play(pkg, (4, 4), 8, 20, 16, True, poll_steps=5)[0], want)


def test_second_run_continues_the_game_indices(pkg):
    """begin_run twice on one engine: the second run's games carry on from the first's indices, as in lockstep."""
    want, _ = lockstep_of(pkg, (4, 4), 8, 20, 16)
    eng = pkg.SelfPlayEngine(pkg.YinYangGame(4, 4), HashEval(), num_simulations=16, concurrent_games=8, seed=11, free_running=True)
    parts = [eng.run(12), eng.run(8)]
    eng.close()
    both = {k: np.concatenate([p[k].cpu().numpy() for p in parts]) for k in KEYS}
    assert both["game_id"][: parts[0]["game_id"].shape[0]].max() == 11
    same(both, want)


def test_split_f16_evaluator(pkg):
    import torch
    game = pkg.YinYangGame(6, 6)
    torch.manual_seed(0)
    ev = pkg.BatchedEvaluator(pkg.YinYangNeuralNetwork(game, 32, 1).cuda().eval())
    assert ev.mode == "f16x3" and ev.row_independent
    want, wstats = play(pkg, (6, 6), 8, 12, 16, False, ev=ev)
    got, gstats = play(pkg, (6, 6), 8, 12, 16, True, ev=ev)
    same(got, want)
    assert gstats["positions"] == wstats["positions"]


def test_unsupported_combinations_and_play_move_raise(pkg):
    game, ev = pkg.YinYangGame(4, 4), HashEval()
    for kw in (dict(leaves_per_step=2), dict(board_semantics="aliased"), dict(reference_quirks=True), dict(rng="numpy"),
               dict(tree_reuse=True)):
        with pytest.raises(ValueError, match="free_running"):
            pkg.SelfPlayEngine(game, ev, num_simulations=8, concurrent_games=4, free_running=True, **kw)
    for kw in (dict(leaves_per_step=2), dict(tree_reuse=True)):
        with pytest.raises(ValueError, match="free_running"):
            pkg.SelfPlayLanes(game, ev, num_simulations=8, concurrent_games=4, free_running=True, **kw)
    # the C ABI refuses what it cannot play, whatever the Python layer checked
    for kw in (dict(leaves_per_step=2), dict(aliased=True)):
        ctx = pkg.engine.BatchedMCTS(4, 4, 4, 8, **kw)
        with pytest.raises(pkg.YYError) as e:
            pkg.engine.SelfPlayRun(ctx, 0, 8, 64)
        assert e.value.code == -2
        ctx.close()
    eng = pkg.SelfPlayEngine(game, ev, num_simulations=8, concurrent_games=4, free_running=True)
    with pytest.raises(RuntimeError, match="free_running"):
        eng.play_move()
    eng.close()


def test_example_buffer_overflow_is_an_error(pkg):
    """An example buffer made too small on purpose, through the C ABI (engine.SelfPlayRun on a tree context, the steps issued
    by hand): 12 games of 16 simulations into 40 rows.  Rows are reserved with one atomic add per finished game and the counter
    only grows, so the games accepted are exactly those that finished before the first refusal.  Checked: overflow > 0 and equal
    to the games missing from the buffer; `rows` == every game's examples (the refused ones included: rows - capacity is what
    did not fit, at least); the stored rows are, game by game, the lockstep engine's examples; they end at the sum of the
    accepted games' rows, beyond which the buffer still holds the zeros it was created with (a stored row's pi sums to 1);
    the first refused game really did not fit.  The engine turns the same counters into an error."""
    import torch
    want, _ = lockstep_of(pkg, (4, 4), 8, 20, 16)
    n_of = {g: int((want["game_id"] == g).sum()) for g in range(12)}
    cap, G = 40, 4
    assert sum(n_of.values()) > cap + max(n_of.values())
    ev = HashEval(False)
    ctx = pkg.engine.BatchedMCTS(G, 4, 4, 16)
    run = pkg.engine.SelfPlayRun(ctx, 11, 16, cap)
    run.arm(12)
    for i in range(pkg.self_play.free_running_step_bound(12, G, 16, 16)):
        run.step(*ev(ctx.planes))
        if i % 64 == 63:
            event, record = run.poll_counters()
            event.synchronize()
            if run.counters(record)["finished"] == 12:
                break
    event, record = run.poll_counters()
    event.synchronize()
    c = run.counters(record)
    assert c["finished"] == 12 and c["failed"] == 0 and c["target"] == 12 and c["positions"] == sum(n_of.values())
    assert c["overflow"] > 0 and c["rows"] == sum(n_of.values()) and c["rows"] - cap > 0
    ex = {k: v.cpu().numpy() for k, v in run.examples(cap).items()}          # the WHOLE buffer
    stored = 0
    accepted = []
    while stored < cap and ex["policies"][stored].sum() > 0:                 # rows of one game are contiguous
        g = int(ex["game_id"][stored])
        assert g in n_of and g not in accepted and stored + n_of[g] <= cap, (g, stored)
        rows, ref = slice(stored, stored + n_of[g]), want["game_id"] == g
        for k in KEYS:
            assert np.array_equal(ex[k][rows], want[k][ref]), (g, k)
        accepted.append(g)
        stored += n_of[g]
    assert len(accepted) == 12 - c["overflow"] and len(accepted) >= 1
    for k in KEYS:                                                           # nothing of a refused game, nothing past the accepted rows
        assert not ex[k][stored:].any(), k
    refused = [g for g in n_of if g not in accepted]
    assert stored + max(n_of[g] for g in refused) > cap                      # the first refusal was due
    run.close()
    ctx.close()
    # the engine's reading of the same counters
    eng = pkg.SelfPlayEngine(pkg.YinYangGame(4, 4), HashEval(), num_simulations=16, concurrent_games=4, seed=11, free_running=True)
    eng._example_capacity = cap
    with pytest.raises(pkg.YYError, match="example buffer"):
        eng.run(12)
    assert eng.run_state.capacity == cap and eng.games_finished == 12
    eng.close()


def test_failed_search_is_abandoned_and_reported(pkg):
    want, _ = lockstep_of(pkg, (4, 4), 8, 20, 16, row_independent=False)
    sel = (want["game_id"] == 3) & (want["ply"] == 4)
    assert sel.sum() == 1
    import torch
    poison = torch.from_numpy(want["states"][sel][0].copy())      # game 3's position at ply 4: a leaf of its earlier searches
    eng = pkg.SelfPlayEngine(pkg.YinYangGame(4, 4), HashEval(False, poison), num_simulations=16, concurrent_games=8, seed=11,
                             free_running=True)
    with pytest.raises(pkg.YYError, match=r"(\d+) of 20 games failed") as e:
        eng.run(20)
    failed = int(str(e.value).split(" of 20 games failed")[0].split()[-1])
    got = {k: v.cpu().numpy() for k, v in eng.collect().items()}
    eng.close()
    played = np.unique(got["game_id"])
    assert failed >= 1 and 3 not in played and len(played) == 20 - failed and eng.games_finished == 20 - failed
    keep = np.isin(want["game_id"], played)
    same(got, {k: v[keep] for k, v in want.items()})


def test_cli_free_running_writes_the_same_file(tmp_path):
    import torch
    import yinyang_game_alphazero_amd as pkg
    mdir, ddir = tmp_path / "models", tmp_path / "data"
    os.makedirs(mdir)
    torch.manual_seed(0)
    pkg.YinYangNeuralNetwork(pkg.YinYangGame(6, 6)).save_model(str(mdir / "best_model.pth.tar"))
    cmd = [sys.executable, os.path.join(ROOT, "train_alphazero.py"), "--mode", "self-play", "--rows", "6", "--cols", "6",
           "--simulations", "25", "--episodes", "4", "--workers", "1", "--model-dir", str(mdir), "--data-dir", str(ddir)]
    files = []
    for extra in ([], ["--free-running"]):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        info = json.loads(r.stdout.strip().splitlines()[-1])
        z = np.load(info["data_file"])
        order = np.lexsort((z["ply"], z["game_id"]))
        files.append({k: z[k][order] for k in z.files})
        os.remove(info["data_file"])
    assert "steps_issued" in info["rank0_stats"]
    for k in files[0]:
        assert np.array_equal(files[0][k], files[1][k]), k
