"""Playout-cap randomisation in the self-play engine (fast_simulations / full_search_probability) on the MI355X, with the hash
evaluator: off is today's engine example for example; on, every move's root holds the simulations the restated draw
(tests/philox_ref.py, purpose 3) says, the games do not depend on slots, lanes or ranks, and the recorded examples are exactly
the fully searched plies with the pi of a full search of that position alone."""
import numpy as np
import pytest

import oracle_lib as O
import philox_ref as P
import tree_model as M
from hash_eval import hash_eval_torch

pytestmark = pytest.mark.gpu
PB, VB = 10, 11
R, C, SEED, ALPHA, EPS = 6, 6, 11, 0.3, 0.25
KEYS = ("states", "policies", "values", "game_id", "ply")


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    import yinyang_game_alphazero_amd as p
    return p


def hash_evaluator(planes, **kw):
    return hash_eval_torch(planes, PB, VB)


class RowIndependent:
    """The hash evaluator as an object that declares what it is: a row's result depends on the row alone, so the engine's
    defaults turn the evaluation reuse on."""
    row_independent = True

    def __call__(self, planes, **kw):
        return hash_eval_torch(planes, PB, VB)


CONFIGS = {"K1-defaults": (RowIndependent, dict(opening_book=3)), "K1-no-reuse": (lambda: hash_evaluator, {}),
           "K4": (lambda: hash_evaluator, dict(leaves_per_step=4))}


def is_full(gid, ply, p):
    r = P.draw_np(SEED, np.asarray(gid, np.int64), np.asarray(ply, np.int64), 3, 0)
    return P.u01_np(r[0], r[1]) < p


def play(pkg, config, sims, games=32, slots=32, lanes=None, trace=None, first=0, stride=1, **cap):
    ev, kw = CONFIGS[config]
    kw = dict(kw, num_simulations=sims, concurrent_games=slots, seed=SEED, first_game_index=first, game_index_stride=stride, **cap)
    game = pkg.YinYangGame(R, C)
    eng = pkg.SelfPlayEngine(game, ev(), **kw) if lanes is None else pkg.SelfPlayLanes(game, ev(), lanes=lanes, **kw)
    if trace is not None:
        assert lanes is None
        inner = eng.search.run

        def traced(boards, rp, num_sims, **k):
            before = [t.clone() for t in (eng.game_id, eng.ply, k["active"], boards, rp)]
            inner(boards, rp, num_sims, **k)
            trace.append([t.cpu().numpy() for t in before + [eng.ctx.root_stats()[0]]])

        eng.search.run = traced
    ex = eng.run(games)
    res = {k: ex[k].cpu().numpy() for k in KEYS}
    res["positions"], res["recorded"], res["reuse"] = eng.positions, eng.recorded, eng.reuse_transpositions
    eng.close()
    return res


def keyed(ex):
    out = {(int(g), int(p)): (ex["states"][i], ex["policies"][i], ex["values"][i]) for i, (g, p) in enumerate(zip(ex["game_id"], ex["ply"]))}
    assert len(out) == len(ex["ply"])
    return out


def assert_same_examples(a, b):
    a, b = keyed(a), keyed(b)
    assert sorted(a) == sorted(b)
    for k in a:
        assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k


@pytest.mark.parametrize("config", list(CONFIGS))
def test_off_is_todays_engine(pkg, config):
    sims = 25
    base = play(pkg, config, sims)
    assert base["reuse"] == (config == "K1-defaults")
    for cap in (dict(fast_simulations=10, full_search_probability=1.0), dict(fast_simulations=None), dict(full_search_probability=1)):
        got = play(pkg, config, sims, **cap)
        for k in KEYS:
            assert np.array_equal(got[k], base[k]), (cap, k)             # row for row
        assert got["recorded"] == got["positions"] == len(base["ply"])
    # fast == full: the same games move for move, of which only the plies drawn "full" are recorded
    half = play(pkg, config, sims, fast_simulations=sims, full_search_probability=0.5)
    keep = is_full(base["game_id"], base["ply"], 0.5)
    assert 0 < keep.sum() < len(keep) and half["positions"] == base["positions"] and half["recorded"] == keep.sum()
    assert_same_examples(half, {k: base[k][keep] for k in KEYS})


@pytest.mark.parametrize("config", ["K1-defaults", "K4"])
def test_playout_cap_semantics(pkg, config):
    import torch
    full, fast, p = 40, 8, 0.5
    cap = dict(fast_simulations=fast, full_search_probability=p)
    trace = []
    got = play(pkg, config, full, games=32, slots=8, trace=trace, **cap)
    K = CONFIGS[config][1].get("leaves_per_step", 1)
    searched = {}
    for gid, ply, active, boards, rp, visits in trace:
        on = active != 0
        want = np.where(is_full(gid[on], ply[on], p), full, fast)
        assert np.array_equal(visits[on], want)                        # every move: 40 or 8 root visits, as the draw says
        for g in np.flatnonzero(on):
            searched[(int(gid[g]), int(ply[g]))] = (boards[g], int(rp[g]))
    assert sorted({g for g, _ in searched}) == list(range(32))
    full_plies = sorted(k for k in searched if is_full([k[0]], [k[1]], p)[0])
    ex = keyed(got)
    assert sorted(ex) == full_plies and 0 < len(full_plies) < len(searched)
    assert got["recorded"] == len(full_plies) and got["positions"] == len(searched)
    dev = torch.device("cuda")
    for (gid, ply), (state, pi, z) in ex.items():
        board, player = searched[(gid, ply)]
        assert np.array_equal(state, board)
        noise = None
        if ply == 0:
            mask = torch.from_numpy(O.valid_mask(board[None], player)).to(dev)
            noise = pkg.engine.root_noise(SEED, torch.tensor([gid], dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                                          torch.ones(1, dtype=torch.uint8, device=dev), mask, ALPHA)[0].cpu().numpy()
        want = (O.search_hash(board, player, full, 1, PB, VB, noise=noise, eps=EPS) if K == 1
                else M.search(board, player, full, K, PB, VB, noise=noise, eps=EPS))
        assert np.array_equal(pi, (want.counts / want.counts.sum()).astype(np.float32)), (gid, ply)
    if config == "K1-defaults":
        # a game's draws do not depend on slot, batch, lane or rank
        assert_same_examples(play(pkg, config, full, games=32, slots=32, **cap), got)
        assert_same_examples(play(pkg, config, full, games=32, slots=8, lanes=2, **cap), got)
        from yinyang_game_alphazero_amd.self_play import shard_games
        parts = [play(pkg, config, full, games=n, slots=8, first=f, stride=s, **cap) for n, f, s in (shard_games(32, r, 2) for r in range(2))]
        assert_same_examples({k: np.concatenate([x[k] for x in parts]) for k in KEYS}, got)
