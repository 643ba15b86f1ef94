"""Per-game simulation budgets in the tree kernels (include/yy_engine.h, yy_mcts_set_sim_budgets) and the playout-cap draw
(yy_selfplay_draw_budgets), tolerance 0: integers, bits of float32, the root's float64 sum.

K = 1: every game of a batch equals the C oracle's search of that game ALONE with its own simulation count; the six device
counters equal the sum over those single searches (copied boards: tests/leaf_parallel_model.py at K = 1, which its CPU test
pins to the oracle and which counts what the device counts; aliased boards, which that model does not have: the device's own
scalar search of each game on a context of one, plus the oracle's evaluation count).  K > 1: leaf_parallel_model per game.
The issue's budget list holds 25, which the 16x12 case (max_sims 20) caps at its max_sims: a host array is validated to
0 .. max_sims; values beyond it are the device-tensor test's."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import philox_ref as P
import tree_model as M
from hash_eval import hash_eval_torch
from test_gpu_leaf_parallel_trace import COUNTERS, PB, VB, Tracer, differences, observables, root_observables
from tree_model import dirichlet_noise, random_root

pytestmark = pytest.mark.gpu
ROOT_KEYS = ("counts", "child_w", "child_p", "visits", "root_w")


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    import yinyang_game_alphazero_amd as p
    return p


def budgets_for(max_sims):
    return np.minimum(np.array([0, 1, 2, 7, 25, max_sims, 3, 0]), max_sims).astype(np.int64)


def root_kind(board, player, flags=0):
    if O.game_ended(board[None], [player], flags)[0] != 0:
        return "terminal"
    return "play" if O.valid_mask(board[None], [player], flags)[0].any() else "pass"


@functools.lru_cache(maxsize=None)
def roots(R, C, plies, seed, G=8, flags=0, endgame=False):
    """G positions after plies + (g % 3) random plies; endgame: positions a few plies from the end of a small board, among them
    a terminal root and a pass root (found by scanning seeds on the CPU oracle), each placed on a game with a budget > 0."""
    rs = [random_root(R, C, plies + g % 3, seed * 131 + g, flags) for g in range(G)]
    if endgame:
        found = {}
        for s in range(400):
            b, p = random_root(R, C, R * C - 4 + s % 4, 7000 + s, flags)
            found.setdefault(root_kind(b, p, flags), (b, p))
        assert {"terminal", "pass"} <= set(found), sorted(found)
        rs[3], rs[4], rs[5] = found["terminal"], found["pass"], found["terminal"]
    boards, players = np.stack([b for b, _ in rs]), np.array([p for _, p in rs], np.int8)
    noise = np.stack([dirichlet_noise(boards[g], int(players[g]), 7 + g, flags=flags) if g % 2 else np.zeros(R * C)
                      for g in range(G)])
    for a in (boards, players, noise):
        a.setflags(write=False)
    return boards, players, noise


def device_search(pkg, boards, players, noise, num_sims, max_sims, K=1, fused=True, mc=None, bound=None, **kw):
    """One traced search -> observables in the form of test_gpu_leaf_parallel_trace (plus the final boards)."""
    import torch
    G, R, C = boards.shape
    own = mc is None
    if own:
        mc = pkg.engine.BatchedMCTS(G, R, C, max_sims, leaves_per_step=K, **kw)
    try:
        tr = Tracer(mc)
        mc.reset_counters()
        mc.search(torch.from_numpy(np.array(boards)).cuda(), torch.from_numpy(np.array(players)).cuda(), tr, num_sims,
                  noise=None if noise is None else torch.from_numpy(np.array(noise)).cuda(), fused=fused, num_sims_bound=bound)
        obs = root_observables(mc)
        obs["flags"], obs["boards"] = tr.observed(range(G))
        obs["final"] = mc.boards().cpu().numpy()
        obs["pi"] = mc.root_policy().cpu().numpy()
        st = mc.status()
        obs["counters"] = {k: st[k] for k in COUNTERS}
        obs["status"] = st
        return obs
    finally:
        if own:
            mc.close()


SHAPES = {"3x3": (3, 3, 40, 0, True), "4x4": (4, 4, 30, 6, False), "8x8": (8, 8, 64, 10, False), "12x12": (12, 12, 32, 20, False),
          "16x12": (16, 12, 20, 10, False)}


@functools.lru_cache(maxsize=None)
def oracle_searches(shape, aliased, with_noise, flags=0):
    R, C, max_sims, plies, endgame = SHAPES[shape]
    boards, players, noise = roots(R, C, plies, 3, flags=flags, endgame=endgame)
    b = budgets_for(max_sims)
    return [O.search_hash(boards[g], int(players[g]), int(b[g]), 0 if aliased else 1, PB, VB,
                          noise=noise[g] if with_noise and noise[g].any() else None, flags=flags) for g in range(len(boards))]


def check_k1_against_oracle(pkg, shape, fused, aliased, with_noise, rowcol=False):
    R, C, max_sims, plies, endgame = SHAPES[shape]
    flags = int(rowcol)
    boards, players, noise = roots(R, C, plies, 3, flags=flags, endgame=endgame)
    nz = noise if with_noise else None
    b = budgets_for(max_sims)
    got = device_search(pkg, boards, players, nz, b, max_sims, fused=fused, aliased=aliased, rowcol=rowcol)
    want = oracle_searches(shape, aliased, with_noise, flags)
    for g, w in enumerate(want):
        assert np.array_equal(got["counts"][g], w.counts), (g, "counts")
        assert np.array_equal(got["child_w"][g].astype(np.float64), w.child_w), (g, "child W")
        assert np.array_equal(got["child_p"][g], w.child_p), (g, "child P")
        assert got["visits"][g] == w.root_visits == b[g], (g, "root visits")
        assert got["root_w"][g] == w.root_w, (g, "root value sum")
        assert np.array_equal(got["final"][g], w.final_board if aliased else boards[g]), (g, "final board")
        fl = got["flags"][g][:, 0]
        assert fl.shape == (int(b.max()),) and not fl[int(b[g]):].any(), (g, "needs_eval after the budget is spent")
    assert got["counters"]["evals"] == sum(w.n_evals for w in want)
    if not aliased:
        runs = [(M.search(boards[g], int(players[g]), int(b[g]), 1, PB, VB, noise=nz[g] if nz is not None and nz[g].any() else None,
                          flags=flags), []) for g in range(len(boards))]
        tot = {k: sum(getattr(r, k) for r, _ in runs) for k in COUNTERS}
    else:
        tot = dict.fromkeys(COUNTERS, 0)
        for g in range(len(boards)):
            # a scalar search of 0 simulations still issues the one select after the root (and counts its descent), so the
            # single-game reference of a budget of 0 is given as a budget too
            one = device_search(pkg, boards[g:g + 1], players[g:g + 1], None if nz is None else nz[g:g + 1],
                                int(b[g]) if b[g] else b[g:g + 1], max_sims, fused=fused, aliased=True, rowcol=rowcol)
            for k in COUNTERS:
                tot[k] += one["counters"][k]
    assert got["counters"] == tot


@pytest.mark.parametrize("with_noise", [False, True], ids=["plain", "noise"])
@pytest.mark.parametrize("aliased", [False, True], ids=["copied", "aliased"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "split"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_k1_budgets_equal_the_oracle_game_by_game(pkg, shape, fused, aliased, with_noise):
    if shape == "3x3":
        R, C, _, plies, _ = SHAPES[shape]
        boards, players, _ = roots(R, C, plies, 3, endgame=True)
        kinds = {root_kind(boards[g], int(players[g])) for g in range(len(boards))}
        assert {"terminal", "pass"} <= kinds
    check_k1_against_oracle(pkg, shape, fused, aliased, with_noise)


def test_k1_budgets_with_the_row_column_rule(pkg):
    check_k1_against_oracle(pkg, "4x4", True, False, True, rowcol=True)


REUSE = {"pass": dict(reuse_pass_value=True), "tt": dict(reuse_transpositions=True), "keep": dict(keep_evaluations=True),
         "all": dict(reuse_pass_value=True, reuse_transpositions=True, keep_evaluations=True), "book": {}}


@pytest.mark.parametrize("tag", list(REUSE))
def test_k1_budgets_with_evaluation_reuse(pkg, tag):
    """Reuse flags on (each alone, all, a small book): root counts and pi equal the run with the flags off, game by game;
    every simulation is an evaluator row, a reused value, a table hit or a terminal revisit."""
    R, C, max_sims = 4, 4, 30
    boards, players, noise = roots(R, C, 6, 3)
    b = budgets_for(max_sims)
    off = device_search(pkg, boards, players, noise, b, max_sims)
    mc = pkg.engine.BatchedMCTS(len(boards), R, C, max_sims, **REUSE[tag])
    try:
        if tag == "book":
            mc.set_book(pkg.engine.OpeningBook(R, C, lambda p: hash_eval_torch(p, PB, VB), 9))
        on = device_search(pkg, boards, players, noise, b, max_sims, mc=mc)
    finally:
        mc.close()
    for k in ("counts", "pi", "visits", "root_w", "child_w"):
        assert np.array_equal(on[k], off[k]), k
    assert on["visits"].tolist() == b.tolist()
    st = on["status"]
    assert st["evals"] + st["reused_values"] + st["transposition_hits"] + st["terminal_revisits"] == int(b.sum())
    assert st["evals"] + st["reused_values"] + st["transposition_hits"] == off["status"]["evals"]
    if tag in ("tt", "keep", "book"):
        assert st["transposition_hits"] > 0
    else:                                                               # with pass values kept, the revisits of a pass node are theirs
        assert st["reused_values"] + st["transposition_hits"] > 0
    for g in range(len(boards)):
        assert not on["flags"][g][int(b[g]):, 0].any()


MULTI = {"4x4-K8": (4, 4, 9, 8, [0, 3, 8, 9, 17, 30], 30), "8x8-K64": (8, 8, 6, 64, [1, 63, 64, 65], 65),
         "16x12-K8": (16, 12, 4, 8, [0, 5, 8, 20], 20)}


@pytest.mark.parametrize("name", list(MULTI))
def test_leaf_parallel_budgets_equal_the_model_game_by_game(pkg, name):
    R, C, plies, K, b, max_sims = MULTI[name]
    boards, players, noise = roots(R, C, plies, 5, G=len(b))
    got = device_search(pkg, boards, players, noise, np.array(b), max_sims, K=K)
    steps = -(-max(b) // K)
    runs = []
    for g in range(len(b)):
        trace = []
        res = M.search(boards[g], int(players[g]), b[g], K, PB, VB, noise=noise[g] if noise[g].any() else None, trace=trace)
        runs.append((res, trace + [[]] * (steps - len(trace))))          # a game out of budget idles through the later steps
    want = observables(runs, K)
    assert differences(got, want) == []
    assert got["visits"].tolist() == b


def test_scalar_path_unchanged_and_budgets_not_sticky(pkg):
    """One context under graph replay: array, scalar, array, scalar.  The scalar searches equal those of a context that never
    saw an array; a uniform array equals the scalar; eager and replayed array searches agree."""
    import torch
    from yinyang_game_alphazero_amd.search import LockstepSearch
    R, C, max_sims, G = 8, 8, 40, 8
    boards, players, _ = roots(R, C, 10, 3)
    tb, tp = torch.from_numpy(np.array(boards)).cuda(), torch.from_numpy(np.array(players)).cuda()
    ev = lambda planes, **kw: hash_eval_torch(planes, PB, VB)
    a1, a2 = budgets_for(max_sims), np.array([40, 0, 13, 13, 1, 2, 39, 40])
    seq = [a1, 40, a2, 17, [17] * G, 17]

    def run(seq, use_graph, K=1):
        mc = pkg.engine.BatchedMCTS(G, R, C, max_sims, leaves_per_step=K)
        ls = LockstepSearch(mc, ev, use_graph=use_graph, unroll=4)
        out = []
        for n in seq:
            mc.reset_counters()
            ls.run(tb, tp, n)
            obs = root_observables(mc)
            obs["counters"] = mc.status()
            out.append(obs)
        graphs = len(ls.graphs)
        mc.close()
        return out, graphs

    def same(x, y):
        return all(np.array_equal(x[k], y[k]) for k in ROOT_KEYS) and x["counters"] == y["counters"]

    for K in (1, 4):
        mixed, graphs = run(seq, True, K)
        assert graphs > 0
        fresh, _ = run([40, 17], True, K)
        eager, _ = run(seq, False, K)
        assert same(mixed[1], fresh[0]) and same(mixed[3], fresh[1]) and same(mixed[5], fresh[1])
        assert same(mixed[4], mixed[3])                                  # uniform array == scalar
        assert all(same(x, y) for x, y in zip(mixed, eager))
        assert mixed[0]["visits"].tolist() == a1.tolist() and mixed[2]["visits"].tolist() == a2.tolist()


@pytest.mark.parametrize("K", [1, 4])
def test_device_tensor_budgets(pkg, K):
    import torch
    R, C, max_sims = 4, 4, 30
    boards, players, noise = roots(R, C, 6, 3)
    b = budgets_for(max_sims)
    host = device_search(pkg, boards, players, noise, b, max_sims, K=K)
    dev = device_search(pkg, boards, players, noise, torch.from_numpy(b.astype(np.int32)).cuda(), max_sims, K=K, bound=max_sims)
    wild = b.copy()
    wild[[0, 5, 7]] = [-5, max_sims + 1000, -(2 ** 31)]                # behave as 0, max_sims, 0
    clamped = device_search(pkg, boards, players, noise, torch.from_numpy(wild.astype(np.int32)).cuda(), max_sims, K=K, bound=max_sims)
    for got in (dev, clamped):
        assert all(np.array_equal(got[k], host[k]) for k in ROOT_KEYS) and got["counters"] == host["counters"]
        assert all(np.array_equal(x, y) for x, y in zip(got["flags"], host["flags"]))
    with pytest.raises(ValueError, match="num_sims_bound"):
        device_search(pkg, boards, players, noise, torch.from_numpy(b.astype(np.int32)).cuda(), max_sims, K=K)


def restated_budgets(seed, game_id, ply, searching, p_full, full_sims, fast_sims):
    """yy_selfplay_draw_budgets on tests/philox_ref.py: purpose 3, element 0, u from the first two words."""
    r = P.draw_np(seed, game_id, ply, 3, 0)
    full = (P.u01_np(r[0], r[1]) < p_full) & (np.asarray(searching) != 0)
    return np.where(np.asarray(searching) != 0, np.where(full, full_sims, fast_sims), 0).astype(np.int32), full.astype(np.uint8)


def test_draw_budgets_equals_the_restatement(pkg):
    import torch
    G, seed = 257, 2 ** 40 + 12345
    rng = np.random.default_rng(5)
    gid = rng.integers(0, 2 ** 40, G).astype(np.int64)
    gid[:3] = [0, 2 ** 32, 2 ** 62 + 1]
    ply = rng.integers(0, 200, G).astype(np.int32)
    searching = (rng.random(G) < 0.7).astype(np.uint8)

    def dev(order, p):
        t = lambda a: torch.from_numpy(a[order]).cuda()
        bud, full = pkg.engine.draw_budgets(seed, t(gid), t(ply), t(searching), p, 800, 100)
        return bud.cpu().numpy(), full.cpu().numpy()

    ident = np.arange(G)
    for p in (0.25, 0.5, 1.0):
        bud, full = dev(ident, p)
        wb, wf = restated_budgets(seed, gid, ply, searching, p, 800, 100)
        assert np.array_equal(bud, wb) and np.array_equal(full, wf)
        assert not bud[searching == 0].any() and not full[searching == 0].any()
        assert set(np.unique(bud[searching != 0])) <= {800, 100}
    assert 0 < wf.sum() == searching.sum()                              # p = 1: every searching game is full
    bud, full = dev(ident, 0.25)
    assert 0 < full.sum() < searching.sum()
    perm = rng.permutation(G)
    pb, pf = dev(perm, 0.25)
    assert np.array_equal(pb, bud[perm]) and np.array_equal(pf, full[perm])
