"""The tree context's counters as one array (GameState.ctr[TC_COUNT], csrc/yy_tree.h): one reset, one summing kernel, five
readers that are slices of its result.  Tolerance 0: integers.

(a) reset_counters() zeroes every counter of every family.  One case per family, each the smallest one at which the family's own
    GPU test asserts a non-zero reading: base -- eight empty 4x4 boards, 16 simulations (test_gpu_shared_replace.py,
    identical_games); forced playouts -- the 5x7 / 64 / eps 0.25 / k = 2 fixture (test_gpu_forced_playouts.py,
    test_the_forced_descent_counter_is_the_models); the replacing shared table -- 24 self-play games on 8 slots of a 64-slot
    table (test_gpu_shared_replace.py, BASE / test_same_games); solver -- the 4x4 case of tests/solver_model.py.  `live` is
    table state, not a counter: it stays.
(b) only status() consumes the sticky failure mark: the other four readers, twice each and in every order of two, return the
    same values and leave the failed game of test_gpu_mcts.py::test_nan_from_the_evaluator_is_a_sticky_error (6x6, a NaN value
    for game 2, then a clean search) for the first status() to report; the second status() is clean.
(c) 300 games -- more than one block of the summing kernel, not a multiple of 64 -- count what three contexts of 100 games count
    on the same boards.
(d) a three-word board (12x12): status() is the sum of tests/leaf_parallel_model.py at K = 1."""
import itertools

import numpy as np
import pytest

import forced_playouts_model as FM
import solver_model as SM
import tree_model as LM
from hash_eval import hash_eval_torch
from tree_model import random_root

pytestmark = pytest.mark.gpu
READERS = ("forced_descents", "solver_counters", "shared_counters", "shared_counters_ex")    # every reader but status()
MODEL_KEYS = ("evals", "levels", "children_scanned", "children_created", "terminal_revisits", "nodes")


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    import yinyang_game_alphazero_amd as p
    return p


def hash_eval(planes):
    return hash_eval_torch(planes, 10, 11)


class RowIndependent:
    """The same evaluator for the self-play engine, which asks whether a row's result depends on its batch."""
    row_independent = True

    def __call__(self, planes):
        return hash_eval(planes)


def read_all(ctx):
    """Every key of the five readers, in one dict."""
    out = {"status." + k: v for k, v in ctx.status().items()}
    out["forced_descents"] = ctx.forced_descents()
    for name in ("solver_counters", "shared_counters", "shared_counters_ex"):
        out.update({name + "." + k: v for k, v in getattr(ctx, name)().items()})
    return out


# ---- (a) the families' cases: each returns (context, what to close, the keys of its family)
def base_case(pkg):
    import torch
    ctx = pkg.engine.BatchedMCTS(8, 4, 4, 16)
    ctx.search(torch.zeros((8, 4, 4), dtype=torch.int8, device="cuda"), torch.ones(8, dtype=torch.int8, device="cuda"), hash_eval, 16)
    # 16 simulations from the empty 4x4 board end on no terminal node
    return ctx, ctx, ["status." + k for k in MODEL_KEYS if k != "terminal_revisits"]


def forced_case(pkg):
    import torch
    from test_gpu_forced_playouts import HashEval
    name, budget, eps, k = "5x7", 64, 0.25, 2.0
    boards, players, noise, _ = FM.roots(name)
    ctx = pkg.engine.BatchedMCTS(FM.GAMES, *FM.SHAPES[name], budget, forced_playouts=k)
    ctx.search(torch.from_numpy(boards).cuda(), torch.from_numpy(players).cuda(), HashEval(), budget,
               noise=torch.from_numpy(noise).cuda(), eps=eps)
    return ctx, ctx, ["forced_descents"]


def shared_case(pkg):
    eng = pkg.SelfPlayEngine(pkg.YinYangGame(4, 4), RowIndependent(), num_simulations=16, concurrent_games=8, seed=11,
                             shared_evaluations=64, shared_evaluations_replace=True)
    eng.run(24)
    return eng.ctx, eng, ["shared_counters_ex." + k for k in ("hits", "inserts", "evicted")] + ["shared_counters.hits"]


def solver_case(pkg):
    import torch
    from test_gpu_fpu import HashEval
    rows, cols, sims = SM.CASES["4x4"][:3]
    m = SM.fixture("4x4")[0]
    ctx = pkg.engine.BatchedMCTS(SM.GAMES, rows, cols, sims, solver=True)
    ctx.search(torch.from_numpy(m.boards).cuda(), torch.from_numpy(m.players).cuda(), HashEval(), sims)
    return ctx, ctx, ["solver_counters.proven_nodes", "solver_counters.proven_descents"]


@pytest.mark.parametrize("case",[base_case, forced_case, shared_case, solver_case], ids=["base", "forced", "shared-replacing", "solver"])
def test_reset_covers_every_counter(pkg, case):
    ctx, owner, family = case(pkg)
    try:
        before = read_all(ctx)
        print(before)
        for k in family:
            assert before[k] > 0, (k, before)
        if case is shared_case:
            assert before["shared_counters_ex.live"] > 0, before          # so that "unchanged" below says something
        ctx.reset_counters()
        after = read_all(ctx)
        assert set(after) == set(before)
        live = "shared_counters_ex.live"
        assert after[live] == before[live], (after[live], before[live])
        assert {k: v for k, v in after.items() if k != live and v != 0} == {}
    finally:
        owner.close()


# ---- (b)
def test_reading_does_not_disturb(pkg):
    import torch
    G = 6
    ctx = pkg.engine.BatchedMCTS(G, 6, 6, 12)
    ctx.set_shared_evaluations(pkg.engine.SharedEvaluations(6, 6, 4096, replace=True))      # non-zero shared counters to read
    boards = torch.zeros((G, 6, 6), dtype=torch.int8, device="cuda")
    players = torch.ones(G, dtype=torch.int8, device="cuda")
    state = {"calls": 0, "poison": True}

    def ev(planes):
        p, v = hash_eval_torch(planes, 6, 4)
        state["calls"] += 1
        if state["poison"] and state["calls"] == 4:
            v[2] = float("nan")
        return p, v

    try:
        ctx.search(boards, players, ev, 12)                   # finishes; game 2 stopped at the NaN, nothing faults
        state.update(calls=0, poison=False)
        ctx.search(boards, players, ev, 12)                   # a clean search: only the sticky mark is left of the failure
        first = {r: getattr(ctx, r)() for r in READERS}
        print(first)
        assert first["shared_counters"]["inserts"] > 0
        for a, b in itertools.product(READERS, repeat=2):     # each reader twice, every order of two
            assert getattr(ctx, a)() == first[a], (a, b)
            assert getattr(ctx, b)() == first[b], (a, b)
        with pytest.raises(pkg.YYError) as e:
            ctx.status()
        assert e.value.code == pkg._lib.YY_E_ARENA
        counters = ctx.status()                               # clean: the call that reported the failure cleared the mark
        assert counters["evals"] > 0
        assert {r: getattr(ctx, r)() for r in READERS} == first
    finally:
        ctx.close()


# ---- (c)
def test_more_games_than_one_block(pkg):
    import torch
    G, sims = 300, 8
    roots = [random_root(4, 4, g % 7, 9000 + g) for g in range(G)]
    boards = torch.from_numpy(np.stack([b for b, _ in roots])).cuda()
    players = torch.tensor([p for _, p in roots], dtype=torch.int8, device="cuda")

    def counted(lo, hi):
        ctx = pkg.engine.BatchedMCTS(hi - lo, 4, 4, sims)
        try:
            ctx.search(boards[lo:hi].contiguous(), players[lo:hi].contiguous(), hash_eval, sims)
            return ctx.status()
        finally:
            ctx.close()

    whole, parts = counted(0, G), [counted(lo, lo + 100) for lo in (0, 100, 200)]
    print(whole, parts)
    assert whole["evals"] > 0
    assert whole == {k: sum(p[k] for p in parts) for k in whole}


# ---- (d)
def test_a_three_word_board_counts_what_the_model_counts(pkg):
    import torch
    G, sims = 3, 8
    roots = [random_root(12, 12, 40 + g, 101 + g) for g in range(G)]
    want = dict.fromkeys(MODEL_KEYS, 0)
    for board, player in roots:
        r = LM.search(board, player, sims, 1)
        for k in MODEL_KEYS:
            want[k] += getattr(r, k)
    ctx = pkg.engine.BatchedMCTS(G, 12, 12, sims)
    try:
        ctx.search(torch.from_numpy(np.stack([b for b, _ in roots])).cuda(),
                   torch.tensor([p for _, p in roots], dtype=torch.int8, device="cuda"), hash_eval, sims)
        got = ctx.status()
    finally:
        ctx.close()
    # evaluation reuse is off in this context: the two counters the model does not have stay 0
    assert got == dict(want, reused_values=0, transposition_hits=0), (got, want)
