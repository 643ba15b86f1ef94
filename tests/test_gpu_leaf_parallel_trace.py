"""Leaf-parallel MCTS on the MI355X, descent by descent: at every step the rows k_mcts_multi flags and the boards it writes into
them, and at the end the root arrays and the six device counters, against tests/leaf_parallel_model.py with tolerance 0
(integers, bits of float32, the root's float64 sum).  MATRIX holds the smallest shapes at which each path exists (NW = 1, 2, 3;
K = 1 .. 64; every leaf kind; a root with more than 64 children; cpuct != 1; YY_FLAG_ROWCOL; sims < K);
tests/test_leaf_parallel_model.py asserts on the CPU that these cases tell every mutant of the model from the true one and
hold every leaf kind.  No C oracle exists for K > 1: the numpy restatement is the reference.

The evaluator's planes hold the board, not the side to move, so of a flagged row the board is compared; a wrong side to move
shows in the children of the node expanded from that row (its legal moves are that side's)."""
import functools

import numpy as np
import pytest

import leaf_parallel_model as M
import oracle_lib as O
from hash_eval import hash_eval_batch, hash_eval_torch, planes_to_boards
from test_leaf_parallel_model import one_move_root, pass_root, terminal_root
from tree_model import dirichlet_noise, random_root

pytestmark = pytest.mark.gpu
PB, VB = 10, 11
COUNTERS = ("evals", "levels", "children_scanned", "children_created", "terminal_revisits", "nodes")


def case(R, C, plies, sims, K, G=4, seed=1, cpuct=1.0, rowcol=False, fused=True, named=False):
    return dict(R=R, C=C, plies=plies, sims=sims, K=K, G=G, seed=seed, cpuct=cpuct, rowcol=rowcol, fused=fused, named=named)


# cheapest model first (the CPU mutant test stops at the first case that catches a mutant)
MATRIX = {
    "8x8-sims<K": case(8, 8, 4, 5, 8, G=3),
    "3x3-K4": case(3, 3, 5, 30, 4, G=6),
    "4x4-named-K8": case(4, 4, 0, 22, 8, named=True),
    "4x4-K8": case(4, 4, 9, 60, 8, G=6),
    "4x4-K16": case(4, 4, 12, 60, 16, G=6, seed=2),
    "4x4-K32": case(4, 4, 9, 70, 32, G=6, seed=10),
    "6x6-late-K8": case(6, 6, 26, 120, 8),
    "9x12-rowcol-K8": case(9, 12, 4, 50, 8, G=3, cpuct=0.5, rowcol=True),
    "8x8-K1-fused": case(8, 8, 4, 150, 1),
    "8x8-K1-split": case(8, 8, 4, 150, 1, fused=False),
    "8x8-K8": case(8, 8, 4, 150, 8),
    "12x12-cpuct-K8": case(12, 12, 40, 150, 8, G=3, cpuct=2.5),
    "12x12-empty-K64": case(12, 12, 0, 200, 64, G=3),
    "16x12-empty-K64": case(16, 12, 0, 130, 64, G=3),
    "8x8-K64": case(8, 8, 30, 300, 64, G=3),
}


def named_roots():
    """A pass root, a root with one legal move, a terminal root and an ordinary game (all 4x4)."""
    rs = [pass_root(), one_move_root(), terminal_root(), random_root(4, 4, 5, 11)]
    return np.stack([b for b, _ in rs]), np.array([p for _, p in rs], np.int8)


@functools.lru_cache(maxsize=None)
def case_roots(name):
    """-> boards int8 [G, R, C], players int8 [G], noise f64 [G, A] (odd games draw Dirichlet noise, even games none)"""
    c = MATRIX[name]
    if c["named"]:
        boards, players = named_roots()
    else:
        rs = [random_root(c["R"], c["C"], c["plies"] + (g % 3 if c["plies"] else 0), c["seed"] * 101 + g, flags=int(c["rowcol"]))
              for g in range(c["G"])]
        boards, players = np.stack([b for b, _ in rs]), np.array([p for _, p in rs], np.int8)
    noise = np.stack([dirichlet_noise(boards[g], int(players[g]), 7 + g, flags=int(c["rowcol"])) if g % 2
                      else np.zeros(boards[g].size) for g in range(len(boards))])
    for a in (boards, players, noise):
        a.setflags(write=False)
    return boards, players, noise


def run_model(boards, players, noise, sims, K, cpuct=1.0, flags=0, mutant=None, evaluator=None):
    """The model on every game of a batch -> [(Result, trace)]; a noise row of zeros is no noise."""
    out = []
    for g in range(len(boards)):
        trace = []
        nz = noise[g] if noise is not None and noise[g].any() else None
        out.append((M.search(boards[g], int(players[g]), sims, K, PB, VB, noise=nz, cpuct=cpuct, flags=flags, trace=trace,
                             mutant=mutant, evaluator=evaluator), trace))
    return out


def observables(runs, K):
    """Everything the device tests compare, from the model's runs: per game and step the K row flags and the boards of the
    flagged rows, the root arrays, and the counters summed over the games."""
    obs = dict(flags=[], boards=[], counters=dict.fromkeys(COUNTERS, 0))
    for res, trace in runs:
        fl = np.zeros((len(trace), K), np.uint8)
        bd = {}
        for s, step in enumerate(trace):
            for j, d in enumerate(step):
                fl[s, j] = d.needs_eval
                if d.needs_eval:
                    bd[(s, j)] = d.board.tobytes()
        obs["flags"].append(fl)
        obs["boards"].append(bd)
        for k in COUNTERS:
            obs["counters"][k] += getattr(res, k)
    for k in ("counts", "child_w", "child_p"):
        obs[k] = np.stack([getattr(res, k) for res, _ in runs])
    obs["visits"] = np.array([res.root_visits for res, _ in runs])
    obs["root_w"] = np.array([res.root_w for res, _ in runs], np.float64)
    return obs


def differences(got, want, games=None):
    """Names of the observables in which two sets differ (tolerance 0), with the first game / step / row that does."""
    G = len(want["flags"])
    diff = []
    for g in (range(G) if games is None else games):
        if got["flags"][g].shape != want["flags"][g].shape:
            diff.append(f"steps of game {g}: {got['flags'][g].shape[0]} != {want['flags'][g].shape[0]}")
            continue
        if not np.array_equal(got["flags"][g], want["flags"][g]):
            s, j = np.argwhere(got["flags"][g] != want["flags"][g])[0]
            diff.append(f"needs_eval of game {g} step {s} row {j}: {got['flags'][g][s]} != {want['flags'][g][s]}")
            continue
        bad = [k for k in want["boards"][g] if got["boards"][g].get(k) != want["boards"][g][k]]
        if bad:
            diff.append(f"board of game {g} (step, row) {bad[0]}")
        for k in ("counts", "child_w", "child_p", "visits", "root_w"):
            if not np.array_equal(got[k][g], want[k][g]):
                diff.append(f"{k} of game {g}")
    if games is None and got["counters"] != want["counters"]:
        diff.append(f"counters {got['counters']} != {want['counters']}")
    return diff


@functools.lru_cache(maxsize=None)
def model_observables(name, mutant=None):
    c = MATRIX[name]
    boards, players, noise = case_roots(name)
    return observables(run_model(boards, players, noise, c["sims"], c["K"], c["cpuct"], int(c["rowcol"]), mutant), c["K"])


# ------------------------------------------------------------------------------------------------- the device side
@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    import yinyang_game_alphazero_amd as p
    return p


class Tracer:
    """Evaluator wrapper: the hash evaluator on the host; every call after the root call records the needs_eval flags and,
    of the flagged rows, the board decoded from the planes."""

    def __init__(self, mc, evaluator=None):
        self.mc, self.evaluator, self.calls, self.flags, self.boards = mc, evaluator, 0, [], []

    def __call__(self, planes):
        import torch
        b = planes_to_boards(planes.cpu().numpy())
        if self.calls:
            fl = self.mc.needs_eval.cpu().numpy().reshape(self.mc.G, self.mc.K).copy()
            self.flags.append(fl)
            self.boards.append(b.reshape(self.mc.G, self.mc.K, -1))
        self.calls += 1
        if self.evaluator is not None:
            return self.evaluator(planes)
        p, v = hash_eval_batch(b, PB, VB)
        return torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda()

    def observed(self, games):
        flags = [np.stack([f[g] for f in self.flags]) if self.flags else np.zeros((0, self.mc.K), np.uint8) for g in games]
        boards = [{(s, j): self.boards[s][g, j].tobytes() for s in range(len(self.flags)) for j in range(self.mc.K)
                   if self.flags[s][g, j]} for g in games]
        return flags, boards


def root_observables(mc):
    counts, cw, cp = (t.cpu().numpy() for t in mc.root_counts(with_children=True))
    visits, wsum = (t.cpu().numpy() for t in mc.root_stats())
    return dict(counts=counts, child_w=cw, child_p=cp, visits=visits.astype(np.int64), root_w=wsum)


def device_search(pkg, boards, players, noise, sims, K, cpuct=1.0, rowcol=False, fused=True, evaluator=None, max_sims=None,
                  **kw):
    """One traced search on a fresh context -> observables in the model's form (the counters: None when status() raised)."""
    import torch
    G, R, C = boards.shape
    mc = pkg.engine.BatchedMCTS(G, R, C, max_sims or sims, cpuct=cpuct, rowcol=rowcol, leaves_per_step=K, **kw)
    try:
        tr = Tracer(mc, evaluator)
        mc.search(torch.from_numpy(np.array(boards)).cuda(), torch.from_numpy(np.array(players)).cuda(), tr, sims,
                  noise=None if noise is None else torch.from_numpy(np.array(noise)).cuda(), fused=fused)
        obs = root_observables(mc)
        obs["flags"], obs["boards"] = tr.observed(range(G))
        try:
            st = mc.status()
            obs["counters"] = {k: st[k] for k in COUNTERS}
        except pkg._lib.YYError as e:
            obs["counters"], obs["error"] = None, e
        return obs
    finally:
        mc.close()


@pytest.mark.parametrize("name", list(MATRIX))
def test_trace_equals_restatement(pkg, name):
    c = MATRIX[name]
    boards, players, noise = case_roots(name)
    got = device_search(pkg, boards, players, noise, c["sims"], c["K"], c["cpuct"], c["rowcol"], c["fused"])
    want = model_observables(name)
    keff_last = c["sims"] - (want["flags"][0].shape[0] - 1) * c["K"]
    for g in range(len(boards)):
        assert not got["flags"][g][-1, keff_last:].any(), (g, "rows past K_eff are not flagged")
    assert differences(got, want) == []


def test_named_roots_k4(pkg):
    """Pass root: one row per step and three duplicates of it; one legal move: one row, three duplicates; terminal root: no
    row at all and a python-float root sum; all in one batch with an ordinary game."""
    boards, players = named_roots()
    K = 4
    for sims in (4, 6):
        got = device_search(pkg, boards, players, None, sims, K)
        runs = run_model(boards, players, None, sims, K)
        assert [d.dup for d in runs[0][1][0]] == [-1, 0, 0, 0] and [d.kind for d in runs[0][1][0]] == [M.ROOTPASS] * 4
        assert [d.dup for d in runs[1][1][0]] == [-1, 0, 0, 0] and runs[1][1][0][0].kind == M.EXPAND
        assert runs[2][0].evals == 0 and runs[2][0].terminal_revisits == sims
        assert differences(got, observables(runs, K)) == []
        for fl in got["flags"][:2]:
            assert fl[0].tolist() == [1, 0, 0, 0]                     # the first step of both: one row, three duplicates
        assert got["flags"][0].sum(axis=1).tolist() == [1] * len(got["flags"][0])
        assert not got["flags"][2].any()
        assert got["visits"].tolist() == [sims] * 4
        tv = float(O.game_ended(boards[2][None], [int(players[2])])[0])
        assert got["root_w"][2] == sum([tv] * sims, 0.0) == runs[2][0].root_w


def uniform_eval(planes):
    import torch
    n, A = planes.shape[0], planes.shape[2] * planes.shape[3]
    return torch.full((n, A), 1.0 / A, dtype=torch.float32, device=planes.device), torch.zeros(n, device=planes.device)


def uniform_model_eval(boards):
    n, A = boards.shape[0], boards[0].size
    return np.full((n, A), 1.0 / A, np.float32), np.zeros(n, np.float32)


@pytest.mark.parametrize("R,C,sims", [(12, 12, 64), (16, 12, 64), (16, 12, 128)])
def test_uniform_evaluator_wide_root_takes_children_in_order(pkg, R, C, sims):
    """Every child of an empty root scores the same until it has a (virtual) visit: descent j of step s takes child 64 s + j,
    across the 64-child slices of the wave's arg-max (lowest index among ties, virtual counts of earlier descents seen)."""
    K, A = 64, R * C
    boards, players = np.zeros((2, R, C), np.int8), np.array([1, -1], np.int8)
    got = device_search(pkg, boards, players, None, sims, K, evaluator=uniform_eval)
    want = observables(run_model(boards, players, None, sims, K, evaluator=uniform_model_eval), K)
    assert differences(got, want) == []
    for g in range(2):
        assert got["flags"][g].shape == (sims // K, K) and got["flags"][g].all()          # no duplicates
        assert np.array_equal(got["counts"][g], (np.arange(A) < sims).astype(np.int32))
        for s in range(sims // K):
            for j in range(K):
                b = np.zeros(A, np.int8)
                b[s * K + j] = players[g]
                assert got["boards"][g][(s, j)] == b.tobytes(), (g, s, j)
    assert got["counters"]["nodes"] == got["counters"]["evals"] == 2 * sims


def test_num_sims_changes_between_graph_replays(pkg):
    """K_eff of the last step comes from device state written by set_num_sims: searches of 60, 37, 60 and 5 simulations on one
    context, the captured step replayed, each equal to the model for its own simulations and to the eager run."""
    import torch
    from yinyang_game_alphazero_amd.self_play import LockstepSearch
    R, C, G, K, max_sims = 8, 8, 4, 8, 60
    rs = [random_root(R, C, 4 + g % 3, 500 + g) for g in range(G)]
    boards, players = np.stack([b for b, _ in rs]), np.array([p for _, p in rs], np.int8)
    ev = lambda planes, **kw: hash_eval_torch(planes, PB, VB)
    want = {sims: observables(run_model(boards, players, None, sims, K), K) for sims in (60, 37, 5)}
    res = []
    for use_graph in (True, False):
        mc = pkg.engine.BatchedMCTS(G, R, C, max_sims, leaves_per_step=K)
        ls = LockstepSearch(mc, ev, use_graph=use_graph, unroll=1)
        out = []
        for sims in (60, 37, 60, 5):
            mc.reset_counters()
            ls.run(torch.from_numpy(boards).cuda(), torch.from_numpy(players).cuda(), sims)
            obs = root_observables(mc)
            st = mc.status()
            obs["counters"] = {k: st[k] for k in COUNTERS}
            for k in ("counts", "child_w", "child_p", "visits", "root_w"):
                assert np.array_equal(obs[k], want[sims][k]), (use_graph, sims, k)
            assert obs["counters"] == want[sims]["counters"], (use_graph, sims)
            out.append(obs)
        if use_graph:
            assert ls.graphs
        res.append(out)
        mc.close()
    for a, b in zip(*res):
        for k in ("counts", "child_w", "child_p", "visits", "root_w"):
            assert np.array_equal(a[k], b[k])
        assert a["counters"] == b["counters"]


def test_arena_overflow_at_k8_is_a_status(pkg):
    """A full node arena at K > 1 stops the game and raises YY_E_ARENA from status(); a game that allocates nothing (terminal
    root) in the same batch is searched to the end, and a later roomy search on a new context is clean."""
    R, C, K, sims = 8, 8, 8, 64
    tb, tp = terminal_root(R, C)
    boards = np.stack([np.zeros((R, C), np.int8), np.zeros((R, C), np.int8), tb])
    players = np.array([1, -1, tp], np.int8)
    got = device_search(pkg, boards, players, None, sims, K, nodes_per_game=8, edges_per_game=100)
    assert got["counters"] is None and got["error"].code == pkg._lib.YY_E_ARENA
    assert (got["visits"][:2] < sims).all()
    want = observables(run_model(boards, players, None, sims, K), K)
    assert differences(got, want, games=[2]) == []
    assert got["visits"][2] == sims and not got["flags"][2].any()
    roomy = device_search(pkg, boards, players, None, sims, K)
    assert roomy["counters"] is not None and differences(roomy, want) == []
