"""The plain-numpy restatement of the leaf-parallel search (tests/leaf_parallel_model.py): at K = 1 it is the reference's
search (the C oracle), and at K > 1 it gives the known answers of the semantics in include/yy_engine.h.  CPU only."""
import numpy as np
import pytest

import oracle_lib as O
import leaf_parallel_model as M
import tree_model
from tree_model import dirichlet_noise, random_root


CASES = [(3, 3, 0, 30), (3, 3, 2, 40), (6, 6, 4, 120), (8, 8, 6, 160), (16, 12, 10, 48)]


@pytest.mark.parametrize("R,C,plies,sims", CASES)
@pytest.mark.parametrize("with_noise", [False, True])
def test_k1_equals_the_oracle(R, C, plies, sims, with_noise):
    for seed in range(2):
        board, player = random_root(R, C, plies, seed)
        noise = dirichlet_noise(board, player, 100 + seed) if with_noise else None
        want = O.search_hash(board, player, sims, 1, 10, 11, noise=noise)
        got = M.search(board, player, sims, 1, 10, 11, noise=noise)
        assert np.array_equal(got.counts, want.counts)
        assert np.array_equal(got.child_w, want.child_w.astype(np.float32))
        assert np.array_equal(got.child_p, want.child_p)
        assert got.root_visits == want.root_visits == sims
        assert got.root_w == want.root_w
        assert got.evals == want.n_evals and got.steps == sims


def uniform_policy(monkeypatch, value=0.0):
    def ev(boards, pbits, vbits):
        b = np.asarray(boards)
        G, A = b.shape[0], b[0].size
        return np.full((G, A), 1.0 / 64, np.float32), np.full(G, value, np.float32)
    monkeypatch.setattr(tree_model, "hash_eval_batch", ev)


def test_fresh_root_k_children_visited_once_in_order(monkeypatch):
    uniform_policy(monkeypatch)
    board = np.zeros((3, 3), np.int8)
    k = int(O.valid_mask(board[None], [1])[0].sum())
    trace = []
    r = M.search(board, 1, k, k, trace=trace)
    assert r.steps == 1 and len(trace) == 1
    assert [p for _, p, _ in trace[0]] == [[a] for a in range(k)]     # descent j takes child j
    assert all(kind == M.EXPAND and dup == -1 for kind, _, dup in trace[0])
    assert np.array_equal(r.counts, np.ones(9, np.int32)) and r.evals == k


def pass_root():
    """A non-terminal position in which the side to move has no legal move (searched from the root as a pass)."""
    for seed in range(400):
        for plies in range(4, 30):
            board, player = random_root(4, 4, plies, seed)
            if O.game_ended(board[None], [player])[0] == 0 and not O.valid_mask(board[None], [player])[0].any():
                return board, player
    raise AssertionError("no pass root found")


def test_pass_root_one_row_four_visits():
    board, player = pass_root()
    trace = []
    r = M.search(board, player, 4, 4, trace=trace)
    assert r.steps == 1 and r.root_visits == 4 and r.evals == 1
    assert [kind for kind, _, _ in trace[0]] == [M.ROOTPASS] * 4
    assert [dup for _, _, dup in trace[0]] == [-1, 0, 0, 0]
    want = O.search_hash(board, player, 4, 1, 10, 11)
    assert r.root_w == want.root_w                                     # the same value four times


def one_move_root():
    for seed in range(400):
        for plies in range(2, 40):
            board, player = random_root(4, 4, plies, seed)
            if O.game_ended(board[None], [player])[0] == 0 and O.valid_mask(board[None], [player])[0].sum() == 1:
                return board, player
    raise AssertionError("no position with one legal move found")


def terminal_root(R=4, C=4):
    """A finished game: random play until the game has ended."""
    for seed in range(400):
        board, player = random_root(R, C, R * C + 2, seed)
        if O.game_ended(board[None], [player])[0] != 0:
            return board, player
    raise AssertionError("no terminal root found")


def test_one_legal_move_produces_duplicates():
    board, player = one_move_root()
    trace = []
    r = M.search(board, player, 3, 3, trace=trace)
    kinds = [kind for kind, _, _ in trace[0]]
    assert kinds[0] == M.EXPAND
    assert [dup for _, _, dup in trace[0]] == [-1, 0, 0]               # all three take the only edge
    assert r.evals == 1 and r.root_visits == 3 and r.counts.sum() == 3


@pytest.mark.parametrize("K", [2, 3, 8, 32])
def test_root_visits_equal_num_sims(K):
    for (R, C, plies, sims) in [(3, 3, 1, 37), (8, 8, 6, 101), (16, 12, 8, 45)]:
        board, player = random_root(R, C, plies, 7)
        r = M.search(board, player, sims, K)
        assert r.root_visits == sims
        assert r.steps == -(-sims // K)
        if O.game_ended(board[None], [player])[0] == 0 and O.valid_mask(board[None], [player])[0].any():
            assert r.counts.sum() == sims
        assert r.evals <= sims


# ---------------------------------------------------------------------------- trace boards, counters, and the GPU matrix
@pytest.mark.parametrize("R,C,plies,sims", CASES)
def test_k1_traced_boards_are_the_oracles_leaves(R, C, plies, sims):
    """The boards of the flagged rows in call order are the boards the C oracle evaluated (it does not log the root call)."""
    for seed in range(2):
        board, player = random_root(R, C, plies, seed)
        noise = dirichlet_noise(board, player, 100 + seed) if seed else None
        want = O.search_hash(board, player, sims, 1, 10, 11, noise=noise, leaf_cap=sims)
        trace = []
        got = M.search(board, player, sims, 1, 10, 11, noise=noise, trace=trace)
        leaves = [d.board for step in trace for d in step if d.needs_eval]
        assert all(len(step) == 1 for step in trace)
        assert len(leaves) == got.evals == want.n_evals == len(want.leaves) > 0
        assert np.array_equal(np.stack(leaves), want.leaves)
        for step in trace:
            for d in step:
                assert d.needs_eval == (d.kind != M.TERMINAL) and (d.board is None) == (not d.needs_eval)
                assert d.player is None or d.player == (player if len(d.actions) % 2 == 0 else -player)


def tree_recount(root):
    """levels, children_created, nodes below the root -- from the final tree alone"""
    levels = created = nodes = 0
    stack = [root]
    while stack:
        n = stack.pop()
        created += len(n.edges)
        for e in n.edges:
            levels += e.N
            if e.child is not None:
                nodes += 1
                stack.append(e.child)
    return levels, created, nodes


@pytest.mark.parametrize("K", [1, 2, 8, 32])
def test_counter_identities(K):
    for (R, C, plies, sims) in [(3, 3, 2, 40), (4, 4, 9, 60), (4, 4, 12, 37), (8, 8, 6, 101), (12, 12, 0, 70)]:
        for seed in range(3):
            board, player = random_root(R, C, plies, seed)
            trace = []
            r = M.search(board, player, sims, K, trace=trace)
            levels, created, nodes = tree_recount(r.root)
            assert r.levels == levels == sum(len(d.actions) for step in trace for d in step)
            assert r.children_created == created                      # every node with children, the root included
            assert r.nodes == nodes                                   # the root is not counted
            kinds = [d for step in trace for d in step]
            assert r.terminal_revisits == sum(d.kind == M.TERMINAL for d in kinds)
            assert r.duplicates == sum(d.dup >= 0 for d in kinds)
            assert r.evals + r.terminal_revisits + r.duplicates == r.root_visits == sims
            assert r.evals == sum(d.needs_eval for d in kinds)
            assert r.children_scanned >= r.levels and (r.levels == 0) == (r.children_scanned == 0)


@pytest.fixture(scope="module")
def gpu_matrix():
    import test_gpu_leaf_parallel_trace as T                          # the case list of the device tests, nothing of the GPU
    return T


@pytest.mark.parametrize("mutant", list(M.MUTANTS))
def test_gpu_matrix_catches_every_mutant(gpu_matrix, mutant):
    """Each deliberately broken rule differs from the true model, on at least one case of the GPU matrix, in something the
    device test compares (row flags, boards of flagged rows, root arrays, counters)."""
    T = gpu_matrix
    for name in T.MATRIX:
        if T.MATRIX[name]["K"] == 1:
            continue
        diff = T.differences(T.model_observables(name, mutant), T.model_observables(name))
        if diff:
            print(f"{mutant} ({M.MUTANTS[mutant]}): caught by {name}: {diff[0][:90]}")
            return
    raise AssertionError(f"no case of the GPU matrix tells the mutant {mutant} from the model: add a case")


def test_gpu_matrix_holds_every_leaf_kind(gpu_matrix):
    T = gpu_matrix
    seen, deep_terminal_k32 = {}, 0
    for name, c in T.MATRIX.items():
        if c["K"] < 8:
            continue
        boards, players, noise = T.case_roots(name)
        for _, trace in T.run_model(boards, players, noise, c["sims"], c["K"], c["cpuct"], int(c["rowcol"])):
            for d in (d for step in trace for d in step):
                kind = "terminal root" if d.kind == M.TERMINAL and not d.actions else d.kind
                seen.setdefault(kind, name)
                if d.dup >= 0:
                    seen.setdefault("duplicate", name)
                deep_terminal_k32 += c["K"] == 32 and d.kind == M.TERMINAL and len(d.actions) >= 1
    print(seen, deep_terminal_k32)
    assert set(seen) == {M.EXPAND, M.REEXPAND, M.ROOTPASS, M.TERMINAL, "terminal root", "duplicate"}
    assert deep_terminal_k32 >= 1
    nw = {-(-c["R"] * c["C"] // 64) for c in T.MATRIX.values()}
    assert nw == {1, 2, 3}                                            # every instantiation of the tree kernels
    assert {1, 64} <= {c["K"] for c in T.MATRIX.values()}
