"""The plain-numpy restatement of the leaf-parallel search (tests/leaf_parallel_model.py): at K = 1 it is the reference's
search (the C oracle), and at K > 1 it gives the known answers of the semantics in include/yy_engine.h.  CPU only."""
import numpy as np
import pytest

import oracle_lib as O
import leaf_parallel_model as M


def random_root(R, C, plies, seed):
    """A position after `plies` random legal moves from the empty board (fewer when the game ends first), side to move."""
    rng = np.random.default_rng(seed)
    board, player = np.zeros((1, R, C), np.int8), np.ones(1, np.int8)
    for _ in range(plies):
        m = O.valid_mask(board, player)[0]
        if not m.any() or O.game_ended(board, player)[0] != 0:
            break
        board, player, _ = O.next_state(board, player, np.array([rng.choice(np.flatnonzero(m))], np.int32))
    return board[0], int(player[0])


def dirichlet_noise(board, player, seed, alpha=0.3):
    legal = np.flatnonzero(O.valid_mask(board[None], [player])[0])
    nz = np.zeros(board.size)
    if len(legal):
        nz[legal] = np.random.default_rng(seed).dirichlet([alpha] * len(legal))
    return nz


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
    monkeypatch.setattr(M, "hash_eval_batch", ev)


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
