"""Leaf-parallel self-play (SelfPlayEngine / SelfPlayLanes / train_alphazero.py with leaves_per_step K) on the MI355X.

The games the engine must play are generated on the host, independently of it: from the empty board, every searched position
goes through the plain-numpy restatement of the K-descent search (tests/leaf_parallel_model.py, hash evaluator) with the
root noise row the engine's own kernel draws for (seed, game, ply 0), pi = counts / simulations, and the move is the engine's
sample_actions kernel on that pi.  Every example the engine records (state, pi as float32, z, ply) must equal those games bit
for bit, for K = 1, 4 and 7 (7 does not divide the 50 simulations: the last step runs one descent), replayed from graphs and
eager, through refilled slots, a packed draining tail, two lanes and the command line."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import tree_model as M
from hash_eval import hash_eval_torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PB, VB = 10, 11
SIMS, SEED, ALPHA, EPS, THR = 50, 7, 0.3, 0.25, 10          # the engine's defaults but for the simulations and the seed
BOARDS = [(4, 4), (5, 7)]                                     # 4x4: pass nodes and early terminals; 5x7: not square
KEYS = ("states", "policies", "values", "game_id", "ply")


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    import yinyang_game_alphazero_amd as p
    return p


def hash_evaluator(planes, **kw):
    return hash_eval_torch(planes, PB, VB)


# ------------------------------------------------------------------ engine runs, each made once and shared
_RUNS = {}


def run(pkg, R, C, K, use_graph=True, slots=4, games=6, row_tiers=None, lanes=None):
    """-> dict(the examples as numpy arrays, status = the tree counters, moves = play_move calls, rows = the engine's final
    row limit).  K = None builds the engine without the keyword."""
    key = (R, C, K, use_graph, slots, games, row_tiers, lanes)
    if key not in _RUNS:
        kw = dict(num_simulations=SIMS, concurrent_games=slots, seed=SEED, use_graph=use_graph, row_tiers=row_tiers)
        if K is not None:
            kw["leaves_per_step"] = K
        game = pkg.YinYangGame(R, C)
        eng = (pkg.SelfPlayEngine(game, hash_evaluator, **kw) if lanes is None
               else pkg.SelfPlayLanes(game, hash_evaluator, lanes=lanes, **kw))
        moves, play_move = [0], eng.play_move

        def counted():
            moves[0] += 1
            return play_move()

        eng.play_move = counted
        ex = eng.run(games)
        res = {k: ex[k].cpu().numpy() for k in KEYS}
        res.update(status=eng.ctx.status(), moves=moves[0], finished=eng.games_finished,
                   rows=[ln.rows for ln in eng.lanes] if lanes else eng.rows)
        eng.close()
        _RUNS[key] = res
    return _RUNS[key]


def by_game(ex):
    """{game id: (states, pi, z) in ply order}; the plies of a game are 0 .. n-1."""
    out = {}
    for g in np.unique(ex["game_id"]):
        sel = np.flatnonzero(ex["game_id"] == g)
        sel = sel[np.argsort(ex["ply"][sel])]
        assert ex["ply"][sel].tolist() == list(range(len(sel)))
        out[int(g)] = tuple(ex[k][sel] for k in ("states", "policies", "values"))
    return out


def assert_same_games(a, b):
    a, b = by_game(a), by_game(b)
    assert sorted(a) == sorted(b)
    for g in a:
        for x, y in zip(a[g], b[g]):
            assert x.shape == y.shape and np.array_equal(x, y), g


# ------------------------------------------------------------------ the games the engine must play, from the host model
_EXPECTED = {}


def expected_games(pkg, R, C, K, games=6):
    """{game id: (states int8 [n,R,C], pi float32 [n,A], z float32 [n])} and the evaluator rows all their searches asked for."""
    import torch
    key = (R, C, K, games)
    if key in _EXPECTED:
        return _EXPECTED[key]
    dev = torch.device("cuda")
    out, evals = {}, 0
    for gid in range(games):
        board, player, ply = np.zeros((R, C), np.int8), 1, 0
        states, pis, movers = [], [], []
        gid_t = torch.tensor([gid], dtype=torch.int64, device=dev)
        while True:
            if not O.valid_mask(board[None], player)[0].any():         # self_play.py:103-125: a pass, two end the game
                player = -player
                if not O.valid_mask(board[None], player)[0].any():
                    result = float(O.game_ended(board[None], player)[0]) or 1e-4
                    final_player = player
                    break
            mask = O.valid_mask(board[None], player)
            mask_t = torch.from_numpy(mask).to(dev)
            ply_t = torch.tensor([ply], dtype=torch.int32, device=dev)
            one = torch.ones(1, dtype=torch.uint8, device=dev)
            noise = None
            if ply == 0:                                                # add_noise = (step == 0): the engine's own draw
                noise = pkg.engine.root_noise(SEED, gid_t, ply_t, one, mask_t, ALPHA)[0].cpu().numpy()
            r = M.search(board, player, SIMS, K, PB, VB, noise=noise, eps=EPS)
            assert r.root_visits == SIMS == int(r.counts.sum())
            evals += r.evals
            pi = r.counts / r.counts.sum()                              # float64, as yy_mcts_root_policy divides
            states.append(board.copy())
            pis.append(pi.astype(np.float32))
            movers.append(player)
            action = pkg.engine.sample_actions(SEED, gid_t, ply_t, one, torch.from_numpy(pi[None]).to(dev), mask_t, THR)
            action = int(action[0])
            assert mask[0, action] == 1
            nb, npl, placed = O.next_state(board[None], player, np.array([action], np.int32))
            assert placed[0] == 1
            board, player, ply = nb[0], int(npl[0]), ply + 1
            ended = float(O.game_ended(board[None], player)[0])
            if ended != 0.0:
                result, final_player = ended, player
                break
        z = np.array([result if m == final_player else -result for m in movers], np.float64).astype(np.float32)
        out[gid] = (np.stack(states), np.stack(pis), z)
    _EXPECTED[key] = (out, evals)
    return _EXPECTED[key]


def assert_plays(ex, want):
    got = by_game(ex)
    assert sorted(got) == sorted(want)
    for g in want:
        for name, x, y in zip(("states", "pi", "z"), got[g], want[g]):
            assert x.shape == y.shape, (g, name, x.shape, y.shape)
            assert np.array_equal(x, y), (g, name, np.argwhere(x != y)[:3])


# ------------------------------------------------------------------ 1. each move is the pinned search
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("K", [1, 4, 7])
@pytest.mark.parametrize("R,C", BOARDS)
def test_every_move_is_the_pinned_search(pkg, R, C, K, use_graph):
    """6 games through 4 slots (slots are refilled): every recorded state, pi and label is the host model's, every action the
    sampling kernel's on that pi (else the next state would differ), and the evaluator was asked for the model's rows."""
    got = run(pkg, R, C, K, use_graph)
    want, evals = expected_games(pkg, R, C, K)
    assert got["finished"] == 6
    assert_plays(got, want)
    assert got["status"]["evals"] == evals


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("R,C", BOARDS)
def test_k1_equals_the_engine_without_the_keyword(pkg, R, C, use_graph):
    a, b = run(pkg, R, C, 1, use_graph), run(pkg, R, C, None, use_graph)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert a["status"] == b["status"] and a["moves"] == b["moves"]


# ------------------------------------------------------------------ 2. graph replay equals eager
@pytest.mark.parametrize("R,C", BOARDS)
def test_graph_replay_equals_eager(pkg, R, C):
    a, b = run(pkg, R, C, 4, True), run(pkg, R, C, 4, False)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert a["status"] == b["status"]


# ------------------------------------------------------------------ 3. games do not depend on the slot batch
@pytest.mark.parametrize("R,C", BOARDS)
def test_games_do_not_depend_on_the_slot_batch_or_the_packed_tail(pkg, R, C):
    """12 games at once, through 4 slots, and through 4 slots with a 2-game tier, so that the draining tail packs the live
    games to the front and the evaluator gets rows * K = 8 of the 16 rows: the rows * K arithmetic."""
    wide = run(pkg, R, C, 4, True, slots=12, games=12)
    narrow = run(pkg, R, C, 4, True, slots=4, games=12)
    packed = run(pkg, R, C, 4, True, slots=4, games=12, row_tiers=(2,))
    packed_eager = run(pkg, R, C, 4, False, slots=4, games=12, row_tiers=(2,))
    assert wide["rows"] == 12 and narrow["rows"] == 4 and packed["rows"] == 2 and packed_eager["rows"] == 2
    want, evals = expected_games(pkg, R, C, 4, games=12)
    for got in (wide, narrow, packed, packed_eager):
        assert got["finished"] == 12
        assert_same_games(got, wide)
        assert got["status"]["evals"] == evals
    assert_plays(wide, want)


# ------------------------------------------------------------------ 4. lanes
@pytest.mark.parametrize("R,C", BOARDS)
def test_lanes_play_the_same_games(pkg, R, C):
    lanes = run(pkg, R, C, 4, True, slots=4, games=6, lanes=2)
    single = run(pkg, R, C, 4, True)
    assert lanes["finished"] == 6
    assert_same_games(lanes, single)
    assert lanes["status"]["evals"] == single["status"]["evals"]


# ------------------------------------------------------------------ 5. counters
@pytest.mark.parametrize("R,C", BOARDS)
def test_counters_after_a_k4_run(pkg, R, C):
    got = run(pkg, R, C, 4, True)
    steps = -(-SIMS // 4)
    assert 0 < got["status"]["evals"] <= got["moves"] * steps * 4 * 4          # moves x steps x slots x K rows offered
    assert got["status"]["reused_values"] == 0 and got["status"]["transposition_hits"] == 0
    counts = np.rint(got["policies"].astype(np.float64) * SIMS)                 # pi = child visits / root visits
    assert (counts.sum(1) == SIMS).all()
    assert np.array_equal((counts / SIMS).astype(np.float32), got["policies"])


# ------------------------------------------------------------------ 6. the command line
CLI = ["--mode", "self-play", "--rows", "4", "--cols", "4", "--simulations", "16", "--episodes", "6", "--concurrent-games", "4",
       "--channels", "32", "--blocks", "1", "--fresh"]


@pytest.fixture(scope="module")
def cli_files(pkg, tmp_path_factory):
    """train_alphazero.py three times at once, each in a fresh child process under its own time limit: --leaves-per-step 4,
    --leaves-per-step 1 and no flag, from one saved network.  -> (model path, {name: loaded examples file})."""
    import torch
    top = tmp_path_factory.mktemp("cli")
    os.makedirs(top / "models")
    model = str(top / "models" / "best_model.pth.tar")
    torch.manual_seed(11)
    pkg.YinYangNeuralNetwork(pkg.YinYangGame(4, 4), 32, 1).save_model(model)
    procs = {}
    for name, extra in (("k4", ["--leaves-per-step", "4"]), ("k1", ["--leaves-per-step", "1"]), ("none", [])):
        cmd = ["timeout", "-k", "10", "150", sys.executable, os.path.join(ROOT, "train_alphazero.py")] + CLI + extra
        procs[name] = subprocess.Popen(cmd + ["--data-dir", name], cwd=str(top), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                       text=True)
    files = {}
    for name, p in procs.items():
        out, err = p.communicate()
        assert p.returncode == 0, (name, p.returncode, err[-2000:])
        found = glob.glob(str(top / name / "self_play_data_*.npz"))
        assert len(found) == 1, (name, found, out)
        with np.load(found[0]) as z:
            files[name] = {k: z[k] for k in KEYS}
    return model, files


def test_cli_self_play_with_k_writes_the_lanes_examples(pkg, cli_files):
    import torch
    model, files = cli_files
    game = pkg.YinYangGame(4, 4)
    net = pkg.YinYangNeuralNetwork(game, 32, 1)
    net.load_model(model)
    lanes = pkg.SelfPlayLanes(game, pkg.BatchedEvaluator(net.cuda().eval(), "auto"), num_simulations=16, concurrent_games=4, lanes=1,
                              seed=1000, leaves_per_step=4)
    ex = lanes.run(6)
    lanes.close()
    got = files["k4"]
    assert got["states"].shape[0] == ex["states"].shape[0] > 6
    for k in KEYS:
        assert np.array_equal(got[k], ex[k].cpu().numpy().astype(got[k].dtype)), k
    assert not np.array_equal(got["policies"], files["k1"]["policies"])         # the flag reached the searches


def test_cli_leaves_per_step_1_is_the_default(cli_files):
    _, files = cli_files
    for k in KEYS:
        assert np.array_equal(files["k1"][k], files["none"][k]), k


# ------------------------------------------------------------------ 7. the network evaluator
def movers_of(states):
    """The side that moved at every example of one game (ply order): black starts, a side without a move passes."""
    player, out = 1, []
    for s in states:
        if not O.valid_mask(s[None], player)[0].any():
            player = -player
        out.append(player)
        player = -player
    return out


def test_real_evaluator_k4_with_a_packed_tail(pkg):
    """32 channels x 1 block, f16x3 (compacted rows, static buffers, rows_hint), 5x7, 4 games, 24 simulations, K = 4, the live
    games packed into a 2-game tier while the batch drains."""
    import torch
    torch.manual_seed(5)
    game = pkg.YinYangGame(5, 7)
    ev = pkg.BatchedEvaluator(pkg.YinYangNeuralNetwork(game, 32, 1).cuda().eval(), "f16x3")
    eng = pkg.SelfPlayEngine(game, ev, num_simulations=24, concurrent_games=4, seed=3, row_tiers=(2,), leaves_per_step=4)
    assert (eng.reuse_pass_value, eng.reuse_transpositions, eng.keep_evaluations, eng.book) == (False, False, False, None)
    ex = {k: v.cpu().numpy() for k, v in eng.run(4).items()}
    status = eng.ctx.status()                                   # raises if any game failed in any search
    assert eng.games_finished == 4 and eng.rows == 2
    assert status["reused_values"] == 0 and status["transposition_hits"] == 0 and status["evals"] > 0
    eng.close()
    games = by_game(ex)
    assert sorted(games) == [0, 1, 2, 3]
    for g, (states, pi, z) in games.items():
        assert not states[0].any() and len(states) > 4
        for s, p, mover in zip(states, pi, movers_of(states)):
            legal = O.valid_mask(s[None], mover)[0].astype(bool)
            assert legal.any() and (p[~legal] == 0).all() and abs(float(p[legal].astype(np.float64).sum()) - 1.0) < 1e-6
            counts = np.rint(p.astype(np.float64) * 24)
            assert counts.sum() == 24 and np.array_equal((counts / 24).astype(np.float32), p)
        assert set(np.abs(z).tolist()) <= {1.0, float(np.float32(1e-4))}
