"""CPU tests of the host side: the C-ABI library loads and exports every symbol include/yy_engine.h
declares (no compute without a GPU), the package fails loudly without a device, the network mirror
(checkpoint format, CPU forward), and the N>1 gather path on gloo with world_size 2."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_abi_exports_every_declared_symbol():
    import yinyang_game_alphazero_amd as pkg
    so = pkg._lib.build()
    header = open(os.path.join(ROOT, "include", "yy_engine.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+char\s*\*|int)\s*\*?\s*(yy_\w+)\s*\(", header, flags=re.M))
    assert len(declared) >= 24
    L = ctypes.CDLL(so)
    for name in declared:
        assert hasattr(L, name), name
    assert declared == set(pkg._lib.exported_symbols())
    assert L.yy_version() >= 100
    # argument validation happens before any device work
    L.yy_last_error.restype = ctypes.c_char_p
    assert L.yy_rules_valid_mask(None, None, 4, 99, 8, 0, None, None) == -2 and b"16x16" in L.yy_last_error()
    assert L.yy_rules_valid_mask(None, None, 4, 8, 8, 0, None, None) == -1
    assert L.yy_mcts_create(None, None) == -1


def test_product_path_fails_loudly_without_gpu():
    import torch
    import yinyang_game_alphazero_amd as pkg
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.YYError):
        pkg.engine.BatchedMCTS(2, 8, 8, 10)
    with pytest.raises(pkg.YYError):
        pkg.engine.valid_mask(torch.zeros((1, 8, 8), dtype=torch.int8), torch.ones(1, dtype=torch.int8))
    with pytest.raises(pkg.YYError):
        pkg.YinYangGame(8, 8).getValidMoves(pkg.YinYangLogic(8, 8), 1)


def test_product_never_imports_the_oracle():
    pkgdir = os.path.join(ROOT, "yinyang-game-alphazero_amd")
    for dirpath, _, files in os.walk(pkgdir):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle_lib" not in src and "yy_oracle" not in src and "libyy_oracle" not in src, f


def test_network_mirror_checkpoint_and_forward(tmp_path):
    import torch
    import yinyang_game_alphazero_amd as pkg
    game = pkg.YinYangGame(6, 6)
    torch.manual_seed(0)
    net = pkg.YinYangNeuralNetwork(game, 16, 2)
    names = set(net.state_dict())
    for k in ("conv1.weight", "bn1.running_mean", "res_blocks.1.conv2.bias", "res_blocks.0.bn1.weight",
              "policy_conv.weight", "policy_bn.bias", "policy_fc.weight", "value_conv.weight", "value_fc1.bias",
              "value_fc2.weight"):
        assert k in names                                    # reference layer names (neural_network.py:49-68)
    path = str(tmp_path / "m" / "best_model.pth.tar")
    net.save_model(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == {"state_dict", "board_size", "action_size"} and tuple(ck["board_size"]) == (6, 6)
    net2 = pkg.YinYangNeuralNetwork(game, 16, 2)
    net2.load_model(path)
    lb = pkg.YinYangLogic(6, 6)
    lb.board[2, 3], lb.board[0, 0] = 1, -1
    x = net.board_to_input(lb)                               # CPU module -> host planes
    import oracle_lib as O
    assert np.array_equal(x.numpy(), O.encode_planes(lb.board[None])[0])
    # the two-stone case the reference pins (src/yin_yang/ai/tests.py:82-104)
    assert x[1, 2, 3] == 1 and x[2, 0, 0] == 1 and x[0, 2, 3] == 0 and x[0, 1, 1] == 1
    assert abs(float(x[3, 2, 0]) - 1 / 6) < 1e-7 and abs(float(x[4, 0, 3]) - 1 / 6) < 1e-7
    p1, v1 = net.predict(lb)
    p2, v2 = net2.predict(lb)
    assert p1.shape == (36,) and p1.dtype == np.float32 and abs(p1.sum() - 1) < 1e-5 and -1 <= v1 <= 1
    assert np.array_equal(p1, p2) and v1 == v2
    with pytest.raises(FileNotFoundError):
        net.load_model(str(tmp_path / "missing.pth.tar"))


def test_children_distribution_known_answers():
    """mcts_tests.py:159-186, 418-445 restated on the host helper."""
    from yinyang_game_alphazero_amd.mcts import children_distribution
    c = np.zeros(9)
    c[:4] = [10, 5, 3, 1]
    p = children_distribution(c, 1.0)
    assert np.allclose(p[:4], np.array([10, 5, 3, 1]) / 19)
    p0 = children_distribution(c, 0)
    assert p0[0] == 1.0 and p0[1] == 0.0
    c2 = np.zeros(9)
    c2[:3] = [100, 50, 10]
    d1, d2, d3 = (children_distribution(c2, t) for t in (1.0, 0.5, 0.1))
    assert d1[0] - d1[1] < d2[0] - d2[1] < d3[0] - d3[1]
    assert np.allclose(children_distribution(np.zeros(9), 1.0), 1 / 9)


GATHER_SCRIPT = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
from yinyang_game_alphazero_amd.self_play import gather_examples, example_capacity
dist.init_process_group("gloo")
r, w = dist.get_rank(), dist.get_world_size()
n = 3 + 4 * r                      # ragged shards: 3 and 7 examples
ex = dict(states=torch.full((n, 4, 4), r, dtype=torch.int8), policies=torch.full((n, 16), float(r)),
          values=torch.arange(n, dtype=torch.float32) + 100 * r, game_id=torch.arange(n) * w + r,
          ply=torch.arange(n))
out = gather_examples(ex)
assert out["states"].shape == (10, 4, 4), out["states"].shape
assert out["values"].tolist() == [0, 1, 2] + [100 + i for i in range(7)]
assert out["states"][:3].eq(0).all() and out["states"][3:].eq(1).all()
assert out["game_id"].tolist() == [0, 2, 4] + [1 + 2 * i for i in range(7)]
empty = {k: v[:0] for k, v in ex.items()}
out2 = gather_examples(empty if r == 0 else ex)         # an empty shard contributes nothing
assert out2["states"].shape[0] == 7
# with the agreed capacity the exchange is exactly ONE collective (north_star: a single all-gather); count them
calls = []
real = dist.all_gather_into_tensor
dist.all_gather_into_tensor = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
saved = {name: getattr(dist, name) for name in ("all_gather", "all_reduce", "broadcast", "gather", "all_to_all")}
for name in saved:
    setattr(dist, name, (lambda nm: (lambda *a, **k: (_ for _ in ()).throw(AssertionError("unexpected collective " + nm))))(name))
cap = example_capacity(total_games=14, world=w, rows_per_game=1)     # 7 rows per rank
out3 = gather_examples(ex, capacity=cap)
assert len(calls) == 1, calls
for k in out:
    assert torch.equal(out3[k], out[k]) and out3[k].dtype == ex[k].dtype, k
try:
    gather_examples(ex, capacity=2)
    raise SystemExit("capacity overflow not detected")
except ValueError:
    pass
dist.all_gather_into_tensor = real
for name, fn in saved.items():
    setattr(dist, name, fn)
# publish: rank 0 writes, every rank returns the same complete file
from yinyang_game_alphazero_amd.self_play import publish_examples_file
from yinyang_game_alphazero_amd.training import TrainingDataQueue
path = publish_examples_file(out, sys.argv[2])
names = [None, None]
dist.all_gather_object(names, path)
assert names[0] == names[1] and os.path.exists(path), names
q = TrainingDataQueue()
q.push_file(path)
assert len(q) == 10
assert not [f for f in os.listdir(sys.argv[2]) if ".tmp" in f]
# ... and the training sample drawn from it is the SAME on every rank (rank 0's indices are broadcast): equal queue lengths,
# equal sample sizes, equal contents -- what DDP's collectives need
import random
random.seed(100 + r)                      # different host RNG states on purpose
smp = q.sample(6)
both = [None, None]
dist.all_gather_object(both, (len(q), smp["states"].tolist(), smp["values"].tolist()))
assert both[0] == both[1], "ranks drew different training samples"
dist.destroy_process_group()
print("rank", r, "ok")
'''


def test_gather_examples_gloo_world2(tmp_path):
    script = tmp_path / "gather.py"
    script.write_text(GATHER_SCRIPT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29571", str(script), ROOT, str(tmp_path / "data")],
                       capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count("ok") == 2


def test_shard_games_partitions_every_world_size():
    from yinyang_game_alphazero_amd.self_play import shard_games
    for total in (0, 1, 7, 8, 100, 4096, 4099):
        for world in (1, 2, 3, 4, 8):
            ids = []
            for r in range(world):
                n, first, stride = shard_games(total, r, world)
                ids += [first + i * stride for i in range(n)]
            assert sorted(ids) == list(range(total)), (total, world)


def test_network_mirror_reproduces_reference_outputs():
    """search_net_8x8.npz holds (board -> policy, value) pairs recorded from the REFERENCE's YinYangNeuralNetwork
    (torch.manual_seed(0), default 128 x 10, CPU) while it searched.  The mirror built with the same seed must have the
    same weights (same module construction and init order) and give the same outputs on the CPU: policy within 1e-6,
    value within 1e-6 (same torch build, so in practice identical up to thread-count-dependent summation order)."""
    import torch
    import yinyang_game_alphazero_amd as pkg
    z = np.load(os.path.join(ROOT, "tests", "golden", "search_net_8x8.npz"))
    torch.manual_seed(0)
    net = pkg.YinYangNeuralNetwork(pkg.YinYangGame(8, 8)).eval()
    n = int(z["n_rec"][0])
    boards, rp, rv = z["rec_boards"][0, :n], z["rec_policy"][0, :n], z["rec_value"][0, :n]
    import oracle_lib as O
    p, v = net.predict_batch(torch.from_numpy(O.encode_planes(boards[:24])))
    assert float(np.abs(p.numpy() - rp[:24]).max()) < 1e-6
    assert float(np.abs(v.numpy() - rv[:24]).max()) < 1e-6
    # and through the single-board API of the reference
    lb = pkg.YinYangLogic(8, 8)
    lb.board = boards[5].copy()
    p1, v1 = net.predict(lb)
    assert float(np.abs(p1 - rp[5]).max()) < 1e-6 and abs(float(v1) - float(rv[5])) < 1e-6


def test_node_view_ucb_and_backup_known_answers():
    """mcts_tests.py:117-157, 358-416 restated on the host Node view: the UCB known answer (child 1 wins: 0.8 + 0.4*sqrt(15)/6
    > 0.5 + 0.2*sqrt(15)/11), first-visit tie -> lowest action, unvisited children score q = 0, backup signs."""
    import math
    import yinyang_game_alphazero_amd as pkg
    Node = pkg.Node
    root = Node()
    for a in range(4):
        root.children[a] = Node(action=a, prior=np.float32(0.25), parent=root)
    assert root.select_child(1.0)[0] == 0                       # S = 0: every score is 0, strict > keeps the lowest action
    c0, c1 = root.children[0], root.children[1]
    c0.visits, c0.value_sum, c0.prior = 10, np.float32(5), np.float32(0.2)
    c1.visits, c1.value_sum, c1.prior = 5, np.float32(4), np.float32(0.4)
    for a in (2, 3):
        root.children[a].prior = np.float32(0.0)                # unvisited, no prior: q = 0, u = 0
    assert 0.8 + 0.4 * math.sqrt(15) / 6 > 0.5 + 0.2 * math.sqrt(15) / 11
    a, ch = root.select_child(c_puct=1.0)
    assert a == 1 and ch is c1
    # a large prior on an unvisited child beats both: u = 1.0 * 0.9 * sqrt(15) / 1
    root.children[3].prior = np.float32(0.9)
    assert root.select_child(1.0)[0] == 3
    # backup through three plies with alternating players (mcts_tests.py:389-416)
    r, c, g = Node(), Node(), Node()
    v = 0.8
    g.update(v); c.update(-v); r.update(v)
    assert (g.visits, c.visits, r.visits) == (1, 1, 1)
    assert g.value_sum == v and c.value_sum == -v and r.value_sum == v and g.get_value() == v
    # distribution helpers on the view (mcts_tests.py:159-186)
    root.children[2].visits = 5
    d = root.get_children_distribution(1.0, action_size=4)
    assert np.allclose(d, np.array([10, 5, 5, 0]) / 20.0) and d.dtype == np.float64
    assert np.array_equal(root.get_children_distribution(0, action_size=4), [1.0, 0.0, 0.0, 0.0])


def test_node_view_select_child_matches_reference_golden():
    """ucb.npz (G7): the reference's Node.select_child on 4000 random child tables -- exact ties, unvisited children,
    value sums held as np.float32 or still as python floats -- against the host Node view (same scalar types, same order)."""
    import yinyang_game_alphazero_amd as pkg
    with np.load(os.path.join(ROOT, "tests", "golden", "ucb.npz")) as f:
        z = {k: f[k] for k in f.files}          # NpzFile decompresses on every access: read each array once
    bad = 0
    for i in range(len(z["k"])):
        node = pkg.Node()
        for a in range(int(z["k"][i])):
            w = z["wsum"][i, a]
            ch = pkg.Node(action=a, prior=z["prior"][i, a], visits=int(z["visits"][i, a]),
                          value_sum=(w if z["w_is_f32"][i, a] else float(w)), parent=node)
            node.children[a] = ch
        bad += int(node.select_child(float(z["cpuct"][i]))[0] != int(z["chosen"][i]))
    assert bad == 0


def test_game_helpers_match_reference_golden():
    """symmetries.npz (G8): YinYangGame.getSymmetries against the reference's 8 (board, pi) forms, same order; plus the other
    host-only helpers (canonical form = identity, action <-> coords, stringRepresentation = the board bytes)."""
    import yinyang_game_alphazero_amd as pkg
    with np.load(os.path.join(ROOT, "tests", "golden", "symmetries.npz")) as f:
        z = {k: f[k] for k in f.files}
    for R in (4, 6, 8):
        game = pkg.YinYangGame(R, R)
        for i in range(z[f"boards_{R}"].shape[0]):
            lb = pkg.YinYangLogic(R, R)
            lb.board = z[f"boards_{R}"][i].copy()
            syms = game.getSymmetries(lb, z[f"pis_{R}"][i])
            assert len(syms) == 8
            for k, (b, p) in enumerate(syms):
                assert np.array_equal(b.get_board(), z[f"sym_boards_{R}"][i, k]) and np.array_equal(p, z[f"sym_pis_{R}"][i, k])
            assert game.getCanonicalForm(lb, -1) is lb
            assert game.stringRepresentation(lb) == z[f"boards_{R}"][i].tobytes()
        assert game._action_to_coords(R + 1) == (1, 1) and game._coords_to_action(2, 3) == 2 * R + 3
        assert game.getBoardSize() == (R, R) and game.getActionSize() == R * R


def test_philox_restatement_known_answers():
    """Random123's published Philox4x32-10 known-answer vectors pin the host restatement the GPU streams are checked against."""
    from philox_ref import philox4x32_10
    assert philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert philox4x32_10([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


BENCH_FLOW_SCRIPT = r'''
import json, os, sys, time, types
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
import bench
dist.init_process_group("gloo")
r, w = dist.get_rank(), dist.get_world_size()

class Ctx:
    evals = 0
    def reset_counters(self): self.evals = 0
    def status(self): return {"evals": self.evals}

class Eng:                      # stand-in engine: 8 games, 10 sims, rank r is slower and produces fewer positions
    G = 8
    def __init__(self): self.ctx, self.n = Ctx(), 0
    def play_move(self):
        time.sleep(0.03 * (r + 1))
        self.ctx.evals += 70 + r
        self.n += 8 - r
        return 8 - r
    def collect(self):
        n, self.n = self.n, 0
        return dict(states=torch.full((n, 4, 4), r, dtype=torch.int8), policies=torch.zeros((n, 16)), values=torch.zeros(n),
                    game_id=torch.arange(n) * w + r, ply=torch.arange(n))

leg = bench.timed_region(Eng(), steps=5, warmup=2, rank=r, world=w, dist=dist, cdev=torch.device("cpu"), sims=10, capacity=64)
assert leg["positions"] == 5 * (8 + 7), leg                       # SUM over ranks of the TIMED steps only
assert leg["evals"] == 5 * (70 + 71)
assert leg["dt"] >= 5 * 0.03 * 2 * 0.98, leg                      # MAX over ranks: the slow rank's time
assert leg["examples"] == 5 * 15 and leg["sims_total"] == 5 * 10 * 8 * 2
if r == 0:
    args = types.SimpleNamespace(sims=10, rows=4, cols=4, steps=5, warmup=2, nn="f16x3", games=8, channels=128, blocks=10,
                                 semantics="copied", quirks=False, no_graph=False)
    print("LINE " + json.dumps(bench.result_line(args, dict(leg, nn="f16x3"), w)))
dist.barrier()
dist.destroy_process_group()
'''


def test_bench_multi_rank_control_flow_gloo_world2(tmp_path):
    """The N > 1 path of bench.py (warm-up, barrier-bracketed timed region, MAX of the time and SUM of the totals over ranks,
    the single example exchange, ONE JSON line from rank 0) driven end to end with a stand-in engine on CPU tensors under
    gloo, world size 2 -- the control flow the driver runs on 2/4/8 GPUs over RCCL."""
    import json
    script = tmp_path / "bench_flow.py"
    script.write_text(BENCH_FLOW_SCRIPT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29577", str(script), ROOT],
                       capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("LINE ")]
    assert len(lines) == 1
    line = json.loads(lines[0][5:])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["n_gpus"] == 2 and line["steps"] == 5 and line["warmup"] == 2 and line["scaling"] == "weak"
    assert abs(line["value"] - 75 / (line["ms_per_step"] * 5 / 1e3)) < 1e-6 * line["value"]
    assert "10 sims" in line["metric"] and "4x4" in line["metric"] and line["vs_baseline"] is None


def test_bench_write_outputs_caps_the_size_with_a_fixed_sample(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float32/float64 .npy files only; outputs over the size cap are cut to a seeded sample of their
    rows (the same rows every time, listed in <name>_rows), outputs under it are written whole."""
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 64 << 10)
    monkeypatch.setattr(bench, "DUMP_GAME_BYTES", 16 << 10)
    rng = np.random.default_rng(0)
    games = {"pi": rng.random((64, 16)), "boards": rng.random((64, 4, 4)).astype(np.float32)}       # 12 KB: whole
    ex = {"examples_states": rng.random((4000, 4, 4)).astype(np.float32),
          "examples_values": rng.random(4000).astype(np.float32)}                                   # 272 KB: sampled
    for run in ("a", "b"):
        bench.write_outputs(str(tmp_path / run), games, ex)
    got = {p.stem: np.load(p) for p in sorted((tmp_path / "a").glob("*.npy"))}
    assert set(got) == {"pi", "boards", "examples_states", "examples_values", "examples_states_rows"}
    assert sum(a.nbytes for a in got.values()) <= 64 << 10
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["pi"], games["pi"]) and np.array_equal(got["boards"], games["boards"])
    rows = got["examples_states_rows"].astype(np.int64)
    assert 0 < len(rows) == len(got["examples_values"]) and np.all(np.diff(rows) > 0)
    assert np.array_equal(got["examples_states"], ex["examples_states"][rows])
    assert np.array_equal(got["examples_values"], ex["examples_values"][rows])
    for p in (tmp_path / "a").glob("*.npy"):
        assert np.array_equal(np.load(p), np.load(tmp_path / "b" / p.name)), p.name


def test_publish_examples_file_name_is_unique_and_leaves_no_partial(tmp_path):
    """Two publications within one second get two files (no overwrite); the temporary name does not match the loaders' glob."""
    import glob
    import torch
    from yinyang_game_alphazero_amd.self_play import publish_examples_file
    ex = dict(states=torch.zeros((3, 4, 4), dtype=torch.int8), policies=torch.full((3, 16), 1.0 / 16), values=torch.zeros(3),
              game_id=torch.arange(3), ply=torch.zeros(3, dtype=torch.int64))
    a = publish_examples_file(ex, str(tmp_path))
    b = publish_examples_file(ex, str(tmp_path))
    assert a != b and os.path.exists(a) and os.path.exists(b)
    assert sorted(glob.glob(str(tmp_path / "self_play_data_*.npz"))) == sorted([a, b])
    assert not glob.glob(str(tmp_path / "*.partial"))
    z = np.load(a)
    assert z["states"].shape == (3, 4, 4) and z["policies"].dtype == np.float64


def test_lane_counters_sum_every_reader_over_the_lanes():
    """self_play._LaneCounters: status(), shared_counters(), shared_counters_ex() and solver_counters() are the key-wise sums of
    the lanes' contexts, whatever keys a reader returns."""
    import types
    from yinyang_game_alphazero_amd.self_play import _LaneCounters
    methods = ("status", "shared_counters", "shared_counters_ex", "solver_counters")

    def lane(base):
        readings = {m: {f"{m}_k{j}": base * (i + 1) + j for j in range(3)} for i, m in enumerate(methods)}
        ctx = types.SimpleNamespace(**{m: (lambda m=m: dict(readings[m])) for m in methods})
        return types.SimpleNamespace(ctx=ctx), readings

    (a, ra), (b, rb) = lane(10), lane(1000)
    both = _LaneCounters([a, b])
    for m in methods:
        assert getattr(both, m)() == {k: ra[m][k] + rb[m][k] for k in ra[m]}, m
        assert getattr(_LaneCounters([a]), m)() == ra[m], m
