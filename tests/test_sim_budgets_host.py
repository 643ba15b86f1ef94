"""Per-game simulation budgets and playout-cap randomisation on the host, on recording stubs (no GPU): every constructor and
generate_self_play_data take fast_simulations / full_search_probability and forward them -- nothing new when they are off --,
every invalid value raises ValueError naming the argument before anything touches the device, the command line takes the two
flags, run_search turns a host array of budgets into the steps of its maximum, and the restated draw keeps its law."""
import subprocess
import sys

import numpy as np
import pytest
import torch

import philox_ref as P
from test_selfplay_leaf_parallel_host import (CLI, ROOT, SIMS, Context, Evaluator, FakeLanes, FakeNet, Game, stubs,  # noqa: F401
                                              untouchable)
from yinyang_game_alphazero_amd import arena, engine, self_play

CAP = dict(fast_simulations=4, full_search_probability=0.25)
OFF = [dict(), dict(fast_simulations=None), dict(fast_simulations=4), dict(fast_simulations=4, full_search_probability=1.0),
       dict(full_search_probability=1)]
INVALID = [(dict(fast_simulations=SIMS + 1, full_search_probability=0.5), "fast_simulations"),
           (dict(fast_simulations=0, full_search_probability=0.5), "fast_simulations"),
           (dict(fast_simulations=-3), "fast_simulations"),
           (dict(fast_simulations=4, full_search_probability=0.0), "full_search_probability"),
           (dict(fast_simulations=4, full_search_probability=1.5), "full_search_probability"),
           (dict(full_search_probability=-0.1), "full_search_probability")]


def test_engine_and_lanes_take_the_arguments(stubs):
    eng = self_play.SelfPlayEngine(Game(), Evaluator(True), num_simulations=SIMS, concurrent_games=3, device="cpu", **CAP)
    assert (eng.fast_sims, eng.p_full) == (4, 0.25) and eng.hist_ply is not None
    for kw in OFF:
        eng = self_play.SelfPlayEngine(Game(), Evaluator(True), num_simulations=SIMS, concurrent_games=3, device="cpu", **kw)
        assert eng.fast_sims is None and eng.p_full == 1.0 and eng.hist_ply is None
    assert all(c == stubs[0] for c in stubs)                            # the tree context is created alike, on or off
    lanes = self_play.SelfPlayLanes(Game(), Evaluator(True), num_simulations=SIMS, concurrent_games=5, lanes=2, device="cpu", **CAP)
    assert [(ln.fast_sims, ln.p_full) for ln in lanes.lanes] == [(4, 0.25)] * 2


def test_lanes_forward_nothing_new_when_off(monkeypatch, stubs):
    made = []
    real = self_play.SelfPlayEngine

    def engine_(game, evaluator, **kw):
        made.append(kw)
        return real(game, evaluator, **kw)

    monkeypatch.setattr(self_play, "SelfPlayEngine", engine_)
    for kw in OFF:
        self_play.SelfPlayLanes(Game(), Evaluator(True), num_simulations=SIMS, concurrent_games=4, lanes=1, device="cpu", **kw)
    assert all("fast_simulations" not in kw and "full_search_probability" not in kw for kw in made) and len(made) == len(OFF)
    self_play.SelfPlayLanes(Game(), Evaluator(True), num_simulations=SIMS, concurrent_games=4, lanes=1, device="cpu", **CAP)
    assert {k: made[-1][k] for k in CAP} == CAP


@pytest.mark.parametrize("kw,name", INVALID, ids=[str(i) for i in range(len(INVALID))])
def test_invalid_values_raise_before_the_device(monkeypatch, untouchable, tmp_path, kw, name):
    monkeypatch.setattr(arena.os, "makedirs", lambda *a, **k: untouchable.append("makedirs"))
    for make in (lambda: self_play.SelfPlayEngine(Game(), Evaluator(True), num_simulations=SIMS, concurrent_games=4, **kw),
                 lambda: self_play.SelfPlayLanes(Game(), Evaluator(True), num_simulations=SIMS, concurrent_games=4, **kw),
                 lambda: self_play.SelfPlayWorker(Game(), "none", num_simulations=SIMS, **kw),
                 lambda: self_play.SelfPlayManager(Game(), "none.pth.tar", num_simulations=SIMS, **kw),
                 lambda: self_play.generate_self_play_data(Game(), "none", str(tmp_path / "d"), num_simulations=SIMS, **kw),
                 lambda: arena.AlphaZero(Game(), str(tmp_path / "m"), str(tmp_path / "d"), num_simulations=SIMS, device="cpu", **kw)):
        with pytest.raises(ValueError, match=name):
            make()
    assert untouchable == []


def test_worker_draws_only_when_on(monkeypatch, untouchable):
    monkeypatch.setattr(self_play, "MCTS", lambda game, net, **kw: None)
    w = self_play.SelfPlayWorker(Game(), "none", num_simulations=SIMS, neural_net=object(), **CAP)
    assert w.playout_cap == CAP
    for kw in OFF:
        assert self_play.SelfPlayWorker(Game(), "none", num_simulations=SIMS, neural_net=object(), **kw).playout_cap == {}


@pytest.mark.parametrize("cap", [{}, dict(fast_simulations=4), CAP])
def test_manager_generate_and_alphazero_forward(monkeypatch, tmp_path, cap):
    FakeLanes.made = []
    monkeypatch.setattr(self_play, "SelfPlayLanes", FakeLanes)
    monkeypatch.setattr(self_play, "YinYangNeuralNetwork", FakeNet)
    monkeypatch.setattr(self_play, "BatchedEvaluator", lambda net, mode: Evaluator(True))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: None)
    monkeypatch.setattr(self_play, "publish_examples_file", lambda ex, out, ref: "file")
    on = cap if len(cap) == 2 else {}
    new = ("fast_simulations", "full_search_probability")
    self_play.SelfPlayManager(Game(), "none.pth.tar", num_workers=1, games_per_worker=4, num_simulations=SIMS, **cap).generate_games_parallel()
    self_play.generate_self_play_data(Game(), "none", str(tmp_path), num_games=4, num_simulations=SIMS, **cap)
    assert len(FakeLanes.made) == 2
    for kw in FakeLanes.made:
        assert {k: kw[k] for k in new if k in kw} == on
    calls = []
    monkeypatch.setattr(arena, "generate_self_play_data", lambda *a, **kw: calls.append(kw) or "file")
    monkeypatch.setattr(arena.YinYangNeuralNetwork, "save_model", lambda self, path: open(path, "wb").close())
    az = arena.AlphaZero(Game(), str(tmp_path / "m"), str(tmp_path / "d"), num_simulations=SIMS, num_channels=32, num_res_blocks=1,
                         device="cpu", **cap)
    az.self_play(az.best_model_path)
    assert {k: calls[0][k] for k in new if k in calls[0]} == on


@pytest.mark.parametrize("mode", ["self-play", "train"])
def test_cli_takes_the_flags_and_refuses_fast_above_simulations(mode):
    import train_alphazero
    args = train_alphazero.parse_args(["--mode", mode, "--simulations", "800", "--fast-simulations", "100", "--full-search-probability", "0.25"])
    assert (args.fast_simulations, args.full_search_probability) == (100, 0.25) and train_alphazero.refused(args) is None
    args = train_alphazero.parse_args(["--mode", mode])
    assert (args.fast_simulations, args.full_search_probability) == (None, 1.0) and train_alphazero.refused(args) is None
    argv = ["--mode", mode, "--simulations", "50", "--fast-simulations", "51", "--full-search-probability", "0.5"]
    p = subprocess.run([sys.executable, "-c", CLI.format(argv=argv)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "torch imported: False" in p.stdout
    err = p.stderr.strip().splitlines()
    assert len(err) == 1 and "--fast-simulations" in err[0] and "--simulations" in err[0]
    for bad in (["--full-search-probability", "0"], ["--full-search-probability", "1.01"], ["--fast-simulations", "0"]):
        assert train_alphazero.refused(train_alphazero.parse_args(["--mode", mode] + bad)) is not None


class Recorder(Context):
    """The stub context with the C ABI calls of run_search recorded instead of made."""

    def __init__(self, G, R, C, max_sims, **kw):
        super().__init__(G, R, C, max_sims, **kw)
        self.calls, self._budgets = [], None

    def set_sim_budgets(self, budgets):
        self.calls.append(("budgets", None if budgets is None else budgets.tolist()))
        self._budgets = budgets

    def set_num_sims(self, n):
        self.calls.append(("num_sims", n))

    begin = lambda self, *a: self.calls.append("begin")
    expand_root = lambda self, *a: self.calls.append("expand_root")
    select = lambda self: self.calls.append("select")
    step = lambda self, *a: self.calls.append("step")
    expand_backup = lambda self, *a: self.calls.append("expand_backup")


@pytest.mark.parametrize("K", [1, 4])
def test_run_search_issues_the_steps_of_the_largest_budget(K):
    mc = Recorder(4, 3, 3, 20, leaves_per_step=K)
    ev = lambda root: (None, None)
    middle = []
    mc.run_search(None, None, [3, 0, 13, 7], ev, middle=middle.append)
    assert mc.calls[0] == ("budgets", [3, 0, 13, 7]) and middle == [mc.steps(13) - 1] and mc.calls[-1] == "expand_backup"
    assert mc.steps(13) == -(-13 // K)
    mc.calls.clear()
    mc.run_search(None, None, np.array([2, 2, 2, 2]), ev)
    assert mc.calls.count("step") == mc.steps(2) - 1 and mc.calls.count("expand_backup") == 1
    mc.calls.clear()
    mc.run_search(None, None, [0, 0, 0, 0], ev)                        # the root only
    assert "step" not in mc.calls and "expand_backup" not in mc.calls and mc.calls[-1] == "select"
    mc.calls.clear()
    mc.run_search(None, None, 9, ev)                                   # an int: the scalar again
    assert mc.calls[0] == ("budgets", None) and mc.calls.count("step") == mc.steps(9) - 1
    for bad in ([1, 2, 3], [1, 2, 3, 21], [0, -1, 2, 2], [1.5, 2, 2, 2], [[1, 2, 3, 4]]):
        with pytest.raises(ValueError, match="num_sims"):
            mc.run_search(None, None, bad, ev)
    with pytest.raises(engine._lib.YYError):
        mc.run_search(None, None, 21, ev)


def test_set_sim_budgets_makes_no_call_on_the_scalar_path(monkeypatch):
    mc = Context(4, 3, 3, 20)
    monkeypatch.setattr(engine, "lib", lambda: pytest.fail("an int num_sims on a context without budgets must not reach the library"))
    mc.set_sim_budgets(None)


def restated_full(seed, game, ply, p):
    r = P.draw_np(seed, game, ply, 3, 0)
    return P.u01_np(r[0], r[1]) < p


def test_the_law_of_the_restated_draw():
    """40 000 (game, ply) keys at P = 0.25: the full share lies within 5 sqrt(P (1 - P) / N) = 0.0108 of P (seeds 0 .. 3 gave
    0.2466, 0.2478, 0.2494, 0.2510 on the CPU before seed 1 was fixed here), and the draw is its own stream: not the move's."""
    n, p = 40000, 0.25
    game, ply = np.arange(n) // 100, np.arange(n) % 100
    share = restated_full(1, game, ply, p).mean()
    assert abs(share - p) < 5 * np.sqrt(p * (1 - p) / n) < 0.0109
    move = P.draw_np(1, game, ply, 1, 0)
    assert not np.array_equal(restated_full(1, game, ply, p), P.u01_np(move[0], move[1]) < p)
    assert restated_full(1, game, ply, 1.0).all()
