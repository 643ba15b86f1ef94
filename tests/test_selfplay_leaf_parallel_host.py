"""leaves_per_step K in the self-play layer, on recording stubs (no GPU): SelfPlayEngine / SelfPlayLanes hand K to the tree
context they create, the None defaults of the reuse options resolve to off at K > 1 and to today's values at K = 1, every
refused combination raises ValueError naming leaves_per_step before anything touches the device, the command line refuses its
two combinations without importing torch, and every reference-named entry point takes the keyword and forwards it."""
import contextlib
import os
import subprocess
import sys

import pytest
import torch

from yinyang_game_alphazero_amd import arena, engine, self_play

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, C, SIMS = 4, 5, 10


class Game:
    def getBoardSize(self):
        return R, C

    def getActionSize(self):
        return R * C


class Evaluator:
    """What the engine reads off an evaluator at construction."""

    def __init__(self, row_independent):
        self.row_independent = row_independent


class Context(engine.BatchedMCTS):
    """engine.BatchedMCTS with the plain fields only; every creation is kept in `made` as (G, keywords)."""
    made = []

    def __init__(self, G, R, C, max_sims, **kw):
        Context.made.append((G, kw))
        self.device = torch.device("cpu")
        self.G, self.R, self.C, self.A, self.K = G, R, C, R * C, max(1, int(kw.get("leaves_per_step", 1)))
        self.rows, self.max_sims, self._num_sims = G * self.K, max_sims, max_sims
        self.keep_evaluations = bool(kw.get("keep_evaluations"))
        self.book, self.book_version, self._evaluator_owner, self._h = None, 0, None, None

    def close(self):
        pass


@pytest.fixture
def stubs(monkeypatch):
    """The tree context replaced by the recorder and the few torch.cuda calls of SelfPlayLanes' constructor by no-ops."""
    Context.made = []
    monkeypatch.setattr(self_play.engine, "BatchedMCTS", Context)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: object())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: None)
    return Context.made


@pytest.fixture
def untouchable(monkeypatch):
    """Everything through which a constructor reaches the device appends to the returned list instead."""
    touched = []

    def touch(name):
        def f(*a, **kw):
            touched.append(name)
            raise AssertionError(f"{name} reached")
        return f

    monkeypatch.setattr(self_play.engine, "BatchedMCTS", touch("BatchedMCTS"))
    monkeypatch.setattr(self_play.engine, "OpeningBook", touch("OpeningBook"))
    monkeypatch.setattr(self_play, "MCTS", touch("MCTS"))
    monkeypatch.setattr(self_play, "YinYangNeuralNetwork", touch("YinYangNeuralNetwork"))
    for name in ("current_device", "Stream", "device", "stream", "synchronize", "is_available"):
        monkeypatch.setattr(torch.cuda, name, touch("torch.cuda." + name))
    for name in ("zeros", "ones", "full", "arange", "empty"):
        monkeypatch.setattr(torch, name, touch("torch." + name))
    return touched


FLAGS = ("reuse_pass_value", "reuse_transpositions", "keep_evaluations")


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("row_independent", [True, False])
def test_engine_hands_k_to_its_context_and_resolves_the_defaults(stubs, K, row_independent):
    eng = self_play.SelfPlayEngine(Game(), Evaluator(row_independent), num_simulations=SIMS, concurrent_games=6, device="cpu",
                                   leaves_per_step=K)
    (G, kw), = stubs
    assert G == 6 and kw["leaves_per_step"] == K and eng.ctx.K == K
    on = row_independent and K == 1                                    # today's value at K = 1, off at K > 1
    assert [kw[f] for f in FLAGS] == [on] * 3 == [getattr(eng, f) for f in FLAGS]
    assert eng.book is None and eng.ctx.book is None
    assert eng.rows == 6 and eng.tiers == [6]                          # game counts at any K


def test_engine_without_the_keyword_is_the_k1_engine(stubs):
    self_play.SelfPlayEngine(Game(), Evaluator(True), num_simulations=SIMS, concurrent_games=3, device="cpu")
    self_play.SelfPlayEngine(Game(), Evaluator(True), num_simulations=SIMS, concurrent_games=3, device="cpu", leaves_per_step=1)
    self_play.SelfPlayEngine(Game(), Evaluator(True), num_simulations=SIMS, concurrent_games=3, device="cpu", leaves_per_step=0)
    assert stubs[0] == stubs[1] == stubs[2] and stubs[0][1]["leaves_per_step"] == 1


def test_engine_at_k1_still_takes_what_k_refuses(stubs):
    self_play.SelfPlayEngine(Game(), Evaluator(False), num_simulations=SIMS, concurrent_games=3, device="cpu", leaves_per_step=1,
                             board_semantics="aliased", reference_quirks=True, reuse_transpositions=True)
    (G, kw), = stubs
    assert kw["aliased"] and kw["reuse_transpositions"] and not kw["reuse_pass_value"]


def test_explicit_false_and_a_zero_stone_book_pass_at_k(stubs):
    eng = self_play.SelfPlayEngine(Game(), Evaluator(True), num_simulations=SIMS, concurrent_games=3, device="cpu", leaves_per_step=3,
                                   reuse_pass_value=False, reuse_transpositions=False, keep_evaluations=False, opening_book=0)
    assert eng.book is None and stubs[0][1]["leaves_per_step"] == 3


@pytest.mark.parametrize("K,sims,steps", [(1, 10, 10), (4, 10, 3), (7, 50, 8), (8, 800, 100)])
def test_rows_hint_divides_by_the_steps_of_a_move(stubs, K, sims, steps):
    """finish_move: evaluator rows of the move / (ceil(sims / K) simulation steps + the root call)."""
    hints = []
    ev = Evaluator(False)
    ev.rows_hint = lambda owner, mean: hints.append((owner, mean))
    eng = self_play.SelfPlayEngine(Game(), ev, num_simulations=sims, concurrent_games=2, device="cpu", leaves_per_step=K)
    eng.ctx.status = lambda: dict(evals=1000)

    class Event:
        def synchronize(self):
            pass

    eng._pending = (torch.zeros(2, dtype=torch.int64), Event(), None, None, None)
    eng.finish_move()
    assert hints == [(id(eng.search), 1000 / float(steps + 1))]


@pytest.mark.parametrize("K", [1, 4])
def test_lanes_pass_k_to_every_lane(stubs, K):
    lanes = self_play.SelfPlayLanes(Game(), Evaluator(True), num_simulations=SIMS, concurrent_games=5, lanes=2, device="cpu",
                                    leaves_per_step=K)
    assert [g for g, _ in stubs] == [3, 2]
    assert all(kw["leaves_per_step"] == K and [kw[f] for f in FLAGS] == [K == 1] * 3 for _, kw in stubs)
    assert lanes.leaves_per_step == K and lanes.book is None and [ln.K for ln in lanes.lanes] == [K, K]
    assert lanes.reuse_pass_value == (K == 1)


class Book:
    """Stands for an engine.OpeningBook handed in by the caller."""


REFUSED = [dict(board_semantics="aliased"), dict(reference_quirks=True), dict(reuse_pass_value=True), dict(reuse_transpositions=True),
           dict(keep_evaluations=True), dict(opening_book=2), dict(opening_book=Book())]


@pytest.mark.parametrize("kw", REFUSED, ids=[next(iter(k)) + "=" + type(next(iter(k.values()))).__name__ for k in REFUSED])
@pytest.mark.parametrize("cls", [self_play.SelfPlayEngine, self_play.SelfPlayLanes])
def test_refused_combinations_raise_before_the_device(untouchable, cls, kw):
    with pytest.raises(ValueError, match="leaves_per_step"):
        cls(Game(), Evaluator(True), num_simulations=SIMS, concurrent_games=4, leaves_per_step=4, **kw)
    assert untouchable == []


@pytest.mark.parametrize("kw", [dict(board_semantics="aliased"), dict(reference_quirks=True), dict(evaluation_reuse=True),
                                dict(opening_book_stones=2)])
def test_manager_refuses_at_construction(untouchable, kw):
    with pytest.raises(ValueError, match="leaves_per_step"):
        self_play.SelfPlayManager(Game(), "none.pth.tar", leaves_per_step=4, **kw)
    self_play.SelfPlayManager(Game(), "none.pth.tar", leaves_per_step=1, **kw)          # K = 1 still takes them
    self_play.SelfPlayManager(Game(), "none.pth.tar", leaves_per_step=4, evaluation_reuse=False, opening_book_stones=0)
    assert untouchable == []


def test_worker_forwards_k_and_refuses_its_own_literal_defaults(monkeypatch, untouchable):
    made = []
    monkeypatch.setattr(self_play, "MCTS", lambda game, net, **kw: made.append(kw))
    net = object()
    self_play.SelfPlayWorker(Game(), "none", num_simulations=SIMS, neural_net=net)
    self_play.SelfPlayWorker(Game(), "none", num_simulations=SIMS, neural_net=net, board_semantics="copied", reference_quirks=False,
                             leaves_per_step=4)
    assert [kw["leaves_per_step"] for kw in made] == [1, 4]
    for kw in (dict(), dict(board_semantics="copied"), dict(reference_quirks=False)):   # aliased boards and quirks are its defaults
        with pytest.raises(ValueError, match="leaves_per_step"):
            self_play.SelfPlayWorker(Game(), "none", num_simulations=SIMS, leaves_per_step=4, **kw)
    assert len(made) == 2 and untouchable == []


class FakeLanes:
    made = []

    def __init__(self, game, evaluator, **kw):
        FakeLanes.made.append(kw)
        self.T, self.positions, self.games_finished = 1, 0, 0
        self.ctx = self

    def status(self):
        return {}

    def run(self, n):
        return dict(states=torch.zeros((0, R, C), dtype=torch.int8))

    collect = lambda self: self.run(0)

    def close(self):
        pass


class FakeNet:
    def __init__(self, *a):
        pass

    def to(self, dev):
        return self

    def eval(self):
        return self


@pytest.mark.parametrize("K,reuse,book", [(1, None, 0), (4, None, 0), (4, False, 0)])
def test_manager_forwards_k_with_reuse_as_given_and_no_book(monkeypatch, K, reuse, book):
    FakeLanes.made = []
    monkeypatch.setattr(self_play, "SelfPlayLanes", FakeLanes)
    monkeypatch.setattr(self_play, "YinYangNeuralNetwork", FakeNet)
    monkeypatch.setattr(self_play, "BatchedEvaluator", lambda net, mode: Evaluator(True))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: None)
    m = self_play.SelfPlayManager(Game(), "none.pth.tar", num_workers=1, games_per_worker=2048, num_simulations=SIMS,
                                  evaluation_reuse=reuse, leaves_per_step=K)
    m.generate_games_parallel()
    kw, = FakeLanes.made
    assert kw["leaves_per_step"] == K and kw["reuse_pass_value"] is reuse and kw["keep_evaluations"] is reuse
    # 2048 games on a 20-cell board: K = 1 with the default reuse builds the 8-stone book, K > 1 none
    assert kw["opening_book"] == (8 if K == 1 else 0)


def test_generate_self_play_data_forwards_k(monkeypatch, tmp_path):
    made = []

    class Manager:
        stats = {}

        def __init__(self, game, model_path, **kw):
            made.append(kw)

        def generate_games_parallel(self):
            return {}

    monkeypatch.setattr(self_play, "SelfPlayManager", Manager)
    monkeypatch.setattr(self_play, "publish_examples_file", lambda ex, out, ref: "file")
    self_play.generate_self_play_data(Game(), "none", str(tmp_path), num_games=4)
    self_play.generate_self_play_data(Game(), "none", str(tmp_path), num_games=4, leaves_per_step=8, seed=3)
    assert [kw["leaves_per_step"] for kw in made] == [1, 8] and made[1]["seed"] == 3


def test_alphazero_forwards_k_to_self_play_and_to_the_arena(monkeypatch, tmp_path):
    calls = {}

    class FakeArena:
        def __init__(self, game, a, b, sims, **kw):
            calls["arena"] = kw

        def play(self, n):
            return dict(a_wins=1, b_wins=1, draws=0, games=n)

    monkeypatch.setattr(arena, "generate_self_play_data", lambda *a, **kw: calls.__setitem__("self_play", kw) or "file")
    monkeypatch.setattr(arena, "Arena", FakeArena)
    monkeypatch.setattr(arena, "_load_evaluator", lambda *a: None)
    monkeypatch.setattr(arena.YinYangNeuralNetwork, "save_model", lambda self, path: open(path, "wb").close())
    for K in (1, 8):
        az = arena.AlphaZero(Game(), str(tmp_path / "m"), str(tmp_path / "d"), num_simulations=SIMS, arena_games=2, num_channels=32,
                             num_res_blocks=1, device="cpu", **({} if K == 1 else dict(leaves_per_step=K)))
        az.self_play(az.best_model_path)
        az.evaluate(az.current_model_path, az.best_model_path)
        assert calls["self_play"]["leaves_per_step"] == K and calls["arena"]["leaves_per_step"] == K


CLI = """
import sys
sys.argv = ["train_alphazero.py"] + {argv!r}
import train_alphazero
try:
    train_alphazero.main()
finally:
    print("torch imported:", "torch" in sys.modules)
"""


@pytest.mark.parametrize("flags", [["--board-semantics", "aliased"], ["--reference-quirks"]], ids=["aliased", "quirks"])
@pytest.mark.parametrize("mode", ["self-play", "train"])
def test_cli_refuses_in_one_line_without_importing_torch(mode, flags):
    argv = ["--mode", mode, "--leaves-per-step", "4"] + flags
    p = subprocess.run([sys.executable, "-c", CLI.format(argv=argv)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0
    assert "torch imported: False" in p.stdout
    err = p.stderr.strip().splitlines()
    assert len(err) == 1 and "--leaves-per-step" in err[0] and flags[0] in err[0]


def test_cli_flag_combinations_that_pass():
    import train_alphazero
    ok = [["--mode", "self-play", "--leaves-per-step", "4"], ["--mode", "train", "--leaves-per-step", "4", "--opening-book-stones", "8"],
          ["--mode", "self-play", "--leaves-per-step", "1", "--board-semantics", "aliased", "--reference-quirks"],
          ["--mode", "self-play", "--board-semantics", "aliased"], ["--mode", "evaluate", "--leaves-per-step", "4", "--reference-quirks"]]
    for argv in ok:
        assert train_alphazero.refused(train_alphazero.parse_args(argv)) is None
