"""Free-running self-play, the parts that need no device: the host-side step bound, the argument checks that are made before
anything touches the GPU, `--free-running` parsing, and the C ABI's own refusals."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import yinyang_game_alphazero_amd as p
    return p


def test_step_bound(pkg):
    bound = pkg.self_play.free_running_step_bound
    # (ceil(num_games / G) + 1) x (A + 2) x (num_simulations + 1)
    assert bound(24, 8, 16, 16) == (3 + 1) * 18 * 17
    assert bound(20, 8, 35, 24) == (3 + 1) * 37 * 25
    assert bound(3, 8, 16, 8) == (1 + 1) * 18 * 9           # fewer games than slots
    assert bound(3, 1, 16, 8) == (3 + 1) * 18 * 9           # one slot
    assert bound(4096, 2048, 64, 800) == 3 * 66 * 801
    assert bound(0, 8, 16, 8) == 18 * 9
    # it is a bound: list scheduling of n jobs of at most L steps on G slots ends within (ceil(n / G) + 1) * L
    import random
    rnd = random.Random(0)
    for _ in range(200):
        n, G, L = rnd.randint(1, 40), rnd.randint(1, 9), rnd.randint(1, 30)
        free = [0] * G
        for _j in range(n):
            k = free.index(min(free))
            free[k] += rnd.randint(1, L)
        assert max(free) <= (-(-n // G) + 1) * L


def test_argument_checks_need_no_device(pkg):
    from yinyang_game_alphazero_amd import options

    def check(free_running, **kw):
        return options.resolve(free_running=free_running, **kw).free_running

    # off: the free-running rule checks nothing, even when every other option conflicts with it -- what the resolver still
    # refuses then is the other options' own rules (tree_reuse and leaves_per_step do not go with each other or aliased boards)
    everything = dict(leaves_per_step=4, board_semantics="aliased", reference_quirks=True, rng="numpy", tree_reuse=True)
    with pytest.raises(options.OptionConflict) as e:
        check(False, **everything)
    assert e.value.option != "free_running" and "free_running" not in str(e.value)
    assert check(False, leaves_per_step=4, rng="numpy") is False
    assert check(False, board_semantics="aliased", reference_quirks=True, rng="numpy") is False
    assert check(False, rng="numpy", tree_reuse=True) is False
    assert check(True) is True
    for kw, word in ((dict(leaves_per_step=2), "leaves_per_step=2"), (dict(board_semantics="aliased"), "aliased"),
                     (dict(reference_quirks=True), "reference_quirks"), (dict(rng="numpy"), "numpy"),
                     (dict(tree_reuse=True), "tree_reuse")):
        with pytest.raises(ValueError, match=word):
            check(True, **kw)
    # the public classes make the check before they build anything on the device (there is none here, or it is not touched)
    game = pkg.YinYangGame(4, 4)
    for cls in (pkg.SelfPlayEngine, pkg.SelfPlayLanes):
        with pytest.raises(ValueError, match="free_running=True"):
            cls(game, lambda planes: None, num_simulations=8, concurrent_games=4, free_running=True, tree_reuse=True)
    with pytest.raises(ValueError, match="free_running=True"):
        pkg.SelfPlayManager(game, "no-such-model", free_running=True, leaves_per_step=2)
    with pytest.raises(ValueError, match="free_running=True"):
        pkg.AlphaZero(game, free_running=True, tree_reuse=True)
    # SelfPlayWorker plays one game at a time through MCTS: it has no batch to free and says so
    with pytest.raises(ValueError, match="SelfPlayWorker"):
        pkg.SelfPlayWorker(game, "no-such-model", free_running=True, neural_net=object())


def test_sort_examples(pkg):
    import torch
    ex = dict(game_id=torch.tensor([5, 2, 5, 2, 9]), ply=torch.tensor([1, 3, 0, 0, 0]), values=torch.arange(5.0))
    out = pkg.self_play.sort_examples(ex)
    assert out["game_id"].tolist() == [2, 2, 5, 5, 9] and out["ply"].tolist() == [0, 3, 0, 1, 0]
    assert out["values"].tolist() == [3.0, 1.0, 2.0, 0.0, 4.0]
    empty = dict(game_id=torch.zeros(0, dtype=torch.int64), ply=torch.zeros(0, dtype=torch.int64))
    assert pkg.self_play.sort_examples(empty)["ply"].numel() == 0


def test_cli_flag(pkg):
    sys.path.insert(0, ROOT)
    import train_alphazero as cli
    assert cli.parse_args(["--mode", "self-play"]).free_running is False
    args = cli.parse_args(["--mode", "self-play", "--free-running"])
    assert args.free_running is True and cli.refused(args) is None
    assert cli.refused(cli.parse_args(["--mode", "train", "--free-running"])) is None
    for extra in (["--leaves-per-step", "2"], ["--board-semantics", "aliased"], ["--reference-quirks"], ["--tree-reuse"]):
        msg = cli.refused(cli.parse_args(["--mode", "self-play", "--free-running"] + extra))
        assert msg and "--free-running" in msg and extra[0] in msg, (extra, msg)
    assert cli.refused(cli.parse_args(["--mode", "evaluate", "--free-running"])) is None      # the flag is self-play's and train's


def test_c_abi_refuses_before_device_work(pkg):
    L = ctypes.CDLL(pkg._lib.build())
    L.yy_last_error.restype = ctypes.c_char_p
    assert L.yy_selfplay_run_create(None, None, None) == -1
    assert L.yy_selfplay_run_destroy(None) == 0
    assert L.yy_selfplay_run_arm(None, None, ctypes.c_int64(1), ctypes.c_int64(0), ctypes.c_int64(1), None, None, None) == -1
    assert L.yy_mcts_step_selfplay(None, None, None, None, None, None, None) == -1
    assert L.yy_selfplay_run_counters(None, None, None) == -1 and b"yy_selfplay_run_counters" in L.yy_last_error()
    assert L.yy_selfplay_run_examples(None, ctypes.c_int64(0), ctypes.c_int64(0), None, None, None, None, None, None) == -1
