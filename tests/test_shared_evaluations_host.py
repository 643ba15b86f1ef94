"""The host rules of the shared evaluation table (options.resolve rule "shared_evaluations", SearchOptions.keywords, the command
line, the keyword on every entry point, the table's symmetry tie).  No device."""
import inspect
import itertools
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def options():
    import yinyang_game_alphazero_amd.options as o
    return o


@pytest.fixture(scope="module")
def cli():
    sys.path.insert(0, ROOT)
    import train_alphazero
    return train_alphazero


def test_slot_counts_round_up_to_a_power_of_two(options):
    assert options.shared_slots(None) == options.shared_slots(False) == 0
    assert options.shared_slots(True) == options.SHARED_EVALUATIONS_DEFAULT_SLOTS == 1 << 23
    for n, want in ((1, 64), (64, 64), (65, 128), (1000, 1024), (1 << 20, 1 << 20), ((1 << 20) + 1, 1 << 21), (1 << 30, 1 << 30)):
        assert options.shared_slots(n) == want
        assert options.resolve(64, shared_evaluations=n).shared_evaluations == want
    for bad in (0, -5, (1 << 30) + 1, 2.5, "many"):
        with pytest.raises(options.OptionConflict) as e:
            options.resolve(64, shared_evaluations=bad)
        assert e.value.option == "shared_evaluations" and e.value.conflicts == ()


def test_off_is_the_resolver_without_the_option(options):
    for off in (dict(), dict(shared_evaluations=None), dict(shared_evaluations=False)):
        for kw in (dict(), dict(leaves_per_step=4), dict(board_semantics="aliased", reference_quirks=True, rng="numpy"),
                   dict(free_running=True, evaluation_symmetry="random", symmetry_seed=3, forced_playouts=2.0, fpu_reduction=0.2)):
            o = options.resolve(64, **kw, **off)
            assert o == options.resolve(64, **kw) and o.shared_evaluations == 0 and "shared_evaluations" not in o.keywords()
    assert options.SearchOptions().keywords() == dict(leaves_per_step=1)


def test_the_option_alone_and_with_every_other_option(options):
    o = options.resolve(64, shared_evaluations=True)
    assert o == options.SearchOptions(shared_evaluations=1 << 23) and o.keywords() == dict(leaves_per_step=1, shared_evaluations=1 << 23)
    assert options.resolve(64, **o.keywords()) == o                          # the next layer resolves to the same options
    grid = dict(tree_reuse=(False, True), free_running=(False, True), evaluation_symmetry=("off", "random"), forced_playouts=(None, 2.0),
                fpu_reduction=(None, 0.2), fast_simulations=(None, 8), evaluation_reuse=((), (True,), (False, False, False)),
                opening_book=(None, 2), rng=("philox", "numpy"))
    n = 0
    for vals in itertools.product(*grid.values()):
        kw = dict(zip(grid, vals), full_search_probability=0.5)
        try:
            plain = options.resolve(64, **kw)
        except options.OptionConflict as e:
            with pytest.raises(options.OptionConflict) as e2:               # an existing refusal stays, with its present message
                options.resolve(64, shared_evaluations=4096, **kw)
            assert (e2.value.option, e2.value.conflicts, str(e2.value)) == (e.option, e.conflicts, str(e))
            continue
        o = options.resolve(64, shared_evaluations=4096, **kw)
        assert o == options.SearchOptions(**dict(plain.__dict__, shared_evaluations=4096))
        assert o.keywords() == dict(plain.keywords(), shared_evaluations=4096)
        n += 1
    assert n > 100


@pytest.mark.parametrize("kw,conflicts", [(dict(board_semantics="aliased"), ("board_semantics",)),
                                          (dict(leaves_per_step=4), ("leaves_per_step",)),
                                          (dict(reference_quirks=True), ("reference_quirks",)),
                                          (dict(board_semantics="aliased", reference_quirks=True), ("board_semantics", "reference_quirks"))])
def test_the_resolver_refuses(options, kw, conflicts):
    with pytest.raises(options.OptionConflict) as e:
        options.resolve(64, shared_evaluations=True, **kw)
    # leaves_per_step > 1 with reference_quirks or aliased boards is refused by the earlier rule of leaves_per_step
    assert e.value.option == "shared_evaluations" and e.value.conflicts == conflicts
    for c in conflicts:
        assert c in str(e.value) and "shared_evaluations" in str(e.value)


def test_every_entry_point_has_the_keyword():
    import yinyang_game_alphazero_amd as pkg
    sp = pkg.self_play
    for f in (pkg.MCTS, sp._Engine.__init__, pkg.SelfPlayLanes, pkg.SelfPlayWorker, pkg.SelfPlayManager, pkg.AlphaZero):
        assert inspect.signature(f).parameters["shared_evaluations"].default is None, f
    for f in (pkg.SelfPlayEngine, sp.LockstepEngine, sp.FreeRunningEngine, pkg.generate_self_play_data):
        assert any(x.kind is inspect.Parameter.VAR_KEYWORD for x in inspect.signature(f).parameters.values()), f
    assert callable(pkg.engine.BatchedMCTS.set_shared_evaluations) and callable(pkg.engine.SharedEvaluations.clear)
    game = pkg.YinYangGame(4, 4)
    assert pkg.SelfPlayManager(game, "no-such-model", shared_evaluations=100).options.shared_evaluations == 128
    with pytest.raises(ValueError, match="shared_evaluations"):
        pkg.SelfPlayManager(game, "no-such-model", shared_evaluations=True, board_semantics="aliased")
    with pytest.raises(ValueError, match="shared_evaluations"):
        pkg.MCTS(game, None, board_semantics="aliased", shared_evaluations=True)         # the reference's default semantics
    with pytest.raises(ValueError, match="shared_evaluations"):
        pkg.SelfPlayWorker(game, "no-such-model", neural_net=object(), shared_evaluations=True)
    assert pkg.MCTS(game, None, board_semantics="copied", shared_evaluations=100).shared_evaluations == 128


@pytest.mark.parametrize("mode", ["self-play", "train"])
def test_the_command_line(cli, mode):
    a = cli.parse_args(["--mode", mode])
    assert a.shared_evaluations is None and cli.refused(a) is None
    a = cli.parse_args(["--mode", mode, "--shared-evaluations"])
    assert a.shared_evaluations is True and cli.refused(a) is None
    a = cli.parse_args(["--mode", mode, "--shared-evaluations", "100000", "--free-running"])
    assert a.shared_evaluations == 100000 and cli.refused(a) is None
    assert any("shared_evaluations" in names for names in cli.HANDED[mode])
    msg = cli.refused(cli.parse_args(["--mode", mode, "--shared-evaluations", "0"]))
    assert msg and msg.startswith("train_alphazero.py: --shared-evaluations 0: out of range")
    msg = cli.refused(cli.parse_args(["--mode", mode, "--shared-evaluations", "--leaves-per-step", "4"]))
    assert msg and msg.startswith("train_alphazero.py: --shared-evaluations: not with --leaves-per-step 4")
    if mode == "self-play":
        msg = cli.refused(cli.parse_args(["--mode", mode, "--shared-evaluations", "64", "--board-semantics", "aliased"]))
        assert msg and "--shared-evaluations 64" in msg and "--board-semantics aliased" in msg


@pytest.mark.parametrize("flag,want", [([], None), (["--shared-evaluations"], 1 << 23), (["--shared-evaluations", "1000"], 1024)])
def test_the_flag_reaches_the_manager(cli, monkeypatch, tmp_path, flag, want):
    """main() up to the manager, with the device calls and the games themselves stubbed out."""
    import torch
    import yinyang_game_alphazero_amd as pkg
    seen = {}

    class Reached(Exception):
        pass

    def games(self):
        seen["manager"] = self
        raise Reached

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(pkg.self_play.SelfPlayManager, "generate_games_parallel", games)
    (tmp_path / "best_model.pth.tar").write_bytes(b"")
    with pytest.raises(Reached):
        cli.main(["--mode", "self-play", "--rows", "4", "--cols", "4", "--model-dir", str(tmp_path), "--data-dir", str(tmp_path / "d")]
                 + flag)
    m = seen["manager"]
    assert m.options.shared_evaluations == (want or 0)
    assert m.options.keywords().get("shared_evaluations") == want


def test_a_table_of_another_symmetry_setting_is_refused():
    """BatchedMCTS.set_shared_evaluations compares board, (evaluation_symmetry, symmetry_seed) and owner before any device call:
    driven here with stand-ins for the context and the table's arrays."""
    import torch
    import yinyang_game_alphazero_amd as pkg
    eng = pkg.engine
    cpu = torch.device("cpu")
    table = eng.SharedEvaluations(4, 4, 100, device=cpu, evaluation_symmetry="random", symmetry_seed=7)
    assert table.slots == 128 and table.symmetry == ("random", 7) and table.memory_bytes == 128 * (4 + 16 + 4 + 64) + 4
    for sym in (("off", None), ("random", 8)):
        ctx = types.SimpleNamespace(R=4, C=4, symmetry=sym, device=cpu, shared=None)
        with pytest.raises(ValueError, match="evaluation_symmetry"):
            eng.BatchedMCTS.set_shared_evaluations(ctx, table)
        assert ctx.shared is None and table.ctx is None
    with pytest.raises(ValueError, match="board size"):
        eng.BatchedMCTS.set_shared_evaluations(types.SimpleNamespace(R=4, C=5, symmetry=("random", 7), device=cpu, shared=None), table)
    table.ctx = object()
    with pytest.raises(ValueError, match="another context"):
        eng.BatchedMCTS.set_shared_evaluations(types.SimpleNamespace(R=4, C=4, symmetry=("random", 7), device=cpu, shared=None), table)
