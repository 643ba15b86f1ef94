"""The host rules of the first-play urgency reduction (options.resolve rule "fpu_reduction", SearchOptions.keywords, the command
line).  No device: the resolver imports neither torch nor numpy."""
import inspect
import itertools
import os
import sys

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


def test_the_range(options):
    for bad in (-0.1, float("inf"), float("nan"), "x"):
        for kw in (dict(fpu_reduction=bad), dict(fpu_reduction=0.2, fpu_reduction_root=bad)):
            with pytest.raises(options.OptionConflict) as e:
                options.resolve(64, **kw)
            assert e.value.option == "fpu_reduction" and e.value.conflicts == () and "fpu_reduction" in str(e.value)
    with pytest.raises(options.OptionConflict) as e:                # the root's value belongs to the option
        options.resolve(64, fpu_reduction_root=0.2)
    assert e.value.option == "fpu_reduction"
    o = options.resolve(64, fpu_reduction=0.2)
    assert (o.fpu_reduction, o.fpu_reduction_root) == (0.2, 0.2)     # the root defaults to the same value
    o = options.resolve(64, fpu_reduction=0.2, fpu_reduction_root=0)
    assert (o.fpu_reduction, o.fpu_reduction_root) == (0.2, 0.0)
    assert options.fpu_r(None) == options.fpu_r(0, None) == options.fpu_r(0.0, 0.0) == (0.0, 0.0)
    assert options.fpu_r(1, 2) == (1.0, 2.0)


def test_off_is_the_resolver_without_the_option(options):
    for off in (dict(), dict(fpu_reduction=None), dict(fpu_reduction=0), dict(fpu_reduction=0.0, fpu_reduction_root=0.0),
                dict(fpu_reduction=None, fpu_reduction_root=None)):
        for kw in (dict(), dict(leaves_per_step=4), dict(tree_reuse=True, fast_simulations=8, full_search_probability=0.5),
                   dict(free_running=True, evaluation_symmetry="random", symmetry_seed=3, forced_playouts=2.0),
                   dict(board_semantics="aliased", reference_quirks=True, rng="numpy")):
            o = options.resolve(64, **kw, **off)
            assert o == options.resolve(64, **kw) and o.keywords() == options.resolve(64, **kw).keywords()
            assert not any(k.startswith("fpu") for k in o.keywords())
    assert options.SearchOptions().keywords() == dict(leaves_per_step=1)


def test_keywords_forward_the_option_only_when_it_is_on(options):
    o = options.resolve(64, fpu_reduction=0.2, fpu_reduction_root=0.0, free_running=True)
    assert o.keywords() == dict(leaves_per_step=1, free_running=True, fpu_reduction=0.2, fpu_reduction_root=0.0)
    assert options.resolve(64, **{k: v for k, v in o.keywords().items()}) == o      # the next layer resolves to the same options


@pytest.mark.parametrize("kw,conflict", [(dict(reference_quirks=True), "reference_quirks"), (dict(rng="numpy"), "rng")])
def test_the_resolver_refuses(options, kw, conflict):
    with pytest.raises(options.OptionConflict) as e:
        options.resolve(64, fpu_reduction=0.2, **kw)
    assert e.value.option == "fpu_reduction" and e.value.conflicts == (conflict,)
    with pytest.raises(options.OptionConflict) as e:
        options.resolve(64, fpu_reduction=0.2, reference_quirks=True, rng="numpy")
    assert e.value.conflicts == ("reference_quirks", "rng")


def test_everything_else_is_allowed(options):
    """K > 1, aliased boards, the playout cap, tree reuse, free-running, evaluation symmetry, forced playouts, evaluation reuse
    and the book: every combination that resolves without the option resolves with it, to the same options plus the two values."""
    grid = dict(leaves_per_step=(1, 4), board_semantics=("copied", "aliased"), tree_reuse=(False, True), free_running=(False, True),
                evaluation_symmetry=("off", "random"), forced_playouts=(None, 2.0), fast_simulations=(None, 8),
                evaluation_reuse=((), (True,)), opening_book=(None, 2))
    n = 0
    for vals in itertools.product(*grid.values()):
        kw = dict(zip(grid, vals), full_search_probability=0.5)
        try:
            plain = options.resolve(64, **kw)
        except options.OptionConflict as e:
            with pytest.raises(options.OptionConflict) as e2:       # an existing refusal stays, with its present message
                options.resolve(64, fpu_reduction=0.2, **kw)
            assert (e2.value.option, e2.value.conflicts, str(e2.value)) == (e.option, e.conflicts, str(e))
            continue
        o = options.resolve(64, fpu_reduction=0.2, **kw)
        assert o == options.SearchOptions(**dict(plain.__dict__, fpu_reduction=0.2, fpu_reduction_root=0.2))
        n += 1
    assert n > 20
    assert options.resolve(64, fpu_reduction=0.2, board_semantics="aliased").fpu_reduction == 0.2


def test_the_rule_is_the_last_in_the_fixed_order(options):
    """Two broken rules: the other option's is named, with the message it has without fpu_reduction."""
    for kw in (dict(evaluation_symmetry="random", rng="numpy"), dict(forced_playouts=2.0, reference_quirks=True),
               dict(free_running=True, rng="numpy"), dict(leaves_per_step=2, reference_quirks=True), dict(fast_simulations=0, rng="numpy")):
        with pytest.raises(options.OptionConflict) as a:
            options.resolve(64, **kw)
        with pytest.raises(options.OptionConflict) as b:
            options.resolve(64, fpu_reduction=0.2, **kw)
        assert a.value.option == b.value.option != "fpu_reduction" and str(a.value) == str(b.value)


def test_every_entry_point_has_the_two_keywords():
    import yinyang_game_alphazero_amd as pkg
    sp = pkg.self_play
    for f in (pkg.engine.BatchedMCTS, pkg.MCTS, pkg.arena.AlphaZeroPlayer, pkg.Arena, pkg.evaluate_vs_random, sp._Engine.__init__,
              pkg.SelfPlayLanes, pkg.SelfPlayWorker, pkg.SelfPlayManager, pkg.AlphaZero):
        p = inspect.signature(f).parameters
        assert p["fpu_reduction"].default is None and p["fpu_reduction_root"].default is None, f
    # SelfPlayEngine hands its keywords to one of the two engines, those to the constructor they share (above), and
    # generate_self_play_data its other keywords to SelfPlayManager
    for f in (pkg.SelfPlayEngine, sp.LockstepEngine, sp.FreeRunningEngine, pkg.generate_self_play_data):
        assert any(x.kind is inspect.Parameter.VAR_KEYWORD for x in inspect.signature(f).parameters.values()), f


@pytest.mark.parametrize("mode", ["self-play", "train", "evaluate"])
def test_the_command_line(cli, mode):
    a = cli.parse_args(["--mode", mode])
    assert a.fpu_reduction is None and a.fpu_reduction_root is None and cli.refused(a) is None
    a = cli.parse_args(["--mode", mode, "--fpu-reduction", "0.2", "--fpu-reduction-root", "0"])
    assert (a.fpu_reduction, a.fpu_reduction_root) == (0.2, 0.0) and cli.refused(a) is None
    assert any("fpu_reduction" in names and "fpu_reduction_root" in names for names in cli.HANDED[mode])
    msg = cli.refused(cli.parse_args(["--mode", mode, "--fpu-reduction", "-1"]))
    assert msg and msg.startswith("train_alphazero.py: --fpu-reduction -1.0: out of range")
    assert cli.refused(cli.parse_args(["--mode", mode, "--fpu-reduction-root", "0.2"]))
    assert cli.refused(cli.parse_args(["--mode", mode, "--fpu-reduction", "0.2", "--leaves-per-step", "4"])) is None
    if mode == "self-play":
        msg = cli.refused(cli.parse_args(["--mode", mode, "--fpu-reduction", "0.2", "--reference-quirks", "--board-semantics", "aliased"]))
        assert msg and "--fpu-reduction 0.2" in msg and "--reference-quirks" in msg
        assert cli.refused(cli.parse_args(["--mode", mode, "--fpu-reduction", "0.2", "--board-semantics", "aliased"])) is None
