"""gumbel_interior in the options resolver, its two views, every constructor that takes gumbel_root and the command line (no GPU)."""
import inspect

import pytest

from yinyang_game_alphazero_amd import arena, engine, mcts, options, self_play


class Game:
    rowcol_rule = False

    def getBoardSize(self):
        return 4, 4

    def getActionSize(self):
        return 16


def test_without_gumbel_root_it_is_refused_naming_gumbel_root():
    for kw in (dict(), dict(gumbel_root=0), dict(gumbel_root=None)):
        with pytest.raises(options.OptionConflict) as e:
            options.resolve(num_simulations=16, gumbel_interior=True, **kw)
        assert (e.value.option, e.value.conflicts) == ("gumbel_root", ())
    with pytest.raises(options.OptionConflict) as e:
        options.resolve(gumbel_root=4, gumbel_interior="yes")
    assert e.value.option == "gumbel_root"


def test_with_fpu_reduction_it_is_refused_naming_gumbel_root():
    with pytest.raises(options.OptionConflict) as e:
        options.resolve(num_simulations=16, gumbel_root=4, gumbel_interior=True, fpu_reduction=0.2)
    assert (e.value.option, e.value.conflicts) == ("gumbel_root", ("fpu_reduction",)) and "fpu_reduction=0.2" in str(e.value)
    # off, or without the sub-option, first-play urgency goes with the Gumbel root search as before
    assert options.resolve(gumbel_root=4, gumbel_interior=True, fpu_reduction=0).fpu_reduction == 0.0
    assert options.resolve(gumbel_root=4, fpu_reduction=0.2).fpu_reduction == 0.2
    assert options.resolve(gumbel_root=4, gumbel_interior=False, fpu_reduction=0.2).gumbel_interior is False


@pytest.mark.parametrize("kw", [dict(leaves_per_step=2), dict(board_semantics="aliased"), dict(reference_quirks=True), dict(rng="numpy"),
                                dict(forced_playouts=2.0), dict(tree_reuse=True), dict(solver=True)], ids=lambda k: next(iter(k)))
def test_it_is_refused_wherever_gumbel_root_is(kw):
    with pytest.raises(options.OptionConflict) as e:
        options.resolve(num_simulations=16, gumbel_root=4, gumbel_interior=True, **kw)
    assert e.value.option == "gumbel_root" and next(iter(kw)) in e.value.conflicts


def test_both_views_carry_it_only_when_on_and_resolve_back_to_the_record():
    off = options.resolve(num_simulations=16, gumbel_root=4)
    assert off.gumbel_interior is False and "gumbel_interior" not in off.keywords() and "gumbel_interior" not in off.tree_keywords()
    assert options.resolve(16, gumbel_root=4, gumbel_interior=None) == options.resolve(16, gumbel_root=4, gumbel_interior=False) == off
    on = options.resolve(num_simulations=16, gumbel_root=4, gumbel_interior=True, fast_simulations=4, full_search_probability=0.5,
                         free_running=True, evaluation_symmetry="random", shared_evaluations=64, shared_evaluations_replace=True)
    assert on.gumbel_interior is True and on.keywords()["gumbel_interior"] is True and on.tree_keywords()["gumbel_interior"] is True
    assert options.resolve(16, **on.keywords()) == on
    assert set(on.tree_keywords()) <= set(inspect.signature(engine.BatchedMCTS).parameters)
    assert "gumbel_interior" not in [r[0] for r in options.RULES]                    # a sub-option, not an option name of the table


# (the SelfPlayEngine factory hands its keywords to _Engine.__init__: test_the_constructors_reach_the_resolver covers it)
TAKERS = [engine.BatchedMCTS, mcts.MCTS, self_play._Engine.__init__, self_play.SelfPlayLanes, self_play.SelfPlayWorker,
          self_play.SelfPlayManager, arena.AlphaZero]


@pytest.mark.parametrize("taker", TAKERS, ids=lambda t: getattr(t, "__qualname__", str(t)))
def test_everything_that_takes_gumbel_root_takes_it(taker):
    params = inspect.signature(taker).parameters
    assert "gumbel_root" in params and params["gumbel_interior"].default is False


def test_the_constructors_reach_the_resolver(tmp_path):
    """each refuses the sub-option without gumbel_root on the host, before anything touches a device, and names gumbel_root"""
    game = Game()
    calls = [lambda: mcts.MCTS(game, None, board_semantics="copied", gumbel_interior=True),
             lambda: self_play.SelfPlayEngine(game, None, num_simulations=8, gumbel_interior=True),
             lambda: self_play.SelfPlayEngine(game, None, num_simulations=8, free_running=True, gumbel_interior=True),
             lambda: self_play.SelfPlayLanes(game, None, lanes=2, num_simulations=8, gumbel_interior=True),
             lambda: self_play.SelfPlayWorker(game, None, num_simulations=8, board_semantics="copied", reference_quirks=False,
                                              neural_net=object(), gumbel_interior=True),
             lambda: self_play.SelfPlayManager(game, "no-such-model", num_simulations=8, gumbel_interior=True),
             lambda: self_play.generate_self_play_data(game, "no-such-model", str(tmp_path / "data"), num_simulations=8,
                                                       gumbel_interior=True),
             lambda: arena.AlphaZero(game, "no-such-dir", "no-such-dir", num_simulations=8, gumbel_interior=True),
             lambda: engine.gumbel_m(None, None, None, True)]
    for call in calls:
        with pytest.raises(options.OptionConflict) as e:
            call()
        assert e.value.option == "gumbel_root"
    m = mcts.MCTS(game, None, board_semantics="copied", gumbel_root=4, gumbel_interior=True)
    assert m.options.gumbel_interior is True and m.options.tree_keywords()["gumbel_interior"] is True
    with pytest.raises(options.OptionConflict) as e:
        mcts.MCTS(game, None, board_semantics="copied", gumbel_root=4, gumbel_interior=True, fpu_reduction=0.2)
    assert (e.value.option, e.value.conflicts) == ("gumbel_root", ("fpu_reduction",))


def test_the_command_line_flag_resolves():
    import train_alphazero as T
    for mode in ("self-play", "train"):
        a = T.parse_args(["--mode", mode, "--gumbel-root", "16", "--gumbel-interior"])
        assert a.gumbel_interior is True and T.refused(a) is None
        assert T.parse_args(["--mode", mode, "--gumbel-root", "16"]).gumbel_interior is False
        msg = T.refused(T.parse_args(["--mode", mode, "--gumbel-interior"]))
        assert msg and "gumbel_interior" in msg
        msg = T.refused(T.parse_args(["--mode", mode, "--gumbel-root", "16", "--gumbel-interior", "--fpu-reduction", "0.2"]))
        assert msg and "--gumbel-root 16" in msg and "--fpu-reduction 0.2" in msg
    assert "gumbel_interior" not in sum(T.HANDED["evaluate"], ())
