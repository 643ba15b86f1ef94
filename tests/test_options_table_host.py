"""The two tables of options.py (no GPU): RULES is asked in its own, documented order -- of two broken rules the earlier one is
named, by `resolve` and by MCTS(...), which asks it once with everything it has --, and both views of a record, keywords() and
tree_keywords(), read HANDED_ON and fit the signatures they are handed to."""
import inspect

import pytest

from yinyang_game_alphazero_amd import engine, mcts, options, self_play

ORDER = ["evaluation_symmetry", "forced_playouts", "gumbel_root", "free_running", "tree_reuse", "leaves_per_step", "fpu_reduction",
         "shared_evaluations", "shared_evaluations_replace", "solver"]       # the playout cap: between tree_reuse and leaves_per_step
CAP = dict(fast_simulations=16, full_search_probability=0.25)
# every option that goes with every other one, and all of them without tree_reuse / solver / forced_playouts but with gumbel_root
ALL_ON = dict(leaves_per_step=1, tree_reuse=True, evaluation_symmetry="random", symmetry_seed=5, forced_playouts=2.0, fpu_reduction=0.2,
              fpu_reduction_root=0.0, shared_evaluations=100, shared_evaluations_replace=True, solver=True)
ALL_ON_GUMBEL = dict({k: v for k, v in ALL_ON.items() if k not in ("tree_reuse", "forced_playouts", "solver")}, gumbel_root=4,
                     gumbel_c_scale=0.5)


class Game:
    def getBoardSize(self):
        return 4, 5

    def getActionSize(self):
        return 20


def test_the_table_is_in_the_documented_order():
    named = [r[0] for r in options.RULES]
    assert [n for i, n in enumerate(named) if n not in named[:i]] == ORDER
    assert named == sorted(named, key=ORDER.index)                      # an option's rules stand together
    for option, others, why in options.RULES:
        assert others and option not in others and why.endswith(("-- not with", "-- not without"))


@pytest.mark.parametrize("earlier, conflicts, kw", [
    ("evaluation_symmetry", ("reference_quirks",), dict(evaluation_symmetry="random", forced_playouts=2, reference_quirks=True)),
    ("forced_playouts", ("reference_quirks",), dict(forced_playouts=2, gumbel_root=4, reference_quirks=True)),
    ("gumbel_root", ("reference_quirks",), dict(gumbel_root=4, free_running=True, reference_quirks=True)),
    ("free_running", ("leaves_per_step", "tree_reuse"), dict(free_running=True, tree_reuse=True, leaves_per_step=4)),
    ("tree_reuse", ("leaves_per_step",), dict(tree_reuse=True, leaves_per_step=4, board_semantics="aliased")),
    ("tree_reuse", ("board_semantics",), dict(tree_reuse=True, board_semantics="aliased", fast_simulations=0)),
    ("fast_simulations", (), dict(fast_simulations=0, leaves_per_step=4, board_semantics="aliased")),
    ("leaves_per_step", ("reference_quirks",), dict(leaves_per_step=4, reference_quirks=True, fpu_reduction=0.2)),
    ("fpu_reduction", ("reference_quirks",), dict(fpu_reduction=0.2, shared_evaluations=64, reference_quirks=True)),
    ("shared_evaluations", ("reference_quirks",), dict(shared_evaluations=64, shared_evaluations_replace="yes", reference_quirks=True)),
    ("shared_evaluations_replace", ("shared_evaluations",), dict(shared_evaluations_replace=True, solver=True, reference_quirks=True)),
], ids=lambda x: x if isinstance(x, str) else None)
def test_of_two_adjacent_broken_rules_the_earlier_one_is_named(earlier, conflicts, kw):
    with pytest.raises(options.OptionConflict) as e:
        options.resolve(64, **kw)
    assert (e.value.option, e.value.conflicts) == (earlier, conflicts)


def test_tree_keywords_is_the_part_of_keywords_a_tree_context_takes():
    assert options.resolve(64).tree_keywords() == dict(leaves_per_step=1) == options.SearchOptions().tree_keywords(seed=7)
    context = inspect.signature(engine.BatchedMCTS).parameters
    for given in (ALL_ON, ALL_ON_GUMBEL):
        o = options.resolve(64, free_running="gumbel_root" in given, **CAP, **given)
        kw, tree = o.keywords(), o.tree_keywords()
        assert set(tree) <= set(kw) and set(tree) <= set(context) and all(tree[k] == kw[k] for k in tree)
        assert set(kw) - set(tree) == {"fast_simulations", "full_search_probability", "shared_evaluations", "shared_evaluations_replace",
                                       "free_running" if o.free_running else "tree_reuse"}
        assert options.resolve(64, **kw) == o
    assert {f for _, fields, _ in options.HANDED_ON for f in fields} | {"leaves_per_step"} == set(options.SearchOptions.__dataclass_fields__)


def test_tree_keywords_fills_the_seed_only_where_none_was_given():
    assert options.resolve(evaluation_symmetry="random").tree_keywords(seed=7)["symmetry_seed"] == 7
    assert options.resolve(evaluation_symmetry="random").tree_keywords()["symmetry_seed"] is None
    assert options.resolve(evaluation_symmetry="random", symmetry_seed=3).tree_keywords(seed=7)["symmetry_seed"] == 3
    assert "symmetry_seed" not in options.resolve(symmetry_seed=3).tree_keywords(seed=7)


def test_every_handed_keyword_is_a_parameter_of_the_layer_that_takes_it():
    for given in (ALL_ON, ALL_ON_GUMBEL):
        o = options.resolve(64, free_running="gumbel_root" in given, **CAP, **given)
        # the mode is the SelfPlayEngine factory's keyword: it picks the class, whose constructor takes all the others
        assert set(o.keywords()) - {"free_running"} <= set(inspect.signature(self_play._Engine.__init__).parameters)
        assert "free_running" in inspect.signature(self_play.SelfPlayEngine).parameters
        assert set(o.keywords()) - set(o.playout_cap) - {"free_running"} <= set(inspect.signature(mcts.MCTS).parameters)


@pytest.mark.parametrize("given", [ALL_ON, ALL_ON_GUMBEL], ids=["all", "gumbel"])
def test_mcts_keeps_the_record_of_its_one_resolve(given):
    m = mcts.MCTS(Game(), None, board_semantics="copied", **given)
    assert m.options == options.resolve(**given)
    assert m.gumbel == (m.options.gumbel_root, m.options.gumbel_c_visit, m.options.gumbel_c_scale)
    assert (m.leaves_per_step, m.tree_reuse, m.solver, m.shared_evaluations) == (1, m.options.tree_reuse, m.options.solver, 128)
    assert m.symmetry == ("random", 5) and (m.fpu_reduction, m.fpu_reduction_root) == (0.2, 0.0)


@pytest.mark.parametrize("option, conflicts, kw", [
    ("evaluation_symmetry", ("board_semantics",), dict(evaluation_symmetry="random", tree_reuse=True)),       # aliased: MCTS's default
    ("gumbel_root", ("leaves_per_step", "solver"), dict(board_semantics="copied", gumbel_root=4, solver=True, leaves_per_step=4,
                                                        shared_evaluations=64)),
    ("leaves_per_step", ("board_semantics",), dict(leaves_per_step=4)),
    ("leaves_per_step", ("evaluation_reuse",), dict(leaves_per_step=4, board_semantics="copied", evaluation_reuse=True)),
], ids=["symmetry+reuse", "gumbel+shared", "K aliased", "K reuse"])
def test_mcts_names_the_option_the_resolver_names(option, conflicts, kw):
    with pytest.raises(options.OptionConflict) as e:
        mcts.MCTS(Game(), None, **kw)
    assert (e.value.option, e.value.conflicts) == (option, conflicts)
    resolver = dict(kw, evaluation_reuse=(kw.get("evaluation_reuse", False),), board_semantics=kw.get("board_semantics", "aliased"))
    with pytest.raises(options.OptionConflict) as r:
        options.resolve(**resolver)
    assert str(r.value) == str(e.value)
