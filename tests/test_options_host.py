"""The options resolver is the one copy of the rules (no GPU): every constructor of the self-play layer and the command line
refuse exactly what options.resolve refuses for the inputs they hand it, name the same option, and do so before anything
touches the device."""
import itertools

import pytest

from test_selfplay_leaf_parallel_host import SIMS, Game, untouchable  # noqa: F401
from yinyang_game_alphazero_amd import arena, options, self_play

CAPS = {"off": {}, "valid": dict(fast_simulations=4, full_search_probability=0.25),
        "above": dict(fast_simulations=SIMS + 1, full_search_probability=0.5)}
MATRIX = list(itertools.product((1, 4), ("copied", "aliased"), (False, True), (False, True), (False, True), CAPS))

# entry point -> (the options it can express, its constructor from those).  Arena has no quirks, cap or mode and says
# board_semantics as `literal`; AlphaZero plays copied boards without the quirks; SelfPlayWorker always refuses free_running.
ENTRY = {
    "SelfPlayEngine": (None, lambda kw, tmp: self_play.SelfPlayEngine(Game(), None, num_simulations=SIMS, concurrent_games=4, **kw)),
    "SelfPlayLanes": (None, lambda kw, tmp: self_play.SelfPlayLanes(Game(), None, num_simulations=SIMS, concurrent_games=4, **kw)),
    "SelfPlayManager": (None, lambda kw, tmp: self_play.SelfPlayManager(Game(), "none.pth.tar", num_simulations=SIMS, **kw)),
    "SelfPlayWorker": (dict(free_running=False),
                       lambda kw, tmp: self_play.SelfPlayWorker(Game(), "none", num_simulations=SIMS, neural_net=object(),
                                                                **{k: v for k, v in kw.items() if k != "free_running"})),
    "AlphaZero": (dict(board_semantics="copied", reference_quirks=False),
                  lambda kw, tmp: arena.AlphaZero(Game(), str(tmp / "m"), str(tmp / "d"), num_simulations=SIMS, device="cpu",
                                                  **{k: v for k, v in kw.items() if k not in ("board_semantics", "reference_quirks")})),
    "Arena": (dict(reference_quirks=False, free_running=False, fast_simulations=None),
              lambda kw, tmp: arena.Arena(Game(), None, None, SIMS, literal=kw["board_semantics"] == "aliased",
                                          leaves_per_step=kw["leaves_per_step"], tree_reuse=kw["tree_reuse"])),
}


def verdict(make):
    """The OptionConflict a constructor raises, None when it goes on to the device (the `untouchable` stubs) or returns."""
    try:
        make()
    except options.OptionConflict as e:
        return e
    except AssertionError as e:
        assert "reached" in str(e), e
    return None


@pytest.mark.parametrize("entry", list(ENTRY))
def test_constructors_refuse_what_the_resolver_refuses(monkeypatch, untouchable, tmp_path, entry):
    monkeypatch.setattr(arena, "YinYangNeuralNetwork", self_play.YinYangNeuralNetwork)      # AlphaZero's first use of a network
    monkeypatch.setattr(arena.os, "makedirs", lambda *a, **k: untouchable.append("makedirs"))
    fixed, make = ENTRY[entry]
    seen = 0
    for K, semantics, quirks, tree, free, cap in MATRIX:
        kw = {**dict(leaves_per_step=K, board_semantics=semantics, reference_quirks=quirks, tree_reuse=tree, free_running=free,
                     fast_simulations=None), **CAPS[cap]}
        if fixed and any(kw[k] != v for k, v in fixed.items()):
            continue                                                   # this entry point cannot express the combination
        seen += 1
        want = verdict(lambda: options.resolve(num_simulations=SIMS, **kw))
        del untouchable[:]
        got = verdict(lambda: make(kw, tmp_path))
        assert (got is None) == (want is None), (entry, kw, got)
        if want is not None:
            assert (got.option, got.conflicts) == (want.option, want.conflicts) and str(got) == str(want), (entry, kw)
            assert untouchable == [], (entry, kw, untouchable)
    assert seen == {"SelfPlayWorker": 48, "AlphaZero": 24, "Arena": 8}.get(entry, 96)


def test_worker_refuses_free_running_whatever_else_is_given(untouchable):
    for K, semantics, quirks, tree, _, cap in MATRIX:
        with pytest.raises(ValueError, match="SelfPlayWorker"):
            self_play.SelfPlayWorker(Game(), "none", num_simulations=SIMS, neural_net=object(), leaves_per_step=K, board_semantics=semantics,
                                     reference_quirks=quirks, tree_reuse=tree, free_running=True, **CAPS[cap])
    assert untouchable == []


def test_keywords_omit_what_is_off():
    assert options.resolve().keywords() == dict(leaves_per_step=1)
    assert options.resolve(leaves_per_step=0, fast_simulations=4).keywords() == dict(leaves_per_step=1)
    on = options.resolve(SIMS, 1, free_running=True, **CAPS["valid"])
    assert on.keywords() == dict(leaves_per_step=1, free_running=True, **CAPS["valid"]) and on.playout_cap == CAPS["valid"]
    assert options.resolve(SIMS, 1, tree_reuse=True).keywords() == dict(leaves_per_step=1, tree_reuse=True)
    assert options.resolve(SIMS, 8).keywords() == dict(leaves_per_step=8)


# ---------------------------------------------------------------------------------------------------- command line
# what each mode looks at, stated here on its own: train's --tree-reuse and --free-running do not look at --board-semantics /
# --reference-quirks (its self-play is always copied, without quirks) although train's --leaves-per-step does; evaluate only
# checks --tree-reuse against --leaves-per-step
SEARCH = ("num_simulations", "leaves_per_step", "fast_simulations", "full_search_probability", "tree_reuse", "free_running")
MODE_HANDS = {"self-play": [SEARCH + ("board_semantics", "reference_quirks")],
              "train": [SEARCH, ("leaves_per_step", "board_semantics", "reference_quirks")],
              "evaluate": [("leaves_per_step", "tree_reuse")]}
FLAG = dict(num_simulations="--simulations", leaves_per_step="--leaves-per-step", fast_simulations="--fast-simulations",
            full_search_probability="--full-search-probability", tree_reuse="--tree-reuse", free_running="--free-running",
            board_semantics="--board-semantics", reference_quirks="--reference-quirks")


@pytest.mark.parametrize("mode", list(MODE_HANDS))
def test_cli_refuses_what_the_resolver_refuses(mode):
    import train_alphazero as cli
    refusals = 0
    for K, semantics, quirks, tree, free, cap in MATRIX:
        kw = {**dict(num_simulations=SIMS, leaves_per_step=K, board_semantics=semantics, reference_quirks=quirks, tree_reuse=tree,
                     free_running=free, fast_simulations=None, full_search_probability=1.0), **CAPS[cap]}
        argv = ["--mode", mode, "--simulations", str(SIMS), "--leaves-per-step", str(K), "--board-semantics", semantics]
        argv += [FLAG[k] for k in ("reference_quirks", "tree_reuse", "free_running") if kw[k]]
        argv += [x for k in CAPS[cap] for x in (FLAG[k], str(kw[k]))]
        want = next((e for e in (verdict(lambda: options.resolve(**{k: kw[k] for k in names})) for names in MODE_HANDS[mode])
                     if e is not None), None)
        msg = cli.refused(cli.parse_args(argv))
        assert (msg is None) == (want is None), (argv, msg)
        if want is not None:
            refusals += 1
            assert "\n" not in msg and msg.startswith("train_alphazero.py: " + FLAG[want.option]), (argv, msg)
            assert all(FLAG[c] in msg for c in want.conflicts), (argv, msg)
    assert 0 < refusals < len(MATRIX)
