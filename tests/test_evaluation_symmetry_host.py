"""Symmetry-randomised evaluation on the host (no GPU): the resolver's rules for the option, and the numpy model the GPU tests
use as their reference checked against itself."""
import numpy as np
import pytest

import symmetry_model as sm
from yinyang_game_alphazero_amd import options


@pytest.mark.parametrize("kw,conflict", [(dict(board_semantics="aliased"), "board_semantics"),
                                         (dict(reference_quirks=True), "reference_quirks"), (dict(rng="numpy"), "rng")])
def test_resolver_refuses_the_parity_options(kw, conflict):
    with pytest.raises(options.OptionConflict, match="evaluation_symmetry") as e:
        options.resolve(16, evaluation_symmetry="random", **kw)
    assert e.value.option == "evaluation_symmetry" and e.value.conflicts == (conflict,)
    assert conflict in str(e.value)
    options.resolve(16, **kw)                                           # without the option the combination stands


def test_resolver_refuses_an_unknown_mode():
    with pytest.raises(options.OptionConflict, match="evaluation_symmetry") as e:
        options.resolve(16, evaluation_symmetry="always")
    assert e.value.option == "evaluation_symmetry" and e.value.conflicts == ()


def test_keywords_omit_the_option_when_it_is_off():
    assert options.resolve().keywords() == dict(leaves_per_step=1)
    assert options.resolve(evaluation_symmetry="off", symmetry_seed=5).keywords() == dict(leaves_per_step=1)
    on = options.resolve(16, evaluation_symmetry="random", symmetry_seed=5)
    assert on.keywords() == dict(leaves_per_step=1, evaluation_symmetry="random", symmetry_seed=5)
    assert options.resolve(16, evaluation_symmetry="random").keywords()["symmetry_seed"] is None       # the engine's seed


def test_it_combines_with_every_other_option():
    for kw in (dict(leaves_per_step=4), dict(fast_simulations=4, full_search_probability=0.5), dict(tree_reuse=True),
               dict(free_running=True), dict(evaluation_reuse=(True, True, True)), dict(opening_book=2)):
        assert options.resolve(16, evaluation_symmetry="random", **kw).evaluation_symmetry == "random"


def test_cli_hands_the_flag_to_the_resolver():
    import train_alphazero as cli
    base = ["--simulations", "16", "--evaluation-symmetry", "random"]
    for mode in ("self-play", "train"):
        assert cli.refused(cli.parse_args(["--mode", mode] + base + ["--symmetry-seed", "3"])) is None
    msg = cli.refused(cli.parse_args(["--mode", "self-play", "--board-semantics", "aliased"] + base))
    assert msg.startswith("train_alphazero.py: --evaluation-symmetry random") and "--board-semantics aliased" in msg
    msg = cli.refused(cli.parse_args(["--mode", "self-play", "--reference-quirks"] + base))
    assert msg.startswith("train_alphazero.py: --evaluation-symmetry random") and "--reference-quirks" in msg


@pytest.mark.parametrize("shape", [(4, 4), (5, 7)])
def test_model_transform_then_inverse_is_the_identity(shape):
    R, C = shape
    rng = np.random.RandomState(3)
    board = rng.randint(-1, 2, size=shape).astype(np.int8)
    cells = np.arange(R * C).reshape(R, C)
    seen = set()
    for s in range(sm.group_size(R, C)):
        t = sm.transform(board, s)
        assert t.shape == board.shape
        assert np.array_equal(sm.inverse(t, s), board) and np.array_equal(sm.transform(sm.inverse(board, s), s), board)
        # the cell map is the same permutation: a stone on cell a of the board sits on cell T_s(a) of the transformed board
        m = sm.cell_map(R, C, s)
        assert sorted(m) == list(range(R * C))
        assert np.array_equal(t.reshape(-1)[m], board.reshape(-1))
        seen.add(sm.transform(cells, s).tobytes())
    assert len(seen) == sm.group_size(R, C)                             # the group's elements are distinct maps


@pytest.mark.parametrize("shape", sm.DRAW_SHAPES)
def test_model_draw_spreads_over_the_group(shape):
    """The positions and the seed the GPU draw test uses: every group element occurs among the 512 draws, none takes more than
    a quarter (square boards) or a half of them -- with the numpy model alone."""
    boards = sm.positions(shape)
    assert boards.shape == (512,) + shape and len(np.unique(boards, axis=0)) == 512
    n = sm.group_size(*shape)
    counts = np.bincount(sm.draw(boards, sm.DRAW_SEED), minlength=n)
    assert len(counts) == n and counts.min() > 0 and counts.max() <= 512 // (4 if n == 8 else 2), counts


def test_model_draw_is_a_function_of_seed_and_position_only():
    rng = np.random.RandomState(5)
    boards = rng.randint(-1, 2, size=(64, 9, 12)).astype(np.int8)
    s = sm.draw(boards, 7)
    order = rng.permutation(64)
    assert np.array_equal(sm.draw(boards[order], 7), s[order])          # not of the batch or the row
    assert np.array_equal(sm.draw(boards[:5], 7), s[:5])
    assert not np.array_equal(sm.draw(boards, 8), s)
    assert s.min() >= 0 and s.max() <= 3
    last = boards.copy()
    last[:, 8, 11] = np.where(last[:, 8, 11] == 1, -1, 1)               # the last cell sits in the second word
    assert not np.array_equal(sm.draw(last, 7), s)
