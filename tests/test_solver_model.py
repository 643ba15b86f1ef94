"""The MCTS solver: the numpy model (tests/solver_model.py) against the model it is built on with the option off, the exhaustive
minimax of the real rules (soundness), what its fixtures show, its mutants, and the host side of the option (options.resolve,
keywords(), the command line).  The fixtures are the ones the GPU tests (tests/test_gpu_solver.py) run.

The minimax is written on the C oracle's rules (oracle_lib: game_ended, valid_mask), the CPU statement of the game every model
here uses: the package's YinYangGame asks the rules kernels and so needs a device, which a CPU test does not have."""
import functools
import os
import sys

import numpy as np
import pytest

import fpu_model as F
import oracle_lib as O
import solver_model as S

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ARENA_ROOT = (3, 3, 6, 400)                                        # rows, cols, plies, seed of the arena-rule position


def same(a, w):
    assert np.array_equal(a.counts, w.counts)
    assert np.array_equal(a.child_w.view(np.uint32), np.asarray(w.child_w, np.float32).view(np.uint32))
    assert np.array_equal(a.child_p.view(np.uint32), w.child_p.view(np.uint32))
    assert a.root_visits == w.root_visits and a.root_w == w.root_w and a.evals == w.evals


@pytest.mark.parametrize("R,C,plies,sims", [(3, 3, 4, 64), (4, 4, 7, 48), (1, 6, 2, 16), (7, 1, 3, 16), (5, 7, 20, 32), (9, 12, 3, 16)])
@pytest.mark.parametrize("kw", [dict(), dict(r=0.2), dict(forced=2.0), dict(r=0.25, r_root=0.0, forced=2.0)], ids=str)
def test_option_off_is_the_fpu_model(R, C, plies, sims, kw):
    """Fresh roots and three moves on kept roots, with root noise: fpu_model.search observable for observable."""
    for seed in range(3):
        board, player = F.random_root(R, C, plies, seed)
        noise = F.dirichlet_noise(board, player, 50 + seed) if seed else None
        a, w = S.search(board, player, sims, solver=False, noise=noise, **kw), F.search(board, player, sims, noise=noise, **kw)
        same(a, w)
        assert a.root_proven == 0 and not a.child_proven.any() and (a.proven_nodes, a.proven_descents, a.proven_roots) == (0, 0, 0)
        for _ in range(2):
            act = int(np.argmax(w.counts))
            ta, ka = S.advance_proven(a.tree, act)
            tw, kw_ = F.advance(w.tree, act)
            assert ka == kw_ and (ta is None) == (tw is None)
            if ta is None or ka >= sims:
                break
            p = ta.root.player
            a, w = S.search(ta, p, sims, solver=False, noise=noise, **kw), F.search(tw, p, sims, noise=noise, **kw)
            same(a, w)


# ------------------------------------------------------------------------------------------------ soundness
@functools.lru_cache(maxsize=None)
def minimax(key, rows, cols, player):
    """The value of the position for `player` to move under the real rules -- a side without a move passes -- as 1, 0 (draw)
    or -1, by exhaustive search."""
    board = np.frombuffer(key, np.int8).reshape(1, rows, cols)
    ended = float(O.game_ended(board, [player])[0])
    if ended != 0.0:
        return 0 if ended == 0.0001 else int(ended)
    moves = np.flatnonzero(O.valid_mask(board, [player])[0])
    if not len(moves):
        return -minimax(key, rows, cols, -player)                  # a pass
    best = -1
    for a in moves:
        b = board.copy()
        b.flat[a] = player
        best = max(best, -minimax(b.tobytes(), rows, cols, -player))
        if best == 1:
            break
    return best


WANT = {S.WIN: 1, S.LOSS: -1, S.DRAW: 0}


@pytest.mark.parametrize("rows,cols,sims", [(3, 3, 400), (2, 2, 64), (2, 4, 200)])
def test_every_proven_status_is_the_minimax_value(rows, cols, sims):
    roots = checked = 0
    for seed in range(6):
        for plies in range(0, rows * cols - 1, 2):
            board, player = F.random_root(rows, cols, plies, [seed, plies])
            for kw in (dict(), dict(r=0.2)):
                res = S.search(board, player, sims, **kw)
                for node, st in res.tree.proven.values():
                    assert node.edges and not node.terminal
                    assert WANT[st] == minimax(node.board.tobytes(), rows, cols, node.player), (seed, plies, st)
                    checked += 1
                if res.root_proven and not res.tree.root.terminal:
                    assert WANT[res.root_proven] == minimax(board.tobytes(), rows, cols, player)
                    roots += 1
    assert roots > 0 and checked > roots


def test_the_fixtures_are_sound_too():
    for name, case in S.CASES.items():
        if case[0] * case[1] > 16:
            continue
        for m in S.fixture(name):
            for r in m.results:
                for node, st in (r.tree.proven.values() if r is not None else ()):
                    assert WANT[st] == minimax(node.board.tobytes(), case[0], case[1], node.player), name


# ------------------------------------------------------------------------------------------------ the machinery fires
def results(name=None):
    return [r for n in ([name] if name else S.CASES) for m in S.fixture(n) for r in m.results if r is not None]


def test_the_fixtures_show_the_machinery():
    assert sum(r.proven_nodes for r in results()) > 0
    assert sum(r.proven_descents for r in results()) > 0
    by_propagation = {s for r in results() for n, s, k in r.tree.log if n is r.tree.root}
    assert by_propagation == {S.WIN, S.LOSS, S.DRAW}               # roots proven WIN, LOSS and DRAW
    assert sum(r.proven_roots for r in results()) >= 3
    assert any(s == S.LOSS and k >= 2 for r in results() for _, s, k in r.tree.log)   # a LOSS that needed every child
    for name in S.CASES:                                           # every case is another search with the option than without
        assert S.observables(S.fixture(name)) != S.observables(S.fixture(name, None, False)), name
        assert all(not r.failed for r in results(name)), name
    for name in ("3x3", "9x12"):
        assert sum(r.proven_roots for r in results(name)) > 0, name
    assert max(len(r.tree.root.edges) for r in results("9x12")) >= 2
    assert sorted({r.root_visits for r in results("4x4-budgets")}) == [4, 16]
    assert sum(r.proven_descents for r in results("4x4-budgets")) > 0


def test_pass_nodes_are_never_proven():
    seen = 0
    for name in ("1x6", "7x1"):
        for r in results(name):
            assert all(node.edges for node, _ in r.tree.proven.values())

            def passes(node):
                return sum((not e.child.terminal and not e.child.edges) + passes(e.child) for e in node.edges if e.child is not None)
            seen += passes(r.tree.root) + (not r.tree.root.edges and not r.tree.root.terminal)
            if not r.tree.root.edges and not r.tree.root.terminal:
                assert r.root_proven == 0
    assert seen > 0


def test_kept_roots_carry_their_proofs():
    carried = searched_on = 0
    for name in ("4x4-reuse", "3x3-reuse"):
        fx = S.fixture(name)
        for t in range(1, len(fx)):
            for g, r in enumerate(fx[t].results):
                if r is None:
                    continue
                assert r.tree.kept
                prev = fx[t - 1].results[g]
                carried += r.ended.count(S.PROVEN) > 0 and r.proven_nodes == 0   # descents stopped at nodes proven a move earlier
                if prev.child_proven[fx[t].actions[g]]:              # the kept root was proven already: it is searched all the same
                    assert r.root_proven == prev.child_proven[fx[t].actions[g]]
                    assert r.root_visits == S.CASES[name][2] and len(r.ended) > 0 and r.proven_roots == 0
                    searched_on += 1
    assert carried > 0 and searched_on > 0


@pytest.mark.parametrize("mutant", sorted(S.MUTANTS))
def test_the_fixtures_tell_every_mutant_from_the_model(mutant):
    hit = [name for name in S.CASES if S.observables(S.fixture(name, mutant)) != S.observables(S.fixture(name))]
    assert hit, mutant


def test_the_arena_rule_has_its_position():
    """A 3x3 position whose search proves a winning root child that is not the most visited one."""
    rows, cols, plies, seed = ARENA_ROOT
    board, player = F.random_root(rows, cols, plies, seed)
    r = S.search(board, player, 64)
    w = S.winning_move(r)
    assert w >= 0 and w != int(np.argmax(r.counts)) and r.child_proven[w] == S.LOSS
    assert minimax(board.tobytes(), rows, cols, player) == 1
    assert S.winning_move(S.search(board, player, 64, solver=False)) == -1


# ------------------------------------------------------------------------------------------------ the host side of the option
def test_the_resolver_refuses_and_names_the_option():
    from yinyang_game_alphazero_amd import options
    assert options.resolve(800, solver=True).solver is True
    assert options.resolve(800).solver is False and options.resolve(800, solver=None).solver is False
    for kw, other in ((dict(leaves_per_step=4), "leaves_per_step"), (dict(board_semantics="aliased"), "board_semantics"),
                      (dict(reference_quirks=True), "reference_quirks"), (dict(rng="numpy"), "rng")):
        with pytest.raises(options.OptionConflict) as e:
            options.resolve(800, solver=True, **kw)
        assert e.value.option == "solver" and other in e.value.conflicts and "solver" in str(e.value), kw
        options.resolve(800, **{k: v for k, v in kw.items() if k not in ("leaves_per_step", "reference_quirks")})
    with pytest.raises(options.OptionConflict) as e:
        options.resolve(800, solver="yes")
    assert e.value.option == "solver"
    # it goes with everything else
    o = options.resolve(800, fast_simulations=100, full_search_probability=0.25, tree_reuse=True, evaluation_symmetry="random",
                        forced_playouts=2.0, fpu_reduction=0.2, shared_evaluations=1024, solver=True)
    assert o.solver and o.tree_reuse and o.forced_playouts == 2.0
    assert options.resolve(800, free_running=True, solver=True).free_running


def test_keywords_omit_the_default():
    from yinyang_game_alphazero_amd import options
    assert options.resolve(800).keywords() == dict(leaves_per_step=1)
    assert options.resolve(800, solver=False).keywords() == dict(leaves_per_step=1)
    assert options.resolve(800, solver=True).keywords() == dict(leaves_per_step=1, solver=True)
    assert options.resolve(800, solver=True, tree_reuse=True).keywords() == dict(leaves_per_step=1, tree_reuse=True, solver=True)


@pytest.mark.parametrize("mode", ["self-play", "train", "evaluate"])
def test_the_command_line_flag(mode):
    import train_alphazero as cli
    assert any("solver" in names for names in cli.HANDED[mode])
    args = cli.parse_args(["--mode", mode, "--solver"])
    assert args.solver is True and cli.refused(args) is None
    assert cli.parse_args(["--mode", mode]).solver is False and cli.refused(cli.parse_args(["--mode", mode])) is None
    msg = cli.refused(cli.parse_args(["--mode", mode, "--solver", "--leaves-per-step", "4"]))
    assert msg and "--solver" in msg and "--leaves-per-step 4" in msg
    if mode == "self-play":
        for extra, flag in ((["--board-semantics", "aliased"], "--board-semantics aliased"), (["--reference-quirks"], "--reference-quirks")):
            msg = cli.refused(cli.parse_args(["--mode", mode, "--solver"] + extra))
            assert msg and "--solver" in msg and flag in msg
