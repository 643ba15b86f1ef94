"""The host rules of the replacing shared evaluation table (shared_evaluations_replace=: options.resolve, SearchOptions.keywords,
the command line, the keyword on every entry point) and the numpy restatement of its device rules (tests/shared_table_model.py:
claim, duplicate, hit mark, sweep, stamp wrap), pinned on hand-made sequences.  No device.

Reading of "two sweeps back to back": a sweep above the high-water mark uses the stamp the last such sweep recorded and then
records the current one, so the second of two sweeps without a launch between them has the current stamp for its cutoff and
evicts everything that is not of the current stamp (the GPU test "a full window comes back" relies on exactly that).  What it
leaves is a fixed point: further sweeps at the same stamp evict nothing new, and a sweep repeated with an unchanged cutoff and
stamp evicts nothing.  Both are pinned below."""
import inspect
import os
import sys

import pytest

from shared_table_model import M32, TOMBSTONE, Table, next_stamp, older

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


# ---- option resolution
def test_off_by_default_and_emitted_only_when_on(options):
    assert options.SearchOptions().shared_evaluations_replace is False
    for kw in (dict(), dict(shared_evaluations=4096), dict(shared_evaluations=4096, shared_evaluations_replace=False),
               dict(shared_evaluations=4096, shared_evaluations_replace=None)):
        o = options.resolve(64, **kw)
        assert o.shared_evaluations_replace is False and "shared_evaluations_replace" not in o.keywords()
    assert options.resolve(64, shared_evaluations=4096).keywords() == dict(leaves_per_step=1, shared_evaluations=4096)
    o = options.resolve(64, shared_evaluations=100, shared_evaluations_replace=True)
    assert o == options.SearchOptions(shared_evaluations=128, shared_evaluations_replace=True)
    assert o.keywords() == dict(leaves_per_step=1, shared_evaluations=128, shared_evaluations_replace=True)
    assert options.resolve(64, **o.keywords()) == o                          # the next layer resolves to the same options
    o = options.resolve(64, shared_evaluations=True, shared_evaluations_replace=True, free_running=True, fast_simulations=8,
                        full_search_probability=0.5, evaluation_symmetry="random", forced_playouts=2.0, fpu_reduction=0.2)
    assert o.shared_evaluations == 1 << 23 and o.shared_evaluations_replace and options.resolve(64, **o.keywords()) == o
    assert 0.0 < options.SHARED_EVALUATIONS_HIGH_WATER < 1.0


@pytest.mark.parametrize("off", [dict(), dict(shared_evaluations=None), dict(shared_evaluations=False)])
def test_refused_without_the_table(options, off):
    with pytest.raises(options.OptionConflict) as e:
        options.resolve(64, shared_evaluations_replace=True, **off)
    assert e.value.option == "shared_evaluations_replace" and e.value.conflicts == ("shared_evaluations",)
    with pytest.raises(options.OptionConflict) as e:
        options.resolve(64, shared_evaluations=64, shared_evaluations_replace="yes")
    assert e.value.option == "shared_evaluations_replace" and e.value.conflicts == ()


@pytest.mark.parametrize("kw,conflicts", [(dict(board_semantics="aliased"), ("board_semantics",)),
                                          (dict(leaves_per_step=4), ("leaves_per_step",)),
                                          (dict(reference_quirks=True), ("reference_quirks",))])
def test_it_inherits_the_refusals_of_the_table(options, kw, conflicts):
    with pytest.raises(options.OptionConflict) as e:
        options.resolve(64, shared_evaluations=True, shared_evaluations_replace=True, **kw)
    with pytest.raises(options.OptionConflict) as plain:
        options.resolve(64, shared_evaluations=True, **kw)
    assert e.value.option == "shared_evaluations" and e.value.conflicts == conflicts and str(e.value) == str(plain.value)


def test_every_entry_point_has_the_keyword():
    import yinyang_game_alphazero_amd as pkg
    sp = pkg.self_play
    for f in (pkg.MCTS, sp._Engine.__init__, pkg.SelfPlayLanes, pkg.SelfPlayWorker, pkg.SelfPlayManager, pkg.AlphaZero,
              pkg.options.resolve):
        assert inspect.signature(f).parameters["shared_evaluations_replace"].default is False, f
    for f in (pkg.SelfPlayEngine, sp.LockstepEngine, sp.FreeRunningEngine, pkg.generate_self_play_data):
        assert any(x.kind is inspect.Parameter.VAR_KEYWORD for x in inspect.signature(f).parameters.values()), f
    p = inspect.signature(pkg.engine.SharedEvaluations).parameters
    assert p["replace"].default is False and "high_water" in p
    assert callable(pkg.engine.SharedEvaluations.sweep) and callable(pkg.engine.BatchedMCTS.shared_counters_ex)
    game = pkg.YinYangGame(4, 4)
    m = pkg.SelfPlayManager(game, "no-such-model", shared_evaluations=100, shared_evaluations_replace=True)
    assert m.options.shared_evaluations == 128 and m.options.shared_evaluations_replace
    assert pkg.MCTS(game, None, board_semantics="copied", shared_evaluations=100, shared_evaluations_replace=True).shared_evaluations_replace
    assert not pkg.MCTS(game, None, board_semantics="copied", shared_evaluations=100).shared_evaluations_replace
    for make in (lambda: pkg.SelfPlayManager(game, "no-such-model", shared_evaluations_replace=True),
                 lambda: pkg.MCTS(game, None, board_semantics="copied", shared_evaluations_replace=True),
                 lambda: pkg.SelfPlayWorker(game, "no-such-model", neural_net=object(), board_semantics="copied", reference_quirks=False,
                                            shared_evaluations_replace=True),
                 lambda: pkg.AlphaZero(game, "m", "d", shared_evaluations_replace=True)):
        with pytest.raises(pkg.options.OptionConflict) as e:
            make()
        assert e.value.option == "shared_evaluations_replace"


def test_the_table_object_on_the_host():
    """Layout and refusals of engine.SharedEvaluations that need no device (CPU tensors stand in)."""
    import torch
    import yinyang_game_alphazero_amd as pkg
    cpu = torch.device("cpu")
    plain = pkg.engine.SharedEvaluations(4, 4, 100, device=cpu)
    t = pkg.engine.SharedEvaluations(4, 4, 100, device=cpu, replace=True)
    assert not plain.replace and plain.meta is not None and plain.memory_bytes == 128 * (4 + 16 + 4 + 64) + 4
    assert t.replace and t.slots == 128 and t.high_water == pkg.options.SHARED_EVALUATIONS_HIGH_WATER
    assert t.claim.dtype == torch.int64 and t.last_hit.dtype == torch.int32 and t.claim.shape == t.last_hit.shape == (128,)
    assert t.memory_bytes == 128 * (8 + 4 + 16 + 4 + 64) + 8 * 8 + 4
    assert t.fill() == 0 and t.counters() == dict(hits=0, inserts=0, dropped=0, duplicates=0, evicted=0, live=0)
    assert plain.counters() == dict(hits=0, inserts=0, dropped=0)
    t.claim[3] = (7 << 32) | 5
    t.claim[4] = TOMBSTONE
    assert t.fill() == 1 and t.live().nonzero().flatten().tolist() == [3] and int(t.stamps()[3]) == 5
    t.clear()
    assert t.fill() == 0
    with pytest.raises(RuntimeError, match="replace=True"):
        plain.sweep()
    t.sweep()                                          # no context has written to it: nothing to do, no device call
    assert pkg.engine.SharedEvaluations(4, 4, 64, device=cpu, replace=True, high_water=0).high_water == 0.0
    with pytest.raises(ValueError, match="high_water"):
        pkg.engine.SharedEvaluations(4, 4, 64, device=cpu, replace=True, high_water=1.5)


@pytest.mark.parametrize("mode", ["self-play", "train"])
def test_the_command_line(cli, mode):
    a = cli.parse_args(["--mode", mode])
    assert a.shared_evaluations_replace is False and cli.refused(a) is None
    a = cli.parse_args(["--mode", mode, "--shared-evaluations", "4096", "--shared-evaluations-replace", "--free-running"])
    assert a.shared_evaluations_replace is True and cli.refused(a) is None
    assert any("shared_evaluations_replace" in names for names in cli.HANDED[mode])
    msg = cli.refused(cli.parse_args(["--mode", mode, "--shared-evaluations-replace"]))
    assert msg and msg.startswith("train_alphazero.py: --shared-evaluations-replace: not with --shared-evaluations None")
    msg = cli.refused(cli.parse_args(["--mode", mode, "--shared-evaluations", "--shared-evaluations-replace", "--leaves-per-step", "4"]))
    assert msg and msg.startswith("train_alphazero.py: --shared-evaluations: not with --leaves-per-step 4")


def test_the_flag_reaches_the_manager(cli, monkeypatch, tmp_path):
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
        cli.main(["--mode", "self-play", "--rows", "4", "--cols", "4", "--model-dir", str(tmp_path), "--data-dir", str(tmp_path / "d"),
                  "--shared-evaluations", "1000", "--shared-evaluations-replace"])
    assert seen["manager"].options.keywords() == dict(leaves_per_step=1, shared_evaluations=1024, shared_evaluations_replace=True)


# ---- the model: stamps
def test_stamps_skip_zero_and_the_tombstone():
    assert next_stamp(1) == 2 and next_stamp(M32 - 2) == M32 - 1
    assert next_stamp(M32 - 1) == 1                    # TOMBSTONE and 0 are both skipped
    assert next_stamp(TOMBSTONE) == 1 and next_stamp(0) == 1
    s, seen = M32 - 4, []
    for _ in range(8):
        s = next_stamp(s)
        seen.append(s)
    assert seen == [M32 - 3, M32 - 2, M32 - 1, 1, 2, 3, 4, 5] and 0 not in seen and TOMBSTONE not in seen


def test_older_survives_the_wrap():
    """Ages, not values: across the wrap a stamp handed out earlier is still the older one."""
    now = 3                                            # handed out after M32 - 1, 1, 2
    assert older(M32 - 5, M32 - 2, now) and not older(M32 - 2, M32 - 5, now)
    assert older(M32 - 2, 1, now) and not older(1, M32 - 2, now)       # M32 - 2 < 1 in launch order, > in value
    assert older(1, 2, now) and not older(2, 2, now) and not older(3, 2, now)
    assert not older(now, now, now) and not older(now, M32 - 2, now)


# ---- the model: claim, duplicate, hit mark
def pos(key, slot=0, tag=1):
    return key, (tag << 32) | slot


def test_one_inserter_per_position_and_launch():
    t = Table(64)
    t.begin_launch()
    assert [t.insert(*pos("a")) for _ in range(3)] == ["inserted", "duplicate", "duplicate"]
    assert t.insert(*pos("b", tag=2)) == "inserted"                       # same window, another tag: the next slot
    assert t.insert(*pos("c", tag=1)) == "duplicate"                      # a false tag match loses one insert, nothing else
    assert t.live_slots() == [0, 1] and t.c == dict(hits=0, inserts=2, dropped=0, duplicates=3, evicted=0, live=0)
    assert t.lookup(*pos("a")) is None                                    # an entry of the launch in flight is passed over
    t.begin_launch()
    assert t.lookup(*pos("a")) == 0 and t.lookup(*pos("b", tag=2)) == 1 and t.lookup(*pos("c")) is None      # keys compared in full
    assert t.insert(*pos("a")) == "inserted" and t.live_slots() == [0, 1, 2]     # another launch: no duplicate across launches
    assert t.last_hit[0] == t.stamp and t.last_hit[2] == t.stamp


def test_a_full_window_drops_and_a_tombstone_is_free_but_not_the_end_of_the_chain():
    t = Table(64)
    t.begin_launch()
    for i in range(8):
        assert t.insert(*pos(i, tag=10 + i)) == "inserted"
    assert t.insert(*pos(8, tag=18)) == "dropped" and t.c["dropped"] == 1
    t.begin_launch()
    t.claim[2] = TOMBSTONE
    assert t.lookup(*pos(5, tag=15)) == 5                                 # behind the tombstone
    assert t.insert(*pos(8, tag=18)) == "inserted" and t.key[2] == 8 and t.stamp_of(2) == t.stamp


# ---- the model: sweep
def filled():
    """Entries a, b inserted at launch 2; a is served at launch 4."""
    t = Table(64)
    t.begin_launch()                                   # 2
    t.insert(*pos("a", tag=1))
    t.insert(*pos("b", tag=2))
    return t


def test_an_entry_hit_in_the_interval_survives_and_an_unused_one_goes_at_the_second_sweep():
    t = filled()
    assert t.sweep(0) == [] and t.cutoff == 2 and t.c["live"] == 2        # the first sweep above the mark only records
    t.begin_launch()                                   # 3
    t.begin_launch()                                   # 4
    assert t.lookup(*pos("a", tag=1)) == 0
    t.insert(*pos("c", tag=3))
    assert t.sweep(0) == [] and t.cutoff == 4          # a, b carry the cutoff's stamp: not older
    t.begin_launch()                                   # 5
    assert t.sweep(0) == [1]                           # b: inserted before the cutoff, never served since; a was, c is newer
    assert t.stamp_of(1) == TOMBSTONE and t.live_slots() == [0, 2]
    assert t.c["evicted"] == 1 and t.c["live"] == 2 and t.cutoff == 5


def test_an_entry_with_the_current_stamp_is_never_evicted():
    t = filled()
    t.sweep(0)
    for _ in range(3):
        t.begin_launch()
    t.insert(*pos("new", tag=9))                       # inserted in the latest launch
    assert t.lookup(*pos("a", tag=1)) == 0             # served in the latest launch: what a pending leaf looks like
    for _ in range(4):                                 # however often the sweep runs before the next launch
        gone = t.sweep(0)
        assert 0 not in gone and 2 not in gone
    assert t.live_slots() == [0, 2] and t.c["evicted"] == 1


def test_two_sweeps_back_to_back_evict_nothing_new():
    t = filled()
    t.sweep(0)
    t.begin_launch()
    t.begin_launch()
    t.lookup(*pos("a", tag=1))
    first = t.sweep(0)                                 # cutoff 2: nothing is older
    second = t.sweep(0)                                # cutoff = the current stamp: everything not of this launch goes
    assert first == [] and second == [1]
    for _ in range(3):                                 # the fixed point: same cutoff, same stamp, nothing new
        assert t.sweep(0) == []
    assert t.c["evicted"] == 1 and t.live_slots() == [0]
    u = filled()                                       # and under the mark a sweep neither evicts nor records
    assert u.sweep(2) == [] and u.cutoff == 0 and u.sweep(2) == [] and u.c["live"] == 2


def test_the_sweep_survives_the_wrap():
    t = Table(64, stamp=M32 - 3)
    t.begin_launch()                                   # M32 - 2
    t.insert(*pos("a", tag=1))
    t.insert(*pos("b", tag=2))
    t.sweep(0)
    t.begin_launch()                                   # M32 - 1
    t.sweep(0)                                         # cutoff M32 - 1 from here on
    t.begin_launch()                                   # 1: wrapped
    assert t.stamp == 1 and t.lookup(*pos("a", tag=1)) == 0
    t.insert(*pos("c", tag=3))
    assert t.sweep(0) == [1]                           # b is older than the cutoff although its stamp is the larger number
    assert t.live_slots() == [0, 2] and t.cutoff == 1
