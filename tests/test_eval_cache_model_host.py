"""tests/eval_cache_model.py on the host: against a reference that shares nothing with it (a Python set per epoch), on hand-built
probe windows, and on the leaf sequences of the CPU oracle for the configurations tests/test_gpu_eval_cache_trace.py runs on
the device -- where every rule must be exercised and every listed fault (MUTANTS) must change the predicted sequence."""
import numpy as np
import pytest

import eval_cache_cases as K
from eval_cache_model import (BOOK, HIT, MISS, MUTANTS, EvalCache, cache_bytes, cache_slots, first_slot, key_hashes, pack_keys,
                              replay)
from shared_table_model import PROBES, tt_first


def test_cache_slots_is_the_sizing_rule():
    assert cache_slots(3, 8, 64) == 64 and cache_slots(16, 8, 64) == 64 and cache_slots(17, 8, 64) == 128
    assert cache_slots(32, 128, 64) == 128 and cache_slots(102, 48, 64) == 512 and cache_slots(802, 4096, 64) == 4096
    # 48 GiB of policy rows: 16384 games of 802 nodes on 8 x 8 fit with 4096 slots each (16 GiB); 65536 games (64 GiB) are
    # halved once.  The halving goes on while the cache has MORE than twice the arena, so its last step may end below that:
    # 65536 games of 1602 nodes on 12 x 12 go 8192 -> 4096 -> 2048 < 3204, whatever the bytes
    assert cache_slots(802, 16384, 64) == 4096 and cache_slots(802, 65536, 64) == 2048
    assert cache_slots(1602, 65536, 144) == 2048 and cache_slots(1602, 1 << 20, 144) == 2048
    assert cache_bytes(128, 48, 64) == 48 * 128 * (4 + 16 + 4 + 256)
    assert cache_bytes(256, 32, 192) == 32 * 256 * (4 + 48 + 4 + 768)


def test_pack_keys_against_python_integers():
    rng = np.random.default_rng(0)
    for R, C in ((8, 8), (9, 12), (12, 12), (12, 16), (5, 7)):
        b = rng.integers(-1, 2, (5, R, C)).astype(np.int8)
        nw = (R * C + 63) // 64
        got = pack_keys(b)
        for i in range(5):
            black = sum(1 << j for j, v in enumerate(b[i].reshape(-1)) if v == 1)
            white = sum(1 << j for j, v in enumerate(b[i].reshape(-1)) if v == -1)
            want = [(black >> (64 * w)) & (2 ** 64 - 1) for w in range(nw)] + [(white >> (64 * w)) & (2 ** 64 - 1) for w in range(nw)]
            assert got[i].tolist() == want


@pytest.mark.parametrize("keep", [False, True], ids=["per-search", "keep"])
@pytest.mark.parametrize("nw", [1, 3])
def test_model_against_a_set_per_epoch(keep, nw):
    """A table large enough that no window overflows: a lookup hits exactly when the key was stored before in an epoch the mode
    may read -- the current one, or with keep any since the last clear.  Searches from the empty board (a restart) and clears
    in between."""
    rng = np.random.default_rng(5 + nw)
    S = 1 << 16
    drawn = rng.integers(0, 2 ** 63, (1200, 2 * nw)).astype(np.uint64)
    firsts, pool = [], []                                   # 400 keys whose windows share no slot: nothing is ever replaced
    for k, f in zip(drawn, tt_first(key_hashes(drawn), S).tolist()):
        if len(pool) < 400 and all(min((f - g) % S, (g - f) % S) >= PROBES for g in firsts):
            firsts.append(f)
            pool.append(k)
    assert len(pool) == 400
    t = EvalCache(S, keep)
    epochs, epoch = {}, 0                                   # the reference: epoch -> set of keys
    root_stones = [7, 8, 0, 1, 2, 0, 3, 4, 5, 0, 1]
    for s, rs in enumerate(root_stones):
        if s in (4, 8):
            t.clear()
            epochs.clear()
        if not keep or rs == 0 or epoch == 0:
            epoch += 1
        t.begin_search(rs)
        assert t.epoch == epoch
        for i in rng.integers(0, len(pool), 300):
            key = tuple(pool[i].tolist())
            readable = set().union(*epochs.values()) if keep and epochs else epochs.get(epoch, set())
            got = t.leaf(key, rs + 1 + int(i) % 5)
            assert got == (HIT if key in readable else MISS), (s, i)
            epochs.setdefault(epoch, set()).add(key)
    assert t.c["fallback_first"] == 0 and t.c["hit_current"] > 100 and (t.c["hit_older"] > 100) == keep


def test_epoch_is_24_bits_and_never_zero():
    t = EvalCache(64, False)
    t.epoch = 0xFFFFFE
    t.begin_search(3)
    assert t.epoch == 0xFFFFFF
    t.begin_search(3)
    assert t.epoch == 1


def _colliding(slots, first, n, nw=1, start=1):
    """n distinct keys whose windows start at slot `first`, by brute force"""
    out, k = [], start
    while len(out) < n:
        key = (k,) + (0,) * (2 * nw - 1)
        if first_slot(key, slots) == first:
            out.append(key)
        k += 1
    return out


@pytest.mark.parametrize("first", [5, 57, 60, 63], ids=["inside", "wraps by 1", "wraps by 4", "wraps by 7"])
def test_hand_built_windows(first):
    """64 slots, keys that share a window (one that wraps round the table's end in three of the cases): each replacement rule."""
    S = 64
    keys = _colliding(S, first, 12)
    win = [(first + i) % S for i in range(PROBES)]
    t = EvalCache(S, True)
    assert t.window(key_hashes(np.array([keys[0]], np.uint64))[0]) == win
    t.begin_search(10)                                      # epoch 1
    # never-used slots are taken in probe order, and a never-used slot ends the probe
    for i in range(PROBES):
        assert t.lookup(keys[i], 12) == (False, win[i])
        t.store(keys[i], 12)
    assert t.c["never_used"] == PROBES
    for i in range(PROBES):                                 # all eight are found where they were put
        assert t.lookup(keys[i], 12) == (True, win[i])
    # a full window of live entries: the first slot is replaced, and the entry that sat there is gone
    assert t.lookup(keys[8], 12) == (False, win[0])
    t.store(keys[8], 12)
    assert t.c["fallback_first"] == 1
    assert t.lookup(keys[0], 12) == (False, win[0]) and t.lookup(keys[8], 12) == (True, win[0])
    # cannot recur: an entry with no more stones than the root.  Stones 11 stay, stones 10 go (<=)
    t.key[win[3]], t.meta[win[3]] = keys[3], (1 << 8) | 11
    t.key[win[5]], t.meta[win[5]] = keys[5], (1 << 8) | 10
    assert t.lookup(keys[9], 12) == (False, win[5]) and t.pending[1] == "cannot_recur"
    assert t.lookup(keys[5], 10) == (True, win[5])          # ... but until it is replaced it is still found
    t.begin_search(11)                                      # the root has moved on: keep, stones > 0 -> the same epoch
    assert t.epoch == 1 and t.lookup(keys[9], 12) == (False, win[3])
    # another epoch: a restart from the empty board.  Every entry is replaceable, the first probed goes; with keep all still hit
    t.begin_search(0)
    assert t.epoch == 2
    assert t.lookup(keys[1], 1) == (True, win[1]) and t.c["hit_older"] == 1
    assert t.lookup(keys[9], 1) == (False, win[0]) and t.pending[1] == "other_epoch"
    t.store(keys[9], 1)
    # a hit refreshes nothing: keys[1] was just hit and is still of epoch 1, so it is the next to go
    assert t.lookup(keys[10], 1) == (False, win[1])
    # without keep the same entries are not read
    u = EvalCache(S, False)
    u.begin_search(4)
    u.lookup(keys[0], 5)
    u.store(keys[0], 5)
    assert u.lookup(keys[0], 5) == (True, win[0])
    u.begin_search(5)
    assert u.lookup(keys[0], 6) == (False, win[0]) and u.pending[1] == "other_epoch"
    # clear: nothing is found, the epoch stays
    t.clear()
    assert t.epoch == 2 and t.lookup(keys[9], 1) == (False, win[0]) and t.pending[1] == "never_used"
    assert t.c["wraps"] == (t.c["lookups"] if first > S - PROBES else 0)


def test_book_comes_first_and_takes_no_slot():
    S = 64
    keys = _colliding(S, 9, 3)
    t = EvalCache(S, True, book={keys[0], keys[1]}, book_stones=3)
    t.begin_search(0)
    assert t.leaf(keys[0], 2) == BOOK and t.leaf(keys[2], 2) == MISS and t.leaf(keys[2], 2) == HIT
    assert t.leaf(keys[1], 4) == MISS                       # more stones than the book holds: not looked up there
    assert t.meta[9] != 0 and t.meta[10] != 0 and t.meta[11] == 0 and t.c["book"] == 1 and t.c["lookups"] == 3


def test_hash_depends_on_every_word():
    """The unmutated hash separates positions that differ in the last white word only (the third word of a board over 128
    cells); the mutant does not."""
    base = np.array([[1, 2, 3, 4, 5, 0]], np.uint64)
    other = base.copy()
    other[0, 5] = 1 << 7
    assert key_hashes(base)[0] != key_hashes(other)[0]
    assert key_hashes(base, "hash_drops_last")[0] == key_hashes(other, "hash_drops_last")[0]
    assert int(tt_first(key_hashes(base), 64)[0]) == first_slot(tuple(base[0].tolist()), 64)


# ---- the configurations of the device test, searched by the CPU oracle
@pytest.fixture(scope="module", params=list(K.CONFIGS))
def traced(request):
    name = request.param
    games = K.oracle_searches(name)
    res = [K.model_replay(name, s) for s in games]
    return name, games, res


def test_configurations_exercise_their_rules(traced):
    """Per configuration: the hits on current-epoch entries, a window that wraps, in the overflowing configuration every store
    class, with keep and a restart the hits on older-epoch entries, with the book the leaves it serves."""
    name, games, res = traced
    c = K.sum_counts(r[1] for r in res)
    print(name, "slots", K.slots_of(K.CONFIGS[name]), c)
    assert not K.coverage_shortfalls(name, c)
    cfg = K.CONFIGS[name]
    assert 32 <= cfg["G"] <= 64 and 30 <= cfg["sims"] <= 150
    assert cfg["sims"] < (cfg.get("nodes_per_game") or cfg["sims"] + 2)


def test_start_batches_hold_pass_roots_and_finished_games():
    import oracle_lib as O
    cfg = K.CONFIGS["8x8-tt"]
    boards, players = K.late_positions(cfg["G"], 8, 8, cfg["max_ply"], cfg["seed"])
    legal, ended = O.valid_mask(boards, players), O.game_ended(boards, players)
    assert ((legal.sum(1) == 0) & (ended == 0)).sum() >= 1 and (ended != 0).sum() >= 1


def test_every_mutant_changes_the_predicted_sequence():
    """Every listed fault changes the hit / miss sequence on the inputs of at least one configuration (and the fault in the
    hash on a board of three words): the device comparison would fail for it."""
    caught = {m: [] for m in MUTANTS}
    for name in K.CONFIGS:
        games = K.oracle_searches(name)
        for m in MUTANTS:
            diff = 0
            for s in games:
                a, b = K.model_replay(name, s)[0], K.model_replay(name, s, mutant=m)[0]
                diff += sum(int((x != y).sum()) for x, y in zip(a, b))
            if diff:
                caught[m].append((name, diff))
    print(caught)
    assert all(caught.values()), caught
    assert "12x12-keep" in dict(caught["hash_drops_last"])


def test_replay_equals_the_calls_one_by_one():
    name = "8x8-keep"
    cfg = K.CONFIGS[name]
    s = K.oracle_searches(name)[3]                          # a game that restarts
    out, c = K.model_replay(name, s)
    t = EvalCache(K.slots_of(cfg), True)
    for i, (rs, keys, stones) in enumerate(s):
        if i in cfg["clear_before"]:
            t.clear()
        t.begin_search(rs)
        got = [t.leaf(k, int(n)) for k, n in zip(keys.tolist(), stones)]
        assert got == out[i].tolist()
    assert t.c == c
