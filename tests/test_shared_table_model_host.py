"""The array restatements of tests/shared_table_model.py that the device tests of the replacing shared evaluation table compare
against (tests/test_gpu_shared_table_state.py): sweep_arrays against the slot-by-slot Table.sweep on a few hundred crafted
tables, and the array arithmetic of bb_hash against Python integers.  No device.

bb_hash has no independent oracle on the host; what pins it to csrc/yy_engine.hip is the device test named above."""
import numpy as np
import pytest

from shared_table_model import (CLOCKS, M32, PROBES, SW_CUTOFF, SW_EVICTED, SW_LIVE, TOMBSTONE, Table, bb_hash, clock,
                                crafted_state, older, stamp_line, sweep_arrays, tt_first, tt_tag, tt_window)


def table_of(claim, last_hit, stamp, cutoff, evicted):
    t = Table(len(claim), stamp=stamp)
    t.claim[:], t.last_hit[:], t.cutoff = claim, last_hit, cutoff
    t.c["evicted"] = evicted
    return t


def live_count(claim):
    st = claim & np.uint64(M32)
    return int(((st != 0) & (st != TOMBSTONE)).sum())


MARKS = ("live", "live-1", "live+1", "0", "slots")


def mark_of(name, live, slots):
    return dict([("live", live), ("live-1", max(live - 1, 0)), ("live+1", live + 1), ("0", 0), ("slots", slots)])[name]


@pytest.mark.parametrize("clk", CLOCKS)
def test_sweep_arrays_is_the_slot_by_slot_sweep(clk):
    """4 clocks x 5 high-water marks x 15 states = 300 tables of 8 to 64 slots; the table without a cutoff is swept twice."""
    c = clock(clk)
    evicted_any = recorded_any = 0
    for mark in MARKS:
        for seed in range(15):
            slots = (8, 16, 32, 64)[seed % 4]
            claim, last = crafted_state(slots, c, 1000 * CLOCKS.index(clk) + seed)
            t = table_of(claim, last, c["now"], c["word"], 77)
            hw = mark_of(mark, live_count(claim), slots)
            cutoff, total = c["word"], 77
            for _ in range(2 if clk == "no-cutoff" else 1):
                gone = t.sweep(hw)
                claim, words, got = sweep_arrays(claim, last, c["now"], cutoff, total, hw)
                assert got.tolist() == gone and np.array_equal(claim, t.claim), (clk, mark, seed)
                assert words == {SW_LIVE: t.c["live"], SW_EVICTED: t.c["evicted"], SW_CUTOFF: t.cutoff}
                assert np.array_equal(t.last_hit, last)
                recorded_any += t.cutoff != cutoff
                cutoff, total = words[SW_CUTOFF], words[SW_EVICTED]
                evicted_any += len(gone)
    assert evicted_any > 0 and (recorded_any > 0 or clk == "now-is-cutoff")       # there the stamp recorded is the old one


def test_sweep_arrays_at_the_mark():
    """Exactly at the mark nothing is evicted and nothing recorded; one entry above it the sweep evicts and records; without
    a cutoff it only records."""
    c = clock("plain")
    claim, last = crafted_state(64, c, 5)
    live = live_count(claim)
    same, words, gone = sweep_arrays(claim, last, c["now"], c["word"], 3, live)
    assert len(gone) == 0 and np.array_equal(same, claim) and words == {SW_LIVE: live, SW_EVICTED: 3, SW_CUTOFF: c["word"]}
    new, words, gone = sweep_arrays(claim, last, c["now"], c["word"], 3, live - 1)
    assert len(gone) > 0 and words == {SW_LIVE: live - len(gone), SW_EVICTED: 3 + len(gone), SW_CUTOFF: c["now"]}
    assert (new[gone] == np.uint64(TOMBSTONE)).all() and np.array_equal(np.delete(new, gone), np.delete(claim, gone))
    for at in range(64):                                # the rule, slot by slot and in words
        st = int(claim[at]) & M32
        want = st not in (0, TOMBSTONE) and older(st, c["cutoff"], c["now"]) and older(int(last[at]), c["cutoff"], c["now"])
        assert (at in gone) == want
    same, words, gone = sweep_arrays(claim, last, c["now"], 0, 3, 0)
    assert len(gone) == 0 and np.array_equal(same, claim) and words == {SW_LIVE: live, SW_EVICTED: 3, SW_CUTOFF: c["now"]}


def test_the_clocks():
    w = clock("wrap")
    assert w["cutoff"] == M32 - 12 and w["now"] == 9 and w["word"] == w["cutoff"]
    assert all(s > w["now"] for s in w["old"]) and any(s > w["cutoff"] for s in w["mid"]) and any(s < w["now"] for s in w["mid"])
    assert 0 not in w["old"] + w["mid"] and TOMBSTONE not in w["old"] + w["mid"]
    assert all(older(s, w["cutoff"], w["now"]) for s in w["old"]) and not any(older(s, w["cutoff"], w["now"]) for s in w["mid"])
    p = clock("plain")
    assert (p["cutoff"], p["now"], p["word"]) == (1000, 1040, 1000) and clock("no-cutoff")["word"] == 0
    e = clock("now-is-cutoff")
    assert e["cutoff"] == e["now"] == 1000 and e["mid"] == []
    assert stamp_line(M32 - 2, 4) == [M32 - 2, M32 - 1, 1, 2]


def test_crafted_states_hold_every_fate():
    c = clock("wrap")
    claim, last = crafted_state(4096, c, 1)
    st = (claim & np.uint64(M32)).astype(np.int64).reshape(-1, 4)
    tag = (claim >> np.uint64(32)).astype(np.int64)
    live = (st != 0) & (st != TOMBSTONE)
    assert (st == 0).all(1).any() and (st == TOMBSTONE).all(1).any() and live.all(1).any()          # quads of one fate
    assert ((st == 0).sum(1) == 1).any() and ((st == TOMBSTONE).sum(1) == 1).any()                  # and mixed ones
    lv = live.reshape(-1)
    assert (tag[lv] >> 31).any() and (tag[lv] == 0).any()
    for cls in (c["old"][0], c["cutoff"], c["mid"][0], c["mid"][-1], c["now"]):                     # both words, every class
        assert (st.reshape(-1)[lv] == cls).any() and (last[lv] == cls).any()
    older_ins = np.array([older(int(s), c["cutoff"], c["now"]) for s in st.reshape(-1)[lv]])
    older_hit = np.array([older(int(s), c["cutoff"], c["now"]) for s in last[lv]])
    for a in (False, True):                                                                         # drawn independently
        for b in (False, True):
            assert ((older_ins == a) & (older_hit == b)).any()


def py_hash(words):
    h, M = 0x9E3779B97F4A7C15, (1 << 64) - 1
    for w in words:
        h ^= int(w) & M
        h ^= h >> 33
        h = (h * 0xFF51AFD7ED558CCD) & M
        h ^= h >> 33
        h = (h * 0xC4CEB9FE1A85EC53) & M
        h ^= h >> 33
    return h


@pytest.mark.parametrize("nw", [1, 2, 3])
def test_bb_hash_array_arithmetic(nw):
    """uint64 array arithmetic against Python integers (not an oracle of the hash: the same statement, other arithmetic), for
    keys as the device tables hold them (int64, sign bit set in some), and the window and tag derived from the hash."""
    rng = np.random.default_rng(nw)
    keys = rng.integers(-(1 << 63), 1 << 63, (50, 2 * nw), dtype=np.int64)
    keys[0] = 0
    keys[1] = -1
    h = bb_hash(keys)
    assert h.dtype == np.uint64 and h.shape == (50,)
    assert [int(x) for x in h] == [py_hash(k) for k in keys]
    assert int(bb_hash(keys[7])) == py_hash(keys[7]) and np.array_equal(bb_hash(keys.view(np.uint64)), h)
    assert len(set(h.tolist())) == 50
    for slots in (64, 4096, 1 << 22):
        first, win = tt_first(h, slots), tt_window(h, slots)
        assert win.shape == (50, PROBES) and np.array_equal(win[:, 0], first)
        for i in range(50):
            assert int(first[i]) == (int(h[i]) & M32) & (slots - 1) and int(tt_tag(h)[i]) == int(h[i]) >> 32
            assert win[i].tolist() == [(int(first[i]) + j) % slots for j in range(PROBES)]
            if slots <= 4096:                                                   # the window the slot-by-slot model probes
                assert win[i].tolist() == Table(slots).window(int(h[i])) and int(tt_tag(h)[i]) == Table.tag(int(h[i]))
