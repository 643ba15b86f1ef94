"""The replacing shared evaluation table, state by state: what the device leaves in `claim`, `last_hit`, `sweep_state` and `stamp`
against the numpy restatement of its rules (tests/shared_table_model.py), exactly -- the data are integers and copied float bits.
tests/test_gpu_shared_replace.py pins that no table decision changes a game; this file pins the decisions themselves.

B  the three sweep launches of csrc/yy_shared_table.hip against sweep_arrays, slot by slot: crafted states written straight into
   the table's tensors, from 64 slots (16 lanes of one wave) to 2^22 (2048 workgroups, two grid-stride trips), under four clocks
   (plain, now == cutoff, across the stamp wrap, no cutoff yet) and high-water marks at, below and far from the live count.
C  k_stamp, leaf_lookup and the sweep with the stamp wrapping in the middle of a self-play run.
D  the probe rules on the device: every live entry of a searched table sits where bb_hash puts it (the device check of the model's
   bb_hash, NW = 1, 2, 3), and planted windows -- tombstone, never-used slot, full window, false tag, current stamp -- with one
   game and one simulation, so that the order of the one lookup and the one insert is fixed."""
import functools

import numpy as np
import pytest

from hash_eval import hash_eval_torch
from shared_table_model import (CLOCKS, M32, SW_COUNT, SW_CUTOFF, SW_EVICTED, SW_EVICTING, SW_LIVE, TOMBSTONE, Table, bb_hash, clock,
                                crafted_state, stamp_line, sweep_arrays, tt_tag, tt_window)
from test_gpu_shared_replace import BASE, KEYS, HashEval, no_table, same, snapshot

pytestmark = pytest.mark.gpu
U32, U64 = np.uint32, np.uint64


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    import yinyang_game_alphazero_amd as p
    return p


def dev(a):
    """A numpy array of unsigned words as the signed device tensor of the same bits."""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({U32: np.int32, U64: np.int64}.get(a.dtype.type, a.dtype))).cuda()


def set_stamp(table, s):
    import torch
    table.stamp.copy_(dev(np.array([s], U32)))
    torch.cuda.synchronize()


def stamp_of(table):
    return int(table.stamp.cpu().numpy().view(U32)[0])


def stamps_live(claim):
    st = (claim & U64(M32)).astype(np.int64)
    return st, np.flatnonzero((st != 0) & (st != TOMBSTONE))


def ev(planes):
    return hash_eval_torch(planes, 10, 11)


# =============================================================================== B. the sweep launches, slot by slot
SLOT_COUNTS = [
    64,            # 16 quads: lanes 0..15 of wave 0 (what tests/test_gpu_shared_replace.py sweeps)
    256,           # 64 quads: exactly one full wave
    512,           # two waves: the first cross-wave sum of block_sum
    1024,          # 256 quads: one full workgroup, four waves
    4096,          # four workgroups: the first cross-workgroup atomicAdd into the sweep words
    1 << 21,       # 2^19 quads: exactly 2048 workgroups, one grid-stride trip each
    1 << 22,       # two grid-stride trips
]
SENTINEL = (0x5151515151515151, 0x6262626262626262, 0x7373737373737373)     # sweep words 5..7: no launch may touch them
STALE_LIVE, EVICTED_BEFORE = 4242, 77


def sweep_cases(slots):
    """(clock, high-water mark, seed) per slot count.  Up to 4096 slots the whole product, 32 cases; the two large tables run
    every clock one entry above the mark, and at the mark 2^21 every clock, 2^22 the plain one: 8 and 5 cases."""
    if slots <= 4096:
        return [(c, m, s) for c in CLOCKS for m in ("live", "live-1", "0", "slots") for s in (0, 1)]
    if slots == 1 << 21:
        return [(c, m, 0) for c in CLOCKS for m in ("live-1", "live")]
    return [(c, "live-1", 0) for c in CLOCKS] + [("plain", "live", 0)]


class SweepRig:
    """A replacing table of `slots` slots on the smallest board (2x2: 48 bytes a slot, 200 MB at 2^22), attached to a context;
    keys, values and rows hold a sentinel pattern that no sweep may change."""

    def __init__(self, pkg, slots):
        import torch
        self.slots = slots
        self.ctx = pkg.engine.BatchedMCTS(1, 2, 2, 4)
        self.table = t = pkg.engine.SharedEvaluations(2, 2, slots, replace=True)
        self.ctx.set_shared_evaluations(t)
        i = torch.arange(slots, dtype=torch.int64, device="cuda")
        t.keys.copy_((i[:, None] * 2 + torch.arange(2, device="cuda") + 1) * -0x61C8864680B583EB)
        t.value.copy_(((i + 1) * 2654435761).to(torch.int32).view(torch.float32))
        t.policy.copy_(((i[:, None] * 4 + torch.arange(4, device="cuda") + 1) * 40503).to(torch.int32).view(torch.float32))
        self.rows = [x.clone() for x in (t.keys, t.value.view(torch.int32), t.policy.view(torch.int32))]

    def close(self):
        self.ctx.close()

    def state(self, clk, seed):
        claim, last = crafted_state(self.slots, clk, seed)
        old = np.array(clk["old"][:4], U64)               # the last workgroup's last quad: live, old in both words -> it goes
        claim[-4:] = (np.array([1 << 31, 0, 7, M32], U64) << U64(32)) | old
        last[-4:] = old.astype(U32)
        return claim, last

    def run(self, clk, mark, seed):
        import torch
        t, slots = self.table, self.slots
        claim, last = self.state(clk, seed)
        live = len(stamps_live(claim)[1])
        hw = dict([("live", live), ("live-1", live - 1), ("0", 0), ("slots", slots)])[mark]
        t.high_water = hw / slots                          # exact: slots is a power of two
        assert int(t.high_water * slots) == hw
        now, word, total = clk["now"], clk["word"], EVICTED_BEFORE
        t.claim.copy_(dev(claim))
        t.last_hit.copy_(dev(last))
        t.sweep_state.copy_(dev(np.array((0, 0, STALE_LIVE, total, word) + SENTINEL, U64)))
        set_stamp(t, now)
        evicted = 0
        for nth in range(2 if word == 0 else 1):           # without a cutoff the first sweep only records, the second evicts
            want, words, gone = sweep_arrays(claim, last, now, word, total, hw)
            t.sweep()
            got = t.claim.cpu().numpy().view(U64)
            tag = (clk, mark, seed, nth)
            assert np.array_equal(got, want), (tag, np.flatnonzero(got != want)[:8])
            # an evicted slot is exactly SH_CLAIM(0, TOMBSTONE); kept and free slots keep every bit (the model's array says both)
            assert (got[gone] == U64(TOMBSTONE)).all()
            assert np.array_equal(t.last_hit.cpu().numpy().view(U32), last), tag
            for x, x0 in zip((t.keys, t.value.view(torch.int32), t.policy.view(torch.int32)), self.rows):
                assert torch.equal(x, x0), tag
            assert stamp_of(t) == now, tag
            sw = [int(x) for x in t.sweep_state.cpu().numpy().view(U64)]
            assert sw[SW_COUNT] == 0 and sw[SW_EVICTING] == 0 and tuple(sw[5:]) == SENTINEL, (tag, sw)
            assert sw[SW_LIVE] == words[SW_LIVE] and sw[SW_EVICTED] == words[SW_EVICTED] and sw[SW_CUTOFF] == words[SW_CUTOFF], (tag, sw, words)
            live_before = words[SW_LIVE] + len(gone)
            assert sw[SW_CUTOFF] == (now if live_before > hw else word), tag     # recorded iff the live count exceeded the mark
            if live_before <= hw or word == 0:
                assert len(gone) == 0, tag
            c = t.counters()
            assert c == dict(hits=0, inserts=0, dropped=0, duplicates=0, evicted=words[SW_EVICTED], live=words[SW_LIVE]), (tag, c)
            assert t.fill() == words[SW_LIVE], tag
            if len(gone):                                  # the state reaches where the case is meant to reach
                assert gone[-1] == slots - 1
                if slots > 1 << 21:                        # both grid-stride trips: 2048 workgroups x 256 quads = 2^21 slots a trip
                    assert gone[0] < 1 << 21 and np.count_nonzero(gone >= 1 << 21) > 1
            claim, word, total = want, words[SW_CUTOFF], words[SW_EVICTED]
            evicted += len(gone)
        return evicted


@pytest.mark.parametrize("slots", SLOT_COUNTS, ids=lambda n: f"{n}-slots")
def test_sweep_is_the_model_slot_by_slot(pkg, slots):
    rig = SweepRig(pkg, slots)
    try:
        evicted = {}
        for c, mark, seed in sweep_cases(slots):
            evicted[c, mark, seed] = rig.run(clock(c), mark, seed)
    finally:
        rig.close()
    for (c, mark, seed), n in evicted.items():             # above the mark every clock evicts (its second sweep without a cutoff)
        assert (n > 0) == (mark in ("live-1", "0")), (c, mark, seed, n)


# =============================================================================== C. the tree steps across the stamp wrap
def table_now(t):
    """The stamp, the insert stamps and the last-hit words as the stream stands: between two launches."""
    return dict(stamp=stamp_of(t), stamps=t.stamps().cpu().numpy(), last_hit=t.last_hit.cpu().numpy().view(U32) if t.replace else None)


def play_parts(pkg, start, parts, high_water=None, every=None, **kw):
    """test_gpu_shared_replace.play with the table's stamp set to `start` before the first launch and the run split into
    run() calls of `parts` games -> (examples, the table's counters / stamp / fill after every part, the table's arrays at
    every `every`-th progress call of the engine, with `prev`, the stamp at the call before -- a lockstep engine calls every
    10 moves, a free-running one after every batch of poll_steps steps and the sweep behind it -- and at the end)."""
    import torch
    shape, G, _, sims = BASE
    eng = pkg.SelfPlayEngine(pkg.YinYangGame(*shape), HashEval(), num_simulations=sims, concurrent_games=G, seed=11, **kw)
    try:
        t = eng.shared
        if high_water is not None:
            t.high_water = high_water
        set_stamp(t, start)
        out, marks, snaps, ticks = [], [], [], [start]

        def progress(_):
            ticks.append(stamp_of(t))                     # the stamp at every call: a snapshot names the one before it
            if every and (len(ticks) - 1) % every == 0:
                snaps.append(dict(table_now(t), prev=ticks[-2]))

        for n in parts:
            out.append(eng.run(n, progress))
            marks.append(dict(t.counters(), stamp=stamp_of(t), fill=t.fill()))
        ex = pkg.self_play.sort_examples({k: torch.cat([o[k] for o in out]) for k in KEYS})
        snaps.append(dict(table_now(t), prev=None))
    finally:
        eng.close()
    return {k: ex[k].cpu().numpy() for k in KEYS}, marks, snaps


PARTS = (BASE[2] // 2, BASE[2] - BASE[2] // 2)
AFTER_WRAP = 40                                          # launches of the first part that carry a wrapped stamp


@functools.lru_cache(maxsize=None)
def launches(pkg, free_running):
    """Tree-step launches of the two parts of the run, measured as the stamp's advance in a plain run from stamp 1 (every
    launch advances it by one there).  Computed once per engine kind."""
    kw = dict(free_running=True, poll_steps=1) if free_running else {}
    _, marks, _ = play_parts(pkg, 1, PARTS, shared_evaluations=64, shared_evaluations_replace=True, **kw)
    return marks[0]["stamp"] - 1, marks[1]["stamp"] - 1


WRAP_CASES = {
    "replacing-lockstep": dict(shared_evaluations=512, shared_evaluations_replace=True, high_water=0.5),
    "replacing-free-running-sweep-every-step": dict(shared_evaluations=64, shared_evaluations_replace=True, high_water=0.0,
                                                    free_running=True, poll_steps=1),
    "insert-only-lockstep": dict(shared_evaluations=8192),
    "replacing-64-slots-lockstep": dict(shared_evaluations=64, shared_evaluations_replace=True),
}


@pytest.mark.parametrize("case", list(WRAP_CASES))
def test_the_stamp_wraps_in_the_middle_of_a_run(pkg, case):
    """The run's 24 games as two run() calls of 12 (the engines continue the game indices: the same games as one run,
    tests/test_gpu_free_running.py).  The start stamp puts the wrap AFTER_WRAP launches before the end of the first part, about
    the middle of the run, so the counters read between the parts are the counters at the wrap: what the second part adds
    is hits and evictions after it, with entries of both sides of the wrap in the table.  (Splitting rather than comparing the
    totals with a run from stamp 1: which of two positions takes the last free slot of two overlapping windows depends on the
    order of the games within a launch, so totals are not a function of the start stamp alone.)"""
    kw = dict(WRAP_CASES[case])
    high_water = kw.pop("high_water", None)
    run_kw = {k: v for k, v in kw.items() if k in ("free_running", "poll_steps")}
    replace = kw.get("shared_evaluations_replace", False)
    first, total = launches(pkg, bool(kw.get("free_running")))
    before = first - AFTER_WRAP                           # launches that carry a stamp up to 2^32 - 2
    assert 0.25 * total < before < 0.75 * total, (first, total)
    start = M32 - 1 - before
    assert stamp_line(start, before + 2)[-2:] == [M32 - 1, 1]
    free = bool(kw.get("free_running"))
    got, marks, snaps = play_parts(pkg, start, PARTS, high_water=high_water, every=48 if free else 1, **kw)
    print(case, "launches", (first, total), "start", start, marks)
    want, _ = no_table(pkg, *BASE, **run_kw)
    same(got, want)
    at_wrap, end = marks
    for m in marks:                                       # it wrapped, and 0 and the tombstone were skipped
        assert 0 < m["stamp"] < start and m["stamp"] != TOMBSTONE, m
    if not kw.get("free_running"):                        # lockstep: the launches are a function of the games alone
        line = stamp_line(start, total + 1)
        assert (at_wrap["stamp"], end["stamp"]) == (line[first], line[total]) == (AFTER_WRAP, AFTER_WRAP + total - first)
    assert end["hits"] > at_wrap["hits"] > 0 and end["inserts"] > at_wrap["inserts"]
    if replace:
        assert end["evicted"] > at_wrap["evicted"]
    # no live entry under stamp 0 or the tombstone: a launch that carried either would have counted inserts that show as free
    for m in marks:
        assert m["fill"] == m["inserts"] - m.get("evicted", 0), m
    assert np.count_nonzero((snaps[-1]["stamps"] != 0) & (snaps[-1]["stamps"] != TOMBSTONE)) == end["fill"]
    assert snaps[-1]["stamp"] == end["stamp"] and len(snaps) >= 3
    seen = wrapped = 0
    for s in snaps:                                       # while the run is going (both sides of the wrap) and at its end
        stamps, now = s["stamps"], s["stamp"]
        live = np.flatnonzero((stamps != 0) & (stamps != TOMBSTONE))
        seen += len(live)
        wrapped += len(live) if now < start else 0
        age = (now - stamps[live]) & M32                  # seen from the stamp of the moment; the two skipped values add 2
        assert (age <= ((now - start) & M32)).all(), (now, age.max())      # every stamp in the table was handed out in this run
        if replace:
            hit = s["last_hit"][live].astype(np.int64)
            assert ((hit != 0) & (hit != TOMBSTONE)).all()
            assert (((now - hit) & M32) <= age).all()     # a last-hit stamp is never older than its insert stamp
            if free and s["prev"] is not None:
                # a sweep after every step, above a mark of 0: the sweep in front of this snapshot had the stamp of the call
                # before for its cutoff (or an older one, if the table was empty then and everything here is newer), so
                # whatever it left was inserted or served since -- an entry kept too long shows here, whatever its number
                assert (((now - hit) & M32) <= ((now - s["prev"]) & M32)).all(), (now, s["prev"])
    assert wrapped > 0 and seen > wrapped                 # entries were looked at on either side of the wrap


# =============================================================================== D. probe rules and structure
def one_game(pkg, R, C, slots, max_sims):
    ctx = pkg.engine.BatchedMCTS(1, R, C, max_sims)
    table = pkg.engine.SharedEvaluations(R, C, slots, replace=True)
    ctx.set_shared_evaluations(table)
    return ctx, table


def search(ctx, board, player, sims):
    import torch
    b = torch.from_numpy(np.ascontiguousarray(np.asarray(board, np.int8)[None])).cuda()
    return ctx.search(b, torch.full((1,), player, dtype=torch.int8, device="cuda"), ev, sims).cpu().numpy()


def midgame(pkg, R, C, plies=4):
    game = pkg.YinYangGame(R, C)
    board, player = game.getInitBoard(), 1
    for _ in range(plies):
        a = int(np.flatnonzero(game.getValidMoves(board, player))[0])
        board, player = game.getNextState(board, player, a)
    return np.asarray(board.board, np.int8), player


def rows_of(pkg, keys, R, C):
    """HashEval's (policy, value) of the positions `keys` (int64 [n, 2 * NW]: black words, white words), as float bits."""
    import torch
    nw = keys.shape[1] // 2
    if not len(keys):
        return np.zeros((0, R * C), U32), np.zeros(0, U32)
    k = torch.from_numpy(np.ascontiguousarray(keys)).cuda()
    boards = pkg.engine.unpack_boards(k[:, :nw].t().contiguous(), k[:, nw:].t().contiguous(), R, C)
    policy, value = ev(pkg.engine.encode_planes(boards))
    return policy.cpu().numpy().view(U32), value.cpu().numpy().view(U32)


def check_structure(pkg, table, R, C):
    """The table is a state the model can reach: every live entry under its key's tag, inside its key's probe window, with no
    never-used slot in front of it, holding the evaluator's row of its key; no key twice under one insert stamp."""
    s = snapshot(table)
    st, live = stamps_live(s["claim"])
    keys = s["keys"][live]
    h = bb_hash(keys)
    assert np.array_equal((s["claim"][live] >> U64(32)).astype(np.int64), tt_tag(h))
    win = tt_window(h, table.slots)
    here = win == live[:, None]
    assert here.sum(1).tolist() == [1] * len(live)
    in_front = np.arange(win.shape[1])[None, :] < here.argmax(1)[:, None]
    assert not ((st[win] == 0) & in_front).any()
    policy, value = rows_of(pkg, keys, R, C)
    assert np.array_equal(s["policy"][live].view(U32), policy) and np.array_equal(s["value"][live].view(U32), value)
    assert len({(int(st[at]), s["keys"][at].tobytes()) for at in live}) == len(live)
    hit = s["last_hit"][live].astype(np.int64)
    assert ((hit != 0) & (hit != TOMBSTONE)).all()
    return len(live)


@pytest.mark.parametrize("slots", [64, 4096])
@pytest.mark.parametrize("R,C,sims", [(4, 4, 256), (9, 12, 128), (12, 12, 128)], ids=["4x4-one-word", "9x12-two-words", "12x12-three-words"])
def test_every_entry_sits_where_the_model_puts_it(pkg, R, C, sims, slots):
    ctx, table = one_game(pkg, R, C, slots, sims)
    try:
        table.high_water = 0.0
        empty = np.zeros((R, C), np.int8)
        search(ctx, empty, 1, sims)
        c = table.counters()
        n = check_structure(pkg, table, R, C)
        assert n == c["inserts"] > 0 and c["evicted"] == 0
        table.sweep()                                     # records the stamp
        search(ctx, *midgame(pkg, R, C), sims // 2)
        table.sweep()                                     # evicts what the second search neither inserted nor was served
        c = table.counters()
        n = check_structure(pkg, table, R, C)
        assert c["evicted"] > 0 and n == c["inserts"] - c["evicted"] == c["live"]      # 64 slots: the first search had filled
        assert n > 0 or slots == 64                       # every window, so the second inserted next to nothing that could stay
        assert np.count_nonzero(stamps_live(table.claim.cpu().numpy().view(U64))[0] == TOMBSTONE) == c["evicted"]
        search(ctx, empty, 1, sims)                       # the first search again: its inserts land in the tombstones
        c2 = table.counters()
        n = check_structure(pkg, table, R, C)
        assert n == c2["inserts"] - c2["evicted"] > 0 and c2["inserts"] > c["inserts"]
        print(R, C, slots, c2, "fill", n)
        ctx.status()
    finally:
        ctx.close()


START = 100                                               # the stamp before a planted search: its select is launch 102, its insert 103


def one_simulation(pkg, table_state=None):
    """One search of one simulation from the empty 4x4 board on a 64-slot table: begin, then three stamped launches -- the root
    expansion, the select (the one lookup), the expansion (the one insert).  -> what the device left."""
    import torch
    ctx, table = one_game(pkg, 4, 4, 64, 4)
    try:
        if table_state is not None:
            for name, a in table_state.items():
                getattr(table, name).copy_(dev(a) if a.dtype.kind == "u" else torch.from_numpy(a).cuda())
        else:
            for x in (table.keys, table.value, table.policy):
                x.zero_()
        set_stamp(table, START)
        counts = search(ctx, np.zeros((4, 4), np.int8), 1, 1)
        visits, wsum = ctx.root_stats()
        out = dict(snapshot(table), counts=counts, wsum=wsum.cpu().numpy().view(U64), visits=visits.cpu().numpy(),
                   stamp=stamp_of(table), c=table.counters(), evals=ctx.status()["evals"])
    finally:
        ctx.close()
    return out


@pytest.fixture(scope="module")
def first_leaf(pkg):
    """P, the first leaf of the search from the empty 4x4 board: the one entry a 1-simulation search leaves in an empty table."""
    r = one_simulation(pkg)
    lookup_stamp, insert_stamp = stamp_line(START, 4)[2:]
    st, live = stamps_live(r["claim"])
    assert len(live) == 1 and r["stamp"] == insert_stamp and r["evals"] == 1
    assert r["c"] == dict(hits=0, inserts=1, dropped=0, duplicates=0, evicted=0, live=0)
    at = int(live[0])
    key = r["keys"][at].copy()
    h = int(bb_hash(key))
    window = tt_window(U64(h), 64).tolist()
    assert at == window[0] and int(r["claim"][at]) == (h >> 32) << 32 | insert_stamp and int(r["last_hit"][at]) == insert_stamp
    policy, value = rows_of(pkg, key[None], 4, 4)
    assert np.array_equal(r["policy"][at].view(U32), policy[0]) and r["value"][at].view(U32) == value[0]
    return dict(key=key, h=h, tag=h >> 32, window=window, policy=r["policy"][at].copy(), value=r["value"][at].copy(),
                counts=r["counts"], wsum=r["wsum"], visits=r["visits"], lookup_stamp=lookup_stamp, insert_stamp=insert_stamp)


def foreign(i):
    """A key that is not P's (no position at all: lookups compare keys in full, nothing else reads them)."""
    return np.array([(i + 3) << 20, i + 1], np.int64)


# window slot -> what sits there: "P" / "P-now" (P under an old stamp / under the stamp of the coming lookup), "tomb", a foreign
# entry ("f": another tag, "f-tag": P's tag), absent: never used.  Then: the slot the lookup hits, the slot the insert takes.
PLANTED = {
    "1-behind-a-tombstone": (dict([(0, "tomb"), (1, "P")]), 1, None),
    "2-behind-a-never-used-slot": (dict([(1, "P")]), None, 0),
    "3-tombstone-in-a-full-window": (dict([(i, "f") for i in range(8)] + [(3, "tomb")]), None, 3),
    "4-full-window": (dict([(i, "f") for i in range(8)]), None, None),
    "5-false-tag": (dict([(0, "f-tag")]), None, 1),
    "5b-false-tag-in-front-of-the-position": (dict([(0, "f-tag"), (1, "P")]), 1, None),
    "6-under-the-current-stamp": (dict([(0, "P-now")]), None, 1),
}


@pytest.mark.parametrize("case", list(PLANTED))
def test_planted_window(pkg, first_leaf, case):
    P = first_leaf
    plan, hit_at, insert_at = PLANTED[case]
    W = P["window"]
    model = Table(64, stamp=START)
    keys = np.full((64, 2), -0x0123456789ABCDEF, np.int64)                # rows nobody may read: a sentinel
    value, policy = np.full(64, -7.5, np.float32), np.full((64, 16), 0.375, np.float32)
    for i, what in plan.items():
        at = W[i]
        if what == "tomb":
            model.claim[at] = U64(TOMBSTONE)
            continue
        mine = what in ("P", "P-now")
        stamp = P["lookup_stamp"] if what == "P-now" else 50 + i
        tag = P["tag"] if mine or what == "f-tag" else P["tag"] ^ (i + 1)
        model.claim[at], model.last_hit[at] = U64(tag << 32 | stamp), stamp
        keys[at] = P["key"] if mine else foreign(i)
        model.key[at] = keys[at].tobytes()
        if mine:                                           # the evaluator's own row: a hit must not change the search
            value[at], policy[at] = P["value"], P["policy"]
    planted = dict(claim=model.claim.copy(), last_hit=model.last_hit.copy(), keys=keys, value=value, policy=policy)
    r = one_simulation(pkg, planted)
    # the model: the select's launch looks P up, the expansion's launch inserts it if that missed
    model.begin_launch()
    model.begin_launch()
    assert model.stamp == P["lookup_stamp"]
    found = model.lookup(P["key"].tobytes(), P["h"])
    model.begin_launch()
    assert model.stamp == P["insert_stamp"] == r["stamp"]
    outcome = "hit" if found is not None else model.insert(P["key"].tobytes(), P["h"])
    print(case, outcome, r["c"], "evals", r["evals"])
    assert found == (None if hit_at is None else W[hit_at])               # the plan above says what the model says
    assert outcome == ("hit" if hit_at is not None else "inserted" if insert_at is not None else "dropped")
    assert np.array_equal(r["claim"], model.claim), np.flatnonzero(r["claim"] != model.claim)
    assert np.array_equal(r["last_hit"], model.last_hit), np.flatnonzero(r["last_hit"] != model.last_hit)
    assert r["c"] == dict(model.c, live=0), (r["c"], model.c)
    assert r["evals"] == (0 if outcome == "hit" else 1)                   # a served leaf asks for no evaluator row
    want = {k: planted[k].copy() for k in ("keys", "value", "policy")}
    if insert_at is not None:
        at = W[insert_at]
        assert int(r["claim"][at]) == P["tag"] << 32 | P["insert_stamp"] and int(r["last_hit"][at]) == P["insert_stamp"]
        want["keys"][at], want["value"][at], want["policy"][at] = P["key"], P["value"], P["policy"]
    if hit_at is not None:
        assert int(r["last_hit"][W[hit_at]]) == P["lookup_stamp"] and r["c"]["hits"] == 1
        assert np.array_equal(r["claim"], planted["claim"])
    if outcome == "dropped":
        assert r["c"]["dropped"] == 1 and np.array_equal(r["claim"], planted["claim"]) and np.array_equal(r["last_hit"], planted["last_hit"])
    for k in want:                                                        # nothing else was written
        assert np.array_equal(r[k].view(np.uint8), want[k].view(np.uint8)), k
    # the planted row is the evaluator's own: the search is the empty-table search
    assert np.array_equal(r["counts"], P["counts"]) and np.array_equal(r["visits"], P["visits"]) and np.array_equal(r["wsum"], P["wsum"])
