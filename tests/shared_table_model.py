"""A numpy restatement of the replacing shared evaluation table (include/yy_engine.h yy_mcts_set_shared_evaluations_replacing,
csrc/yy_engine.hip shared_store / leaf_lookup, csrc/yy_shared_table.hip): claim, duplicate, hit mark, sweep and the stamp-wrap
rule, one slot operation at a time and in program order.  A launch is the span between two begin_launch() calls; within it
the model applies the calls in the order given (the device's games run concurrently; the properties pinned here do not depend
on the order).  Positions are (key, hash) pairs: the key is what lookups compare in full, the hash picks the probe window (low
bits) and the tag (high 32 bits)."""
import numpy as np

TOMBSTONE = 0xFFFFFFFF
PROBES = 8
M32 = 0xFFFFFFFF


def next_stamp(s):
    """The successor of a stamp: 0 and TOMBSTONE are never handed out."""
    s = (s + 1) & M32
    return 1 if s in (0, TOMBSTONE) else s


def older(x, cutoff, now):
    """x is older than cutoff, both seen from `now`, on ages modulo 2^32."""
    return ((now - x) & M32) > ((now - cutoff) & M32)


# the sweep words (sh_sweep, csrc/yy_tree.h): live entries counted by the running sweep, entries it evicted (both 0 between
# sweeps), live entries after the last sweep, entries evicted in all, the stamp recorded by the last sweep above the mark
SW_COUNT, SW_EVICTING, SW_LIVE, SW_EVICTED, SW_CUTOFF, SWEEP_WORDS = 0, 1, 2, 3, 4, 8


def sweep_arrays(claim, last_hit, stamp, cutoff, evicted_total, high_water_slots):
    """One sweep (yy_mcts_shared_evaluations_sweep) over whole arrays, vectorised: Table.sweep below, restated so that a table
    of 2^22 slots is swept in one numpy pass.  claim u64 [slots], last_hit u32 [slots]; stamp: the current one; cutoff: the
    sweep word (0: none yet); evicted_total: the running total before the sweep.
    Returns (the new claim array, {SW_LIVE, SW_EVICTED, SW_CUTOFF: the words after the sweep}, the evicted slots, ascending)."""
    claim = np.asarray(claim).view(np.uint64)
    last = np.asarray(last_hit).view(np.uint32)
    ins = (claim & np.uint64(M32)).astype(np.uint32)
    live = (ins != 0) & (ins != TOMBSTONE)
    n_live = int(np.count_nonzero(live))
    out, gone, new_cutoff = claim.copy(), np.empty(0, np.int64), int(cutoff)
    if n_live > high_water_slots:
        if cutoff:
            now, keep = np.uint32(stamp), np.uint32((int(stamp) - int(cutoff)) & M32)
            # ages modulo 2^32 (array arithmetic on uint32 wraps): older than the cutoff in BOTH words
            gone = np.flatnonzero(live & ((now - ins) > keep) & ((now - last) > keep))
            out[gone] = np.uint64(TOMBSTONE)
        new_cutoff = int(stamp)
    return out, {SW_LIVE: n_live - len(gone), SW_EVICTED: int(evicted_total) + len(gone), SW_CUTOFF: new_cutoff}, gone


# ---- what the device derives from a position's key words
def bb_hash(words):
    """bb_hash<NW> of csrc/yy_engine.hip in numpy uint64: the golden-ratio seed, then murmur3's 64-bit finaliser after every
    key word, black words first.  words: integer [..., 2 * NW] (black words, then white words: a row of the table's `keys`),
    NW = 1, 2 or 3; returns uint64 [...].
    There is no independent host oracle for it (the host tests only hold the array arithmetic against Python integers): its
    check against the device is tests/test_gpu_shared_table_state.py, where every live entry of a device table must sit under
    bb_hash(key) >> 32 inside the window that starts at tt_first(bb_hash(key))."""
    w = np.ascontiguousarray(words)
    w = w.view(np.uint64) if w.dtype == np.int64 else w.astype(np.uint64)
    assert w.shape[-1] in (2, 4, 6), w.shape
    shape, w = w.shape[:-1], w.reshape(-1, w.shape[-1])  # arrays, never numpy scalars: only array arithmetic wraps silently
    h = np.full(w.shape[0], 0x9E3779B97F4A7C15, np.uint64)
    s33 = np.uint64(33)
    for i in range(w.shape[-1]):
        h = h ^ w[..., i]
        h = h ^ (h >> s33)
        h = h * np.uint64(0xFF51AFD7ED558CCD)             # uint64 array products wrap
        h = h ^ (h >> s33)
        h = h * np.uint64(0xC4CEB9FE1A85EC53)
        h = h ^ (h >> s33)
    return h.reshape(shape)


def tt_first(h, slots):
    """The first slot of the probe window: the low 32 bits of the hash under the slot mask."""
    return ((np.asarray(h, np.uint64) & np.uint64(M32)) & np.uint64(slots - 1)).astype(np.int64)


def tt_window(h, slots):
    """The PROBES slots a position may sit in, in probe order: linear from tt_first, wrapping.  [..., PROBES]"""
    return (tt_first(h, slots)[..., None] + np.arange(PROBES)) & (slots - 1)


def tt_tag(h):
    """The claim word's tag: the high 32 bits of the hash."""
    return (np.asarray(h, np.uint64) >> np.uint64(32)).astype(np.int64)


# ---- crafted sweep states: what tests/test_shared_table_model_host.py sweeps with both restatements and
# tests/test_gpu_shared_table_state.py with the device's launches
def stamp_line(start, n):
    """n stamps in the order they are handed out, from `start` on: next_stamp, never a plain addition."""
    line = [int(start)]
    while len(line) < n:
        line.append(next_stamp(line[-1]))
    return line


CLOCKS = ("plain", "now-is-cutoff", "wrap", "no-cutoff")


def clock(name):
    """The stamps an entry's two words are drawn from, by class: dict(old: handed out before the cutoff, cutoff, mid: after the
    cutoff and before now (may be empty), now, word: the cutoff as the sweep word holds it).
    plain: cutoff 1000, now 1040.  now-is-cutoff: what the second of two sweeps back to back sees.  wrap: the cutoff handed out
    12 launches before the stamps wrap, now 9 launches after, old and mid stamps on either side.  no-cutoff: the plain stamps
    with the sweep word still 0 (no sweep has been above the mark yet)."""
    if name == "wrap":
        line = stamp_line(M32 - 40, 49)
        assert line[39] == M32 - 1 and line[40] == 1 and line[-1] == 9          # 0 and the tombstone were skipped
        ic = 40 - 12
    else:
        line = stamp_line(960, 41 if name == "now-is-cutoff" else 81)
        ic = 40
        assert line[ic] == 1000 and line[-1] == (1000 if name == "now-is-cutoff" else 1040)
    return dict(old=line[:ic], cutoff=line[ic], mid=line[ic + 1:-1], now=line[-1], word=0 if name == "no-cutoff" else line[ic])


def crafted_state(slots, clk, seed):
    """A table state for one sweep -> (claim u64 [slots], last_hit u32 [slots]).  Every slot is never used (claim 0), a
    tombstone, or live with its insert stamp and its last-hit stamp drawn INDEPENDENTLY from the classes {old, cutoff, mid,
    now} of clock `clk`; the sweep handles four slots a thread, so a quarter of the quads give their four slots one fate and a
    quarter four different ones (never used, tombstone, live and old in both words, live and current).  Tags are random 32-bit
    words, every seventh with bit 31 set, every eleventh 0.  The last-hit words of free slots hold noise."""
    assert slots % 4 == 0
    rng = np.random.default_rng(seed)
    kind = rng.choice(3, slots, p=[0.15, 0.15, 0.7])                      # 0 never used, 1 tombstone, 2 live
    ins_c, hit_c = rng.integers(0, 4, slots), rng.integers(0, 4, slots)  # 0 old, 1 cutoff, 2 mid, 3 now
    mode = np.repeat(rng.integers(0, 4, slots // 4), 4)                   # per quad; 0, 1: every slot on its own
    lead = np.repeat(np.arange(0, slots, 4), 4)
    one = mode == 2                                                       # one fate for the quad: its first slot's
    kind[one], ins_c[one], hit_c[one] = kind[lead[one]], ins_c[lead[one]], hit_c[lead[one]]
    four = mode == 3                                                      # four different fates, in a random order
    order = rng.permuted(np.tile(np.arange(4), (slots // 4, 1)), axis=1).reshape(-1)[four]
    kind[four] = np.array([0, 1, 2, 2])[order]
    ins_c[four], hit_c[four] = np.array([0, 0, 0, 3])[order], np.array([0, 0, 0, 2])[order]

    def stamps(cls):
        old, mid = np.array(clk["old"], np.uint32), np.array(clk["mid"] or [clk["cutoff"]], np.uint32)
        return np.choose(cls, [old[rng.integers(0, len(old), slots)], np.uint32(clk["cutoff"]),
                               mid[rng.integers(0, len(mid), slots)], np.uint32(clk["now"])]).astype(np.uint32)

    tag = rng.integers(0, 1 << 32, slots, dtype=np.uint64)
    tag[::7] |= np.uint64(1 << 31)
    tag[3::11] = 0
    claim = np.where(kind == 2, (tag << np.uint64(32)) | stamps(ins_c).astype(np.uint64), np.uint64(0))
    claim[kind == 1] = np.uint64(TOMBSTONE)
    last_hit = np.where(kind == 2, stamps(hit_c), rng.integers(0, 1 << 32, slots, dtype=np.uint64).astype(np.uint32))
    return claim.astype(np.uint64), last_hit.astype(np.uint32)


class Table:
    def __init__(self, slots, stamp=1):
        assert slots >= 8 and slots & (slots - 1) == 0
        self.slots = slots
        self.claim = np.zeros(slots, np.uint64)          # tag << 32 | insert stamp
        self.last_hit = np.zeros(slots, np.uint32)
        self.key = [None] * slots
        self.stamp = stamp
        self.cutoff = 0                                   # the stamp recorded by the last sweep above the mark; 0: none yet
        self.c = dict(hits=0, inserts=0, dropped=0, duplicates=0, evicted=0, live=0)

    # ---- what the device derives from a position
    @staticmethod
    def tag(h):
        return (h >> 32) & M32

    def window(self, h):
        return [((h & M32) + i) & (self.slots - 1) for i in range(PROBES)]

    def stamp_of(self, at):
        return int(self.claim[at]) & M32

    def is_free(self, at):
        return self.stamp_of(at) in (0, TOMBSTONE)

    def live_slots(self):
        return [at for at in range(self.slots) if not self.is_free(at)]

    # ---- a tree-step launch
    def begin_launch(self):
        self.stamp = next_stamp(self.stamp)

    def lookup(self, key, h):
        """leaf_lookup: the slot that serves `key`, or None.  Entries of this launch and tombstones are passed over, a
        never-used slot ends the probe; a hit leaves this launch's stamp in the slot's last-hit word."""
        for at in self.window(h):
            s = self.stamp_of(at)
            if s == 0:
                return None
            if s == self.stamp or s == TOMBSTONE:
                continue
            if self.key[at] == key:
                self.last_hit[at] = self.stamp
                self.c["hits"] += 1
                return at
        return None

    def insert(self, key, h):
        """shared_store: 'inserted', 'duplicate' or 'dropped'."""
        mine = (self.tag(h) << 32) | self.stamp
        for at in self.window(h):
            if self.is_free(at):
                self.claim[at] = np.uint64(mine)
                self.last_hit[at] = self.stamp
                self.key[at] = key
                self.c["inserts"] += 1
                return "inserted"
            if int(self.claim[at]) == mine:
                self.c["duplicates"] += 1
                return "duplicate"
        self.c["dropped"] += 1
        return "dropped"

    # ---- between two launches
    def sweep(self, high_water_slots):
        """yy_mcts_shared_evaluations_sweep: returns the slots evicted."""
        live = self.live_slots()
        gone = []
        if len(live) > high_water_slots:
            if self.cutoff:
                gone = [at for at in live if older(self.stamp_of(at), self.cutoff, self.stamp)
                        and older(int(self.last_hit[at]), self.cutoff, self.stamp)]
                for at in gone:
                    self.claim[at] = np.uint64(TOMBSTONE)
            self.cutoff = self.stamp
        self.c["live"] = len(live) - len(gone)
        self.c["evicted"] += len(gone)
        return gone
