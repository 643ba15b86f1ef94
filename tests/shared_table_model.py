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


class Table:
    def __init__(self, slots, stamp=1):
        assert slots >= 8 and slots & (slots - 1) == 0
        self.slots = slots
        self.claim = np.zeros(slots, np.uint64)          # tag << 32 | insert stamp
        self.last_hit = np.zeros(slots, np.uint32)
        self.key = [None] * slots
        self.stamp = stamp
        self.cutoff = 0                                   # the stamp recorded by the last sweep that evicted; 0: none yet
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
