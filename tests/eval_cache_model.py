"""A numpy / plain-Python restatement of ONE game's evaluation cache (YY_FLAG_REUSE_TRANSPOSITIONS / YY_FLAG_KEEP_EVALUATIONS,
include/yy_engine.h; csrc/yy_engine.hip leaf_lookup, cache_store, cache_of, yy_mcts_create, yy_mcts_cache_clear; csrc/yy_tree.h
root_setup), one lookup and one store at a time and in program order.  One wavefront holds one game and one leaf is pending at
K = 1: a lookup happens in a selection and its store in the expansion that follows, nothing crosses between games, so the
restatement is exact: tests/test_gpu_eval_cache_trace.py holds every needs_eval bit of the device against it.

A position is its key words (black words, then white words: 2 * NW integers) and its stone count.  A slot's metadata word is
epoch << 8 | stones, 0 = never used; the hash (bb_hash, tests/shared_table_model.py) only picks the probe window.

What is NOT covered: the 24-bit epoch wrap (begin_search restates it, but a game reaches it after 16.7 M searches of one slot and
the engine has no hook to set an epoch, so no test drives the device there), leaves_per_step > 1 (no cache) and the captured
free-running step (no per-step needs_eval on the host).

MUTANTS are deliberate faults, selected by keyword and used by tests/test_eval_cache_model_host.py only: each must change the
predicted hit / miss sequence on the inputs of the GPU test, which proves that the GPU comparison would fail for that fault."""
import numpy as np

from shared_table_model import PROBES, bb_hash, tt_first, tt_window

EPOCH_MASK = 0xFFFFFF
MISS, HIT, BOOK = 0, 1, 2
STORE_CLASSES = ("never_used", "other_epoch", "cannot_recur", "fallback_first")
HIT_CLASSES = ("hit_current", "hit_older")
MUTANTS = ("probes7",              # a probe window of 7
           "no_stop",              # the probe does not end at a never-used slot
           "store_first",          # a store always takes the window's first slot
           "stones_dropped",       # no "cannot recur" rule
           "stones_lt",            # the rule with < instead of <=
           "epoch_every_search",   # the epoch advances on every search under keep
           "epoch_stuck",          # the epoch never advances at an empty root
           "clear_noop",           # clear() leaves the entries findable
           "hash_drops_last")      # the hash does not depend on the last white word


def cache_slots(node_cap, G, A):
    """Slots per game (yy_mcts_create): the power of two >= 4 * node_cap, at least 64, halved while the policy rows of all G
    games exceed 48 GiB and the cache still has more than 2 * node_cap slots.  node_cap = nodes_per_game, or max_sims + 2."""
    cap = 64
    while cap < 4 * node_cap:
        cap *= 2
    while cap > 2 * node_cap and float(G) * float(cap) * A * 4.0 > 48.0 * 1073741824.0:
        cap //= 2
    return cap


def cache_bytes(slots, G, A):
    """What the cache adds to a context's allocation: metadata, key, value and policy row of every slot of every game."""
    nw = (A + 63) // 64
    return G * slots * (4 + 16 * nw + 4 + 4 * A)


def pack_keys(boards):
    """int8 [n, R, C] boards (1 black, -1 white) -> uint64 [n, 2 * NW] key words: cell r * C + c is bit (cell & 63) of word
    cell >> 6, black words first."""
    b = np.asarray(boards, np.int8)
    n, A = b.shape[0], b.shape[1] * b.shape[2]
    nw = (A + 63) // 64
    flat = np.zeros((n, nw * 64), np.uint64)
    flat[:, :A] = b.reshape(n, A) == 1
    w = np.uint64(1) << np.arange(64, dtype=np.uint64)
    out = np.zeros((n, 2 * nw), np.uint64)
    out[:, :nw] = (flat.reshape(n, nw, 64) * w).sum(2, dtype=np.uint64)
    flat[:, :A] = b.reshape(n, A) == -1
    out[:, nw:] = (flat.reshape(n, nw, 64) * w).sum(2, dtype=np.uint64)
    return out


def key_hashes(keys, mutant=None):
    """bb_hash of uint64 [n, 2 * NW] key words; the hash mutant blanks the last white word first."""
    k = np.ascontiguousarray(keys, np.uint64).reshape(-1, np.shape(keys)[-1])
    if mutant == "hash_drops_last":
        k = k.copy()
        k[:, -1] = 0
    return bb_hash(k) if len(k) else np.zeros(0, np.uint64)


class EvalCache:
    """One game's cache.  book: a set of key tuples served before the cache for positions of at most book_stones stones."""

    def __init__(self, slots, keep, mutant=None, book=None, book_stones=0):
        assert slots >= 64 and slots & (slots - 1) == 0 and (mutant is None or mutant in MUTANTS)
        self.slots, self.keep, self.mutant = slots, bool(keep), mutant
        self.book, self.book_stones = book, book_stones
        self.meta = [0] * slots
        self.key = [None] * slots          # a cleared slot keeps its key words, as the device's arrays do
        self.epoch, self.root_stones = 0, 0
        self.pending = None                # (slot, store class) of the last miss
        self.c = dict.fromkeys(STORE_CLASSES + HIT_CLASSES + ("lookups", "book", "wraps"), 0)

    def begin_search(self, root_stones):
        """root_setup: without keep every search is a new epoch; with keep the epoch advances when the root has no stones, or
        while it is still 0.  24 bits, never 0."""
        ep = self.epoch
        advance = (not self.keep) or root_stones == 0 or ep == 0
        if self.mutant == "epoch_every_search":
            advance = True
        if self.mutant == "epoch_stuck":
            advance = (not self.keep) or ep == 0
        if advance:
            ep = (ep + 1) & EPOCH_MASK
        if ep == 0:
            ep = 1
        self.epoch, self.root_stones = ep, int(root_stones)

    def window(self, h):
        n = PROBES - 1 if self.mutant == "probes7" else PROBES
        return [int(x) for x in tt_window(np.uint64(h), self.slots)[:n]]

    def lookup(self, key, stones, h=None, window=None):
        """leaf_lookup's cache part -> (hit, slot): the slot that serves the position, or the slot its evaluation will go into.
        A hit refreshes nothing."""
        key = tuple(int(x) for x in key)
        if window is None:
            window = self.window(key_hashes(np.array([key], np.uint64), self.mutant)[0] if h is None else h)
        self.c["lookups"] += 1
        self.c["wraps"] += window[-1] < window[0]
        slot, cls, ep = -1, None, self.epoch
        for at in window:
            m = self.meta[at]
            if m == 0 and self.mutant != "no_stop":                    # never used: the position is not in the table
                if slot < 0:
                    slot, cls = at, "never_used"
                break
            cur = (m >> 8) == ep
            if (cur or self.keep) and self.key[at] == key:
                self.c["hit_current" if cur else "hit_older"] += 1
                self.pending = None
                return True, at
            if slot < 0:
                if self.mutant == "stones_dropped":
                    gone = False
                elif self.mutant == "stones_lt":
                    gone = (m & 0xFF) < self.root_stones
                else:
                    gone = (m & 0xFF) <= self.root_stones
                if not cur or gone:
                    slot, cls = at, "never_used" if m == 0 else "cannot_recur" if cur else "other_epoch"
        if slot < 0:
            slot, cls = window[0], "fallback_first"                    # every probed entry is live: replace the first
        if self.mutant == "store_first":
            slot = window[0]
        self.pending = (slot, cls)
        return False, slot

    def store(self, key, stones):
        """cache_store: the fresh evaluation goes into the slot the lookup chose."""
        slot, cls = self.pending
        self.pending = None
        self.c[cls] += 1
        self.key[slot] = tuple(int(x) for x in key)
        self.meta[slot] = (self.epoch << 8) | (int(stones) & 0xFF)

    def clear(self):
        """yy_mcts_cache_clear: the metadata is zeroed, the epoch stays."""
        if self.mutant != "clear_noop":
            self.meta = [0] * self.slots

    def leaf(self, key, stones, h=None, window=None):
        """One leaf that consults the tables, in the device's order: the book (the leaf is then neither looked up in the cache
        nor stored), else the cache, and on a miss the store of the evaluation.  -> BOOK, HIT or MISS."""
        key = tuple(int(x) for x in key)
        if self.book is not None and stones <= self.book_stones and key in self.book:
            self.c["book"] += 1
            return BOOK
        hit, _ = self.lookup(key, stones, h, window)
        if hit:
            return HIT
        self.store(key, stones)
        return MISS


def replay(searches, slots, keep, mutant=None, book=None, book_stones=0, clear_before=()):
    """One game.  searches: per search (root_stones, keys uint64 [n, 2 * NW], stones int [n]): the leaves that consult the cache,
    in order (the root call looks nothing up and stores nothing).  clear_before: the searches in front of which the cache is
    cleared.  -> (per search a uint8 [n] of MISS / HIT / BOOK, the classification counts)."""
    t = EvalCache(slots, keep, mutant, book, book_stones)
    probes = PROBES - 1 if mutant == "probes7" else PROBES
    out = []
    for s, (root_stones, keys, stones) in enumerate(searches):
        if s in clear_before:
            t.clear()
        t.begin_search(root_stones)
        keys = np.asarray(keys, np.uint64).reshape(len(stones), np.shape(keys)[-1])
        wins = tt_window(key_hashes(keys, mutant), slots)[:, :probes].tolist() if len(stones) else []
        res = np.zeros(len(stones), np.uint8)
        for i, (k, n, w) in enumerate(zip(keys.tolist(), stones, wins)):
            res[i] = t.leaf(k, int(n), window=w)
        out.append(res)
    return out, dict(t.c)


def first_slot(key, slots):
    """The first slot of a position's probe window (hand-built windows of the host test)."""
    return int(tt_first(key_hashes(np.array([key], np.uint64))[0], slots))
