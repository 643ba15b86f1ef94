"""The per-game evaluation cache on the device (csrc/yy_engine.hip leaf_lookup / cache_store / cache_of, csrc/yy_tree.h
root_setup, yy_mcts_create's sizing, yy_mcts_cache_clear) against tests/eval_cache_model.py, bit for bit.

Every configuration of tests/eval_cache_cases.py is searched twice with the hash evaluator: by a base context, whose flagged
rows are exactly the leaves the cached context consults its tables with (option-off; reuse_pass_value alone for a cached
context that has it), and by the cached context.  The evaluator callable records needs_eval at every call, in the base run also
the position of every row.  The two searches are the same search (asserted), so call i of both concerns the same leaf of every
game: the base run's flagged positions, replayed through the model game by game, predict every needs_eval bit of the cached
run, both counters, and -- through cache_slots -- the bytes the cache adds to the context.  The coverage conditions of the host
test are asserted again on what was recorded, so a configuration that exercises nothing fails."""
import numpy as np
import pytest

import eval_cache_cases as K
from eval_cache_model import BOOK, HIT, MISS, cache_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    import yinyang_game_alphazero_amd as pkg
    return pkg


def _trace(pkg, name, fused):
    import torch
    E = pkg.engine
    cfg = K.CONFIGS[name]
    (R, C), G, sims = cfg["shape"], cfg["G"], cfg["sims"]
    kw = dict(aliased=bool(cfg.get("aliased")), nodes_per_game=cfg.get("nodes_per_game", 0))
    base = E.BatchedMCTS(G, R, C, sims, **kw, **cfg["base"])
    cached = E.BatchedMCTS(G, R, C, sims, **kw, **cfg["flags"])
    book = None
    if cfg.get("book_stones"):
        from hash_eval import hash_eval_torch
        book = E.OpeningBook(R, C, lambda p: hash_eval_torch(p, K.PBITS, K.VBITS), cfg["book_stones"])
        assert book.stored == book.n and book.max_stones == cfg["book_stones"]
        stored = {tuple(r) for r in book.table_keys[book.meta != 0].cpu().numpy().astype(np.uint64).tolist()}
        assert stored == K.book_positions(R, C, cfg["book_stones"])          # the model is given what the device's book holds
        cached.set_book(book)
        book = stored
    rec_b, rec_c = K.Recorder(base, True), K.Recorder(cached, False)
    games = [[] for _ in range(G)]      # per game and search: (root stones, keys, stones) of its lookups
    calls, got = [], []                 # per search: per game the calls that looked something up; the cached needs_eval [sims, G]

    def search(s, boards, players):
        if s in cfg.get("clear_before", ()):
            cached.clear_evaluation_cache()
        out = []
        for m, rec in ((base, rec_b), (cached, rec_c)):         # a fresh upload each: the aliased search plays on the caller's boards
            c = m.search(torch.from_numpy(boards).cuda(), torch.from_numpy(players).cuda(), rec, sims, fused=fused)
            out.append((c, *m.root_stats(), m.root_policy()))
        for a, b in zip(*out):
            assert torch.equal(a, b), (name, s)                 # the same search: call i concerns the same leaf in both runs
        ne, pos = rec_b.take()
        assert ne.shape == (sims, G)
        per_game = [K.game_lookups(ne, pos, g) for g in range(G)]
        calls.append([p[0] for p in per_game])
        for g, p in enumerate(per_game):
            games[g].append((int(np.count_nonzero(boards[g])), p[1], p[2]))
        got.append(rec_c.take()[0])
        return out[0][0].cpu().numpy()

    K.run_config(cfg, search)
    status = cached.status(), base.status()
    extra = cached.memory_bytes() - base.memory_bytes()
    base.close()
    cached.close()

    res = [K.model_replay(name, s, book=book) for s in games]
    bad = []
    for s in range(cfg["searches"]):
        for g in range(G):
            want = K.expected_needs_eval(sims, calls[s][g], res[g][0][s])
            if not np.array_equal(want, got[s][:, g]):
                bad.append((s, g, int(np.flatnonzero(want != got[s][:, g])[0])))
    outcomes = np.concatenate([o for r in res for o in r[0]])
    c = K.sum_counts(r[1] for r in res)
    print("%s %s: %d lookups compared, %d hits, %d book, %d misses; %s" % (
        name, "fused" if fused else "split", len(outcomes), int((outcomes == HIT).sum()), int((outcomes == BOOK).sum()),
        int((outcomes == MISS).sum()), c))
    assert not bad, (name, "search, game, first differing call", bad[:8], len(bad))
    assert status[0]["transposition_hits"] == int((outcomes != MISS).sum()), (status[0], c)
    assert status[0]["evals"] == int((outcomes == MISS).sum()), (status[0], c)
    assert status[1]["evals"] == len(outcomes) and status[1]["transposition_hits"] == 0
    assert extra == cache_bytes(K.slots_of(cfg), G, R * C), (extra, K.slots_of(cfg))
    assert not K.coverage_shortfalls(name, c)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "split"])
@pytest.mark.parametrize("name", ["8x8-tt", "8x8-pass+tt"])
def test_cache_trace_8x8(pkg, name, fused):
    """One bitboard word, 512 slots, two searches of a context without keep (every search its own epoch: the second finds
    nothing of the first and replaces its entries first); mid-game batches with pass roots and finished games; both steppings."""
    _trace(pkg, name, fused)


@pytest.mark.parametrize("name", ["9x12-tt", "12x12-tt", "12x16-tt"])
def test_cache_trace_two_and_three_words(pkg, name):
    _trace(pkg, name, True)


@pytest.mark.parametrize("name", ["8x8-keep", "12x12-keep"])
def test_cache_trace_keep_across_moves_overflowing(pkg, name):
    """All three flags, 128 slots a game, searches of advancing positions with restarts from the empty board (the epoch advances,
    hits on older-epoch entries follow), a clear between two searches, and a stretch that fills every window with live entries:
    every store class, both hit classes, one word and three."""
    _trace(pkg, name, True)


def test_cache_trace_book_before_cache(pkg):
    """A 3-stone book on a keep context: a leaf the book serves is neither a miss nor stored, and takes no slot."""
    _trace(pkg, "6x6-book", True)


def test_cache_trace_aliased_boards(pkg):
    """The key is the position the leaf really has on the shared board."""
    _trace(pkg, "8x8-aliased-tt", True)
