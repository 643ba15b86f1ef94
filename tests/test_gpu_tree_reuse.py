"""Tree reuse across moves on the device (include/yy_engine.h yy_mcts_advance, engine.BatchedMCTS.advance), tolerance 0:
integers, bits of float32, the root's float64 sum.

Every case of tests/tree_reuse_cases.py -- G = 8 games on 3x3, 4x4, 1x6, 7x1, 5x7, 2x9 (one bitboard word), 9x12 (two), 12x16
(three, more than 64 children per node), plus two longer ones -- is played on ONE context, ply by ply, with the hash evaluator,
and compared with its replay on tests/tree_reuse_model.py through the public outputs only: root_counts(with_children=True),
root_stats, the needs_eval row and the planes of every step, the status() counters, and kept_visits.  max_sims equals the
budget, so the arenas (max_sims + 2 nodes) run to their caps with a kept tree and status() must stay clean.  The CPU test
tests/test_tree_reuse_model.py checks that these cases keep trees, top them up, fall back to fresh roots, advance twice, reach
terminal children and noise kept roots.  Every test here needs yy_mcts_advance."""
import functools

import numpy as np
import pytest

import tree_reuse_cases as Cs
from hash_eval import hash_eval_torch, planes_to_boards

pytestmark = pytest.mark.gpu
COUNTERS = ("evals", "levels", "children_scanned", "children_created", "terminal_revisits", "nodes")


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    import yinyang_game_alphazero_amd as p
    return p


class Tracer:
    """The hash evaluator on the device; every call after the root call keeps the needs_eval flags and the planes of the step.
    bad_policy: the root call returns another position's row (rolled by one action), which a kept root must not read."""

    def __init__(self, mc, pbits, bad_policy):
        self.mc, self.pbits, self.bad, self.calls, self.flags, self.planes = mc, pbits, bad_policy, 0, [], []

    def __call__(self, planes):
        import torch
        root = self.calls == 0
        if not root:
            self.flags.append(self.mc.needs_eval.clone())
            self.planes.append(planes.clone())
        self.calls += 1
        p, v = hash_eval_torch(planes, self.pbits, Cs.VB)
        return (torch.roll(p, 1, dims=1).contiguous() if root and self.bad else p), v


def root_obs(mc):
    counts, cw, cp = (t.cpu().numpy() for t in mc.root_counts(with_children=True))
    visits, wsum = (t.cpu().numpy() for t in mc.root_stats())
    return counts, cw, cp, visits, wsum


@functools.lru_cache(maxsize=None)
def device_run(name, **kw):
    """Case `name` on one context (keywords: BatchedMCTS's, and book=N stones) -> per ply dict(root=..., flags [steps, G], boards
    [steps, G, R, C], counters, kept1, after1, kept2, after); raises if status() is not clean."""
    import torch
    import yinyang_game_alphazero_amd as pkg
    R, C, sims, G, _, _, pb = Cs.CASES[name]
    kw = dict(kw)
    book = kw.pop("book", 0)
    mc = pkg.engine.BatchedMCTS(G, R, C, sims, **kw)
    if book:
        mc.set_book(pkg.engine.OpeningBook(R, C, lambda planes: hash_eval_torch(planes, pb, Cs.VB), book))
    out = []
    try:
        for p in Cs.replay(name):
            tr = Tracer(mc, pb, p.bad_policy)
            mc.reset_counters()
            mc.search(torch.from_numpy(p.boards).cuda(), torch.from_numpy(p.players).cuda(), tr,
                      sims if p.budgets is None else p.budgets, noise=torch.from_numpy(p.noise).cuda() if p.noise.any() else None,
                      active=torch.from_numpy(p.active).cuda())
            o = dict(root=root_obs(mc), counters=mc.status())
            o["flags"] = torch.stack(tr.flags).cpu().numpy() if tr.flags else np.zeros((0, G), np.uint8)
            o["boards"] = (planes_to_boards(torch.stack(tr.planes).cpu().numpy().reshape(-1, 5, R, C)).reshape(-1, G, R, C)
                           if tr.planes else np.zeros((0, G, R, C), np.int8))
            o["kept1"] = mc.advance(torch.from_numpy(p.actions).cuda()).cpu().numpy()
            o["after1"] = root_obs(mc)
            if p.double:
                o["kept2"] = mc.advance(torch.from_numpy(p.actions2).cuda()).cpu().numpy()
            o["after"] = root_obs(mc)
            mc.status()
            out.append(o)
    finally:
        mc.close()
    return out


def check_roots(name, got, counters=True):
    """The statistics of every searched root, the kept visits and the roots the advances leave equal the model's."""
    for t, (p, o) in enumerate(zip(Cs.replay(name), got)):
        counts, cw, cp, visits, wsum = o["root"]
        for g, r in enumerate(p.results):
            if r is None:
                assert not counts[g].any(), (t, g)
                continue
            where = (name, t, g, "kept" if p.used_kept[g] else "fresh")
            assert np.array_equal(counts[g], r.counts), where
            assert np.array_equal(cw[g].view(np.uint32), r.child_w.view(np.uint32)), where
            assert np.array_equal(cp[g].view(np.uint32), r.child_p.view(np.uint32)), where
            assert (int(visits[g]), float(wsum[g])) == (r.root_visits, float(r.root_w)), where
        assert np.array_equal(o["kept1"], p.kept1), (name, t, o["kept1"], p.kept1)
        if p.double:
            assert np.array_equal(o["kept2"], p.kept2), (name, t, o["kept2"], p.kept2)
        counts, cw, cp, visits, wsum = o["after"]
        for g, (mcnt, mw, mp, mn, mwsum) in enumerate(p.after):
            where = (name, t, g, "after the advance")
            assert np.array_equal(counts[g], mcnt), where
            assert np.array_equal(cw[g].view(np.uint32), mw.view(np.uint32)), where
            assert np.array_equal(cp[g].view(np.uint32), mp.view(np.uint32)), where
            assert (int(visits[g]), float(wsum[g])) == (mn, float(mwsum)), where
        if counters:
            for k in COUNTERS:
                assert o["counters"][k] == sum(getattr(r, k) for r in p.results if r is not None), (name, t, k)


@pytest.mark.parametrize("name", list(Cs.CASES))
def test_every_ply_equals_the_model(name):
    """Advance by the most visited, a once-visited, an unvisited and a terminal child, by -1 and by an action off the board; then
    budget = kept visits (nothing is selected), top-ups with scalar and per-game budgets, two advances in a row, a board other
    than the kept one, inactive games and budgets below the kept visits -- all in one batch per ply."""
    got = device_run(name)
    check_roots(name, got)
    for t, (p, o) in enumerate(zip(Cs.replay(name), got)):
        steps = o["flags"].shape[0]
        assert steps == p.bound, (name, t)
        for g, r in enumerate(p.results):
            needs = np.zeros(steps, np.uint8)
            if r is not None:
                needs[:len(r.needs)] = r.needs
            assert np.array_equal(o["flags"][:, g], needs), (name, t, g)
            if r is not None:                                     # the evaluated positions, in order, are the model's trace
                rows = o["boards"][np.flatnonzero(needs), g]
                assert len(rows) == len(r.trace) and all(np.array_equal(a, b) for a, b in zip(rows, r.trace)), (name, t, g)


def test_a_kept_root_that_holds_its_budget_selects_nothing():
    name = "5x7"
    p, o = Cs.replay(name)[1], device_run(name)[1]                # ply 1: budget = kept visits
    full = [g for g in range(8) if p.used_kept[g] and p.kept_in[g] >= 2]
    assert full
    for g in full:
        assert not o["flags"][:, g].any() and o["root"][3][g] == p.kept_in[g] == o["root"][0][g].sum() + 1


def test_noise_goes_into_the_stored_priors_of_a_kept_root():
    """Ply 2 of the per-board cases hands every root a foreign policy row and noise: the kept roots' priors are
    f32(f64(f32(0.75 * stored prior)) + 0.25 * noise), and a zero noise row leaves them untouched."""
    seen = set()
    for name in ("4x4", "5x7", "12x16"):
        before, now, p = device_run(name)[1]["after"], device_run(name)[2]["root"], Cs.replay(name)[2]
        for g in range(8):
            if not p.used_kept[g]:
                continue
            legal = before[0][g] + (before[2][g] != 0) > 0
            stored = before[2][g]
            if p.noise[g].any():
                want = (np.float32(0.75) * stored).astype(np.float32).astype(np.float64) + 0.25 * p.noise[g]
                assert np.array_equal(now[2][g][legal], want.astype(np.float32)[legal]), (name, g)
                seen.add("noised")
            else:
                assert np.array_equal(now[2][g], stored), (name, g)
                seen.add("zero row")
    assert seen == {"noised", "zero row"}


@pytest.mark.parametrize("name,book", [("4x4", 0), ("5x7", 0), ("9x12", 0), ("5x5-long", 0), ("4x4", 7), ("4x4-long", 6)])
def test_evaluation_reuse_and_the_book_leave_the_statistics_alone(name, book):
    """YY_FLAG_REUSE_PASS_VALUE | REUSE_TRANSPOSITIONS | KEEP_EVALUATIONS, without and with a book of the positions of up to
    `book` stones: the same counts, priors and value sums as with the flags off, from fewer evaluator rows."""
    kw = dict(reuse_pass_value=True, reuse_transpositions=True, keep_evaluations=True)
    if book:
        kw["book"] = book
    got = device_run(name, **kw)
    check_roots(name, got, counters=False)
    plain = device_run(name)
    assert sum(o["counters"]["evals"] for o in got) < sum(o["counters"]["evals"] for o in plain)


def test_a_board_other_than_the_kept_one_is_searched_afresh(pkg):
    import torch
    name = "5x7"
    R, C, sims, G, _, _, pb = Cs.CASES[name]
    p0, p1 = Cs.replay(name)[0], Cs.replay(name)[3]              # two unrelated sets of positions
    ev = lambda planes: hash_eval_torch(planes, pb, Cs.VB)

    def run(advance):
        mc = pkg.engine.BatchedMCTS(G, R, C, sims)
        mc.search(torch.from_numpy(p0.boards).cuda(), torch.from_numpy(p0.players).cuda(), ev, sims)
        kept = mc.advance(torch.from_numpy(p0.actions).cuda()).cpu().numpy() if advance else None
        mc.reset_counters()
        mc.search(torch.from_numpy(p1.boards).cuda(), torch.from_numpy(p1.players).cuda(), ev, sims)
        out = root_obs(mc), mc.status()
        mc.close()
        return out, kept

    (a, ca), kept = run(True)
    (b, cb), _ = run(False)
    assert (kept >= 2).sum() >= 3
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and ca == cb


def test_refusals_launch_nothing(pkg):
    import torch
    R, C, sims, G = 4, 4, 12, 4
    boards, players = torch.zeros((G, R, C), dtype=torch.int8).cuda(), torch.ones(G, dtype=torch.int8).cuda()
    ev = lambda planes: hash_eval_torch(planes, 10, Cs.VB)
    act = torch.zeros(G, dtype=torch.int32).cuda()
    for kw in (dict(aliased=True), dict(leaves_per_step=4)):
        mc = pkg.engine.BatchedMCTS(G, R, C, sims, **kw)
        mc.search(boards.clone(), players, lambda pl: hash_eval_torch(pl, 10, Cs.VB), sims)
        before, size = root_obs(mc), mc.memory_bytes()
        with pytest.raises(pkg._lib.YYError) as e:
            mc.advance(act)
        assert e.value.code == -2                                  # YY_E_UNSUPPORTED
        assert all(np.array_equal(x, y) for x, y in zip(before, root_obs(mc))) and mc.memory_bytes() == size
        mc.close()
    mc = pkg.engine.BatchedMCTS(G, R, C, sims)
    mc.begin(boards, players)
    with pytest.raises(pkg._lib.YYError) as e:                     # root expansion pending
        mc.advance(act)
    assert e.value.code == -5
    mc.expand_root(ev(mc.planes)[0])
    mc.select()
    with pytest.raises(pkg._lib.YYError) as e:                     # select pending
        mc.advance(act)
    assert e.value.code == -5                                      # YY_E_STATE
    for _ in range(sims - 1):
        mc.step(*ev(mc.planes))
    mc.expand_backup(*ev(mc.planes))                               # the refused calls disturbed nothing: the search is the usual one
    want = pkg.engine.BatchedMCTS(G, R, C, sims)
    assert np.array_equal(mc.root_counts().cpu().numpy(), want.search(boards, players, ev, sims).cpu().numpy())
    size = mc.memory_bytes()
    assert (mc.advance(mc.root_counts().argmax(1).to(torch.int32)).cpu().numpy() >= 1).all()
    assert mc.memory_bytes() == size + 4 * G * (sims + 2)          # the remap array, int32 [G, node_cap], from the first advance on
    mc.status()
    mc.close()
    want.close()


# ------------------------------------------------------------------ engine level
SIMS, SLOTS, SEED = 24, 8, 5


def hash_evaluator(planes, **kw):
    return hash_eval_torch(planes, 10, Cs.VB)


def engine_games(pkg, R, C, **kw):
    eng = pkg.SelfPlayLanes(pkg.YinYangGame(R, C), hash_evaluator, num_simulations=SIMS, concurrent_games=SLOTS, lanes=2, seed=SEED,
                            reuse_pass_value=False, reuse_transpositions=False, keep_evaluations=False, **kw)
    ex = {k: v.cpu().numpy() for k, v in eng.run(SLOTS).items()}
    eng.ctx.status()
    eng.close()
    return ex


def loop_games(pkg, R, C, tree_reuse, fast=None, p_full=1.0):
    """SelfPlayEngine's move, written out over BatchedMCTS.search + advance with the engine's own draws; every game in its own
    slot of one context -> {game id: [(state, pi)] per recorded ply}, and the kept visits seen."""
    import torch
    E = pkg.engine
    G, A, dev = SLOTS, R * C, torch.device("cuda")
    mc = E.BatchedMCTS(G, R, C, SIMS)
    boards, players = torch.zeros((G, R, C), dtype=torch.int8, device=dev), torch.ones(G, dtype=torch.int8, device=dev)
    ply, gid = torch.zeros(G, dtype=torch.int32, device=dev), torch.arange(G, dtype=torch.int64, device=dev)
    alive, passes = torch.ones(G, dtype=torch.bool, device=dev), None
    games, kept_seen = {g: [] for g in range(G)}, []
    for _ in range(4 * A):
        if not bool(alive.any()):
            break
        pending, searching = alive.clone(), torch.zeros(G, dtype=torch.bool, device=dev)
        passes = torch.zeros(G, dtype=torch.int32, device=dev)
        for _ in range(2):
            has = E.valid_mask(boards, players).bool().any(1)
            go = pending & has
            searching |= go
            pending &= ~go
            nomove = pending & ~has
            passes += nomove.to(torch.int32)
            over = nomove & (passes >= 2)
            alive &= ~over
            pending &= ~over
            players = torch.where(nomove & ~over, -players, players).contiguous()
        searching &= alive
        mask, s_u8 = E.valid_mask(boards, players), searching.to(torch.uint8)
        noise = E.root_noise(SEED, gid, ply, (searching & (ply == 0)).to(torch.uint8), mask, 0.3)
        record = searching
        if fast is None:
            mc.search(boards, players, hash_evaluator, SIMS, noise=noise, active=s_u8)
        else:
            budgets, is_full = E.draw_budgets(SEED, gid, ply, s_u8, p_full, SIMS, fast)
            mc.search(boards, players, hash_evaluator, budgets, noise=noise, active=s_u8, num_sims_bound=SIMS)
            record = searching & is_full.bool()
        pi = mc.root_policy()
        for g in np.flatnonzero(record.cpu().numpy()):
            games[int(g)].append((boards[g].cpu().numpy().copy(), pi[g].to(torch.float32).cpu().numpy()))
        action = E.sample_actions(SEED, gid, ply, s_u8, pi, mask, 10)
        old = players.clone()
        E.step_(boards, players, action)
        players = torch.where(searching, players, old).contiguous()
        ply += searching.to(torch.int32)
        done = searching & (E.game_ended(boards, players) != 0)
        alive &= ~done
        if tree_reuse:
            kept_seen.append(mc.advance(torch.where(done | ~searching, torch.full_like(action, -1), action)).cpu().numpy())
    mc.status()
    mc.close()
    return games, kept_seen


def assert_games_equal(ex, games):
    for g, rows in games.items():
        sel = np.flatnonzero(ex["game_id"] == g)
        sel = sel[np.argsort(ex["ply"][sel], kind="stable")]
        assert len(sel) == len(rows) > 0, g
        for i, (state, pi) in zip(sel, rows):
            assert np.array_equal(ex["states"][i], state) and np.array_equal(ex["policies"][i], pi), (g, i)


@pytest.mark.parametrize("R,C", [(4, 4), (6, 6)])
def test_the_engine_plays_the_games_of_the_written_out_loop(pkg, R, C):
    games, kept = loop_games(pkg, R, C, True)
    assert sum(int((k >= 2).sum()) for k in kept) >= SLOTS                                          # trees were kept at all
    on = engine_games(pkg, R, C, tree_reuse=True)
    assert_games_equal(on, games)
    off = engine_games(pkg, R, C)                                  # default off: today's transcripts
    assert_games_equal(off, loop_games(pkg, R, C, False)[0])
    assert_games_equal(engine_games(pkg, R, C, tree_reuse=False), loop_games(pkg, R, C, False)[0])
    assert not all(np.array_equal(a, b) for a, b in zip(on["policies"], off["policies"]))


def test_tree_reuse_with_the_playout_cap_and_a_single_engine(pkg):
    games, kept = loop_games(pkg, 4, 4, True, fast=6, p_full=0.5)
    eng = pkg.SelfPlayEngine(pkg.YinYangGame(4, 4), hash_evaluator, num_simulations=SIMS, concurrent_games=SLOTS, seed=SEED,
                             tree_reuse=True, fast_simulations=6, full_search_probability=0.5)
    ex = {k: v.cpu().numpy() for k, v in eng.run(SLOTS).items()}
    eng.ctx.status()
    eng.close()
    for g, rows in games.items():
        sel = np.flatnonzero(ex["game_id"] == g)
        sel = sel[np.argsort(ex["ply"][sel], kind="stable")]
        assert len(sel) == len(rows), g
        for i, (state, pi) in zip(sel, rows):
            assert np.array_equal(ex["states"][i], state) and np.array_equal(ex["policies"][i], pi), (g, i)


def test_tree_reuse_refuses_leaf_parallel_and_aliased_boards(pkg):
    game = pkg.YinYangGame(4, 4)
    for make in (lambda: pkg.SelfPlayEngine(game, hash_evaluator, num_simulations=8, concurrent_games=4, tree_reuse=True, leaves_per_step=4),
                 lambda: pkg.SelfPlayLanes(game, hash_evaluator, num_simulations=8, concurrent_games=4, tree_reuse=True, leaves_per_step=4),
                 lambda: pkg.SelfPlayEngine(game, hash_evaluator, num_simulations=8, concurrent_games=4, tree_reuse=True,
                                            board_semantics="aliased"),
                 lambda: pkg.MCTS(game, hash_evaluator, num_simulations=8, tree_reuse=True, leaves_per_step=4, board_semantics="copied")):
        with pytest.raises(ValueError, match="tree_reuse"):
            make()


def test_the_reference_api_continues_from_the_kept_tree(pkg):
    """MCTS(tree_reuse=True): reuse_tree returns what it returns without it and advances the device tree; the next search of
    that position tops the kept root up, so its children hold num_simulations - 1 visits, not num_simulations."""
    game = pkg.YinYangGame(5, 5)
    m = pkg.MCTS(game, hash_evaluator, num_simulations=40, board_semantics="copied", dirichlet_noise=False, tree_reuse=True)
    board = game.getInitBoard()
    pi, root = m.search(board, 1)
    a = int(np.argmax(pi))
    kept = root.children[a].visits
    assert sum(c.visits for c in root.children.values()) == 40 and kept >= 2
    nb, npl = game.getNextState(board, 1, a)
    new_root = m.reuse_tree(root, nb, npl, a)
    assert new_root is root.children[a] and new_root.parent is None
    pi2, root2 = m.search(nb, npl)
    assert root2.visits == 40 and sum(c.visits for c in root2.children.values()) == 39
    plain = pkg.MCTS(game, hash_evaluator, num_simulations=40, board_semantics="copied", dirichlet_noise=False)
    _, fresh = plain.search(nb, npl)
    assert sum(c.visits for c in fresh.children.values()) == 40
    m.close()
    plain.close()


def test_the_arena_plays_matches_with_tree_reuse(pkg):
    """Every searching player on trees of its own, advanced by both sides' moves: the match ends, every game is scored, no
    search fails (Arena.play raises on a failed game), and a match between two fixed evaluators is deterministic."""
    game = pkg.YinYangGame(4, 4)
    first = pkg.Arena(game, hash_evaluator, hash_evaluator, SIMS, tree_reuse=True).play(6, record=False)
    again = pkg.Arena(game, hash_evaluator, hash_evaluator, SIMS, tree_reuse=True).play(6)
    assert first == again and first["a_wins"] + first["b_wins"] + first["draws"] == first["games"] == 6
    vs_random = pkg.Arena(game, hash_evaluator, "random", SIMS, tree_reuse=True, seed=3).play(5)
    assert vs_random["a_wins"] + vs_random["b_wins"] + vs_random["draws"] == 5
    with pytest.raises(ValueError, match="tree_reuse"):
        pkg.Arena(game, hash_evaluator, "random", SIMS, tree_reuse=True, literal=True)
