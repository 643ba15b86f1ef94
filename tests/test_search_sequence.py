"""The C ABI call order of one search, stated once in engine.BatchedMCTS.run_search and driven by BatchedMCTS.search (eager)
and search.LockstepSearch (graph replay): both drivers on a recording stub context and a recording evaluator.  No GPU."""
import pytest
import torch

from yinyang_game_alphazero_amd import engine
from yinyang_game_alphazero_amd._lib import YYError
from yinyang_game_alphazero_amd.search import LockstepSearch

G, R, C, MAX_SIMS = 4, 6, 6, 8
A = R * C


class Recorder(engine.BatchedMCTS):
    """A context with the plain fields only: every C ABI method appends its name to `log` instead of launching."""

    def __init__(self, K=1, max_sims=MAX_SIMS):
        self.device = torch.device("cpu")
        self.G, self.R, self.C, self.A, self.K = G, R, C, A, K
        self.rows, self.max_sims, self._num_sims = G * K, max_sims, max_sims
        self.keep_evaluations = False
        self.book, self.book_version, self._evaluator_owner = None, 0, None
        self.planes = torch.zeros((self.rows, 5, R, C), dtype=torch.float32)
        self.needs_eval = torch.zeros(self.rows, dtype=torch.uint8)
        self._h = None
        self.log, self.heights = [], []

    def set_num_sims(self, num_sims):
        self.log.append(("set_num_sims", num_sims))

    def begin(self, boards, root_players, active=None):
        self.log.append("begin")

    def expand_root(self, policy, noise=None, eps=0.25):
        self.log.append("expand_root")

    def select(self):
        self.log.append("select")

    def step(self, policy, value):
        self.log.append("step")
        self.heights.append((policy.shape[0], value.shape[0]))

    def expand_backup(self, policy, value):
        self.log.append("expand_backup")
        self.heights.append((policy.shape[0], value.shape[0]))

    def root_counts(self, with_children=False):
        self.log.append("root_counts")
        return torch.zeros((self.G, self.A), dtype=torch.int32)

    def close(self):
        self.log.append("close")


class Evaluator:
    """Uniform policy, zero value; logs "eval" on the context and keeps (rows seen, sorted keyword names, needs_eval rows)."""

    def __init__(self, ctx, **protocol):
        self.ctx, self.calls = ctx, []
        for k, v in protocol.items():
            setattr(self, k, v)

    def __call__(self, planes, **kw):
        self.ctx.log.append("eval")
        need = kw.get("needs_eval")
        self.calls.append((planes.shape[0], sorted(kw), None if need is None else need.shape[0]))
        g = planes.shape[0]
        return torch.full((g, A), 1.0 / A), torch.zeros(g)


def expected(num_sims, K, fused=True):
    log = ([("set_num_sims", num_sims)] if K > 1 else []) + ["begin", "eval", "expand_root", "select"]
    if num_sims == 0:
        return log
    S = -(-num_sims // K)
    log += (S - 1) * (["eval", "step"] if fused else ["eval", "expand_backup", "select"])
    return log + ["eval", "expand_backup"]


def positions():
    return torch.zeros((G, R, C), dtype=torch.int8), torch.ones(G, dtype=torch.int8)


CASES = [(K, n) for K in (1, 3) for n in (0, 1, 2, 3, 7)]


@pytest.mark.parametrize("K,num_sims", CASES)
@pytest.mark.parametrize("fused", [True, False])
def test_search_issues_the_sequence_and_no_keyword(K, num_sims, fused):
    ctx = Recorder(K)
    ev = Evaluator(ctx)
    ctx.search(*positions(), ev, num_sims, fused=fused)
    assert ctx.log == expected(num_sims, K, fused) + ["root_counts"]
    assert all(c == (G * K, [], None) for c in ev.calls)


@pytest.mark.parametrize("K,num_sims", CASES)
def test_lockstep_issues_the_sequence(K, num_sims):
    ctx = Recorder(K)
    LockstepSearch(ctx, Evaluator(ctx), use_graph=False).run(*positions(), num_sims)
    assert ctx.log == expected(num_sims, K)


@pytest.mark.parametrize("K,num_sims", CASES)
def test_lockstep_keywords_follow_the_evaluator_protocol(K, num_sims):
    ctx = Recorder(K)
    ev = Evaluator(ctx, supports_compaction=True, supports_static=True)
    LockstepSearch(ctx, ev, use_graph=False).run(*positions(), num_sims)
    assert ctx.log == expected(num_sims, K)
    assert ev.calls[0] == (G * K, ["static"], None)                                  # never needs_eval on the root call
    assert all(c == (G * K, ["needs_eval", "static"], G * K) for c in ev.calls[1:])


def test_lockstep_rows_limit_evaluates_the_front_rows_into_full_height_buffers():
    K, rows, num_sims = 3, 2, 7
    ctx = Recorder(K)
    ev = Evaluator(ctx, supports_compaction=True, supports_static=True)
    LockstepSearch(ctx, ev, use_graph=False).run(*positions(), num_sims, rows=rows)
    assert ctx.log == expected(num_sims, K)
    assert ev.calls[0] == (rows * K, ["static"], None)
    assert all(c == (rows * K, ["needs_eval", "static"], rows * K) for c in ev.calls[1:])
    assert ctx.heights == [(G * K, G * K)] * 3                                       # two fused steps and the last backup


@pytest.mark.parametrize("K", [1, 3])
def test_both_drivers_refuse_more_simulations_than_the_context_holds(K):
    texts = []
    for drive in (lambda ctx, ev: ctx.search(*positions(), ev, MAX_SIMS + 1),
                  lambda ctx, ev: LockstepSearch(ctx, ev, use_graph=False).run(*positions(), MAX_SIMS + 1)):
        ctx = Recorder(K)
        with pytest.raises(YYError) as e:
            drive(ctx, Evaluator(ctx))
        assert "begin" not in ctx.log and "eval" not in ctx.log
        texts.append(str(e.value))
    assert texts[0] == texts[1] and "max_sims" in texts[0]


class FakeGraph:
    """Stands for a captured graph of `steps` steps: capturing runs nothing, a replay issues the steps."""

    def __init__(self, search, rows, steps):
        self.search, self.rows, self.steps, self.replays = search, rows, steps, 0

    def replay(self):
        self.replays += 1
        for _ in range(self.steps):
            self.search._sim_step(self.rows)


@pytest.mark.parametrize("unroll,S,first,second", [
    (4, 4, {}, {}),                                    # 3 middle steps: not more than eager_sims, nothing captured
    (4, 5, {1: 1}, {1: 5}),                            # 4: the one-step graph only
    (4, 11, {1: 7}, {1: 17}),                          # 10: 7 left after the warm-up, fewer than 2 * unroll
    (4, 12, {1: 0, 4: 2}, {1: 3, 4: 4}),               # 11: 8 left, both graphs
    (4, 13, {1: 1, 4: 2}, {1: 1, 4: 5}),
    (1, 5, {1: 1}, {1: 5}),                            # unroll 1: one-step graphs only, whatever is left
    (1, 13, {1: 9}, {1: 21}),
])
def test_capture_policy_on_fake_graphs(monkeypatch, unroll, S, first, second):
    """Which graphs a first search captures (eager_sims = 3) and how often each is replayed, then a second, all-replay search;
    values are total replays per graph length after the first and after the second search."""
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: None)
    monkeypatch.setattr(LockstepSearch, "_captured", lambda self, rows, steps: FakeGraph(self, rows, steps))
    ctx = Recorder(1, max_sims=S)
    ls = LockstepSearch(ctx, Evaluator(ctx), use_graph=True, eager_sims=3, unroll=unroll)
    for want in (first, second):
        del ctx.log[:]
        ls.run(*positions(), S)
        assert ctx.log == expected(S, 1)
        assert {g.steps: g.replays for g in ls.graphs.values()} == want
        assert len(ls.graphs) == len(want) and set(ls.graphs) == {G if n == 1 else (G, n) for n in want}


def test_both_drivers_go_through_the_one_shared_function(monkeypatch):
    monkeypatch.setattr(Recorder, "run_search", lambda self, *a, **kw: self.log.append("run_search"), raising=True)
    ctx = Recorder(3)
    ctx.search(*positions(), Evaluator(ctx), 7)
    assert ctx.log == ["run_search", "root_counts"]
    ctx = Recorder(3)
    LockstepSearch(ctx, Evaluator(ctx), use_graph=False).run(*positions(), 7)
    assert ctx.log == ["run_search"]
