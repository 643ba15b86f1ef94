"""Graph-replayed driver of engine.BatchedMCTS.run_search: what SelfPlayEngine, Arena and MCTS (above 8 simulations) search with."""
import gc
import os

import torch


class LockstepSearch:
    """MCTS.search for G games with the simulation loop replayed from a hipGraph.

    One graph = [evaluator forward on ctx.planes] + [yy_mcts_step]; everything in it is enqueued on
    the capture stream (the C ABI takes the stream as an argument), so a replay costs one host call
    instead of ~60 kernel launches."""

    def __init__(self, ctx, evaluator, use_graph=True, eager_sims=3, unroll=None):
        self.ctx, self.evaluator, self.use_graph, self.eager_sims = ctx, evaluator, use_graph, eager_sims
        # simulations per replayed graph: besides the one-step graph a second one holds `unroll` consecutive steps
        # (fewer host calls, and no graph-to-graph launch gap between the steps inside it); 1 = one-step graphs only
        self.unroll = max(1, int(os.environ.get("YY_GRAPH_UNROLL", "8") if unroll is None else unroll))
        self.graphs = {}       # evaluated rows -> captured step
        self.timer = None      # optional object with start()/stop() bracketing every tree-kernel launch (bench.py)
        self._policy = self._value = None
        self._book_version, self._graph_evaluator = ctx.book_version, evaluator

    @property
    def graph(self):
        return self.graphs.get(self.ctx.G)

    @graph.setter
    def graph(self, g):
        if g is None:
            self.graphs.clear()
        else:
            self.graphs[self.ctx.G] = g

    def _evaluate(self, rows, compact=False):
        """Evaluator on the leaf rows of the first `rows` games (all searching games must sit there); returns full-height buffers.
        compact: pass the step's needs_eval flags to an evaluator that can skip the rows whose leaf needs no evaluation
        (terminal revisits, mcts.py:365-366; finished or idle slots).  With K leaves per step a game has K rows."""
        ctx = self.ctx
        full, rows = ctx.rows, rows * ctx.K        # G * K evaluator rows in all
        kw = {}
        if compact and getattr(self.evaluator, "supports_compaction", False):
            kw["needs_eval"] = ctx.needs_eval if rows >= full else ctx.needs_eval[:rows]
        if getattr(self.evaluator, "supports_static", False):
            kw["static"] = id(self)                # private buffers: the results are consumed by the tree kernel before this search's next call
        if rows >= full:
            return self.evaluator(ctx.planes, **kw)
        policy, value = self.evaluator(ctx.planes[:rows], **kw)
        if self._policy is None:
            self._policy = torch.zeros((full, policy.shape[1]), dtype=torch.float32, device=ctx.device)
            self._value = torch.zeros(full, dtype=torch.float32, device=ctx.device)
        self._policy[:rows].copy_(policy)
        self._value[:rows].copy_(value)
        return self._policy, self._value

    def _sim_step(self, rows):
        policy, value = self._evaluate(rows, compact=True)
        if self.timer is not None:
            self.timer.start()
        self.ctx.step(policy, value)
        if self.timer is not None:
            self.timer.stop()

    def _drop_stale_graphs(self):
        """A captured step has its kernel arguments frozen (the book's tables) and calls the evaluator it was captured with."""
        if self.ctx.book_version != self._book_version or self._graph_evaluator is not self.evaluator:
            self.graphs.clear()
            self._book_version, self._graph_evaluator = self.ctx.book_version, self.evaluator

    def _captured(self, rows, steps):
        """`steps` steps captured into one graph.  Python's cycle collector is kept out of the capture: it runs when it pleases,
        and a dropped engine that sits in a reference cycle (a caller that wrapped one of its methods, say) takes its captured
        graphs and its device buffers with it only then -- destroying a graph or freeing device memory is not allowed while a
        stream is capturing, and a destructor has no way to report the failure.  So automatic collection is off until the capture
        has ended; what it would have collected waits for the next collection outside.  (No gc.collect() in front: a full
        collection per capture cost the default bench line 2 %.)"""
        graph = torch.cuda.CUDAGraph()
        was_enabled = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph):
                for _ in range(steps):
                    self._sim_step(rows)
        finally:
            if was_enabled:
                gc.enable()
        return graph

    def _capture(self, gkey, rows, n):
        """First visit of `gkey` with more than eager_sims steps to issue: eager_sims real steps as warm-up, then the one-step
        graph and, when at least 2 * unroll steps remain, the unroll-step graph.  Returns the steps done."""
        for _ in range(self.eager_sims):                       # warm-up (MIOpen algo search etc.) = real sims
            self._sim_step(rows)
        torch.cuda.synchronize(self.ctx.device)
        self.graphs[gkey] = self._captured(rows, 1)            # stored only once the capture has succeeded
        if self.unroll > 1 and n - self.eager_sims >= 2 * self.unroll:
            self.graphs[(gkey, self.unroll)] = self._captured(rows, self.unroll)
        return self.eager_sims

    def _middle_steps(self, rows, n):
        """The n steps between the first select and the last evaluation: replayed where a graph exists, issued otherwise."""
        gkey = rows if not hasattr(self.evaluator, "form_key") else (rows, self.evaluator.form_key(id(self)))
        done = 0
        if self.use_graph and gkey not in self.graphs and n > self.eager_sims:
            done = self._capture(gkey, rows, n)
        graphs = self.graphs if self.use_graph else {}
        graph, many = graphs.get(gkey), graphs.get((gkey, self.unroll))
        while done < n:
            if many is not None and n - done >= self.unroll:
                many.replay()
                done += self.unroll
            elif graph is not None:
                graph.replay()
                done += 1
            else:
                self._sim_step(rows)
                done += 1

    def issue(self, n):
        """n steps of whatever _sim_step issues, outside a search of run(): the free-running driver's call."""
        self.ctx.bind_evaluator(self.evaluator)
        self._drop_stale_graphs()
        self._middle_steps(self.ctx.G, n)

    def run(self, boards, root_players, num_sims, noise=None, eps=0.25, active=None, rows=None, num_sims_bound=None):
        """rows: evaluate only leaf rows [0, rows) -- the caller guarantees every active game has an index below it
        (SelfPlayEngine packs the live games to the front when a batch drains).  One graph per distinct `rows`.
        num_sims / num_sims_bound: an int or per-game budgets (engine.BatchedMCTS.run_search); the captured steps do not
        depend on them."""
        ctx = self.ctx
        ctx.bind_evaluator(self.evaluator)                     # kept evaluations / the book belong to ONE network (may drop the book)
        self._drop_stale_graphs()
        rows = ctx.G if rows is None else min(int(rows), ctx.G)
        ctx.run_search(boards, root_players, num_sims, lambda root: self._evaluate(rows, compact=not root), noise, eps, active,
                       lambda n: self._middle_steps(rows, n), num_sims_bound)


class FreeRunningSearch(LockstepSearch):
    """The step of free-running self-play under LockstepSearch's capture scheme (a few eager steps, then the one-step graph and
    the unrolled one, keyed by the evaluator's form_key): one step = [evaluator on the rows flagged by needs_eval] +
    [engine.SelfPlayRun.step: the tree step with root noise + the move kernel].  The steps of all games are the same launch
    sequence whatever the games are doing, so issue(n) replays it n times; nothing is read back."""

    def __init__(self, ctx, evaluator, run, use_graph=True, eager_sims=3, unroll=None):
        super().__init__(ctx, evaluator, use_graph=use_graph, eager_sims=eager_sims, unroll=unroll)
        self.run_state = run              # the captured steps hold its pointers: a new run means a new FreeRunningSearch

    def _sim_step(self, rows):
        policy, value = self._evaluate(rows, compact=True)
        if self.timer is not None:
            self.timer.start()
        self.run_state.step(policy, value)
        if self.timer is not None:
            self.timer.stop()
