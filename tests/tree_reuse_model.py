"""Plain-numpy float32 restatement of tree reuse across moves (include/yy_engine.h yy_mcts_advance).

TEST INFRASTRUCTURE.  One game, copied boards, K = 1: the search, the Tree and advance() of tests/tree_model.py.

  search(root_or_board, player, budget)  a board: the reference's search from a fresh root (oracle_lib.search_hash, and
                                         leaf_parallel_model.search at K = 1).  A Tree (what advance() returns): the search
                                         tops the kept root up -- it stops when root.visits == budget, so a root that already
                                         holds its budget runs nothing.  The root call is made either way; on a kept root its
                                         policy row is ignored and a noise row that is non-zero over the root's moves is mixed
                                         into the STORED priors, p = f32(f64(f32(1-eps)*P) + eps*noise).
  advance(tree, action)                  -> (Tree or None, kept_visits).  The child under `action` becomes the root when the
                                         root has an edge with that action whose child is a node that is not terminal and has
                                         children; its visits are the edge's N, its value sum the edge's W (float32).

Counters are counted per search() call the way leaf_parallel_model counts them (its module docstring); a kept root adds no
children_created of its own (it is not expanded again).

`mutant=` (MUTANTS) breaks one rule on purpose; tests/test_tree_reuse_model.py asserts that the GPU cases' inputs tell each from
the true model."""
import tree_model
from hash_eval import hash_eval_batch  # noqa: F401  (the callers build the root_policy rows with it)
from tree_model import TERMINAL, Tree, advance  # noqa: F401

MUTANTS = {
    "root_sum": "the kept root's visits are the sum of its children's N (one less than the edge's N)",
    "budget_additional": "the budget of a kept root counts additional simulations, not the root's visits",
    "noise_policy": "noise on a kept root is mixed into the root call's policy row, not into the stored priors",
    "keep_terminal": "a terminal child is kept",
    "edge_order": "the kept nodes' edges do not keep their order (descending action)",
}


def search(root_or_board, player, budget, pbits=10, vbits=11, trace=None, mutant=None, **options):
    """tree_model.search at K = 1 -> Result, with needs (one bool per simulation run: did it take an evaluator row).  trace:
    optional list; every simulation that takes a row appends its board int8 [R, C].  root_policy: the row handed to the root
    expansion in place of the evaluator's (what yy_mcts_expand_root is given); a kept root does not read it."""
    assert mutant is None or mutant in MUTANTS
    steps = []
    r = tree_model.search(root_or_board, player, budget, 1, pbits, vbits, trace=steps, mutant=mutant and "tree_reuse." + mutant,
                          **options)
    r.needs = [kind != TERMINAL for kind in r.ended]
    if trace is not None:
        trace.extend(d.board.copy() for step in steps for d in step if d.needs_eval)
    return r
