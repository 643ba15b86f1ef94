"""Plain-numpy float32 restatement of the leaf-parallel search (leaves_per_step K, include/yy_engine.h and DESIGN.md).

TEST INFRASTRUCTURE.  One game, copied boards, the rules of the CPU oracle (oracle_lib) and the exact hash evaluator of
hash_eval.py; the search sequence itself, the plain PUCT _select and the counters are tests/tree_model.py's.  Every step runs K_eff = min(K, simulations not yet started) descents on the tree as it stands; descent j sees
on every edge the virtual count v of the descents 0 .. j-1 of this step that walked it, and scores a child with n = N + v,
w = v > 0 ? f32(W - f32(v)) : W, S = sum of the children's n.  A descent that ends on the leaf of an earlier one (same
unexpanded edge, same childless node) takes no evaluation and shares the earlier one's.  Then, in descent order, the first
occurrence of a leaf expands it and every descent backs its value up.  At K = 1 this is the reference's search
(oracle_lib.search_hash), which tests/test_leaf_parallel_model.py checks.

The device counters (BatchedMCTS.COUNTERS, GameState.ctr in csrc/yy_engine.hip) are counted where the kernels count them:
  levels             every edge a descent walks (one select_child call), so at the end the sum of N over all edges;
  children_scanned   the children of the node of every such call;
  children_created   the edges of every node expanded WITH children -- the root's own expansion included (the root call goes
                     through the same expand_leaf), a terminal or childless node adds 0, and so does a re-expansion;
  nodes              the nodes a search adds below the root, one per `expand` leaf -- the root itself is NOT counted;
  terminal_revisits  the descents that ended on a terminal node, a terminal root's included;
  evals              the evaluator rows asked for after the root call (the root call is not counted).
evals + terminal descents + duplicate descents == root_visits.  A failed game (NaN value or prior, full arena, path too deep)
is outside this model: it has no arena and no NaN.  On the device such a game keeps what it counted up to the failure -- levels,
children_scanned and terminal_revisits of the descents walked, evals of every step whose selection completed (the step whose
expansion then fails included), nodes and children_created of the expansions done before the failing one -- and counts nothing
afterwards.

`mutant=` (MUTANTS) breaks one rule on purpose; tests/test_leaf_parallel_model.py asserts that the GPU cases tell each from the
true model."""
import tree_model
from tree_model import EXPAND, REEXPAND, ROOTPASS, TERMINAL, Descent, Edge, Node, Result, _expand, _select  # noqa: F401

MUTANTS = {
    "keep_w": "the virtual visits are not subtracted from W (w = W, n = N + v)",
    "s_parent": "S is N(node) - 1 (the root: its completed simulations), not the sum of the children's N + v",
    "dup_row": "a duplicate leaf takes an evaluator row of its own",
    "tie_high": "ties go to the highest action",
    "full_last": "the last step runs K descents, not K_eff",
    "reverse_backup": "the expansion + backup phase runs in reverse descent order",
    "terminal_f32": "a terminal value is backed up as float32 where the python-float rule applies (terminal root)",
    "v_low64": "virtual counts are dropped for the children of index >= 64 of a node",
}


def search(board, player, sims, K, pbits=10, vbits=11, mutant=None, **options):
    """tree_model.search with K descents per step; mutant: one of MUTANTS, or None for the true search.  -> Result"""
    assert mutant is None or mutant in MUTANTS
    return tree_model.search(board, player, sims, K, pbits, vbits, mutant=mutant and "leaf_parallel." + mutant, **options)
