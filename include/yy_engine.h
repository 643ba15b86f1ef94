/*
 * yy_engine.h -- C ABI of libyy_hip.so, the MI355X (gfx950) Yin-Yang self-play hot path.
 *
 * The reference (Arash-san/YinYang-Game-AlphaZero) is pure Python and has no FFI: the drop-in
 * boundary is its Python class API.  This header is the C-ABI a maintainer would bind with ctypes
 * from those classes (INTEGRATION.md shows the stubs); every entry point cites the reference
 * interface it replaces as path:line under the reference root.
 *
 * Conventions
 *   - plain pointers and sizes only; ALL data pointers are DEVICE pointers (HBM) unless the
 *     parameter is documented as host; no torch types.
 *   - every function returns an int status (YY_OK or a negative YY_E_*); yy_last_error() gives a
 *     thread-local message.  No C++ exception crosses the ABI.
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *     no call synchronises unless documented ("sync").
 *   - boards are int8 [G,R,C] row-major, 0 empty / +1 black / -1 white
 *     (src/yin_yang/yin_yang_logic.py:8-18); players are int8 +1 / -1; an action is x*C+y
 *     (src/yin_yang/yin_yang_game.py:180-186).  1 <= R,C <= 16 and R*C <= 192.
 */
#ifndef YY_ENGINE_H
#define YY_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YY_OK 0
#define YY_E_INVALID (-1)     /* null pointer, non-positive size, bad enum */
#define YY_E_UNSUPPORTED (-2) /* board larger than 16x16 / 192 cells */
#define YY_E_NOMEM (-3)       /* hipMalloc failed */
#define YY_E_HIP (-4)         /* HIP runtime error (message in yy_last_error) */
#define YY_E_STATE (-5)       /* call order violation (e.g. expand before select) */
#define YY_E_ARENA (-6)       /* a game's tree arena overflowed (reported by yy_mcts_status) */

/* rule / semantics flags */
#define YY_FLAG_ROWCOL 1u  /* also enforce the browser-only full-row/column rule
                              (src/gui/static/js/yin_yang_game.js:338-384). Default off: the
                              Python rules have no such rule. */
#define YY_FLAG_ALIASED 2u /* MCTS shares ONE board per game through the whole tree and mutates
                              it, exactly like the reference (yin_yang_game.py:52-58 +
                              ai/mcts.py:385-397).  Default (flag clear) = "copied": every
                              expanded node owns its board. */
#define YY_FLAG_REUSE_PASS_VALUE 4u /* copied boards only (yy_mcts_create refuses it with YY_FLAG_ALIASED).  The
                              reference evaluates a non-terminal node without legal moves again on EVERY visit
                              (ai/mcts.py:93-95 is_expanded() is False without children, :371-397 evaluate + expand).
                              With copied boards the node's position never changes, so the evaluator returns the
                              same value each time; with this flag the value of the first evaluation is kept in the
                              node record and a revisit takes it from there: no planes written, needs_eval = 0,
                              counters[6] (TC_REUSED) += 1.  Visit counts, value sums and pi are unchanged (tests/test_gpu_mcts.py
                              ::test_evaluation_reuse_*); counters[0] (TC_EVALS, evaluator rows) gets smaller.  Default off:
                              the evaluator call sequence is then the reference's, row for row. */

#define YY_FLAG_REUSE_TRANSPOSITIONS 8u /* evaluation cache, one search at a time.  The reference evaluates every leaf
                              (ai/mcts.py:371-397), also when the position was evaluated before: another move order
                              inside the same search, a pass node visited again.  A deterministic evaluator returns the
                              same (policy, value) each time -- its input planes encode the board only, not the side to
                              move (ai/neural_network.py:156-196).  With this flag every game keeps a table in HBM
                              [position -> policy row f32[A], value], open addressing on a 64-bit mix of the bitboards,
                              <= 8 probes, keys compared in full; a leaf whose position is in the table takes its
                              evaluation from there instead of an evaluator row (needs_eval = 0, no planes written,
                              counters[7] (TC_TABLE_HITS) += 1).  Only entries written by the current search are used.  Same visit
                              counts, value sums and pi (tests/test_gpu_mcts.py::test_evaluation_reuse_*).  Works with
                              copied and aliased boards (the key is the position, not the node).  Default off: the
                              evaluator's call sequence is then the reference's, row for row. */
#define YY_FLAG_KEEP_EVALUATIONS 16u /* implies the table of YY_FLAG_REUSE_TRANSPOSITIONS and keeps its entries from one
                              search to the next (the next move's search re-derives much of the subtree the game walked
                              into: at 8x8 / 800 simulations about half of the rows that are new within a search were
                              evaluated by an earlier search of the same game).  Entries are replaced oldest-game first,
                              then positions that cannot recur (no more stones than the root).  REQUIRES that every
                              search of the context uses the same evaluator: call yy_mcts_cache_clear when it changes.
                              The rules in full (restated by tests/eval_cache_model.py): a fresh evaluation goes into the
                              first probed slot that is never used, of another epoch, or holds no more stones than the
                              root, else into the first slot of the window; a hit refreshes nothing (an entry of an older
                              epoch that is hit is still the first to be replaced); a pass root's own position is stored
                              as one that cannot recur and is found until its slot is taken; the epoch (24 bits, never
                              0) advances only at a root without stones, and yy_mcts_cache_clear leaves it. */

#define YY_FLAG_EVAL_SYMMETRY 32u /* symmetry-randomised evaluation (not in the reference; copied boards only: create refuses it
                              with YY_FLAG_ALIASED).  Every position (black, white) is shown to the evaluator under a board symmetry
                              s = sym(symmetry_seed, black, white) drawn from the project's Philox streams: a pure function of
                              the seed and the position -- not of slot, game, ply, simulation, batch or rank -- so the evaluation
                              cache, the book and "a row's result does not depend on its batch" stay true.  Keying: Philox4x32-10
                              with the key symmetry_seed ^ 0x59595F53594D5F34 (the domain tag: every other stream keys with its
                              seed itself), the NW 64-bit word pairs chained: block i has the counter (black[i] lo, black[i] hi,
                              white[i] lo, white[i] hi) ^ the output of block i - 1 (zero for i = 0); s = the top 3 (square
                              boards) or 2 bits of the last block's first word.  Square boards, s in 0 .. 7: np.rot90(board,
                              s & 3), then np.fliplr when s & 4; other boards, s in 0 .. 3: np.flipud when s & 1, np.fliplr when
                              s & 2.  The row written for the position (yy_mcts_begin, select, step) is planes(T_s(board)), all
                              five planes encoded from the transformed board; the prior of action a is policy[T_s(a)], T_s(a) =
                              where cell a lands; the value is used as is.  Noise, the NaN rule, edge order, cache keys and every
                              read-out stay in the original frame; the cache and the book hold rows as the evaluator returned
                              them and are read through the same map (a book must be built with yy_encode_planes_sym and the
                              same seed).  Flag clear: every kernel does what it did without it. */

#define YY_FLAG_FORCED_PLAYOUTS 64u /* forced playouts with policy target pruning at the search root (Wu, "Accelerating Self-Play
                              Learning in Go", section 3.2; not in the reference).  k = yy_mcts_config.forced_playouts, positive
                              and finite (else YY_E_INVALID), fixed at creation.  Copied boards and leaves_per_step <= 1 only: create
                              returns YY_E_UNSUPPORTED with YY_FLAG_ALIASED or K > 1.  Forcing, at depth 0 of every descent: with S
                              the sum of the root's child visits that its PUCT uses (root visits, one less on a root kept by
                              yy_mcts_advance), P the edge's stored prior (the noised one at a noised root) and N its visits, an
                              edge is forced iff N >= 1 and f64(N)*f64(N) < (k*f64(P))*f64(S); the descent takes the forced edge of
                              the lowest action, else the PUCT choice.  Below the root, expansion and backup are untouched.
                              Pruning: yy_mcts_root_policy and the move of yy_mcts_step_selfplay compute pi from counts N': c* =
                              the most visited edge (lowest action on ties) keeps N; every other edge with N > 0 gives back, one
                              visit at a time and at most n_f = min{m >= 0: f64(m)*f64(m) >= (k*f64(P))*f64(S)} of them, every
                              visit without which its PUCT score (N' - 1 in the exploration term, W / N unchanged) stays below
                              c*'s score at the final S; N' == 1 becomes 0.  yy_mcts_root_counts returns the raw visits.
                              Flag clear: every kernel does what it did without it. */

#define YY_FLAG_FPU_REDUCTION 128u /* first-play urgency reduction in the PUCT selection (KataGo / Lc0 practice; not in the
                              reference, which scores an unvisited child with q = 0).  r = yy_mcts_config.fpu_reduction at every
                              node below the root, r = yy_mcts_config.fpu_reduction_root at the root (depth 0 of a descent); r
                              positive and finite, the root's finite and >= 0 (else YY_E_INVALID), fixed at creation.  Every
                              board semantics, every leaves_per_step, every other flag.  At the node a descent selects from, with
                              N and W of each child as its score reads them (leaves_per_step > 1: N + v and W less the virtual
                              visits), over the children with N > 0:
                                SN = sum of N                                          (integer)
                                SW = f32(f64(sum of (int64)(f64(W) * 2^32)) * 2^-32)   (each term truncated toward zero)
                                SP = f32(f64(sum of (uint64)(f64(P) * 2^40)) * 2^-40)  (P the stored prior: the noised one at a
                                                                                        noised root; each term truncated)
                              so that the sums do not depend on the order of the children.  A child with N == 0 is scored with
                                q_fpu = f32( f32(SW / SN) - f32( r * f32(sqrt(SP)) ) )
                              in place of 0 -- the division, the square root, the product and the difference each the correctly
                              rounded float32 one, in this order -- and with q_fpu = 0 when SN == 0.  Its exploration term, the
                              `+ 0.0f` and the score of every visited child are unchanged.  The estimate of the node's value is
                              the mean over its visited children on purpose: it is in the units and the sign convention of the
                              W / N it stands in for.  Flag clear: every kernel does what it did without it. */

#define YY_FLAG_SOLVER 256u /* MCTS-Solver (Winands et al. 2008; Lc0's "certainty propagation"; not in the reference): exact
                              results are proven in the tree and descents stop below them.  Copied boards and leaves_per_step
                              <= 1 only (create returns YY_E_UNSUPPORTED otherwise); every other flag.  A node may carry a proven
                              status for its side to move -- 1 WIN, 2 LOSS, 3 DRAW -- with the exact value f32 1 / -1 / 1e-4,
                              the terminal values of the tree.  A terminal node is proven with the class of its terminal value.
                              A node without children (the mover has no move, the game is not over) is never proven: no proof
                              looks through a pass.  After the backup of a descent that ended on a terminal node (a revisit, or
                              the expansion that found the position terminal) or on a proven node, the path is walked upwards
                              from the leaf's parent: a node with k > 0 children becomes WIN if any child that exists is LOSS
                              for the child's mover; otherwise, if all k children exist and all are proven, DRAW if any is
                              DRAW, else LOSS; the walk stops at the first node whose status does not change.  The root may
                              become proven.  A proven node below the root ends a descent there: no evaluator row
                              (needs_eval = 0), its exact value is backed up exactly as a terminal revisit's is (a python
                              number, the same arithmetic), and the walk runs again (it changes nothing).  The root is never
                              treated as terminal: a search keeps spreading its budget over the root's children.  Selection
                              scores, visit counts, value sums and the root distribution are computed as without the flag;
                              the value sums of a proven node are not rewritten.  yy_mcts_advance carries the statuses with
                              the node records.  Flag clear: no node ever carries a status and every kernel does what it did
                              without it. */

#define YY_FLAG_GUMBEL_ROOT 512u /* Gumbel root search (Danihelka et al., "Policy improvement by planning with Gumbel", ICLR
                              2022; not in the reference): Gumbel noise, sequential halving and a completed-Q policy target at
                              the ROOT of every search; below the root the descent is untouched.  m = yy_mcts_config.gumbel_root
                              in 2 .. 64, c_visit = gumbel_c_visit finite and >= 0, c_scale = gumbel_c_scale finite and > 0 (else
                              YY_E_INVALID; the paper's board-game values: 16, 50, 1), fixed at creation.  Copied boards and
                              leaves_per_step <= 1 only, and not with YY_FLAG_FORCED_PLAYOUTS or YY_FLAG_SOLVER: create returns
                              YY_E_UNSUPPORTED; yy_mcts_advance returns YY_E_UNSUPPORTED on such a context (each a follow-up).
                              Base score: the root expansion needs the Gumbel rows of yy_mcts_set_gumbel (YY_E_STATE without)
                              and writes, for root edge j of action a and stored prior P (the noised one at a noised root;
                              eps = 0 is recommended), s0[j] = f32(f64(g[a]) + log(f64(P))); P == 0 gives -inf.
                              Budget: n = the game's simulation budget -- its entry of yy_mcts_set_sim_budgets, else the scalar
                              of yy_mcts_set_num_sims, which a context with the flag stores at K = 1 as well.
                              Considered visits: with k root children and m' = min(m, k), seq(m', n) is 0, 1, .. n-1 for
                              m' <= 1; else, with L = ceil(log2 m'), c = m' and v = 0: phases of extra = max(1, n / (L*c))
                              (integer division) rounds, round r of a phase being c entries of value v + r; after a phase
                              v += extra, c = max(2, c / 2); cut after n entries (mctx's table).
                              Selection at depth 0 of a descent, S the sum of the root children's visits and v = seq[S]:
                              among the children with N == v (all children when there is none) the largest
                              f32(s0 + sigma), the lowest edge (= lowest action) on ties, -inf ties included;
                              sigma = f32(f32(f32(c_visit + f32(maxN)) * c_scale) * q), maxN the largest child visit count,
                              q = f32(W / f32(N)) for N > 0, else 0, W the edge's value sum as PUCT reads it.  So the first m'
                              root descents expand the m' children of largest g + log P; no candidate set is stored.
                              Policy target: yy_mcts_root_policy (both temperatures) and the example record of
                              yy_mcts_step_selfplay return pi' = softmax(log f64(P) + sigma64(cq)) over the root's edges in
                              float64, sigma64(x) = (f64(c_visit) + f64(maxN)) * f64(c_scale) * x, cq = f64(W) / f64(N) of a
                              visited child, and for an unvisited one SW / SN over the visited children, SW = f64(sum of
                              (int64)(f64(W) * 2^32)) * 2^-32 (each term truncated toward zero: no order dependence), 0 when
                              none is visited (YY_FLAG_GUMBEL_INTERIOR completes with the paper's v_mix instead).  A root
                              without children keeps the uniform row.  yy_mcts_root_counts stays raw.
                              The move: yy_mcts_root_gumbel_action -- among the children with the largest visit count the
                              largest f32(s0 + sigma), the lowest edge on ties -- which yy_mcts_step_selfplay plays at every ply
                              (no temperature rule, no move draw).  Flag clear: every kernel does what it did without it. */

#define YY_FLAG_GUMBEL_INTERIOR 1024u /* the rest of Gumbel AlphaZero (Danihelka et al. 2022, section 5 and appendix D): v_mix
                              and completed-Q selection below the root.  Only with YY_FLAG_GUMBEL_ROOT, and not with
                              YY_FLAG_FPU_REDUCTION (no PUCT score is left for it to act on): create returns YY_E_UNSUPPORTED.  It goes
                              with and is refused with whatever YY_FLAG_GUMBEL_ROOT is.  Flag clear: every kernel does what it
                              did without it, the plain Gumbel root search included.  With it:
                              (1) The root record keeps the evaluator's value of the root position, as every other expanded
                              node's does; nothing is backed up.  The root expansion is yy_mcts_expand_root_value
                              (yy_mcts_expand_root returns YY_E_UNSUPPORTED); yy_mcts_step_selfplay reads the value of the root's
                              row.  A NaN value fails the game like any other expansion's.
                              (2) The improved policy of a node with k > 0 edges, from its own evaluator value vhat (f32) and
                              per edge the stored prior P (f32), visits N and value sum W (f32).  All products, sums and
                              quotients below are the correctly rounded float64 ones, one rounding each, never contracted:
                                p(a)  = (uint64)(max(f64(P) * 2^40, 0))             (truncated; the prior in units of 2^-40)
                                q(a)  = f64(W) / f64(N)                             (N > 0)
                                S     = sum of N,  maxN = largest N                 (integers)
                                SPv   = sum over N > 0 of p(a)                      (integer)
                                SPQ   = sum over N > 0 of (int64)(f64(p(a)) * q(a)) (integer, each term truncated toward zero;
                                                                                      a NaN or infinite product adds 0)
                                v_mix = f64(vhat)                                             if S == 0
                                v_mix = (f64(vhat) + f64(S) * wq) / f64(1 + S),  wq = f64(SPQ) / f64(SPv), 0 when SPv == 0
                                cq(a) = q(a) if N > 0, else v_mix
                                x(a)  = ((f64(c_visit) + f64(maxN)) * f64(c_scale)) * cq(a)   (sigma of the root's target; no
                                                                                               min-max rescaling of q)
                                xm    = the largest x(a) over the edges with p(a) > 0 (NaNs passed over)
                                t(a)  = (uint64)((f64(p(a)) * E(x(a) + (-xm))) * 2^12)         (truncated; 0 where p(a) == 0)
                                Z     = sum of t(a)                                            (integer, below 2^53)
                                pi'(a) = f64(t(a)) / f64(Z)
                              so no sum depends on the order of the children, no log is taken, and with finite value sums the
                              edge that sets xm has E = 1, hence Z > 0.  Every p(a) == 0: t(a) = 1 for every edge (the uniform
                              row).  An edge whose x(a) - xm is a NaN (a NaN or infinite value sum) carries no term, its pi'
                              and score are NaN; when that leaves Z == 0, every pi' and every score is the NaN 0 / 0.
                              vhat is taken with the sign it is stored with -- the evaluator's value for the node's side to
                              move -- while W / N of an edge is in the tree's inherited convention (the backed-up value as the
                              CHILD's side to move sees it, mcts.py:406-412): v_mix mixes the two as they stand.
                              E(x), x <= 0, is the project's own exponential: 0 below -708; else n = rint(x * log2e) (half to even),
                              r = (x + (-(n * ln2_hi))) + (-(n * ln2_lo)), log2e = 0x1.71547652b82fep+0, ln2_hi = 0x1.62e42feep-1,
                              ln2_lo = 0x1.a39ef35793c76p-33; p = 1/13!, then p = p * r + 1/i! for i = 12 .. 0 (the constants
                              are the float64 quotients 1.0 / i!; multiply and add rounded separately); E = p * 2^n, exact.
                              Within 1e-14 relative of exp (the Taylor remainder on |r| <= 0.3466 is below 2^-53).
                              (3) Policy target: yy_mcts_root_policy and the example record of yy_mcts_step_selfplay return pi'
                              of the root in place of the softmax above.
                              (4) Selection at depth > 0 of a descent: the child of the largest
                                f64(pi'(a)) + (-(f64(N(a)) / f64(1 + S)))
                              compared as float64, the lowest edge on ties; a NaN score is never the largest, and the game fails
                              when every score is NaN.  PUCT is not consulted below the root.  Depth 0 (sequential halving), the
                              path, the counters, expansion and backup are unchanged; so is yy_mcts_root_gumbel_action. */

typedef void *yy_stream_t;

const char *yy_last_error(void);
int yy_version(void);

/* ------------------------------------------------------------------ stateless rules kernels */

/* YinYangGame.getValidMoves(board, player)  (yin_yang_game.py:60-78 over
 * yin_yang_logic.py:31-128).  out_mask: uint8 [G,A], 1 = legal.  players: int8 [G]. */
int yy_rules_valid_mask(const int8_t *boards, const int8_t *players, int G, int R, int C,
                        uint32_t flags, uint8_t *out_mask, yy_stream_t stream);

/* YinYangGame.getNextState(board, player, action)  (yin_yang_game.py:39-58,
 * yin_yang_logic.py:24-29): place iff legal IN PLACE, then players[g] = -players[g] regardless.
 * placed: uint8 [G] (may be NULL). */
int yy_rules_step(int8_t *boards, int8_t *players, const int32_t *actions, int G, int R, int C,
                  uint32_t flags, uint8_t *placed, yy_stream_t stream);

/* YinYangGame.getGameEnded(board, player)  (yin_yang_game.py:80-110): out float64 [G] holding
 * exactly the reference's values 0, +1, -1, 0.0001.  counts: int32 [G,2] = count_pieces()
 * (yin_yang_logic.py:130-134), may be NULL. */
int yy_rules_game_ended(const int8_t *boards, const int8_t *players, int G, int R, int C,
                        uint32_t flags, double *out, int32_t *counts, yy_stream_t stream);

/* YinYangNeuralNetwork.board_to_input(board)  (ai/neural_network.py:156-196):
 * out float32 [G,5,R,C] = [empty, black, white, row fill, column fill]. */
int yy_encode_planes(const int8_t *boards, int G, int R, int C, float *out, yy_stream_t stream);

/* Symmetry-randomised evaluation (YY_FLAG_EVAL_SYMMETRY): yy_encode_planes of every board under the symmetry drawn for it
 * from `seed` -- the row a context created with that symmetry_seed writes for the position (for the book's builder) -- and
 * the drawn symmetry itself, out int8 [G] (0 .. 7 on square boards, 0 .. 3 on others). */
int yy_encode_planes_sym(const int8_t *boards, int G, int R, int C, uint64_t seed, float *out, yy_stream_t stream);
int yy_eval_symmetry(const int8_t *boards, int G, int R, int C, uint64_t seed, int8_t *out, yy_stream_t stream);

/* Native packed form of the same rules: one game per lane on bitboards.
 * black/white: uint64 [NW][G] (word-major SoA, NW = ceil(R*C/64), bit a = cell a);
 * mask_p1/mask_m1: uint64 [NW][G] legal masks for +1 / -1; result: int8 [G] game-ended code from
 * BLACK's (+1) point of view: 0 ongoing, +1, -1, 2 = draw.  Any output may be NULL. */
int yy_rules_mask_terminal_bb(const uint64_t *black, const uint64_t *white, int G, int R, int C,
                              uint32_t flags, uint64_t *mask_p1, uint64_t *mask_m1,
                              int8_t *result, yy_stream_t stream);

/* int8 boards <-> packed bitboards (layout as above). */
int yy_pack_boards(const int8_t *boards, int G, int R, int C, uint64_t *black, uint64_t *white,
                   yy_stream_t stream);
int yy_unpack_boards(const uint64_t *black, const uint64_t *white, int G, int R, int C,
                     int8_t *boards, yy_stream_t stream);

/* ------------------------------------------------------------------ batched MCTS context
 * One context = G concurrent games searched in lockstep; replaces Node + MCTS.search/_simulate
 * (ai/mcts.py:28-225, 275-414).  Per lockstep step:
 *     yy_mcts_select        -> leaf planes for the evaluator   (mcts.py:356-362, 385-397)
 *     <policy/value CNN on planes, caller's business>
 *     yy_mcts_expand_backup <- policy, value                   (mcts.py:50-91, 406-412)
 * or the fused yy_mcts_step (= expand_backup of the previous leaves + select of the next). */

typedef struct yy_mcts_config {
    int32_t G;                 /* concurrent games */
    int32_t R, C;              /* board */
    int32_t max_sims;          /* largest num_simulations a search will run (sizes the arenas) */
    float cpuct;               /* mcts.py:231 cpuct */
    uint32_t flags;            /* YY_FLAG_* */
    int64_t edges_per_game;    /* 0 = worst case (max_sims+2)*A */
    int64_t nodes_per_game;    /* 0 = max_sims+2 */
    int32_t leaves_per_step;   /* K: descents per game per step (leaf parallelism with virtual visits); 0 and 1 = one,
                                  the reference's search.  1 < K <= 64 needs copied boards and no YY_FLAG_REUSE_* /
                                  YY_FLAG_KEEP_EVALUATIONS (create returns YY_E_UNSUPPORTED) and no book.  See below. */
    uint64_t symmetry_seed;    /* YY_FLAG_EVAL_SYMMETRY: the seed of the symmetry draw; ignored without the flag */
    double forced_playouts;    /* YY_FLAG_FORCED_PLAYOUTS: k (KataGo: 2.0); ignored without the flag */
    float fpu_reduction;       /* YY_FLAG_FPU_REDUCTION: r below the root (KataGo: 0.2); ignored without the flag */
    float fpu_reduction_root;  /* YY_FLAG_FPU_REDUCTION: r at the root (KataGo: 0 at a noised root); ignored without the flag */
    int32_t gumbel_root;       /* YY_FLAG_GUMBEL_ROOT: m, the root actions sequential halving starts from (2 .. 64; the paper: 16) */
    float gumbel_c_visit;      /* YY_FLAG_GUMBEL_ROOT: c_visit of sigma (the paper: 50); ignored without the flag */
    float gumbel_c_scale;      /* YY_FLAG_GUMBEL_ROOT: c_scale of sigma (the paper: 1.0); ignored without the flag */
} yy_mcts_config;

/* Leaf-parallel steps (leaves_per_step = K > 1).  Every select (or step) runs, per game, descents j = 0 .. K_eff-1 one after
 * another, K_eff = min(K, simulations of this search not yet started) -- computed on the device from root.visits and the count
 * set by yy_mcts_set_num_sims (or the game's own budget, yy_mcts_set_sim_budgets), so that one captured step serves every step of a search.  The tree and its statistics do not
 * change during these descents.  Descent j sees on every edge a virtual count v = the number of descents 0 .. j-1 of this step
 * that walked that edge, and scores a child with n = N + v, w = v > 0 ? f32(W - f32(v)) : W, in the float32 order of
 * mcts.py:97-145: S = sum over the children of (N + v), sq = f32(sqrt(S)), u = f32(f32(f32(cpuct*P)*sq) / f32(1+n)),
 * q = n > 0 ? f32(w / f32(n)) : 0, the largest q + u wins, the lowest action on ties.  With v = 0 this is the K = 1 formula.
 * A descent that ends on the leaf of an earlier descent of the same step (the same unexpanded edge, the same childless node,
 * the pass root) asks for no row: it shares that descent's evaluation and still counts as a simulation.  A terminal leaf asks
 * for no row either.  Rows are game-major: select / step write planes [G*K,5,R,C] and needs_eval [G*K], row g*K + j for descent
 * j of game g, needs_eval = 1 only for the first occurrence of a leaf that needs an evaluation (counters[0], TC_EVALS, counts those rows);
 * expand_backup / step read policy [G*K,A] and value [G*K].  After the evaluator, for j = 0 .. K_eff-1 in order: the first
 * occurrence of a leaf expands it as with K = 1, then every descent backs its value up along its own path as with K = 1.  So
 * every step adds K_eff visits to the root, and root.visits == num_sims after ceil(num_sims / K) steps.  yy_mcts_begin writes
 * the root planes to row g*K and yy_mcts_expand_root reads policy row g*K (the noise stays [G,A]). */

typedef struct yy_mcts yy_mcts; /* opaque */

/* sync. Allocates the arenas in HBM on the current device. */
int yy_mcts_create(const yy_mcts_config *cfg, yy_mcts **out);
int yy_mcts_destroy(yy_mcts *ctx);
/* bytes of HBM held by the context (host out); with K > 1 it includes the per-descent paths and leaf records */
int yy_mcts_memory_bytes(const yy_mcts *ctx, uint64_t *out);
/* Simulations of the searches begun after this call (0 = max_sims, the default); host only, read by yy_mcts_begin.  Used
 * by leaf-parallel contexts (K > 1) to run the last step of a search with fewer descents; K = 1 ignores it. */
int yy_mcts_set_num_sims(yy_mcts *ctx, int32_t num_sims);
/* Per-game simulation budgets of the searches begun after this call: budgets_dev = DEVICE int32 [G], or NULL = every game
 * gets the scalar again (yy_mcts_set_num_sims at K > 1; no limit but the caller's step count at K = 1: today's search).  Host
 * only: it stores the pointer, which every following yy_mcts_begin reads on its stream -- the array must stay valid until then
 * -- and copies, clamped on the device to 0 .. max_sims, into the context.  The step kernels only see that copy, so one
 * captured step serves every budget array.  K = 1: a game whose root holds budget[g] visits selects nothing (needs_eval[g] =
 * 0, no arena and no counter touched, like an inactive game) and the following expand_backup / step skips it.  K > 1: K_eff =
 * min(K, budget[g] - simulations started).  Budget 0 = the root expansion only.  The caller issues the steps of the largest
 * budget; games of smaller budgets idle through the rest. */
int yy_mcts_set_sim_budgets(yy_mcts *ctx, const int32_t *budgets_dev);

/* Tree reuse across moves (not in the reference's search; opt-in: a context that never calls this behaves as before).
 * Re-root every game's tree at the child of its root under actions[g] (DEVICE int32 [G]); to be called after a completed
 * search (no select pending: else YY_E_STATE) and before the next yy_mcts_begin; may be called several times in a row (own
 * move, then the opponent's).  kept_visits: DEVICE int32 [G] or NULL: the visits the new root carries, 0 = nothing kept.
 * A game keeps its subtree when it is active without error, 0 <= actions[g] < A, its root has an edge with that action whose
 * child is a node that is not terminal and has children; every other game (action -1, an unvisited child, a pass root, ...)
 * is left with an empty tree.  For a kept game the subtree is compacted, in place, to the front of the game's arenas (the
 * child becomes node 0; edges stay contiguous per node and in ascending action; priors, visits, value sums, node flags, stored
 * values and boards are carried bit for bit), root visits = the edge's N, root value sum = the edge's W (float32).
 * The next yy_mcts_begin consumes the mark and continues from the kept tree only if boards[g] / root_players[g] are the kept
 * node's and the game is active -- else it builds the fresh root of every search.  On a kept root yy_mcts_expand_root ignores
 * the policy row and mixes a non-zero noise row into the STORED priors of the root's edges, p = f32(f64(f32(1-eps)*P) +
 * eps*noise); the search then tops the root up: it stops at root.visits == budget (the game's entry of
 * yy_mcts_set_sim_budgets, else the scalar of yy_mcts_set_num_sims -- which K = 1 honours for kept games only), and a kept
 * root that already holds its budget selects nothing.  The caller issues the steps of the full budget.
 * Copied boards and leaves_per_step <= 1 only: YY_FLAG_ALIASED or K > 1 return YY_E_UNSUPPORTED.  The first call allocates
 * the context's remap array (int32 [G, nodes_per_game], counted by yy_mcts_memory_bytes from then on). */
int yy_mcts_advance(yy_mcts *ctx, const int32_t *actions, int32_t *kept_visits, yy_stream_t stream);

/* MCTS.search prologue (mcts.py:288-295): fresh root per game from boards int8 [G,R,C] and
 * root_players int8 [G]; active uint8 [G] (NULL = all active; inactive games are skipped by every
 * later call).  Writes the root planes float32 [G,5,R,C] for evaluator call #0. */
int yy_mcts_begin(yy_mcts *ctx, const int8_t *boards, const int8_t *root_players,
                  const uint8_t *active, float *planes_out, yy_stream_t stream);

/* Root expansion (mcts.py:297-317).  policy float32 [G,A] = softmax output of call #0 (the value
 * is discarded by the reference).  noise: NULL, or float64 [G,A] holding each game's Dirichlet
 * draw scattered to its legal action indices; priors become
 * f32( f64(f32(1-eps) * p) + eps*noise )  exactly as mcts.py:310-312 evaluates under numpy 2.
 * A game whose noise row is all zero keeps its raw priors (add_exploration_noise=False). */
int yy_mcts_expand_root(yy_mcts *ctx, const float *policy, const double *noise, double eps,
                        yy_stream_t stream);
/* The same root expansion with the evaluator's value of call #0, float32 [G] (row g*K with K leaves per step): a context with
 * YY_FLAG_GUMBEL_INTERIOR keeps it in the root record (and needs this form); any other context discards it as above. */
int yy_mcts_expand_root_value(yy_mcts *ctx, const float *policy, const float *value, const double *noise, double eps,
                              yy_stream_t stream);

/* Selection + leaf state (mcts.py:356-399 up to the predict call): PUCT descent in float32
 * (mcts.py:97-145), place-if-legal, terminal test and legal mask of the new position, and the 5
 * input planes written to row g of planes_out float32 [G,5,R,C].  needs_eval uint8 [G] = 1 when
 * row g must be evaluated (0: terminal leaf revisited, or inactive). */
int yy_mcts_select(yy_mcts *ctx, float *planes_out, uint8_t *needs_eval, yy_stream_t stream);

/* Expansion + backup (mcts.py:50-91, 147-156, 406-412) for the leaves chosen by the last select.
 * policy float32 [G,A], value float32 [G] (rows with needs_eval == 0 are ignored). */
int yy_mcts_expand_backup(yy_mcts *ctx, const float *policy, const float *value,
                          yy_stream_t stream);

/* Fused: expand_backup(policy, value) then select(planes_out, needs_eval) in ONE launch. */
int yy_mcts_step(yy_mcts *ctx, const float *policy, const float *value, float *planes_out,
                 uint8_t *needs_eval, yy_stream_t stream);

/* Root child visit counts int32 [G,A] (Node.get_children_visit_counts, mcts.py:168-181);
 * optional per-child value_sum float32 [G,A] and prior float32 [G,A] (NULL to skip). */
int yy_mcts_root_counts(yy_mcts *ctx, int32_t *counts, float *child_w, float *child_p,
                        yy_stream_t stream);

/* Node.get_children_distribution(T) for T == 1 (counts/sum, uniform 1/A when all zero) or T == 0
 * (uniform over the arg-max set) in float64 [G,A]  (mcts.py:183-215). */
int yy_mcts_root_policy(yy_mcts *ctx, int temperature_is_zero, double *pi, yy_stream_t stream);

/* root.visits int32 [G] and root.value_sum float64 [G] (mcts.py:39-40). */
int yy_mcts_root_stats(yy_mcts *ctx, int32_t *visits, double *value_sum, yy_stream_t stream);

/* The board each game's root refers to after the search, int8 [G,R,C]: unchanged in copied mode,
 * the mutated caller board in aliased mode. */
int yy_mcts_get_boards(yy_mcts *ctx, int8_t *boards, yy_stream_t stream);

/* Test and tool support only, no part of a search: the trees as they stand.  caps (HOST int64 [2], or NULL) = {node records, edge records} per game;
 * nodes uint32 [G, caps[0], 4] = per node {first edge, k | flags << 16 | player << 24, terminal or proven value (f32 bits), the
 * evaluator's value (f32 bits)}; edges uint32 [G, caps[1], 4] = per edge {prior (f32 bits), N, W (f32 bits), child | action <<
 * 24; child 0xFFFFFF = none}; sizes int32 [G, 2] = {nodes, edges} in use.  Device pointers, each may be NULL; async copies. */
int yy_mcts_tree(yy_mcts *ctx, uint32_t *nodes, uint32_t *edges, int32_t *sizes, int64_t *caps, yy_stream_t stream);

/* sync. Host outputs: number of games that failed in ANY search since the previous status call -- arena overflow,
 * NaN priors or a NaN value from the evaluator; such a game stops searching, and the flag is sticky: yy_mcts_begin
 * does not clear it, only this call does -- and
 * counters[8] = {evaluator rows requested, selection levels walked, children scanned during
 * selection, children created, terminal revisits, nodes created, pass values reused, evaluation-cache hits} accumulated since create
 * or the last yy_mcts_reset_counters: TC_EVALS .. TC_TABLE_HITS of csrc/yy_tree.h, which names every counter of this and the
 * readers below.  Returns YY_E_ARENA if any game overflowed. */
int yy_mcts_status(yy_mcts *ctx, int32_t *n_overflow, uint64_t *counters);
int yy_mcts_reset_counters(yy_mcts *ctx, yy_stream_t stream);
/* sync. YY_FLAG_FORCED_PLAYOUTS: the root descents, over all games, that took a forced edge since create or the last
 * yy_mcts_reset_counters (host out; 0 without the flag). */
int yy_mcts_forced_descents(yy_mcts *ctx, uint64_t *out);
/* YY_FLAG_SOLVER.  yy_mcts_root_proven: the proven status of every game's root, root int8 [G], and of the root's children by
 * action, child int8 [G,A] (0 none -- also: no such child yet --, 1 WIN, 2 LOSS, 3 DRAW, each for the side to move AT THAT NODE:
 * a child that is LOSS is a winning move); all 0 without the flag and for an inactive game.  yy_mcts_solver_counters: sync;
 * host out[3] = {nodes proven by propagation, descents that ended on a proven node below the root, searches whose root became
 * proven} over all games since create or the last yy_mcts_reset_counters (0 without the flag).  Both after a completed search:
 * YY_E_STATE with a select or a root expansion pending. */
int yy_mcts_root_proven(yy_mcts *ctx, int8_t *root, int8_t *child, yy_stream_t stream);
int yy_mcts_solver_counters(yy_mcts *ctx, uint64_t *out);
/* YY_FLAG_GUMBEL_ROOT (YY_E_UNSUPPORTED without the flag).  yy_mcts_set_gumbel: rows_dev = DEVICE float32 [G,A], the Gumbel
 * variable of every action at every game's root (yy_selfplay_root_gumbel draws them), owned by the caller.  Host only, like
 * yy_mcts_set_sim_budgets: it stores the pointer, which the root expansions read on their stream, so the array must stay
 * valid and in place, and be set before the first step is captured; the caller rewrites its contents before every search.
 * yy_selfplay_run_create points the context at the run's own rows.  yy_mcts_root_gumbel: out float32 [G,A] = s0 by action, NaN
 * for an action without a root edge and for an inactive game.  yy_mcts_root_gumbel_action: out int32 [G] = the Gumbel winner
 * (above), -1 for an inactive game and for a root without children. */
int yy_mcts_set_gumbel(yy_mcts *ctx, const float *rows_dev);
int yy_mcts_root_gumbel(yy_mcts *ctx, float *out, yy_stream_t stream);
int yy_mcts_root_gumbel_action(yy_mcts *ctx, int32_t *out, yy_stream_t stream);
/* Shared book of pre-evaluated positions.  Every self-play game starts from the empty board, so the searches of the first plies
 * of ALL games walk the same few hundred thousand positions (8x8: 770 232 positions with <= 8 stones are reachable).  The
 * caller enumerates them, evaluates them once in large batches with the SAME evaluator the searches use, and hands the table
 * to the contexts: a leaf with at most `max_stones` stones is looked up there first (same hash / probe / full key compare as
 * the per-game cache) and, on a hit, needs no evaluator row (counters[7], TC_TABLE_HITS).  Read-only during play, so no atomics on the
 * lookup side; arrays stay owned by the caller and must outlive the context (or be unset with meta = NULL).
 *   yy_book_insert: keys u64 [n, 2*NW] (black words, white words), distinct -> slot_of i32 [n] (-1 = no free slot within
 *   the probe window); fills meta u32 [cap] (zeroed by the caller, cap a power of two) and table_keys u64 [cap, 2*NW].
 *   The caller then scatters its value f32 [cap] and policy f32 [cap, A] rows by slot_of. */
int yy_book_insert(const uint64_t *keys, int n, int R, int C, uint32_t *meta, uint64_t *table_keys, int64_t cap,
                   int32_t *slot_of, yy_stream_t stream);
int yy_mcts_set_book(yy_mcts *ctx, const uint32_t *meta, const uint64_t *keys, const float *value, const float *policy,
                     int64_t cap, int max_stones);
/* Forget every cached evaluation (YY_FLAG_REUSE_TRANSPOSITIONS / YY_FLAG_KEEP_EVALUATIONS): to be called when the evaluator
 * (the network) changes between two searches of one context.  Async on `stream`. */
int yy_mcts_cache_clear(yy_mcts *ctx, yy_stream_t stream);
/* Shared evaluation table: the dynamic form of the book.  The games of ONE context fill it while they play: every fresh
 * evaluator row of a non-root leaf is inserted (next to the game's own cache), and a leaf whose position any game of the
 * context had evaluated in an EARLIER launch takes the stored policy row and value instead of an evaluator row
 * (counters[7], TC_TABLE_HITS, and hits, TC_SH_HITS, in yy_mcts_shared_counters).  Lookup order: book, the game's own cache, the shared table.
 *   meta u32 [slots] (zeroed by the caller; 0 = never used, else the step stamp of the launch that inserted the entry),
 *   keys u64 [slots, 2*NW], value f32 [slots], policy f32 [slots, A], slots a power of two in 64 .. 2^30,
 *   stamp u32 [1] in device memory: the step stamp.  The context advances it by one thread in a launch of its own in front
 *   of every tree-step launch (only while a table is set) and keeps it non-zero; the tree kernel reads it once per wave.
 * An entry that carries the current stamp is passed over by lookups -- its key and row may still be in flight in another
 * workgroup -- so everything a lookup trusts was written by a launch that completed earlier on the same stream: the kernel
 * boundary publishes, and the slot claim (one atomicCAS, as in yy_book_insert) is the only atomic.  Insert-only (the
 * replacing form below is the one that deduplicates and evicts): no eviction, no overwrite; a full probe window drops the insert (counted); two games inserting one position in one launch
 * take two slots.  The arrays stay owned by the caller and must outlive the context (or be unset with meta = NULL); ONE
 * table belongs to ONE context on ONE stream, and holds the outputs of one evaluator under one symmetry setting.  Set it
 * with no select pending and before the first step is captured.  YY_E_UNSUPPORTED for YY_FLAG_ALIASED and
 * leaves_per_step > 1.  yy_mcts_shared_evaluations_clear zeroes the meta of the context's table (async on `stream`): the table
 * is empty again.  Like the setter it needs a context with no select or root expansion pending (YY_E_STATE otherwise): a
 * pending leaf may name a slot, and an emptied slot could be claimed and rewritten in the launch that reads it.  A context
 * armed by yy_selfplay_run_arm stays pending.
 * yy_mcts_shared_counters (sync; host out [3]): leaves served, rows inserted, inserts dropped, over all games since create
 * or the last yy_mcts_reset_counters. */
int yy_mcts_set_shared_evaluations(yy_mcts *ctx, uint32_t *meta, uint64_t *keys, float *value, float *policy, int64_t slots,
                                   uint32_t *stamp);
int yy_mcts_shared_evaluations_clear(yy_mcts *ctx, yy_stream_t stream);
int yy_mcts_shared_counters(yy_mcts *ctx, uint64_t *out);
/* The replacing form of the shared evaluation table: one slot per position and launch, and eviction, so that a table of a fixed
 * size serves a run of any length.  Everything above holds -- lookup order, the stamp, what a lookup trusts, the refusals,
 * the owner of the arrays, yy_mcts_shared_evaluations_clear (which zeroes the claim words) -- except "insert-only".
 *   claim u64 [slots] (zeroed by the caller) in the place of meta: low half = the stamp of the inserting launch (0 = never used,
 *     0xFFFFFFFF = TOMBSTONE, an evicted slot; both are free, and the stamp takes neither value), high half = a tag of the
 *     position, the half of its hash that indexing does not use.  Slot and tag are taken in ONE 64-bit atomicCAS on the value
 *     observed, still the only atomic of the option.
 *   last_hit u32 [slots]: the stamp of the last launch that served the entry (a plain store by the lookup that hits; its
 *     insert stamp until then).
 *   sweep_state u64 [8] (zeroed by the caller): the sweeps' counters and the stamp the last evicting sweep recorded.
 * One inserter per position and launch: an inserter that meets a slot claimed in ITS launch with ITS tag stops and counts a
 * duplicate; of all games that insert one position in one launch exactly one takes a slot.  (Two different positions with one
 * tag in one probe window and one launch cost one insert, nothing else: lookups compare keys in full.)  A lookup passes over
 * a TOMBSTONE instead of ending its probe there.
 * yy_mcts_shared_evaluations_sweep enqueues the eviction on `stream` (no host sync; YY_E_STATE for a context without a replacing
 * table, nothing is launched): a counting pass over the claim words, then an evicting pass that does nothing while the live
 * entries are <= high_water_slots and else turns every entry into a TOMBSTONE whose insert stamp and last-hit stamp are both
 * older (modulo 2^32, on ages) than the stamp recorded by the last sweep above the mark, and records the current stamp for
 * the next one; the first sweep above the mark only records.  Second chance over the whole table: what was inserted or
 * served since the last evicting sweep stays.  It must run on the context's stream BETWEEN two tree-step launches, never
 * captured into a step; it may run with selects pending -- a pending leaf found its slot in the latest launch, so the slot's
 * last-hit stamp is the current one, which no cutoff is newer than -- which is what excludes the hazard named above for
 * the clear.  No eviction or duplicate decision changes a game: a table only returns the evaluator's own row for a position.
 * yy_mcts_shared_counters_ex (sync; host out [6]): hits, inserts, dropped, duplicates (since create or the last
 * yy_mcts_reset_counters), evicted (since the table was set or the last yy_mcts_reset_counters), live entries left by the
 * last sweep; the last three are 0 for an insert-only table. */
int yy_mcts_set_shared_evaluations_replacing(yy_mcts *ctx, uint64_t *claim, uint32_t *last_hit, uint64_t *keys, float *value,
                                             float *policy, int64_t slots, uint32_t *stamp, uint64_t *sweep_state);
int yy_mcts_shared_evaluations_sweep(yy_mcts *ctx, int64_t high_water_slots, yy_stream_t stream);
int yy_mcts_shared_counters_ex(yy_mcts *ctx, uint64_t *out);

/* ------------------------------------------------------------------ evaluator epilogue
 * Batched leaf evaluator fast path (the reference evaluates one board per call:
 * ai/neural_network.py:94-123, 125-154).  In-place fused epilogue of one convolution of the tower
 * on a channels-last bf16 activation tensor x [rows, C] (rows = G*R*Cb cells):
 *     x = relu?( x + bias[c] (+ residual) )         bias float32 [C]; residual bf16 [rows, C] or NULL
 * (eval-mode BatchNorm is folded into the convolution weights and this bias on the host). */
int yy_nn_bias_act_bf16(void *x, const float *bias, const void *residual, int64_t rows, int C,
                        int relu, yy_stream_t stream);

/* The residual tower of the evaluator (stem + residual blocks, ai/neural_network.py:16-33, 105-110)
 * as ONE LDS-resident MFMA kernel: planes float32 [G,5,R,R] -> out bf16 [G,R,R,128] (channels-last
 * activations after the last block).  weights: bf16 chunks in fragment order and bias float32
 * [n_layers,128], both produced on the host from the module with eval-mode BatchNorm folded
 * (network.pack_tower).  n_layers = 1 + 2*res_blocks <= 21.  Boards 6x6, 8x8 or 12x12 (planes
 * [G,5,R,R], out [G,R,R,128]) and 128 channels; anything else returns YY_E_UNSUPPORTED and the
 * caller uses library convolutions + yy_nn_bias_act_bf16.  The launch picks the workgroup shape from G (8x8: one, two
 * or four boards per workgroup, so that small batches still spread over the chip); a board's output bits do not depend on G. */
int yy_nn_tower_bf16(const float *planes, const void *weights, const float *bias, void *out, int G,
                     int R, int C, int channels, int n_layers, yy_stream_t stream);

/* Same kernel, with the policy_conv / value_conv 1x1 head convolutions + BatchNorm + ReLU
 * (neural_network.py:113, 118) fused behind the tower: out_heads bf16 [G,2,32,R*R] = [policy features,
 * value features] in the reference's NCHW flatten order (channel*R*R + cell, :114 / :119), ready for
 * policy_fc / value_fc1.  weights holds one extra 16 KB chunk ([ks 8][nt 2][h 2][c 32][j 8]) and bias
 * one extra row [n_layers] = [policy bias 32 | value bias 32 | 0...]. */
int yy_nn_tower_heads_bf16(const float *planes, const void *weights, const float *bias,
                           void *out_heads, int G, int R, int C, int channels, int n_layers,
                           yy_stream_t stream);

/* The residual tower in EXACT float32 on the f32-input MFMA (v_mfma_f32_32x32x2_f32; a k-ordered fmaf chain,
 * bitwise f32): the fast form of the fp32 parity evaluator.  planes float32 [G,5,8,8] -> out float32 [G,8,8,128]
 * (channels-last activations after the last block); weights float32 chunks in fragment order and bias float32
 * [n_layers,128] from network.pack_tower_f32.  8x8 boards, 128 channels. */
int yy_nn_tower_f32(const float *planes, const void *weights, const float *bias, float *out, int G,
                    int R, int C, int channels, int n_layers, yy_stream_t stream);

/* Head finish (neural_network.py:115, 120-121, 152): h bf16 [G, A+H] = policy logits then value_fc1
 * outputs (bias added); policy float32 [G,A] = softmax(logits); value float32 [G] =
 * tanh(relu(hidden) . w2 + b2) with w2 float32 [H], b2 float32 [1]. */
int yy_nn_head_finish_bf16(const void *h, int G, int A, int H, const float *w2, const float *b2,
                           float *policy, float *value, yy_stream_t stream);

/* The residual tower at FLOAT32 accuracy on the F16 matrix cores ("split-f16"): activations and weights are held as
 * hi = f16(x), lo = f16(x - hi) (22 significant bits); per output element one f32 accumulator takes w_hi*x_hi and a second
 * one w_lo*x_hi + w_hi*x_lo; bias / residual / ReLU in f32.  To keep the lo parts in float16's normal range the weights are
 * stored times 2^weight_exp and the activations (and the bias rows of the tower) live times 2^act_exp -- exact scalings chosen
 * by the packers in network.py.  Agrees with a float64 evaluation to ~5e-7 of scale, like the float32 module itself.
 * Replaces ai/neural_network.py:94-119 (float32 on the CPU in the reference).
 *
 * yy_nn_tower_f16x3_regs = the round-2 form (csrc/yy_tower_h3r.hip: v_mfma_f32_32x32x16_f16, boards 6x6 / 8x8 / 12x12,
 * 128 channels), kept as the A/B partner of yy_nn_tower_g below: weights / head_w in the wave-major order of
 * network.pack_tower_h3r / pack_heads_h3r ([9 + 36*(n_layers-1)][8192] / [2][8192] f16); bias float32 [n_layers (+1), 128];
 * exactly one of out (float32 [G,R,R,128] tower activations) and out_heads (float32 [G,2,32,R*R] = [policy features, value
 * features] in the reference's NCHW flatten order, neural_network.py:114 / :119; needs head_w) is non-NULL; rows / n_rows
 * (device pointers, or both NULL): evaluate planes[rows[i]] for i < *n_rows into dense row i, workgroups past *n_rows exit. */
int yy_nn_tower_f16x3_regs(const float *planes, const void *weights, const void *head_w, const float *bias,
                           float *out, float *out_heads, const int32_t *rows, const int32_t *n_rows, int G,
                           int R, int C, int channels, int n_layers, int weight_exp, int head_exp,
                           int act_exp, yy_stream_t stream);

/* The GENERAL form of the float32-accurate tower (csrc/yy_tower_g.hip; the form the engine uses): any R x C board with at
 * most 144 cells (train_alphazero.py:35-36 takes any --rows / --cols), 32 / 64 / 96 / 128 channels and up to 10 residual
 * blocks (ai/neural_network.py:39), on v_mfma_f32_16x16x32_f16: a workgroup of channels/32 waves evaluates `boards` boards =
 * nb blocks of 16 (board, cell) columns (boards * R * C <= 16 * nb; nb one of yy_nn_tower_g_forms).  Same split-f16 numerics
 * and the same I/O conventions as yy_nn_tower_f16x3_regs: weights = f16 chunks [9 + 9*(channels/32)*(n_layers-1)]
 * [channels*64] in MFMA operand order (network.pack_tower_g) times 2^weight_exp; bias float32 [n_layers, channels] times
 * 2^act_exp; exactly one of out (float32 [G,R,C,channels]) and out_heads (float32 [G,2,32,R*C]: needs head_w = f16
 * [4][channels/32][2][512] times 2^head_exp and head_bias float32 [64], network.pack_heads_g) is non-NULL; rows / n_rows as
 * above.  The launch only computes when gate_lo < live rows <= gate_hi (-1, INT_MAX: always), so that two forms can be
 * enqueued and the one fitting the device-side row count runs.  A row's results do not depend on nb, boards or its position
 * in the batch (same accumulation order per output element in every form).  layout 0: where boards * C == 16 and nb == R
 * (8x8 with two boards per workgroup) the kernel lays a block out as one row of every board and skips the MFMAs of the taps
 * that only see the zero border; at 128 channels and nb = 8 that form runs on a 2x2 grid of waves (each 64 channels x half
 * the blocks).  layout 1 forces the plain column layout, layout 2 the row-aligned blocks on the one-wave-per-32-channels grid
 * (same bits in every layout; the A/B partners for timing).  Replaces ai/neural_network.py:94-119. */
int yy_nn_tower_g(const float *planes, const void *weights, const void *head_w, const float *bias, const float *head_bias,
                  float *out, float *out_heads, const int32_t *rows, const int32_t *n_rows, int G, int R, int C,
                  int channels, int n_layers, int weight_exp, int head_exp, int act_exp, int nb, int boards, int gate_lo,
                  int gate_hi, int layout, yy_stream_t stream);
/* the nb values yy_nn_tower_g is built for at this channel count: writes up to 8 ints, returns how many (0: unsupported) */
int yy_nn_tower_g_forms(int channels, int *nb_out);
/* Test hook for the ReLU of yy_nn_tower_g's 2x2-grid form: over the float32 bit patterns start .. start + count - 1 (wrapping
 * at 2^32), counts into counts[0] (device uint32, accumulated) the inputs where it differs from the NaN-keeping ReLU of the other
 * forms (bits differ for a non-NaN input, or a NaN input does not give a NaN) and lowers counts[1] to the smallest such pattern. */
int yy_nn_tower_g_relu_check(uint32_t start, uint32_t count, uint32_t *counts, yy_stream_t stream);

/* policy_fc and value_fc1 (neural_network.py:115, :120; float32 on the CPU in the reference) as one split-f16 GEMM kernel of
 * our own (csrc/yy_fc_heads.hip), on the dense feature rows a tower launch wrote: feats float32 [G,2,K] (K = 32*R*C) ->
 * logits float32 [G,A] = policy_fc(feats[:,0]), hidden float32 [G,H] = value_fc1(feats[:,1]), bias added.  wpk / bias / jobs
 * from network.pack_fc_heads: jobs int32 [n_jobs][4] = (head, first output, outputs <= 64, first 8 KB weight block), weights f16
 * [n_jobs][ceil(K/128)*4][4][2][64][8] times 2^weight_exp; features are split as x * 2^act_exp = hi + lo.  n_rows (device, or
 * NULL = G): rows past *n_rows are neither read nor written.  Every output element is one fixed k-ascending MFMA chain (no
 * split-K, no batch-size dependent tiling): a row's outputs do not depend on G, *n_rows or its position in the batch, which
 * is what lets the search reuse evaluations across launches of different sizes (YY_FLAG_REUSE_*). */
int yy_nn_fc_heads_f16x3(const float *feats, const void *wpk, const float *bias, const int32_t *jobs, int n_jobs,
                         float *logits, float *hidden, const int32_t *n_rows, int G, int K, int A, int H,
                         int weight_exp, int act_exp, yy_stream_t stream);

/* float32 head finish (neural_network.py:115, 120-121, 152): logits float32 [G,A] (policy_fc output, bias added), hidden
 * float32 [G,H] (value_fc1 output, bias added) of dense row i -> policy[g] = softmax(logits[i]),
 * value[g] = tanh(relu(hidden[i]) . w2 + b2), g = rows ? rows[i] : i, for i < (n_rows ? *n_rows : G). */
int yy_nn_head_finish_f32(const float *logits, const float *hidden, int G, int A, int H, const float *w2,
                          const float *b2, const int32_t *rows, const int32_t *n_rows, float *policy,
                          float *value, yy_stream_t stream);

/* Leaf-batch compaction for the lockstep step: rows[0 .. *n) = ascending indices g < G with flags[g] != 0 (the games whose
 * selected leaf needs an evaluation: yy_mcts_select / yy_mcts_step write these flags; a terminal revisit does not,
 * mcts.py:365-366).  All pointers are device pointers. */
int yy_compact_rows(const uint8_t *flags, int G, int32_t *rows, int32_t *n, yy_stream_t stream);

/* ------------------------------------------------------------------ episode-loop random draws
 * Counter-based (Philox4x32-10) replacements of the two draws the reference takes from numpy's global stream (and the
 * playout-cap draw, which the reference does not have), keyed by
 * (seed, GLOBAL game index, ply, purpose, element) so that a game's transcript does not depend on its slot, on the batch
 * size, on refill order or on the number of ranks.  All pointers are device pointers.
 *
 * yy_selfplay_root_noise: np.random.dirichlet([alpha] * k) over the k legal moves (ai/mcts.py:298-312), for the games with
 * draw[g] != 0: noise float64 [G,A], zero rows elsewhere (yy_mcts_expand_root treats an all-zero row as "no noise"). */
int yy_selfplay_root_noise(uint64_t seed, const int64_t *game_id, const int32_t *ply, const uint8_t *draw,
                           const uint8_t *mask, int G, int A, double alpha, double *noise, yy_stream_t stream);

/* yy_selfplay_root_gumbel: Gumbel root search (YY_FLAG_GUMBEL_ROOT).  rows float32 [G,A]: rows[g,a] = f32(-log(-log(u))) in
 * float64, u the 53-bit uniform of the first two words of the block keyed (seed, game_id[g], ply[g], purpose 4, element a),
 * strictly inside (0, 1): u == 0 is replaced by 2^-54.  Every game and every action is drawn; what yy_mcts_set_gumbel takes. */
int yy_selfplay_root_gumbel(uint64_t seed, const int64_t *game_id, const int32_t *ply, int G, int A, float *rows,
                            yy_stream_t stream);

/* yy_selfplay_sample_actions: the move choice of SelfPlayWorker.play_game (ai/self_play.py:143-160) for the games with
 * searching[g] != 0 (action -1 otherwise): ply < temperature_threshold -> sample from pi * mask renormalised (uniform over
 * the legal moves when that sum is 0); else a uniformly random member of argmax(pi).  pi float64 [G,A], mask uint8 [G,A]. */
int yy_selfplay_sample_actions(uint64_t seed, const int64_t *game_id, const int32_t *ply,
                               const uint8_t *searching, const double *pi, const uint8_t *mask, int G, int A,
                               int temperature_threshold, int32_t *action, yy_stream_t stream);

/* yy_selfplay_draw_budgets: playout-cap randomisation.  One uniform u in [0, 1) per game with searching[g] != 0, keyed (seed,
 * game_id[g], ply[g], purpose 3, element 0): is_full[g] = u < p_full, budgets[g] = is_full ? full_sims : fast_sims.  Games that
 * are not searching get budget 0 and is_full 0.  budgets int32 [G] is what yy_mcts_set_sim_budgets takes; is_full uint8 [G]. */
int yy_selfplay_draw_budgets(uint64_t seed, const int64_t *game_id, const int32_t *ply, const uint8_t *searching, int G,
                             double p_full, int full_sims, int fast_sims, int32_t *budgets, uint8_t *is_full,
                             yy_stream_t stream);

/* ------------------------------------------------------------------ free-running self-play (not in the reference; opt-in)
 * The move of the episode loop as a device kernel inside the search step (csrc/yy_selfplay_move.hip): a game whose search is
 * complete -- no pending leaf, root.visits == its budget -- plays its move in the same step and sets up the root of its next
 * search, while the other games of the context keep simulating.  One step is
 *     <evaluator on planes, rows with needs_eval != 0>  ->  yy_mcts_step_selfplay
 * and a move costs budget + 1 steps of that game only.  A game's transcript is the lockstep engine's bit for bit: pi, the
 * example record, the move draw (yy_selfplay_sample_actions), getNextState, getGameEnded, up to two passes at the new position
 * (flip on no move, end on the second, 0 -> 1e-4), the root prologue of yy_mcts_begin, the playout-cap draw
 * (yy_selfplay_draw_budgets) and, at ply 0 with epsilon > 0, the noise row (yy_selfplay_root_noise; zeros at every other ply)
 * are the same device functions.  A finished game's examples are labelled (z by player against the final player) and appended
 * to the run's example buffer (rows reserved with one atomic add), and the run's next game starts in the slot from the empty
 * board, black to move, with id first_game_index + k * stride (k from an atomic counter); past the target the slot goes idle.
 * A game whose search failed (yy_mcts_status) is abandoned, its examples dropped, counted, and its slot refilled.
 * Needs copied boards and leaves_per_step <= 1: else YY_E_UNSUPPORTED.  Re-rooting (yy_mcts_advance) is not offered here. */
typedef struct yy_selfplay_config {
    uint64_t seed;                   /* key of the per-game counter streams */
    double dirichlet_alpha;          /* positive and finite when dirichlet_epsilon > 0 */
    double dirichlet_epsilon;        /* 0: no noise, the step passes no noise array */
    double full_search_probability;  /* playout cap: P (with fast_simulations > 0) */
    int32_t temperature_threshold;
    int32_t num_simulations;         /* budget of a (full) search, 1 .. max_sims of the context */
    int32_t fast_simulations;        /* 0 = no playout cap; else 1 .. num_simulations */
    int32_t reserved;
    int64_t example_capacity;        /* rows of the example buffer; a run needs at most num_games * (R*C + 2) */
} yy_selfplay_config;

typedef struct yy_selfplay_run yy_selfplay_run; /* opaque; one per context */

/* sync. Allocates, on the current device, the per-slot state (board, player, ply, game id, example history), the noise array
 * float64 [G,A], the counters and the example buffer. */
int yy_selfplay_run_create(yy_mcts *ctx, const yy_selfplay_config *cfg, yy_selfplay_run **out);
int yy_selfplay_run_destroy(yy_selfplay_run *run);
/* Starts a run of num_games games: counters and example buffer reset, game j < G starts in slot j (root pending, planes in row
 * j, needs_eval[j] = 1), the other slots idle.  planes float32 [G,5,R,C] and needs_eval uint8 [G] are the step's. */
int yy_selfplay_run_arm(yy_mcts *ctx, yy_selfplay_run *run, int64_t num_games, int64_t first_game_index, int64_t stride,
                        float *planes, uint8_t *needs_eval, yy_stream_t stream);
/* One step: yy_mcts_step's launch with the run's noise array (only a root expansion mixes noise) + the move kernel.  Two
 * launches, no host read: capturable.  policy float32 [G,A] / value float32 [G] of the rows flagged by the previous call. */
int yy_mcts_step_selfplay(yy_mcts *ctx, yy_selfplay_run *run, const float *policy, const float *value, float *planes,
                          uint8_t *needs_eval, yy_stream_t stream);
/* Asynchronous copy of the counters to out (HOST, pinned; uint64 [8]) on `stream`; no device synchronisation:
 * {games started (may run past the target), finished, failed, positions searched, examples recorded, example rows reserved,
 * games whose rows did not fit the buffer (nothing is written past it; the caller must treat > 0 as an error), target}. */
int yy_selfplay_run_counters(yy_selfplay_run *run, uint64_t *out, yy_stream_t stream);
/* Rows [first, first + count) of the example buffer, in the order the games finished, copied on `stream` to states int8
 * [count,R,C], policies float32 [count,A], values float32 [count], game_id int64 [count], ply int64 [count] (device). */
int yy_selfplay_run_examples(yy_selfplay_run *run, int64_t first, int64_t count, int8_t *states, float *policies,
                             float *values, int64_t *game_id, int64_t *ply, yy_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* YY_ENGINE_H */
