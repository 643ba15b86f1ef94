// yy_tree.h -- what the kernels that run ONE GAME PER WAVEFRONT share: the wave helpers, the records of the MCTS context
// (yy_engine.hip owns the context; yy_selfplay_move.hip sets roots up and reads them inside the step), and the one copy of
// every rule and formula that both the stateless / read-out kernels and the in-step move kernel apply: the root prologue
// (k_begin), the root distribution (k_root_policy), getNextState (k_step) and getGameEnded (k_game_ended).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/yy_engine.h"
#include "yy_bitboard.h"
#include "yy_draws.h"

// ------------------------------------------------------------------------------------ helpers
__device__ __forceinline__ uint32_t rfl(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int rfl(int v) { return (int)__builtin_amdgcn_readfirstlane((uint32_t)v); }
__device__ __forceinline__ uint64_t rfl64(uint64_t v) {
    return ((uint64_t)rfl((uint32_t)(v >> 32)) << 32) | rfl((uint32_t)v);
}
__device__ __forceinline__ float rflf(float v) { return __uint_as_float(rfl(__float_as_uint(v))); }
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
// number of set bits of m below this lane's position
__device__ __forceinline__ int mbcnt(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int NW> __device__ __forceinline__ BB<NW> bb_uniform_load(const uint64_t *p) {
    BB<NW> r;
#pragma unroll
    for (int i = 0; i < NW; i++) r.w[i] = rfl64(p[i]);
    return r;
}
template <int NW> __device__ __forceinline__ void bb_store_lane0(uint64_t *p, BB<NW> b) {
    if (lane_id() == 0) {
#pragma unroll
        for (int i = 0; i < NW; i++) p[i] = b.w[i];
    }
}

// wave-cooperative: int8 board (cell per lane) -> uniform bitboards via ballot
template <int NW>
__device__ __forceinline__ void board_to_bb(const int8_t *b, int A, BB<NW> &black, BB<NW> &white) {
#pragma unroll
    for (int j = 0; j < NW; j++) {
        int cell = j * 64 + lane_id();
        int v = (cell < A) ? (int)b[cell] : 0;
        black.w[j] = __ballot(v == 1);
        white.w[j] = __ballot(v == -1);
    }
}
template <int NW>
__device__ __forceinline__ void bb_to_board(int8_t *b, int A, BB<NW> black, BB<NW> white) {
#pragma unroll
    for (int j = 0; j < NW; j++) {
        int cell = j * 64 + lane_id();
        if (cell < A)
            b[cell] = ((black.w[j] >> lane_id()) & 1) ? 1 : (((white.w[j] >> lane_id()) & 1) ? -1 : 0);
    }
}

// row r of `occ` as the low C bits (C <= 16; may straddle a word boundary)
template <int NW> __device__ __forceinline__ uint32_t bb_row_bits(BB<NW> occ, int r, int C) {
    int s = r * C, w = s >> 6, o = s & 63;
    uint64_t lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        if (i == w) lo = occ.w[i];
        if (i == w + 1) hi = occ.w[i];
    }
    uint64_t v = lo >> o;
    if (o) v |= hi << (64 - o);
    return (uint32_t)v & ((1u << C) - 1u);
}

// wave-cooperative board_to_input (neural_network.py:156-196): lane = cell, coalesced rows
template <int NW>
__device__ __forceinline__ void write_planes(float *out, const YYGeo &geo, BB<NW> black, BB<NW> white) {
    const int A = geo.A, C = geo.C;
    BB<NW> occ = black | white;
    BB<NW> col0 = bb_load<NW>(geo.col0);
#pragma unroll
    for (int j = 0; j < NW; j++) {
        int cell = j * 64 + lane_id();
        if (cell < A) {
            int r = cell / C, c = cell - r * C;
            bool bk = (black.w[j] >> lane_id()) & 1, wh = (white.w[j] >> lane_id()) & 1;
            int rowk = __popc(bb_row_bits(occ, r, C));
            int colk = bb_popc(occ & bb_shl(col0, c));
            out[cell] = (!bk && !wh) ? 1.0f : 0.0f;
            out[A + cell] = bk ? 1.0f : 0.0f;
            out[2 * A + cell] = wh ? 1.0f : 0.0f;
            out[3 * A + cell] = geo.rowfill[rowk];
            out[4 * A + cell] = geo.colfill[colk];
        }
    }
}

// ------------------------------------------------------------------------------------ symmetry-randomised evaluation
// Board symmetries by number s.  Square boards, s in 0 .. 7: np.rot90(board, s & 3) (counter-clockwise), then np.fliplr when
// s & 4.  Other boards, s in 0 .. 3: np.flipud when s & 1, np.fliplr when s & 2.  sym_apply maps a cell forwards (where it
// lands on the transformed board) or backwards (the cell of the original board that lands here).
__device__ __forceinline__ int sym_apply(const YYGeo &geo, const int s, const int cell, const bool inverse) {
    const int R = geo.R, C = geo.C;
    int r = cell / C, c = cell - r * C;
    if (R != C) {                                  // two commuting flips: the map is its own inverse
        if (s & 1) r = R - 1 - r;
        if (s & 2) c = C - 1 - c;
    } else {
        const int n1 = C - 1;
        int k = s & 3;
        if (inverse) {                             // undo the flip, then turn the remaining 4 - k quarters
            if (s & 4) c = n1 - c;
            k = (4 - k) & 3;
        }
        const int r0 = r, c0 = c;                  // one quarter turn: (r, c) -> (n - 1 - c, r)
        r = (k == 0) ? r0 : (k == 1) ? n1 - c0 : (k == 2) ? n1 - r0 : c0;
        c = (k == 0) ? c0 : (k == 1) ? r0 : (k == 2) ? n1 - c0 : n1 - r0;
        if (!inverse && (s & 4)) c = n1 - c;
    }
    return r * C + c;
}
// where cell `cell` lands under symmetry s: the entry of the transformed frame's policy row that is this action's prior
__device__ __forceinline__ int sym_cell(const YYGeo &geo, const int s, const int cell) { return sym_apply(geo, s, cell, false); }

// the symmetry the position (black, white) is evaluated under (yy_draws.h): wave-uniform
template <int NW> __device__ __forceinline__ int sym_of(const YYGeo &geo, const uint64_t seed, BB<NW> black, BB<NW> white) {
    return sp::draw_symmetry(seed, black.w, white.w, NW, sp::symmetry_group(geo.R, geo.C));
}

// wave-cooperative: the position under symmetry s.  Lane = destination cell; it tests the bit of the cell that lands there, and
// one ballot per word and colour rebuilds the uniform words.  Every lane of the wavefront must call it.
template <int NW> __device__ __forceinline__ void bb_symmetry(const YYGeo &geo, BB<NW> &black, BB<NW> &white, const int s) {
    BB<NW> nb, nw;
#pragma unroll
    for (int j = 0; j < NW; j++) {
        const int cell = j * 64 + lane_id();
        const bool on = cell < geo.A;
        const int src = on ? sym_apply(geo, s, cell, true) : 0;
        nb.w[j] = __ballot(on && bb_test(black, src));
        nw.w[j] = __ballot(on && bb_test(white, src));
    }
    black = nb;
    white = nw;
}

// the evaluator row of a position: its planes, with `sym` those of the position under its drawn symmetry
template <int NW>
__device__ __forceinline__ void write_eval_planes(float *out, const YYGeo &geo, const uint32_t sym, const uint64_t seed,
                                                  BB<NW> black, BB<NW> white) {
    if (sym) bb_symmetry<NW>(geo, black, white, sym_of<NW>(geo, seed, black, white));   // wave-uniform branch
    write_planes<NW>(out, geo, black, white);
}

// ------------------------------------------------------------------------------------ rules, one copy
// getNextState (yin_yang_game.py:39-58, yin_yang_logic.py:24-34) of `player` playing `action`: the stone is placed iff the
// action is on the board and legal; the caller flips the side to move regardless.  Returns whether it was placed.
template <int NW>
__device__ __forceinline__ bool bb_play(const YYGeo &geo, const GeoBB<NW> &gb, BB<NW> &black, BB<NW> &white, const int player,
                                        const int action) {
    bool ok = false;
    if (action >= 0 && action < geo.A) {  // yin_yang_logic.py:34 bounds check
        bool pre = bb_pre2x2(black, white, gb);
        BB<NW> m = (player == 1) ? bb_legal(black, white, pre, geo, gb) : bb_legal(white, black, pre, geo, gb);
        ok = bb_test(m, action);
    }
    if (ok) {                             // yin_yang_game.py:55-56
        if (player == 1) black = black | bb_bit<NW>(action);
        else white = white | bb_bit<NW>(action);
    }
    return ok;
}

// getGameEnded(board, player) (yin_yang_game.py:80-110) as the reference's float64: 0 ongoing, 1e-4 draw, +-1 for `player`
template <int NW>
__device__ __forceinline__ double bb_game_ended(const YYGeo &geo, const GeoBB<NW> &gb, BB<NW> black, BB<NW> white,
                                                const int player) {
    bool pre = bb_pre2x2(black, white, gb);
    BB<NW> mb = bb_legal(black, white, pre, geo, gb), mw = bb_legal(white, black, pre, geo, gb);
    int res = bb_result_black(black, white, mb, mw);
    double v = 0.0;
    if (res == 2) v = 0.0001;                                   // yin_yang_game.py:107
    else if (res != 0) v = (player == 1) ? (double)res : (double)-res;
    return v;
}

// =============================================================================== MCTS context records
enum : uint8_t { K_NONE = 0, K_TERMINAL = 1, K_EXPAND = 2, K_REEXPAND = 3, K_ROOTPASS = 4, K_ROOTINIT = 5, K_REUSE = 6, K_ROOTKEPT = 7,
                 K_PROVEN = 8 };   // YY_FLAG_SOLVER: the descent ended on a proven node below the root
#define CHILD_NONE 0x00FFFFFFu
#define NF_TERMINAL 1u
#define NF_HASVALUE 2u   // childless node whose evaluator value (record .w) may be reused (YY_FLAG_REUSE_PASS_VALUE)
// YY_FLAG_SOLVER: the proven status of a node with children, for its side to move, in two flag bits (PV_*); its exact value
// is kept where a terminal node keeps its terminal value (record .z).  Never set without the flag.
#define NF_PROVEN_SHIFT 2
#define NF_PROVEN_MASK 0xCu
enum { PV_NONE = 0, PV_WIN = 1, PV_LOSS = 2, PV_DRAW = 3 };

// The pending leaf of one descent: what selection leaves for the expansion + backup that follows the evaluator.  K = 1 keeps
// the one record of a game in its GameState; leaf-parallel steps (leaves_per_step K > 1) keep descent j of game g in
// leaves[g*K + j].  board / mask / player / terminal / tv are set only for a leaf that is evaluated (leaf_store).
struct LeafRec {
    int32_t path_len, node;  // edges on the path == depth of the leaf; the leaf's node record when it already has one, else -1
    int32_t dup;             // K > 1: >= 0: an earlier descent of this step that ended on the same leaf (its row is shared), else -1
    float tv;                // terminal value of a freshly evaluated leaf (f32 of 1 / -1 / 1e-4)
    uint8_t kind, terminal;
    int8_t player;
    uint8_t pad[5];
    uint64_t board[2 * YY_MAX_NW];
    uint64_t mask[YY_MAX_NW];
};

// GameState.ctr: what a game counts since create / yy_mcts_reset_counters (lane 0 counts).  In the order of the readers' outputs:
// yy_mcts_status, yy_mcts_forced_descents, yy_mcts_shared_counters(_ex), yy_mcts_solver_counters
enum {
    TC_EVALS,           // evaluator rows requested
    TC_LEVELS,          // selection levels walked
    TC_SCANNED,         // children scanned during selection
    TC_CREATED,         // children (edges) created
    TC_TERMINAL,        // descents that ended on a terminal node already in the tree
    TC_NODES,           // nodes created
    TC_REUSED,          // pass values taken from the node record (YY_FLAG_REUSE_PASS_VALUE)
    TC_TABLE_HITS,      // leaves served by a position table: the game's cache, the book or the shared table
    TC_FORCED,          // forced playouts: root descents that took a forced edge
    TC_SH_HITS,         // shared evaluation table: leaves it served
    TC_SH_INSERTS,      //   rows inserted
    TC_SH_DROPPED,      //   inserts dropped (probe window full)
    TC_SH_DUPLICATES,   //   replacing mode: inserts that met their position claimed in the same launch
    TC_SV_NODES,        // solver (YY_FLAG_SOLVER): nodes proven by propagation
    TC_SV_DESCENTS,     //   descents ended on a proven node below the root
    TC_SV_ROOTS,        //   searches whose root became proven
    TC_COUNT
};

struct GameState {
    int32_t n_nodes, n_edges;
    int32_t root_N;
    float root_W;
    double root_W_py;       // root.value_sum while it is still a python float (terminal root only)
    int8_t root_player;
    uint8_t active, err, root_w_is_py;
    uint8_t err_ever;       // sticky: set with err, survives yy_mcts_begin, cleared only by yy_mcts_status
    uint8_t kept;           // yy_mcts_advance left this game's tree re-rooted at node 0; consumed by the next yy_mcts_begin
    uint8_t root_kept;      // the root of the current search is a kept node: its own first visit expanded it, so its children's
                            // visits sum to root_N - 1 (a fresh root's: root_N)
    int32_t leaf_src;       // where this leaf's evaluation comes from: SRC_NONE (an evaluator row), src_cache(slot), src_book(slot),
                            // src_shared(slot)
    int32_t leaf_ec_slot;   // leaf_src == SRC_NONE: the cache slot this leaf's evaluation goes into
    uint32_t ec_epoch;      // entries of other epochs are replaceable (see root_setup)
    int32_t root_stones;    // stones on the root board: a cached position with no more stones cannot be a leaf again
    int32_t budget;         // K = 1: simulations of this game's current search (root_setup); at root_N == budget selection stops
    LeafRec leaf;           // K = 1: the pending leaf
    uint64_t ctr[TC_COUNT]; // the TC_* counters
};
static_assert(sizeof(GameState) == 280, "GameState changed size");
static_assert(offsetof(GameState, ctr) == 152, "GameState.ctr moved");

// A game stops searching (arena overflow, non-finite evaluator output, no selectable child); called by lane 0.  err_ever
// survives yy_mcts_begin and is cleared only by yy_mcts_status.
__device__ __forceinline__ void fail_game(GameState *st) { st->err = st->err_ever = 1; }

// A table of evaluated positions: open addressing on bb_hash, keys compared in full.  The shared book is one such table,
// game g's evaluation cache another (cache_of: a slice of the context's ec arrays).
struct PosTable {
    uint32_t *meta;         // [slots]  0 = never used; cache: epoch << 8 | stones, book: 1, shared table: the inserting launch's stamp
    uint64_t *key;          // [slots, 2*NW]  the position
    float *val;             // [slots]  the evaluator's value
    float *pol;             // [slots, A]  the evaluator's policy row
    uint32_t mask;          // slots - 1 (slots is a power of two)
};

// The device's view of a context, the by-value argument of every context kernel: filled once by yy_mcts_create (the book
// part by yy_mcts_set_book) and kept in the context, so that a launch passes what the host itself allocates through.
struct MctsDev {
    YYGeo geo;
    int32_t G;
    uint32_t aliased, reuse;
    float cpuct;
    int64_t node_cap, edge_cap, path_cap;
    uint4 *edges, *nodes;
    uint64_t *nboard, *gboard;
    int32_t *path;
    // evaluation cache (YY_FLAG_REUSE_TRANSPOSITIONS / YY_FLAG_KEEP_EVALUATIONS): the arrays of all G games, mask + 1 slots
    // per game; meta == nullptr: off
    PosTable ec;
    uint32_t ec_keep;
    // shared book of pre-evaluated positions (yy_mcts_set_book; arrays owned by the caller, read-only here); meta == nullptr: none
    PosTable bk;
    int32_t bk_stones;
    // shared evaluation table (yy_mcts_set_shared_evaluations; arrays owned by the caller): what any game of the context had
    // evaluated in an EARLIER launch serves every game; insert-only.  meta == nullptr: off, every kernel does what it did
    // without it.  *sh_stamp: the step stamp, never 0, advanced by k_stamp in front of every tree-step launch
    PosTable sh;
    uint32_t *sh_stamp;
    // replacing mode (yy_mcts_set_shared_evaluations_replacing; nullptr: the insert-only table above, every kernel does what it
    // did with it).  sh_claim [slots]: SH_CLAIM(tag, stamp) -- the inserting launch's stamp in the low half (0: never used,
    // SH_TOMBSTONE: evicted, both free), the upper half of the position's bb_hash in the high half; sh.meta then names the
    // same words and only says "a table is set".  sh_hit [slots]: the stamp of the last launch that served the entry (its
    // insert stamp until then).  sh_sweep [SH_SWEEP_WORDS]: the state of the sweeps (yy_shared_table.hip)
    unsigned long long *sh_claim;
    uint32_t *sh_hit;
    unsigned long long *sh_sweep;
    GameState *state;
    float *sqrt_tab;
    int32_t sqrt_n;         // entries of sqrt_tab: max_sims + 2 (+ K when K > 1: virtual visits)
    // symmetry-randomised evaluation (YY_FLAG_EVAL_SYMMETRY): a position's row is written under sym_of(position) and its policy
    // row read through sym_cell; 0: off, every kernel does what it did without it
    uint32_t sym;
    uint64_t sym_seed;
    // forced playouts with policy target pruning (YY_FLAG_FORCED_PLAYOUTS): k of yy_mcts_config.forced_playouts; 0.0: off, every
    // kernel does what it did without it.  K = 1 and copied boards only (yy_mcts_create)
    double forced;
    // first-play urgency reduction (YY_FLAG_FPU_REDUCTION): r below the root and r at the root; fpu == 0: off, every kernel
    // does what it did without it (an unvisited child scores q = 0)
    float fpu, fpu_root;
    // MCTS solver (YY_FLAG_SOLVER): proven statuses are propagated after a descent that ended on an exact value, and a proven
    // node below the root ends a descent; 0: off, no node ever carries a proven flag and every kernel does what it did without it
    uint32_t solver;
    // Gumbel root search (YY_FLAG_GUMBEL_ROOT): m of yy_mcts_config.gumbel_root; 0: off, every kernel does what it did without
    // it.  K = 1 and copied boards only (yy_mcts_create).  g_rows: the caller's Gumbel variables f32 [G][A] by action
    // (yy_mcts_set_gumbel); g_s0: f32 [G][A], the base score g + log P of game g's root edge j at g*A + j (root expansion)
    uint32_t gumbel;
    float g_cvisit, g_cscale;
    const float *g_rows;
    float *g_s0;
    // Gumbel search below the root (YY_FLAG_GUMBEL_INTERIOR, only with YY_FLAG_GUMBEL_ROOT): the root record keeps the evaluator's
    // value, unvisited children are completed with v_mix and a descent below the root takes the child of the largest
    // pi'(a) - N(a) / (1 + S); 0: off, every kernel does what it did without it
    uint32_t g_interior;
};

// ---- shared evaluation table, replacing mode: the claim word and the sweep state (yy_engine.hip, yy_shared_table.hip)
#define SH_TOMBSTONE 0xFFFFFFFFu           // the stamp of an evicted slot; k_stamp never hands it out, as it never hands out 0
#define SH_CLAIM(tag, stamp) (((unsigned long long)(tag) << 32) | (unsigned long long)(stamp))
__host__ __device__ __forceinline__ uint32_t sh_stamp_of(unsigned long long claim) { return (uint32_t)claim; }
__host__ __device__ __forceinline__ bool sh_free(uint32_t stamp) { return stamp == 0u || stamp == SH_TOMBSTONE; }
// the successor of a stamp: 0 and SH_TOMBSTONE are skipped, so the stamps run 1 .. 2^32 - 2 and wrap to 1
__host__ __device__ __forceinline__ uint32_t sh_next_stamp(uint32_t s) {
    s += 1u;
    return sh_free(s) ? 1u : s;
}
// sh_sweep words: live entries counted by the running sweep, entries it evicted, live entries after the last sweep, entries
// evicted since the table was set or the counters reset, the stamp recorded by the last sweep above the mark (0: none yet)
enum { SH_SW_COUNT = 0, SH_SW_EVICTING = 1, SH_SW_LIVE = 2, SH_SW_EVICTED = 3, SH_SW_CUTOFF = 4, SH_SWEEP_WORDS = 8 };

struct MultiDev {  // by-value kernel argument of the K > 1 kernels, next to MctsDev
    int32_t K;               // leaves per step (1: one descent per game per step)
    LeafRec *leaves;         // [G*K]
    int32_t *mst;            // [G][2] = {simulations of the current search, descents of the pending step}
};

struct yy_mcts {
    yy_mcts_config cfg;
    MctsDev dev;            // every pointer, capacity and the geometry live here only
    MultiDev multi;
    int32_t target_sims;    // simulations of the next searches (K > 1: sets the descents of the last step on the device)
    const int32_t *budgets; // device int32 [G] of per-game simulation budgets for the next yy_mcts_begin; nullptr: target_sims for all
    uint64_t *scratch;      // [TC_COUNT + 1]: the counters summed over the games, then the failed games (tree_counters)
    int32_t *remap;         // [G][node_cap] old node index -> new one (k_advance); allocated by the first yy_mcts_advance
    uint64_t bytes;
    int pending;            // 1 = a select is pending an expand_backup
};

template <int NW> __device__ __forceinline__ int pos_stones(BB<NW> black, BB<NW> white) { return bb_popc(black) + bb_popc(white); }

__device__ __forceinline__ uint32_t node_pack(int k, uint32_t flags, int player) {
    return (uint32_t)k | (flags << 16) | ((uint32_t)(player & 0xFF) << 24);
}
__device__ __forceinline__ int node_k(uint32_t y) { return (int)(y & 0xFFFFu); }
__device__ __forceinline__ uint32_t node_flags(uint32_t y) { return (y >> 16) & 0xFFu; }
__device__ __forceinline__ int node_player(uint32_t y) { return (int)(int8_t)(y >> 24); }

// ---- solver (YY_FLAG_SOLVER): the three exact values are the terminal ones, f32 of 1 / -1 / 1e-4 for the side to move
__device__ __forceinline__ int proven_class(float v) { return (v == 1.0f) ? PV_WIN : (v == -1.0f) ? PV_LOSS : PV_DRAW; }
__device__ __forceinline__ float proven_value(int s) { return (s == PV_WIN) ? 1.0f : (s == PV_LOSS) ? -1.0f : 0.0001f; }
// the proven status of a node record: a terminal node's is the class of its terminal value, every other node's its flag pair
__device__ __forceinline__ int node_proven(uint4 hdr) {
    const uint32_t f = node_flags(hdr.y);
    return (f & NF_TERMINAL) ? proven_class(__uint_as_float(hdr.z)) : (int)((f & NF_PROVEN_MASK) >> NF_PROVEN_SHIFT);
}

// getGameEnded(board, player) as float32 + the mask of `player` (yin_yang_game.py:80-110)
template <int NW>
__device__ __forceinline__ void leaf_rules(const YYGeo &geo, const GeoBB<NW> &gb, BB<NW> black, BB<NW> white,
                                           int player, BB<NW> &mask, bool &terminal, float &tv) {
    bool pre = bb_pre2x2(black, white, gb);
    BB<NW> mb = bb_legal(black, white, pre, geo, gb), mw = bb_legal(white, black, pre, geo, gb);
    int res = bb_result_black(black, white, mb, mw);
    mask = (player == 1) ? mb : mw;
    terminal = (res != 0);
    tv = (res == 2) ? 0.0001f : ((player == 1) ? (float)res : (float)-res);
}

// the position half of a leaf record: what the expansion needs of a leaf that is evaluated
template <int NW>
__device__ __forceinline__ void leaf_store(LeafRec *rec, BB<NW> black, BB<NW> white, BB<NW> mask, int player, bool term,
                                           float tv) {
    if (lane_id() == 0) {
#pragma unroll
        for (int i = 0; i < NW; i++) {
            rec->board[i] = black.w[i];
            rec->board[NW + i] = white.w[i];
            rec->mask[i] = mask.w[i];
        }
        rec->player = (int8_t)player;
        rec->terminal = term;
        rec->tv = tv;
    }
}

// ---- root prologue: mcts.py:288-295.  The root of game g's next search on the position (black, white) with `player` to move:
// a fresh root (keep == false: the arena is reset, `budget` stored, a K_ROOTINIT expansion left pending in `rec` for an active
// game) or, with keep, the tree yy_mcts_advance left (k_begin has written its state); for both the evaluation-cache epoch, the
// root board and -- for an active game -- the planes of the root call, written to `planes_row`.
template <int NW>
__device__ __forceinline__ void root_setup(const MctsDev &d, GameState *st, LeafRec *rec, const int g, BB<NW> black, BB<NW> white,
                                           const int player, const bool act, const bool keep, const int budget,
                                           float *planes_row) {
    if (!keep && lane_id() == 0) {
        st->kept = 0;
        st->root_kept = 0;
        st->n_nodes = 1;  // node 0 = root
        st->n_edges = 0;
        st->root_N = 0;
        st->root_W = 0.0f;
        st->root_W_py = 0.0;
        st->root_w_is_py = 1;
        st->root_player = (int8_t)player;
        st->active = act;
        st->err = 0;
        st->budget = budget;
        rec->kind = act ? K_ROOTINIT : K_NONE;
        rec->node = 0;
        rec->path_len = 0;
        rec->dup = -1;
        d.nodes[(size_t)g * d.node_cap] = make_uint4(0u, node_pack(0, 0, player), 0u, 0u);
    }
    if (d.ec.meta && lane_id() == 0) {
        // Entries of an older epoch are the first to be replaced.  Without YY_FLAG_KEEP_EVALUATIONS every search is its own
        // epoch and only entries of the current one are looked at (reuse inside one search); with it the epoch changes when
        // a game starts over from the empty board, so a game's searches share their evaluations.
        const int stones = pos_stones<NW>(black, white);
        uint32_t ep = st->ec_epoch;
        if (!d.ec_keep || stones == 0 || ep == 0u) ep = (ep + 1u) & 0xFFFFFFu;
        if (ep == 0u) ep = 1u;
        st->ec_epoch = ep;
        st->root_stones = stones;
    }
    uint64_t *gbd = d.gboard + (size_t)g * 2 * NW;
    bb_store_lane0<NW>(gbd, black);
    bb_store_lane0<NW>(gbd + NW, white);
    if (!d.aliased && !keep) {
        uint64_t *nb = d.nboard + (size_t)g * d.node_cap * 2 * NW;
        bb_store_lane0<NW>(nb, black);
        bb_store_lane0<NW>(nb + NW, white);
    }
    if (act) {
        // root.expand's rules (mcts.py:63-71) for the pending K_ROOTINIT expansion
        const GeoBB<NW> gb = geo_bb<NW>(d.geo);
        BB<NW> mask;
        bool term;
        float tv;
        if (!keep) {
            leaf_rules<NW>(d.geo, gb, black, white, player, mask, term, tv);
            leaf_store<NW>(rec, black, white, mask, player, term, tv);
        }
        write_eval_planes<NW>(planes_row, d.geo, d.sym, d.sym_seed, black, white);
    }
}

// ------------------------------------------------------------------------------------ the edge score, one copy
// float -> unsigned key with the same order (all non-NaN keys are > 0)
__device__ __forceinline__ uint32_t f32_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Order-preserving key of one child's PUCT score (mcts.py:120-133), float32 order of SURVEY 8a/a12: the exploration term with
// `nu` visits, the mean value over `nq`.  Selection scores an edge with nu == nq (child_key); policy target pruning asks what
// the edge would have scored with fewer visits and its real mean value.  q0: the value an unvisited child (nq == 0) is scored
// with -- 0 in the reference, the node's first-play urgency with YY_FLAG_FPU_REDUCTION (fpu_value, yy_engine.hip).
__device__ __forceinline__ uint32_t child_key_at(float cpuct, float sq, float P, int nu, int nq, float w, float q0 = 0.0f) {
    const float t1 = __fmul_rn(cpuct, P);
    const float t2 = __fmul_rn(t1, sq);
    const float u = __fdiv_rn(t2, (float)(1 + nu));
    const float q = (nq > 0) ? __fdiv_rn(w, (float)nq) : q0;
    const float ucb = __fadd_rn(__fadd_rn(q, u), 0.0f);   // + 0.0f: -0.0 compares equal to +0.0 (mcts.py:133)
    return f32_key(ucb);
}
__device__ __forceinline__ uint32_t child_key(float cpuct, float sq, float P, int n, float w, float q0 = 0.0f) {
    return child_key_at(cpuct, sq, P, n, n, w, q0);
}

// ------------------------------------------------------------------------------------ forced playouts (YY_FLAG_FORCED_PLAYOUTS)
// k * P(c) * S in float64, in this order: the square of the visits a root edge of stored prior P is owed once the root's
// children hold S visits.  An edge is forced while it has been visited and N * N is below the bound.
__device__ __forceinline__ double forced_bound(const double k, const float P, const int S) {
    return __dmul_rn(__dmul_rn(k, (double)P), (double)S);
}
__device__ __forceinline__ bool edge_forced(const double k, const float P, const int n, const int S) {
    return n >= 1 && __dmul_rn((double)n, (double)n) < forced_bound(k, P, S);
}

// Policy target pruning: the counts cn[i] of this lane's root edges (edge i*64 + lane; 0 past the k-th) become the pruned
// counts N'.  c* = the most visited edge, the lowest index on ties, keeps its count; every other visited edge gives back, one
// at a time and at most n_f = min{m >= 0: m*m >= k*P*S} of them, the visits without which it would still score below c* (its
// mean value held), and an edge left with one visit is left with none.
template <int NW>
__device__ __forceinline__ void prune_forced(const MctsDev &d, const uint4 *edges, const int first, const int k, const int S,
                                             int (&cn)[NW]) {
    int mx = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) mx = max(mx, cn[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
    if (mx == 0) return;                                                        // wave-uniform: no edge was visited
    int star = -1;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const uint64_t m = __ballot(i * 64 + lane_id() < k && cn[i] == mx);
        if (star < 0 && m) star = i * 64 + (int)__ffsll((unsigned long long)m) - 1;
    }
    const float sq = d.sqrt_tab[min(S, d.sqrt_n - 1)];
    const uint4 es = edges[first + star];
    const uint32_t kstar = child_key(d.cpuct, sq, __uint_as_float(rfl(es.x)), (int)rfl(es.y), __uint_as_float(rfl(es.z)));
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const int j = i * 64 + lane_id();
        if (j >= k || j == star || cn[i] == 0) continue;
        const uint4 e = edges[first + j];
        const float P = __uint_as_float(e.x), w = __uint_as_float(e.z);
        const int n = cn[i];
        const double bound = forced_bound(d.forced, P, S);
        int np = n;
        // first-play urgency does not enter here: only visited edges are scored (nq == n >= 1), as edge_forced only looks at
        // visited edges, so forcing and pruning are the same with and without YY_FLAG_FPU_REDUCTION
        for (int m = 0; np >= 1 && __dmul_rn((double)m, (double)m) < bound; m++) {   // m < n_f
            if (child_key_at(d.cpuct, sq, P, np - 1, n, w) < kstar) np -= 1;
            else break;
        }
        cn[i] = (np == 1) ? 0 : np;
    }
}

// ------------------------------------------------------------------------------------ Gumbel root search (YY_FLAG_GUMBEL_ROOT)
// seq(m', n)[S] (include/yy_engine.h): the visit count the root child that descent S of a search of n simulations goes to must
// have.  Inside a phase the c considered children all hold v visits at its start, so the table is never built: round r of a
// phase is c entries of v + r.  Wave-uniform scalar work: at most ceil(log2 m') halvings, then phases of n / (2L) rounds.
__device__ __forceinline__ int gumbel_seq_at(const int mp, const int n, const int S) {
    if (mp <= 1) return S;
    const int L = 32 - __clz(mp - 1);   // ceil(log2 m'), m' >= 2
    int c = mp, v = 0, pos = 0;
    for (;;) {
        const int extra = max(1, n / (L * c));
        if (S < pos + extra * c) return v + (S - pos) / c;
        pos += extra * c;
        v += extra;
        c = max(2, c / 2);
    }
}
// Order-preserving key of f32(s0 + sigma) of a root child with N visits and value sum W, maxN the largest child visit count:
// sigma = f32(f32(f32(c_visit + maxN) * c_scale) * q), q = f32(W / N) or 0.  + 0.0f as in child_key_at; a NaN score gets key 0
__device__ __forceinline__ uint32_t gumbel_key(const MctsDev &d, const float s0, const int maxN, const int N, const float W) {
    const float q = (N > 0) ? __fdiv_rn(W, (float)N) : 0.0f;
    const float sg = __fmul_rn(__fmul_rn(__fadd_rn(d.g_cvisit, (float)maxN), d.g_cscale), q);
    const float sc = __fadd_rn(__fadd_rn(s0, sg), 0.0f);
    return (sc != sc) ? 0u : f32_key(sc);
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t t = (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
// The Gumbel winner of game g's root: among the children with the largest visit count the largest f32(s0 + sigma), the lowest
// edge on ties; its action, or -1 for an inactive game and for a root without children.  Every lane of the wavefront calls it.
template <int NW> __device__ __forceinline__ int gumbel_winner(const MctsDev &d, const int g) {
    const uint4 hdr = d.nodes[(size_t)g * d.node_cap];
    const int k = node_k(rfl(hdr.y)), first = rfl((int)hdr.x);
    if (rfl((int)d.state[g].active) == 0 || k == 0) return -1;
    const uint4 *edges = d.edges + (size_t)g * d.edge_cap;
    const float *s0 = d.g_s0 + (size_t)g * d.geo.A;
    uint4 e[NW];
    int mx = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const int j = i * 64 + lane_id();
        e[i] = (j < k) ? edges[first + j] : make_uint4(0u, 0u, 0u, 0u);
        mx = max(mx, (int)e[i].y);
    }
    mx = wave_max_i32(mx);
    uint64_t best = 0;                                                          // key << 32 | ~edge: the largest key, then the lowest edge
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const int j = i * 64 + lane_id();
        if (j < k && (int)e[i].y == mx) {
            const uint64_t c = ((uint64_t)gumbel_key(d, s0[j], mx, mx, __uint_as_float(e[i].z)) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)j);
            best = c > best ? c : best;
        }
    }
    best = wave_max_u64(best);
    const int j = (int)(0xFFFFFFFFu - (uint32_t)best);
    return (int)(rfl(edges[first + j].w) >> 24);
}

// ---- Gumbel search below the root (YY_FLAG_GUMBEL_INTERIOR): v_mix, completed Q and the improved policy pi', in arithmetic that a
// numpy restatement reproduces bit for bit (include/yy_engine.h): no log, the project's own exponential, integer sums.
// E(x) = exp(x) for x <= 0: correctly rounded float64 products and sums only (no contraction), an exact scaling by 2^n.
__device__ __forceinline__ double gumbel_exp(const double x) {
    if (x < -708.0) return 0.0;
    const double n = __builtin_rint(__dmul_rn(x, 0x1.71547652b82fep+0));        // log2(e)
    const double r = __dadd_rn(__dadd_rn(x, -__dmul_rn(n, 0x1.62e42feep-1)), -__dmul_rn(n, 0x1.a39ef35793c76p-33));   // ln2 hi, lo
    double p = 1.0 / 6227020800.0;                                              // Taylor, degree 13, Horner
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 479001600.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 39916800.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 3628800.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 362880.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 40320.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 5040.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 720.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 120.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 24.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0 / 6.0);
    p = __dadd_rn(__dmul_rn(p, r), 0.5);
    p = __dadd_rn(__dmul_rn(p, r), 1.0);
    p = __dadd_rn(__dmul_rn(p, r), 1.0);
    // n in -1022 .. 0: 2^n is a normal number and the product is exact
    return __dmul_rn(p, __longlong_as_double((long long)((int)n + 1023) << 52));
}
// float64 -> unsigned key with the same order; a NaN gets key 0, every other value a key > 0
__device__ __forceinline__ uint64_t f64_key(const double f) {
    const uint64_t u = (uint64_t)__double_as_longlong(f);
    return (f != f) ? 0ull : (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
#define GI_NAN 0xFFFFFFFFFFFFFFFFull   // the term of an edge whose completed q is a NaN
// What the improved policy of a node needs, from its k > 0 edges e[] (edge i*64 + lane in e[i], zero past the k-th) and its own
// evaluator value vhat: S = the children's visits, v_mix, sigma's scale and maximum, the terms t[] (gumbel_term) and their sum
// Z: pi'(a) = f64(t(a)) / f64(Z).  The sums are integers (P and P * q in units of 2^-40, the terms in units of 2^-52), so that
// they do not depend on which lane holds which child.  Only the edges and the terms are kept per edge; priors and sigmas are
// recomputed where they are read.  One copy: the descent below the root (do_select) and the root's policy target read it.
struct GumbelNode { int S; bool anyp; double vmix, scale, xm; uint64_t Z; };
// the prior of an edge in units of 2^-40 (truncated), and sigma of its completed q
// (a negative prior counts as 0, as a NaN would: expansion refuses NaN priors)
__device__ __forceinline__ uint64_t gumbel_prior(const uint4 e) {
    return (uint64_t)fmax(__dmul_rn((double)__uint_as_float(e.x), 1099511627776.0), 0.0);
}
__device__ __forceinline__ double gumbel_sigma(const GumbelNode &n, const uint4 e) {
    return __dmul_rn(n.scale, ((int)e.y > 0) ? __ddiv_rn((double)__uint_as_float(e.z), (double)(int)e.y) : n.vmix);
}
// t(a) in units of 2^-52: GI_NAN for an edge whose sigma is a NaN against the maximum, 1 for every edge when every prior is 0
__device__ __forceinline__ uint64_t gumbel_term(const GumbelNode &n, const uint4 e) {
    if (!n.anyp) return 1ull;
    const uint64_t p = gumbel_prior(e);
    if (!p) return 0ull;
    const double a = __dadd_rn(gumbel_sigma(n, e), -n.xm);                      // <= 0 wherever a term is taken
    return (a != a) ? GI_NAN : (uint64_t)__dmul_rn(__dmul_rn((double)p, gumbel_exp(a)), 4096.0);
}
template <int NW>
__device__ __forceinline__ GumbelNode gumbel_improved(const MctsDev &d, const uint4 (&e)[NW], const int k, const float vhat,
                                                      uint64_t (&t)[NW]) {
    int mx = 0, S = 0;
    uint64_t spv = 0;
    long long spq = 0;
    bool anyp = false;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const int n = (int)e[i].y;
        const uint64_t p = gumbel_prior(e[i]);
        anyp |= p != 0ull;
        mx = max(mx, n);
        if (n > 0) {
            S += n;
            spv += p;
            const double pq = __dmul_rn((double)p, __ddiv_rn((double)__uint_as_float(e[i].z), (double)n));
            spq += (fabs(pq) < 0x1p62) ? (long long)pq : 0ll;                   // a NaN or infinite value sum adds nothing here
        }
    }
    mx = wave_max_i32(mx);
    S = wave_sum(S);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        spv += __shfl_xor((unsigned long long)spv, o, 64);
        spq += __shfl_xor(spq, o, 64);
    }
    GumbelNode r;
    r.S = S;
    r.anyp = __ballot(anyp) != 0;                                               // false: every prior 0, the uniform row
    r.vmix = (double)vhat;
    if (S > 0) {
        const double wq = spv ? __ddiv_rn((double)spq, (double)spv) : 0.0;       // the prior-weighted mean of the visited children
        r.vmix = __ddiv_rn(__dadd_rn((double)vhat, __dmul_rn((double)S, wq)), (double)(1 + S));
    }
    r.scale = __dmul_rn(__dadd_rn((double)d.g_cvisit, (double)mx), (double)d.g_cscale);
    double xm = -INFINITY;
#pragma unroll
    for (int i = 0; i < NW; i++)
        if (gumbel_prior(e[i])) xm = fmax(xm, gumbel_sigma(r, e[i]));           // sigma_max: over the edges that can carry mass
    r.xm = sp::wave_max_f64(xm);
    uint64_t z = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        t[i] = (i * 64 + lane_id() < k) ? gumbel_term(r, e[i]) : 0ull;
        if (t[i] != GI_NAN) z += t[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) z += __shfl_xor((unsigned long long)z, o, 64);
    r.Z = z;
    return r;
}

// The policy target of the Gumbel root search into pi[0 .. A): pi' = softmax(log P + sigma64(cq)) over the k > 0 root edges
// of an active game, in float64 (include/yy_engine.h); an unvisited child is completed with the visited children's SW / SN,
// SW summed in units of 2^-32 like first-play urgency's, so that it does not depend on which lane holds which child.  With
// YY_FLAG_GUMBEL_INTERIOR (vhat: the root record's evaluator value) the target is gumbel_improved's pi', completed with v_mix.
template <int NW>
__device__ __forceinline__ void gumbel_distribution(const MctsDev &d, const uint4 *edges, const int first, const int k,
                                                    const float vhat, double *pi) {
    const int A = d.geo.A;
    uint4 e[NW];
    int mx = 0, sn = 0;
    long long sw = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const int j = i * 64 + lane_id();
        e[i] = (j < k) ? edges[first + j] : make_uint4(0u, 0u, 0u, 0u);
    }
    if (d.g_interior) {                                                         // wave-uniform: completed with v_mix, pi' = t / Z
        uint64_t t[NW];
        const GumbelNode gn = gumbel_improved<NW>(d, e, k, vhat, t);
        for (int a = lane_id(); a < A; a += 64) pi[a] = 0.0;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NW; i++)
            if (i * 64 + lane_id() < k)
                pi[(int)(e[i].w >> 24)] = (t[i] == GI_NAN) ? __longlong_as_double(0x7FF8000000000000ll) : __ddiv_rn((double)t[i], (double)gn.Z);
        return;
    }
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const int n = (int)e[i].y;
        mx = max(mx, n);
        if (n > 0) {
            sn += n;
            sw += (long long)__dmul_rn((double)__uint_as_float(e[i].z), 4294967296.0);
        }
    }
    mx = wave_max_i32(mx);
    sn = wave_sum(sn);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sw += __shfl_xor(sw, o, 64);
    const double cq0 = sn ? __ddiv_rn(__dmul_rn((double)sw, 0x1p-32), (double)sn) : 0.0;
    const double scale = __dmul_rn(__dadd_rn((double)d.g_cvisit, (double)mx), (double)d.g_cscale);
    double l[NW], lm = -INFINITY;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const int n = (int)e[i].y;
        const double cq = (n > 0) ? __ddiv_rn((double)__uint_as_float(e[i].z), (double)n) : cq0;
        l[i] = (i * 64 + lane_id() < k) ? __dadd_rn(log((double)__uint_as_float(e[i].x)), __dmul_rn(scale, cq)) : -INFINITY;
        lm = fmax(lm, l[i]);
    }
    lm = sp::wave_max_f64(lm);
    double x[NW], part = 0.0;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        // every prior 0: the uniform row over the root's edges
        x[i] = (i * 64 + lane_id() < k) ? ((lm > -INFINITY) ? exp(l[i] - lm) : 1.0) : 0.0;
        part += x[i];
    }
    const double tot = sp::wave_sum_f64(part);
    for (int a = lane_id(); a < A; a += 64) pi[a] = 0.0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NW; i++)
        if (i * 64 + lane_id() < k) pi[(int)(e[i].w >> 24)] = x[i] / tot;
}

// Node.get_children_distribution (mcts.py:183-215) of game g's root for T == 1 and T == 0 into pi[0 .. A) (float64; global
// memory or LDS), with forced playouts on the pruned counts; with the Gumbel root search its policy target for both.  Every
// thread of the one-wavefront block calls it.
template <int NW> __device__ __forceinline__ void root_distribution(const MctsDev &d, const int g, const int tzero, double *pi) {
    const int A = d.geo.A;
    const uint4 hdr = d.nodes[(size_t)g * d.node_cap];
    const int k = node_k(rfl(hdr.y)), first = rfl((int)hdr.x);
    const uint4 *edges = d.edges + (size_t)g * d.edge_cap;
    const bool act = rfl((int)d.state[g].active) != 0;
    if (d.gumbel && act && k > 0) {                                             // wave-uniform
        gumbel_distribution<NW>(d, edges, first, k, rflf(__uint_as_float(hdr.w)), pi);
        return;
    }
    int cn[NW];                                                                 // k <= A <= 64 * NW: edge i*64 + lane
    int sum = 0, mx = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const int j = i * 64 + lane_id();
        cn[i] = (act && j < k) ? (int)edges[first + j].y : 0;
        sum += cn[i];
    }
    sum = wave_sum(sum);
    if (d.forced > 0.0 && act) {                                                // wave-uniform; S = the children's visits
        prune_forced<NW>(d, edges, first, k, sum, cn);
        sum = 0;
#pragma unroll
        for (int i = 0; i < NW; i++) sum += cn[i];
        sum = wave_sum(sum);
    }
#pragma unroll
    for (int i = 0; i < NW; i++) mx = max(mx, cn[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
    double fill;
    int nbest = 0;
    if (tzero) {
        // counts == max over ALL A actions (zeros included when max == 0), mcts.py:200-203
        if (mx == 0) nbest = A;
        else {
#pragma unroll
            for (int i = 0; i < NW; i++) nbest += (i * 64 + lane_id() < k && cn[i] == mx);
            nbest = wave_sum(nbest);
        }
        fill = (mx == 0) ? 1.0 / (double)A : 0.0;
    } else {
        fill = (sum > 0) ? 0.0 : 1.0 / (double)A;                                  // mcts.py:209-213
    }
    for (int a = lane_id(); a < A; a += 64) pi[a] = act ? fill : 0.0;
    __syncthreads();
    if (!act) return;
    if (tzero ? (mx > 0) : (sum > 0)) {
#pragma unroll
        for (int i = 0; i < NW; i++) {
            const int j = i * 64 + lane_id();
            if (j < k) {
                const int a = (int)(edges[first + j].w >> 24), n = cn[i];
                pi[a] = tzero ? ((n == mx) ? 1.0 / (double)nbest : 0.0) : (double)n / (double)sum;
            }
        }
    }
}
