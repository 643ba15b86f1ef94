// yy_selfplay_move.hip -- free-running self-play: the move of the episode loop as a device kernel inside the search step.
//
// Lockstep self-play (self_play.py, SelfPlayEngine._enqueue_move) plays the moves of all G slots together: every game waits
// until the slowest search of the batch is done.  Here a step is
//     evaluator(planes, needs_eval)  ->  k_mcts(expand + backup, select; noise, eps)  ->  k_selfplay_move
// and k_selfplay_move, ONE GAME PER WAVEFRONT, lets a game whose search is complete (no pending leaf, root visits == budget)
// play its move at once: pi from the root, the example record, the move draw, the board step, the end test, the pass handling
// at the new position and the root of the next search (a pending K_ROOTINIT expansion, planes in row g, needs_eval[g] = 1)
// -- or, when the game is over, its labelled examples appended to the run's example buffer and the next game of the run
// started in the slot.  The next step's evaluator launch carries the root's row among the leaf rows and its k_mcts expands
// the root and selects the first leaf, so a move costs budget + 1 steps of that game alone.  Every other wavefront reads five
// fields and returns.
//
// Nothing here restates a rule, a draw or a formula: the root prologue, the root distribution, getNextState and getGameEnded
// come from yy_tree.h, the draws from yy_draws.h -- the very functions k_begin, k_root_policy, k_step, k_game_ended,
// k_root_noise, k_sample_actions and k_draw_budgets apply -- so a game's transcript is the lockstep engine's, bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/yy_engine.h"
#include "yy_bitboard.h"
#include "yy_common.h"
#include "yy_draws.h"
#include "yy_tree.h"

enum { C_STARTED = 0, C_FINISHED, C_FAILED, C_POSITIONS, C_RECORDED, C_ROWS, C_OVERFLOW, C_TARGET, C_COUNT };

// the device's view of a run: by-value kernel argument (captured steps keep it, so nothing in it changes after create; what
// yy_selfplay_run_arm sets lives behind the pointers)
struct SpDev {
    uint64_t seed;
    double alpha, eps, p_full;
    int32_t thr, full_sims, fast_sims;   // fast_sims == 0: no playout cap
    int32_t T;                           // examples a game can hold
    int64_t cap;                         // rows of the example buffer
    // per slot
    uint64_t *board;                     // [G][2*NW] black words, white words
    int8_t *player;
    int32_t *ply, *n_ex;
    uint8_t *alive, *is_full;
    int64_t *game_id;
    int8_t *h_state;                     // [G][T][A]
    float *h_pi;                         // [G][T][A]
    int8_t *h_player;                    // [G][T]
    int32_t *h_ply;                      // [G][T]
    double *noise;                       // [G][A] the row k_mcts mixes into a root expansion (all zero: none)
    float *gumbel;                       // [G][A] Gumbel root search: the row a root expansion takes its base scores from; else nullptr
    unsigned long long *ctr;             // [C_COUNT]
    int64_t *prm;                        // [2] first game index, stride
    // finished examples
    int8_t *ex_state;                    // [cap][A]
    float *ex_pi;                        // [cap][A]
    float *ex_z;
    int64_t *ex_gid, *ex_ply;
};

struct yy_selfplay_run {
    yy_mcts *ctx;
    yy_selfplay_config cfg;
    SpDev dev;
    void *mem[24];
    int n_mem;
};

// What follows a move, and what starts a game: the game at (black, white), `player` to move, either goes on -- after up to
// two passes (self_play.py:103-125: flip on no move, end on the second) its next root is set up -- or leaves its slot: over
// (examples labelled and appended) or failed (examples dropped), and the run's next game starts here from the empty board,
// or the slot goes idle.
template <int NW>
__device__ __forceinline__ void settle(const MctsDev &d, const SpDev &r, const int g, BB<NW> black, BB<NW> white, int player,
                                       int ply, int64_t gid, int n, bool over, bool failed, double res, float *planes,
                                       uint8_t *needs_eval) {
    const int lane = lane_id(), A = d.geo.A, T = r.T;
    const GeoBB<NW> gb = geo_bb<NW>(d.geo);
    GameState *st = d.state + g;
    BB<NW> mask = bb_zero<NW>();
    for (;;) {
        if (!over && !failed) {
            int passes = 0;
            for (int it = 0; it < 2; it++) {
                const bool pre = bb_pre2x2(black, white, gb);
                mask = (player == 1) ? bb_legal(black, white, pre, d.geo, gb) : bb_legal(white, black, pre, d.geo, gb);
                if (bb_any(mask)) break;
                if (++passes >= 2) {
                    over = true;
                    res = bb_game_ended<NW>(d.geo, gb, black, white, player);
                    if (res == 0.0) res = 0.0001;                               // self_play.py:110-112
                    break;
                }
                player = -player;
            }
            if (!over) break;
        }
        // ---- the game leaves its slot
        if (!failed) {
            // z by player against the final player (self_play.py:114-121, 170-188), rows reserved with one atomic add
            n = min(n, T);
            __syncthreads();                                                    // the record lane 0 wrote in this launch
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(&r.ctr[C_ROWS], (unsigned long long)n);
            base = rfl64(base);
            if (base + (unsigned long long)n > (unsigned long long)r.cap) {
                if (lane == 0) atomicAdd(&r.ctr[C_OVERFLOW], 1ull);             // nothing is written past the buffer
            } else {
                for (int i = 0; i < n; i++) {
                    const size_t src = ((size_t)g * T + i) * A, dst = ((size_t)base + i) * A;
#pragma unroll
                    for (int j = 0; j < NW; j++) {
                        const int cell = j * 64 + lane;
                        if (cell < A) {
                            r.ex_state[dst + cell] = r.h_state[src + cell];
                            r.ex_pi[dst + cell] = r.h_pi[src + cell];
                        }
                    }
                }
                for (int i = lane; i < n; i += 64) {
                    const bool same = (int)r.h_player[(size_t)g * T + i] == player;
                    r.ex_z[base + i] = (float)(same ? res : -res);
                    r.ex_gid[base + i] = gid;
                    r.ex_ply[base + i] = (int64_t)r.h_ply[(size_t)g * T + i];
                }
            }
        }
        unsigned long long k = 0;
        if (lane == 0) {
            atomicAdd(&r.ctr[failed ? C_FAILED : C_FINISHED], 1ull);
            k = atomicAdd(&r.ctr[C_STARTED], 1ull);
        }
        k = rfl64(k);
        if (k >= r.ctr[C_TARGET]) {                                             // no game left to start: the slot goes idle
            if (lane == 0) {
                r.alive[g] = 0;
                r.game_id[g] = -1;
                r.n_ex[g] = 0;
                st->active = 0;
                st->leaf.kind = K_NONE;
                needs_eval[g] = 0;
            }
            return;
        }
        black = bb_zero<NW>();
        white = bb_zero<NW>();
        player = 1;                                                             // black starts (self_play.py:81)
        ply = 0;
        n = 0;
        gid = r.prm[0] + (int64_t)k * r.prm[1];
        over = failed = false;
    }
    // ---- the game goes on: the root of its next search (mcts.py:288-295)
    bool full = true;
    if (r.fast_sims > 0) full = sp::draw_full_search(r.seed, gid, ply, r.p_full);
    root_setup<NW>(d, st, &st->leaf, g, black, white, player, true, false, full ? r.full_sims : r.fast_sims,
                   planes + (size_t)g * 5 * A);
    uint64_t *sb = r.board + (size_t)g * 2 * NW;
    bb_store_lane0<NW>(sb, black);
    bb_store_lane0<NW>(sb + NW, white);
    if (lane == 0) {
        needs_eval[g] = 1;
        r.player[g] = (int8_t)player;
        r.ply[g] = ply;
        r.n_ex[g] = n;
        r.game_id[g] = gid;
        r.is_full[g] = full;
        r.alive[g] = 1;
    }
    if (r.eps > 0.0) {                                                          // add_noise = (step == 0), self_play.py:131
        bool legal[3];
#pragma unroll
        for (int j = 0; j < 3; j++) legal[j] = j < NW && j * 64 + lane < A && ((mask.w[j < NW ? j : 0] >> lane) & 1);
        sp::dirichlet_row(r.seed, gid, ply, ply == 0, legal, A, r.alpha, r.noise + (size_t)g * A);
    }
    if (r.gumbel) {                                                             // Gumbel root search: k_root_gumbel's row, at every ply
        for (int a = lane; a < A; a += 64) r.gumbel[(size_t)g * A + a] = sp::gumbel_draw(r.seed, gid, ply, a);
    }
}

template <int NW>
__global__ void __launch_bounds__(64) k_selfplay_move(MctsDev d, SpDev r, float *planes, uint8_t *needs_eval) {
    __shared__ double pi[64 * YY_MAX_NW];
    const int g = blockIdx.x, lane = lane_id(), A = d.geo.A;
    GameState *st = d.state + g;
    // the common case is "nothing to do": the five fields are loaded before any is tested -- one round trip to memory
    const int s_alive = r.alive[g], s_kind = st->leaf.kind, s_err = st->err, s_N = st->root_N, s_budget = st->budget;
    const bool failed = rfl(s_err) != 0;                                        // a failed search never reaches its budget
    if ((rfl(s_alive) == 0) | (rfl(s_kind) != K_NONE) | (!failed & (rfl(s_N) < rfl(s_budget)))) return;
    const GeoBB<NW> gb = geo_bb<NW>(d.geo);
    const uint64_t *sb = r.board + (size_t)g * 2 * NW;
    BB<NW> black = bb_uniform_load<NW>(sb), white = bb_uniform_load<NW>(sb + NW);
    int player = rfl((int)r.player[g]), ply = rfl(r.ply[g]), n = rfl(r.n_ex[g]);
    const int64_t gid = (int64_t)rfl64((uint64_t)r.game_id[g]);
    bool over = false;
    double res = 0.0;
    if (!failed) {
        root_distribution<NW>(d, g, 0, pi);                                     // T == 1 distribution, self_play.py:329
        __syncthreads();
        // ---- the example before the move (self_play.py:140); under playout cap only the fully searched moves
        const bool rec = r.fast_sims == 0 || rfl((int)r.is_full[g]) != 0;
        if (rec) {
            const size_t at = (size_t)g * r.T + min(n, r.T - 1);
            bb_to_board<NW>(r.h_state + at * A, A, black, white);
#pragma unroll
            for (int j = 0; j < NW; j++) {
                const int cell = j * 64 + lane;
                if (cell < A) r.h_pi[at * A + cell] = (float)pi[cell];
            }
            if (lane == 0) {
                r.h_player[at] = (int8_t)player;
                r.h_ply[at] = ply;
            }
            n += 1;
        }
        // ---- the move (self_play.py:143-163) and the end test (:167)
        const bool pre = bb_pre2x2(black, white, gb);
        const BB<NW> mask = (player == 1) ? bb_legal(black, white, pre, d.geo, gb) : bb_legal(white, black, pre, d.geo, gb);
        int action = -1;
        if (d.gumbel) {                                                         // wave-uniform: the Gumbel winner, at every ply
            action = gumbel_winner<NW>(d, g);
        } else {
            if (lane == 0)
                action = sp::pick_action(r.seed, gid, ply, r.thr, pi, [&mask](int a) { return bb_test(mask, a); }, A);
            action = rfl(action);
        }
        bb_play<NW>(d.geo, gb, black, white, player, action);
        player = -player;                                                       // yin_yang_game.py:58, regardless
        ply += 1;
        const double ended = bb_game_ended<NW>(d.geo, gb, black, white, player);
        if (ended != 0.0) {
            over = true;
            res = ended;
        }
        if (lane == 0) {
            atomicAdd(&r.ctr[C_POSITIONS], 1ull);
            if (rec) atomicAdd(&r.ctr[C_RECORDED], 1ull);
        }
    }
    settle<NW>(d, r, g, black, white, player, ply, gid, n, over, failed, res, planes, needs_eval);
}

__global__ void k_selfplay_reset(SpDev r, int G, long long num_games, long long first, long long stride) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int i = 0; i < C_COUNT; i++) r.ctr[i] = 0ull;
    r.ctr[C_STARTED] = (unsigned long long)(num_games < G ? num_games : G);
    r.ctr[C_TARGET] = (unsigned long long)num_games;
    r.prm[0] = first;
    r.prm[1] = stride;
}

// slot g starts game g of the run (empty board, black to move), the slots past the run's games are idle
template <int NW>
__global__ void __launch_bounds__(64) k_selfplay_arm(MctsDev d, SpDev r, long long num_games, float *planes,
                                                     uint8_t *needs_eval) {
    const int g = blockIdx.x;
    if (g < num_games) {
        settle<NW>(d, r, g, bb_zero<NW>(), bb_zero<NW>(), 1, 0, r.prm[0] + (int64_t)g * r.prm[1], 0, false, false, 0.0, planes,
                   needs_eval);
    } else if (lane_id() == 0) {
        GameState *st = d.state + g;
        r.alive[g] = 0;
        r.game_id[g] = -1;
        r.n_ex[g] = 0;
        st->active = 0;
        st->leaf.kind = K_NONE;
        needs_eval[g] = 0;
    }
}

#define SP_DISPATCH_NW(NWv, ...)                               \
    switch (NWv) {                                             \
        case 1: { constexpr int NW = 1; __VA_ARGS__; } break;  \
        case 2: { constexpr int NW = 2; __VA_ARGS__; } break;  \
        default: { constexpr int NW = 3; __VA_ARGS__; } break; \
    }

// ---------------------------------------------------------------------------------- host API
extern "C" int yy_selfplay_run_destroy(yy_selfplay_run *r) {
    if (!r) return YY_OK;
    for (int i = 0; i < r->n_mem; i++)
        if (r->mem[i]) (void)hipFree(r->mem[i]);
    delete r;
    return YY_OK;
}

extern "C" int yy_selfplay_run_create(yy_mcts *c, const yy_selfplay_config *cfg, yy_selfplay_run **out) {
    if (!c || !cfg || !out) return yy_tower_set_err(YY_E_INVALID, "yy_selfplay_run_create: null pointer");
    if (c->multi.K > 1)
        return yy_tower_set_err(YY_E_UNSUPPORTED, "free-running self-play: leaves_per_step > 1 is not supported (the move kernel reads the one pending leaf of a game)");
    if (c->cfg.flags & YY_FLAG_ALIASED)
        return yy_tower_set_err(YY_E_UNSUPPORTED, "free-running self-play needs copied boards (YY_FLAG_ALIASED is not supported)");
    if (cfg->num_simulations < 1 || cfg->num_simulations > c->cfg.max_sims)
        return yy_tower_set_err(YY_E_INVALID, "yy_selfplay_run_create: num_simulations outside 1 .. max_sims");
    if (cfg->fast_simulations < 0 || cfg->fast_simulations > cfg->num_simulations)
        return yy_tower_set_err(YY_E_INVALID, "yy_selfplay_run_create: fast_simulations outside 0 .. num_simulations");
    if (!(cfg->full_search_probability >= 0.0 && cfg->full_search_probability <= 1.0))
        return yy_tower_set_err(YY_E_INVALID, "yy_selfplay_run_create: full_search_probability outside [0, 1]");
    if (!(cfg->dirichlet_epsilon >= 0.0 && cfg->dirichlet_epsilon <= 1.0) ||
        (cfg->dirichlet_epsilon > 0.0 && !(cfg->dirichlet_alpha > 0.0 && cfg->dirichlet_alpha < INFINITY)))
        return yy_tower_set_err(YY_E_INVALID, "yy_selfplay_run_create: dirichlet_epsilon outside [0, 1] or dirichlet_alpha not positive and finite");
    if (cfg->example_capacity < 1) return yy_tower_set_err(YY_E_INVALID, "yy_selfplay_run_create: example_capacity < 1");
    yy_selfplay_run *r = new yy_selfplay_run();
    memset(r, 0, sizeof *r);
    r->ctx = c;
    r->cfg = *cfg;
    SpDev &s = r->dev;
    const size_t G = (size_t)c->cfg.G, A = (size_t)c->dev.geo.A, NW = (size_t)c->dev.geo.NW, T = A + 2;
    const size_t cap = (size_t)cfg->example_capacity;
    s.seed = cfg->seed;
    s.alpha = cfg->dirichlet_alpha;
    s.eps = cfg->dirichlet_epsilon;
    s.p_full = cfg->full_search_probability;
    s.thr = cfg->temperature_threshold;
    s.full_sims = cfg->num_simulations;
    s.fast_sims = cfg->fast_simulations;
    s.T = (int32_t)T;         // a game has at most A placements; passes add no example
    s.cap = (int64_t)cap;
    struct { void **p; size_t n; } allocs[] = {
        {(void **)&s.board, G * 2 * NW * sizeof(uint64_t)},
        {(void **)&s.player, G},
        {(void **)&s.ply, G * sizeof(int32_t)},
        {(void **)&s.n_ex, G * sizeof(int32_t)},
        {(void **)&s.alive, G},
        {(void **)&s.is_full, G},
        {(void **)&s.game_id, G * sizeof(int64_t)},
        {(void **)&s.h_state, G * T * A},
        {(void **)&s.h_pi, G * T * A * sizeof(float)},
        {(void **)&s.h_player, G * T},
        {(void **)&s.h_ply, G * T * sizeof(int32_t)},
        {(void **)&s.noise, G * A * sizeof(double)},
        {(void **)&s.ctr, C_COUNT * sizeof(unsigned long long)},
        {(void **)&s.prm, 2 * sizeof(int64_t)},
        {(void **)&s.ex_state, cap * A},
        {(void **)&s.ex_pi, cap * A * sizeof(float)},
        {(void **)&s.ex_z, cap * sizeof(float)},
        {(void **)&s.ex_gid, cap * sizeof(int64_t)},
        {(void **)&s.ex_ply, cap * sizeof(int64_t)},
        {(void **)&s.gumbel, c->dev.gumbel ? G * A * sizeof(float) : 0},
    };
    for (auto &a : allocs) {
        if (a.n == 0) continue;
        const hipError_t me = hipMalloc(a.p, a.n);
        if (me != hipSuccess) {
            (void)hipGetLastError();
            *a.p = nullptr;
            yy_selfplay_run_destroy(r);
            return yy_tower_set_err(YY_E_NOMEM, "yy_selfplay_run_create: hipMalloc failed");
        }
        r->mem[r->n_mem++] = *a.p;
        const hipError_t ze = hipMemset(*a.p, 0, a.n);      // every slot idle, every noise row zero
        if (ze != hipSuccess) {
            yy_selfplay_run_destroy(r);
            return yy_hip_fail("yy_selfplay_run_create: hipMemset", ze);
        }
    }
    HIP_TRY(hipDeviceSynchronize());
    if (s.gumbel) c->dev.g_rows = s.gumbel;   // Gumbel root search: the context's root expansions read the run's rows (yy_mcts_set_gumbel)
    *out = r;
    return YY_OK;
}

extern "C" int yy_selfplay_run_arm(yy_mcts *c, yy_selfplay_run *r, int64_t num_games, int64_t first_game_index,
                                   int64_t stride, float *planes, uint8_t *needs_eval, yy_stream_t s) {
    if (!c || !r || !planes || !needs_eval) return yy_tower_set_err(YY_E_INVALID, "yy_selfplay_run_arm: null pointer");
    if (r->ctx != c) return yy_tower_set_err(YY_E_INVALID, "yy_selfplay_run_arm: the run belongs to another context");
    if (num_games < 0 || first_game_index < 0 || stride < 1)
        return yy_tower_set_err(YY_E_INVALID, "yy_selfplay_run_arm: num_games < 0, first_game_index < 0 or stride < 1");
    const int G = c->cfg.G;
    hipLaunchKernelGGL(k_selfplay_reset, dim3(1), dim3(64), 0, (hipStream_t)s, r->dev, G, (long long)num_games,
                       (long long)first_game_index, (long long)stride);
    HIP_TRY(hipGetLastError());
    SP_DISPATCH_NW(c->dev.geo.NW, k_selfplay_arm<NW><<<dim3(G), dim3(64), 0, (hipStream_t)s>>>(c->dev, r->dev, (long long)num_games,
                                                                                                planes, needs_eval));
    HIP_TRY(hipGetLastError());
    c->pending = 1;    // every live slot holds a pending root expansion: the next call is yy_mcts_step_selfplay
    return YY_OK;
}

extern "C" int yy_mcts_step_selfplay(yy_mcts *c, yy_selfplay_run *r, const float *policy, const float *value, float *planes,
                                     uint8_t *needs_eval, yy_stream_t s) {
    if (!c || !r || !policy || !value || !planes || !needs_eval)
        return yy_tower_set_err(YY_E_INVALID, "yy_mcts_step_selfplay: null pointer");
    if (r->ctx != c) return yy_tower_set_err(YY_E_INVALID, "yy_mcts_step_selfplay: the run belongs to another context");
    if (c->pending != 1) return yy_tower_set_err(YY_E_STATE, "yy_mcts_step_selfplay without yy_selfplay_run_arm");
    if (int e = yy_mcts_step_noise(c, policy, value, r->dev.eps > 0.0 ? r->dev.noise : nullptr, r->dev.eps, planes, needs_eval, s))
        return e;
    SP_DISPATCH_NW(c->dev.geo.NW,
                   k_selfplay_move<NW><<<dim3(c->cfg.G), dim3(64), 0, (hipStream_t)s>>>(c->dev, r->dev, planes, needs_eval));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

extern "C" int yy_selfplay_run_counters(yy_selfplay_run *r, uint64_t *out, yy_stream_t s) {
    if (!r || !out) return yy_tower_set_err(YY_E_INVALID, "yy_selfplay_run_counters: null pointer");
    HIP_TRY(hipMemcpyAsync(out, r->dev.ctr, C_COUNT * sizeof(uint64_t), hipMemcpyDeviceToHost, (hipStream_t)s));
    return YY_OK;
}

extern "C" int yy_selfplay_run_examples(yy_selfplay_run *r, int64_t first, int64_t count, int8_t *states, float *policies,
                                        float *values, int64_t *game_id, int64_t *ply, yy_stream_t s) {
    if (!r) return yy_tower_set_err(YY_E_INVALID, "yy_selfplay_run_examples: null pointer");
    if (count == 0) return YY_OK;
    if (!states || !policies || !values || !game_id || !ply || first < 0 || count < 0 || first + count > r->dev.cap)
        return yy_tower_set_err(YY_E_INVALID, "yy_selfplay_run_examples: null pointer, or rows outside the example buffer");
    const SpDev &d = r->dev;
    const size_t A = (size_t)r->ctx->dev.geo.A, f = (size_t)first, n = (size_t)count;
    hipStream_t st = (hipStream_t)s;
    HIP_TRY(hipMemcpyAsync(states, d.ex_state + f * A, n * A, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(policies, d.ex_pi + f * A, n * A * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(values, d.ex_z + f, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(game_id, d.ex_gid + f, n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(ply, d.ex_ply + f, n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    return YY_OK;
}
