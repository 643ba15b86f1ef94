// yy_selfplay.hip -- the random draws of the episode loop as counter-based streams keyed by the GLOBAL game index.
//
// Reference: the root Dirichlet noise np.random.dirichlet([alpha] * k) at the first move of a game
// (src/yin_yang/ai/mcts.py:298-312, self_play.py:131) and the move choice np.random.choice (self_play.py:143-160) both
// draw from ONE global numpy stream in the order one process happens to reach them.  A batched engine that did the same
// (one generator over the whole [G, A] batch) makes a game's noise and moves depend on its slot, on G, on which other games
// finished and on the world size.  Here every draw is a pure function of
//     (seed, global game index, ply, purpose, element index)
// through Philox4x32-10, so game g's transcript is the same whatever slot, batch or rank plays it (SURVEY 8(d) config 2:
// per-game seeds 1000 + g; 8(e): results independent of W).
//   purpose 0 = Dirichlet noise: Gamma(alpha) per legal cell (Marsaglia-Tsang, with the U^(1/alpha) boost for alpha < 1),
//               normalised over the game's legal cells in float64; a row whose linear total is below 2^-900 (exactly 0
//               included: alpha ~ 1e-3 underflows U^(1/alpha)) is redone in log space, so no drawing row with a legal cell
//               comes out all zero (alpha >= 0.06 keeps every boosted cell above 2^-883, so such rows never take that path);
//   purpose 1 = move choice: ONE uniform u in [0, 1) per (game, ply); temperature 1: first action whose running sum of
//               pi[a] * mask[a] (ascending a, float64) exceeds u * total (uniform over the legal moves if the total is 0);
//               temperature 0: the floor(u * n)-th of the n actions tied at max(pi).
//   purpose 3 = playout cap (not in the reference): ONE uniform u in [0, 1) per (game, ply); u < p_full = a full search.
//   purpose 4 = Gumbel root search (not in the reference): g(a) = f32(-log(-log(u))) per (game, ply, action a), u a 53-bit
//               uniform strictly inside (0, 1) (yy_draws.h, gumbel_draw).
// One game per wavefront; the inverse CDF runs on lane 0 (A <= 192) so that its float64 sums have one fixed order, which the
// host restatement in tests/ reproduces bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/yy_engine.h"

#include "yy_common.h"
#include "yy_draws.h"   // the streams and the draws themselves: shared with the in-step move kernel (yy_selfplay_move.hip)

namespace sp {

// noise[g, a] = Dirichlet(alpha) over the legal cells of the games with draw[g] != 0 (zeros elsewhere: the tree kernel
// treats an all-zero row as "no noise", mcts.py:298)
__global__ void __launch_bounds__(64) k_root_noise(uint64_t seed, const int64_t *__restrict__ game_id,
                                                   const int32_t *__restrict__ ply, const uint8_t *__restrict__ drawf,
                                                   const uint8_t *__restrict__ mask, int A, double alpha,
                                                   double *__restrict__ noise) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const bool on = drawf[g] != 0;
    bool legal[3] = {false, false, false};
    int64_t gid = 0;
    int p = 0;
    if (on) {
        gid = game_id[g];
        p = ply[g];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int a = j * 64 + lane;
            legal[j] = a < A && mask[(size_t)g * A + a];
        }
    }
    dirichlet_row(seed, gid, p, on, legal, A, alpha, noise + (size_t)g * A);
}

// self_play.py:143-160; action = -1 for games that are not searching
__global__ void __launch_bounds__(64) k_sample_actions(uint64_t seed, const int64_t *__restrict__ game_id,
                                                       const int32_t *__restrict__ ply, const uint8_t *__restrict__ searching,
                                                       const double *__restrict__ pi, const uint8_t *__restrict__ mask, int A,
                                                       int temperature_threshold, int32_t *__restrict__ action) {
    const int g = blockIdx.x;
    if (threadIdx.x != 0) return;
    if (!searching[g]) {
        action[g] = -1;
        return;
    }
    const uint8_t *m = mask + (size_t)g * A;
    action[g] = pick_action(seed, game_id[g], ply[g], temperature_threshold, pi + (size_t)g * A,
                            [m](int a) { return m[a] != 0; }, A);
}

// playout-cap randomisation: the simulation budget of every searching game's next search, and whether it is a full one
__global__ void __launch_bounds__(256) k_draw_budgets(uint64_t seed, const int64_t *__restrict__ game_id,
                                                      const int32_t *__restrict__ ply, const uint8_t *__restrict__ searching,
                                                      int G, double p_full, int full_sims, int fast_sims,
                                                      int32_t *__restrict__ budgets, uint8_t *__restrict__ is_full) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    bool full = false;
    if (searching[g]) full = draw_full_search(seed, game_id[g], ply[g], p_full);
    budgets[g] = !searching[g] ? 0 : full ? full_sims : fast_sims;
    is_full[g] = full;
}

// Gumbel root search: rows[g, a] = the Gumbel variable of action a at the root of (game_id[g], ply[g]), for every a < A
__global__ void __launch_bounds__(64) k_root_gumbel(uint64_t seed, const int64_t *__restrict__ game_id,
                                                    const int32_t *__restrict__ ply, int A, float *__restrict__ rows) {
    const int g = blockIdx.x;
    const int64_t gid = game_id[g];
    const int p = ply[g];
    for (int a = threadIdx.x; a < A; a += 64) rows[(size_t)g * A + a] = gumbel_draw(seed, gid, p, a);
}

}   // namespace sp

extern "C" int yy_selfplay_root_gumbel(uint64_t seed, const int64_t *game_id, const int32_t *ply, int G, int A, float *rows,
                                       yy_stream_t s) {
    if (G == 0) return YY_OK;
    if (!game_id || !ply || !rows || G < 0 || A < 1 || A > 192)
        return yy_tower_set_err(YY_E_INVALID, "yy_selfplay_root_gumbel: bad argument");
    sp::k_root_gumbel<<<dim3(G), dim3(64), 0, (hipStream_t)s>>>(seed, game_id, ply, A, rows);
    if (hipGetLastError() != hipSuccess) return yy_tower_set_err(YY_E_HIP, "yy_selfplay_root_gumbel: launch failed");
    return YY_OK;
}

extern "C" int yy_selfplay_root_noise(uint64_t seed, const int64_t *game_id, const int32_t *ply, const uint8_t *draw,
                                      const uint8_t *mask, int G, int A, double alpha, double *noise, yy_stream_t s) {
    if (G == 0) return YY_OK;
    if (!game_id || !ply || !draw || !mask || !noise || G < 0 || A < 1 || A > 192 || !(alpha > 0.0 && alpha < INFINITY))
        return yy_tower_set_err(YY_E_INVALID, "yy_selfplay_root_noise: bad argument");
    sp::k_root_noise<<<dim3(G), dim3(64), 0, (hipStream_t)s>>>(seed, game_id, ply, draw, mask, A, alpha, noise);
    if (hipGetLastError() != hipSuccess) return yy_tower_set_err(YY_E_HIP, "yy_selfplay_root_noise: launch failed");
    return YY_OK;
}

extern "C" int yy_selfplay_sample_actions(uint64_t seed, const int64_t *game_id, const int32_t *ply, const uint8_t *searching,
                                          const double *pi, const uint8_t *mask, int G, int A, int temperature_threshold,
                                          int32_t *action, yy_stream_t s) {
    if (G == 0) return YY_OK;
    if (!game_id || !ply || !searching || !pi || !mask || !action || G < 0 || A < 1 || A > 192)
        return yy_tower_set_err(YY_E_INVALID, "yy_selfplay_sample_actions: bad argument");
    sp::k_sample_actions<<<dim3(G), dim3(64), 0, (hipStream_t)s>>>(seed, game_id, ply, searching, pi, mask, A,
                                                                   temperature_threshold, action);
    if (hipGetLastError() != hipSuccess) return yy_tower_set_err(YY_E_HIP, "yy_selfplay_sample_actions: launch failed");
    return YY_OK;
}

extern "C" int yy_selfplay_draw_budgets(uint64_t seed, const int64_t *game_id, const int32_t *ply, const uint8_t *searching,
                                        int G, double p_full, int full_sims, int fast_sims, int32_t *budgets, uint8_t *is_full,
                                        yy_stream_t s) {
    if (G == 0) return YY_OK;
    if (!game_id || !ply || !searching || !budgets || !is_full || G < 0 || full_sims < 0 || fast_sims < 0 ||
        !(p_full >= 0.0 && p_full <= 1.0))
        return yy_tower_set_err(YY_E_INVALID, "yy_selfplay_draw_budgets: bad argument");
    sp::k_draw_budgets<<<dim3((G + 255) / 256), dim3(256), 0, (hipStream_t)s>>>(seed, game_id, ply, searching, G, p_full,
                                                                                full_sims, fast_sims, budgets, is_full);
    if (hipGetLastError() != hipSuccess) return yy_tower_set_err(YY_E_HIP, "yy_selfplay_draw_budgets: launch failed");
    return YY_OK;
}
