// yy_draws.h -- the random draws of the episode loop, one copy: the counter streams and the three draws built on them.  The
// batch kernels of yy_selfplay.hip (k_root_noise, k_sample_actions, k_draw_budgets) and the in-step move kernel of
// yy_selfplay_move.hip apply these very functions, so a game's noise, moves and budgets do not depend on which of them drew.
// Every draw is a pure function of (seed, global game index, ply, purpose, element) through Philox4x32-10 (see yy_selfplay.hip);
// the evaluation symmetry of a position (draw_symmetry, used by the tree kernels through yy_tree.h) one of (seed, position).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sp {

struct U4 {
    uint32_t x, y, z, w;
};
// Philox4x32-10 (Salmon et al., SC'11): counter c, key k
__device__ __forceinline__ U4 philox(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
        U4 n;
        n.x = (uint32_t)(p1 >> 32) ^ c.y ^ k0;
        n.y = (uint32_t)p1;
        n.z = (uint32_t)(p0 >> 32) ^ c.w ^ k1;
        n.w = (uint32_t)p0;
        c = n;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}
// 53-bit uniform in [0, 1) from two words
__device__ __forceinline__ double u01(uint32_t hi, uint32_t lo) {
    return (double)((((uint64_t)hi << 32) | lo) >> 11) * 0x1.0p-53;
}
// key = seed; counter = (game index lo, game index hi, ply << 8 | purpose, element)
__device__ __forceinline__ U4 draw(uint64_t seed, int64_t game, int ply, int purpose, uint32_t element) {
    const U4 c = {(uint32_t)game, (uint32_t)((uint64_t)game >> 32), ((uint32_t)ply << 8) | (uint32_t)purpose, element};
    return philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// Gamma(alpha, 1): Marsaglia-Tsang on alpha' = alpha (+1 when alpha < 1), attempt t uses element = cell * 64 + t.
// Returns g ~ Gamma(alpha'); the cell's value is g * ub^(1/alpha) when alpha < 1 (the boost), else g.
__device__ inline double gamma_draw(uint64_t seed, int64_t game, int ply, int cell, double alpha, double &ub) {
    const bool boost = alpha < 1.0;
    const double a = boost ? alpha + 1.0 : alpha;
    const double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double g = d;     // value if 64 attempts were all rejected (probability < 1e-80)
    ub = 0.5;
    for (int t = 0; t < 64; t++) {
        const U4 r = draw(seed, game, ply, 0, (uint32_t)(cell * 64 + t));
        const U4 q = draw(seed, game, ply, 2, (uint32_t)(cell * 64 + t));
        const double u1 = 1.0 - u01(r.x, r.y), u2 = u01(r.z, r.w);      // u1 in (0, 1]
        const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
        const double v1 = 1.0 + c * z;
        if (v1 <= 0.0) continue;
        const double v = v1 * v1 * v1;
        const double u3 = 1.0 - u01(q.x, q.y);
        if (log(u3) < 0.5 * z * z + d - d * v + d * log(v)) {
            g = d * v;
            ub = 1.0 - u01(q.z, q.w);
            break;
        }
    }
    return g;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// One game's noise row by its wavefront: noise[a] = Dirichlet(alpha) over the legal cells when `on` (wave-uniform), zeros
// otherwise (the tree kernel treats an all-zero row as "no noise", mcts.py:298).  Lane l owns the cells l, l + 64, l + 128;
// legal[j] says whether cell j * 64 + l is a legal move (false for a cell >= A).
__device__ __forceinline__ void dirichlet_row(uint64_t seed, int64_t gid, int p, bool on, const bool legal_in[3], int A,
                                              double alpha, double *__restrict__ noise) {
    const int lane = threadIdx.x;
    const bool boost = alpha < 1.0;
    double x[3] = {0.0, 0.0, 0.0}, gm[3] = {0.0, 0.0, 0.0}, ub[3] = {1.0, 1.0, 1.0}, part = 0.0;
    bool legal[3] = {false, false, false};
    if (on) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int a = j * 64 + lane;
            if (a < A && legal_in[j]) {
                legal[j] = true;
                gm[j] = gamma_draw(seed, gid, p, a, alpha, ub[j]);
                x[j] = boost ? gm[j] * pow(ub[j], 1.0 / alpha) : gm[j];
                part += x[j];
            }
        }
    }
    // one fixed summation order: lanes' partial sums (cells a, a+64, a+128) combined by the xor butterfly
    double tot = wave_sum_f64(part);
    if (on && tot < 0x1.0p-900) {       // wave-uniform: redo the row in log space, relative to the row's largest cell
        double lx[3];
#pragma unroll
        for (int j = 0; j < 3; j++)
            lx[j] = !legal[j] ? -INFINITY : boost ? log(gm[j]) + log(ub[j]) / alpha : log(gm[j]);
        const double m = wave_max_f64(fmax(fmax(lx[0], lx[1]), lx[2]));
        part = 0.0;
        if (m > -INFINITY) {            // at least one legal cell
#pragma unroll
            for (int j = 0; j < 3; j++) {
                x[j] = legal[j] ? exp(lx[j] - m) : 0.0;
                part += x[j];
            }
        }
        tot = wave_sum_f64(part);
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int a = j * 64 + lane;
        if (a < A) noise[a] = (on && tot > 0.0) ? x[j] / tot : 0.0;
    }
}

// self_play.py:143-160 on one thread: the move of (game gid, ply) from its distribution p[0 .. A) and legal(a); -1 when there
// is nothing to pick.  ONE uniform u: temperature 1 (ply < temperature_threshold): the first action whose running sum of
// p[a] * legal(a) exceeds u * total (uniform over the legal moves if the total is 0); temperature 0: the floor(u * n)-th of the
// n actions tied at max(p).
template <class Legal>
__device__ __forceinline__ int pick_action(uint64_t seed, int64_t gid, int ply, int temperature_threshold, const double *p,
                                           Legal legal_at, int A) {
    const U4 r = draw(seed, gid, ply, 1, 0u);
    const double u = u01(r.x, r.y);
    int pick = -1;
    if (ply < temperature_threshold) {               // temperature 1: p = pi * valid / sum (:150-160)
        double tot = 0.0;
        int legal = 0;
        for (int a = 0; a < A; a++) {
            tot += legal_at(a) ? p[a] : 0.0;
            legal += legal_at(a) ? 1 : 0;
        }
        if (tot > 0.0) {
            const double target = u * tot;
            double c = 0.0;
            for (int a = 0; a < A; a++) {
                const double w = legal_at(a) ? p[a] : 0.0;
                c += w;
                if (w > 0.0) {
                    pick = a;                           // remembers the last action with mass (rounding guard)
                    if (c > target) break;
                }
            }
        } else if (legal > 0) {                         // uniform over the legal moves (:156-158)
            int k = min((int)(u * (double)legal), legal - 1);
            for (int a = 0; a < A; a++)
                if (legal_at(a) && k-- == 0) { pick = a; break; }
        }
    } else {                                            // temperature 0: random arg-max (:143-146)
        double mx = p[0];
        for (int a = 1; a < A; a++) mx = fmax(mx, p[a]);
        int n = 0;
        for (int a = 0; a < A; a++) n += (p[a] == mx);
        int k = min((int)(u * (double)n), n - 1);
        for (int a = 0; a < A; a++)
            if (p[a] == mx && k-- == 0) { pick = a; break; }
    }
    return pick;
}

// playout-cap randomisation: ONE uniform u per (game, ply), purpose 3; u < p_full = the search of this move is a full one
__device__ __forceinline__ bool draw_full_search(uint64_t seed, int64_t gid, int ply, double p_full) {
    const U4 r = draw(seed, gid, ply, 3, 0u);
    return u01(r.x, r.y) < p_full;
}

// Gumbel root search (YY_FLAG_GUMBEL_ROOT): the Gumbel(0, 1) variable of action a at the root of (game, ply), purpose 4 (0 .. 3
// are the streams above): g = f32(-log(-log(u))) in float64, u the 53-bit uniform of the block's first two words, strictly
// inside (0, 1) -- the one value u01 can give outside it, 0, is replaced by 2^-54.
#define YY_DRAW_GUMBEL 4
__device__ __forceinline__ float gumbel_draw(uint64_t seed, int64_t gid, int ply, int a) {
    const U4 r = draw(seed, gid, ply, YY_DRAW_GUMBEL, (uint32_t)a);
    double u = u01(r.x, r.y);
    if (u == 0.0) u = 0x1.0p-54;
    return (float)(-log(-log(u)));
}

// symmetry-randomised evaluation: the symmetry a POSITION is evaluated under, a pure function of (seed, black, white) -- not
// of game, ply, slot or batch.  The four counter words of every block are taken by the position, so the domain tag sits in the
// key: seed ^ SYM_TAG, where every other stream keys with the seed itself.  The NW word pairs are chained: block i has the
// counter (black[i] lo, black[i] hi, white[i] lo, white[i] hi) ^ the output of block i - 1 (zero for i = 0).  The draw is
// the top bits of the last block's first word: uniform over `group` = 8 (square boards) or 4 elements.
#define YY_SYM_TAG 0x59595F53594D5F34ull   // "YY_SYM_4": purposes 0 .. 3 are the streams above
__host__ __device__ __forceinline__ int symmetry_group(int R, int C) { return R == C ? 8 : 4; }
__device__ __forceinline__ int draw_symmetry(uint64_t seed, const uint64_t *black, const uint64_t *white, int nw, int group) {
    const uint64_t key = seed ^ YY_SYM_TAG;
    U4 h = {0u, 0u, 0u, 0u};
    for (int i = 0; i < nw; i++) {
        const U4 c = {h.x ^ (uint32_t)black[i], h.y ^ (uint32_t)(black[i] >> 32), h.z ^ (uint32_t)white[i],
                      h.w ^ (uint32_t)(white[i] >> 32)};
        h = philox(c, (uint32_t)key, (uint32_t)(key >> 32));
    }
    return (int)(h.x >> (group == 8 ? 29 : 30));
}

}   // namespace sp
