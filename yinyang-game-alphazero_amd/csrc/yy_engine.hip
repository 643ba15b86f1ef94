// yy_engine.hip -- HIP kernels + C ABI (include/yy_engine.h) of the Yin-Yang self-play hot path
// for MI355X (gfx950, wave64).  Written for CDNA4 only.  Two parts: the stateless rules kernels and the MCTS context
// (tree kernels for K = 1 and K > 1 leaves per step on shared building blocks, read-out, book).  The evaluator's kernels are
// in yy_tower*.hip, yy_fc_heads.hip and yy_nn_epilogue.hip, the episode loop's draws in yy_selfplay.hip.
//
// Execution model
//   * tree kernels: ONE GAME PER WAVEFRONT (block = 64 threads, blockIdx.x = game).  Lane l owns
//     board cell(s) l, l+64, l+128 and child edge(s) l, l+64, ... of the node being scanned, so a
//     node's children are read with one coalesced 16-B-per-lane load, the PUCT arg-max is a
//     wave reduction, the legal mask -> child list compaction is a ballot/mbcnt prefix sum, and
//     the 5 input planes are written as coalesced rows.  Bitboards are wave-uniform (SGPRs).
//   * stateless rules kernels: ONE GAME PER LANE on the same bitboard code, boards staged through
//     LDS so the int8 [G,R,C] tensors are read/written coalesced.
//   * blockIdx -> game is fixed, and blocks are dealt round-robin over the 8 XCDs, so a game's
//     arena stays in the same XCD's L2 from launch to launch (speed only, never correctness).
//
// HBM layout (all per context, game-major):
//   edges  uint4 [G][edge_cap]   {prior f32, visits i32, value_sum f32, child(24b)|action<<24}
//   nodes  uint4 [G][node_cap]   {first_edge, k | flags<<16 | player<<24, terminal value f32, -}
//   nboard u64   [G][node_cap][2*NW]   (copied mode only) black words then white words
//   gboard u64   [G][2*NW]       root board (copied) / THE shared board (aliased)
//   path   i32   [G][K][path_cap]   edge indices chosen by the last selection (K = leaves per step, 1 by default)
//   state  GameState [G]         counters, root statistics, the pending leaf record
//   leaves LeafRec [G][K]        (K > 1 only) the pending leaf record of every descent of the step
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../include/yy_engine.h"
#include "yy_bitboard.h"
#include "yy_common.h"
#include "yy_tree.h"

#define YY_VERSION 111

// ------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
static int set_err(int code, const char *fmt, const char *a = "", const char *b = "") {
    snprintf(g_err, sizeof g_err, fmt, a, b);
    return code;
}

extern "C" const char *yy_last_error(void) { return g_err; }
extern "C" int yy_tower_set_err(int code, const char *msg) { return set_err(code, "%s%s", msg); }   // for the other .hip files (yy_common.h)
extern "C" int yy_version(void) { return YY_VERSION; }

static int check_geo(int G, int R, int C) {
    if (G <= 0 || R <= 0 || C <= 0) return set_err(YY_E_INVALID, "non-positive size%s%s");
    if (R > YY_MAX_DIM || C > YY_MAX_DIM || R * C > 64 * YY_MAX_NW)
        return set_err(YY_E_UNSUPPORTED, "board larger than 16x16 / 192 cells%s%s");
    return YY_OK;
}

// ------------------------------------------------------------------------------------ helpers
// Wave64 reductions on the VALU with DPP (row_shr 1/2/4/8 scan inside each 16-lane row, then row_bcast15 /
// row_bcast31 across rows; lane 63 ends up with the total): ~6 dependent VALU ops instead of 6 LDS-crossbar
// shuffles.  Used on the latency-critical PUCT descent.
#define YY_DPP_STEP(OP, ID, v, ctrl, rmask) \
    v = OP(v, (uint32_t)__builtin_amdgcn_update_dpp((int)(ID), (int)(v), ctrl, rmask, 0xf, false))
__device__ __forceinline__ uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t uadd32(uint32_t a, uint32_t b) { return a + b; }
__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
    YY_DPP_STEP(umax32, 0u, v, 0x111, 0xf);
    YY_DPP_STEP(umax32, 0u, v, 0x112, 0xf);
    YY_DPP_STEP(umax32, 0u, v, 0x114, 0xf);
    YY_DPP_STEP(umax32, 0u, v, 0x118, 0xf);
    YY_DPP_STEP(umax32, 0u, v, 0x142, 0xa);
    YY_DPP_STEP(umax32, 0u, v, 0x143, 0xc);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_umin(uint32_t v) {
    YY_DPP_STEP(umin32, 0xFFFFFFFFu, v, 0x111, 0xf);
    YY_DPP_STEP(umin32, 0xFFFFFFFFu, v, 0x112, 0xf);
    YY_DPP_STEP(umin32, 0xFFFFFFFFu, v, 0x114, 0xf);
    YY_DPP_STEP(umin32, 0xFFFFFFFFu, v, 0x118, 0xf);
    YY_DPP_STEP(umin32, 0xFFFFFFFFu, v, 0x142, 0xa);
    YY_DPP_STEP(umin32, 0xFFFFFFFFu, v, 0x143, 0xc);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_uadd(uint32_t v) {
    YY_DPP_STEP(uadd32, 0u, v, 0x111, 0xf);
    YY_DPP_STEP(uadd32, 0u, v, 0x112, 0xf);
    YY_DPP_STEP(uadd32, 0u, v, 0x114, 0xf);
    YY_DPP_STEP(uadd32, 0u, v, 0x118, 0xf);
    YY_DPP_STEP(uadd32, 0u, v, 0x142, 0xa);
    YY_DPP_STEP(uadd32, 0u, v, 0x143, 0xc);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// The same scan on 64-bit integers (sums modulo 2^64, so two's-complement values add as well): both halves move by the same
// DPP control, the add carries between them.
#define YY_DPP_STEP64(v, ctrl, rmask)                                                                                     \
    v += ((uint64_t)(uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), ctrl, rmask, 0xf, false) << 32) | \
         (uint64_t)(uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, ctrl, rmask, 0xf, false)
__device__ __forceinline__ uint64_t wave_uadd64(uint64_t v) {
    YY_DPP_STEP64(v, 0x111, 0xf);
    YY_DPP_STEP64(v, 0x112, 0xf);
    YY_DPP_STEP64(v, 0x114, 0xf);
    YY_DPP_STEP64(v, 0x118, 0xf);
    YY_DPP_STEP64(v, 0x142, 0xa);
    YY_DPP_STEP64(v, 0x143, 0xc);
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63) << 32) |
           (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
}

// ------------------------------------------------------------------------- stateless kernels
// One game per lane; the block's boards (64 games x A bytes, contiguous in HBM) are staged through
// LDS so global traffic is coalesced.
#define RULES_BLOCK 64

template <int NW>
__device__ __forceinline__ void lds_board_to_bb(const int8_t *lb, int A, BB<NW> &black, BB<NW> &white) {
    black = bb_zero<NW>();
    white = bb_zero<NW>();
    for (int a = 0; a < A; a++) {
        int v = lb[a];
        if (v == 1) black.w[a >> 6] |= 1ull << (a & 63);
        if (v == -1) white.w[a >> 6] |= 1ull << (a & 63);
    }
}

// stage this block's boards global -> LDS (coalesced bytes)
__device__ __forceinline__ void stage_in(int8_t *lds, const int8_t *boards, int g0, int ng, int A) {
    const int n = ng * A;
    const int8_t *src = boards + (size_t)g0 * A;
    for (int i = threadIdx.x; i < n; i += blockDim.x) lds[i] = src[i];
    __syncthreads();
}

template <int NW>
__global__ void __launch_bounds__(RULES_BLOCK) k_valid_mask(const int8_t *boards, const int8_t *players,
                                                            int G, YYGeo geo, uint8_t *out) {
    __shared__ int8_t lds[RULES_BLOCK * 64 * YY_MAX_NW];
    const int A = geo.A, g0 = blockIdx.x * RULES_BLOCK;
    const int ng = min(RULES_BLOCK, G - g0);
    stage_in(lds, boards, g0, ng, A);
    const int g = g0 + threadIdx.x;
    BB<NW> mask = bb_zero<NW>();
    if (threadIdx.x < ng) {
        GeoBB<NW> gb = geo_bb<NW>(geo);
        BB<NW> black, white;
        lds_board_to_bb<NW>(lds + threadIdx.x * A, A, black, white);
        bool pre = bb_pre2x2(black, white, gb);
        mask = (players[g] == 1) ? bb_legal(black, white, pre, geo, gb) : bb_legal(white, black, pre, geo, gb);
    }
    __syncthreads();
    if (threadIdx.x < ng)
        for (int a = 0; a < A; a++) lds[threadIdx.x * A + a] = (int8_t)bb_test(mask, a);
    __syncthreads();
    uint8_t *dst = out + (size_t)g0 * A;
    for (int i = threadIdx.x; i < ng * A; i += blockDim.x) dst[i] = (uint8_t)lds[i];
}

template <int NW>
__global__ void __launch_bounds__(RULES_BLOCK) k_step(int8_t *boards, int8_t *players, const int32_t *actions,
                                                      int G, YYGeo geo, uint8_t *placed) {
    const int g = blockIdx.x * RULES_BLOCK + threadIdx.x;
    if (g >= G) return;
    const int A = geo.A;
    GeoBB<NW> gb = geo_bb<NW>(geo);
    BB<NW> black = bb_zero<NW>(), white = bb_zero<NW>();
    int8_t *b = boards + (size_t)g * A;
    for (int a = 0; a < A; a++) {
        int v = b[a];
        if (v == 1) black.w[a >> 6] |= 1ull << (a & 63);
        if (v == -1) white.w[a >> 6] |= 1ull << (a & 63);
    }
    const int p = players[g], a = actions[g];
    const bool ok = bb_play<NW>(geo, gb, black, white, p, a);
    if (ok) b[a] = (p == 1) ? 1 : -1;  // yin_yang_game.py:55-56
    players[g] = (int8_t)-p;           // yin_yang_game.py:58, regardless
    if (placed) placed[g] = ok;
}

template <int NW>
__global__ void __launch_bounds__(RULES_BLOCK) k_game_ended(const int8_t *boards, const int8_t *players, int G,
                                                            YYGeo geo, double *out, int32_t *counts) {
    __shared__ int8_t lds[RULES_BLOCK * 64 * YY_MAX_NW];
    const int A = geo.A, g0 = blockIdx.x * RULES_BLOCK;
    const int ng = min(RULES_BLOCK, G - g0);
    stage_in(lds, boards, g0, ng, A);
    if (threadIdx.x >= ng) return;
    const int g = g0 + threadIdx.x;
    GeoBB<NW> gb = geo_bb<NW>(geo);
    BB<NW> black, white;
    lds_board_to_bb<NW>(lds + threadIdx.x * A, A, black, white);
    out[g] = bb_game_ended<NW>(geo, gb, black, white, players[g]);
    if (counts) {
        counts[2 * g] = bb_popc(black);
        counts[2 * g + 1] = bb_popc(white);
    }
}

template <int NW>
__global__ void __launch_bounds__(64) k_encode(const int8_t *boards, int G, YYGeo geo, float *out) {
    const int g = blockIdx.x;
    BB<NW> black, white;
    board_to_bb<NW>(boards + (size_t)g * geo.A, geo.A, black, white);
    write_planes<NW>(out + (size_t)g * 5 * geo.A, geo, black, white);
}

// k_encode under symmetry-randomised evaluation: the row the tree kernels write for this position (write_eval_planes) and / or
// the symmetry it was drawn (either output may be null)
template <int NW>
__global__ void __launch_bounds__(64) k_encode_sym(const int8_t *boards, int G, YYGeo geo, uint64_t seed, float *out,
                                                   int8_t *sym_out) {
    const int g = blockIdx.x;
    BB<NW> black, white;
    board_to_bb<NW>(boards + (size_t)g * geo.A, geo.A, black, white);
    if (sym_out && lane_id() == 0) sym_out[g] = (int8_t)sym_of<NW>(geo, seed, black, white);
    if (out) write_eval_planes<NW>(out + (size_t)g * 5 * geo.A, geo, 1u, seed, black, white);
}

template <int NW>
__global__ void __launch_bounds__(64) k_pack(const int8_t *boards, int G, YYGeo geo, uint64_t *black, uint64_t *white) {
    const int g = blockIdx.x;
    BB<NW> b, w;
    board_to_bb<NW>(boards + (size_t)g * geo.A, geo.A, b, w);
    if (lane_id() == 0) {
#pragma unroll
        for (int j = 0; j < NW; j++) {
            black[(size_t)j * G + g] = b.w[j];
            white[(size_t)j * G + g] = w.w[j];
        }
    }
}

template <int NW>
__global__ void __launch_bounds__(64) k_unpack(const uint64_t *black, const uint64_t *white, int G, YYGeo geo,
                                               int8_t *boards) {
    const int g = blockIdx.x;
    BB<NW> b, w;
#pragma unroll
    for (int j = 0; j < NW; j++) {
        b.w[j] = rfl64(black[(size_t)j * G + g]);
        w.w[j] = rfl64(white[(size_t)j * G + g]);
    }
    bb_to_board<NW>(boards + (size_t)g * geo.A, geo.A, b, w);
}

// packed rules: one game per lane, SoA word-major bitboards -> fully coalesced 8-B loads/stores
template <int NW>
__global__ void __launch_bounds__(256) k_mask_terminal_bb(const uint64_t *black, const uint64_t *white, int G,
                                                          YYGeo geo, uint64_t *m1, uint64_t *m2, int8_t *result) {
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < G; g += gridDim.x * blockDim.x) {
        GeoBB<NW> gb = geo_bb<NW>(geo);
        BB<NW> b, w;
#pragma unroll
        for (int j = 0; j < NW; j++) {
            b.w[j] = black[(size_t)j * G + g];
            w.w[j] = white[(size_t)j * G + g];
        }
        bool pre = bb_pre2x2(b, w, gb);
        BB<NW> mb = bb_legal(b, w, pre, geo, gb), mw = bb_legal(w, b, pre, geo, gb);
#pragma unroll
        for (int j = 0; j < NW; j++) {
            if (m1) m1[(size_t)j * G + g] = mb.w[j];
            if (m2) m2[(size_t)j * G + g] = mw.w[j];
        }
        if (result) result[g] = (int8_t)bb_result_black(b, w, mb, mw);
    }
}

#define DISPATCH_NW(NWv, ...)                                  \
    switch (NWv) {                                             \
        case 1: { constexpr int NW = 1; __VA_ARGS__; } break;  \
        case 2: { constexpr int NW = 2; __VA_ARGS__; } break;  \
        default: { constexpr int NW = 3; __VA_ARGS__; } break; \
    }

extern "C" int yy_rules_valid_mask(const int8_t *boards, const int8_t *players, int G, int R, int C, uint32_t flags,
                                   uint8_t *out, yy_stream_t s) {
    if (G == 0) return YY_OK;
    if (int e = check_geo(G, R, C)) return e;
    if (!boards || !players || !out) return set_err(YY_E_INVALID, "null pointer%s%s");
    YYGeo geo;
    yy_make_geo(&geo, R, C, flags);
    dim3 grid((G + RULES_BLOCK - 1) / RULES_BLOCK);
    DISPATCH_NW(geo.NW, k_valid_mask<NW><<<grid, dim3(RULES_BLOCK), 0, (hipStream_t)s>>>(boards,
                                            players, G, geo, out));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

extern "C" int yy_rules_step(int8_t *boards, int8_t *players, const int32_t *actions, int G, int R, int C,
                             uint32_t flags, uint8_t *placed, yy_stream_t s) {
    if (G == 0) return YY_OK;
    if (int e = check_geo(G, R, C)) return e;
    if (!boards || !players || !actions) return set_err(YY_E_INVALID, "null pointer%s%s");
    YYGeo geo;
    yy_make_geo(&geo, R, C, flags);
    dim3 grid((G + RULES_BLOCK - 1) / RULES_BLOCK);
    DISPATCH_NW(geo.NW, k_step<NW><<<grid, dim3(RULES_BLOCK), 0, (hipStream_t)s>>>(boards, players,
                                            actions, G, geo, placed));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

extern "C" int yy_rules_game_ended(const int8_t *boards, const int8_t *players, int G, int R, int C, uint32_t flags,
                                   double *out, int32_t *counts, yy_stream_t s) {
    if (G == 0) return YY_OK;
    if (int e = check_geo(G, R, C)) return e;
    if (!boards || !players || !out) return set_err(YY_E_INVALID, "null pointer%s%s");
    YYGeo geo;
    yy_make_geo(&geo, R, C, flags);
    dim3 grid((G + RULES_BLOCK - 1) / RULES_BLOCK);
    DISPATCH_NW(geo.NW, k_game_ended<NW><<<grid, dim3(RULES_BLOCK), 0, (hipStream_t)s>>>(boards,
                                            players, G, geo, out, counts));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

extern "C" int yy_encode_planes(const int8_t *boards, int G, int R, int C, float *out, yy_stream_t s) {
    if (G == 0) return YY_OK;
    if (int e = check_geo(G, R, C)) return e;
    if (!boards || !out) return set_err(YY_E_INVALID, "null pointer%s%s");
    YYGeo geo;
    yy_make_geo(&geo, R, C, 0);
    DISPATCH_NW(geo.NW, k_encode<NW><<<dim3(G), dim3(64), 0, (hipStream_t)s>>>(boards, G, geo, out));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

static int encode_sym(const int8_t *boards, int G, int R, int C, uint64_t seed, float *out, int8_t *sym_out, yy_stream_t s) {
    if (G == 0) return YY_OK;
    if (int e = check_geo(G, R, C)) return e;
    if (!boards || (!out && !sym_out)) return set_err(YY_E_INVALID, "null pointer%s%s");
    YYGeo geo;
    yy_make_geo(&geo, R, C, 0);
    DISPATCH_NW(geo.NW, k_encode_sym<NW><<<dim3(G), dim3(64), 0, (hipStream_t)s>>>(boards, G, geo, seed, out, sym_out));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

extern "C" int yy_encode_planes_sym(const int8_t *boards, int G, int R, int C, uint64_t seed, float *out, yy_stream_t s) {
    return encode_sym(boards, G, R, C, seed, out, nullptr, s);
}

extern "C" int yy_eval_symmetry(const int8_t *boards, int G, int R, int C, uint64_t seed, int8_t *out, yy_stream_t s) {
    return encode_sym(boards, G, R, C, seed, nullptr, out, s);
}

extern "C" int yy_pack_boards(const int8_t *boards, int G, int R, int C, uint64_t *black, uint64_t *white,
                              yy_stream_t s) {
    if (G == 0) return YY_OK;
    if (int e = check_geo(G, R, C)) return e;
    if (!boards || !black || !white) return set_err(YY_E_INVALID, "null pointer%s%s");
    YYGeo geo;
    yy_make_geo(&geo, R, C, 0);
    DISPATCH_NW(geo.NW,
                k_pack<NW><<<dim3(G), dim3(64), 0, (hipStream_t)s>>>(boards, G, geo, black, white));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

extern "C" int yy_unpack_boards(const uint64_t *black, const uint64_t *white, int G, int R, int C, int8_t *boards,
                                yy_stream_t s) {
    if (G == 0) return YY_OK;
    if (int e = check_geo(G, R, C)) return e;
    if (!boards || !black || !white) return set_err(YY_E_INVALID, "null pointer%s%s");
    YYGeo geo;
    yy_make_geo(&geo, R, C, 0);
    DISPATCH_NW(geo.NW,
                k_unpack<NW><<<dim3(G), dim3(64), 0, (hipStream_t)s>>>(black, white, G, geo, boards));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

extern "C" int yy_rules_mask_terminal_bb(const uint64_t *black, const uint64_t *white, int G, int R, int C,
                                         uint32_t flags, uint64_t *m1, uint64_t *m2, int8_t *result, yy_stream_t s) {
    if (G == 0) return YY_OK;
    if (int e = check_geo(G, R, C)) return e;
    if (!black || !white) return set_err(YY_E_INVALID, "null pointer%s%s");
    YYGeo geo;
    yy_make_geo(&geo, R, C, flags);
    int blocks = (G + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    DISPATCH_NW(geo.NW, k_mask_terminal_bb<NW><<<dim3(blocks), dim3(256), 0, (hipStream_t)s>>>(black,
                                            white, G, geo, m1, m2, result));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

// =============================================================================== MCTS context
#define TT_PROBES 8

// slot hash of a position: murmur3's 64-bit finalizer after every word -- positions of one search differ in a few bits, and a
// single multiply leaves the low bits (the slot index) clustered (measured: probe runs of 8 at 5 % load)
template <int NW> __device__ __forceinline__ uint64_t bb_hash(const uint64_t *black, const uint64_t *white) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (int i = 0; i < 2 * NW; i++) {
        h ^= (i < NW) ? black[i] : white[i - NW];
        h ^= h >> 33;
        h *= 0xFF51AFD7ED558CCDull;
        h ^= h >> 33;
        h *= 0xC4CEB9FE1A85EC53ull;
        h ^= h >> 33;
    }
    return h;
}

// ---- the position table: each of probe sequence, key compare and stone count exists once, for the cache, the book's
// lookup and the book's build (k_book_insert)
// The probe sequence of hash h in a table of mask + 1 slots: TT_PROBES slots from tt_first on, linear, wrapping.  visit(slot)
// says whether to go on, that the position is not there, or that this is its slot: the slot is returned, else -1.
enum TTStep { TT_NEXT, TT_MISS, TT_HIT };
__device__ __forceinline__ uint32_t tt_first(uint64_t h, uint32_t mask) { return (uint32_t)h & mask; }
template <class F> __device__ __forceinline__ int tt_probe(uint64_t h, uint32_t mask, F visit) {
    uint32_t at = tt_first(h, mask);
    for (int pr = 0; pr < TT_PROBES; pr++, at = (at + 1u) & mask) {
        const TTStep r = visit(at);
        if (r == TT_HIT) return (int)at;
        if (r == TT_MISS) break;
    }
    return -1;
}
// slot `at` holds the position (black, white): every word is compared, the hash only picks the probe sequence
template <int NW> __device__ __forceinline__ bool tt_key_is(const PosTable &t, uint32_t at, BB<NW> black, BB<NW> white) {
    const uint64_t *k = t.key + (size_t)at * 2 * NW;
    const BB<NW> ob = bb_uniform_load<NW>(k), ow = bb_uniform_load<NW>(k + NW);
    bool same = true;
#pragma unroll
    for (int i = 0; i < NW; i++) same = same && ob.w[i] == black.w[i] && ow.w[i] == white.w[i];
    return same;
}

template <int NW> __device__ __forceinline__ PosTable cache_of(const MctsDev &d, const int g) {
    const size_t o = (size_t)g * ((size_t)d.ec.mask + 1);
    return PosTable{d.ec.meta + o, d.ec.key + o * 2 * NW, d.ec.val + o, d.ec.pol + o * d.geo.A, d.ec.mask};
}

// Where a leaf's evaluation comes from (GameState.leaf_src): the evaluator, slot s of the game's cache, slot s of the book,
// slot s of the shared evaluation table (a cache has at most 2^26 slots per game, the shared table at most 2^30)
#define SRC_NONE (-1)
#define SRC_SHARED 0x40000000
__device__ __forceinline__ int src_cache(uint32_t s) { return (int)s; }
__device__ __forceinline__ int src_book(uint32_t s) { return -2 - (int)s; }
__device__ __forceinline__ int src_shared(uint32_t s) { return (int)s | SRC_SHARED; }

// Evaluation cache: the evaluator is a function of the position alone (the planes encode the board, not the side to move),
// so a position it has already seen -- another move order inside this search, a pass node visited again, with
// YY_FLAG_KEEP_EVALUATIONS an earlier search of the same game, or one of the book -- needs no evaluator row: the stored
// policy row and value ARE this leaf's evaluation.  Returns the leaf_src of the position (black, white); on SRC_NONE with a
// cache, `slot` is where cache_store puts the fresh evaluation (else -1).  The order is book, the game's own cache, the shared
// table; `stamp` is the step stamp of this launch (shared table only).
template <int NW>
__device__ __forceinline__ int leaf_lookup(const MctsDev &d, const GameState *st, const int g, BB<NW> black, BB<NW> white,
                                           int &slot, const uint32_t stamp) {
    slot = -1;
    if (!d.ec.meta && !d.bk.meta && !d.sh.meta) return SRC_NONE;
    const uint64_t h = bb_hash<NW>(black.w, white.w);
    // the shared book: positions of the first plies evaluated once for ALL games before play; read-only
    if (d.bk.meta && pos_stones<NW>(black, white) <= d.bk_stones) {
        const int at = tt_probe(h, d.bk.mask, [&](uint32_t at) {
            if (rfl((int)d.bk.meta[at]) == 0) return TT_MISS;                      // never used: the position is not in the book
            return tt_key_is<NW>(d.bk, at, black, white) ? TT_HIT : TT_NEXT;
        });
        if (at >= 0) return src_book((uint32_t)at);
    }
    if (d.ec.meta) {
        const PosTable t = cache_of<NW>(d, g);
        const uint32_t ep = (uint32_t)rfl((int)st->ec_epoch);
        const int rstones = rfl(st->root_stones);
        const int at = tt_probe(h, t.mask, [&](uint32_t at) {
            const uint32_t m = (uint32_t)rfl((int)t.meta[at]);
            if (m == 0u) { if (slot < 0) slot = (int)at; return TT_MISS; }         // never used: the position is not in the table
            const bool cur = (m >> 8) == ep;
            if ((cur || d.ec_keep) && tt_key_is<NW>(t, at, black, white)) return TT_HIT;
            // replaceable: another epoch, or a position that cannot come back (a leaf has more stones than the root)
            if (slot < 0 && (!cur || (int)(m & 0xFFu) <= rstones)) slot = (int)at;
            return TT_NEXT;
        });
        if (slot < 0) slot = (int)tt_first(h, t.mask);                             // every probed entry is live: replace the first
        if (at >= 0) return src_cache((uint32_t)at);
    }
    // the shared evaluation table: what any game of the context had evaluated in an EARLIER launch.  An entry that carries this
    // launch's stamp is passed over -- another workgroup may still be writing its key and row, and nothing of this launch has
    // been published (no fence, no acquire: the kernel boundary publishes) -- so everything trusted here was complete before
    // this launch began.  A stale 0 read for a slot claimed in this launch ends the probe one entry early: a miss, never a wrong hit.
    // Replacing mode (d.sh_claim, the second branch): the stamp is the low half of the slot's claim word;
    // an evicted slot (SH_TOMBSTONE, stale or claimed again in this launch alike) is passed over, not the end of the chain --
    // entries behind it were inserted while it was taken; and a hit leaves this launch's stamp in the slot's last-hit word (a
    // plain store: every writer of a launch writes the same value, and the sweep that reads it is a later launch)
    if (d.sh.meta && !d.sh_claim) {
        const int at = tt_probe(h, d.sh.mask, [&](uint32_t at) {
            const uint32_t m = (uint32_t)rfl((int)d.sh.meta[at]);
            if (m == 0u) return TT_MISS;
            if (m == stamp) return TT_NEXT;
            return tt_key_is<NW>(d.sh, at, black, white) ? TT_HIT : TT_NEXT;
        });
        if (at >= 0) return src_shared((uint32_t)at);
    } else if (d.sh_claim) {
        const uint32_t *low = (const uint32_t *)d.sh_claim;       // the stamp: the low half of a claim word (little-endian)
        const int at = tt_probe(h, d.sh.mask, [&](uint32_t at) {
            const uint32_t m = (uint32_t)rfl((int)low[2 * (size_t)at]);
            if (m == 0u) return TT_MISS;
            if (m == stamp || m == SH_TOMBSTONE) return TT_NEXT;
            return tt_key_is<NW>(d.sh, at, black, white) ? TT_HIT : TT_NEXT;
        });
        if (at >= 0) {
            if (lane_id() == 0) d.sh_hit[at] = stamp;
            return src_shared((uint32_t)at);
        }
    }
    return SRC_NONE;
}

// the evaluation of game g's pending leaf: its policy row and value, from the evaluator's row g or the slot `src` names.
// value == nullptr: the root call, whose value is discarded (mcts.py:288; yy_mcts_expand_root is not given it)
struct LeafEval { const float *prow; float v; };
template <int NW>
__device__ __forceinline__ LeafEval leaf_eval(const MctsDev &d, const int g, const int src, const float *policy,
                                              const float *value) {
    if (src == SRC_NONE) return LeafEval{policy + (size_t)g * d.geo.A, value ? rflf(value[g]) : 0.0f};
    if (src >= SRC_SHARED) {                                                       // only ever set with a shared table
        const size_t s = (size_t)(src - SRC_SHARED);
        return LeafEval{d.sh.pol + s * d.geo.A, rflf(d.sh.val[s])};
    }
    const bool book = src < SRC_NONE;
    const PosTable t = book ? d.bk : cache_of<NW>(d, g);
    const size_t s = (size_t)(book ? -2 - src : src);
    return LeafEval{t.pol + s * d.geo.A, rflf(t.val[s])};
}

// a fresh evaluation (the evaluator's row g, value v) of game g's pending leaf goes into the cache slot leaf_lookup chose
template <int NW>
__device__ __forceinline__ void cache_store(const MctsDev &d, const GameState *st, const int g, const float *policy,
                                            const float v) {
    const PosTable t = cache_of<NW>(d, g);
    const size_t slot = (size_t)rfl(st->leaf_ec_slot);
    const int lane = lane_id(), A = d.geo.A;
#pragma unroll
    for (int j = 0; j < NW; j++) {
        const int cell = j * 64 + lane;
        if (cell < A) t.pol[slot * A + cell] = policy[(size_t)g * A + cell];
    }
    if (lane == 0) {
        const uint64_t *board = st->leaf.board;
#pragma unroll
        for (int i = 0; i < 2 * NW; i++) t.key[slot * 2 * NW + i] = board[i];
        t.val[slot] = v;
        t.meta[slot] = (st->ec_epoch << 8) | (uint32_t)(pos_stones<NW>(bb_load<NW>(board), bb_load<NW>(board + NW)) & 0xFF);
    }
}

// The same fresh evaluation goes into the shared table: lane 0 claims the first slot of the probe window that nobody has ever
// used (the one atomic of the option, as in k_book_insert), stamped with this launch's stamp so that no lookup of this launch
// trusts it; key, value and row follow as plain stores, published by the end of the launch.  Insert-only: a claimed slot is
// never written again, a full window drops the row.  Two games that insert one position in one launch take two slots.
// Replacing mode (d.sh_claim) differs in the claim alone: see there.
template <int NW>
__device__ __forceinline__ void shared_store(const MctsDev &d, GameState *st, const int g, const float *policy, const float v,
                                             const uint32_t stamp) {
    const int lane = lane_id(), A = d.geo.A;
    const uint64_t *board = st->leaf.board;
    int got = -1;
    if (lane == 0 && !d.sh_claim) {
        // a slot that a plain load already shows taken stays taken (insert-only), so it costs no atomic: once the table is full
        // a dropped row is eight loads.  A stale 0 is settled by the atomicCAS that follows
        got = tt_probe(bb_hash<NW>(board, board + NW), d.sh.mask, [&](uint32_t at) {
            if (d.sh.meta[at] != 0u) return TT_NEXT;
            return atomicCAS(&d.sh.meta[at], 0u, stamp) == 0u ? TT_HIT : TT_NEXT;
        });
        st->ctr[got >= 0 ? TC_SH_INSERTS : TC_SH_DROPPED] += 1;
    } else if (lane == 0) {
        // Replacing mode: ONE inserter per position and launch.  The claim word carries this launch's stamp and the half of the
        // hash that indexing does not use, taken in ONE 64-bit atomicCAS on the value observed (0 or a tombstone: both free), so
        // a slot is never claimed without its tag.  An inserter that meets its own (stamp, tag) -- by the plain load or as the
        // value its failed CAS returns -- stops: the position is being inserted by another game of this launch.  Exactly one of
        // the games that insert position P in a launch takes a slot (if the window has room): within a launch a slot only goes
        // from free to taken (the sweep is a launch of its own), and all of them walk the same window in the same order.  Had
        // two of them taken slots a before b, the second would have passed a, which it does only when a shows a claim that is
        // not P's in this launch -- a taken slot that P's first inserter could then never have claimed.  A stale load can only
        // show an older state (free), which the CAS settles.  Two positions with one tag in one window and one launch: the
        // second stops as a duplicate and its row is not stored -- one insert lost, nothing else, since lookups compare keys
        const uint64_t h = bb_hash<NW>(board, board + NW);
        const unsigned long long mine = SH_CLAIM((uint32_t)(h >> 32), stamp);
        bool dup = false;
        got = tt_probe(h, d.sh.mask, [&](uint32_t at) {
            unsigned long long seen = d.sh_claim[at];
            if (sh_free(sh_stamp_of(seen))) {
                const unsigned long long old = atomicCAS(&d.sh_claim[at], seen, mine);
                if (old == seen) return TT_HIT;
                seen = old;
            }
            if (seen == mine) { dup = true; return TT_MISS; }
            return TT_NEXT;
        });
        st->ctr[got >= 0 ? TC_SH_INSERTS : dup ? TC_SH_DUPLICATES : TC_SH_DROPPED] += 1;
        if (got >= 0) d.sh_hit[got] = stamp;         // no lookup of this launch reads or marks a slot claimed in it
    }
    got = rfl(got);
    if (got < 0) return;
    const size_t slot = (size_t)got;
#pragma unroll
    for (int j = 0; j < NW; j++) {
        const int cell = j * 64 + lane;
        if (cell < A) d.sh.pol[slot * A + cell] = policy[(size_t)g * A + cell];
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 2 * NW; i++) d.sh.key[slot * 2 * NW + i] = board[i];
        d.sh.val[slot] = v;
    }
}

// ---- building blocks shared by the K = 1 and the K > 1 tree kernel: each float32 / float64 sequence of the parity contract
// with the reference exists once, here.
#define BEST_NONE 0x7FFFFFFF

// child_key, the order-preserving key of one child's PUCT score (mcts.py:120-133), lives in yy_tree.h: the root distribution
// prunes forced playouts with it.  K = 1 passes the edge's N and W, K > 1 the counts with this step's virtual visits
// (do_select_multi).

// First-play urgency (YY_FLAG_FPU_REDUCTION, include/yy_engine.h): the q an unvisited child of a node is scored with.  Every
// lane adds its own children (the counts and W that child_key is given: with the virtual visits at K > 1) to a FpuPart; the
// sums are integers -- W in units of 2^-32, truncated toward zero, P in units of 2^-40 -- so that they do not depend on which
// lane holds which child.  fpu_value reduces them over the wave, and only when some child is unvisited and some is visited.
struct FpuPart {
    uint32_t n = 0;      // sum of N over the children with N > 0
    int64_t w = 0;       // sum of (int64)(f64(W) * 2^32) over them
    uint64_t p = 0;      // sum of (uint64)(f64(P) * 2^40) over them
    bool unvisited = false;
    __device__ __forceinline__ void add(const float P, const int N, const float W) {
        if (N > 0) {
            n += (uint32_t)N;
            w += (int64_t)__dmul_rn((double)W, 4294967296.0);
            p += (uint64_t)__dmul_rn((double)P, 1099511627776.0);
        } else {
            unvisited = true;
        }
    }
};
// q_fpu = f32( f32(SW / SN) - f32(r * f32(sqrt(SP))) ); 0 when no child is visited (or none is unvisited: nobody reads it)
__device__ __forceinline__ float fpu_value(const FpuPart &a, const float r) {
    if (!__ballot(a.unvisited)) return 0.0f;
    const uint32_t SN = wave_uadd(a.n);
    if (SN == 0u) return 0.0f;
    const int64_t sw = (int64_t)wave_uadd64((uint64_t)a.w);
    const uint64_t sp = wave_uadd64(a.p);
    const float SW = (float)__dmul_rn((double)sw, 0x1p-32);
    const float SP = (float)__dmul_rn((double)sp, 0x1p-40);
    return __fsub_rn(__fdiv_rn(SW, (float)SN), __fmul_rn(r, __fsqrt_rn(SP)));
}

// Wave arg-max over the k children of a node: every lane brings the best key `bk` of its own children and that child's index
// `bi` (BEST_NONE: none).  Returns the child with the largest key, the lowest index among ties = the lowest action
// (mcts.py:133), or BEST_NONE when no child is selectable (every key 0: NaN scores).
__device__ __forceinline__ int best_child(uint32_t bk, int bi, int k) {
    const uint32_t mx = wave_umax(bk);
    const bool tied = (bk == mx) && (bi != BEST_NONE);
    int best;
    if (k <= 64) {   // lane == child index: the lowest tied lane
        const uint64_t tm = __ballot(tied);
        best = tm ? (int)__ffsll((unsigned long long)tm) - 1 : BEST_NONE;
    } else {
        const uint32_t mi = wave_umin(tied ? (uint32_t)bi : 0xFFFFFFFFu);
        best = (mi == 0xFFFFFFFFu) ? BEST_NONE : (int)mi;
    }
    if (mx == 0u) best = BEST_NONE;
    return best;
}

// The position a descent ended on, and its side to move (the return value).  A pass root is evaluated on its own board
// (mcts.py:371-381); every other leaf on its parent's board after getNextState (mcts.py:385-391): place iff legal
// (yin_yang_game.py:52-58).  With copied boards the action is one of the parent's legal moves on this very board, so it
// always places and is placed here.  The aliased board has moved on since: do_select tests legality and places it.
template <int NW>
__device__ __forceinline__ int leaf_position(const MctsDev &d, const GameState *st, const int g, const uint4 *nodes,
                                             const int kind, const int parent, const int action, const bool aliased,
                                             BB<NW> &black, BB<NW> &white) {
    const uint64_t *src = aliased ? d.gboard + (size_t)g * 2 * NW
                                  : d.nboard + ((size_t)g * d.node_cap + (kind == K_ROOTPASS ? 0 : parent)) * 2 * NW;
    black = bb_uniform_load<NW>(src);
    white = bb_uniform_load<NW>(src + NW);
    if (kind == K_ROOTPASS) return rfl((int)st->root_player);
    const int pplayer = node_player(rfl(nodes[parent].y));
    if (!aliased) {
        if (pplayer == 1) black = black | bb_bit<NW>(action);
        else white = white | bb_bit<NW>(action);
    }
    return -pplayer;
}

// Node.expand (mcts.py:50-91) of the evaluated leaf `rec`: v is its value, prow its policy row (the evaluator's row, a cache
// row or a book row), path the edges that led to it.  A K_EXPAND leaf gets its node here; every other kind has one.
// `hold`: a node without children keeps v for YY_FLAG_REUSE_PASS_VALUE.  Returns false on a NaN value, a full node or edge
// arena or a NaN prior: the caller marks the game failed, it stops searching, and what was written up to there is never read.
template <int NW>
__device__ __forceinline__ bool expand_leaf(const MctsDev &d, GameState *st, const int g, const LeafRec *rec,
                                            const int32_t *path, const float *prow, const float v, const bool hold,
                                            const bool aliased, const double *noise, const double eps) {
    if (v != v) return false;   // a NaN from the evaluator must not enter the statistics
    const int lane = lane_id();
    const int A = d.geo.A;
    uint4 *nodes = d.nodes + (size_t)g * d.node_cap;
    uint4 *edges = d.edges + (size_t)g * d.edge_cap;
    const int lplayer = rfl((int)rec->player);
    const bool term = rfl((int)rec->terminal) != 0;
    int node = rfl(rec->node);
    int n_nodes = rfl(st->n_nodes), n_edges = rfl(st->n_edges);
    if (rfl((int)rec->kind) == K_EXPAND) {
        if (n_nodes >= (int)d.node_cap) return false;
        node = n_nodes++;
        if (lane == 0) {
            uint4 *pe = edges + path[rfl(rec->path_len) - 1];
            pe->w = (pe->w & 0xFF000000u) | (uint32_t)node;
            st->ctr[TC_NODES] += 1;
        }
    }
    BB<NW> mask;
#pragma unroll
    for (int i = 0; i < NW; i++) mask.w[i] = rfl64(rec->mask[i]);
    if (!aliased) {
        uint64_t *nb = d.nboard + ((size_t)g * d.node_cap + node) * 2 * NW;
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 2 * NW; i++) nb[i] = rec->board[i];
        }
    }
    if (term) {                                                                 // mcts.py:63-68
        if (lane == 0)
            nodes[node] = make_uint4(0u, node_pack(0, NF_TERMINAL, lplayer), __float_as_uint(rec->tv), __float_as_uint(v));
    } else {                                                                    // mcts.py:71-89
        const int k = bb_popc(mask);
        if (n_edges + k > (int)d.edge_cap) return false;
        const float keep = (float)(1.0 - eps);
        // a game whose noise row is all zero over its legal moves drew no noise (a Dirichlet draw
        // sums to 1): it keeps the raw priors, like add_exploration_noise=False (mcts.py:298)
        bool mix = false;
        if (noise) {
            uint64_t any = 0;
#pragma unroll
            for (int j = 0; j < NW; j++) {
                const int cell = j * 64 + lane;
                const bool nz = ((mask.w[j] >> lane) & 1) && noise[(size_t)g * A + cell] != 0.0;
                any |= __ballot(nz);
            }
            mix = any != 0;
        }
        int base = n_edges;
        bool bad = false;   // a NaN prior (python: `score > best` is never true for it, select_child returns None and the game raises)
        // symmetry-randomised evaluation: prow (the evaluator's, a cache's or the book's row) is in the frame of the position
        // under its drawn symmetry, where action `cell` sits at sym_cell(s, cell); everything below stays in the original frame
        int s = 0;
        if (d.sym) {                                                            // wave-uniform
            BB<NW> lb, lw;
#pragma unroll
            for (int i = 0; i < NW; i++) {
                lb.w[i] = rfl64(rec->board[i]);
                lw.w[i] = rfl64(rec->board[NW + i]);
            }
            s = sym_of<NW>(d.geo, d.sym_seed, lb, lw);
        }
#pragma unroll
        for (int j = 0; j < NW; j++) {
            const int cell = j * 64 + lane;
            if ((mask.w[j] >> lane) & 1) {
                float p = prow[d.sym ? sym_cell(d.geo, s, cell) : cell];
                bad |= (p != p);
                if (mix) {                                                      // mcts.py:310-312
                    const float kp = __fmul_rn(keep, p);
                    p = (float)__dadd_rn((double)kp, __dmul_rn(eps, noise[(size_t)g * A + cell]));
                }
                edges[base + mbcnt(mask.w[j])] =
                    make_uint4(__float_as_uint(p), 0u, 0u, CHILD_NONE | ((uint32_t)cell << 24));
            }
            base += yy_popc64(mask.w[j]);
        }
        if (__ballot(bad)) return false;
        if (lane == 0) {
            nodes[node] = make_uint4((uint32_t)n_edges, node_pack(k, (hold && k == 0) ? NF_HASVALUE : 0u, lplayer), 0u,
                                     __float_as_uint(v));                       // .w = the evaluator's value of this position
            st->ctr[TC_CREATED] += (uint64_t)k;
        }
        n_edges += k;
    }
    if (lane == 0) {
        st->n_nodes = n_nodes;
        st->n_edges = n_edges;
    }
    return true;
}

// Backup (mcts.py:147-156, 406-412) of v along the `depth` edges of `path`: edge i leads to the node at depth i+1 and the
// leaf is at `depth`; players alternate every ply, so the sign is the parity of the distance to the leaf.  v_is_py: v is a
// python number (a terminal value), not an np.float32.
__device__ __forceinline__ void backup_path(uint4 *edges, const int32_t *path, const int depth, const float v,
                                            const bool v_is_py, GameState *st) {
    const int lane = lane_id();
    for (int i = lane; i < depth; i += 64) {
        uint4 *e = edges + path[i];
        const int dist = depth - (i + 1);
        const float sv = (dist & 1) ? -v : v;
        uint4 r = *e;
        r.y = (uint32_t)((int)r.y + 1);
        r.z = __float_as_uint(__fadd_rn(__uint_as_float(r.z), sv));
        *e = r;
    }
    if (lane == 0) {
        const float sv = (depth & 1) ? -v : v;
        st->root_N += 1;
        if (st->root_w_is_py && v_is_py && depth == 0) {
            // terminal root: python float + python number stays a python float (f64)
            st->root_W_py += (double)((sv == 0.0001f) ? 0.0001 : (sv == -0.0001f ? -0.0001 : (double)sv));
        } else {
            const float base = st->root_w_is_py ? (float)st->root_W_py : st->root_W;
            st->root_W = __fadd_rn(base, sv);
            st->root_w_is_py = 0;
        }
    }
}

// ---- root prologue: mcts.py:288-295 (root_setup, yy_tree.h)
// The simulation budget of game g: K > 1 keeps it in mst[2g], K = 1 in GameState.budget.  `budgets` (int32 [G], clamped to
// 0 .. max_sims here) when the caller set one (yy_mcts_set_sim_budgets), else `target` for every game.  The pointer is an
// argument of this kernel only: the step kernels read the stored budgets, so a captured step serves every budget array.
template <int NW> __global__ void __launch_bounds__(64) k_begin(MctsDev d, MultiDev m, int target, int kept_target,
                                                                const int32_t *budgets, int max_sims, const int8_t *boards,
                                                                const int8_t *players, const uint8_t *active,
                                                                float *planes) {
    const int g = blockIdx.x;
    const int K = m.K;          // K > 1: the root row is row g*K, the pending root expansion is leaf record g*K
    GameState *st = d.state + g;
    LeafRec *rec = K > 1 ? m.leaves + (size_t)g * K : &st->leaf;
    const bool act = active ? (active[g] != 0) : true;
    BB<NW> black, white;
    board_to_bb<NW>(boards + (size_t)g * d.geo.A, d.geo.A, black, white);
    // Tree reuse: yy_mcts_advance left the subtree of the move played at node 0.  The mark is consumed here whatever follows, so
    // that no tree is used twice; the tree is kept only for the position it was built for (board, side to move) of an active
    // game -- a caller that advanced by one move and searches another position gets the fresh root of every search.
    bool keep = false;
    if (rfl((int)st->kept)) {
        const uint64_t *nb = d.nboard + (size_t)g * d.node_cap * 2 * NW;
        const BB<NW> kb = bb_uniform_load<NW>(nb), kw = bb_uniform_load<NW>(nb + NW);
        bool same = act && rfl((int)players[g]) == rfl((int)st->root_player);
#pragma unroll
        for (int i = 0; i < NW; i++) same = same && kb.w[i] == black.w[i] && kw.w[i] == white.w[i];
        keep = same;
    }
    if (keep) {
        // the arena, root_N, root_W and root_player stay as yy_mcts_advance left them; the search tops the root up to the budget.
        // K = 1 stores no scalar budget for a fresh root (the host issues exactly that many steps); a kept root needs it
        if (lane_id() == 0) {
            st->kept = 0;
            st->root_kept = 1;
            st->active = 1;
            st->err = 0;
            st->budget = budgets ? min(max(budgets[g], 0), max_sims) : kept_target;
            rec->kind = K_ROOTKEPT;
            rec->node = 0;
            rec->path_len = 0;
            rec->dup = -1;
        }
    }
    root_setup<NW>(d, st, rec, g, black, white, rfl((int)players[g]), act, keep,
                   budgets ? min(max(budgets[g], 0), max_sims) : target, planes + (size_t)g * K * 5 * d.geo.A);
    if (K > 1 && lane_id() == 0) {
        m.mst[2 * g] = budgets ? min(max(budgets[g], 0), max_sims) : target;
        m.mst[2 * g + 1] = act ? 1 : 0;
    }
}

// ---- selection: mcts.py:356-362 (descent), 385-391 (state of the leaf), 63-71 (its rules)
template <int NW>
__device__ __forceinline__ void do_select(const MctsDev &d, const int g, float *planes, uint8_t *needs_eval,
                                          const uint32_t stamp) {
    GameState *st = d.state + g;
    const int lane = lane_id();
    // a game whose root has had its budget of simulations selects nothing, like an inactive one: no arena, no counter.  The
    // four fields are loaded before any of them is tested, so that they cost one round trip to memory, not one each
    const int s_active = st->active, s_err = st->err, s_budget = st->budget;
    const int s_kept = st->root_kept;
    int s_carry = st->root_N;
    s_carry = rfl(s_carry);
    if ((rfl(s_active) == 0) | (rfl(s_err) != 0) | (s_carry >= rfl(s_budget))) {
        if (lane == 0) {
            st->leaf.kind = K_NONE;
            if (needs_eval) needs_eval[g] = 0;
        }
        return;
    }
    s_carry -= rfl(s_kept);   // a kept root (tree reuse) was itself expanded by its first visit: its children hold root_N - 1
    const GeoBB<NW> gb = geo_bb<NW>(d.geo);
    const uint4 *nodes = d.nodes + (size_t)g * d.node_cap;
    uint4 *edges = d.edges + (size_t)g * d.edge_cap;
    int32_t *path = d.path + (size_t)g * d.path_cap;

    int node = 0, depth = 0, parent = -1, action = -1, kind;
    uint64_t c_levels = 0, c_scan = 0;
    int c_forced = 0;   // wave-uniform: this descent took a forced edge (stored with the counters below)
    for (;;) {
        const uint4 hdr = nodes[node];
        const uint32_t hy = rfl(hdr.y);
        const int k = node_k(hy), first = rfl((int)hdr.x);
        // solver: a proven flag is only ever set with YY_FLAG_SOLVER, so without it this is the terminal test it was.  A proven
        // node below the root ends the descent like a terminal one; the root is never treated as terminal
        if (node_flags(hy) & (NF_TERMINAL | NF_PROVEN_MASK)) {
            if (node_flags(hy) & NF_TERMINAL) { kind = K_TERMINAL; break; }        // mcts.py:360, 365
            if (node != 0) { kind = K_PROVEN; break; }
        }
        if (k == 0) {                                                              // mcts.py:93-95
            // A node without children is evaluated again on every visit.  With copied boards its board never changes,
            // so that evaluation returns the value it returned the first time: YY_FLAG_REUSE_PASS_VALUE takes it from
            // the node record instead of spending an evaluator row on it (same statistics, fewer rows).
            kind = (d.reuse && (node_flags(hy) & NF_HASVALUE)) ? K_REUSE : (node == 0) ? K_ROOTPASS : K_REEXPAND;
            break;
        }
        if (depth >= (int)d.path_cap) { kind = K_NONE; if (lane == 0) fail_game(st); break; }
        // ---- Node.select_child (mcts.py:97-145)
        // sum of child visits (mcts.py:112).  Copied boards: every visit of an expanded node after its
        // first descends into exactly one child, so the sum is N(node)-1 (root: completed simulations) and
        // is carried down the descent; aliased boards can give a pass node children later, so sum there.
        // solver: only the root is descended from while proven (a kept root, or one proven in this search), and the visits
        // that ended ON it while it was a proven node below a root went into no child: sum there as well.
        int S;
        if (d.aliased | (node_flags(hy) & NF_PROVEN_MASK)) {
            uint32_t part = 0;
            for (int j = lane; j < k; j += 64) part += edges[first + j].y;
            S = (int)wave_uadd(part);
        } else {
            S = s_carry;
        }
        // forced playouts: at the root a visited edge that is still owed visits (edge_forced, yy_tree.h) is taken before any
        // score is looked at, the lowest action first.  Wave-uniform branch; below the root only `depth == 0` is tested, at the
        // root without the option one float64 compare more
        int best = BEST_NONE;
        if (depth == 0 && d.forced > 0.0) {
            for (int j0 = 0; j0 < k && best == BEST_NONE; j0 += 64) {
                const int j = j0 + lane;
                bool f = false;
                if (j < k) {
                    const uint4 e = edges[first + j];
                    f = edge_forced(d.forced, __uint_as_float(e.x), (int)e.y, S);
                }
                const uint64_t fm = __ballot(f);
                if (fm) best = j0 + (int)__ffsll((unsigned long long)fm) - 1;
            }
            c_forced += (best != BEST_NONE);
        }
        uint32_t w;
        if (best != BEST_NONE) {
            const uint4 e = edges[first + best];
            w = rfl(e.w);
            s_carry = (int)rfl(e.y) - 1;
        } else if (depth == 0 && d.gumbel) {
            // Gumbel root search: sequential halving as a pure function of the root's edges and S (include/yy_engine.h).  The
            // child to visit is, among those with N == seq(min(m, k), budget)[S] (all when there is none), the one of the
            // largest g + log P + sigma(q), the lowest edge on ties.  Wave-uniform branch, like the forced-playouts one
            uint32_t mxn = 0;
            for (int j = lane; j < k; j += 64) mxn = umax32(mxn, edges[first + j].y);
            const int maxN = (int)wave_umax(mxn);
            const int v = gumbel_seq_at(min((int)d.gumbel, k), rfl(s_budget), S);
            const float *s0 = d.g_s0 + (size_t)g * d.geo.A;
            uint32_t ck = 0, cw = 0, cn = 0, ak = 0, aw = 0, an = 0;              // best of the considered children / of all
            int ci = BEST_NONE, ai = BEST_NONE;
            for (int j = lane; j < k; j += 64) {
                const uint4 e = edges[first + j];
                const uint32_t key = gumbel_key(d, s0[j], maxN, (int)e.y, __uint_as_float(e.z));
                if (key > ak) { ak = key; ai = j; aw = e.w; an = e.y; }
                if ((int)e.y == v && key > ck) { ck = key; ci = j; cw = e.w; cn = e.y; }
            }
            const bool considered = __ballot(ci != BEST_NONE) != 0;
            const uint32_t bw = considered ? cw : aw, bn = considered ? cn : an;
            best = best_child(considered ? ck : ak, considered ? ci : ai, k);
            if (best == BEST_NONE) { kind = K_NONE; if (lane == 0) fail_game(st); break; }  // every score NaN
            w = (uint32_t)__builtin_amdgcn_readlane((int)bw, best & 63);
            s_carry = (int)__builtin_amdgcn_readlane((int)bn, best & 63) - 1;
        } else if (d.g_interior) {
            // Gumbel search below the root (YY_FLAG_GUMBEL_INTERIOR, include/yy_engine.h): the child of the largest
            // pi'(a) - N(a) / (1 + S), the lowest edge on ties; PUCT and first-play urgency are not consulted.  Wave-uniform
            // branch on the flag word, like the two above; the node's edges are held in registers for the two passes
            uint4 e[NW];
#pragma unroll
            for (int i = 0; i < NW; i++) e[i] = (i * 64 + lane < k) ? edges[first + i * 64 + lane] : make_uint4(0u, 0u, 0u, 0u);
            uint64_t t[NW];
            const GumbelNode gn = gumbel_improved<NW>(d, e, k, rflf(__uint_as_float(hdr.w)), t);
            const double zf = (double)gn.Z, s1 = (double)(1 + gn.S);
            uint64_t bk = 0;
            uint32_t bw = 0, bn = 0;
            int bi = BEST_NONE;
#pragma unroll
            for (int i = 0; i < NW; i++) {
                if (i * 64 + lane < k && t[i] != GI_NAN) {
                    const uint64_t key = f64_key(__dadd_rn(__ddiv_rn((double)t[i], zf), -__ddiv_rn((double)(int)e[i].y, s1)));
                    if (key > bk) { bk = key; bi = i * 64 + lane; bw = e[i].w; bn = e[i].y; }   // strict >: lowest edge of a lane
                }
            }
            const uint64_t mxk = wave_max_u64(bk);
            const uint32_t mi = wave_umin((bk == mxk && bi != BEST_NONE) ? (uint32_t)bi : 0xFFFFFFFFu);
            if (mxk == 0ull || mi == 0xFFFFFFFFu) { kind = K_NONE; if (lane == 0) fail_game(st); break; }   // every score NaN
            best = (int)mi;
            w = (uint32_t)__builtin_amdgcn_readlane((int)bw, best & 63);
            s_carry = (int)__builtin_amdgcn_readlane((int)bn, best & 63) - 1;
        } else {
            const float sq = d.sqrt_tab[min(S, d.sqrt_n - 1)];   // f32(math.sqrt(sum_visits))
            // first-play urgency: one more pass over the node's edges for the sums behind the q of its unvisited children
            // (copied and aliased boards alike).  Wave-uniform branch; without the option q0 stays the reference's 0
            float q0 = 0.0f;
            if (d.fpu > 0.0f) {
                FpuPart fp;
                for (int j = lane; j < k; j += 64) {
                    const uint4 e = edges[first + j];
                    fp.add(__uint_as_float(e.x), (int)e.y, __uint_as_float(e.z));
                }
                q0 = fpu_value(fp, depth == 0 ? d.fpu_root : d.fpu);
            }
            uint32_t bk = 0, bw = 0, bn = 0;
            int bi = BEST_NONE;
            for (int j = lane; j < k; j += 64) {
                const uint4 e = edges[first + j];
                const uint32_t key = child_key(d.cpuct, sq, __uint_as_float(e.x), (int)e.y, __uint_as_float(e.z), q0);
                if (key > bk) { bk = key; bi = j; bw = e.w; bn = e.y; }               // strict >: lowest j of a lane
            }
            best = best_child(bk, bi, k);
            if (best == BEST_NONE) { kind = K_NONE; if (lane == 0) fail_game(st); break; }  // no selectable child
            w = (uint32_t)__builtin_amdgcn_readlane((int)bw, best & 63);
            s_carry = (int)__builtin_amdgcn_readlane((int)bn, best & 63) - 1;
        }
        if (lane == 0) path[depth] = first + best;
        depth++;
        c_levels++;
        c_scan += (uint64_t)k;
        parent = node;
        action = (int)(w >> 24);
        const uint32_t child = w & CHILD_NONE;
        if (child == CHILD_NONE) { kind = K_EXPAND; node = -1; break; }
        node = (int)child;
    }

    bool need = false;
    if (kind == K_EXPAND || kind == K_REEXPAND || kind == K_ROOTPASS) {
        BB<NW> black, white;
        const int lplayer = leaf_position<NW>(d, st, g, nodes, kind, parent, action, d.aliased != 0u, black, white);
        if (d.aliased && kind != K_ROOTPASS) {   // the shared board: the full legality test, then the stone goes onto it
            const int pplayer = -lplayer;
            bool pre = bb_pre2x2(black, white, gb);
            BB<NW> m = (pplayer == 1) ? bb_legal(black, white, pre, d.geo, gb) : bb_legal(white, black, pre, d.geo, gb);
            if (bb_test(m, action)) {
                if (pplayer == 1) black = black | bb_bit<NW>(action);
                else white = white | bb_bit<NW>(action);
                uint64_t *dst = d.gboard + (size_t)g * 2 * NW;
                bb_store_lane0<NW>(dst, black);
                bb_store_lane0<NW>(dst + NW, white);
            }
        }
        BB<NW> mask;
        bool term;
        float tv;
        leaf_rules<NW>(d.geo, gb, black, white, lplayer, mask, term, tv);
        int slot;
        const int src = leaf_lookup<NW>(d, st, g, black, white, slot, stamp);
        if (src == SRC_NONE) write_eval_planes<NW>(planes + (size_t)g * 5 * d.geo.A, d.geo, d.sym, d.sym_seed, black, white);
        leaf_store<NW>(&st->leaf, black, white, mask, lplayer, term, tv);
        if (lane == 0) {
            st->leaf_src = src;
            st->leaf_ec_slot = slot;
        }
        need = src == SRC_NONE;
        if (!need && lane == 0) {
            st->ctr[TC_TABLE_HITS] += 1;
            if (src >= SRC_SHARED) st->ctr[TC_SH_HITS] += 1;
        }
    }
    if (lane == 0) {
        st->leaf.kind = (uint8_t)kind;
        st->leaf.node = node;
        st->leaf.path_len = depth;
        st->ctr[TC_LEVELS] += c_levels;
        st->ctr[TC_SCANNED] += c_scan;
        if (need) st->ctr[TC_EVALS] += 1;
        if (kind == K_TERMINAL) st->ctr[TC_TERMINAL] += 1;
        if (kind == K_REUSE) st->ctr[TC_REUSED] += 1;
        if (kind == K_PROVEN) st->ctr[TC_SV_DESCENTS] += 1;
        if (c_forced) st->ctr[TC_FORCED] += 1;
        if (needs_eval) needs_eval[g] = need;
    }
}

// Root noise on a kept root (tree reuse): the root's edges exist, so the draw is mixed into their STORED priors with the very
// sequence expand_leaf uses on a fresh root (mcts.py:310-312); a row that is zero over the root's moves drew nothing.  Only a
// root is ever noised and yy_mcts_advance drops it, so the priors below a root are always the raw ones.
__device__ __forceinline__ void noise_kept_root(const MctsDev &d, const int g, const uint4 *nodes, uint4 *edges,
                                                const double *noise, const double eps) {
    const int lane = lane_id();
    const uint4 hdr = nodes[0];
    const int k = node_k(rfl(hdr.y)), first = rfl((int)hdr.x);
    const double *nrow = noise + (size_t)g * d.geo.A;
    uint64_t any = 0;
    for (int j0 = 0; j0 < k; j0 += 64) {
        const int j = j0 + lane;
        any |= __ballot(j < k && nrow[edges[first + j].w >> 24] != 0.0);
    }
    if (!any) return;
    const float keep = (float)(1.0 - eps);
    for (int j = lane; j < k; j += 64) {
        uint4 *e = edges + first + j;
        const float kp = __fmul_rn(keep, __uint_as_float(e->x));
        e->x = __float_as_uint((float)__dadd_rn((double)kp, __dmul_rn(eps, nrow[e->w >> 24])));
    }
}

// ---- solver (YY_FLAG_SOLVER; Winands et al. 2008, "Monte-Carlo Tree Search Solver"): after the backup of a descent of `depth`
// edges that ended on a terminal or proven node, the path is walked upwards from the leaf's parent.  A node with k > 0 children
// is a WIN for its side to move if any child that exists is a LOSS for the child's; else, if all k children exist and all are
// proven, a DRAW if any is one, else a LOSS.  The walk stops at the first node whose status does not change (a status never
// changes once set, so that is a node that stays open or one that is proven already); the root may become proven.  A node
// without children (a pass) is never proven, and the statistics of a proven node are not rewritten.  Wave-uniform: per level one
// pass over the node's edges and the headers of its children.
__device__ __forceinline__ void solver_propagate(GameState *st, uint4 *nodes, const uint4 *edges, const int32_t *path,
                                                 const int depth) {
    const int lane = lane_id();
    int c_proven = 0, c_root = 0;
    for (int lvl = depth - 1; lvl >= 0; lvl--) {
        __syncthreads();   // lane 0 wrote the leaf's record and its parent's edge (expand_leaf), and the level below
        const int n = (lvl == 0) ? 0 : (int)(rfl(edges[path[lvl - 1]].w) & CHILD_NONE);
        const uint4 hdr = nodes[n];
        const uint32_t hy = rfl(hdr.y);
        const int k = node_k(hy), first = rfl((int)hdr.x);
        if ((node_flags(hy) & (NF_TERMINAL | NF_PROVEN_MASK)) || k == 0) break;
        uint64_t loss = 0, draw = 0, open = 0;
        for (int j0 = 0; j0 < k; j0 += 64) {
            const int j = j0 + lane;
            int s = -1;                                                             // no such child
            if (j < k) {
                const uint32_t c = edges[first + j].w & CHILD_NONE;
                s = (c == CHILD_NONE) ? (int)PV_NONE : node_proven(nodes[c]);
            }
            loss |= __ballot(s == PV_LOSS);
            draw |= __ballot(s == PV_DRAW);
            open |= __ballot(s == PV_NONE);
        }
        const int s = loss ? PV_WIN : open ? PV_NONE : draw ? PV_DRAW : PV_LOSS;
        if (s == PV_NONE) break;
        if (lane == 0)
            nodes[n] = make_uint4(hdr.x, hdr.y | ((uint32_t)s << (16 + NF_PROVEN_SHIFT)), __float_as_uint(proven_value(s)), hdr.w);
        c_proven += 1;
        c_root += (n == 0);
    }
    if (lane == 0 && c_proven) {
        st->ctr[TC_SV_NODES] += (uint64_t)c_proven;
        st->ctr[TC_SV_ROOTS] += (uint64_t)c_root;
    }
}

// ---- expansion + backup: mcts.py:50-91 (expand_leaf), 147-156 + 406-412 (backup_path)
template <int NW>
__device__ __forceinline__ void do_expand_backup(const MctsDev &d, const int g, const float *policy,
                                                 const float *value, const double *noise, const double eps,
                                                 const uint32_t stamp) {
    GameState *st = d.state + g;
    const int lane = lane_id();
    const int kind = rfl((int)st->leaf.kind);
    if (kind == K_NONE) return;
    const uint4 *nodes = d.nodes + (size_t)g * d.node_cap;
    uint4 *edges = d.edges + (size_t)g * d.edge_cap;
    if (kind == K_ROOTKEPT) {   // yy_mcts_expand_root on a kept root: already expanded, the policy row is not read
        if (noise) noise_kept_root(d, g, nodes, edges, noise, eps);
        if (lane == 0) st->leaf.kind = K_NONE;
        return;
    }
    const int32_t *path = d.path + (size_t)g * d.path_cap;
    const int depth = rfl(st->leaf.path_len);
    const int node = rfl(st->leaf.node);
    float v;
    bool v_is_py = false;   // value is a python number (terminal value), not np.float32
    bool exact = false;     // solver: the descent ended on a terminal or proven node
    if (kind == K_TERMINAL || kind == K_PROVEN) {
        v = rflf(__uint_as_float(nodes[node].z));                                   // mcts.py:366; a proven node's exact value
        v_is_py = true;
        exact = true;
    } else if (kind == K_REUSE) {
        v = rflf(__uint_as_float(nodes[node].w));                                   // the np.float32 the evaluator returned for this node
    } else {
        // the root call of mcts.py:288 looks nothing up, and its value is discarded: yy_mcts_expand_root is not given it
        const bool root = kind == K_ROOTINIT;
        const int src = (root || !(d.ec.meta || d.bk.meta || d.sh.meta)) ? SRC_NONE : rfl(st->leaf_src);
        // YY_FLAG_GUMBEL_INTERIOR: the root keeps the evaluator's value of its position in its record, like every other expansion
        const LeafEval ev = leaf_eval<NW>(d, g, src, policy, (root && !d.g_interior) ? nullptr : value);
        v = ev.v;
        const bool hold = d.reuse && !root;   // a pass node keeps its value; a pass root that of its first simulation
        if (!expand_leaf<NW>(d, st, g, &st->leaf, path, ev.prow, v, hold, d.aliased != 0u, root ? noise : nullptr, eps)) {
            // NaN from the evaluator or a full arena: the game stops searching, the error is sticky
            if (lane == 0) { fail_game(st); st->leaf.kind = K_NONE; }
            return;
        }
        if (d.ec.meta && src == SRC_NONE && !root) cache_store<NW>(d, st, g, policy, v);
        if (d.sh.meta && src == SRC_NONE && !root) shared_store<NW>(d, st, g, policy, v, stamp);
        exact = d.solver && kind == K_EXPAND && rfl((int)st->leaf.terminal) != 0;   // the new node is a terminal one
        if (root && d.gumbel) {                                                     // wave-uniform
            // Gumbel root search: the base score of every root edge, from its STORED prior (the noised one at a noised root)
            __syncthreads();                                                        // the edges other lanes wrote in expand_leaf
            const uint4 hdr = nodes[0];
            const int k = node_k(rfl(hdr.y)), first = rfl((int)hdr.x);
            const float *grow = d.g_rows + (size_t)g * d.geo.A;
            float *s0 = d.g_s0 + (size_t)g * d.geo.A;
            for (int j = lane; j < k; j += 64) {
                const uint4 e = edges[first + j];
                s0[j] = (float)__dadd_rn((double)grow[e.w >> 24], log((double)__uint_as_float(e.x)));
            }
        }
    }
    if (lane == 0) st->leaf.kind = K_NONE;
    if (kind == K_ROOTINIT) return;                                                 // no backup
    backup_path(edges, path, depth, v, v_is_py, st);
    if (d.solver && exact) solver_propagate(st, d.nodes + (size_t)g * d.node_cap, edges, path, depth);   // wave-uniform
}

template <int NW> __global__ void __launch_bounds__(64) k_mcts(MctsDev d, int do_backup, int do_sel,
                                                               const float *policy, const float *value,
                                                               const double *noise, double eps, float *planes,
                                                               uint8_t *needs_eval) {
    const int g = blockIdx.x;
    // the step stamp of this launch, read once per wave: k_stamp advanced it in front of this launch (launch_mcts)
    const uint32_t stamp = d.sh.meta ? rfl(*d.sh_stamp) : 0u;
    if (do_backup) do_expand_backup<NW>(d, g, policy, value, noise, eps, stamp);
    if (do_backup && do_sel) __syncthreads();   // edges/nodes written above are re-read below by other lanes
    if (do_sel) do_select<NW>(d, g, planes, needs_eval, stamp);
}

// The step stamp of the shared evaluation table: one thread, in a launch of its own between two tree-step launches of the
// context's stream, so that every tree-step launch has a stamp of its own.  Never 0 (0 marks a slot nobody has used).  The
// stamp lives in device memory: a captured step freezes its arguments.
// SH_TOMBSTONE (an evicted slot of the replacing table) is skipped like 0.
__global__ void k_stamp(uint32_t *stamp) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    *stamp = sh_next_stamp(*stamp);
}

// =============================================================================== leaf-parallel steps (K > 1)
// Every step runs K_eff = min(K, simulations of the search not yet started) descents per game, one after another, on the tree
// as it stands at the start of the step.  Descent j sees on every edge a virtual count v = the number of descents 0 .. j-1 of
// this step that walked it, and scores a child with n = N + v and w = v > 0 ? f32(W - f32(v)) : W, S = sum of the children's
// n (include/yy_engine.h).  Only the paths are stored: the descents that reached the current node by the same path
// are a bit mask `match` over the lanes, and lane i < j reads the edge descent i took out of it.  A descent ending on the leaf
// of an earlier one (same unexpanded edge, same childless node, the pass root) takes no row and shares that evaluation.
template <int NW>
__device__ __forceinline__ void do_select_multi(const MctsDev &d, const MultiDev &m, const int g, float *planes,
                                                uint8_t *needs_eval) {
    GameState *st = d.state + g;
    const int lane = lane_id();
    const int K = m.K;
    int32_t *ms = m.mst + 2 * g;
    int keff = 0;
    if (rfl((int)st->active) && !rfl((int)st->err)) keff = min(K, max(0, rfl(ms[0]) - rfl(st->root_N)));
    const GeoBB<NW> gb = geo_bb<NW>(d.geo);
    const uint4 *nodes = d.nodes + (size_t)g * d.node_cap;
    const uint4 *edges = d.edges + (size_t)g * d.edge_cap;
    uint64_t c_levels = 0, c_scan = 0, c_evals = 0, c_term = 0;
    bool failed = false;
    for (int j = 0; j < keff; j++) {
        int32_t *path = d.path + ((size_t)g * K + j) * d.path_cap;
        int node = 0, depth = 0, parent = -1, action = -1, kind;
        uint64_t match = (1ull << j) - 1ull;                       // earlier descents on the same path (j < 64)
        for (;;) {
            const uint4 hdr = nodes[node];
            const uint32_t hy = rfl(hdr.y);
            const int k = node_k(hy), first = rfl((int)hdr.x);
            if (node_flags(hy) & NF_TERMINAL) { kind = K_TERMINAL; break; }
            if (k == 0) { kind = (node == 0) ? K_ROOTPASS : K_REEXPAND; break; }
            if (depth >= (int)d.path_cap) { kind = K_NONE; break; }
            // every descent in `match` reached this node, which has children: each went on through one of them
            const int vi = ((match >> lane) & 1) ? d.path[((size_t)g * K + lane) * d.path_cap + depth] - first : -1;
            int v[NW];
#pragma unroll
            for (int t = 0; t < NW; t++) v[t] = 0;
            for (uint64_t mm = match; mm; mm &= mm - 1ull) {
                const int c = __builtin_amdgcn_readlane(vi, (int)__ffsll((unsigned long long)mm) - 1);
#pragma unroll
                for (int t = 0; t < NW; t++) v[t] += (c == t * 64 + lane) ? 1 : 0;
            }
            uint4 e[NW];
            uint32_t part = 0;
#pragma unroll
            for (int t = 0; t < NW; t++) {
                const int jj = t * 64 + lane;
                e[t] = (jj < k) ? edges[first + jj] : make_uint4(0u, 0u, 0u, 0u);
                part += e[t].y + (uint32_t)v[t];
            }
            const int S = (int)wave_uadd(part);                    // sum of the children's N + v (mcts.py:112)
            const float sq = d.sqrt_tab[min(S, d.sqrt_n - 1)];
            // first-play urgency on the counts the children are scored with: N + v, and W less the virtual visits
            float q0 = 0.0f;
            if (d.fpu > 0.0f) {                                    // wave-uniform
                FpuPart fp;
#pragma unroll
                for (int t = 0; t < NW; t++) {
                    if (t * 64 + lane < k) {
                        const float W = __uint_as_float(e[t].z);
                        fp.add(__uint_as_float(e[t].x), (int)e[t].y + v[t], (v[t] > 0) ? __fsub_rn(W, (float)v[t]) : W);
                    }
                }
                q0 = fpu_value(fp, depth == 0 ? d.fpu_root : d.fpu);
            }
            uint32_t bk = 0, bw = 0;
            int bi = BEST_NONE;
#pragma unroll
            for (int t = 0; t < NW; t++) {
                const int jj = t * 64 + lane;
                if (jj < k) {
                    const float W = __uint_as_float(e[t].z);
                    const float w = (v[t] > 0) ? __fsub_rn(W, (float)v[t]) : W;
                    const uint32_t key = child_key(d.cpuct, sq, __uint_as_float(e[t].x), (int)e[t].y + v[t], w, q0);
                    if (key > bk) { bk = key; bi = jj; bw = e[t].w; }
                }
            }
            const int best = best_child(bk, bi, k);
            if (best == BEST_NONE) { kind = K_NONE; break; }
            const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)bw, best & 63);
            if (lane == 0) path[depth] = first + best;
            match = __ballot(vi == best);                          // vi == -1 outside `match`
            depth++;
            c_levels++;
            c_scan += (uint64_t)k;
            parent = node;
            action = (int)(w >> 24);
            const uint32_t child = w & CHILD_NONE;
            if (child == CHILD_NONE) { kind = K_EXPAND; node = -1; break; }
            node = (int)child;
        }
        if (kind == K_NONE) { failed = true; break; }
        // the earlier descents left in `match` walked the same path and so ended on the same leaf
        const int dup = match ? (int)__ffsll((unsigned long long)match) - 1 : -1;
        const bool need = (kind == K_EXPAND || kind == K_REEXPAND || kind == K_ROOTPASS) && dup < 0;
        LeafRec *rec = m.leaves + (size_t)g * K + j;
        if (need) {
            BB<NW> black, white;
            const int lplayer = leaf_position<NW>(d, st, g, nodes, kind, parent, action, false, black, white);
            BB<NW> mask;
            bool term;
            float tv;
            leaf_rules<NW>(d.geo, gb, black, white, lplayer, mask, term, tv);
            write_eval_planes<NW>(planes + ((size_t)g * K + j) * 5 * d.geo.A, d.geo, d.sym, d.sym_seed, black, white);
            leaf_store<NW>(rec, black, white, mask, lplayer, term, tv);
        }
        if (lane == 0) {
            rec->kind = (uint8_t)kind;
            rec->node = node;
            rec->path_len = depth;
            rec->dup = dup;
            if (needs_eval) needs_eval[(size_t)g * K + j] = need;
        }
        c_evals += need ? 1 : 0;
        c_term += (kind == K_TERMINAL) ? 1 : 0;
        __syncthreads();   // this descent's path is read by the lanes of the next one
    }
    if (failed && lane == 0) fail_game(st);                     // path too deep / no selectable child: the game stops
    if (needs_eval && lane < K && (failed || lane >= keff)) needs_eval[(size_t)g * K + lane] = 0;
    if (lane == 0) {
        ms[1] = failed ? 0 : keff;
        st->ctr[TC_LEVELS] += c_levels;
        st->ctr[TC_SCANNED] += c_scan;
        if (!failed) st->ctr[TC_EVALS] += c_evals;
        st->ctr[TC_TERMINAL] += c_term;
    }
}

// expansion + backup of the K_eff descents of the last step, in descent order: the first occurrence of a leaf expands it
// (expand_leaf), then every descent backs its value up along its own path (backup_path)
template <int NW>
__device__ __forceinline__ void do_expand_backup_multi(const MctsDev &d, const MultiDev &m, const int g, const float *policy,
                                                       const float *value, const double *noise, const double eps) {
    GameState *st = d.state + g;
    const int lane = lane_id();
    const int K = m.K;
    int32_t *ms = m.mst + 2 * g;
    const int nl = rfl(ms[1]);
    if (nl == 0) return;
    const uint4 *nodes = d.nodes + (size_t)g * d.node_cap;
    uint4 *edges = d.edges + (size_t)g * d.edge_cap;
    for (int j = 0; j < nl; j++) {
        const LeafRec *rec = m.leaves + (size_t)g * K + j;
        const int kind = rfl((int)rec->kind);
        const int depth = rfl(rec->path_len);
        const int dup = rfl(rec->dup);
        const int32_t *path = d.path + ((size_t)g * K + j) * d.path_cap;
        const size_t row = (size_t)g * K + (dup >= 0 ? dup : j);
        float v;
        bool v_is_py = false;
        if (kind == K_TERMINAL) {
            v = rflf(__uint_as_float(nodes[rfl(rec->node)].z));
            v_is_py = true;
        } else if (dup >= 0) {
            v = rflf(value[row]);                                  // checked when the first occurrence was expanded
        } else {
            v = (kind == K_ROOTINIT) ? 0.0f : rflf(value[row]);
            if (!expand_leaf<NW>(d, st, g, rec, path, policy + row * d.geo.A, v, false, false, noise, eps)) {
                // NaN from the evaluator or a full arena: the game stops, the error is sticky
                if (lane == 0) { fail_game(st); ms[1] = 0; }
                return;
            }
        }
        if (kind == K_ROOTINIT) break;                             // no backup
        backup_path(edges, path, depth, v, v_is_py, st);
        __syncthreads();   // the next descent's backup and expansion read what this one wrote
    }
    if (lane == 0) ms[1] = 0;
}

template <int NW> __global__ void __launch_bounds__(64) k_mcts_multi(MctsDev d, MultiDev m, int do_backup, int do_sel,
                                                                     const float *policy, const float *value,
                                                                     const double *noise, double eps, float *planes,
                                                                     uint8_t *needs_eval) {
    const int g = blockIdx.x;
    if (do_backup) do_expand_backup_multi<NW>(d, m, g, policy, value, noise, eps);
    if (do_backup && do_sel) __syncthreads();
    if (do_sel) do_select_multi<NW>(d, m, g, planes, needs_eval);
}

// =============================================================================== tree reuse: re-root at the move played
// k_advance re-roots game g's tree at the child of its root under actions[g] and compacts that child's subtree to the front of
// the game's node, edge and board arenas, in place.  It relies on how expand_leaf grows a copied-board tree:
//   * a node with children gets its record and its edge range in the same call (K_EXPAND; the root: k_begin + K_ROOTINIT before
//     anything else), so node indices and the edge ranges of the nodes that have one both ascend in creation order;
//   * a child is created after its parent: its index is the larger one;
//   * a childless node that is expanded again (K_REEXPAND) has k = 0 again -- its board never changes -- so its first-edge
//     field, the only one that does not ascend, names no edge.
// Hence one ascending pass over the old indices decides membership (a node is kept iff its parent was, and the parent came
// earlier), the new index of a kept node is its rank among the kept ones, and with new <= old for node records, boards and edge
// ranges every move goes downwards onto records the pass has already left behind: no second copy of the arenas.  A second,
// parallel pass rewrites the child indices inside the kept edges through remap[].
// The chain over the nodes is serial; per 64 nodes it costs one round trip for the headers and the marks, plus one per KEPT node
// for its edges (marks inside the 64-node window travel through LDS, the others through remap[]).
template <int NW> __global__ void __launch_bounds__(64) k_advance(MctsDev d, const int32_t *actions, int32_t *kept_visits,
                                                                  int32_t *remap_all) {
    __shared__ int32_t win[64];
    const int g = blockIdx.x, lane = lane_id();
    GameState *st = d.state + g;
    uint4 *nodes = d.nodes + (size_t)g * d.node_cap;
    uint4 *edges = d.edges + (size_t)g * d.edge_cap;
    uint64_t *nboard = d.nboard + (size_t)g * d.node_cap * 2 * NW;
    int32_t *remap = remap_all + (size_t)g * d.node_cap;
    const int n_nodes = rfl(st->n_nodes), n_edges = rfl(st->n_edges);
    const int a = rfl(actions[g]);
    const uint4 rhdr = nodes[0];
    const int rk = node_k(rfl(rhdr.y)), rfirst = rfl((int)rhdr.x);
    // ---- the edge of the move played, and whether its subtree is kept
    int child = -1, keptN = 0;
    float keptW = 0.0f;
    bool ok = rfl((int)st->active) != 0 && rfl((int)st->err) == 0 && a >= 0 && a < d.geo.A && n_nodes <= (int)d.node_cap &&
              rk > 0 && rfirst >= 0 && rfirst + rk <= n_edges && n_edges <= (int)d.edge_cap;
    if (ok) {
        ok = false;
        for (int j0 = 0; j0 < rk; j0 += 64) {
            const int j = j0 + lane;
            const uint4 e = (j < rk) ? edges[rfirst + j] : make_uint4(0u, 0u, 0u, 0xFF000000u | CHILD_NONE);
            const uint64_t hit = __ballot(j < rk && (int)(e.w >> 24) == a);
            if (hit) {
                const int l = (int)__ffsll((unsigned long long)hit) - 1;
                const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)e.w, l);
                keptN = __builtin_amdgcn_readlane((int)e.y, l);
                keptW = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)e.z, l));
                child = (int)(w & CHILD_NONE);
                ok = (w & CHILD_NONE) != CHILD_NONE && child > 0 && child < n_nodes;
                break;
            }
        }
    }
    uint32_t chy = 0;
    if (ok) {
        chy = rfl(nodes[child].y);
        ok = !(node_flags(chy) & NF_TERMINAL) && node_k(chy) > 0;   // a terminal or childless position is searched afresh
    }
    if (!ok) {
        // nothing kept: the tree is emptied, so that a second advance finds no edge and the next yy_mcts_begin starts afresh
        if (lane == 0) {
            st->kept = 0;
            st->n_nodes = 1;
            st->n_edges = 0;
            st->root_N = 0;
            st->root_W = 0.0f;
            st->root_W_py = 0.0;
            st->root_w_is_py = 1;
            nodes[0] = make_uint4(0u, node_pack(0, 0, node_player(rfl(rhdr.y))), 0u, 0u);
            if (kept_visits) kept_visits[g] = 0;
        }
        return;
    }
    // ---- pass 1: membership, ranks and the moves, ascending
    for (int i = child + lane; i < n_nodes; i += 64) remap[i] = (i == child) ? 0 : -1;
    __syncthreads();
    int rank = 0, ne = 0;          // kept nodes / kept edges so far == the next new index / first edge
    bool bad = false;
    for (int base = child; base < n_nodes; base += 64) {
        __syncthreads();           // the marks earlier windows stored beyond themselves
        const int mine = base + lane;
        const uint4 hdr = (mine < n_nodes) ? nodes[mine] : make_uint4(0u, 0u, 0u, 0u);
        win[lane] = (mine < n_nodes) ? remap[mine] : -1;
        __syncthreads();
        for (int t = 0; t < 64 && base + t < n_nodes; t++) {
            if (rfl(win[t]) < 0) continue;
            const int i = base + t;
            const uint32_t hy = (uint32_t)__builtin_amdgcn_readlane((int)hdr.y, t);
            const int first = __builtin_amdgcn_readlane((int)hdr.x, t);
            const int k = (node_flags(hy) & NF_TERMINAL) ? 0 : node_k(hy);
            if (k > 0 && (first < ne || first + k > n_edges)) { bad = true; break; }   // never in a tree expand_leaf built
            for (int j0 = 0; j0 < k; j0 += 64) {
                const int j = j0 + lane;
                if (j < k) {
                    const uint4 e = edges[first + j];
                    edges[ne + j] = e;                                   // ne <= first: onto edges already moved or dropped
                    const int c = (int)(e.w & CHILD_NONE);
                    if ((e.w & CHILD_NONE) != CHILD_NONE && c > i && c < n_nodes) {
                        if (c < base + 64) win[c - base] = 0;
                        else remap[c] = 0;
                    }
                }
            }
            if (lane == 0) {
                nodes[rank] = make_uint4(k > 0 ? (uint32_t)ne : 0u, hy, (uint32_t)__builtin_amdgcn_readlane((int)hdr.z, t),
                                         (uint32_t)__builtin_amdgcn_readlane((int)hdr.w, t));
                remap[i] = rank;
            }
            if (rank != i && lane < 2 * NW) nboard[(size_t)rank * 2 * NW + lane] = nboard[(size_t)i * 2 * NW + lane];
            rank++;
            ne += k;
            __syncthreads();       // win[] marks of this node's children before the next node's test
        }
        if (bad) break;
    }
    __syncthreads();
    // ---- pass 2: the child indices inside the kept edges
    if (!bad)
        for (int e = lane; e < ne; e += 64) {
            const uint32_t w = edges[e].w;
            const uint32_t c = w & CHILD_NONE;
            if (c != CHILD_NONE) {
                const int nc = (c < (uint32_t)n_nodes) ? remap[c] : -1;
                edges[e].w = (w & 0xFF000000u) | (nc >= 0 ? (uint32_t)nc : CHILD_NONE);
            }
        }
    if (lane == 0) {
        if (bad) {                 // an inconsistent arena: the game fails like one whose arena overflowed
            fail_game(st);
            st->kept = 0;
            if (kept_visits) kept_visits[g] = 0;
        } else {
            st->n_nodes = rank;
            st->n_edges = ne;
            st->root_N = keptN;
            st->root_W = keptW;
            st->root_W_py = 0.0;
            st->root_w_is_py = 0;
            st->root_player = (int8_t)node_player(chy);
            st->kept = 1;
            if (kept_visits) kept_visits[g] = keptN;
        }
    }
}

template <int NW> __global__ void __launch_bounds__(64) k_root_counts(MctsDev d, int32_t *counts, float *cw, float *cp) {
    const int g = blockIdx.x, A = d.geo.A;
    const uint4 hdr = d.nodes[(size_t)g * d.node_cap];
    const int k = node_k(rfl(hdr.y)), first = rfl((int)hdr.x);
    const bool act = rfl((int)d.state[g].active) != 0;
    for (int a = lane_id(); a < A; a += 64) {
        counts[(size_t)g * A + a] = 0;
        if (cw) cw[(size_t)g * A + a] = 0.0f;
        if (cp) cp[(size_t)g * A + a] = 0.0f;
    }
    __syncthreads();
    if (!act) return;
    const uint4 *edges = d.edges + (size_t)g * d.edge_cap;
    for (int j = lane_id(); j < k; j += 64) {
        const uint4 e = edges[first + j];
        const int a = (int)(e.w >> 24);
        counts[(size_t)g * A + a] = (int)e.y;
        if (cw) cw[(size_t)g * A + a] = __uint_as_float(e.z);
        if (cp) cp[(size_t)g * A + a] = __uint_as_float(e.x);
    }
}

// Node.get_children_distribution (mcts.py:183-215) for T == 1 and T == 0
template <int NW> __global__ void __launch_bounds__(64) k_root_policy(MctsDev d, int tzero, double *pi) {
    root_distribution<NW>(d, blockIdx.x, tzero, pi + (size_t)blockIdx.x * d.geo.A);
}

__global__ void k_root_stats(MctsDev d, int32_t *visits, double *wsum) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= d.G) return;
    const GameState *st = d.state + g;
    if (visits) visits[g] = st->root_N;
    if (wsum) wsum[g] = st->root_w_is_py ? st->root_W_py : (double)st->root_W;
}

template <int NW> __global__ void __launch_bounds__(64) k_get_boards(MctsDev d, int8_t *boards) {
    const int g = blockIdx.x;
    const uint64_t *src = d.gboard + (size_t)g * 2 * NW;
    BB<NW> b = bb_uniform_load<NW>(src), w = bb_uniform_load<NW>(src + NW);
    bb_to_board<NW>(boards + (size_t)g * d.geo.A, d.geo.A, b, w);
}

// Every counter summed over the games into out[0 .. TC_COUNT).  take_failures (yy_mcts_status alone): out[TC_COUNT] counts the
// games that failed in ANY search since the last such call, and their sticky marks are cleared; else no mark is touched
__global__ void k_tree_counters(MctsDev d, int take_failures, uint64_t *out /*[TC_COUNT + 1], zeroed*/) {
    uint64_t acc[TC_COUNT + 1] = {};
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < d.G; g += gridDim.x * blockDim.x) {
        GameState *st = d.state + g;
        for (int i = 0; i < TC_COUNT; i++) acc[i] += st->ctr[i];
        if (take_failures) {
            acc[TC_COUNT] += (st->err || st->err_ever) ? 1 : 0;
            st->err_ever = 0;
        }
    }
    for (int i = 0; i <= TC_COUNT; i++)
        if (acc[i]) atomicAdd((unsigned long long *)&out[i], (unsigned long long)acc[i]);
}

// sync; what k_tree_counters sums, on the host
static int tree_counters(yy_mcts *c, bool take_failures, uint64_t h[TC_COUNT + 1]) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(c->scratch, 0, (TC_COUNT + 1) * sizeof(uint64_t)));
    hipLaunchKernelGGL(k_tree_counters, dim3(64), dim3(256), 0, 0, c->dev, (int)take_failures, c->scratch);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(h, c->scratch, (TC_COUNT + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return YY_OK;
}

__global__ void k_reset_counters(MctsDev d) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= d.G) return;
    for (int i = 0; i < TC_COUNT; i++) d.state[g].ctr[i] = 0;
    if (g == 0 && d.sh_sweep) d.sh_sweep[SH_SW_EVICTED] = 0;
}

// solver: the root's proven status int8 [G] and that of the root's children by action int8 [G,A] (PV_*: 0 none, 1 WIN, 2 LOSS,
// 3 DRAW, each for the side to move at that node); all 0 without YY_FLAG_SOLVER and for an inactive game
template <int NW> __global__ void __launch_bounds__(64) k_root_proven(MctsDev d, int8_t *root, int8_t *child) {
    const int g = blockIdx.x, A = d.geo.A;
    const uint4 *nodes = d.nodes + (size_t)g * d.node_cap;
    const uint4 hdr = nodes[0];
    const int k = node_k(rfl(hdr.y)), first = rfl((int)hdr.x);
    const bool on = d.solver && rfl((int)d.state[g].active) != 0;
    for (int a = lane_id(); a < A; a += 64) child[(size_t)g * A + a] = 0;
    if (lane_id() == 0) root[g] = on ? (int8_t)node_proven(hdr) : (int8_t)0;
    __syncthreads();
    if (!on || (node_flags(rfl(hdr.y)) & NF_TERMINAL)) return;
    const uint4 *edges = d.edges + (size_t)g * d.edge_cap;
    for (int j = lane_id(); j < k; j += 64) {
        const uint4 e = edges[first + j];
        const uint32_t c = e.w & CHILD_NONE;
        if (c != CHILD_NONE) child[(size_t)g * A + (int)(e.w >> 24)] = (int8_t)node_proven(nodes[c]);
    }
}

// Gumbel root search: s0 by action f32 [G,A] (NaN: no such root edge, an inactive game) / the Gumbel winner int32 [G]
template <int NW> __global__ void __launch_bounds__(64) k_root_gumbel_scores(MctsDev d, float *out) {
    const int g = blockIdx.x, A = d.geo.A;
    const uint4 hdr = d.nodes[(size_t)g * d.node_cap];
    const int k = node_k(rfl(hdr.y)), first = rfl((int)hdr.x);
    for (int a = lane_id(); a < A; a += 64) out[(size_t)g * A + a] = __uint_as_float(0x7FC00000u);
    __syncthreads();
    if (rfl((int)d.state[g].active) == 0) return;
    const uint4 *edges = d.edges + (size_t)g * d.edge_cap;
    for (int j = lane_id(); j < k; j += 64) out[(size_t)g * A + (int)(edges[first + j].w >> 24)] = d.g_s0[(size_t)g * A + j];
}
template <int NW> __global__ void __launch_bounds__(64) k_root_gumbel_action(MctsDev d, int32_t *out) {
    const int a = gumbel_winner<NW>(d, blockIdx.x);
    if (lane_id() == 0) out[blockIdx.x] = a;
}

// ---------------------------------------------------------------------------------- host API
extern "C" int yy_mcts_create(const yy_mcts_config *cfg, yy_mcts **out) {
    if (!cfg || !out) return set_err(YY_E_INVALID, "null pointer%s%s");
    if (int e = check_geo(cfg->G, cfg->R, cfg->C)) return e;
    if (cfg->max_sims < 1) return set_err(YY_E_INVALID, "max_sims < 1%s%s");
    if ((cfg->flags & YY_FLAG_REUSE_PASS_VALUE) && (cfg->flags & YY_FLAG_ALIASED))
        return set_err(YY_E_INVALID, "YY_FLAG_REUSE_PASS_VALUE needs copied boards: with the aliased board a node's position changes between visits%s%s");
    if ((cfg->flags & YY_FLAG_EVAL_SYMMETRY) && (cfg->flags & YY_FLAG_ALIASED))
        return set_err(YY_E_UNSUPPORTED, "YY_FLAG_EVAL_SYMMETRY needs copied boards (YY_FLAG_ALIASED reproduces the reference, which has no such option)%s%s");
    if (cfg->flags & YY_FLAG_FORCED_PLAYOUTS) {
        if (cfg->flags & YY_FLAG_ALIASED)
            return set_err(YY_E_UNSUPPORTED, "YY_FLAG_FORCED_PLAYOUTS needs copied boards (YY_FLAG_ALIASED reproduces the reference, which has no such option)%s%s");
        if (cfg->leaves_per_step > 1)
            return set_err(YY_E_UNSUPPORTED, "YY_FLAG_FORCED_PLAYOUTS: leaves_per_step > 1 is not supported (the forcing test is part of the one-descent selection)%s%s");
        if (!(cfg->forced_playouts > 0.0 && cfg->forced_playouts < (double)INFINITY))
            return set_err(YY_E_INVALID, "YY_FLAG_FORCED_PLAYOUTS: forced_playouts must be positive and finite%s%s");
    }
    if (cfg->flags & YY_FLAG_FPU_REDUCTION) {
        if (!(cfg->fpu_reduction > 0.0f && cfg->fpu_reduction < INFINITY))
            return set_err(YY_E_INVALID, "YY_FLAG_FPU_REDUCTION: fpu_reduction must be positive and finite%s%s");
        if (!(cfg->fpu_reduction_root >= 0.0f && cfg->fpu_reduction_root < INFINITY))
            return set_err(YY_E_INVALID, "YY_FLAG_FPU_REDUCTION: fpu_reduction_root must be finite and >= 0%s%s");
    }
    if (cfg->flags & YY_FLAG_SOLVER) {
        if (cfg->flags & YY_FLAG_ALIASED)
            return set_err(YY_E_UNSUPPORTED, "YY_FLAG_SOLVER needs copied boards: with the aliased board a node's position changes between visits%s%s");
        if (cfg->leaves_per_step > 1)
            return set_err(YY_E_UNSUPPORTED, "YY_FLAG_SOLVER: leaves_per_step > 1 is not supported (proofs under virtual visits are a follow-up)%s%s");
    }
    if (cfg->flags & YY_FLAG_GUMBEL_ROOT) {
        if (cfg->flags & YY_FLAG_ALIASED)
            return set_err(YY_E_UNSUPPORTED, "YY_FLAG_GUMBEL_ROOT needs copied boards (YY_FLAG_ALIASED reproduces the reference, which has no such option)%s%s");
        if (cfg->leaves_per_step > 1)
            return set_err(YY_E_UNSUPPORTED, "YY_FLAG_GUMBEL_ROOT: leaves_per_step > 1 is not supported (sequential halving is part of the one-descent selection)%s%s");
        if (cfg->flags & (YY_FLAG_FORCED_PLAYOUTS | YY_FLAG_SOLVER))
            return set_err(YY_E_UNSUPPORTED, "YY_FLAG_GUMBEL_ROOT does not go with YY_FLAG_FORCED_PLAYOUTS or YY_FLAG_SOLVER (each plans the root's visits itself)%s%s");
        if (cfg->gumbel_root < 2 || cfg->gumbel_root > 64)
            return set_err(YY_E_INVALID, "YY_FLAG_GUMBEL_ROOT: gumbel_root outside 2 .. 64%s%s");
        if (!(cfg->gumbel_c_visit >= 0.0f && cfg->gumbel_c_visit < INFINITY))
            return set_err(YY_E_INVALID, "YY_FLAG_GUMBEL_ROOT: gumbel_c_visit must be finite and >= 0%s%s");
        if (!(cfg->gumbel_c_scale > 0.0f && cfg->gumbel_c_scale < INFINITY))
            return set_err(YY_E_INVALID, "YY_FLAG_GUMBEL_ROOT: gumbel_c_scale must be positive and finite%s%s");
    }
    if ((cfg->flags & YY_FLAG_GUMBEL_INTERIOR) && !(cfg->flags & YY_FLAG_GUMBEL_ROOT))
        return set_err(YY_E_UNSUPPORTED, "YY_FLAG_GUMBEL_INTERIOR needs YY_FLAG_GUMBEL_ROOT (it completes the Gumbel root search below the root)%s%s");
    if ((cfg->flags & YY_FLAG_GUMBEL_INTERIOR) && (cfg->flags & YY_FLAG_FPU_REDUCTION))
        return set_err(YY_E_UNSUPPORTED, "YY_FLAG_GUMBEL_INTERIOR does not go with YY_FLAG_FPU_REDUCTION (no PUCT score is left below the root, and the root never had one)%s%s");
    if (cfg->leaves_per_step < 0) return set_err(YY_E_INVALID, "leaves_per_step < 0%s%s");
    if (cfg->leaves_per_step > 64) return set_err(YY_E_UNSUPPORTED, "leaves_per_step > 64%s%s");
    if (cfg->leaves_per_step > 1) {
        if (cfg->flags & YY_FLAG_ALIASED)
            return set_err(YY_E_UNSUPPORTED, "leaves_per_step > 1 needs copied boards (YY_FLAG_ALIASED is not supported)%s%s");
        if (cfg->flags & (YY_FLAG_REUSE_PASS_VALUE | YY_FLAG_REUSE_TRANSPOSITIONS | YY_FLAG_KEEP_EVALUATIONS))
            return set_err(YY_E_UNSUPPORTED, "leaves_per_step > 1 does not support evaluation reuse (YY_FLAG_REUSE_PASS_VALUE, "
                                             "YY_FLAG_REUSE_TRANSPOSITIONS, YY_FLAG_KEEP_EVALUATIONS)%s%s");
    }
    yy_mcts *c = new yy_mcts();
    memset(c, 0, sizeof *c);
    c->cfg = *cfg;
    c->target_sims = cfg->max_sims;
    MctsDev &d = c->dev;
    MultiDev &m = c->multi;
    d.G = cfg->G;
    d.aliased = (cfg->flags & YY_FLAG_ALIASED) ? 1u : 0u;
    d.reuse = (cfg->flags & YY_FLAG_REUSE_PASS_VALUE) ? 1u : 0u;
    d.ec_keep = (cfg->flags & YY_FLAG_KEEP_EVALUATIONS) ? 1u : 0u;
    d.cpuct = cfg->cpuct;
    d.sym = (cfg->flags & YY_FLAG_EVAL_SYMMETRY) ? 1u : 0u;
    d.sym_seed = d.sym ? cfg->symmetry_seed : 0ull;
    d.forced = (cfg->flags & YY_FLAG_FORCED_PLAYOUTS) ? cfg->forced_playouts : 0.0;
    d.fpu = (cfg->flags & YY_FLAG_FPU_REDUCTION) ? cfg->fpu_reduction : 0.0f;
    d.fpu_root = (cfg->flags & YY_FLAG_FPU_REDUCTION) ? cfg->fpu_reduction_root : 0.0f;
    d.solver = (cfg->flags & YY_FLAG_SOLVER) ? 1u : 0u;
    d.gumbel = (cfg->flags & YY_FLAG_GUMBEL_ROOT) ? (uint32_t)cfg->gumbel_root : 0u;
    d.g_cvisit = d.gumbel ? cfg->gumbel_c_visit : 0.0f;
    d.g_cscale = d.gumbel ? cfg->gumbel_c_scale : 0.0f;
    d.g_interior = (cfg->flags & YY_FLAG_GUMBEL_INTERIOR) ? 1u : 0u;
    m.K = cfg->leaves_per_step > 1 ? cfg->leaves_per_step : 1;
    // virtual visits: a sum of child counts reaches max_sims - 1 + K - 1 within a step
    d.sqrt_n = cfg->max_sims + 2 + (m.K > 1 ? m.K : 0);
    yy_make_geo(&d.geo, cfg->R, cfg->C, cfg->flags & YY_FLAG_ROWCOL);
    const int A = d.geo.A, NW = d.geo.NW;
    d.node_cap = cfg->nodes_per_game > 0 ? cfg->nodes_per_game : (int64_t)cfg->max_sims + 2;
    d.edge_cap = cfg->edges_per_game > 0 ? cfg->edges_per_game : ((int64_t)cfg->max_sims + 2) * A;
    if (d.node_cap >= (int64_t)CHILD_NONE || d.edge_cap > 0x7FFFFFFFll)
        { delete c; return set_err(YY_E_UNSUPPORTED, "arena per game too large%s%s"); }
    // copied mode: every level places a stone, so depth <= A+1; aliased mode: depth <= sims
    d.path_cap = d.aliased ? (int64_t)cfg->max_sims + 2 : (int64_t)A + 2;
    const size_t G = (size_t)cfg->G;
    const bool ec_on = (cfg->flags & (YY_FLAG_REUSE_TRANSPOSITIONS | YY_FLAG_KEEP_EVALUATIONS)) != 0;
    // slots per game: 4x the node arena (the positions of several searches of a game stay useful), fewer when the
    // policy rows of all games would exceed 48 GiB, never fewer than 2x the arena of one search
    int64_t ec_cap = 64;
    while (ec_cap < 4 * d.node_cap) ec_cap *= 2;
    while (ec_cap > 2 * d.node_cap && (double)G * (double)ec_cap * A * 4.0 > 48.0 * 1073741824.0) ec_cap /= 2;
    d.ec.mask = (uint32_t)(ec_cap - 1);
    struct { void **p; size_t n; } allocs[] = {
        {(void **)&d.edges, G * d.edge_cap * sizeof(uint4)},
        {(void **)&d.nodes, G * d.node_cap * sizeof(uint4)},
        {(void **)&d.nboard, d.aliased ? 8 : G * d.node_cap * 2 * NW * sizeof(uint64_t)},
        {(void **)&d.gboard, G * 2 * NW * sizeof(uint64_t)},
        {(void **)&d.path, G * m.K * d.path_cap * sizeof(int32_t)},
        {(void **)&d.state, G * sizeof(GameState)},
        {(void **)&d.sqrt_tab, (size_t)d.sqrt_n * sizeof(float)},
        {(void **)&m.leaves, m.K > 1 ? G * m.K * sizeof(LeafRec) : 0},
        {(void **)&m.mst, m.K > 1 ? G * 2 * sizeof(int32_t) : 0},
        {(void **)&c->scratch, (TC_COUNT + 1) * sizeof(uint64_t)},
        {(void **)&d.ec.meta, ec_on ? G * (size_t)ec_cap * sizeof(uint32_t) : 0},
        {(void **)&d.ec.key, ec_on ? G * (size_t)ec_cap * 2 * NW * sizeof(uint64_t) : 0},
        {(void **)&d.ec.val, ec_on ? G * (size_t)ec_cap * sizeof(float) : 0},
        {(void **)&d.ec.pol, ec_on ? G * (size_t)ec_cap * A * sizeof(float) : 0},
        {(void **)&d.g_s0, d.gumbel ? G * A * sizeof(float) : 0},
    };
    for (auto &a : allocs) {
        if (a.n == 0) continue;
        const hipError_t me = hipMalloc(a.p, a.n);
        if (me != hipSuccess) {
            (void)hipGetLastError();
            char what[96];
            snprintf(what, sizeof what, " (%zu bytes after %llu allocated)", a.n, (unsigned long long)c->bytes);
            *a.p = nullptr;
            yy_mcts_destroy(c);
            return set_err(YY_E_NOMEM, "hipMalloc failed: %s%s", hipGetErrorString(me), what);
        }
        c->bytes += a.n;
    }
    // f32(math.sqrt(S)) table built with the host's correctly rounded double sqrt (mcts.py:130)
    float *tab = new float[d.sqrt_n];
    for (int s = 0; s < d.sqrt_n; s++) tab[s] = (float)sqrt((double)s);
    hipError_t e = hipMemset(d.state, 0, G * sizeof(GameState));
    if (e == hipSuccess) e = hipMemset(d.nodes, 0, G * d.node_cap * sizeof(uint4));
    if (e == hipSuccess && d.ec.meta) e = hipMemset(d.ec.meta, 0, G * (size_t)ec_cap * sizeof(uint32_t));
    if (e == hipSuccess && m.mst) e = hipMemset(m.mst, 0, G * 2 * sizeof(int32_t));
    if (e == hipSuccess && d.g_s0) e = hipMemset(d.g_s0, 0, G * A * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(d.sqrt_tab, tab, (size_t)d.sqrt_n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    delete[] tab;
    if (e != hipSuccess) { yy_mcts_destroy(c); return set_err(YY_E_HIP, "arena initialisation: %s%s", hipGetErrorString(e)); }
    *out = c;
    return YY_OK;
}

extern "C" int yy_mcts_destroy(yy_mcts *c) {
    if (!c) return YY_OK;
    const MctsDev &d = c->dev;
    void *ps[] = {d.edges, d.nodes, d.nboard, d.gboard, d.path, d.state, d.sqrt_tab, c->scratch, d.ec.meta, d.ec.key, d.ec.val, d.ec.pol,
                  c->multi.leaves, c->multi.mst, c->remap, d.g_s0};
    for (void *p : ps)
        if (p) (void)hipFree(p);
    delete c;
    return YY_OK;
}

extern "C" int yy_mcts_set_num_sims(yy_mcts *c, int32_t num_sims) {
    if (!c) return set_err(YY_E_INVALID, "null pointer%s%s");
    if (num_sims < 0 || num_sims > c->cfg.max_sims) return set_err(YY_E_INVALID, "num_sims outside 0 .. max_sims%s%s");
    c->target_sims = num_sims == 0 ? c->cfg.max_sims : num_sims;
    return YY_OK;
}

extern "C" int yy_mcts_set_sim_budgets(yy_mcts *c, const int32_t *budgets_dev) {
    if (!c) return set_err(YY_E_INVALID, "null pointer%s%s");
    c->budgets = budgets_dev;
    return YY_OK;
}

extern "C" int yy_mcts_set_gumbel(yy_mcts *c, const float *rows_dev) {
    if (!c) return set_err(YY_E_INVALID, "null pointer%s%s");
    if (!c->dev.gumbel) return set_err(YY_E_UNSUPPORTED, "yy_mcts_set_gumbel: the context was created without YY_FLAG_GUMBEL_ROOT%s%s");
    c->dev.g_rows = rows_dev;
    return YY_OK;
}

extern "C" int yy_mcts_root_gumbel(yy_mcts *c, float *out, yy_stream_t s) {
    if (!c || !out) return set_err(YY_E_INVALID, "null pointer%s%s");
    if (!c->dev.gumbel) return set_err(YY_E_UNSUPPORTED, "yy_mcts_root_gumbel: the context was created without YY_FLAG_GUMBEL_ROOT%s%s");
    DISPATCH_NW(c->dev.geo.NW, k_root_gumbel_scores<NW><<<dim3(c->cfg.G), dim3(64), 0, (hipStream_t)s>>>(c->dev, out));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

extern "C" int yy_mcts_root_gumbel_action(yy_mcts *c, int32_t *out, yy_stream_t s) {
    if (!c || !out) return set_err(YY_E_INVALID, "null pointer%s%s");
    if (!c->dev.gumbel) return set_err(YY_E_UNSUPPORTED, "yy_mcts_root_gumbel_action: the context was created without YY_FLAG_GUMBEL_ROOT%s%s");
    DISPATCH_NW(c->dev.geo.NW, k_root_gumbel_action<NW><<<dim3(c->cfg.G), dim3(64), 0, (hipStream_t)s>>>(c->dev, out));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

extern "C" int yy_mcts_memory_bytes(const yy_mcts *c, uint64_t *out) {
    if (!c || !out) return set_err(YY_E_INVALID, "null pointer%s%s");
    *out = c->bytes;
    return YY_OK;
}

extern "C" int yy_mcts_begin(yy_mcts *c, const int8_t *boards, const int8_t *players, const uint8_t *active,
                             float *planes, yy_stream_t s) {
    if (!c || !boards || !players || !planes) return set_err(YY_E_INVALID, "null pointer%s%s");
    DISPATCH_NW(c->dev.geo.NW, k_begin<NW><<<dim3(c->cfg.G), dim3(64), 0, (hipStream_t)s>>>(c->dev, c->multi,
                                                   // Gumbel root search plans the budget: the real count, not "no limit"
                                                   (c->multi.K > 1 || c->dev.gumbel) ? c->target_sims : 0x7FFFFFFF, c->target_sims, c->budgets, c->cfg.max_sims,
                                                   boards, players, active, planes));
    HIP_TRY(hipGetLastError());
    c->pending = 2;  // root expansion pending
    return YY_OK;
}

extern "C" int yy_mcts_advance(yy_mcts *c, const int32_t *actions, int32_t *kept_visits, yy_stream_t s) {
    if (!c || !actions) return set_err(YY_E_INVALID, "null pointer%s%s");
    if (c->cfg.flags & YY_FLAG_ALIASED)
        return set_err(YY_E_UNSUPPORTED, "yy_mcts_advance needs copied boards: with the aliased board a node's position changes between visits%s%s");
    if (c->multi.K > 1) return set_err(YY_E_UNSUPPORTED, "yy_mcts_advance: leaves_per_step > 1 does not support tree reuse%s%s");
    if (c->dev.gumbel)
        return set_err(YY_E_UNSUPPORTED, "yy_mcts_advance: YY_FLAG_GUMBEL_ROOT does not support tree reuse (a kept root has no base scores and its visits are not a halving schedule's)%s%s");
    if (c->pending != 0) return set_err(YY_E_STATE, "yy_mcts_advance with a select or a root expansion pending%s%s");
    if (!c->remap) {
        const size_t n = (size_t)c->cfg.G * c->dev.node_cap * sizeof(int32_t);
        const hipError_t me = hipMalloc((void **)&c->remap, n);
        if (me != hipSuccess) {
            (void)hipGetLastError();
            c->remap = nullptr;
            return set_err(YY_E_NOMEM, "hipMalloc failed: %s%s", hipGetErrorString(me), " (tree reuse remap array)");
        }
        c->bytes += n;
    }
    DISPATCH_NW(c->dev.geo.NW, k_advance<NW><<<dim3(c->cfg.G), dim3(64), 0, (hipStream_t)s>>>(c->dev, actions, kept_visits, c->remap));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

static int launch_mcts(yy_mcts *c, int backup, int sel, const float *policy, const float *value, const double *noise,
                       double eps, float *planes, uint8_t *needs_eval, yy_stream_t s) {
    // Gumbel root search: a root expansion reads the Gumbel rows
    if (backup && c->dev.gumbel && !c->dev.g_rows) return set_err(YY_E_STATE, "YY_FLAG_GUMBEL_ROOT: no Gumbel rows set (yy_mcts_set_gumbel)%s%s");
    // shared evaluation table: every tree-step launch gets a stamp of its own; without the table nothing is launched here
    if (c->dev.sh.meta) {
        hipLaunchKernelGGL(k_stamp, dim3(1), dim3(1), 0, (hipStream_t)s, c->dev.sh_stamp);
        HIP_TRY(hipGetLastError());
    }
    if (c->multi.K > 1) {
        DISPATCH_NW(c->dev.geo.NW, k_mcts_multi<NW><<<dim3(c->cfg.G), dim3(64), 0, (hipStream_t)s>>>(c->dev, c->multi, backup, sel,
                                                       policy, value, noise, eps, planes, needs_eval));
    } else {
        DISPATCH_NW(c->dev.geo.NW, k_mcts<NW><<<dim3(c->cfg.G), dim3(64), 0, (hipStream_t)s>>>(c->dev, backup, sel,
                                                       policy, value, noise, eps, planes, needs_eval));
    }
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

extern "C" int yy_mcts_expand_root(yy_mcts *c, const float *policy, const double *noise, double eps, yy_stream_t s) {
    if (!c || !policy) return set_err(YY_E_INVALID, "null pointer%s%s");
    if (c->dev.g_interior)
        return set_err(YY_E_UNSUPPORTED, "yy_mcts_expand_root: YY_FLAG_GUMBEL_INTERIOR keeps the root's value (yy_mcts_expand_root_value)%s%s");
    if (c->pending != 2) return set_err(YY_E_STATE, "yy_mcts_expand_root without yy_mcts_begin%s%s");
    int e = launch_mcts(c, 1, 0, policy, nullptr, noise, eps, nullptr, nullptr, s);
    if (e == YY_OK) c->pending = 0;
    return e;
}

extern "C" int yy_mcts_expand_root_value(yy_mcts *c, const float *policy, const float *value, const double *noise, double eps,
                                         yy_stream_t s) {
    if (!c || !policy || !value) return set_err(YY_E_INVALID, "null pointer%s%s");
    if (c->pending != 2) return set_err(YY_E_STATE, "yy_mcts_expand_root_value without yy_mcts_begin%s%s");
    // without the flag the kernel discards the value, as yy_mcts_expand_root does
    int e = launch_mcts(c, 1, 0, policy, value, noise, eps, nullptr, nullptr, s);
    if (e == YY_OK) c->pending = 0;
    return e;
}

extern "C" int yy_mcts_select(yy_mcts *c, float *planes, uint8_t *needs_eval, yy_stream_t s) {
    if (!c || !planes) return set_err(YY_E_INVALID, "null pointer%s%s");
    if (c->pending != 0) return set_err(YY_E_STATE, "yy_mcts_select with an expansion pending%s%s");
    int e = launch_mcts(c, 0, 1, nullptr, nullptr, nullptr, 0.0, planes, needs_eval, s);
    if (e == YY_OK) c->pending = 1;
    return e;
}

extern "C" int yy_mcts_expand_backup(yy_mcts *c, const float *policy, const float *value, yy_stream_t s) {
    if (!c || !policy || !value) return set_err(YY_E_INVALID, "null pointer%s%s");
    if (c->pending != 1) return set_err(YY_E_STATE, "yy_mcts_expand_backup without yy_mcts_select%s%s");
    int e = launch_mcts(c, 1, 0, policy, value, nullptr, 0.0, nullptr, nullptr, s);
    if (e == YY_OK) c->pending = 0;
    return e;
}

extern "C" int yy_mcts_step(yy_mcts *c, const float *policy, const float *value, float *planes, uint8_t *needs_eval,
                            yy_stream_t s) {
    if (!c || !policy || !value || !planes) return set_err(YY_E_INVALID, "null pointer%s%s");
    if (c->pending != 1) return set_err(YY_E_STATE, "yy_mcts_step without a pending select%s%s");
    return launch_mcts(c, 1, 1, policy, value, nullptr, 0.0, planes, needs_eval, s);
}

// yy_mcts_step with a noise array for the root expansions pending among the leaves (yy_common.h; yy_mcts_step_selfplay)
extern "C" __attribute__((visibility("hidden"))) int yy_mcts_step_noise(yy_mcts *c, const float *policy, const float *value, const double *noise, double eps,
                                  float *planes, uint8_t *needs_eval, yy_stream_t s) {
    return launch_mcts(c, 1, 1, policy, value, noise, eps, planes, needs_eval, s);
}

extern "C" int yy_mcts_root_counts(yy_mcts *c, int32_t *counts, float *cw, float *cp, yy_stream_t s) {
    if (!c || !counts) return set_err(YY_E_INVALID, "null pointer%s%s");
    DISPATCH_NW(c->dev.geo.NW,
                k_root_counts<NW><<<dim3(c->cfg.G), dim3(64), 0, (hipStream_t)s>>>(c->dev, counts, cw, cp));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

extern "C" int yy_mcts_root_policy(yy_mcts *c, int tzero, double *pi, yy_stream_t s) {
    if (!c || !pi) return set_err(YY_E_INVALID, "null pointer%s%s");
    DISPATCH_NW(c->dev.geo.NW,
                k_root_policy<NW><<<dim3(c->cfg.G), dim3(64), 0, (hipStream_t)s>>>(c->dev, tzero, pi));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

extern "C" int yy_mcts_root_stats(yy_mcts *c, int32_t *visits, double *wsum, yy_stream_t s) {
    if (!c) return set_err(YY_E_INVALID, "null pointer%s%s");
    hipLaunchKernelGGL(k_root_stats, dim3((c->cfg.G + 255) / 256), dim3(256), 0, (hipStream_t)s, c->dev, visits, wsum);
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

__global__ void k_tree_sizes(MctsDev d, int32_t *sizes) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= d.G) return;
    sizes[2 * g] = d.state[g].n_nodes;
    sizes[2 * g + 1] = d.state[g].n_edges;
}

extern "C" int yy_mcts_tree(yy_mcts *c, uint32_t *nodes, uint32_t *edges, int32_t *sizes, int64_t *caps, yy_stream_t s) {
    if (!c) return set_err(YY_E_INVALID, "null pointer%s%s");
    const MctsDev &d = c->dev;
    if (caps) { caps[0] = d.node_cap; caps[1] = d.edge_cap; }
    const size_t G = (size_t)c->cfg.G;
    if (nodes) HIP_TRY(hipMemcpyAsync(nodes, d.nodes, G * d.node_cap * sizeof(uint4), hipMemcpyDeviceToDevice, (hipStream_t)s));
    if (edges) HIP_TRY(hipMemcpyAsync(edges, d.edges, G * d.edge_cap * sizeof(uint4), hipMemcpyDeviceToDevice, (hipStream_t)s));
    if (sizes) {
        hipLaunchKernelGGL(k_tree_sizes, dim3((c->cfg.G + 255) / 256), dim3(256), 0, (hipStream_t)s, d, sizes);
        HIP_TRY(hipGetLastError());
    }
    return YY_OK;
}

extern "C" int yy_mcts_get_boards(yy_mcts *c, int8_t *boards, yy_stream_t s) {
    if (!c || !boards) return set_err(YY_E_INVALID, "null pointer%s%s");
    DISPATCH_NW(c->dev.geo.NW, k_get_boards<NW><<<dim3(c->cfg.G), dim3(64), 0, (hipStream_t)s>>>(c->dev, boards));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

extern "C" int yy_mcts_status(yy_mcts *c, int32_t *n_overflow, uint64_t *counters) {
    if (!c) return set_err(YY_E_INVALID, "null pointer%s%s");
    uint64_t h[TC_COUNT + 1];
    if (int e = tree_counters(c, true, h)) return e;
    if (counters) {
        for (int i = TC_EVALS; i < TC_FORCED; i++) counters[i] = h[i];
    }
    if (n_overflow) *n_overflow = (int32_t)h[TC_COUNT];
    if (h[TC_COUNT]) return set_err(YY_E_ARENA, "tree arena overflow or non-finite evaluator output in at least one game since the last status call%s%s");
    return YY_OK;
}

extern "C" int yy_mcts_forced_descents(yy_mcts *c, uint64_t *out) {
    if (!c || !out) return set_err(YY_E_INVALID, "null pointer%s%s");
    uint64_t h[TC_COUNT + 1];
    if (int e = tree_counters(c, false, h)) return e;
    *out = h[TC_FORCED];
    return YY_OK;
}

extern "C" int yy_mcts_root_proven(yy_mcts *c, int8_t *root, int8_t *child, yy_stream_t s) {
    if (!c || !root || !child) return set_err(YY_E_INVALID, "null pointer%s%s");
    if (c->pending != 0) return set_err(YY_E_STATE, "yy_mcts_root_proven with a select or a root expansion pending%s%s");
    DISPATCH_NW(c->dev.geo.NW, k_root_proven<NW><<<dim3(c->cfg.G), dim3(64), 0, (hipStream_t)s>>>(c->dev, root, child));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

extern "C" int yy_mcts_solver_counters(yy_mcts *c, uint64_t *out) {
    if (!c || !out) return set_err(YY_E_INVALID, "null pointer%s%s");
    if (c->pending != 0) return set_err(YY_E_STATE, "yy_mcts_solver_counters with a select or a root expansion pending%s%s");
    uint64_t h[TC_COUNT + 1];
    if (int e = tree_counters(c, false, h)) return e;
    for (int i = TC_SV_NODES; i < TC_COUNT; i++) out[i - TC_SV_NODES] = h[i];
    return YY_OK;
}

// ---- shared book of pre-evaluated positions
template <int NW> __global__ void k_book_insert(const uint64_t *__restrict__ keys, int n, uint32_t *meta, uint64_t *tkeys,
                                                uint32_t mask, int32_t *slot_of) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t *k = keys + (size_t)i * 2 * NW;
    // the sequence leaf_lookup walks; keys are distinct: a taken slot is another position
    const int got = tt_probe(bb_hash<NW>(k, k + NW), mask,
                             [&](uint32_t at) { return atomicCAS(&meta[at], 0u, 1u) == 0u ? TT_HIT : TT_NEXT; });
    if (got >= 0)
        for (int j = 0; j < 2 * NW; j++) tkeys[(size_t)got * 2 * NW + j] = k[j];
    slot_of[i] = got;      // -1: no free slot within the probe window (the position stays out of the book)
}

extern "C" int yy_book_insert(const uint64_t *keys, int n, int R, int C, uint32_t *meta, uint64_t *table_keys, int64_t cap,
                              int32_t *slot_of, yy_stream_t s) {
    if (n == 0) return YY_OK;
    if (!keys || !meta || !table_keys || !slot_of || n < 0 || cap < 64 || (cap & (cap - 1)) || cap > (1ll << 31))
        return set_err(YY_E_INVALID, "yy_book_insert: bad argument (cap must be a power of two)%s%s");
    if (int e = check_geo(1, R, C)) return e;
    const int nw = (R * C + 63) / 64;
    DISPATCH_NW(nw, k_book_insert<NW><<<dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)s>>>(keys, n, meta, table_keys,
                                                                                               (uint32_t)(cap - 1), slot_of));
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

extern "C" int yy_mcts_set_book(yy_mcts *c, const uint32_t *meta, const uint64_t *keys, const float *val, const float *pol,
                                int64_t cap, int max_stones) {
    if (!c) return set_err(YY_E_INVALID, "null pointer%s%s");
    if (!meta) { c->dev.bk = PosTable{}; c->dev.bk_stones = 0; return YY_OK; }
    if (!keys || !val || !pol || cap < 64 || (cap & (cap - 1)) || cap > (1ll << 31) || max_stones < 1)
        return set_err(YY_E_INVALID, "yy_mcts_set_book: bad argument (cap must be a power of two)%s%s");
    if (c->multi.K > 1) return set_err(YY_E_UNSUPPORTED, "yy_mcts_set_book: leaves_per_step > 1 does not support evaluation reuse%s%s");
    // the caller's arrays are only read through this table (leaf_lookup, leaf_eval)
    c->dev.bk = PosTable{(uint32_t *)meta, (uint64_t *)keys, (float *)val, (float *)pol, (uint32_t)(cap - 1)};
    c->dev.bk_stones = max_stones;
    return YY_OK;
}

// ---- shared evaluation table (MctsDev.sh)
extern "C" int yy_mcts_set_shared_evaluations(yy_mcts *c, uint32_t *meta, uint64_t *keys, float *val, float *pol, int64_t slots,
                                              uint32_t *stamp) {
    if (!c) return set_err(YY_E_INVALID, "null pointer%s%s");
    // a pending leaf may name a slot of the table that is set now (GameState.leaf_src)
    if (c->pending != 0) return set_err(YY_E_STATE, "yy_mcts_set_shared_evaluations with a select or a root expansion pending%s%s");
    if (!meta) {
        c->dev.sh = PosTable{};
        c->dev.sh_stamp = nullptr;
        c->dev.sh_claim = nullptr;
        c->dev.sh_hit = nullptr;
        c->dev.sh_sweep = nullptr;
        return YY_OK;
    }
    if (c->cfg.flags & YY_FLAG_ALIASED)
        return set_err(YY_E_UNSUPPORTED, "yy_mcts_set_shared_evaluations needs copied boards (YY_FLAG_ALIASED reproduces the reference, which asks the network for every leaf)%s%s");
    if (c->multi.K > 1)
        return set_err(YY_E_UNSUPPORTED, "yy_mcts_set_shared_evaluations: leaves_per_step > 1 does not support evaluation reuse%s%s");
    if (!keys || !val || !pol || !stamp || slots < 64 || (slots & (slots - 1)) || slots > (1ll << 30))
        return set_err(YY_E_INVALID, "yy_mcts_set_shared_evaluations: bad argument (slots must be a power of two in 64 .. 2^30)%s%s");
    c->dev.sh = PosTable{meta, keys, val, pol, (uint32_t)(slots - 1)};
    c->dev.sh_stamp = stamp;
    c->dev.sh_claim = nullptr;
    c->dev.sh_hit = nullptr;
    c->dev.sh_sweep = nullptr;
    return YY_OK;
}

// The replacing table: the insert-only setter's checks and state, then the claim words in the place of meta (MctsDev.sh_claim)
extern "C" int yy_mcts_set_shared_evaluations_replacing(yy_mcts *c, uint64_t *claim, uint32_t *last_hit, uint64_t *keys, float *val,
                                                        float *pol, int64_t slots, uint32_t *stamp, uint64_t *sweep_state) {
    if (c && claim && (!last_hit || !sweep_state))
        return set_err(YY_E_INVALID, "yy_mcts_set_shared_evaluations_replacing: bad argument (last_hit and sweep_state are needed)%s%s");
    if (int e = yy_mcts_set_shared_evaluations(c, (uint32_t *)claim, keys, val, pol, slots, stamp)) return e;
    if (!claim) return YY_OK;
    c->dev.sh_claim = (unsigned long long *)claim;
    c->dev.sh_hit = last_hit;
    c->dev.sh_sweep = (unsigned long long *)sweep_state;
    return YY_OK;
}

// hits, inserts, dropped (, duplicates): out[0 .. n)
static int shared_counters(yy_mcts *c, uint64_t *out, int n) {
    if (!c || !out) return set_err(YY_E_INVALID, "null pointer%s%s");
    uint64_t h[TC_COUNT + 1];
    if (int e = tree_counters(c, false, h)) return e;
    for (int i = 0; i < n; i++) out[i] = h[TC_SH_HITS + i];
    return YY_OK;
}

extern "C" int yy_mcts_shared_counters_ex(yy_mcts *c, uint64_t *out) {
    if (int e = shared_counters(c, out, 4)) return e;
    out[4] = out[5] = 0;
    if (c->dev.sh_sweep) {
        uint64_t sw[SH_SWEEP_WORDS];
        HIP_TRY(hipMemcpy(sw, c->dev.sh_sweep, sizeof sw, hipMemcpyDeviceToHost));
        out[4] = sw[SH_SW_EVICTED];
        out[5] = sw[SH_SW_LIVE];
    }
    return YY_OK;
}

extern "C" int yy_mcts_shared_counters(yy_mcts *c, uint64_t *out) { return shared_counters(c, out, 3); }

extern "C" int yy_mcts_shared_evaluations_clear(yy_mcts *c, yy_stream_t s) {
    if (!c) return set_err(YY_E_INVALID, "null pointer%s%s");
    // a pending leaf may name a slot (GameState.leaf_src): emptied, another game could claim and rewrite it in the launch that reads it
    if (c->pending != 0) return set_err(YY_E_STATE, "yy_mcts_shared_evaluations_clear with a select or a root expansion pending%s%s");
    const PosTable &sh = c->dev.sh;
    // replacing mode: sh.meta names the claim words, eight bytes a slot; the sweeps start over (live, cutoff), the count of
    // evicted entries goes on
    const size_t word = c->dev.sh_claim ? sizeof(uint64_t) : sizeof(uint32_t);
    if (sh.meta) HIP_TRY(hipMemsetAsync(sh.meta, 0, ((size_t)sh.mask + 1) * word, (hipStream_t)s));
    if (c->dev.sh_sweep) {
        HIP_TRY(hipMemsetAsync(c->dev.sh_sweep + SH_SW_LIVE, 0, sizeof(uint64_t), (hipStream_t)s));
        HIP_TRY(hipMemsetAsync(c->dev.sh_sweep + SH_SW_CUTOFF, 0, sizeof(uint64_t), (hipStream_t)s));
    }
    return YY_OK;
}

extern "C" int yy_mcts_cache_clear(yy_mcts *c, yy_stream_t s) {
    if (!c) return set_err(YY_E_INVALID, "null pointer%s%s");
    const PosTable &ec = c->dev.ec;
    if (ec.meta) HIP_TRY(hipMemsetAsync(ec.meta, 0, (size_t)c->cfg.G * ((size_t)ec.mask + 1) * sizeof(uint32_t), (hipStream_t)s));
    return YY_OK;
}

extern "C" int yy_mcts_reset_counters(yy_mcts *c, yy_stream_t s) {
    if (!c) return set_err(YY_E_INVALID, "null pointer%s%s");
    hipLaunchKernelGGL(k_reset_counters, dim3((c->cfg.G + 255) / 256), dim3(256), 0, (hipStream_t)s, c->dev);
    HIP_TRY(hipGetLastError());
    return YY_OK;
}
