// yy_tower.hip -- the policy/value CNN's residual tower as ONE LDS-resident MFMA kernel (gfx950), bf16 storage / f32
// accumulation, in two forms that share every sequence below and return the same bits.
//
// Reference computation: YinYangNeuralNetwork.forward, stem + residual blocks
// (src/yin_yang/ai/neural_network.py:16-33, 94-110) at eval time with BatchNorm folded into the
// convolutions, on 6x6, 8x8 or 12x12 boards with 128 channels.
//
// MI355X design.  A 3x3 convolution never looks outside its board, so the whole tower of a board can run inside one
// workgroup with no inter-workgroup dependency:
//   * workgroup = 4 waves = TB boards; their TB*R*R (board, cell) pairs are the MFMA columns, 32 to a column tile (a tile
//     may straddle boards; every column keeps its own board for the 3x3 neighbourhood);
//   * the activations [column][128 ch] bf16 live in LDS for ALL layers (rows padded by 16 B so ds_read_b128 fragment
//     reads are conflict-free and use immediate offsets); they never touch HBM;
//   * each layer is an implicit GEMM  D[cout][col] = sum_{tap,cin} W[cout][tap,cin] * X[cin][col+tap]
//     on v_mfma_f32_32x32x16_bf16 (weights = A operand, shifted activations = B operand; out-of-board taps read a zero
//     row); a wave accumulates CT column tiles x NT weight tiles, then applies bias, residual (kept packed in registers)
//     and ReLU and writes bf16 back to LDS;
//   * weights stream L2 -> LDS with global_load_lds_dwordx4 through a ring of 16 KB chunks (one chunk = one tap x 64
//     input channels, pre-packed on the host in fragment order), counted s_waitcnt vmcnt, NSLOT - 1 chunks in flight;
//   * LDS: activations + ring + 11.5 KB bias table + zero row -> 1 workgroup/CU, one wave per SIMD with the whole
//     register file.
//
// k_tower: 8x8, wave = board.  4 boards per workgroup, wave w owns the 64 columns (2 tiles) of board w and all 128
//     output channels (4 weight tiles): 6 fragment reads per 8 MFMAs.  The kernel for G > 512.
// k_towerq<R, TB>: wave = output-channel quarter.  Wave w owns couts [32w, 32w+32) for ALL CT = TB*R*R/32 column tiles:
//     CT + 1 reads per CT MFMAs.
//   <6, 8>  6x6: 8 boards = 288 columns = 9 tiles; 9 accumulators (144 registers) + packed residual (72).
//   <12, 2> 12x12: two boards = 9 full tiles, the same shape as <6, 8>.
//   <8, 1>  8x8, one or two boards per workgroup: the low-latency forms for small batches (arena matches, single-board
//   <8, 2>  MCTS.search, a few hundred concurrent games), where k_tower's grid leaves most CUs idle and a step costs one
//           full workgroup latency whatever G is.  A quarter of the MFMA work per wave, more LDS reads per MFMA (1.5 /
//           1.25 instead of 0.75) -- the right trade only while the chip is not full.
//
// What the two forms do NOT share, on purpose:
//   * the dimension a wave owns: a board's columns (k_tower: <CT, NT> = <2, 4>) or a quarter of the output channels
//     (k_towerq: <CT, 1>).  The accumulation order of every output element is the same, hence the same bits.
//   * ring discipline and depth.  k_tower's waves all read the whole chunk: shared ring, 5 slots, 4 chunks in flight,
//     counted vmcnt + s_barrier per chunk.  k_towerq's chunk layout [ks 4][nt 4][1 KB] and issue_chunk's piece order
//     make wave w load exactly the pieces (nt == w) it reads itself: wave-private ring, 4 slots, 3 in flight, the
//     counted vmcnt is all a chunk needs.
//   * barriers around the k_towerq epilogue: its waves read every input channel of every column, so a layer's input
//     must be read by all before any wave overwrites it, and written by all before the next layer starts.  k_tower's
//     epilogue is wave-private (a wave reads and writes only its own board's cells).
//   * bias fetch batching: the epilogue fetches the bias vectors of two weight tiles at a time, back to back -- two
//     batches of 8 in k_tower (16 at once would cost registers), all 4 up front in k_towerq.
//   * head work split: a k_tower wave runs both 1x1 heads on its own board (2 tiles x 2 heads) and stages the result in
//     its own, now dead, activation rows; a k_towerq wave runs head (w & 1) on half of the column tiles, and the
//     workgroup stages in the global layout from the start of LDS, behind one more barrier.
//   * LDS size: k_tower claims the CU's whole 160 KB, k_towerq what its layout needs (both: one workgroup per CU).
// Roofline: MFMA (bf16 dense 2.5 PFLOP/s).  Algorithmic FLOPs per board: 2*9*16*128*R*R (stem, K padded to 16)
// + (layers-1) * 2*9*128*128*R*R (+ 2*128*64*R*R for the heads).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/yy_engine.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(2))) short s16x2;

#define TW_CH 128
#define TW_ROW_BYTES 272           // 256 B of channels + 16 B pad: consecutive columns land on consecutive 16-B bank slots
#define TW_CHUNK_BYTES 16384       // [ks 4][ntile 4][h 2][c 32][j 8] bf16
#define TW_MAX_LAYERS 23
#define YY_TOWER_TB1_MAX_G 256     // <= one 1-board workgroup per CU
#define YY_TOWER_TB2_MAX_G 512     // <= one 2-board workgroup per CU

#include "yy_common.h"

namespace tw {

// LDS layout: activations | weight ring | bias table | 256 B of zeros
template <int NCOL_, int NSLOT_> struct Lds {
    static constexpr int NCOL = NCOL_, NSLOT = NSLOT_;
    static constexpr int RING_OFF = NCOL * TW_ROW_BYTES;
    static constexpr int BIAS_OFF = RING_OFF + NSLOT * TW_CHUNK_BYTES;
    static constexpr int ZERO_OFF = BIAS_OFF + TW_MAX_LAYERS * TW_CH * 4;
    static constexpr int LDS_BYTES = ZERO_OFF + 256;
};
// The two forms (see the head of the file).  CT x NT: column tiles x weight tiles of a wave, the wave's first column and
// weight tile; HT x HN: the same for the 1x1 heads; STG_STRIDE: distance of two boards in the heads' staging area.
struct BoardWaves : Lds<256, 5> {
    static constexpr int R = 8, CELLS = 64, TB = 4, CT = 2, NT = 4, HT = 2, HN = 2;
    static constexpr bool SHARED_RING = true;
    static constexpr int STG_STRIDE = CELLS * TW_ROW_BYTES, LDS_BYTES = 160 * 1024;
    static_assert(LDS_BYTES >= Lds<256, 5>::LDS_BYTES, "layout must fit");
    static __device__ __forceinline__ int col0(int wave) { return wave * CELLS; }
    static __device__ __forceinline__ int nt0(int) { return 0; }
};
template <int R_, int TB_> struct QuarterWaves : Lds<TB_ * R_ * R_, 4> {
    static constexpr int R = R_, CELLS = R_ * R_, TB = TB_, CT = TB_ * R_ * R_ / 32, NT = 1, HT = (CT + 1) / 2, HN = 1;
    static_assert(TB_ * R_ * R_ % 32 == 0, "columns must fill whole MFMA tiles");
    static constexpr bool SHARED_RING = false;
    static constexpr int STG_STRIDE = 2 * 32 * CELLS * 2;
    static __device__ __forceinline__ int col0(int) { return 0; }
    static __device__ __forceinline__ int nt0(int wave) { return wave; }
};

__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
    bf16x2 t;
    t[0] = (__bf16)a;
    t[1] = (__bf16)b;
    return __builtin_bit_cast(uint32_t, t);
}
__device__ __forceinline__ uint32_t cvt_pk(f32x2 v) {   // ONE v_cvt_pk_bf16_f32
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ uint32_t relu_pk(uint32_t p) {   // max(x, 0) on two packed bf16 as signed int16
    const s16x2 z = {0, 0};
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, p), z));
}
__device__ __forceinline__ float bf_lo(uint32_t p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float bf_hi(uint32_t p) { return __uint_as_float(p & 0xFFFF0000u); }
// byte offset of the 16-B slot holding channels [8*chunk, 8*chunk+8) of column col = board_in_workgroup * CELLS + cell
__device__ __forceinline__ uint32_t act_off(int col, int chunk) { return (uint32_t)(col * TW_ROW_BYTES + chunk * 16); }
__device__ __forceinline__ void lds_sync() {   // LDS traffic of every wave done and visible to the workgroup
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// every thread moves 4 x 16 B of a 16 KB chunk: global (fragment order) -> LDS ring slot, no VGPR data
template <class F>
__device__ __forceinline__ void issue_chunk(const unsigned char *wchunk, unsigned char *lds, int slot, int wave, int lane) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int piece = (r * 4 + wave) * 1024;   // wave-uniform 1 KiB piece
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(wchunk + piece + lane * 16),
                                         (__attribute__((address_space(3))) void *)(lds + F::RING_OFF + slot * TW_CHUNK_BYTES + piece),
                                         16, 0, 0);
    }
}

// fragments of one k-step (16 input channels of one tap): CT activation tiles + NT weight tiles, CT + NT ds_read_b128
template <int CT, int NT> struct Frags {
    bf16x8 x[CT], w[NT];
};
template <class F>
__device__ __forceinline__ void load_frags(Frags<F::CT, F::NT> &f, const unsigned char *lds, int slot, int half, int ks,
                                           const uint32_t (&cbase)[F::CT], int nt0, int lane) {
    const int h = lane >> 5, c = lane & 31;
    // cbase already contains this lane's h*16; (half, ks) are compile-time after unrolling -> immediate offsets
    const unsigned char *wslot = lds + F::RING_OFF + slot * TW_CHUNK_BYTES + (h * 32 + c) * 16 + ks * 4096 + nt0 * 1024;
#pragma unroll
    for (int tt = 0; tt < F::CT; tt++)
        f.x[tt] = __builtin_bit_cast(bf16x8, *(const u32x4 *)(lds + cbase[tt] + half * 128 + ks * 32));
#pragma unroll
    for (int nt = 0; nt < F::NT; nt++) f.w[nt] = __builtin_bit_cast(bf16x8, *(const u32x4 *)(wslot + nt * 1024));
}
// ZERO: first k-step of an accumulation, C = 0 (inline constant), no accumulator initialisation
template <int CT, int NT, bool ZERO> __device__ __forceinline__ void mma_step(f32x16 (&acc)[CT][NT], const Frags<CT, NT> &f) {
    const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tt = 0; tt < CT; tt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
            acc[tt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.w[nt], f.x[tt], ZERO ? z : acc[tt][nt], 0, 0, 0);
}
// issue order hint: the CT + NT LDS reads of the NEXT k-step inside the CT * NT MFMAs of this one, as (1 MFMA + 2 reads)
// groups, then the odd read, then the MFMAs left, which cover the last reads' latency
template <int CT, int NT> __device__ __forceinline__ void interleave_hint() {
    constexpr int NR = CT + NT, PAIRS = NR / 2, ODD = NR & 1, REST = CT * NT - PAIRS - ODD;
#pragma unroll
    for (int j = 0; j < PAIRS; j++) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // 1 MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // 2 DS reads
    }
    if (ODD) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    if (REST > 0) __builtin_amdgcn_sched_group_barrier(0x008, REST, 0);
}

// Per-lane geometry, computed ONCE per kernel: this lane's column in tile tt is col = col0 + tt*32 + c = board*CELLS + cell,
// its tap neighbour is column col + dy*R + dx.  rowbase = LDS offset of the column's own row (+ this lane's h*16), okmask =
// 9-bit mask of the taps whose neighbour is on the board, zbase = the zero row.  The per-chunk tap geometry is then four
// full-rate VALU ops per tile (and, compare, add a wave-uniform shift, select).
template <int CT> struct LaneGeo {
    uint32_t rowbase[CT], okmask[CT], zbase;
};
template <class F> __device__ __forceinline__ void make_lane_geo(LaneGeo<F::CT> &g, int col0, int c, int h) {
    g.zbase = (uint32_t)F::ZERO_OFF + (uint32_t)(h * 16);
#pragma unroll
    for (int tt = 0; tt < F::CT; tt++) {
        const int col = col0 + tt * 32 + c;
        const int cell = col % F::CELLS;
        const int y = cell / F::R, x = cell - y * F::R;
        g.rowbase[tt] = (uint32_t)(col * TW_ROW_BYTES) + (uint32_t)(h * 16);
        uint32_t m = 0;
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const int sy = y + tap / 3 - 1, sx = x + tap % 3 - 1;
            if (((unsigned)sy < (unsigned)F::R) && ((unsigned)sx < (unsigned)F::R)) m |= 1u << tap;
        }
        g.okmask[tt] = m;
    }
}
// LDS row base of the tap's neighbour column for each of this lane's columns (the zero row when off-board); `tap` is wave-uniform
template <class F> __device__ __forceinline__ void tap_geo(int tap, const LaneGeo<F::CT> &g, uint32_t (&cbase)[F::CT]) {
    const int shift = ((tap / 3 - 1) * F::R + (tap % 3 - 1)) * TW_ROW_BYTES;   // scalar unit
    const uint32_t bit = 1u << tap;
#pragma unroll
    for (int tt = 0; tt < F::CT; tt++) cbase[tt] = (g.okmask[tt] & bit) ? g.rowbase[tt] + (uint32_t)shift : g.zbase;
}

// The ring: NSLOT - 1 chunks in flight, 4 loads per thread and chunk, hence the counted waits.
__device__ __forceinline__ void wait_chunk(int younger) {   // all but the `younger` youngest chunks have landed
    if (younger >= 3) wait_vmcnt<12>();
    else if (younger == 2) wait_vmcnt<8>();
    else if (younger == 1) wait_vmcnt<4>();
    else wait_vmcnt<0>();
}
template <class F>
__device__ __forceinline__ void prime_ring(unsigned char *lds, const unsigned char *weights, int n_chunks, int wave, int lane) {
    constexpr int DIST = F::NSLOT - 1;
#pragma unroll
    for (int pc = 0; pc < DIST; pc++)
        if (pc < n_chunks) issue_chunk<F>(weights + (size_t)pc * TW_CHUNK_BYTES, lds, pc % F::NSLOT, wave, lane);
    wait_chunk(n_chunks >= DIST ? DIST - 1 : 0);   // chunk 0 has landed
    if constexpr (F::SHARED_RING) {                   // ... for every wave
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
}
// Top of chunk `chunk` (the i-th of its layer): make chunk+1 available, refill the slot chunk-1 used.
template <class F>
__device__ __forceinline__ void advance_ring(unsigned char *lds, const unsigned char *weights, int i, int chunk, int n_chunks,
                                             int wave, int lane) {
    constexpr int DIST = F::NSLOT - 1;
    if (chunk + 1 < n_chunks) {
        wait_chunk(min(DIST - 2, n_chunks - 2 - chunk));   // chunks younger than chunk+1 may stay in flight
        if constexpr (F::SHARED_RING) {
            __builtin_amdgcn_s_barrier();   // chunk+1 landed everywhere; everyone finished chunk-1
            asm volatile("" ::: "memory");
        }
    }
    // Private ring: no barrier per chunk.  Barriers remain where the waves exchange activations: at the start of a layer
    // (the previous layer's epilogue, or the prologue, is visible to every wave) and before its epilogue.
    if constexpr (!F::SHARED_RING)
        if (i == 0) lds_sync();
    if (chunk + DIST < n_chunks)
        issue_chunk<F>(weights + (size_t)(chunk + DIST) * TW_CHUNK_BYTES, lds, (chunk + DIST) % F::NSLOT, wave, lane);
}

// One layer's chunks: KS k-steps per chunk whose LDS reads are software-pipelined one k-step ahead, across the chunk
// boundary too (only the first k-step of a layer exposes its read latency).  Shared ring: chunk `chunk` is visible to every
// wave on entry and exit of every iteration, so the layer's first fragments are read ahead of the first barrier; private
// ring: they are another wave's output and are read behind the layer-start barrier.
template <class F, int KS>
__device__ __forceinline__ void run_layer(f32x16 (&acc)[F::CT][F::NT], unsigned char *lds, const unsigned char *weights, int &chunk,
                                          int n_chunks, const LaneGeo<F::CT> &geo, int wave, int lane) {
    constexpr int NCH = (KS == 1) ? 9 : 18, CT = F::CT, NT = F::NT;
    const int nt0 = F::nt0(wave);
    uint32_t cb[CT];
    tap_geo<F>(0, geo, cb);
    Frags<CT, NT> cur;
    if constexpr (F::SHARED_RING) load_frags<F>(cur, lds, chunk % F::NSLOT, 0, 0, cb, nt0, lane);
    for (int i = 0; i < NCH; i++, chunk++) {
        const int half = (KS == 1) ? 0 : (i & 1);
        advance_ring<F>(lds, weights, i, chunk, n_chunks, wave, lane);
        if constexpr (!F::SHARED_RING)
            if (i == 0) load_frags<F>(cur, lds, chunk % F::NSLOT, 0, 0, cb, nt0, lane);
        const bool last = (i == NCH - 1);
        uint32_t ncb[CT];
        const int ni = last ? i : i + 1;
        tap_geo<F>((KS == 1) ? ni : (ni >> 1), geo, ncb);
        const int nhalf = (KS == 1) ? 0 : (ni & 1);
#pragma unroll
        for (int ks = 0; ks < KS; ks++) {
            Frags<CT, NT> nxt;
            const bool has_next = (ks + 1 < KS) || !last;
            if (ks + 1 < KS) load_frags<F>(nxt, lds, chunk % F::NSLOT, half, ks + 1, cb, nt0, lane);
            else if (!last) load_frags<F>(nxt, lds, (chunk + 1) % F::NSLOT, nhalf, 0, ncb, nt0, lane);
            if (i == 0 && ks == 0) mma_step<CT, NT, true>(acc, cur);
            else mma_step<CT, NT, false>(acc, cur);
            if (has_next) {
                interleave_hint<CT, NT>();
                cur = nxt;
            }
        }
#pragma unroll
        for (int tt = 0; tt < CT; tt++) cb[tt] = ncb[tt];
    }
}

// Layer epilogue of the lane's 4 couts x 1 column of accumulator quad q of one tile (couts nt*32 + 8q + 4h + i): + bias
// (+ residual), bf16 rounding of each pair, ReLU on the packed pair (v_pk_max_i16: bf16 is
// sign-magnitude), keep the result packed for the skip connection, 8-byte store to the column's activation row.
template <bool RES>
__device__ __forceinline__ void epilogue_quad(const f32x16 &a, int q, f32x4 b, uint32_t (&res)[2], bool keep, unsigned char *dst) {
    f32x2 v01 = {a[4 * q + 0] + b[0], a[4 * q + 1] + b[1]};
    f32x2 v23 = {a[4 * q + 2] + b[2], a[4 * q + 3] + b[3]};
    if constexpr (RES) {
        v01 += (f32x2){bf_lo(res[0]), bf_hi(res[0])};
        v23 += (f32x2){bf_lo(res[1]), bf_hi(res[1])};
    }
    const uint32_t p0 = relu_pk(cvt_pk(v01)), p1 = relu_pk(cvt_pk(v23));
    if (keep) {
        res[0] = p0;
        res[1] = p1;
    }
    const u32x2 pk = {p0, p1};
    *(u32x2 *)dst = pk;
}
// No MFMA runs in the epilogue, so every stall is paid in full: the bias vectors of two weight tiles are fetched back to
// back (one LDS latency per batch instead of one per vector), and the residual branch is resolved once per layer (RES).
template <class F, bool RES>
__device__ __forceinline__ void layer_epilogue(const f32x16 (&acc)[F::CT][F::NT], uint32_t (&res)[F::CT][F::NT][4][2], unsigned char *lds,
                                               int L, bool keep, int wave, int lane) {
    constexpr int NB = F::NT < 2 ? F::NT : 2;
    const int h = lane >> 5, c = lane & 31, nt0 = F::nt0(wave), col0 = F::col0(wave);
    const unsigned char *bl = lds + F::BIAS_OFF + (L * TW_CH + nt0 * 32 + 4 * h) * 4;
    unsigned char *dst = lds + act_off(col0 + c, nt0 * 4) + h * 8;   // the lane's 8 bytes of (tile 0, quad 0); the rest are immediates
#pragma unroll
    for (int ntb = 0; ntb < F::NT; ntb += NB) {
        f32x4 b[NB][4];
#pragma unroll
        for (int n2 = 0; n2 < NB; n2++)
#pragma unroll
            for (int q = 0; q < 4; q++) b[n2][q] = *(const f32x4 *)(bl + ((ntb + n2) * 32 + 8 * q) * 4);
#pragma unroll
        for (int n2 = 0; n2 < NB; n2++) {
            const int nt = ntb + n2;
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int tt = 0; tt < F::CT; tt++)
                    epilogue_quad<RES>(acc[tt][nt], q, b[n2][q], res[tt][nt][q], keep, dst + act_off(tt * 32, nt * 4 + q));
        }
    }
}

// Head bias + ReLU + bf16 of accumulator quad q of one (column tile, head): -> staging [channel 32][cell CELLS] of the
// column's board and head (the reference's NCHW flatten order, neural_network.py:114/:119)
template <int CELLS>
__device__ __forceinline__ void stage_head_quad(const f32x16 &a, int q, f32x4 b, unsigned char *stg, int cell, int h) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float v = fmaxf(a[4 * q + i] + b[i], 0.0f);
        const int ch = 8 * q + 4 * h + i;
        *(unsigned short *)(stg + (ch * CELLS + cell) * 2) = (unsigned short)(pack_bf16(v, 0.0f) & 0xFFFFu);
    }
}

// weights: bf16 chunks [9 + 18*(n_layers-1) (+1 head chunk)][8192] in fragment order (network.pack_tower);
// bias f32 [n_layers (+1)][128]; planes f32 [G,5,R,R]; out bf16 [G,R,R,128] or out_heads bf16 [G,2,32,R*R].
template <class F>
__device__ __forceinline__ void tower(const float *__restrict__ planes, const unsigned char *__restrict__ weights,
                                      const float *__restrict__ bias, unsigned short *__restrict__ out,
                                      unsigned short *__restrict__ out_heads, int G, int n_layers) {
    constexpr int CT = F::CT, NT = F::NT, CELLS = F::CELLS, NCOL = F::NCOL;
    __shared__ __attribute__((aligned(16))) unsigned char lds[F::LDS_BYTES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g0 = blockIdx.x * F::TB;                     // first board of the workgroup
    const int h = lane >> 5, c = lane & 31;
    const int col0 = F::col0(wave);

    // ---- prologue: bias table + zero row + input planes -> LDS (ordinary loads, drained before the ring starts)
    for (int i = threadIdx.x; i < (n_layers + (out_heads ? 1 : 0)) * TW_CH; i += 256)
        ((float *)(lds + F::BIAS_OFF))[i] = bias[i];
    if (threadIdx.x < 64) ((uint32_t *)(lds + F::ZERO_OFF))[threadIdx.x] = 0u;
    for (int col = threadIdx.x; col < NCOL; col += 256) {
        // 5 planes (neural_network.py:156-196) -> channels 0..4 of a 16-channel input, rest zero
        const int gb = g0 + col / CELLS, cell = col % CELLS;
        float p[5];
#pragma unroll
        for (int k = 0; k < 5; k++) p[k] = (gb < G) ? planes[((size_t)gb * 5 + k) * CELLS + cell] : 0.0f;
        u32x4 v0 = {pack_bf16(p[0], p[1]), pack_bf16(p[2], p[3]), pack_bf16(p[4], 0.0f), 0u};
        u32x4 z = {0u, 0u, 0u, 0u};
        *(u32x4 *)(lds + act_off(col, 0)) = v0;
        *(u32x4 *)(lds + act_off(col, 1)) = z;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

    // the policy/value 1x1 head convolutions ride the same ring as one extra 16 KB chunk after the tower
    const int n_chunks = 9 + 18 * (n_layers - 1) + (out_heads ? 1 : 0);
    prime_ring<F>(lds, weights, n_chunks, wave, lane);

    LaneGeo<CT> geo;
    make_lane_geo<F>(geo, col0, c, h);
    uint32_t res[CT][NT][4][2];   // residual x, packed bf16 in the accumulator layout
    int chunk = 0;
    for (int L = 0; L < n_layers; L++) {
        f32x16 acc[CT][NT];
        if (L == 0) run_layer<F, 1>(acc, lds, weights, chunk, n_chunks, geo, wave, lane);
        else run_layer<F, 4>(acc, lds, weights, chunk, n_chunks, geo, wave, lane);
        if constexpr (!F::SHARED_RING) lds_sync();        // every wave has finished reading this layer's input
        const bool conv2 = (L >= 2) && ((L & 1) == 0);   // second conv of a block: + residual
        const bool keep = (L == 0) || conv2;             // output is a block input x: keep it for the skip
        if (conv2) layer_epilogue<F, true>(acc, res, lds, L, keep, wave, lane);
        else layer_epilogue<F, false>(acc, res, lds, L, keep, wave, lane);
        if constexpr (F::SHARED_RING) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    // what follows reads other waves' columns, except the head convolutions of a wave that owns its board
    if (!F::SHARED_RING || !out_heads) lds_sync();
    if (out_heads) {
        // ---- policy_conv / value_conv (1x1, 128 -> 32 each; neural_network.py:59-60, 65-66, 113, 118) + bias + ReLU
        // chunk layout [ks 8][nt 2][h 2][c 32][j 8]: nt 0 = policy channels, nt 1 = value channels.  The wave runs heads
        // [head0, head0 + HN) on up to HT column tiles from tile t0 of its columns (k_towerq: the first HT tiles for
        // w < 2, the remaining CT - HT for the others; a surplus tile is a duplicate, never stored).
        constexpr int HT = F::HT, HN = F::HN;
        const int head0 = (HN == 2) ? 0 : (wave & 1), t0 = (HN == 2) ? 0 : (wave >> 1) * HT;
        const int nt_cnt = (HN == 2 || (wave >> 1) == 0) ? HT : CT - HT;
        const unsigned char *hw = lds + F::RING_OFF + (chunk % F::NSLOT) * TW_CHUNK_BYTES + (h * 32 + c) * 16 + head0 * 1024;
        uint32_t xb[HT];
#pragma unroll
        for (int t = 0; t < HT; t++) xb[t] = act_off(min(col0 + (t0 + t) * 32 + c, NCOL - 1), 0) + h * 16;
        f32x16 hacc[HT][HN];
#pragma unroll
        for (int ks = 0; ks < 8; ks++) {
            Frags<HT, HN> f;
#pragma unroll
            for (int t = 0; t < HT; t++) f.x[t] = __builtin_bit_cast(bf16x8, *(const u32x4 *)(lds + xb[t] + ks * 32));
#pragma unroll
            for (int n = 0; n < HN; n++) f.w[n] = __builtin_bit_cast(bf16x8, *(const u32x4 *)(hw + (ks * 2 + n) * 1024));
            if (ks == 0) mma_step<HT, HN, true>(hacc, f);
            else mma_step<HT, HN, false>(hacc, f);
        }
        // k_tower stages in the wave's own (now dead) activation rows; k_towerq from the start of LDS, in the global layout
        // of these boards, once everyone has read the activations
        if constexpr (F::SHARED_RING) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        else lds_sync();
#pragma unroll
        for (int n = 0; n < HN; n++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const f32x4 b = *(const f32x4 *)(lds + F::BIAS_OFF + (n_layers * TW_CH + (head0 + n) * 32 + 8 * q + 4 * h) * 4);
#pragma unroll
                for (int t = 0; t < HT; t++)
                    if (t < nt_cnt) {
                        const int col = col0 + (t0 + t) * 32 + c, bd = col / CELLS, cell = col % CELLS;
                        stage_head_quad<CELLS>(hacc[t][n], q, b, lds + bd * F::STG_STRIDE + (head0 + n) * 32 * CELLS * 2, cell, h);
                    }
            }
        lds_sync();
        constexpr int PER_BOARD = 2 * 32 * CELLS * 2;      // 4608 B at 6x6, 8192 B at 8x8
        for (int p = threadIdx.x; p < F::TB * PER_BOARD / 16; p += 256) {
            const int bd = (p * 16) / PER_BOARD;
            if (g0 + bd < G)
                *(u32x4 *)((unsigned char *)out_heads + (size_t)g0 * PER_BOARD + (size_t)p * 16) =
                    *(const u32x4 *)(lds + p * 16 + bd * (F::STG_STRIDE - PER_BOARD));
        }
        return;
    }
    // ---- final activations -> HBM, [board][cell][128] bf16 (channels-last), 1 KiB per wave store
    for (int p = threadIdx.x; p < NCOL * 16; p += 256) {
        const int col = p >> 4, ch = p & 15;
        if (g0 + col / CELLS < G)
            *(u32x4 *)(out + ((size_t)g0 * CELLS + col) * TW_CH + ch * 8) = *(const u32x4 *)(lds + act_off(col, ch));
    }
}

#define TOWER_ARGS                                                                                                     \
    const float *__restrict__ planes, const unsigned char *__restrict__ weights, const float *__restrict__ bias,      \
        unsigned short *__restrict__ out, unsigned short *__restrict__ out_heads, int G, int n_layers

__global__ void __launch_bounds__(256, 1) k_tower(TOWER_ARGS) {
    tower<BoardWaves>(planes, weights, bias, out, out_heads, G, n_layers);
}
template <int R, int TB> __global__ void __launch_bounds__(256, 1) k_towerq(TOWER_ARGS) {
    tower<QuarterWaves<R, TB>>(planes, weights, bias, out, out_heads, G, n_layers);
}

}   // namespace tw

template <auto KERNEL, int TB>
static int launch(const float *planes, const void *weights, const float *bias, void *out, void *out_heads, int G, int n_layers,
                  yy_stream_t s) {
    KERNEL<<<dim3((G + TB - 1) / TB), dim3(256), 0, (hipStream_t)s>>>(planes, (const unsigned char *)weights, bias, (unsigned short *)out,
                                                                     (unsigned short *)out_heads, G, n_layers);
    if (hipGetLastError() != hipSuccess) return yy_tower_set_err(YY_E_HIP, "yy_nn_tower: launch failed");
    return YY_OK;
}

static int launch_tower(const float *planes, const void *weights, const float *bias, void *out, void *out_heads, int G,
                        int R, int C, int channels, int n_layers, yy_stream_t s) {
    if (G == 0) return YY_OK;
    if (!planes || !weights || !bias || (!out && !out_heads) || G < 0)
        return yy_tower_set_err(YY_E_INVALID, "yy_nn_tower: bad argument");
    const bool b8 = (R == 8 && C == 8), b12 = (R == 12 && C == 12), b6 = (R == 6 && C == 6);
    if (!(b8 || b12 || b6) || channels != TW_CH || n_layers < 1 || n_layers + (out_heads ? 1 : 0) > TW_MAX_LAYERS || (n_layers & 1) == 0)
        return yy_tower_set_err(YY_E_UNSUPPORTED, "yy_nn_tower: needs 6x6, 8x8 or 12x12 boards, 128 channels, at most 10 residual blocks");
    if (b12) return launch<tw::k_towerq<12, 2>, 2>(planes, weights, bias, out, out_heads, G, n_layers, s);
    if (b6) return launch<tw::k_towerq<6, 8>, 8>(planes, weights, bias, out, out_heads, G, n_layers, s);
    // small batches: 4 boards per workgroup would leave most of the 256 CUs idle; spread the boards over more, lighter
    // workgroups (same results bit for bit)
    if (G <= YY_TOWER_TB1_MAX_G) return launch<tw::k_towerq<8, 1>, 1>(planes, weights, bias, out, out_heads, G, n_layers, s);
    if (G <= YY_TOWER_TB2_MAX_G) return launch<tw::k_towerq<8, 2>, 2>(planes, weights, bias, out, out_heads, G, n_layers, s);
    return launch<tw::k_tower, 4>(planes, weights, bias, out, out_heads, G, n_layers, s);
}

extern "C" int yy_nn_tower_bf16(const float *planes, const void *weights, const float *bias, void *out, int G, int R,
                                int C, int channels, int n_layers, yy_stream_t s) {
    return launch_tower(planes, weights, bias, out, nullptr, G, R, C, channels, n_layers, s);
}

extern "C" int yy_nn_tower_heads_bf16(const float *planes, const void *weights, const float *bias, void *out_heads, int G,
                                      int R, int C, int channels, int n_layers, yy_stream_t s) {
    return launch_tower(planes, weights, bias, nullptr, out_heads, G, R, C, channels, n_layers, s);
}
