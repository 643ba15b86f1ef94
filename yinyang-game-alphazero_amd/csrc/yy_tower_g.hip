// yy_tower_g.hip -- the split-f16 (float32-accurate) evaluator tower, GENERAL form: any R x C board with at most 144 cells,
// 32 / 64 / 96 / 128 channels, any number of residual blocks up to 10 (train_alphazero.py:35-36 takes any --rows / --cols,
// ai/neural_network.py:39 any num_channels / num_res_blocks).  Evaluator mode "f16x3" (network.BatchedEvaluator).
//
// Reference computation: YinYangNeuralNetwork.forward, stem + residual blocks + the two 1x1 head convolutions
// (src/yin_yang/ai/neural_network.py:16-33, 94-119), float32 on the CPU.  Numerics as in yy_tower_h3.hip: every activation
// x and weight w is a PAIR of float16 numbers hi = f16(x), lo = f16(x - hi) (22 significant bits), weights stored times 2^kw
// and activations times 2^ka so that the lo parts stay normal; per output element one f32 accumulator takes w_hi*x_hi and a
// second one w_lo*x_hi + w_hi*x_lo; epilogue fma(acc1 + acc2, 2^-kw, bias) (+ f32 residual), ReLU, split again.
//
// What is different from yy_tower_h3r.hip (32x32x16 MFMA, 32-column tiles, square boards of 6 / 8 / 12 only):
//   * v_mfma_f32_16x16x32_f16: the output tile of a wave is 32 output channels (two 16-row M blocks) x NB column blocks of
//     16 (board, cell) columns.  Columns come in blocks of 16 instead of 32, so 6x6 (4 boards = 144 columns) and 12x12 (144)
//     are exactly 9 blocks -- no padding tile -- and any other board wastes less than one block per workgroup.  The chip holds
//     a higher clock on this MFMA shape at equal cycles per FLOP (MI355X_MICROARCH.md, DVFS give-back item 7).
//   * the (board, cell) geometry is computed at run time from R, C: non-square boards, any number of boards per workgroup.
//   * one k-step of 32 input channels per weight chunk (one MFMA K), so a chunk is [wave][M block 2][part 2][lane 64][8 f16]
//     = 4 KB per wave, loaded global -> register in MFMA operand order and kept in a ring of D chunks (as in yy_tower_h3r).
//   * LDS rows of 2*CH bytes with a stride of 288 B (CH = 96, 128) / 160 B (CH = 32, 64): stride/16 = 2 mod 8 makes the
//     16-column x 4-k-group ds_read_b128 pattern of this MFMA's B operand conflict-free; an off-board tap reads the zero rows
//     at the offset (its own row address mod 256): the bank the lane would have used anyway, so padding reads do not collide
//     with the valid lanes either (the single shared zero slot of yy_tower_h3r.hip cost 22 % extra LDS cycles).
//   * activation fragments are refreshed IN PLACE, block by block, right after their last use (the next chunk's fragment of
//     column block nb is read while the MFMAs of block nb + 1 run): 8*NB registers instead of 16*NB.
//   * bias rows come from scalar loads (no LDS table): NB = 9 with the f32 residual parked in LDS needs 154 of the 160 KB.
//   * k_tower_g (one wave per 32-channel slice) and k_tower_g22 (2x2 wave grid of the 8x8 form, further down) compute the same bits
//     from ONE copy of every shared sequence: stage_planes, mma_split, for_each_tap, epilogue_quad, heads_tail, store_activations.
//   * ROW-ALIGNED form (RB, boards * C == 16 and NB == R, e.g. 8x8 with two boards): column nb*16 + n is row nb of board n / C,
//     x = n % C, so a row shift is a whole block.  Block 0 then reads only the zero rows at the three dy = -1 taps and block
//     NB - 1 at the three dy = +1 taps: those 6 of the 9 * NB (tap, block) pairs of every channel group are dropped at compile
//     time, MFMAs and fragment reads both (1/12 of the tower's MFMAs at NB = 8).  A dropped pair only added exact zeros (finite
//     weights times zero rows, to an accumulator that starts at +0), so every output bit is the one the column form computes.
// Accumulation order per output element is the same for every (NB, boards-per-workgroup) form: identical bits whichever form
// evaluates a board (tests/test_gpu_network.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/yy_engine.h"

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

#include "yy_common.h"

namespace tg {

template <int NW_, int NB_, int D_, bool RB_> struct Geo {
    static constexpr int NW = NW_, NB = NB_, D = D_, CH = 32 * NW_, NCOL = 16 * NB_;
    static constexpr bool RB = RB_;                                 // row-aligned column blocks (see the head of this file)
    static constexpr int RS = (NW_ >= 3) ? 288 : 160;              // row stride: data 2*CH bytes, stride/16 = 2 (mod 8)
    static constexpr int ZERO_OFF = NCOL * RS;                     // two zero rows' worth (512 B) behind the columns of a part
    static constexpr int PART_BYTES = ZERO_OFF + 512;
    static constexpr int RES_OFF = 2 * PART_BYTES;                 // f32 residual: [wave][M block 2][column block NB] x 1 KB, lane-private 16-B slots
    static constexpr int LDS_BYTES = RES_OFF + NW_ * 2 * NB_ * 1024;
    static constexpr int CHUNK_BYTES = NW_ * 4096;
    static_assert(9 % D_ == 0, "ring position = tap % D");
    static_assert(ZERO_OFF % 256 == 0 && PART_BYTES % 256 == 0, "zero rows / parts keep the bank phase");
    static_assert(PART_BYTES + 256 < 65536 && LDS_BYTES <= 163840, "LDS layout");
};

// two f32 -> packed (hi, hi) and (lo, lo) f16 pairs: hi = f16(x) (round to nearest even), lo = f16(x - hi); x - hi is exact in f32
__device__ __forceinline__ void split_pair(const f32x2 a, uint32_t &hi, uint32_t &lo) {
    const f16x2 h = __builtin_convertvector(a, f16x2);
    const f32x2 r = a - __builtin_convertvector(h, f32x2);
    const f16x2 l = __builtin_convertvector(r, f16x2);
    hi = __builtin_bit_cast(uint32_t, h);
    lo = __builtin_bit_cast(uint32_t, l);
}
__device__ __forceinline__ f32x2 join_pair(const uint32_t hi, const uint32_t lo) {
    const f32x2 h = __builtin_convertvector(__builtin_bit_cast(f16x2, hi), f32x2);
    const f32x2 l = __builtin_convertvector(__builtin_bit_cast(f16x2, lo), f32x2);
    return h + l;
}

// this wave's fragments of one weight chunk: [M block MB]{hi, lo}, 8 * MB registers (k_tower_g: MB = 2, k_tower_g22: MB = 4)
template <int MB> struct WChunk {
    f16x8 h[MB], l[MB];
};
// The four 1 KB fragment loads of a chunk: wbase = weights + chunk * CHUNK_BYTES (uniform), voff = wave * 4096 + lane * 16.
// Plain loads that the compiler counts itself: it waits for a ring entry with a counted vmcnt (the 4 * (D - 1) younger loads
// stay in flight) and a sched_group_barrier keeps the refill right behind the chunk that freed the entry.  (yy_tower_h3r.hip
// issues these loads from inline asm with a hand-counted vmcnt: under register pressure the compiler then copies or spills
// the destination registers BEFORE the data has landed -- the failure this form cannot have.)
__device__ __forceinline__ void load_w(WChunk<2> &w, const unsigned char *wbase, uint32_t voff) {
    const u32x4 *p = (const u32x4 *)(wbase + voff);
    w.h[0] = __builtin_bit_cast(f16x8, p[0]);
    w.l[0] = __builtin_bit_cast(f16x8, p[64]);
    w.h[1] = __builtin_bit_cast(f16x8, p[128]);
    w.l[1] = __builtin_bit_cast(f16x8, p[192]);
}

// (board in the workgroup, cell) of column col = nb*16 + n: column form board = col / cells, cell = col % cells; row-aligned
// form board = n / C, cell = nb * C + n % C.  The LDS row of a column is the column index in both.
template <class GEO> __device__ __forceinline__ void col_board_cell(int col, int C, int cells, int &board, int &cell) {
    if constexpr (GEO::RB) {
        const int n = col & 15;
        board = n / C;
        cell = (col >> 4) * C + (n - board * C);
    } else {
        board = col / cells;
        cell = col - board * cells;
    }
}

// per-lane geometry of column nb*16 + n (n = lane & 15); the lane's k group (lane >> 4: input channels [8*kg, 8*kg+8) of a
// 32-channel chunk) is folded into the row base.  Columns of boards >= TB are padding: they read zero rows only.
template <class GEO> struct LaneGeo {
    uint32_t rowbase[GEO::NB], okmask[GEO::NB];
};
template <class GEO> __device__ __forceinline__ void make_lane_geo(LaneGeo<GEO> &g, int lane, int R, int C, int TB) {
    const int n = lane & 15, kg = lane >> 4, cells = R * C;
#pragma unroll
    for (int nb = 0; nb < GEO::NB; nb++) {
        const int col = nb * 16 + n;
        int board, cell;
        col_board_cell<GEO>(col, C, cells, board, cell);
        const int y = cell / C, x = cell - y * C;
        g.rowbase[nb] = (uint32_t)(col * GEO::RS + kg * 16);
        uint32_t m = 0;
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const int sy = y + tap / 3 - 1, sx = x + tap % 3 - 1;
            if (((unsigned)sy < (unsigned)R) && ((unsigned)sx < (unsigned)C)) m |= 1u << tap;
        }
        g.okmask[nb] = (board < TB) ? m : 0u;
    }
}
// LDS byte address (hi part, channel-group offset excluded) column block nb reads for TAP: its shifted row, or -- off the
// board -- the zero rows at (that address mod 256): same bank, no conflict with the lanes that read real rows
template <class GEO, int TAP>
__device__ __forceinline__ uint32_t tap_addr(int nb, int crs, const LaneGeo<GEO> &g) {
    const int shift = (TAP / 3 - 1) * crs + (TAP % 3 - 1) * GEO::RS;   // wave-uniform; crs = C * RS (row-aligned: 16 * RS)
    const uint32_t a = g.rowbase[nb] + (uint32_t)shift;
    return (g.okmask[nb] & (1u << TAP)) ? a : ((a & 255u) | (uint32_t)GEO::ZERO_OFF);
}

// Row-aligned form: (tap, column block) pairs that read nothing but zero rows -- block 0 at dy = -1, block NB - 1 at dy = +1
template <class GEO> constexpr bool off_board(int tap, int nb) {
    return GEO::RB && ((nb == 0 && tap < 3) || (nb == GEO::NB - 1 && tap >= 6));
}

// Activation fragments of one chunk ({hi, lo} x 4 registers per column block), refreshed IN PLACE: right after the MFMAs of block
// nb its slot takes the NEXT chunk's fragment of block nb, i.e. a fragment is requested a whole chunk (6 * NB MFMAs) before its use
// and 8 * NB registers hold activations.  (A shorter rotating window of 3-4 blocks -- 24-32 registers -- was the first form of this
// kernel; with one scheduling region per chunk the full window measures 1.8 % faster at NB = 8 and still fits at NB = 9.)
template <int P> struct XWin {
    f16x8 h[P], l[P];
};
template <class GEO> __device__ __forceinline__ void load_x1(XWin<GEO::NB> &f, int slot, const unsigned char *lds, uint32_t cb) {
    f.h[slot] = __builtin_bit_cast(f16x8, *(const u32x4 *)(lds + cb));
    f.l[slot] = __builtin_bit_cast(f16x8, *(const u32x4 *)(lds + cb + GEO::PART_BYTES));
}
// acc1 += w_hi * x_hi ;  acc2 += w_lo * x_hi + w_hi * x_lo for a wave's MB M blocks of one column block (3 * MB MFMAs).  Two
// accumulators because every MFMA rounds its accumulator once: the large sum is rounded once per k-step (as in an f32 dot
// product) and the 2^-11-times-smaller corrections round among themselves.  The MFMA order inside an M block is the bit contract.
template <int MB, bool ZERO>
__device__ __forceinline__ void mma_split(f32x4 (&acc1)[MB], f32x4 (&acc2)[MB], const WChunk<MB> &w, const f16x8 xh, const f16x8 xl) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mb = 0; mb < MB; mb++) {
        const f32x4 a = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.l[mb], xh, ZERO ? z : acc2[mb], 0, 0, 0);
        acc1[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.h[mb], xh, ZERO ? z : acc1[mb], 0, 0, 0);
        acc2[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.h[mb], xl, a, 0, 0, 0);
    }
}
// The nine taps of one input-channel group as compile-time constants: step(tap, starts the sums, LDS base of this chunk, of the
// chunk after it).  zt: only the layer's first chunk starts the sums; the group's last tap prefetches from the next group (nxt).
template <class STEP, class ZT>
__device__ __forceinline__ void for_each_tap(STEP &step, ZT zt, const unsigned char *cur, const unsigned char *nxt) {
    step(std::integral_constant<int, 0>{}, zt, cur, cur);
    step(std::integral_constant<int, 1>{}, std::false_type{}, cur, cur);
    step(std::integral_constant<int, 2>{}, std::false_type{}, cur, cur);
    step(std::integral_constant<int, 3>{}, std::false_type{}, cur, cur);
    step(std::integral_constant<int, 4>{}, std::false_type{}, cur, cur);
    step(std::integral_constant<int, 5>{}, std::false_type{}, cur, cur);
    step(std::integral_constant<int, 6>{}, std::false_type{}, cur, cur);
    step(std::integral_constant<int, 7>{}, std::false_type{}, cur, cur);
    step(std::integral_constant<int, 8>{}, std::false_type{}, cur, nxt);
}

// One chunk = tap J of input-channel group kq: 6 * NB MFMAs.  lds_cur / lds_next = LDS base + the channel-group offset of this
// chunk / of the chunk after it (the layer's last chunk prefetches in-bounds bytes nobody uses).
template <class GEO, int J, bool ZERO>
__device__ __forceinline__ void run_chunk(f32x4 (&acc1)[GEO::NB][2], f32x4 (&acc2)[GEO::NB][2], const WChunk<2> &w, XWin<GEO::NB> &X,
                                          const unsigned char *lds_cur, const unsigned char *lds_next, int crs, const LaneGeo<GEO> &geo) {
    constexpr int NB = GEO::NB, P = NB;   // P: window length
    static_assert(!GEO::RB || P == NB, "the row-aligned skips assume the full window");
#pragma unroll
    for (int nb = 0; nb < NB; nb++) {
        // off-board pairs (row-aligned form): neither the MFMAs nor the fragment read that would feed them
        const bool mma = !off_board<GEO>(J, nb), ld = nb + P < NB || !off_board<GEO>((J + 1) % 9, nb + P - NB);
        if (mma) mma_split<2, ZERO>(acc1[nb], acc2[nb], w, X.h[nb % P], X.l[nb % P]);
        if (nb + P < NB) load_x1<GEO>(X, nb % P, lds_cur, tap_addr<GEO, J>(nb + P, crs, geo));
        else if (ld) load_x1<GEO>(X, nb % P, lds_next, tap_addr<GEO, (J + 1) % 9>(nb + P - NB, crs, geo));
        if (mma) __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
        if (ld) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    }
}

// One layer: KQ input-channel groups of 32 (stem: 1, the 5 planes zero-padded to 32 channels) x 9 taps, ring position =
// tap % D (compile-time).  After its last use a ring entry is refilled with the chunk D further down the stream (the next
// group / the next layer).  Weight stream order: [layer][kq][tap].
template <class GEO, bool STEM>
__device__ __forceinline__ void run_layer(f32x4 (&acc1)[GEO::NB][2], f32x4 (&acc2)[GEO::NB][2], WChunk<2> (&W)[GEO::D], const unsigned char *lds,
                                          const unsigned char *weights, uint32_t voff, int &chunk, int n_tower, int crs,
                                          const LaneGeo<GEO> &geo) {
    constexpr int KQ = STEM ? 1 : GEO::NW, NB = GEO::NB, D = GEO::D, P = NB;
    XWin<NB> X;
#pragma unroll
    for (int nb = 0; nb < P; nb++)
        if (!off_board<GEO>(0, nb)) load_x1<GEO>(X, nb, lds, tap_addr<GEO, 0>(nb, crs, geo));
    if constexpr (GEO::RB) {   // block 0 skips the layer's first chunk (tap 0): its sums start from +0, as that chunk's would
#pragma unroll
        for (int mb = 0; mb < 2; mb++) acc1[0][mb] = acc2[0][mb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    auto step = [&](auto jt, auto zt, const unsigned char *lds_cur, const unsigned char *lds_next) {
        constexpr int J = decltype(jt)::value, S = J % D;
        run_chunk<GEO, J, decltype(zt)::value>(acc1, acc2, W[S], X, lds_cur, lds_next, crs, geo);
        // refill the ring entry just consumed (the tail of the stream re-reads the last chunk: uniform vmcnt)
        load_w(W[S], weights + (size_t)min(chunk + D, n_tower - 1) * GEO::CHUNK_BYTES, voff);
        __builtin_amdgcn_sched_group_barrier(0x020, 4, 0);     // the four fragment loads stay here, behind this chunk's MFMAs
        // one scheduling region per chunk: the sched_group_barrier solver is superlinear in region size -- with the nine chunks of a
        // channel group in one region this file took 8 minutes to compile, with this line 20 seconds; same kernel time
        __builtin_amdgcn_sched_barrier(0);
        chunk++;
    };
    for_each_tap(step, std::true_type{}, lds, lds + 64);                   // channel group 0, peeled: no zero / non-zero branch
#pragma unroll 1
    for (int kq = 1; kq < KQ; kq++) for_each_tap(step, std::false_type{}, lds + kq * 64, lds + (kq + 1) * 64);
}

// The prologue both kernels share: the zero rows of both parts (512 B each), then the 5 planes of every column (gathered through
// rows, times 2^ka, split) into channels 0..4 of a 32-channel zero-padded input.
template <class GEO>
__device__ __forceinline__ void stage_planes(unsigned char *lds, const float *planes, const int *rows, int g0, int n_live, int C,
                                             int cells, int TB, float in_scale) {
    constexpr int RS = GEO::RS, NT = 64 * GEO::NW;
    for (int t = threadIdx.x; t < 128; t += NT)
        ((u32x2 *)(lds + GEO::ZERO_OFF + (t >> 6) * GEO::PART_BYTES))[t & 63] = (u32x2){0u, 0u};
    for (int col = threadIdx.x; col < GEO::NCOL; col += NT) {
        int b, cell;
        col_board_cell<GEO>(col, C, cells, b, cell);
        const int gb = g0 + b;
        const bool live = b < TB && gb < n_live;
        const int src = live ? (rows ? rows[gb] : gb) : 0;
        float p[6];
#pragma unroll
        for (int k = 0; k < 5; k++) p[k] = live ? planes[((size_t)src * 5 + k) * cells + cell] * in_scale : 0.0f;
        p[5] = 0.0f;
        uint32_t hi[3], lo[3];
#pragma unroll
        for (int k = 0; k < 3; k++) split_pair((f32x2){p[2 * k], p[2 * k + 1]}, hi[k], lo[k]);
        const u32x4 z = {0u, 0u, 0u, 0u};
        *(u32x4 *)(lds + col * RS) = (u32x4){hi[0], hi[1], hi[2], 0u};
        *(u32x4 *)(lds + GEO::PART_BYTES + col * RS) = (u32x4){lo[0], lo[1], lo[2], 0u};
#pragma unroll
        for (int q = 1; q < 4; q++) {
            *(u32x4 *)(lds + col * RS + 16 * q) = z;
            *(u32x4 *)(lds + GEO::PART_BYTES + col * RS + 16 * q) = z;
        }
    }
}

// One lane's four output channels of one (M block, column block) after a layer: (acc1 + acc2) * 2^-kw + bias (+ the f32 residual
// at res) and RELU in f32, kept at res for the skip (KEEP: the output is a block input x), split again into the packed words of
// the hi and the lo part.  Activations, bias rows and residual live in the 2^ka-scaled domain.  The callers keep their loops,
// their bias source and the LDS offsets they store hi and lo at.
template <bool CONV2, bool KEEP, float (*RELU)(float)>
__device__ __forceinline__ void epilogue_quad(const f32x4 acc1, const f32x4 acc2, float acc_scale, const f32x4 bq, unsigned char *res,
                                              u32x2 &hi, u32x2 &lo) {
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = __builtin_fmaf(acc1[i] + acc2[i], acc_scale, bq[i]);
    if (CONV2) v += *(const f32x4 *)res;
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = RELU(v[i]);
    if (KEEP) *(f32x4 *)res = v;
    uint32_t h01, l01, h23, l23;
    split_pair((f32x2){v[0], v[1]}, h01, l01);
    split_pair((f32x2){v[2], v[3]}, h23, l23);
    hi = (u32x2){h01, h23};
    lo = (u32x2){l01, l23};
}

// After the last layer, with out_heads: the 1x1 head convs (neural_network.py:113, 118): unit hm = head * 2 + M block (16 of a
// head's 32 channels), dealt to the waves round-robin; a wave runs its units over every column block.  head_w: [hm 4][kq NW]
// [part 2][lane 64][8 f16].  The per-lane geometry is derived again from a laundered lane id: kept alive from the prologue it would
// sit in scratch across the whole tower.  The asm statement has no "memory" clobber, the form k_tower_g had (k_tower_g22's copy
// carried one): k_tower_g22 stays free of scratch and within its registers without it.
template <class GEO>
__device__ __forceinline__ void heads_tail(const unsigned char *lds, const unsigned char *head_w, const float *head_bias, float *out_heads,
                                           int g0, int n_live, int C, int cells, int TB, int lane, int wave, float head_scale) {
    constexpr int NW = GEO::NW, NB = GEO::NB, RS = GEO::RS;
    int lane2 = lane;
    asm volatile("" : "+v"(lane2));
    const int n16 = lane2 & 15, kg = lane2 >> 4;
    for (int hm = wave; hm < 4; hm += NW) {
        const int head = hm >> 1, mb = hm & 1;
        f16x8 wh[NW], wl[NW];
#pragma unroll
        for (int kq = 0; kq < NW; kq++) {
            const unsigned char *p = head_w + ((size_t)(hm * NW + kq) * 2) * 1024 + lane2 * 16;
            wh[kq] = __builtin_bit_cast(f16x8, *(const u32x4 *)p);
            wl[kq] = __builtin_bit_cast(f16x8, *(const u32x4 *)(p + 1024));
        }
        const float *hb = head_bias + head * 32 + mb * 16;      // uniform: scalar loads
        float sb[16];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            sb[k] = hb[k];
            asm volatile("" : "+s"(sb[k]));
        }
        f32x4 b;
#pragma unroll
        for (int i = 0; i < 4; i++) b[i] = kg == 0 ? sb[i] : kg == 1 ? sb[4 + i] : kg == 2 ? sb[8 + i] : sb[12 + i];
#pragma unroll
        for (int nb = 0; nb < NB; nb++) {
            const uint32_t xb = (uint32_t)((nb * 16 + n16) * RS + kg * 16);
            f32x4 h1 = {0.f, 0.f, 0.f, 0.f}, h2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kq = 0; kq < NW; kq++) {   // mma_split's order, one M block, chained over the k-steps
                const f16x8 xh = __builtin_bit_cast(f16x8, *(const u32x4 *)(lds + xb + kq * 64));
                const f16x8 xl = __builtin_bit_cast(f16x8, *(const u32x4 *)(lds + xb + GEO::PART_BYTES + kq * 64));
                const f32x4 a = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[kq], xh, h2, 0, 0, 0);
                h1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[kq], xh, h1, 0, 0, 0);
                h2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[kq], xl, a, 0, 0, 0);
            }
            // features f32 [row][head][channel 32][cell] (the reference's NCHW flatten order)
            int bd, cell;
            col_board_cell<GEO>(nb * 16 + n16, C, cells, bd, cell);
            const int gb = g0 + bd;
            if (bd < TB && gb < n_live) {
                float *o = out_heads + (((size_t)gb * 2 + head) * 32 + mb * 16 + kg * 4) * cells + cell;
#pragma unroll
                for (int i = 0; i < 4; i++) o[i * cells] = relu_keep_nan(__builtin_fmaf(h1[i] + h2[i], head_scale, b[i]));
            }
        }
    }
}

// After the last layer, without out_heads: activations [column][CH] f32 = (hi + lo) * 2^-ka
template <class GEO>
__device__ __forceinline__ void store_activations(const unsigned char *lds, float *out, int g0, int n_live, int C, int cells, int TB,
                                                  float out_scale) {
    constexpr int CH = GEO::CH, RS = GEO::RS, NT = 64 * GEO::NW;
    const int ncol = TB * cells;            // <= 16 * NB (checked on the host; row-aligned: == 16 * NB)
    for (int p = threadIdx.x; p < ncol * (CH / 4); p += NT) {
        const int col = p / (CH / 4), ch4 = p % (CH / 4);
        int b, cell;
        col_board_cell<GEO>(col, C, cells, b, cell);
        if (b < TB && g0 + b < n_live) {
            const u32x2 ph = *(const u32x2 *)(lds + col * RS + ch4 * 8);
            const u32x2 pl = *(const u32x2 *)(lds + GEO::PART_BYTES + col * RS + ch4 * 8);
            const f32x2 v01 = join_pair(ph.x, pl.x), v23 = join_pair(ph.y, pl.y);
            *(f32x4 *)(out + ((size_t)(g0 + b) * cells + cell) * CH + ch4 * 4) = (f32x4){v01.x, v01.y, v23.x, v23.y} * out_scale;
        }
    }
}

template <int NW_, int NB_, int D_, bool RB_>
__global__ void __launch_bounds__(64 * NW_, 1)
k_tower_g(const float *__restrict__ planes, const unsigned char *__restrict__ weights, const unsigned char *__restrict__ head_w,
          const float *__restrict__ bias, const float *__restrict__ head_bias, float *__restrict__ out, float *__restrict__ out_heads,
          const int *__restrict__ rows, const int *__restrict__ n_rows, int G, int R, int C, int TB, int n_layers, float in_scale,
          float acc_scale, float head_scale, float out_scale, int gate_lo, int gate_hi) {
    using GEO = Geo<NW_, NB_, D_, RB_>;
    constexpr int NW = GEO::NW, NB = GEO::NB, D = GEO::D, CH = GEO::CH, RS = GEO::RS;
    __shared__ __attribute__((aligned(256))) unsigned char lds[GEO::LDS_BYTES];
    const int n_live = n_rows ? min(*n_rows, G) : G;
    if (n_live <= gate_lo || n_live > gate_hi) return;     // the launch only runs for row counts in (gate_lo, gate_hi]
    const int g0 = blockIdx.x * TB;                        // first dense row of the workgroup
    if (g0 >= n_live) return;                              // whole workgroup, before any barrier
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cells = R * C, n_tower = 9 + 9 * NW * (n_layers - 1), crs = (GEO::RB ? 16 : C) * RS;

    // the weight stream starts first: D chunks in flight before anything else is touched
    const uint32_t voff = (uint32_t)(wave * 4096 + lane * 16);
    WChunk<2> W[D];
#pragma unroll
    for (int j = 0; j < D; j++) load_w(W[j], weights + (size_t)min(j, n_tower - 1) * GEO::CHUNK_BYTES, voff);

    stage_planes<GEO>(lds, planes, rows, g0, n_live, C, cells, TB, in_scale);
    LaneGeo<GEO> geo;
    make_lane_geo<GEO>(geo, lane, R, C, TB);
    const int n16 = lane & 15, kg = lane >> 4;
    unsigned char *res_lds = lds + GEO::RES_OFF + (wave * 2 * NB) * 1024 + lane * 16;   // slot (mb * NB + nb) * 1 KB, lane-private
    int chunk = 0;
    // epilogue_quad per (M block, column block), back to LDS.  A lane holds output channels co0 + 0..3 (co0 = 32*wave + 16*mb + 4*kg)
    // of column nb*16 + n16.
    auto epilogue = [&](const int L, f32x4 (&acc1)[NB][2], f32x4 (&acc2)[NB][2], auto conv2_tag, auto keep_tag) {
        constexpr bool CONV2 = decltype(conv2_tag)::value, KEEP = decltype(keep_tag)::value;
        const float *bl = bias + L * CH + wave * 32;          // uniform address: scalar loads, pinned in SGPRs before the selects
        float sb[32];
#pragma unroll
        for (int k = 0; k < 32; k++) {
            sb[k] = bl[k];
            asm volatile("" : "+s"(sb[k]));
        }
        f32x4 bq[2];
#pragma unroll
        for (int mb = 0; mb < 2; mb++)
#pragma unroll
            for (int i = 0; i < 4; i++)
                bq[mb][i] = kg == 0 ? sb[mb * 16 + i] : kg == 1 ? sb[mb * 16 + 4 + i] : kg == 2 ? sb[mb * 16 + 8 + i] : sb[mb * 16 + 12 + i];
#pragma unroll
        for (int nb = 0; nb < NB; nb++) {
            const uint32_t rowoff = (uint32_t)((nb * 16 + n16) * RS);
#pragma unroll
            for (int mb = 0; mb < 2; mb++) {
                u32x2 hi, lo;
                epilogue_quad<CONV2, KEEP, relu_keep_nan>(acc1[nb][mb], acc2[nb][mb], acc_scale, bq[mb], res_lds + (mb * NB + nb) * 1024, hi, lo);
                const uint32_t co2 = (uint32_t)((wave * 32 + mb * 16 + kg * 4) * 2);
                *(u32x2 *)(lds + rowoff + co2) = hi;
                *(u32x2 *)(lds + GEO::PART_BYTES + rowoff + co2) = lo;
            }
        }
    };
    {   // the stem (its own code: 9 one-k-step chunks), outside the loop over the CH -> CH layers
        f32x4 acc1[NB][2], acc2[NB][2];
        __syncthreads();                                   // the prologue's LDS writes are visible
        run_layer<GEO, true>(acc1, acc2, W, lds, weights, voff, chunk, n_tower, crs, geo);
        __syncthreads();                                   // every wave has finished reading the input
        epilogue(0, acc1, acc2, std::false_type{}, std::true_type{});
    }
    for (int L = 1; L < n_layers; L++) {
        f32x4 acc1[NB][2], acc2[NB][2];
        __syncthreads();                                   // the previous layer's epilogue is visible
        run_layer<GEO, false>(acc1, acc2, W, lds, weights, voff, chunk, n_tower, crs, geo);
        __syncthreads();                                   // every wave has finished reading this layer's input
        if ((L & 1) == 0) epilogue(L, acc1, acc2, std::true_type{}, std::true_type{});      // second conv of a block: + skip, keep
        else epilogue(L, acc1, acc2, std::false_type{}, std::false_type{});
    }
    __syncthreads();
    if (out_heads) heads_tail<GEO>(lds, head_w, head_bias, out_heads, g0, n_live, C, cells, TB, lane, wave, head_scale);
    else store_activations<GEO>(lds, out, g0, n_live, C, cells, TB, out_scale);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 2x2 WAVE GRID form of the row-aligned 8-block tower (k_tower_g22): 128 channels, R = 8, boards * C == 16, 8 column blocks (the
// large form of the 8x8 evaluator).  k_tower_g<4, 8, 9, true> gives wave w output channels 32w .. 32w+31 x all 8 blocks: every wave
// reads every B fragment of a chunk and one 2 KB fragment (hi + lo) feeds 6 MFMAs.  Here wave (mh, nh) = (wave >> 1, wave & 1) owns
// channels 64mh .. 64mh+63 (4 M blocks) x column blocks 4nh .. 4nh+3 (rows 4nh .. 4nh+3 of both boards): a fragment feeds 12 MFMAs,
// the LDS bytes read per chunk halve (32 KB per CU instead of 64), the MFMAs per wave and chunk stay 48.
//   * weights: the packing of k_tower_g.  A wave's A operand is the 8 KB of k_tower_g's waves 2mh and 2mh+1 ([M block 4][part 2]
//     [lane 64][8 f16]); both nh waves load the same bytes (the second request is served by the vector L1).  Ring of D = 3 such
//     chunks (96 registers) next to 128 accumulators and 32 fragment registers: no AGPR <-> VGPR copies, no spill.
//   * row ownership: a lane fetches its A rows so that the two M blocks of a pair hold 8 consecutive output channels of its column
//     (load_w22, same packed bytes): the epilogue stores 16-byte pieces, 16 ds_write_b128 per lane and layer instead of 32
//     ds_write_b64, 2-way instead of 4-way conflicted on the 32 store banks (288 B = 8 banks per column).
//   * skips: wave nh = 0 drops block 0 at the three dy = -1 taps, nh = 1 block 7 at the three dy = +1 taps (3 of its 36 (tap,
//     block) pairs).  nh selects one of two compiled copies of the tower, so the skips stay compile-time.
// Every output element keeps its MFMA chain -- [layer][channel group][tap], acc1 / acc2, the same row and column of the same-shaped
// MFMA with the same operands -- so the bits are k_tower_g's.  Both kernels call the one copy of stage_planes, mma_split,
// for_each_tap, epilogue_quad, heads_tail and store_activations above.  What differs here is deliberate and stays: tap addresses
// computed once per kernel (Taps22: the peeled channel group reads at them directly, the looped one adds its channel offset)
// against rowbase / okmask selects (81 address registers do not fit at NB = 9); bias rows from an LDS table (one ds_read_b128 per
// M block) against SGPRs and per-lane selects (NB = 9 has no LDS to spare); relu_max (one v_maximum3_f32) against relu_keep_nan;
// the ring depth; the two weight offsets and the row ownership of load_w22; off22 against off_board; and run_chunk22 / run_layer22 next to run_chunk /
// run_layer, whose scheduling barriers and address forms are what each form's speed consists of.
template <int D_> struct Geo22 : Geo<4, 8, D_, true> {   // rows, parts, zero rows, RES_OFF and weight chunks of k_tower_g<4, 8, D, true>
    static constexpr int NBW = 4, MBW = 4;                               // column blocks and M blocks of a wave
    static constexpr int BIAS_OFF = Geo22::RES_OFF + Geo22::NW * MBW * NBW * 1024;   // behind the residual [wave][M block 4][block 4] x 1 KB
    static constexpr int LDS_BYTES = BIAS_OFF + 21 * Geo22::CH * 4;     // f32 bias rows [layer <= 21][CH]; replaces the base's
    static_assert(LDS_BYTES <= 163840, "LDS layout");
};

// NaN-keeping ReLU in one VALU, v_maximum3_f32 (IEEE 754-2019 maximum: a NaN operand gives a NaN, maximum(-0, +0) = +0): the bits
// of relu_keep_nan for every input that is not a NaN; a NaN stays a NaN (tests/test_gpu_tower_grid.py runs all 2^32 inputs).
__device__ __forceinline__ float relu_max(float v) { return __builtin_elementwise_maximum(v, 0.0f); }

// (tap, local column block) pairs of wave column half NH that read nothing but zero rows
template <int NH> constexpr bool off22(int tap, int b) { return (NH == 0 && b == 0 && tap < 3) || (NH == 1 && b == 3 && tap >= 6); }

// per-lane LDS byte address (hi part, channel group 0) of every (tap, local block) pair that is not dropped
struct Taps22 {
    uint32_t a[9][4];
};
template <class GEO, int NH> __device__ __forceinline__ void make_taps22(Taps22 &t, int lane, int R, int C, int TB) {
    const int n = lane & 15, kg = lane >> 4, cells = R * C;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int col = (4 * NH + b) * 16 + n;
        int board, cell;
        col_board_cell<GEO>(col, C, cells, board, cell);
        const int y = cell / C, x = cell - y * C;
        const uint32_t base = (uint32_t)(col * GEO::RS + kg * 16);
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            if (off22<NH>(tap, b)) continue;
            const int sy = y + tap / 3 - 1, sx = x + tap % 3 - 1;
            const uint32_t a = base + (uint32_t)((tap / 3 - 1) * 16 * GEO::RS + (tap % 3 - 1) * GEO::RS);
            const bool ok = board < TB && (unsigned)sy < (unsigned)R && (unsigned)sx < (unsigned)C;
            t.a[tap][b] = ok ? a : ((a & 255u) | (uint32_t)GEO::ZERO_OFF);
        }
    }
}

// A wave's A fragments of one weight chunk are WChunk<4>: 32 registers, rows of the fragments of k_tower_g's waves 2mh and 2mh + 1
// (8 KB of the chunk: [fragment 4][part 2][lane slot 64][16 B], fragment f = channels 64mh + 16f .. + 15, slot = row + 16 * k group).
// ROW OWNERSHIP: an MFMA's D rows 4kg + i sit in lane group kg, so with k_tower_g's rows a lane would hold channels 16m + 4kg + i of M
// block m: four separated 8-byte pieces of its column's LDS row.  Here row 4kg + i of M block 2j + e is channel 32j + 8kg + 4e + i
// instead: the two M blocks of pair j give a lane 8 consecutive channels, one 16-byte store per part (tower22's epilogue).  Which
// channel a row of an M block stands for enters no output element's MFMA chain (same operands, same k order, same accumulator), so
// every bit stays.  The re-assignment is done here, by where a lane fetches its A rows from: lane (r = lane & 15, q = lane >> 4)
// reads, for M block 2j + e, fragment 2j + (r >> 3), slot 8 * ((r >> 2) & 1) + 4e + (r & 3) + 16q.  w22_lane is the lane's part of
// that offset, w22_imm the part the instruction carries.
constexpr uint32_t w22_lane(int lane) {
    const int r = lane & 15, q = lane >> 4;
    return (uint32_t)((r >> 3) * 2048 + (8 * ((r >> 2) & 1) + (r & 3) + 16 * q) * 16);
}
constexpr uint32_t w22_imm(int j, int e, int p) { return (uint32_t)(j * 4096 + e * 64 + p * 1024); }
// over (j, e, p, lane) the 16-byte pieces fetched are each piece of the wave's 8 KB exactly once, and the piece of (j, e, p, lane)
// is part p, k group q of channel 32j + 8 * (r >> 2) + 4e + (r & 3): row r = 4kg + i of M block 2j + e is channel 32j + 8kg + 4e + i
constexpr bool w22_map_ok() {
    bool seen[512] = {};
    for (int j = 0; j < 2; j++)
        for (int e = 0; e < 2; e++)
            for (int p = 0; p < 2; p++)
                for (int lane = 0; lane < 64; lane++) {
                    const uint32_t o = w22_imm(j, e, p) + w22_lane(lane);
                    if (o % 16 != 0 || o >= 8192 || seen[o / 16]) return false;
                    seen[o / 16] = true;
                    const int frag = (int)(o / 2048), part = (int)(o / 1024) & 1, slot = (int)(o % 1024) / 16;
                    const int r = lane & 15, kg = r >> 2, i = r & 3;
                    if (part != p || (slot >> 4) != (lane >> 4) || 16 * frag + (slot & 15) != 32 * j + 8 * kg + 4 * e + i) return false;
                }
    return true;
}
static_assert(w22_map_ok(), "load_w22: a bijection onto the wave's 8 KB of a chunk that gives a lane 8 consecutive channels per M-block pair");
// wbase: uniform chunk address; voff[j] = 8192 * mh + w22_imm(j, 0, 0) + w22_lane(lane) (two registers, so that every load is
// "uniform base + lane offset + immediate" with no per-chunk 64-bit address arithmetic and every immediate fits the instruction)
__device__ __forceinline__ void load_w22(WChunk<4> &w, const unsigned char *wbase, const uint32_t (&voff)[2]) {
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const unsigned char *p = wbase + voff[m >> 1];
        w.h[m] = __builtin_bit_cast(f16x8, *(const u32x4 *)(p + w22_imm(0, m & 1, 0)));
        w.l[m] = __builtin_bit_cast(f16x8, *(const u32x4 *)(p + w22_imm(0, m & 1, 1)));
    }
}

// One chunk = tap J of an input-channel group: 48 MFMAs less the dropped pairs.  Right after the MFMAs of block b its fragment
// slot takes the next chunk's fragment of block b (tap J + 1; the last tap reads the next channel group at koff_next).
template <int NH, int J, bool ZERO>
__device__ __forceinline__ void run_chunk22(f32x4 (&acc1)[4][4], f32x4 (&acc2)[4][4], const WChunk<4> &w, XWin<4> &X,
                                            const unsigned char *lds_cur, const unsigned char *lds_next, const Taps22 &t, int part_bytes) {
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const bool mma = !off22<NH>(J, b), ld = !off22<NH>((J + 1) % 9, b);
        if (mma) mma_split<4, ZERO>(acc1[b], acc2[b], w, X.h[b], X.l[b]);
        if (ld) {
            const unsigned char *p = (J == 8 ? lds_next : lds_cur) + t.a[(J + 1) % 9][b];
            X.h[b] = __builtin_bit_cast(f16x8, *(const u32x4 *)p);
            X.l[b] = __builtin_bit_cast(f16x8, *(const u32x4 *)(p + part_bytes));
        }
        if (mma) __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
        if (ld) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    }
}

// One layer (stem: one channel group), as run_layer: ring position = tap % D, weight stream order [layer][kq][tap].
template <class GEO, int NH, bool STEM>
__device__ __forceinline__ void run_layer22(f32x4 (&acc1)[4][4], f32x4 (&acc2)[4][4], WChunk<4> (&W)[GEO::D], const unsigned char *lds,
                                            const unsigned char *weights, const uint32_t (&voff)[2], int &chunk, int n_tower,
                                            const Taps22 &t) {
    constexpr int KQ = STEM ? 1 : GEO::NW, D = GEO::D;
    XWin<4> X;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        if (off22<NH>(0, b)) {   // this block skips the layer's first chunk (tap 0): its sums start from +0, as that chunk's would
#pragma unroll
            for (int m = 0; m < 4; m++) acc1[b][m] = acc2[b][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
        } else {
            X.h[b] = __builtin_bit_cast(f16x8, *(const u32x4 *)(lds + t.a[0][b]));
            X.l[b] = __builtin_bit_cast(f16x8, *(const u32x4 *)(lds + t.a[0][b] + GEO::PART_BYTES));
        }
    }
    auto step = [&](auto jt, auto zt, const unsigned char *lds_cur, const unsigned char *lds_next) {
        constexpr int J = decltype(jt)::value, S = J % D;
        run_chunk22<NH, J, decltype(zt)::value>(acc1, acc2, W[S], X, lds_cur, lds_next, t, GEO::PART_BYTES);
        load_w22(W[S], weights + (size_t)min(chunk + D, n_tower - 1) * GEO::CHUNK_BYTES, voff);
        __builtin_amdgcn_sched_group_barrier(0x020, 8, 0);     // the eight fragment loads stay behind this chunk's MFMAs
        __builtin_amdgcn_sched_barrier(0);                       // one scheduling region per chunk (see run_layer)
        chunk++;
    };
    for_each_tap(step, std::true_type{}, lds, lds + 64);          // channel group 0, peeled: reads at the tap addresses themselves
#pragma unroll 1
    for (int kq = 1; kq < KQ; kq++) {
        uint32_t cur = kq * 64, nxt = cur + 64;   // uniform channel-group offsets: one v_add per fragment address
        asm volatile("" : "+s"(cur), "+s"(nxt));
        for_each_tap(step, std::false_type{}, lds + cur, lds + nxt);
    }
}

// Everything of wave column half NH up to the last layer's epilogue: the weight ring and the prologue (plus the bias table), then the
// stem and the CH -> CH layers, each followed by its epilogue.  A lane holds, of column (4NH + b)*16 + n16, output channels 64mh + 32j + 8kg + 4e + 0..3
// in M block 2j + e (load_w22): 8 consecutive channels per pair j, stored as one 16-byte piece per part.
template <class GEO, int NH>
__device__ __forceinline__ void tower22(unsigned char *lds, const float *__restrict__ planes, const unsigned char *__restrict__ weights,
                                        const float *__restrict__ bias, const int *__restrict__ rows, int g0, int n_live, int R, int C,
                                        int TB, int n_layers, int lane, int wave, float in_scale, float acc_scale) {
    constexpr int NW = GEO::NW, D = GEO::D, CH = GEO::CH, RS = GEO::RS, NT = 64 * NW;
    const int cells = R * C, n_tower = 9 + 9 * NW * (n_layers - 1);
    uint32_t voff[2] = {(uint32_t)((wave >> 1) * 8192) + w22_imm(0, 0, 0) + w22_lane(lane), (uint32_t)((wave >> 1) * 8192) + w22_imm(1, 0, 0) + w22_lane(lane)};
    asm volatile("" : "+v"(voff[1]));
    WChunk<4> W[D];
#pragma unroll
    for (int j = 0; j < D; j++) load_w22(W[j], weights + (size_t)min(j, n_tower - 1) * GEO::CHUNK_BYTES, voff);

    for (int i = threadIdx.x; i < n_layers * CH; i += NT) ((float *)(lds + GEO::BIAS_OFF))[i] = bias[i];
    stage_planes<GEO>(lds, planes, rows, g0, n_live, C, cells, TB, in_scale);
    const int mh = wave >> 1, n16 = lane & 15, kg = lane >> 4;
    Taps22 t;
    make_taps22<GEO, NH>(t, lane, R, C, TB);
    unsigned char *res_lds = lds + GEO::RES_OFF + wave * 16 * 1024 + lane * 16;      // slot (m * 4 + b) * 1 KB, lane-private
    int chunk = 0;
    auto epilogue = [&](const int L, f32x4 (&acc1)[4][4], f32x4 (&acc2)[4][4], auto conv2_tag, auto keep_tag) {
        constexpr bool CONV2 = decltype(conv2_tag)::value, KEEP = decltype(keep_tag)::value;
        const unsigned char *bl = lds + GEO::BIAS_OFF + (L * CH + mh * 64 + kg * 8) * 4;
        f32x4 bq[4];
#pragma unroll
        for (int m = 0; m < 4; m++) bq[m] = *(const f32x4 *)(bl + (m >> 1) * 128 + (m & 1) * 16);
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t rowoff = (uint32_t)(((4 * NH + b) * 16 + n16) * RS);
#pragma unroll
            for (int j = 0; j < 2; j++) {
                u32x2 hi[2], lo[2];
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const int m = 2 * j + e;
                    epilogue_quad<CONV2, KEEP, relu_max>(acc1[b][m], acc2[b][m], acc_scale, bq[m], res_lds + (m * 4 + b) * 1024, hi[e], lo[e]);
                }
                // 16-byte pieces at row + 16 * k: the slots the B fragment reads use (one 8-lane store group = 8 columns of one piece)
                const uint32_t co2 = (uint32_t)((mh * 64 + j * 32 + kg * 8) * 2);
                *(u32x4 *)(lds + rowoff + co2) = (u32x4){hi[0].x, hi[0].y, hi[1].x, hi[1].y};
                *(u32x4 *)(lds + GEO::PART_BYTES + rowoff + co2) = (u32x4){lo[0].x, lo[0].y, lo[1].x, lo[1].y};
            }
        }
    };
    {
        f32x4 acc1[4][4], acc2[4][4];
        __syncthreads();                                   // the prologue's LDS writes are visible
        run_layer22<GEO, NH, true>(acc1, acc2, W, lds, weights, voff, chunk, n_tower, t);
        __syncthreads();                                   // every wave has finished reading the input
        epilogue(0, acc1, acc2, std::false_type{}, std::true_type{});
    }
    for (int L = 1; L < n_layers; L++) {
        f32x4 acc1[4][4], acc2[4][4];
        __syncthreads();
        run_layer22<GEO, NH, false>(acc1, acc2, W, lds, weights, voff, chunk, n_tower, t);
        __syncthreads();
        if ((L & 1) == 0) epilogue(L, acc1, acc2, std::true_type{}, std::true_type{});      // second conv of a block: + skip, keep
        else epilogue(L, acc1, acc2, std::false_type{}, std::false_type{});
    }
}

template <int D_>
__global__ void __launch_bounds__(256, 1)
k_tower_g22(const float *__restrict__ planes, const unsigned char *__restrict__ weights, const unsigned char *__restrict__ head_w,
            const float *__restrict__ bias, const float *__restrict__ head_bias, float *__restrict__ out, float *__restrict__ out_heads,
            const int *__restrict__ rows, const int *__restrict__ n_rows, int G, int R, int C, int TB, int n_layers, float in_scale,
            float acc_scale, float head_scale, float out_scale, int gate_lo, int gate_hi) {
    using GEO = Geo22<D_>;
    __shared__ __attribute__((aligned(256))) unsigned char lds[GEO::LDS_BYTES];
    const int n_live = n_rows ? min(*n_rows, G) : G;
    if (n_live <= gate_lo || n_live > gate_hi) return;
    const int g0 = blockIdx.x * TB;
    if (g0 >= n_live) return;
    const int lane = threadIdx.x & 63, cells = R * C;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // nh selects the compiled copy: everything up to the last layer's epilogue runs inside it, so no value crosses the branch
    if (wave & 1) tower22<GEO, 1>(lds, planes, weights, bias, rows, g0, n_live, R, C, TB, n_layers, lane, wave, in_scale, acc_scale);
    else tower22<GEO, 0>(lds, planes, weights, bias, rows, g0, n_live, R, C, TB, n_layers, lane, wave, in_scale, acc_scale);
    __syncthreads();
    if (out_heads) heads_tail<GEO>(lds, head_w, head_bias, out_heads, g0, n_live, C, cells, TB, lane, wave, head_scale);
    else store_activations<GEO>(lds, out, g0, n_live, C, cells, TB, out_scale);
}

// yy_nn_tower_g_relu_check: relu_max against relu_keep_nan, one bit pattern per thread and step
__global__ void __launch_bounds__(256) k_relu_check(uint32_t start, uint32_t count, uint32_t *counts) {
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < count; i += gridDim.x * 256u) {   // 64-bit: no wrap below count
        const uint32_t x = start + (uint32_t)i;
        float v = __builtin_bit_cast(float, x);
        asm volatile("" : "+v"(v));
        const float a = relu_keep_nan(v), b = relu_max(v);
        const bool ok = __builtin_isnan(v) ? __builtin_isnan(b) : __builtin_bit_cast(uint32_t, a) == __builtin_bit_cast(uint32_t, b);
        if (!ok) {
            atomicAdd(&counts[0], 1u);
            atomicMin(&counts[1], x);
        }
    }
}

}   // namespace tg

namespace {

struct TgArgs {
    const float *planes;
    const void *weights, *head_w;
    const float *bias, *head_bias;
    float *out, *out_heads;
    const int *rows, *n_rows;
    int G, R, C, TB, n_layers;
    float sc[4];
    int gate_lo, gate_hi;
    hipStream_t s;
};

// every form runs 64 threads per 32-channel slice (nw slices) and TB boards per workgroup
template <auto KERNEL> int launch_tg(int nw, const TgArgs &a) {
    KERNEL<<<dim3((a.G + a.TB - 1) / a.TB), dim3(64 * nw), 0, a.s>>>(
        a.planes, (const unsigned char *)a.weights, (const unsigned char *)a.head_w, a.bias, a.head_bias, a.out, a.out_heads, a.rows,
        a.n_rows, a.G, a.R, a.C, a.TB, a.n_layers, a.sc[0], a.sc[1], a.sc[2], a.sc[3], a.gate_lo, a.gate_hi);
    if (hipGetLastError() != hipSuccess) return yy_tower_set_err(YY_E_HIP, "yy_nn_tower_g: launch failed");
    return YY_OK;
}

// instantiated forms: 128 channels with 4..9 column blocks; narrower networks with 9 (and 4 for small batches).  The
// row-aligned layout is taken whenever the form admits it (boards * C == 16, nb == R) and it is instantiated: 128 channels at
// nb = 8 (8x8, two boards: the large form of the 8x8 evaluator; the 2x2 wave grid k_tower_g22) and nb = 4 (4x4, four boards).
// layout 1: force the column layout; layout 2: the row-aligned nb = 8 form on k_tower_g's one-wave-per-channel-slice grid.
int dispatch_tg(int nw, int nb, int layout, const TgArgs &a) {
    const bool rb = layout != 1 && a.TB * a.C == 16 && nb == a.R;
    if (nw == 4) {
        if (rb && nb == 8) return layout == 2 ? launch_tg<tg::k_tower_g<4, 8, 9, true>>(nw, a) : launch_tg<tg::k_tower_g22<3>>(nw, a);
        if (rb && nb == 4) return launch_tg<tg::k_tower_g<4, 4, 9, true>>(nw, a);
        switch (nb) {
        case 4: return launch_tg<tg::k_tower_g<4, 4, 9, false>>(nw, a);
        case 5: return launch_tg<tg::k_tower_g<4, 5, 9, false>>(nw, a);
        case 6: return launch_tg<tg::k_tower_g<4, 6, 9, false>>(nw, a);
        case 7: return launch_tg<tg::k_tower_g<4, 7, 9, false>>(nw, a);
        case 8: return launch_tg<tg::k_tower_g<4, 8, 9, false>>(nw, a);
        case 9: return launch_tg<tg::k_tower_g<4, 9, 9, false>>(nw, a);
        }
    } else if (nb == 4 || nb == 9) {
        if (nw == 1) return nb == 4 ? launch_tg<tg::k_tower_g<1, 4, 9, false>>(nw, a) : launch_tg<tg::k_tower_g<1, 9, 3, false>>(nw, a);
        if (nw == 2) return nb == 4 ? launch_tg<tg::k_tower_g<2, 4, 9, false>>(nw, a) : launch_tg<tg::k_tower_g<2, 9, 3, false>>(nw, a);
        if (nw == 3) return nb == 4 ? launch_tg<tg::k_tower_g<3, 4, 9, false>>(nw, a) : launch_tg<tg::k_tower_g<3, 9, 3, false>>(nw, a);
    }
    return yy_tower_set_err(YY_E_UNSUPPORTED, "yy_nn_tower_g: no kernel form for this (channels, column blocks)");
}

}   // namespace

// Column blocks (of 16 columns) the kernel forms exist for, per channel count: yy_nn_tower_g_forms(channels, out[8]) -> count.
extern "C" int yy_nn_tower_g_forms(int channels, int *nb_out) {
    if (channels == 128) {
        for (int i = 0; i < 6; i++) nb_out[i] = 4 + i;
        return 6;
    }
    if (channels == 32 || channels == 64 || channels == 96) {
        nb_out[0] = 4;
        nb_out[1] = 9;
        return 2;
    }
    return 0;
}

// weights: f16 chunks [9 + 9*(channels/32)*(n_layers-1)][channels/32][2][2][64][8] (network.pack_tower_g) times 2^weight_exp;
// head_w f16 [4][channels/32][2][64][8] times 2^head_exp and head_bias f32 [64] (pack_heads_g), or both NULL with out_heads NULL;
// bias f32 [n_layers, channels] times 2^act_exp; planes f32 [G,5,R,C]; out f32 [G,R,C,channels] or out_heads f32 [G,2,32,R*C].
// nb = column blocks per workgroup (a form listed by yy_nn_tower_g_forms), boards = boards per workgroup (boards*R*C <= 16*nb).
// rows / n_rows (device, or both NULL): evaluate planes[rows[i]] for i < *n_rows into dense row i; the launch only runs when
// gate_lo < live rows <= gate_hi (pass -1, INT_MAX for "always").  layout: 0 = the row-aligned column blocks where the form
// admits them (8x8 two-board form: the 2x2 wave grid), 1 = always the column layout, 2 = the row-aligned blocks with one wave per
// 32-channel slice (k_tower_g<4, 8, 9, true>) where the 2x2 grid would run.  Same bits in every layout; 1 and 2 are for timing.
extern "C" int yy_nn_tower_g(const float *planes, const void *weights, const void *head_w, const float *bias, const float *head_bias,
                             float *out, float *out_heads, const int32_t *rows, const int32_t *n_rows, int G, int R, int C,
                             int channels, int n_layers, int weight_exp, int head_exp, int act_exp, int nb, int boards, int gate_lo,
                             int gate_hi, int layout, yy_stream_t s) {
    if (G == 0) return YY_OK;
    if (!planes || !weights || !bias || (!out && !out_heads) || (out_heads && (!head_w || !head_bias)) || G < 0 || (rows && !n_rows))
        return yy_tower_set_err(YY_E_INVALID, "yy_nn_tower_g: bad argument");
    if (R < 1 || C < 1 || R * C > 144 || channels < 32 || channels > 128 || (channels & 31) || n_layers < 1 || n_layers > 21 ||
        (n_layers & 1) == 0 || layout < 0 || layout > 2)
        return yy_tower_set_err(YY_E_UNSUPPORTED,
                                "yy_nn_tower_g: needs boards of at most 144 cells, 32/64/96/128 channels, at most 10 residual blocks");
    if (boards < 1 || nb < 1 || boards * R * C > 16 * nb) return yy_tower_set_err(YY_E_INVALID, "yy_nn_tower_g: boards * cells > 16 * nb");
    TgArgs a = {planes, weights, head_w, bias, head_bias, out, out_heads, rows, n_rows, G, R, C, boards, n_layers,
                {ldexpf(1.0f, act_exp), ldexpf(1.0f, -weight_exp), ldexpf(1.0f, -(head_exp + act_exp)), ldexpf(1.0f, -act_exp)},
                gate_lo, gate_hi, (hipStream_t)s};
    return dispatch_tg(channels / 32, nb, layout, a);
}

extern "C" int yy_nn_tower_g_relu_check(uint32_t start, uint32_t count, uint32_t *counts, yy_stream_t s) {
    if (!counts) return yy_tower_set_err(YY_E_INVALID, "yy_nn_tower_g_relu_check: bad argument");
    if (count == 0) return YY_OK;
    tg::k_relu_check<<<dim3(4096), dim3(256), 0, (hipStream_t)s>>>(start, count, counts);
    if (hipGetLastError() != hipSuccess) return yy_tower_set_err(YY_E_HIP, "yy_nn_tower_g_relu_check: launch failed");
    return YY_OK;
}
