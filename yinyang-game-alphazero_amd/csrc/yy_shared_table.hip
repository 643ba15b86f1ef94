// yy_shared_table.hip -- eviction of the replacing shared evaluation table (yy_mcts_set_shared_evaluations_replacing): second
// chance over the whole table, as launches of their own between two tree-step launches of the context's stream, never inside
// a tree step.  The tree kernels of yy_engine.hip only ever turn a free slot (never used, or a tombstone) into a taken one and
// leave stamps behind: the insert stamp in the low half of the slot's claim word, the stamp of the last launch that served
// the entry in its last-hit word.  A sweep is three launches:
//   k_shared_count   live entries (claim stamp neither 0 nor SH_TOMBSTONE), reduced per wave, one atomic add per workgroup
//   k_shared_evict   every workgroup reads that count and returns at once when it is <= high_water; else every entry whose
//                    insert stamp AND last-hit stamp are both older than the cutoff -- the stamp recorded by the last sweep
//                    above the mark -- becomes a tombstone: what was inserted or served since then stays, the rest goes
//   k_shared_close   one thread: books the sweep (live after it, evicted in all) and, above the mark, records the current
//                    stamp as the next cutoff -- in a launch of its own, after every workgroup of the pass has read the old one
// A sweep under the high-water mark records nothing, so the interval an entry has to be used in runs from the last sweep above
// the mark (whether or not it found an entry to evict): a whole fill of the table, not one move.  Before the first recording
// there is no cutoff and nothing is evicted.
//
// Why a sweep may run with selects pending (free-running self-play): a pending leaf that names a slot found it in the latest
// tree-step launch, which left the current stamp in the slot's last-hit word; the cutoff is a stamp recorded earlier, never
// newer than the current one; so that slot is not older than the cutoff and stays, and the launch that reads it finds the row
// it was promised.  Nothing else reads a slot by number.
//
// Stamps wrap (sh_next_stamp: 1 .. 2^32 - 2, then 1 again), so "older" is decided on ages, not on values: age(x) = current - x
// modulo 2^32 grows with every launch since x was handed out (the two skipped values add two to every age across a wrap, to
// all alike), and x is older than the cutoff iff age(x) > age(cutoff).  That holds for entries younger than 2^32 launches; an
// entry left alone for longer looks young again and stays one interval longer -- an eviction less, never a wrong row.
//
// Both passes stream: 16-byte loads (two claim words, four last-hit words), four slots a thread and iteration, grid-stride
// over at most 2048 workgroups, and no store for an entry that stays.
#include "yy_common.h"
#include "yy_tree.h"

#define SH_SWEEP_BLOCK 256
#define SH_SWEEP_MAX_GRID 2048

__device__ __forceinline__ bool sh_live(unsigned long long claim) { return !sh_free(sh_stamp_of(claim)); }

__device__ __forceinline__ unsigned block_sum(unsigned v, unsigned *part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) part[wave] = v;
    __syncthreads();
    unsigned s = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < SH_SWEEP_BLOCK / 64; w++) s += part[w];
    return s;                                   // thread 0 holds the workgroup's sum
}

// slots is a power of two >= 64: quads = slots / 4 groups of four slots
__global__ void __launch_bounds__(SH_SWEEP_BLOCK) k_shared_count(const ulonglong2 *__restrict__ claim, const int64_t quads,
                                                                  unsigned long long *sweep) {
    __shared__ unsigned part[SH_SWEEP_BLOCK / 64];
    unsigned n = 0;
    for (int64_t q = (int64_t)blockIdx.x * SH_SWEEP_BLOCK + threadIdx.x; q < quads; q += (int64_t)gridDim.x * SH_SWEEP_BLOCK) {
        const ulonglong2 a = claim[2 * q], b = claim[2 * q + 1];
        n += (unsigned)sh_live(a.x) + (unsigned)sh_live(a.y) + (unsigned)sh_live(b.x) + (unsigned)sh_live(b.y);
    }
    const unsigned s = block_sum(n, part);
    if (threadIdx.x == 0 && s) atomicAdd(&sweep[SH_SW_COUNT], (unsigned long long)s);
}

__global__ void __launch_bounds__(SH_SWEEP_BLOCK) k_shared_evict(unsigned long long *claim, const uint4 *__restrict__ hit,
                                                                  const int64_t quads, const int64_t high_water,
                                                                  const uint32_t *__restrict__ stamp, unsigned long long *sweep) {
    __shared__ unsigned part[SH_SWEEP_BLOCK / 64];
    if ((int64_t)sweep[SH_SW_COUNT] <= high_water) return;          // uniform over the launch: k_shared_count has completed
    const uint32_t cutoff = (uint32_t)sweep[SH_SW_CUTOFF];
    if (cutoff == 0u) return;                                       // no sweep has recorded a stamp yet: k_shared_close does now
    const uint32_t now = *stamp, keep = now - cutoff;               // an entry of age <= keep was used since the cutoff
    unsigned n = 0;
    for (int64_t q = (int64_t)blockIdx.x * SH_SWEEP_BLOCK + threadIdx.x; q < quads; q += (int64_t)gridDim.x * SH_SWEEP_BLOCK) {
        const ulonglong2 a = ((const ulonglong2 *)claim)[2 * q], b = ((const ulonglong2 *)claim)[2 * q + 1];
        const uint4 h = hit[q];
        const unsigned long long c[4] = {a.x, a.y, b.x, b.y};
        const uint32_t last[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (!sh_live(c[i])) continue;
            if (now - sh_stamp_of(c[i]) > keep && now - last[i] > keep) {
                claim[4 * q + i] = SH_CLAIM(0u, SH_TOMBSTONE);
                n += 1;
            }
        }
    }
    const unsigned s = block_sum(n, part);
    if (threadIdx.x == 0 && s) atomicAdd(&sweep[SH_SW_EVICTING], (unsigned long long)s);
}

__global__ void k_shared_close(const int64_t high_water, const uint32_t *stamp, unsigned long long *sweep) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long live = sweep[SH_SW_COUNT], gone = sweep[SH_SW_EVICTING];
    sweep[SH_SW_LIVE] = live - gone;
    sweep[SH_SW_EVICTED] += gone;
    if ((int64_t)live > high_water) sweep[SH_SW_CUTOFF] = *stamp;
    sweep[SH_SW_COUNT] = 0;
    sweep[SH_SW_EVICTING] = 0;
}

extern "C" int yy_mcts_shared_evaluations_sweep(yy_mcts *c, int64_t high_water_slots, yy_stream_t s) {
    if (!c) return yy_tower_set_err(YY_E_INVALID, "yy_mcts_shared_evaluations_sweep: null pointer");
    const MctsDev &d = c->dev;
    if (!d.sh_claim)
        return yy_tower_set_err(YY_E_STATE, "yy_mcts_shared_evaluations_sweep: the context has no replacing shared evaluation table "
                                            "(yy_mcts_set_shared_evaluations_replacing)");
    if (high_water_slots < 0) return yy_tower_set_err(YY_E_INVALID, "yy_mcts_shared_evaluations_sweep: high_water_slots < 0");
    const int64_t quads = ((int64_t)d.sh.mask + 1) / 4;
    const int64_t want = (quads + SH_SWEEP_BLOCK - 1) / SH_SWEEP_BLOCK;
    const dim3 grid((unsigned)(want < SH_SWEEP_MAX_GRID ? want : SH_SWEEP_MAX_GRID)), block(SH_SWEEP_BLOCK);
    hipLaunchKernelGGL(k_shared_count, grid, block, 0, (hipStream_t)s, (const ulonglong2 *)d.sh_claim, quads, d.sh_sweep);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_shared_evict, grid, block, 0, (hipStream_t)s, d.sh_claim, (const uint4 *)d.sh_hit, quads, high_water_slots,
                       (const uint32_t *)d.sh_stamp, d.sh_sweep);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_shared_close, dim3(1), dim3(1), 0, (hipStream_t)s, high_water_slots, (const uint32_t *)d.sh_stamp, d.sh_sweep);
    HIP_TRY(hipGetLastError());
    return YY_OK;
}
