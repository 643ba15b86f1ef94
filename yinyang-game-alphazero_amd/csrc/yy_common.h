// yy_common.h -- what the .hip files of libyy_hip.so share: the error reporting behind yy_last_error() and the device
// one-liners that more than one kernel file needs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/yy_engine.h"

// Sets the calling thread's yy_last_error() text and returns `code` (defined in yy_engine.hip).
extern "C" int yy_tower_set_err(int code, const char *msg);

// The fused tree step (yy_mcts_step's launch) with the noise rows of the root expansions that are pending among the leaves
// (defined in yy_engine.hip next to the kernel; the caller has checked the context's state).  Only root expansions mix noise.
// Internal to libyy_hip.so: hidden visibility, not part of the C ABI of include/yy_engine.h.
extern "C" __attribute__((visibility("hidden"))) int yy_mcts_step_noise(yy_mcts *ctx, const float *policy, const float *value, const double *noise, double eps,
                                  float *planes, uint8_t *needs_eval, yy_stream_t stream);

static inline int yy_hip_fail(const char *what, hipError_t e) {
    char msg[512];
    snprintf(msg, sizeof msg, "%s: %s", what, hipGetErrorString(e));
    return yy_tower_set_err(YY_E_HIP, msg);
}
#define HIP_TRY(x)                                        \
    do {                                                  \
        hipError_t e_ = (x);                              \
        if (e_ != hipSuccess) return yy_hip_fail(#x, e_); \
    } while (0)

// ReLU that keeps NaN (as torch.relu does): fmaxf(NaN, 0) is 0, which would turn an overflowed activation (hi = inf, lo = -inf
// -> NaN in the next accumulators) back into a finite, wrong result.  Every other input gets fmaxf's result, bit for bit.
__device__ __forceinline__ float relu_keep_nan(float v) { return __builtin_isnan(v) ? v : fmaxf(v, 0.0f); }

// Counted wait on the LDS-DMA weight ring (yy_tower.hip, yy_tower_f32.hip): at most N vector-memory loads still in flight.
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
