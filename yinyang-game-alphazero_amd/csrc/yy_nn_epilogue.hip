// yy_nn_epilogue.hip -- the evaluator's elementwise epilogue kernels and their C ABI entries (include/yy_engine.h):
// bias + residual + ReLU over bf16 activations, the bf16 and float32 head finish (softmax / tanh), leaf-row compaction.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/yy_engine.h"
#include "yy_common.h"

// Fused bias + residual + ReLU over a channels-last bf16 activation tensor, in place:
//     x[r, c] = relu( x[r, c] + bias[c] (+ residual[r, c]) )
// This replaces the 3-4 separate elementwise passes PyTorch/MIOpen run after every convolution of
// the policy/value tower (bias add, residual add, clamp) by ONE pass: 16-B loads/stores per lane,
// f32 arithmetic, one bf16 rounding.  HBM-bound: (2 or 3) * rows * C * 2 bytes per launch.
typedef __attribute__((ext_vector_type(8))) unsigned short us8;

__device__ __forceinline__ float bf2f(unsigned short h) { return __uint_as_float(((uint32_t)h) << 16); }
__device__ __forceinline__ unsigned short f2bf(float f) {   // round-to-nearest-even, NaN stays NaN
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (unsigned short)((u >> 16) | 0x40u);
    return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

template <bool HAS_RES, bool RELU, bool FIXED>
__global__ void __launch_bounds__(256) k_bias_act(us8 *x, const float *bias, const us8 *res, size_t n_vec, int cvec) {
    // cvec = C / 8 vectors per row.  FIXED: the grid stride is a multiple of cvec, so a lane keeps the
    // same 8 channels for its whole grid-stride walk and the bias slice lives in registers.
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    float b[8];
    if (FIXED) {
        const float4 *bp = reinterpret_cast<const float4 *>(bias + (tid % (size_t)cvec) * 8);
        const float4 b0 = bp[0], b1 = bp[1];
        b[0] = b0.x; b[1] = b0.y; b[2] = b0.z; b[3] = b0.w;
        b[4] = b1.x; b[5] = b1.y; b[6] = b1.z; b[7] = b1.w;
    }
    for (size_t i = tid; i < n_vec; i += stride) {
        if (!FIXED) {
            const int cb = (int)(i % (size_t)cvec) * 8;
#pragma unroll
            for (int j = 0; j < 8; j++) b[j] = bias[cb + j];
        }
        const us8 v = x[i];
        us8 r;
        if (HAS_RES) r = res[i];
        us8 o;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            float f = bf2f(v[j]) + b[j];
            if (HAS_RES) f += bf2f(r[j]);
            if (RELU) f = fmaxf(f, 0.0f);
            o[j] = f2bf(f);
        }
        x[i] = o;
    }
}

template <bool FIXED>
static void launch_bias_act(us8 *xv, const float *bias, const us8 *rv, size_t n_vec, int cvec, int relu, unsigned blocks,
                            hipStream_t st) {
    if (rv) {
        if (relu) k_bias_act<true, true, FIXED><<<dim3(blocks), dim3(256), 0, st>>>(xv, bias, rv, n_vec, cvec);
        else k_bias_act<true, false, FIXED><<<dim3(blocks), dim3(256), 0, st>>>(xv, bias, rv, n_vec, cvec);
    } else {
        if (relu) k_bias_act<false, true, FIXED><<<dim3(blocks), dim3(256), 0, st>>>(xv, bias, rv, n_vec, cvec);
        else k_bias_act<false, false, FIXED><<<dim3(blocks), dim3(256), 0, st>>>(xv, bias, rv, n_vec, cvec);
    }
}

extern "C" int yy_nn_bias_act_bf16(void *x, const float *bias, const void *residual, int64_t rows, int C, int relu,
                                   yy_stream_t s) {
    if (rows == 0) return YY_OK;
    if (!x || !bias || rows < 0 || C <= 0) return yy_tower_set_err(YY_E_INVALID, "bad argument");
    if (C % 8) return yy_tower_set_err(YY_E_UNSUPPORTED, "channels must be a multiple of 8");
    const int cvec = C / 8;
    const size_t n_vec = (size_t)rows * (size_t)cvec;
    size_t blocks = (n_vec + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;          // ~8 blocks per CU, grid-stride the rest
    const bool fixed = (256 % cvec) == 0;            // grid stride (blocks*256) is then a multiple of cvec
    if (fixed) launch_bias_act<true>((us8 *)x, bias, (const us8 *)residual, n_vec, cvec, relu, (unsigned)blocks, (hipStream_t)s);
    else launch_bias_act<false>((us8 *)x, bias, (const us8 *)residual, n_vec, cvec, relu, (unsigned)blocks, (hipStream_t)s);
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

// Head finish (neural_network.py:115, 120-121 + predict's softmax :152): row g of h holds the A policy logits
// followed by the H hidden activations of value_fc1 (bias already added by the GEMM, bf16).  One wave per
// row: policy = softmax(logits) in f32; value = tanh(sum_j relu(hidden_j) * w2_j + b2).
__global__ void __launch_bounds__(64) k_head_finish(const unsigned short *__restrict__ h, int A, int H,
                                                    const float *__restrict__ w2, const float *__restrict__ b2,
                                                    float *__restrict__ policy, float *__restrict__ value) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const unsigned short *row = h + (size_t)g * (A + H);
    float mx = -INFINITY;
    for (int a = lane; a < A; a += 64) mx = fmaxf(mx, bf2f(row[a]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.0f;
    for (int a = lane; a < A; a += 64) sum += expf(bf2f(row[a]) - mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    for (int a = lane; a < A; a += 64) policy[(size_t)g * A + a] = expf(bf2f(row[a]) - mx) / sum;
    float acc = 0.0f;
    for (int j = lane; j < H; j += 64) acc += fmaxf(bf2f(row[A + j]), 0.0f) * w2[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) value[g] = tanhf(acc + b2[0]);
}

// float32 head finish (evaluator modes "f16x3" / float32 towers): logits f32 [Gd, A] and value_fc1 outputs f32 [Gd, H]
// (bias added, no ReLU yet) of DENSE row i -> policy[g] = softmax(logits[i]), value[g] = tanh(relu(hidden[i]) . w2 + b2)
// with g = rows ? rows[i] : i; blocks i >= *n_rows exit (the rows a compacted launch did not evaluate).
__global__ void __launch_bounds__(64) k_head_finish_f32(const float *__restrict__ logits, const float *__restrict__ hidden,
                                                        int A, int H, const float *__restrict__ w2,
                                                        const float *__restrict__ b2, const int32_t *__restrict__ rows,
                                                        const int32_t *__restrict__ n_rows, float *__restrict__ policy,
                                                        float *__restrict__ value) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (n_rows && i >= *n_rows) return;
    const int g = rows ? rows[i] : i;
    const float *row = logits + (size_t)i * A;
    float mx = -INFINITY;
    for (int a = lane; a < A; a += 64) mx = fmaxf(mx, row[a]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.0f;
    for (int a = lane; a < A; a += 64) sum += expf(row[a] - mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    for (int a = lane; a < A; a += 64) policy[(size_t)g * A + a] = expf(row[a] - mx) / sum;
    const float *hr = hidden + (size_t)i * H;
    float acc = 0.0f;
    for (int j = lane; j < H; j += 64) acc += relu_keep_nan(hr[j]) * w2[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) value[g] = tanhf(acc + b2[0]);
}

extern "C" int yy_nn_head_finish_f32(const float *logits, const float *hidden, int G, int A, int H, const float *w2,
                                     const float *b2, const int32_t *rows, const int32_t *n_rows, float *policy, float *value,
                                     yy_stream_t s) {
    if (G == 0) return YY_OK;
    if (!logits || !hidden || !w2 || !b2 || !policy || !value || G < 0 || A <= 0 || H <= 0 || (rows && !n_rows))
        return yy_tower_set_err(YY_E_INVALID, "bad argument");
    k_head_finish_f32<<<dim3(G), dim3(64), 0, (hipStream_t)s>>>(logits, hidden, A, H, w2, b2, rows, n_rows, policy, value);
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

// Leaf-batch compaction: rows[0 .. *n) = the indices g with flags[g] != 0, ascending; one 1024-thread workgroup.
__global__ void __launch_bounds__(1024) k_compact_rows(const uint8_t *__restrict__ flags, int G, int32_t *__restrict__ rows,
                                                       int32_t *__restrict__ n) {
    __shared__ int wsum[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = (G + 1023) / 1024, lo = min(t * per, G), hi = min(lo + per, G);
    int cnt = 0;
    for (int g = lo; g < hi; g++) cnt += flags[g] != 0;
    int incl = cnt;                                             // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; w++) base += wsum[w];
    int pos = base + incl - cnt;
    for (int g = lo; g < hi; g++)
        if (flags[g] != 0) rows[pos++] = g;
    if (t == 1023) *n = base + incl;
}

extern "C" int yy_compact_rows(const uint8_t *flags, int G, int32_t *rows, int32_t *n, yy_stream_t s) {
    if (!flags || !rows || !n || G < 0) return yy_tower_set_err(YY_E_INVALID, "bad argument");
    k_compact_rows<<<dim3(1), dim3(1024), 0, (hipStream_t)s>>>(flags, G, rows, n);
    HIP_TRY(hipGetLastError());
    return YY_OK;
}

extern "C" int yy_nn_head_finish_bf16(const void *h, int G, int A, int H, const float *w2, const float *b2, float *policy,
                                      float *value, yy_stream_t s) {
    if (G == 0) return YY_OK;
    if (!h || !w2 || !b2 || !policy || !value || G < 0 || A <= 0 || H <= 0) return yy_tower_set_err(YY_E_INVALID, "bad argument");
    k_head_finish<<<dim3(G), dim3(64), 0, (hipStream_t)s>>>((const unsigned short *)h, A, H, w2, b2, policy, value);
    HIP_TRY(hipGetLastError());
    return YY_OK;
}
