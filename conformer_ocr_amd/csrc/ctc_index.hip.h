// The search index's two kernels (the definition is conformer_ocr_amd/index.py pack_host / expand_host).
//   pack    per frame the `keep` classes of the largest logit (ties: the lower class), in that order, each with
//             code = min(255, ceil((m - x[c]) * inv_step)),   m = the frame's maximum:
//           one float32 subtraction, one float32 multiply (never fused), ceil.  code == 0 exactly when x[c] == m.
//   unpack  the dense table the spotter reads: -(code * step) for the kept classes, -(255 * step) for every other one.
// Pack: one wave per frame.  The row is read once, coalesced; lane l holds classes l + 64 j.  `keep` rounds follow: every lane's best
// live class, then a 6-step butterfly on (value, class) that prefers the larger value and then the smaller class; the winner is retired
// in its lane's bit mask (a value cannot mark it: -inf is a legitimate logit).  Lane k keeps round k's record; the records go out as
// two coalesced vector stores.  Rows of up to 512 classes live in registers (J <= 8 values a lane); wider rows stay where they are --
// in LDS when the row fits 64 KB, else in global memory (the L2 serves the passes after the first) -- and a round selects the best
// class AFTER the previous winner in the order (value descending, class ascending), so nothing has to be retired.
// Unpack: one wave per row; lane e holds entry e, every lane composes the values of its classes from the entries (the last entry of a
// class wins, an entry whose class is >= C matches no class and is thereby ignored) and stores each element of the row exactly once.
// Every loop is bounded by C or keep; nothing waits on another wave; no atomics.
#pragma once
#include "common.hip.h"

#define COCR_INDEX_MAX_KEEP 32
#define COCR_INDEX_REG_CLASSES 512      // widest row the pack kernel holds in registers
#define COCR_INDEX_LDS_CLASSES 16384    // widest row it stages in LDS (64 KB, one wave per workgroup)
#define COCR_INDEX_NONE 0x7fffffff

__device__ __forceinline__ bool index_better(float ov, int oc, float v, int c) { return ov > v || (ov == v && oc < c); }

// the wave-wide best (value, class); uniform on return
__device__ __forceinline__ void index_wave_best(float &v, int &c) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float ov = __shfl_xor(v, d, 64);
        const int oc = __shfl_xor(c, d, 64);
        if (index_better(ov, oc, v, c)) { v = ov; c = oc; }
    }
}

__device__ __forceinline__ int index_code(float m, float v, float inv_step) {
    const float q = ceilf(__fmul_rn(__fsub_rn(m, v), inv_step));
    return q < 255.f ? (int)q : 255;                       // (+inf and NaN: 255)
}

__device__ __forceinline__ void index_store(uint16_t *classes, uint8_t *codes, size_t row, int keep, int lane, int cls, int code) {
    if (lane < keep) {
        classes[row * keep + lane] = (uint16_t)cls;
        codes[row * keep + lane] = (uint8_t)code;
    }
}

template <int J>
__global__ __launch_bounds__(256) void posterior_pack_kernel(const float *__restrict__ logits, int T, int C, long rows, const int32_t *__restrict__ lens,
                                                             int keep, float inv_step, uint16_t *__restrict__ classes, uint8_t *__restrict__ codes) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int n = (int)(row / T), t = (int)(row - (long)n * T);
    int my_cls = 0, my_code = 255;
    if (t < lens[n]) {                                       // (wave-uniform)
        const float *x = logits + (size_t)row * C;
        float v[J];
        unsigned live = 0;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int c = lane + 64 * j;
            v[j] = c < C ? x[c] : -INFINITY;
            if (c < C) live |= 1u << j;
        }
        float m = 0.f;
        for (int k = 0; k < keep; ++k) {
            float bv = -INFINITY;
            int bc = COCR_INDEX_NONE;
#pragma unroll
            for (int j = 0; j < J; ++j)                      // classes ascend with j: a strictly greater value only
                if ((live >> j & 1) && (bc == COCR_INDEX_NONE || v[j] > bv)) { bv = v[j]; bc = lane + 64 * j; }
            index_wave_best(bv, bc);
            if (k == 0) m = bv;
            if (bc != COCR_INDEX_NONE && (bc & 63) == lane) live &= ~(1u << (bc >> 6));
            if (lane == k) { my_cls = bc; my_code = index_code(m, bv, inv_step); }
        }
    }
    index_store(classes, codes, (size_t)row, keep, lane, my_cls, my_code);
}

// one wave per workgroup and frame; LDS: the row is staged in dynamic LDS
template <bool LDS>
__global__ __launch_bounds__(64) void posterior_pack_wide_kernel(const float *__restrict__ logits, int T, int C, const int32_t *__restrict__ lens, int keep,
                                                                 float inv_step, uint16_t *__restrict__ classes, uint8_t *__restrict__ codes) {
    extern __shared__ __attribute__((aligned(16))) float index_row[];
    const int lane = threadIdx.x;
    const size_t row = blockIdx.x;
    const int n = (int)(row / T), t = (int)(row - (size_t)n * T);
    int my_cls = 0, my_code = 255;
    if (t < lens[n]) {
        const float *x = logits + row * C;
        float pv = INFINITY, m = 0.f;
        int pc = -1;
        for (int k = 0; k < keep; ++k) {
            float bv = -INFINITY;
            int bc = COCR_INDEX_NONE;
            for (int c = lane; c < C; c += 64) {
                float val;
                if (LDS && k > 0) val = index_row[c];
                else {
                    val = x[c];
                    if (LDS) index_row[c] = val;             // (read back by the same lane only)
                }
                const bool after = val < pv || (val == pv && c > pc);
                if (after && (bc == COCR_INDEX_NONE || val > bv)) { bv = val; bc = c; }
            }
            index_wave_best(bv, bc);
            if (k == 0) m = bv;
            pv = bv; pc = bc;
            if (lane == k) { my_cls = bc; my_code = index_code(m, bv, inv_step); }
        }
    }
    index_store(classes, codes, row, keep, lane, my_cls, my_code);
}

static inline hipError_t launch_posterior_pack(hipStream_t s, const float *logits, int N, int T, int C, const int32_t *lens, int keep, float inv_step,
                                               uint16_t *classes, uint8_t *codes) {
    const long rows = (long)N * T;
    if (C <= COCR_INDEX_REG_CLASSES) {
        const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
        auto go = [&](auto kern) { hipLaunchKernelGGL(kern, grid, block, 0, s, logits, T, C, rows, lens, keep, inv_step, classes, codes); };
        if (C <= 64) go(posterior_pack_kernel<1>);
        else if (C <= 128) go(posterior_pack_kernel<2>);
        else if (C <= 256) go(posterior_pack_kernel<4>);
        else go(posterior_pack_kernel<8>);
    } else if (C <= COCR_INDEX_LDS_CLASSES) {
        hipLaunchKernelGGL(posterior_pack_wide_kernel<true>, dim3((unsigned)rows), dim3(64), (size_t)C * 4, s, logits, T, C, lens, keep, inv_step, classes, codes);
    } else {
        hipLaunchKernelGGL(posterior_pack_wide_kernel<false>, dim3((unsigned)rows), dim3(64), 0, s, logits, T, C, lens, keep, inv_step, classes, codes);
    }
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void posterior_unpack_kernel(const uint16_t *__restrict__ classes, const uint8_t *__restrict__ codes, long rows, int keep, int C,
                                                               float step, float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    int cls = COCR_INDEX_NONE;
    float val = 0.f;
    if (lane < keep) {
        cls = classes[(size_t)row * keep + lane];
        val = -__fmul_rn((float)codes[(size_t)row * keep + lane], step);
    }
    const float floor_v = -__fmul_rn(255.f, step);
    float *o = out + (size_t)row * C;
    for (int c0 = 0; c0 < C; c0 += 64) {                     // (wave-uniform trip count: the shuffles below see all lanes)
        const int c = c0 + lane;
        float r = floor_v;
        for (int e = 0; e < keep; ++e) {
            const int ce = __shfl(cls, e, 64);
            const float ve = __shfl(val, e, 64);
            if (ce == c) r = ve;
        }
        if (c < C) o[c] = r;
    }
}

static inline hipError_t launch_posterior_unpack(hipStream_t s, const uint16_t *classes, const uint8_t *codes, int N, int T, int keep, int C, float step,
                                                 float *out) {
    const long rows = (long)N * T;
    hipLaunchKernelGGL(posterior_unpack_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, classes, codes, rows, keep, C, step, out);
    return hipGetLastError();
}
