// LayerNorm over the channel dimension (eps 1e-5, affine) on the fp32 residual stream -- the
// nn.LayerNorm that opens each FFN / attention / conv module (reference feed_forward.py:46,
// attention.py:139,148, convolution.py:136) and closes each block (encoder.py:99).
//
// One wave normalises 4 rows at a time (4 independent load -> reduce -> write chains in flight); a row is
// D/4 float4 chunks, lane owns chunks lane, lane+64, ... (NV = ceil(D/256)); mean and the centred second
// moment (like torch) by wave-shuffle reductions.  Optional chain: a block's closing LayerNorm writes the
// fp32 stream back and the next module's LayerNorm is applied to that result in the same pass (two
// LayerNorms back to back with different affine parameters), writing the GEMM operand in the compute dtype.
// HBM-bound: algorithmic bytes = one fp32 read (+ one fp32 write if chained) + one T write per element.
#pragma once
#include "common.hip.h"

// ---- the row pass every LayerNorm of the dense-product path shares (layernorm_kernel and splitk_reduce_ln_kernel below, EpiResidualLN
// in gemm.hip.h): each keeps only its own row source
// gamma or beta of the lane's chunks; zero beyond the row width D = 4 nchunk, so those chunks come out of the affine step as zeros
template <int NV> __device__ __forceinline__ void ln_affine_load(f32x4 (&a)[NV], const float *p, int nchunk, int lane) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = lane + 64 * v;
        a[v] = c < nchunk ? *reinterpret_cast<const f32x4 *>(p + 4 * c) : (f32x4){0, 0, 0, 0};
    }
}
// xv <- LayerNorm(xv) for the wave's 4 rows; s[r]: the lane's share of row r's sum on entry, of the new row's on return (a second
// LayerNorm can follow).  The rows are nnorm chunks wide for the statistics (inv_d = 1 / (4 nnorm)): the chunks from nnorm on hold exact
// zeros (zero padding), so the sums need no mask, the centred squares do.
template <int NV>
__device__ __forceinline__ void ln_rows4(f32x4 (&xv)[4][NV], float (&s)[4], const f32x4 (&gam)[NV], const f32x4 (&bet)[NV], int lane, int nnorm, float inv_d,
                                         float eps) {
    float mean[4], q[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) mean[r] = wave_sum(s[r]) * inv_d;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        q[r] = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const bool ok = lane + 64 * v < nnorm;
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = ok ? xv[r][v][e] - mean[r] : 0.f; q[r] += d * d; }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float rstd = 1.0f / sqrtf(wave_sum(q[r]) * inv_d + eps);
        s[r] = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                xv[r][v][e] = (xv[r][v][e] - mean[r]) * rstd * gam[v][e] + bet[v][e];
                s[r] += xv[r][v][e];
            }
    }
}
// rows m0 .. m0+3 (those below M) of the wave's chunks -> out (M, D) as T
template <typename T, int NV> __device__ __forceinline__ void ln_rows4_store(T *out, int m0, int M, int D, int lane, const f32x4 (&xv)[4][NV]) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = lane + 64 * v;
            if (m0 + r < M && c < (D >> 2)) {
                T *p = out + (size_t)(m0 + r) * D + 4 * c;
                if constexpr (sizeof(T) == 2) { bf16x4 o = {(T)xv[r][v][0], (T)xv[r][v][1], (T)xv[r][v][2], (T)xv[r][v][3]}; *reinterpret_cast<bf16x4 *>(p) = o; }
                else { *reinterpret_cast<f32x4 *>(p) = xv[r][v]; }
            }
        }
}

template <typename T, int NV>
__global__ __launch_bounds__(256) void layernorm_kernel(const float *x, int M, int D, int Dn, float eps,      // Dn: LayerNorm width (columns [Dn, D): zero padding)
                                                        const float *__restrict__ g1, const float *__restrict__ b1,
                                                        float *out_f32,                    // nullable: LN1 result, fp32 (may alias x)
                                                        const float *__restrict__ g2, const float *__restrict__ b2,  // nullable
                                                        T *__restrict__ out_t)             // nullable: LN2(LN1) or LN1 as T
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = (blockIdx.x * 4 + wave) * 4;
    if (row0 >= M) return;
    const float inv_d = 1.0f / (float)Dn;
    const int nchunk = D >> 2, nnorm = Dn >> 2;
    f32x4 ga[NV], ba[NV], gb[NV], bb[NV];
    ln_affine_load<NV>(ga, g1, nchunk, lane);
    ln_affine_load<NV>(ba, b1, nchunk, lane);
    if (g2) {
        ln_affine_load<NV>(gb, g2, nchunk, lane);
        ln_affine_load<NV>(bb, b2, nchunk, lane);
    }
    f32x4 xv[4][NV];
    float s[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = row0 + r;
        s[r] = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = lane + 64 * v;
            xv[r][v] = (m < M && c < nchunk) ? *reinterpret_cast<const f32x4 *>(x + (size_t)m * D + 4 * c) : (f32x4){0, 0, 0, 0};
            s[r] += xv[r][v][0] + xv[r][v][1] + xv[r][v][2] + xv[r][v][3];
        }
    }
    ln_rows4<NV>(xv, s, ga, ba, lane, nnorm, inv_d, eps);
    if (out_f32) ln_rows4_store<float, NV>(out_f32, row0, M, D, lane, xv);
    if (!out_t) return;
    if (g2) ln_rows4<NV>(xv, s, gb, bb, lane, nnorm, inv_d, eps);
    ln_rows4_store<T, NV>(out_t, row0, M, D, lane, xv);
}

template <typename T>
static inline void launch_layernorm(hipStream_t s, const float *x, int M, int D, int Dn, const float *g1, const float *b1, float *out_f32, const float *g2,
                                    const float *b2, T *out_t) {
    dim3 grid(ceil_div(M, 16));
    if (D <= 256) hipLaunchKernelGGL((layernorm_kernel<T, 1>), grid, dim3(256), 0, s, x, M, D, Dn, 1e-5f, g1, b1, out_f32, g2, b2, out_t);
    else if (D <= 512) hipLaunchKernelGGL((layernorm_kernel<T, 2>), grid, dim3(256), 0, s, x, M, D, Dn, 1e-5f, g1, b1, out_f32, g2, b2, out_t);
    else hipLaunchKernelGGL((layernorm_kernel<T, 4>), grid, dim3(256), 0, s, x, M, D, Dn, 1e-5f, g1, b1, out_f32, g2, b2, out_t);
}

// x = sum_z partial[z] + bias (split-K partial sums of the frontend output linear), then LayerNorm -> xn: one wave per 4 rows,
// D <= 256 (one float4 chunk per lane).
template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_ln_kernel(const float *__restrict__ partial, int splits, size_t zstride, const float *__restrict__ bias,
                                                               int M, int D, int Dn, const float *__restrict__ g1, const float *__restrict__ b1,
                                                               float *__restrict__ x, T *__restrict__ xn) {      // Dn: LayerNorm width (columns [Dn, D) are zero padding)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = (blockIdx.x * 4 + wave) * 4;
    if (row0 >= M) return;
    const int nchunk = D >> 2, c = lane, cc = min(c, nchunk - 1);
    const f32x4 bb = *reinterpret_cast<const f32x4 *>(bias + 4 * cc);
    f32x4 v[4][1];
    float s[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const size_t off = (size_t)min(row0 + r, M - 1) * D + 4 * cc;
        f32x4 t = bb;
        for (int z = 0; z < splits; ++z) t += *reinterpret_cast<const f32x4 *>(partial + z * zstride + off);
        if (c >= nchunk) t = (f32x4){0, 0, 0, 0};
        v[r][0] = t;
        s[r] = t[0] + t[1] + t[2] + t[3];
    }
    ln_rows4_store<float, 1>(x, row0, M, D, lane, v);
    f32x4 ga[1], be[1];
    ln_affine_load<1>(ga, g1, nchunk, lane);
    ln_affine_load<1>(be, b1, nchunk, lane);
    ln_rows4<1>(v, s, ga, be, lane, Dn >> 2, 1.0f / (float)Dn, 1e-5f);
    ln_rows4_store<T, 1>(xn, row0, M, D, lane, v);
}
