// Knowledge distillation: the Kullback-Leibler term between a teacher's and a student's per-frame posteriors at temperature tau, and its
// gradient with respect to the student's logits (the definition is conformer_ocr_amd/distill.py kd_loss_host):
//     p = softmax(zT / tau), q = softmax(zS / tau)
//     KD[n] = tau^2 sum_{t < len[n]} sum_c p(c) (log p(c) - log q(c))            d KD / d zS[n, t, :] = tau (q - p)
// distill_frame_kernel: one wave per frame (4 frames per workgroup), the classes strided over the 64 lanes.  While a row fits 16 values
// per lane (ncls <= 1024) both rows are read ONCE and stay in registers; a wider row takes a first pass over memory for its maximum and
// sum (online, per lane) and a second for the outputs.  16-byte accesses (VEC) where ncls % 4 == 0 and all three pointers are 16-byte
// aligned, one float at a time otherwise.  The log-probabilities are (a - max) - log(sum exp(a - max)), never log(p): a teacher
// probability that underflows to 0 contributes exactly 0.  The student's and the teacher's row go through the SAME functions
// (dk_row_regs / dk_row_wide), hence the same instruction sequence: rows of equal values give q - p and log p - log q exactly 0.
// Frames t >= len[n] load no logits: their gradient is 0 (accumulate: ctc_w x what is there).
// The per-frame KL values go to a scratch of N T floats; distill_line_kernel adds each line's valid frames in index order in double
// (64 contiguous chunks, one per lane, then the 64 partial sums in lane order): no floating-point atomics, the same bits on every call.
// Inputs must be finite.  Memory-bound: algorithmic bytes = N T C 4 x (2 reads + 1 write; + 1 read with accumulate).
#pragma once
#include "common.hip.h"

#define COCR_DK_REG 16                  // values per lane and row held in registers: rows of up to 64 x 16 classes

struct DkRow { float mx, lse; };        // of a = z / tau:  log softmax(a)(c) = (a(c) - mx) - lse

// column of register j of a lane: VEC: 4 consecutive columns per 16-byte access, accesses 64 apart; scalar: columns 64 apart
template <bool VEC> __device__ __forceinline__ int dk_col(int lane, int j) { return VEC ? (lane + 64 * (j >> 2)) * 4 + (j & 3) : lane + 64 * j; }

// Loads a row of ncls <= 64 * COCR_DK_REG logits into d[] as a - mx (a = z / tau; -inf beyond the row) and returns its statistics.
template <bool VEC> __device__ __forceinline__ DkRow dk_row_regs(const float *__restrict__ z, int ncls, float tau, int lane, float (&d)[COCR_DK_REG]) {
    if (VEC) {
#pragma unroll
        for (int i = 0; i < COCR_DK_REG / 4; ++i) {
            const int c = (lane + 64 * i) * 4;
            f32x4 v = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (c < ncls) v = *reinterpret_cast<const f32x4 *>(z + c);
#pragma unroll
            for (int k = 0; k < 4; ++k) d[4 * i + k] = v[k];
        }
    } else {
#pragma unroll
        for (int j = 0; j < COCR_DK_REG; ++j) { const int c = lane + 64 * j; d[j] = c < ncls ? z[c] : -INFINITY; }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < COCR_DK_REG; ++j) { d[j] = d[j] / tau; mx = fmaxf(mx, d[j]); }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < COCR_DK_REG; ++j) { d[j] -= mx; sum += expf(d[j]); }
    return DkRow{mx, logf(wave_sum(sum))};
}

// The statistics of a row too wide for the registers: one pass over memory, a running (maximum, sum) per lane, merged over the wave.
template <bool VEC> __device__ __forceinline__ DkRow dk_row_wide(const float *__restrict__ z, int ncls, float tau, int lane) {
    constexpr int W = VEC ? 4 : 1;
    float m = -INFINITY, s = 0.f;
    for (int c = lane * W; c < ncls; c += 64 * W) {
        float v[W];
        if (VEC) { const f32x4 x = *reinterpret_cast<const f32x4 *>(z + c); for (int k = 0; k < W; ++k) v[k] = x[k]; }
        else v[0] = z[c];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const float a = v[k] / tau;
            if (a > m) { s = s * expf(m - a) + 1.0f; m = a; }
            else s += expf(a - m);
        }
    }
    const float mx = wave_max(m);
    const float sum = wave_sum(m == -INFINITY ? 0.f : s * expf(m - mx));
    return DkRow{mx, logf(sum)};
}

// g = accumulate ? ctc_w g + v : v
__device__ __forceinline__ float dk_combine(float old, float v, float ctc_w, int accumulate) { return accumulate ? ctc_w * old + v : v; }

template <bool VEC, bool REG>
__global__ __launch_bounds__(256) void distill_frame_kernel(const float *__restrict__ student, const float *__restrict__ teacher, int frames, int T, int ncls,
                                                            const int32_t *__restrict__ lens, float tau, float *__restrict__ frame_kl, float *grad, float ctc_w,
                                                            float kd_w, int accumulate) {
    constexpr int W = VEC ? 4 : 1;
    const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= frames) return;                                   // (whole waves: no wave-wide operation is left half-populated)
    const int n = f / T, t = f - n * T;
    const size_t row = (size_t)f * ncls;
    float *g = grad ? grad + row : nullptr;
    if (t >= min(max(lens[n], 0), T)) {                        // past the line: no logits are read
        if (g) {
            for (int c = lane * W; c < ncls; c += 64 * W) {
                if (VEC) {
                    f32x4 o = {0.f, 0.f, 0.f, 0.f};
                    if (accumulate) { o = *reinterpret_cast<const f32x4 *>(g + c); for (int k = 0; k < 4; ++k) o[k] = ctc_w * o[k]; }
                    *reinterpret_cast<f32x4 *>(g + c) = o;
                } else g[c] = accumulate ? ctc_w * g[c] : 0.f;
            }
        }
        return;
    }
    const float *zs = student + row, *zt = teacher + row;
    const float gs = kd_w * tau;
    float kl = 0.f;
    if (REG) {
        float ds[COCR_DK_REG], dt[COCR_DK_REG];
        const DkRow rs = dk_row_regs<VEC>(zs, ncls, tau, lane, ds), rt = dk_row_regs<VEC>(zt, ncls, tau, lane, dt);
        float o[COCR_DK_REG];
#pragma unroll
        for (int j = 0; j < COCR_DK_REG; ++j) {
            const float lq = ds[j] - rs.lse, lp = dt[j] - rt.lse;
            const float q = expf(lq), p = expf(lp);
            const bool valid = dk_col<VEC>(lane, j) < ncls;
            if (valid) kl += p * (lp - lq);
            o[j] = gs * (q - p);
        }
        if (g) {
            if (VEC) {
#pragma unroll
                for (int i = 0; i < COCR_DK_REG / 4; ++i) {
                    const int c = (lane + 64 * i) * 4;
                    if (c >= ncls) continue;
                    f32x4 old = {0.f, 0.f, 0.f, 0.f}, v;
                    if (accumulate) old = *reinterpret_cast<const f32x4 *>(g + c);
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = dk_combine(old[k], o[4 * i + k], ctc_w, accumulate);
                    *reinterpret_cast<f32x4 *>(g + c) = v;
                }
            } else {
#pragma unroll
                for (int j = 0; j < COCR_DK_REG; ++j) {
                    const int c = lane + 64 * j;
                    if (c < ncls) g[c] = dk_combine(accumulate ? g[c] : 0.f, o[j], ctc_w, accumulate);
                }
            }
        }
    } else {
        const DkRow rs = dk_row_wide<VEC>(zs, ncls, tau, lane), rt = dk_row_wide<VEC>(zt, ncls, tau, lane);
        for (int c = lane * W; c < ncls; c += 64 * W) {
            float vs[W], vt[W], old[W], out[W];
            if (VEC) {
                const f32x4 xs = *reinterpret_cast<const f32x4 *>(zs + c), xt = *reinterpret_cast<const f32x4 *>(zt + c);
                f32x4 og = {0.f, 0.f, 0.f, 0.f};
                if (g && accumulate) og = *reinterpret_cast<const f32x4 *>(g + c);
                for (int k = 0; k < W; ++k) { vs[k] = xs[k]; vt[k] = xt[k]; old[k] = og[k]; }
            } else { vs[0] = zs[c]; vt[0] = zt[c]; old[0] = (g && accumulate) ? g[c] : 0.f; }
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const float lq = (vs[k] / tau - rs.mx) - rs.lse, lp = (vt[k] / tau - rt.mx) - rt.lse;
                const float q = expf(lq), p = expf(lp);
                kl += p * (lp - lq);
                out[k] = dk_combine(old[k], gs * (q - p), ctc_w, accumulate);
            }
            if (g) {
                if (VEC) { f32x4 v; for (int k = 0; k < W; ++k) v[k] = out[k]; *reinterpret_cast<f32x4 *>(g + c) = v; }
                else g[c] = out[0];
            }
        }
    }
    kl = wave_sum(kl);
    if (lane == 0) frame_kl[f] = kl;
}

// kd[n] = tau^2 x (the line's per-frame values added in index order, in double); one wave per line
__global__ __launch_bounds__(64) void distill_line_kernel(const float *__restrict__ frame_kl, int T, const int32_t *__restrict__ lens, float tau, float *__restrict__ kd) {
    __shared__ double part[64];
    const int n = blockIdx.x, lane = threadIdx.x;
    const int len = min(max(lens[n], 0), T), chunk = (len + 63) / 64;
    const float *fk = frame_kl + (size_t)n * T;
    double s = 0.0;
    for (int t = lane * chunk; t < min(len, (lane + 1) * chunk); ++t) s += (double)fk[t];
    part[lane] = s;
    __syncthreads();
    if (lane == 0) {
        double sum = 0.0;
        for (int l = 0; l < 64; ++l) sum += part[l];
        kd[n] = (float)((double)tau * (double)tau * sum);
    }
}

static inline void launch_distill(hipStream_t s, const float *student, const float *teacher, int N, int T, int ncls, const int32_t *lens, float tau, float *frame_kl,
                                  float *kd, float *grad, float ctc_w, float kd_w, int accumulate) {
    const bool vec = ncls % 4 == 0 && (((uintptr_t)student | (uintptr_t)teacher | (uintptr_t)grad) & 15) == 0, reg = ncls <= 64 * COCR_DK_REG;
    const int frames = N * T;
    const dim3 grid(ceil_div(frames, 4)), block(256);
    auto kern = distill_frame_kernel<false, false>;
    if (vec && reg) kern = distill_frame_kernel<true, true>;
    else if (vec) kern = distill_frame_kernel<true, false>;
    else if (reg) kern = distill_frame_kernel<false, true>;
    hipLaunchKernelGGL(kern, grid, block, 0, s, student, teacher, frames, T, ncls, lens, tau, frame_kl, grad, ctc_w, kd_w, accumulate);
    hipLaunchKernelGGL(distill_line_kernel, dim3(N), dim3(64), 0, s, (const float *)frame_kl, T, lens, tau, kd);
}
