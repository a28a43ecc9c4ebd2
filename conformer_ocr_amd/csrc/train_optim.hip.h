// The optimizer step and the gradient window on flat vectors (cocr_train_adamw, cocr_train_optim_step, cocr_decoder_optim_step,
// cocr_grad_accumulate, cocr_grad_norm: train.hip).  Not part of the training step: nothing here is launched from train_step.hip.h.
#pragma once
#include "common.hip.h"

// ---- torch.optim.AdamW (model.py:283-284) on a flat parameter vector ------------------------------------------------------------------------------
__global__ static void k_adamw_flat(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, size_t n, float lr,
                                    float b1, float b2, float eps, float wd, float bc1, float bc2) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float w = p[i] * (1.0f - lr * wd);
        const float gi = g[i], mi = b1 * m[i] + (1.0f - b1) * gi, vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        w -= lr / bc1 * mi / (sqrtf(vi) / sqrtf(bc2) + eps);
        p[i] = w;
    }
}

// The same step with PER-TENSOR step counts (torch keeps `state['step']` per parameter): the elements of up to COCR_ADAMW_RANGES ranges of
// the flat vector take their own bias corrections -- an output layer adopted after k frozen-backbone steps (cocr_train_adopt_decoder)
// continues at step k + 1 while every other tensor starts at 1.  Unused ranges are empty (lo == hi); the arithmetic per element is
// k_adamw_flat's, so equal corrections give its result bit for bit.
#define COCR_ADAMW_RANGES 4
struct AdamwRanges { unsigned long long lo[COCR_ADAMW_RANGES], hi[COCR_ADAMW_RANGES]; float bc1[COCR_ADAMW_RANGES], bc2[COCR_ADAMW_RANGES]; };
__global__ static void k_adamw_flat_ranges(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, size_t n, float lr,
                                           float b1, float b2, float eps, float wd, float bc1, float bc2, AdamwRanges r) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float c1 = bc1, c2 = bc2;
#pragma unroll
        for (int k = 0; k < COCR_ADAMW_RANGES; ++k)
            if (i >= r.lo[k] && i < r.hi[k]) { c1 = r.bc1[k]; c2 = r.bc2[k]; }
        float w = p[i] * (1.0f - lr * wd);
        const float gi = g[i], mi = b1 * m[i] + (1.0f - b1) * gi, vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        w -= lr / c1 * mi / (sqrtf(vi) / sqrtf(c2) + eps);
        p[i] = w;
    }
}

// ---- one optimizer step of any kind on a flat parameter vector (cocr_train_optim_step / cocr_decoder_optim_step) --------------------------------
// Per element the definitions are torch's single-tensor implementations in fp32 (g' = g + wd p folds the L2 decay into the gradient for
// every kind but AdamW, whose decay is decoupled):
//   AdamW    p *= 1 - lr wd;  m = b1 m + (1 - b1) g;   v = b2 v + (1 - b2) g^2;    p -= lr / bc1 m / (sqrt(v) / sqrt(bc2) + eps)      (k_adamw_flat's expressions)
//   Adam                      m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;   p -= lr / bc1 m / (sqrt(v) / sqrt(bc2) + eps)
//   SGD      buf = mu buf + g';  p -= lr buf            (mu = 0: p -= lr g', the slot is not touched; dampening 0, no Nesterov)
//   RMSprop  sq = alpha sq + (1 - alpha) g'^2;  a = sqrt(sq) + eps;  mu > 0: buf = mu buf + g' / a, p -= lr buf;  else p -= lr g' / a     (not centered)
// The two state vectors are slots whose meaning depends on the kind: AdamW / Adam (exp_avg, exp_avg_sq), SGD (momentum buffer, unused),
// RMSprop (square_avg, momentum buffer).  Slots start zeroed: torch's "buf = g' on a tensor's first step" is mu 0 + g', no flag needed.
// FLAG: Adam kinds -- per-range bias corrections (AdamwRanges, tested per element: a range starts at any float offset); SGD / RMSprop --
// momentum on.  Elements [head, head + 4 nvec) go 16 bytes per lane on all four vectors (the host picks `head` so that they are
// aligned there, or head = n when the vectors' alignments differ); the few before and after go one by one.
// serve_b / serve_f (either may be null): the value the serving forward reads (bf16 / fp32 copy of the output layer).
// gs (cocr_train_optim_step_ex's grad_scale): every gradient element enters the step as fl(gs g), rounded on its own; 1.0f leaves every float as it is.
struct OptimArgs { float lr, wd, b1, b2, eps, mu, alpha, bc1, bc2, gs; };

// Which products the compiler fuses into the following sum is its choice per kernel, and it chooses differently for the 16-byte form of
// a loop than for the scalar one.  So this function takes no such choice: contraction is off, every operation is rounded on its own, and the
// AdamW branch names the three fused operations k_adamw_flat compiles to (1 - lr wd, and (1 - b1) g onto the rounded b1 m; v's two
// products and the final difference are not fused there).  That is what makes the AdamW instance equal cocr_train_adamw bit for bit
// (tests/test_hip_optim.py holds the two against each other), and a vector lane equal the scalar path for every kind.
template <int KIND, bool FLAG>
__device__ __forceinline__ void optim_elem(float &p, const float g_in, float &s0, float &s1, const OptimArgs &a, const float c1, const float c2) {
#pragma clang fp contract(off)
    const float g = a.gs * g_in;
    if constexpr (KIND == COCR_OPT_ADAMW) {
        float w = p * __builtin_fmaf(-a.lr, a.wd, 1.0f);
        const float gi = g, mi = __builtin_fmaf(1.0f - a.b1, gi, a.b1 * s0), vi = gi * ((1.0f - a.b2) * gi) + a.b2 * s1;
        s0 = mi; s1 = vi;
        w -= a.lr / c1 * mi / (sqrtf(vi) / sqrtf(c2) + a.eps);
        p = w;
    } else if constexpr (KIND == COCR_OPT_ADAM) {
        float w = p;
        const float gi = g + a.wd * w, mi = a.b1 * s0 + (1.0f - a.b1) * gi, vi = a.b2 * s1 + (1.0f - a.b2) * gi * gi;
        s0 = mi; s1 = vi;
        w -= a.lr / c1 * mi / (sqrtf(vi) / sqrtf(c2) + a.eps);
        p = w;
    } else if constexpr (KIND == COCR_OPT_SGD) {
        const float gi = g + a.wd * p;
        if constexpr (FLAG) { const float b = a.mu * s0 + gi; s0 = b; p -= a.lr * b; }
        else p -= a.lr * gi;
    } else {
        const float gi = g + a.wd * p, sq = a.alpha * s0 + (1.0f - a.alpha) * gi * gi, d = sqrtf(sq) + a.eps;
        s0 = sq;
        if constexpr (FLAG) { const float b = a.mu * s1 + gi / d; s1 = b; p -= a.lr * b; }
        else p -= a.lr * (gi / d);
    }
}

template <int KIND, bool FLAG>
__global__ __launch_bounds__(256) static void k_optim_flat(float *__restrict__ P, const float *__restrict__ G, float *__restrict__ S0, float *__restrict__ S1, size_t n,
                                                           size_t head, size_t nvec, OptimArgs a, AdamwRanges r, bf16_t *__restrict__ serve_b, float *__restrict__ serve_f) {
    constexpr bool adam = KIND == COCR_OPT_ADAMW || KIND == COCR_OPT_ADAM;
    constexpr bool use0 = adam || KIND == COCR_OPT_RMSPROP || FLAG;            // SGD without momentum touches no slot,
    constexpr bool use1 = adam || (KIND == COCR_OPT_RMSPROP && FLAG);          // RMSprop without momentum and SGD not the second
    auto corr = [&](size_t i, float &c1, float &c2) {
        c1 = a.bc1; c2 = a.bc2;
        if constexpr (adam && FLAG) {
#pragma unroll
            for (int k = 0; k < COCR_ADAMW_RANGES; ++k)
                if (i >= r.lo[k] && i < r.hi[k]) { c1 = r.bc1[k]; c2 = r.bc2[k]; }
        }
    };
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
    for (size_t q = tid; q < nvec; q += nthr) {
        const size_t i = head + 4 * q;
        f32x4 p = *reinterpret_cast<const f32x4 *>(P + i);
        const f32x4 g = *reinterpret_cast<const f32x4 *>(G + i);
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
        if constexpr (use0) s0 = *reinterpret_cast<const f32x4 *>(S0 + i);
        if constexpr (use1) s1 = *reinterpret_cast<const f32x4 *>(S1 + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float c1, c2, pe = p[e], s0e = s0[e], s1e = s1[e];
            corr(i + e, c1, c2);
            optim_elem<KIND, FLAG>(pe, g[e], s0e, s1e, a, c1, c2);
            p[e] = pe; s0[e] = s0e; s1[e] = s1e;
        }
        *reinterpret_cast<f32x4 *>(P + i) = p;
        if constexpr (use0) *reinterpret_cast<f32x4 *>(S0 + i) = s0;
        if constexpr (use1) *reinterpret_cast<f32x4 *>(S1 + i) = s1;
        if (serve_b)
#pragma unroll
            for (int e = 0; e < 4; ++e) serve_b[i + e] = from_f32<bf16_t>(p[e]);
        if (serve_f)
#pragma unroll
            for (int e = 0; e < 4; ++e) serve_f[i + e] = p[e];
    }
    // the elements in front of the aligned part and behind it
    const size_t nscal = n - 4 * nvec;
    for (size_t j = tid; j < nscal; j += nthr) {
        const size_t i = j < head ? j : j + 4 * nvec;
        float c1, c2, pe = P[i], s0e = 0.f, s1e = 0.f;
        if constexpr (use0) s0e = S0[i];
        if constexpr (use1) s1e = S1[i];
        corr(i, c1, c2);
        optim_elem<KIND, FLAG>(pe, G[i], s0e, s1e, a, c1, c2);
        P[i] = pe;
        if constexpr (use0) S0[i] = s0e;
        if constexpr (use1) S1[i] = s1e;
        if (serve_b) serve_b[i] = from_f32<bf16_t>(pe);
        if (serve_f) serve_f[i] = pe;
    }
}

// ---- the gradient window on flat vectors (cocr_grad_accumulate / cocr_grad_norm) ---------------------------------------------------------------
// dst[i] = overwrite ? fl(scale src[i]) : fl(dst[i] + fl(scale src[i])): two fp32 operations, each rounded on its own (contraction off, as in
// optim_elem), which is torch's acc.add_(g * s) bit for bit.  dst may be src (overwrite: the in-place scale), so neither pointer is
// __restrict__ and every element is read before it is written by the lane that owns it.  Elements [head, head + 4 nvec) go 16 bytes per
// lane (the host picks `head` so that both vectors are aligned there, or head = n when their alignments differ); the rest one by one.
__device__ __forceinline__ float accum_elem(const float d, const float s, const float scale, const bool overwrite) {
#pragma clang fp contract(off)
    const float t = scale * s;
    return overwrite ? t : d + t;
}
__global__ __launch_bounds__(256) static void k_grad_accumulate(float *dst, const float *src, size_t n, size_t head, size_t nvec, float scale, int overwrite) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
    for (size_t q = tid; q < nvec; q += nthr) {
        const size_t i = head + 4 * q;
        const f32x4 s = *reinterpret_cast<const f32x4 *>(src + i);
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
        if (!overwrite) d = *reinterpret_cast<const f32x4 *>(dst + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = accum_elem(d[e], s[e], scale, overwrite != 0);
        *reinterpret_cast<f32x4 *>(dst + i) = d;
    }
    const size_t nscal = n - 4 * nvec;
    for (size_t j = tid; j < nscal; j += nthr) {
        const size_t i = j < head ? j : j + 4 * nvec;
        dst[i] = accum_elem(overwrite ? 0.f : dst[i], src[i], scale, overwrite != 0);
    }
}

// Sum of squares in double, stage one: chunk c of `nchunk` owns the elements [c len, min(n, (c + 1) len)), len a multiple of 4 that depends
// on n only.  Within a chunk, group q (4 consecutive elements) belongs to thread q % 256; a thread adds its elements' squares in index
// order (an fp32 x fp32 product is exact in double, so fusing it into the sum changes nothing), then the 256 thread sums are folded by a
// fixed LDS tree.  Which element is added where depends on its index alone: a pointer that is not 16-byte aligned (vec = 0) loads the
// same groups one float at a time.  No atomics; the chunk sums go to part[c].
#define COCR_NORM_MAX_CHUNKS 1024
__global__ __launch_bounds__(256) static void k_sumsq_chunks(const float *__restrict__ g, size_t n, size_t len, int vec, double *__restrict__ part) {
    __shared__ double red[256];
    const size_t lo = (size_t)blockIdx.x * len, hi = lo + len < n ? lo + len : n;
    double acc = 0.0;
    for (size_t i = lo + 4 * (size_t)threadIdx.x; i < hi; i += 4 * 256) {
        if (i + 4 <= hi) {
            float x[4];
            if (vec) { const f32x4 v = *reinterpret_cast<const f32x4 *>(g + i); x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; x[3] = v[3]; }
            else { x[0] = g[i]; x[1] = g[i + 1]; x[2] = g[i + 2]; x[3] = g[i + 3]; }
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += (double)x[e] * (double)x[e];
        } else {
            for (size_t j = i; j < hi; ++j) acc += (double)g[j] * (double)g[j];
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
// stage two: the chunk sums in index order, the square root, one double (one workgroup; the sums come through LDS so that the serial
// additions do not each wait for memory)
__global__ __launch_bounds__(256) static void k_sumsq_finish(const double *__restrict__ part, int nchunk, double *__restrict__ out) {
    __shared__ double s[COCR_NORM_MAX_CHUNKS];
    for (int i = threadIdx.x; i < nchunk; i += 256) s[i] = part[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < nchunk; ++i) t += s[i];
        *out = sqrt(t);
    }
}

// master copy -> the serving copy of the output layer (cocr_decoder_optim_restore)
__global__ static void k_serve_copy(const float *__restrict__ p, size_t n, bf16_t *__restrict__ serve_b, float *__restrict__ serve_f) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        if (serve_b) serve_b[i] = from_f32<bf16_t>(p[i]);
        if (serve_f) serve_f[i] = p[i];
    }
}
