// Keyword spotting: where a label sequence (a query) occurs in a line's frames, with free ends -- the max-plus
// recursion of forced alignment (ctc_align.hip.h) without the outer blanks, a path being allowed to begin at any frame.  The definition
// is search.spot_host:
//   r_t(c) = logits[t, c] - max_c' logits[t, c']  (<= 0; no exp, no log: the softmax normaliser cancels in the ratio to the best path);
//   states s in [0, 2 L - 1): even = labels[s / 2], odd = blank;
//   delta_t(s) = max(delta_{t-1}(s), delta_{t-1}(s-1), [delta_{t-1}(s-2) if s is even, s >= 2 and the two labels differ],
//                    [0 if s = 0: a fresh start]) + r_t(class(s)),
//   a candidate replacing the running best only when STRICTLY greater, tried in that order; sigma_t(s): the frame at which the state's
//   path entered state 0 (a fresh start sets it to t), carried along with delta -- there are no back-pointers;
//   candidates e_t = delta_t(S-1) with start sigma_t(S-1); hits: up to K times the largest live e (ties: the largest t), stop below
//   min_score, then every live candidate whose [sigma_u, u] intersects the hit's [sigma, t] dies.
// One workgroup of 4 waves takes 4 queries of one line (grid (ceil(Q / 4), N)); one wave runs one (line, query) pair:
//   A  mx_t = max_c logits[t, c] of the valid frames (all 4 waves, one frame per wave at a time) -> LDS: once per frame, not per state.
//   B  the recursion, on the shared machine of ctc_lattice.hip.h (DESIGN.md "The lattice kernels' shared pieces": states over the lanes,
//      the prefetch ring, and the neighbour exchange once for delta and once for sigma).  The lane of state S-1 stores e_t and sigma_t:
//      in LDS beside mx when the four waves' tables fit (ET_LDS), else in the pair's region of a global workspace (same code).
//   C  selection on the same wave: per round one pass for the wave-wide arg-max (lane i scans frames i, i + 64, ...) and one pass that
//      kills the overlapping candidates (e_u = -inf).  Lane k keeps hit k; the records go out as ordinary vector stores.
// Every loop is bounded by T, S or K; nothing waits on another workgroup; no atomics: results are reproducible run to run.
#pragma once
#include "ctc_lattice.hip.h"

#define COCR_SPOT_MAX_HITS 8

// dynamic LDS: mx (lattice_row_bytes(T)), then with ET_LDS per wave e (T floats) and sigma (T ints), each padded alike
__host__ __device__ static inline size_t ctcs_pair_words(int T) { return 2 * (lattice_row_bytes(T) / 4); }

template <int SJ, bool ET_LDS>
__global__ __launch_bounds__(256) void ctc_spot_kernel(const float *__restrict__ logits, int T, int C, const int32_t *__restrict__ lens,
                                                       const int32_t *__restrict__ query_lens, const int32_t *__restrict__ query_off,
                                                       const int32_t *__restrict__ queries, int Q, int K, float min_score,
                                                       int32_t *__restrict__ starts, int32_t *__restrict__ ends, float *__restrict__ score,
                                                       int32_t *__restrict__ counts, unsigned *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ctcs_smem[];
    __shared__ int32_t lab_all[4][COCR_LATTICE_MAX_LABELS + 1];
    const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x * 4 + wave;
    const int len = min(max(lens[n], 0), T);
    const float *x = logits + (size_t)n * T * C;
    const size_t row = lattice_row_bytes(T);
    float *mx = reinterpret_cast<float *>(ctcs_smem);
    const int L = q < Q ? query_lens[q] : 0;
    int32_t *lab = lab_all[wave];
    if (q < Q) {
        const int off = query_off[q];
        for (int k = lane; k < L; k += 64) lab[k] = queries[off + k];
    }
    // ---- A: the per-frame maximum
    for (int t = wave; t < len; t += 4) {
        const float m = row_max(x + (size_t)t * C, C, lane);
        if (lane == 0) mx[t] = m;
    }
    __syncthreads();
    if (q >= Q) return;                                   // (no barrier follows)

    const size_t pair = (size_t)n * Q + q;
    float *ev = ET_LDS ? reinterpret_cast<float *>(ctcs_smem + row * (1 + 2 * wave)) : reinterpret_cast<float *>(ws + pair * ctcs_pair_words(T));
    int32_t *sv = reinterpret_cast<int32_t *>(reinterpret_cast<unsigned char *>(ev) + row);
    const int S = 2 * L - 1;

    // ---- B: the recursion
    if (len > 0) {
        int cls[SJ];
        bool skip[SJ], live[SJ], last[SJ];
        lattice_states<SJ, 0>(lab, S, lane, false, cls, skip, live);
        float a[SJ];
        int sg[SJ];
#pragma unroll
        for (int j = 0; j < SJ; ++j) { last[j] = lane + 64 * j == S - 1; a[j] = -INFINITY; sg[j] = -1; }
        int src1, src2;
        lattice_src_fwd(lane, src1, src2);
        lattice_ring(x, C, mx, cls, 0, len, [&](int t, float (&cur)[SJ]) {            // cur: r_t(class(s)) of this lane's states
            float r1[SJ], r2[SJ];
            int g1[SJ], g2[SJ], ns[SJ];
            lattice_rotate(a, r1, r2, src1, src2);
            lattice_rotate(sg, g1, g2, src1, src2);
#pragma unroll
            for (int j = 0; j < SJ; ++j) {
                const float n1 = lattice_seam_fwd(r1, j, lane, 1, -INFINITY), n2 = lattice_seam_fwd(r2, j, lane, 2, -INFINITY);
                // (below state 0 there is no path: its score is -inf and its start never taken, so any value does; the rotated one
                // needs no select)
                const int s1 = lattice_seam_fwd(g1, j, lane, 1, g1[0]), s2 = lattice_seam_fwd(g2, j, lane, 2, g2[0]);
                float best = a[j];
                int from = sg[j];
                if (n1 > best) { best = n1; from = s1; }
                if (skip[j] && n2 > best) { best = n2; from = s2; }
                if (j == 0 && lane == 0 && 0.f > best) { best = 0.f; from = t; }      // the fresh start, state 0 only
                cur[j] = live[j] ? best + cur[j] : -INFINITY;
                ns[j] = from;
            }
#pragma unroll
            for (int j = 0; j < SJ; ++j) {
                a[j] = cur[j]; sg[j] = ns[j];
                if (last[j]) { ev[t] = a[j]; sv[t] = sg[j]; }
            }
        });
        if (!ET_LDS) __threadfence();                // the workspace words written above are read below by other lanes
        __threadfence_block();
    }

    // ---- C: the hits (lane k keeps hit k)
    int my_st = -1, my_en = -1, count = 0;
    float my_sc = -INFINITY;
    for (int k = 0; k < K; ++k) {
        float be = -INFINITY;
        int bt = -1;
        for (int t = lane; t < len; t += 64) {
            const float e = ev[t];
            if (e > -INFINITY && e >= be) { be = e; bt = t; }     // a lane's frames ascend: an equal score later wins
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float oe = __shfl_xor(be, d, 64);
            const int ot = __shfl_xor(bt, d, 64);
            if (oe > be || (oe == be && ot > bt)) { be = oe; bt = ot; }
        }
        if (bt < 0 || be < min_score) break;               // (wave-uniform: every lane holds the same pair)
        const int st = sv[bt];
        if (lane == k) { my_st = st; my_en = bt; my_sc = be; }
        ++count;
        if (k + 1 == K) break;
        for (int u = lane; u < len; u += 64)
            if (ev[u] > -INFINITY && !(u < st || sv[u] > bt)) ev[u] = -INFINITY;
    }
    if (lane < K) {
        const size_t o = pair * K + lane;
        starts[o] = my_st; ends[o] = my_en; score[o] = my_sc;
    }
    if (lane == 0) counts[pair] = count;
}

// et_lds: the candidate tables are in the `lds` bytes of dynamic LDS (then ws is not read)
static inline hipError_t launch_ctc_spot(hipStream_t s, int sj, bool et_lds, size_t lds, const float *logits, int N, int T, int C, const int32_t *lens,
                                         const int32_t *query_lens, const int32_t *query_off, const int32_t *queries, int Q, int K, float min_score,
                                         int32_t *starts, int32_t *ends, float *score, int32_t *counts, unsigned *ws) {
    return with_sj(sj, [&](auto SJ) {
        auto go = [&](auto kern) {
            return lattice_launch(kern, dim3((Q + 3) / 4, N), lds, s, logits, T, C, lens, query_lens, query_off, queries, Q, K, min_score, starts, ends, score, counts, ws);
        };
        return et_lds ? go(ctc_spot_kernel<decltype(SJ)::value, true>) : go(ctc_spot_kernel<decltype(SJ)::value, false>);
    });
}

