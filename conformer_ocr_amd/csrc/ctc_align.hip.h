// Forced alignment: the best path of a KNOWN label sequence through a line's frames -- the lattice of the CTC
// loss (ctc_loss.hip.h) with max in place of log-sum-exp, plus back-pointers and a traceback.  The definition is align.viterbi_align:
//   delta_0(0) = lp_0(blank), delta_0(1) = lp_0(l'_1);
//   delta_t(s) = max(delta_{t-1}(s), delta_{t-1}(s-1), [delta_{t-1}(s-2) if s is odd, s >= 3 and l'_s != l'_{s-2}]) + lp_t(l'_s),
//   a candidate replacing the running best only when STRICTLY greater, tried in the order stay, s-1, s-2;
//   end state S-1, or S-2 when delta_{T-1}(S-2) > delta_{T-1}(S-1).
// Per line n (one workgroup of 4 waves):
//   A  lz_t = logsumexp_c(logits[t, c]) of the valid frames (all 4 waves, one frame per wave at a time) -> LDS; lp_t(c) = logits[t, c] - lz_t
//      is formed where it is needed, the log-softmax is never stored.
//   B  the recursion on wave 0, on the shared machine of ctc_lattice.hip.h (DESIGN.md "The lattice kernels' shared pieces": states over
//      the lanes, the neighbour exchange, the prefetch ring).  A step is a compare chain; its outcome (0 stay, 1 from s-1, 2 from s-2) is the
//      back-pointer: 2 bits, a lane packing 16 consecutive frames of its state into one word, bp[(t >> 4) * 64 SJ + s] -- in LDS when
//      the table fits (BP_LDS), else in the line's region of a global workspace (same code).
//   C  traceback on wave 0: per block of 16 frames ONE wave-wide read (lane i takes the word of state s - i: a path moves at most 2 states
//      per frame, 32 per block), then 16 scalar steps; lane 0 writes the first / last frame of every label's run to LDS.
//   D  confidences, thread k for label k: exp of the largest lp over its run; starts / ends / conf go out together.
// Every loop is bounded by T, S or L; nothing waits on another workgroup; no atomics: results are reproducible run to run.
#pragma once
#include "ctc_lattice.hip.h"

// dynamic LDS of one line: lz (lattice_row_bytes(T)), then the back-pointer table when it lives in LDS
__host__ __device__ static inline size_t ctca_bp_words(int T, int sj) { return (size_t)((T + 15) / 16) * 64 * sj; }

template <int SJ, bool BP_LDS>
__global__ __launch_bounds__(256) void ctc_align_kernel(const float *__restrict__ logits, int T, int C, const int32_t *__restrict__ lens,
                                                        const int32_t *__restrict__ label_lens, const int32_t *__restrict__ label_off,
                                                        const int32_t *__restrict__ labels, int32_t *__restrict__ starts,
                                                        int32_t *__restrict__ ends, float *__restrict__ conf, float *__restrict__ score,
                                                        int32_t *__restrict__ counts, unsigned *__restrict__ ws, size_t ws_stride) {
    constexpr int SP = 64 * SJ;
    extern __shared__ __attribute__((aligned(16))) unsigned char ctca_smem[];
    __shared__ int32_t lab[COCR_LATTICE_MAX_LABELS + 1], run_st[COCR_LATTICE_MAX_LABELS + 1], run_en[COCR_LATTICE_MAX_LABELS + 1];
    __shared__ float fin[64 * 8];
    __shared__ int sh_ok;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = min(max(lens[n], 0), T);
    const int L = label_lens[n];
    const int S = 2 * L + 1;
    const float *x = logits + (size_t)n * T * C;
    float *lz = reinterpret_cast<float *>(ctca_smem);
    unsigned *bp = BP_LDS ? reinterpret_cast<unsigned *>(ctca_smem + lattice_row_bytes(T)) : ws + (size_t)n * ws_stride;
    const int off = label_off[n];

    for (int k = tid; k < L; k += 256) { lab[k] = labels[off + k]; run_st[k] = 0; run_en[k] = -1; }
    // ---- A: the per-frame normaliser
    for (int t = wave; t < len; t += 4) {
        const float *xt = x + (size_t)t * C;
        const float l = row_lse(xt, C, lane, row_max(xt, C, lane));
        if (lane == 0) lz[t] = l;
    }
    __syncthreads();

    // ---- B: the recursion, C: the traceback (wave 0)
    if (wave == 0) {
        int ok = (len == 0 && L == 0) ? 1 : 0;
        float best_score = ok ? 0.f : -INFINITY;
        if (len > 0) {
            int cls[SJ];
            bool skip[SJ], live[SJ];
            lattice_states<SJ, 1>(lab, S, lane, false, cls, skip, live);
            float a[SJ];
            unsigned acc[SJ];
#pragma unroll
            for (int j = 0; j < SJ; ++j) {
                const int s = lane + 64 * j;
                a[j] = (live[j] && s < 2) ? x[cls[j]] - lz[0] : -INFINITY;
                acc[j] = 0u;
            }
            int src1, src2;
            lattice_src_fwd(lane, src1, src2);
            lattice_ring(x, C, lz, cls, 1, len, [&](int t, float (&cur)[SJ]) {       // cur: lp_t(l'_s) of this lane's states
                float r1[SJ], r2[SJ];
                lattice_rotate(a, r1, r2, src1, src2);
                const int sh = 2 * (t & 15);
                const bool flush = (t & 15) == 15 || t == len - 1;
#pragma unroll
                for (int j = 0; j < SJ; ++j) {
                    const float n1 = lattice_seam_fwd(r1, j, lane, 1, -INFINITY), n2 = lattice_seam_fwd(r2, j, lane, 2, -INFINITY);
                    float best = a[j];
                    unsigned code = 0u;
                    if (n1 > best) { best = n1; code = 1u; }
                    if (skip[j] && n2 > best) { best = n2; code = 2u; }
                    cur[j] = live[j] ? best + cur[j] : -INFINITY;
                    acc[j] |= code << sh;
                }
#pragma unroll
                for (int j = 0; j < SJ; ++j) {
                    a[j] = cur[j];
                    if (flush) { bp[(size_t)(t >> 4) * SP + lane + 64 * j] = acc[j]; acc[j] = 0u; }
                }
            });
#pragma unroll
            for (int j = 0; j < SJ; ++j) fin[lane + 64 * j] = a[j];
            if (!BP_LDS) __threadfence();                // the workspace words written above are read below by other lanes
            __threadfence_block();

            int s = S - 1;
            if (S > 1 && fin[S - 2] > fin[S - 1]) s = S - 2;
            best_score = fin[s];
            ok = best_score != -INFINITY;
            if (ok) {
                s = __builtin_amdgcn_readfirstlane(s);
                int last = len - 1;                      // last frame of the run the walk is in
                for (int blk = (len - 1) >> 4; blk >= 0; --blk) {
                    const int s0 = s, sl = s0 - lane;
                    const unsigned w = sl >= 0 ? bp[(size_t)blk * SP + sl] : 0u;
                    const int t_hi = min(len - 1, 16 * blk + 15), t_lo = max(16 * blk, 1);
                    for (int t = t_hi; t >= t_lo; --t) {
                        const unsigned word = (unsigned)__builtin_amdgcn_readlane((int)w, s0 - s);
                        const int code = (int)((word >> (2 * (t & 15))) & 3u);
                        if (code) {                      // frame t is the first of state s
                            if ((s & 1) && lane == 0) { run_st[s >> 1] = t; run_en[s >> 1] = last; }
                            s = __builtin_amdgcn_readfirstlane(s - code);
                            last = t - 1;
                        }
                    }
                }
                if ((s & 1) && lane == 0) { run_st[s >> 1] = 0; run_en[s >> 1] = last; }
            }
        }
        if (lane == 0) {
            sh_ok = ok;
            score[n] = best_score;
            counts[n] = ok ? L : -1;
        }
    }
    __syncthreads();

    // ---- D: confidences; the records go out
    const bool ok = sh_ok != 0;
    for (int k = tid; k < L; k += 256) {
        int st = -1, en = -1;
        float cf = 0.f;
        if (ok) {
            st = run_st[k]; en = run_en[k];
            const int c = lab[k];
            float mx = -INFINITY;
            for (int t = st; t <= en; ++t) mx = fmaxf(mx, x[(size_t)t * C + c] - lz[t]);
            cf = expf(mx);
        }
        starts[off + k] = st; ends[off + k] = en; conf[off + k] = cf;
    }
}

// bp_lds: the back-pointer table is in the `lds` bytes of dynamic LDS (then ws is not read)
static inline hipError_t launch_ctc_align(hipStream_t s, int sj, bool bp_lds, size_t lds, const float *logits, int N, int T, int C, const int32_t *lens,
                                          const int32_t *label_lens, const int32_t *label_off, const int32_t *labels, int32_t *starts, int32_t *ends,
                                          float *conf, float *score, int32_t *counts, unsigned *ws, size_t ws_stride) {
    return with_sj(sj, [&](auto SJ) {
        auto go = [&](auto kern) {
            return lattice_launch(kern, dim3(N), lds, s, logits, T, C, lens, label_lens, label_off, labels, starts, ends, conf, score, counts, ws, ws_stride);
        };
        return bp_lds ? go(ctc_align_kernel<decltype(SJ)::value, true>) : go(ctc_align_kernel<decltype(SJ)::value, false>);
    });
}
