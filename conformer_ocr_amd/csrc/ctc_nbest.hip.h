// N-best output of the beam searches (the definition is conformer_ocr_amd/nbest.py nbest_host): the first
// `nbest` prefixes of the final beam, each with its records, its exact CTC log-probability and its raw n-gram sum.
// The walk kernels (ctc.hip.h, ctc_lm.hip.h) run unchanged with their back-pointers in global memory, [N][T][COCR_BEAM_MAX], over a
// region filled with 0xFF bytes: a valid back-pointer is (parent << 16) | label with parent < 32, so -1 marks a rank that was not
// alive in that frame.  The survivors of the last frame sit in rank order at rows 0 .. live - 1.
// ctc_nbest_kernel, one workgroup of 256 threads per line:
//   stage   log Z of the line's frames -> LDS; with IN_LDS the line's back-pointer rows too (16-byte loads, `bs` = beam rounded up to
//           four entries per row), else they are read where they are;
//   trace   lane j < nbest of wave 0 walks chain j from (len - 1, j): up to 32 independent chains advance in one wave.  A sentinel at
//           the first step: hypothesis j does not exist.  Every appended label is pushed on the chain's stack as (label << 16) |
//           frame, last label first (LDS with IN_LDS, else a workspace region);
//   records ends / confidences by the 1-best kernels' beam_run (ctc.hip.h), parallel over (hypothesis, label): hypothesis 0 is bit for
//           bit what the walk kernel writes;
//   score   one wave per hypothesis, the four waves round robin: the forward recursion of the criterion (ctc_loss.hip.h) on the
//           blank-extended labels with the shared pieces of ctc_lattice.hip.h -- nothing goes through memory inside the T-step chain
//           -- in the narrowest form (1, 2, 4 or 8 states per lane) that holds the hypothesis; more than COCR_LATTICE_MAX_LABELS
//           labels: NaN; the empty hypothesis is the single blank state.  With an n-gram model: lm_lookup for 64 labels at a time,
//           added with __fadd_rn in label order (the host's float32 sum bit for bit).
// Plain vector loads and stores; no atomics.
#pragma once
#include "ctc_lm.hip.h"
#include "ctc_loss.hip.h"

// entries per staged back-pointer row
__host__ __device__ static inline int nbest_bp_stride(int beam) { return (beam + 3) & ~3; }
// dynamic LDS for lines of at most `cap` frames: log Z alone, or with the back-pointer rows and the label stacks
static inline size_t nbest_lds_bytes(int cap, int beam, int nbest, bool all) {
    return lattice_row_bytes(cap) + (all ? (size_t)cap * ((size_t)nbest_bp_stride(beam) + (size_t)nbest) * 4 : 0);
}

// log p(labels | frames 0 .. len - 1), len >= 1: lab holds L labels, S = 2 L + 1 <= 64 SJ
template <int SJ>
__device__ __forceinline__ float nbest_forward(const float *x, int C, const float *lz, const int32_t *lab, int S, int len, int lane) {
    int cls[SJ];
    bool skip[SJ], live[SJ];
    lattice_states<SJ, 1>(lab, S, lane, false, cls, skip, live);
    float a[SJ];
#pragma unroll
    for (int j = 0; j < SJ; ++j) {
        const int s = lane + 64 * j;
        a[j] = (live[j] && s < 2) ? x[cls[j]] - lz[0] : -INFINITY;
    }
    int src1, src2;
    lattice_src_fwd(lane, src1, src2);
    lattice_ring(x, C, lz, cls, 1, len, [&](int, float (&cur)[SJ]) {               // cur: lp_t(l'_s) of this lane's states
        float r1[SJ], r2[SJ];
        lattice_rotate(a, r1, r2, src1, src2);
#pragma unroll
        for (int j = 0; j < SJ; ++j) {
            const float n1 = lattice_seam_fwd(r1, j, lane, 1, -INFINITY), n2 = lattice_seam_fwd(r2, j, lane, 2, -INFINITY);
            const float v = ctcl_lse3(a[j], n1, skip[j] ? n2 : -INFINITY) + cur[j];
            cur[j] = live[j] ? v : -INFINITY;
        }
#pragma unroll
        for (int j = 0; j < SJ; ++j) a[j] = cur[j];
    });
    float f1 = -INFINITY, f2 = -INFINITY;                                          // the last label's state and the blank behind it
#pragma unroll
    for (int j = 0; j < SJ; ++j) {
        const float v1 = __shfl(a[j], (S - 1) & 63, 64), v2 = __shfl(a[j], (S - 2) & 63, 64);
        if (j == (S - 1) >> 6) f1 = v1;
        if (S > 1 && j == (S - 2) >> 6) f2 = v2;
    }
    return ctcl_lse3(f1, f2, -INFINITY);
}

// SJMAX: the widest form a line of this call can need (2 min(longest line, 255) + 1 states).  bp_all: [N][T][COCR_BEAM_MAX];
// lz_all: log Z of frame (n, t) at lz_all[(n T + t) lz_stride]; stk_ws (without IN_LDS): [N][nbest][T]; cap: frames of the longest line.
// LM: with the n-gram sum.  (That form carries the 16 bytes of scratch that lm_lookup's out-of-line probe continuation hands its result back
// through, as ctc_lm_walk_kernel does; they are touched only when a first probe meets a foreign key.  The plain form has none.)
template <int SJMAX, bool IN_LDS, bool LM>
__global__ __launch_bounds__(256) void ctc_nbest_kernel(const float *__restrict__ logits, int T, int C, const int32_t *__restrict__ lens, int beam, int nbest,
                                                        const int32_t *__restrict__ bp_all, const float *__restrict__ lz_all, int lz_stride,
                                                        cocr_lm_tables L, int32_t *__restrict__ labels, int32_t *__restrict__ starts,
                                                        int32_t *__restrict__ ends, float *__restrict__ conf, int32_t *__restrict__ counts,
                                                        int32_t *__restrict__ nhyp, float *__restrict__ scores, int max_per_line,
                                                        unsigned *__restrict__ stk_ws, int cap) {
    constexpr int NB = COCR_BEAM_MAX;
    extern __shared__ __attribute__((aligned(16))) unsigned char nbest_dyn[];
    __shared__ int32_t lab_w[4][COCR_LATTICE_MAX_LABELS + 1];                      // the labels of the hypothesis a wave scores
    __shared__ int cnt_s[NB], off_s[NB + 1], nh_s;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = min(min(max(lens[n], 0), T), cap);
    const float *lg = logits + (size_t)n * T * C;
    const int32_t *bpg = bp_all + (size_t)n * T * NB;
    const int bs = nbest_bp_stride(beam);
    float *lz = reinterpret_cast<float *>(nbest_dyn);                              // [cap]
    int32_t *bpl = reinterpret_cast<int32_t *>(nbest_dyn + lattice_row_bytes(cap));   // [cap][bs]
    const int sstride = IN_LDS ? cap : T;                                          // entries per chain stack
    unsigned *stk = IN_LDS ? reinterpret_cast<unsigned *>(bpl + (size_t)cap * bs) : stk_ws + (size_t)n * nbest * T;

    // ---- stage
    for (int t = tid; t < len; t += 256) lz[t] = lz_all[((size_t)n * T + t) * lz_stride];
    if (IN_LDS) {
        const int q = bs >> 2;
        for (int i = tid; i < len * q; i += 256) {
            const int t = i / q, u = i - t * q;
            *reinterpret_cast<int4 *>(&bpl[t * bs + 4 * u]) = *reinterpret_cast<const int4 *>(&bpg[(size_t)t * NB + 4 * u]);
        }
    }
    __syncthreads();

    // ---- trace
    if (wave == 0) {
        int cnt = 0;
        bool exists = false;
        if (lane < nbest) {
            if (len == 0) exists = lane == 0;                                      // no frame: the empty prefix alone
            else {
                int e = lane;
                unsigned *my = stk + (size_t)lane * sstride;
                for (int t = len - 1; t >= 0; --t) {
                    const int v = IN_LDS ? bpl[t * bs + e] : bpg[(size_t)t * NB + e];
                    if (v < 0) break;                                              // not alive (only at the first step: a live rank's parent was alive)
                    exists = true;
                    if (v & 0xffff) my[cnt++] = ((unsigned)(v & 0xffff) << 16) | (unsigned)t;
                    e = min(v >> 16, beam - 1);
                }
            }
        }
        const int nh = __popcll(__ballot(exists));                                 // the live ranks are 0 .. nh - 1
        if (lane < NB) cnt_s[lane] = exists ? cnt : 0;
        // offsets of the hypotheses' (truncated) label rows in the records pass
        int kept = (exists && lane < NB) ? min(cnt, max_per_line) : 0, run = kept;
#pragma unroll
        for (int o = 1; o < NB; o <<= 1) {
            const int up = __shfl_up(run, o, 64);
            if (lane >= o) run += up;
        }
        if (lane < NB) off_s[lane + 1] = run;
        if (lane == 0) { off_s[0] = 0; nh_s = nh; nhyp[n] = nh; }
    }
    __threadfence_block();
    __syncthreads();
    const int nh = nh_s;

    // ---- records: ends / confidences, parallel over (hypothesis, label)
    const int total = off_s[NB];
    for (int i = tid; i < total; i += 256) {
        int j = 0;
        while (off_s[j + 1] <= i) ++j;
        const int k = i - off_s[j], cnt = cnt_s[j];
        const unsigned *my = stk + (size_t)j * sstride;
        const unsigned ent = my[cnt - 1 - k];
        const int c = (int)(ent >> 16), s0 = (int)(ent & 0xffffu), limit = k + 1 < cnt ? (int)(my[cnt - 2 - k] & 0xffffu) : len;      // (the next label's start, kept in the row or not)
        const BeamRun r = beam_run(lg, C, c, s0, limit, [=](int t) { return lz[t]; });
        const size_t o = ((size_t)n * nbest + j) * max_per_line + k;
        labels[o] = c; starts[o] = s0; ends[o] = r.end; conf[o] = r.conf();
    }

    // ---- scores: hypothesis j0 + wave
    for (int j0 = 0; j0 < nbest; j0 += 4) {
        const int j = j0 + wave;
        const bool mine = j < nbest, alive = mine && j < nh;
        const int cnt = alive ? cnt_s[j] : 0;
        const unsigned *my = stk + (size_t)(mine ? j : 0) * sstride;
        const bool fits = cnt <= COCR_LATTICE_MAX_LABELS;
        if (alive && fits)
            for (int k = lane; k < cnt; k += 64) lab_w[wave][k] = (int32_t)(my[cnt - 1 - k] >> 16);
        __syncthreads();
        float logp = -INFINITY, lmv = -INFINITY;
        if (alive) {
            if (!fits) logp = __builtin_nanf("");
            else if (len == 0) logp = 0.f;
            else {
                const int S = 2 * cnt + 1;
                const int32_t *lab = lab_w[wave];
                if (S <= 64) logp = nbest_forward<1>(lg, C, lz, lab, S, len, lane);
                else if (SJMAX >= 2 && S <= 128) logp = nbest_forward<(SJMAX >= 2 ? 2 : 1)>(lg, C, lz, lab, S, len, lane);
                else if (SJMAX >= 4 && S <= 256) logp = nbest_forward<(SJMAX >= 4 ? 4 : 1)>(lg, C, lz, lab, S, len, lane);
                else if (SJMAX >= 8) logp = nbest_forward<(SJMAX >= 8 ? 8 : 1)>(lg, C, lz, lab, S, len, lane);
            }
            lmv = 0.f;
            if (LM) {
                for (int base = 0; base < cnt; base += 64) {                       // 64 lookups side by side, then their sum in label order
                    const int k = base + lane;
                    float v = 0.f;
                    if (k < cnt) {
                        unsigned short ctx[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) ctx[u] = (u < COCR_LM_CTX && k - 1 - u >= 0) ? (unsigned short)(my[cnt - k + u] >> 16) : (unsigned short)0;
                        v = lm_lookup(L, ctx, (int)(my[cnt - 1 - k] >> 16));
                    }
                    const int m = min(64, cnt - base);
                    for (int i = 0; i < m; ++i) lmv = __fadd_rn(lmv, __shfl(v, i, 64));
                }
            }
        }
        if (mine && lane == 0) {
            const size_t o = (size_t)n * nbest + j;
            counts[o] = cnt;
            scores[2 * o] = logp; scores[2 * o + 1] = lmv;
        }
        __syncthreads();                                                           // (lab_w is rewritten in the next round)
    }
}

// lds: nbest_lds_bytes(cap, beam, nbest, in_lds)
template <class... A>
static inline hipError_t launch_ctc_nbest(hipStream_t s, int sjmax, bool in_lds, bool lm, size_t lds, int N, A... args) {
    return with_sj(sjmax, [&](auto SJ) {
        constexpr int sj = decltype(SJ)::value;
        auto go = [&](auto kern) { return lattice_launch(kern, dim3(N), lds, s, args...); };
        if (lm) return in_lds ? go(ctc_nbest_kernel<sj, true, true>) : go(ctc_nbest_kernel<sj, false, true>);
        return in_lds ? go(ctc_nbest_kernel<sj, true, false>) : go(ctc_nbest_kernel<sj, false, false>);
    });
}
