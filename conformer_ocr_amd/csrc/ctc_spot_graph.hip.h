// Pattern spotting: where a regular expression over labels matches in a line's frames -- keyword spotting
// (ctc_spot.hip.h) with the chain of states replaced by a GRAPH of label states (Glushkov's position automaton, compiled on the host:
// conformer_ocr_amd/pattern.py).  The definition is pattern.spot_pattern_host:
//   label state q in [0, P) of class cls[q], with a blank state q' after it; flags first[q] / last[q]; preds[q] strictly ascending;
//   delta_t(q)  = best + r_t(cls[q]) over: stay; for each p of preds[q], ascending: delta_{t-1}(p'), then delta_{t-1}(p) if
//                 cls[p] != cls[q]; the fresh start 0 if first[q] (sets sigma = t);
//   delta_t(q') = best + r_t(0) over: stay, then delta_{t-1}(q);
//   a candidate replacing the running best only when STRICTLY greater, tried in that order; sigma carried along with delta;
//   e_t = max over last[q] of delta_t(q) (ties: the lowest q) with start sigma_t and final state final_t = q; selection as in 7i.
// Grid, wave-per-(line, pattern) shape, phase A and phase C are ctc_spot_kernel's; phase A also leaves r_t(0) of the blank beside the
// row maxima (one value per frame, not per state), phase C also carries the final state.  (Phase C is a copy: ctc_spot_kernel keeps
// its own inline, so its compiled code is what it was.)
//   B  label state q on lane q & 63, register q >> 6 (SJ in {1, 2, 4}); its blank state in the same lane and slot, so the blank update
//      is lane-local.  Predecessors are arbitrary, so their values do not come by lane rotation: every frame each lane puts
//      delta(q), delta(q'), sigma(q), sigma(q') of its states into a per-wave LDS exchange array indexed by state, then walks its
//      states' predecessor lists (CSR, copied once from the uploaded tables into LDS, each entry carrying "the classes differ").
//      The exchange is ordered inside ONE wave only: a wave's LDS operations complete in issue order, and a wavefront-scope fence
//      keeps the compiler from moving them.  There is no workgroup barrier inside the frame loop (a wave with q >= Q has left).
//      The lane of the best last state (wave arg-max, ties to the lowest q; skipped when the pattern has one last state) stores
//      e_t, sigma_t, final_t: in LDS when they fit (ET_LDS), else in the pair's region of a global workspace.
// Every loop is bounded by T, P, the edge count or K; nothing waits on another workgroup; no atomics: reproducible run to run.
#pragma once
#include "ctc_lattice.hip.h"

#define COCR_GRAPH_MAX_STATES 256
#define COCR_GRAPH_MAX_EDGES 4096
#define COCR_GRAPH_MAX_HITS 8

// per pair (e, sigma, final), each a padded row of T words
__host__ __device__ static inline size_t ctcg_pair_words(int T) { return 3 * (lattice_row_bytes(T) / 4); }

struct __attribute__((aligned(8))) CtcgCell { float d; int32_t s; };

// static LDS of one wave: the exchange arrays and the predecessor lists
struct CtcgWave {
    CtcgCell xa[COCR_GRAPH_MAX_STATES], xb[COCR_GRAPH_MAX_STATES];        // (delta, sigma) of the label states / of their blank states: one 8-byte read each
    uint16_t off[COCR_GRAPH_MAX_STATES + 2];                              // CSR offsets into ent
    uint16_t ent[COCR_GRAPH_MAX_EDGES];                                   // predecessor p | (cls[p] != cls[q]) << 8
};
#define COCR_GRAPH_STATIC_LDS (4 * sizeof(CtcgWave))

// the wave's LDS traffic of one frame stays in program order (a wave's LDS operations complete in issue order)
__device__ __forceinline__ void ctcg_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <int SJ, bool ET_LDS>
__global__ __launch_bounds__(256) void ctc_spot_graph_kernel(const float *__restrict__ logits, int T, int C, const int32_t *__restrict__ lens,
                                                             const int32_t *__restrict__ pat_states, const int32_t *__restrict__ state_off,
                                                             const int32_t *__restrict__ edge_off, const int32_t *__restrict__ cls_all,
                                                             const int32_t *__restrict__ flags_all, const int32_t *__restrict__ poff_all,
                                                             const int32_t *__restrict__ preds_all, int Q, int K, float min_score,
                                                             int32_t *__restrict__ starts, int32_t *__restrict__ ends, float *__restrict__ score,
                                                             int32_t *__restrict__ finals, int32_t *__restrict__ counts, unsigned *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ctcg_smem[];
    __shared__ CtcgWave graph_all[4];
    const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x * 4 + wave;
    const int len = min(max(lens[n], 0), T);
    const float *x = logits + (size_t)n * T * C;
    const size_t row = lattice_row_bytes(T);
    float *mx = reinterpret_cast<float *>(ctcg_smem);
    float *rb = reinterpret_cast<float *>(ctcg_smem + row);
    CtcgWave &g = graph_all[wave];
    const int P = q < Q ? min(pat_states[q], COCR_GRAPH_MAX_STATES) : 0;
    const int32_t *pcls = cls_all, *pflags = flags_all;
    if (q < Q) {
        const int so = state_off[q];
        pcls = cls_all + so; pflags = flags_all + so;
        const int32_t *poff = poff_all + so + q, *ppred = preds_all + edge_off[q];
        for (int s = lane; s <= P; s += 64) g.off[s] = (uint16_t)min(poff[s], COCR_GRAPH_MAX_EDGES);
        for (int s = lane; s < P; s += 64) {
            const int lo = min(poff[s], COCR_GRAPH_MAX_EDGES), hi = min(poff[s + 1], COCR_GRAPH_MAX_EDGES), c = pcls[s];
            for (int e = lo; e < hi; ++e) {
                const int p = ppred[e] & (COCR_GRAPH_MAX_STATES - 1);
                g.ent[e] = (uint16_t)(p | (pcls[p] != c ? 256 : 0));
            }
        }
    }
    // ---- A: the per-frame maximum and the blank's r_t(0)
    for (int t = wave; t < len; t += 4) {
        const float m = row_max(x + (size_t)t * C, C, lane);
        if (lane == 0) { mx[t] = m; rb[t] = x[(size_t)t * C] - m; }
    }
    __syncthreads();
    if (q >= Q) return;                                   // (no barrier follows)

    const size_t pair = (size_t)n * Q + q;
    float *ev = ET_LDS ? reinterpret_cast<float *>(ctcg_smem + row * (2 + 3 * wave)) : reinterpret_cast<float *>(ws + pair * ctcg_pair_words(T));
    int32_t *sv = reinterpret_cast<int32_t *>(reinterpret_cast<unsigned char *>(ev) + row);
    int32_t *fv = reinterpret_cast<int32_t *>(reinterpret_cast<unsigned char *>(ev) + 2 * row);

    // ---- B: the recursion
    if (len > 0) {
        int cls[SJ], lo[SJ], hi[SJ];
        bool live[SJ], first[SJ], last[SJ];
        float a[SJ], b[SJ];
        int sg[SJ], sbk[SJ];
        int my_last = 0;
#pragma unroll
        for (int j = 0; j < SJ; ++j) {
            const int s = lane + 64 * j;
            live[j] = s < P;
            cls[j] = live[j] ? pcls[s] : 0;
            const int f = live[j] ? pflags[s] : 0;
            first[j] = f & 1; last[j] = f & 2;
            my_last += last[j] ? 1 : 0;
            lo[j] = live[j] ? g.off[s] : 0;
            hi[j] = live[j] ? g.off[s + 1] : 0;
            a[j] = b[j] = -INFINITY; sg[j] = sbk[j] = -1;
        }
        const bool one_last = wave_sum((float)my_last) == 1.f;            // (wave-uniform) the usual case: no arg-max
        lattice_ring(x, C, mx, cls, 0, len, [&](int t, float (&cur)[SJ]) {            // cur: r_t(class(q)) of this lane's label states
            const float rblank = rb[t];
#pragma unroll
            for (int j = 0; j < SJ; ++j) {
                if (live[j]) {
                    const int s = lane + 64 * j;
                    g.xa[s] = CtcgCell{a[j], sg[j]}; g.xb[s] = CtcgCell{b[j], sbk[j]};
                }
            }
            ctcg_wave_fence();
            float be = -INFINITY;                 // this lane's best last state
            int bq = INT_MAX, bs = -1;
#pragma unroll
            for (int j = 0; j < SJ; ++j) {
                float best = a[j];
                int from = sg[j];
                for (int e = lo[j]; e < hi[j]; ++e) {
                    const int ent = g.ent[e], p = ent & 255;
                    const CtcgCell vb = g.xb[p], va = g.xa[p];
                    if (vb.d > best) { best = vb.d; from = vb.s; }
                    if ((ent & 256) && va.d > best) { best = va.d; from = va.s; }
                }
                if (first[j] && 0.f > best) { best = 0.f; from = t; }          // the fresh start
                float bb = b[j];
                int bf = sbk[j];
                if (a[j] > bb) { bb = a[j]; bf = sg[j]; }                      // the blank state: stay, then its label state
                a[j] = live[j] && best > -INFINITY ? best + cur[j] : -INFINITY;
                sg[j] = a[j] > -INFINITY ? from : -1;
                b[j] = live[j] && bb > -INFINITY ? bb + rblank : -INFINITY;
                sbk[j] = b[j] > -INFINITY ? bf : -1;
                if (last[j] && a[j] > be) { be = a[j]; bq = lane + 64 * j; bs = sg[j]; }      // (j ascends: the lane's lowest q wins a tie)
            }
            ctcg_wave_fence();                    // the reads above stay in front of the next frame's writes
            if (one_last) {
                if (my_last) { ev[t] = be; sv[t] = bs; fv[t] = be > -INFINITY ? bq : -1; }
            } else {
                float we = be;
                int wq = bq;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const float oe = __shfl_xor(we, d, 64);
                    const int oq = __shfl_xor(wq, d, 64);
                    if (oe > we || (oe == we && oq < wq)) { we = oe; wq = oq; }
                }
                if (wq == INT_MAX) { if (lane == 0) { ev[t] = -INFINITY; sv[t] = -1; fv[t] = -1; } }
                else if (be == we && bq == wq) { ev[t] = be; sv[t] = bs; fv[t] = bq; }
            }
        });
        if (!ET_LDS) __threadfence();                // the workspace words written above are read below by other lanes
        __threadfence_block();
    }

    // ---- C: the hits (lane k keeps hit k) -- ctc_spot_kernel's selection, the final state riding along
    int my_st = -1, my_en = -1, my_fin = -1, count = 0;
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
        if (lane == k) { my_st = st; my_en = bt; my_sc = be; my_fin = fv[bt]; }
        ++count;
        if (k + 1 == K) break;
        for (int u = lane; u < len; u += 64)
            if (ev[u] > -INFINITY && !(u < st || sv[u] > bt)) ev[u] = -INFINITY;
    }
    if (lane < K) {
        const size_t o = pair * K + lane;
        starts[o] = my_st; ends[o] = my_en; score[o] = my_sc; finals[o] = my_fin;
    }
    if (lane == 0) counts[pair] = count;
}

// et_lds: the candidate tables are in the `lds` bytes of dynamic LDS (then ws is not read).  The kernel's static LDS
// (COCR_GRAPH_STATIC_LDS) is large, so the limit raised for the dynamic part stays below 160 KB - static.
static inline hipError_t launch_ctc_spot_graph(hipStream_t s, int sj, bool et_lds, size_t lds, const float *logits, int N, int T, int C, const int32_t *lens,
                                               const int32_t *pat_states, const int32_t *state_off, const int32_t *edge_off, const int32_t *cls_all,
                                               const int32_t *flags_all, const int32_t *poff_all, const int32_t *preds_all, int Q, int K, float min_score,
                                               int32_t *starts, int32_t *ends, float *score, int32_t *finals, int32_t *counts, unsigned *ws) {
    return with_sj(sj, [&](auto SJ) {
        constexpr int sjv = decltype(SJ)::value > 4 ? 4 : decltype(SJ)::value;           // (a pattern holds at most 256 label states)
        auto go = [&](auto kern) {
            const hipError_t e = raise_lds_limit((const void *)kern, lds, 8 * 1024, 104 * 1024);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(kern, dim3((Q + 3) / 4, N), dim3(256), lds, s, logits, T, C, lens, pat_states, state_off, edge_off, cls_all, flags_all, poff_all,
                               preds_all, Q, K, min_score, starts, ends, score, finals, counts, ws);
            return hipSuccess;
        };
        return et_lds ? go(ctc_spot_graph_kernel<sjv, true>) : go(ctc_spot_graph_kernel<sjv, false>);
    });
}
