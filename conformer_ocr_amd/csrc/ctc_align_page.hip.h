// Text-to-page alignment: the best path of a page's running text through the frames of its lines in reading
// order -- forced alignment (ctc_align.hip.h) over the concatenated frames, with the two rules of a line break.  The definition is
// align.viterbi_align_page; t counts the page's frames, a BREAK frame is the first frame of a line k >= 1 that has frames:
//   delta_0(0) = lp_0(blank), delta_0(1) = lp_0(l'_1);  delta_t(s) = best + lp_t(l'_s), the candidates tried in this order, a later
//   one replacing the running best only when STRICTLY greater:
//     0  delta_{t-1}(s)      -- not for an odd s at a break frame: a label never spans two lines;
//     1  delta_{t-1}(s-1);
//     2  delta_{t-1}(s-2)    odd s >= 3, if l'_s != l'_{s-2} or t is a break frame;
//     3  delta_{t-1}(s-3)    odd s >= 5 whose label s-2 is optional (the blank before the skipped label);
//     4  delta_{t-1}(s-4)    odd s >= 5 whose label s-2 is optional, if l'_s != l'_{s-4} or t is a break frame;
//   end state S-1, or S-2 when strictly greater.
// Per page (one workgroup of NW <= 16 waves, launched with exactly the waves the call's largest S needs):
//   A  lz of every valid frame of the page's lines (all waves, one frame per wave at a time; row_max / row_lse) -> LDS, or the page's
//      workspace region when the call's longest page does not fit; the log-softmax is never stored.
//   B  the recursion with all states in registers: wave w, register j, lane l hold state (w SJ + j) 64 + l.  Neighbours s-1 .. s-4 by
//      four lane rotations per register, the previous register's at the register seam; across a wave seam each wave publishes its
//      top four delta into a double-buffered LDS slot (frame parity) and the workgroup takes ONE barrier per frame: a wave reads slot
//      (t-1) & 1 and writes slot t & 1, which nobody reads before the barrier that ends frame t.  Every wave walks the same lines and
//      frames (the line table is read uniformly), so every wave executes every barrier.  The gathered logits are requested ahead
//      line by line in a register ring as lattice_ring does (4 frames ahead).  Back-pointers: the compare chain's outcome 0..4,
//      8 frames x 4 bits per word and state, bp[(t >> 3) SP + s] in the page's workspace region (SP = 64 SJ NW).  VGPRs 43 / 57 /
//      79 / 128 and no scratch for SJ = 1 / 2 / 4 / 8 (tests/test_align_page_kernel.py holds the scratch at 0).  16 waves leave 128
//      registers per lane: a form of 16 registers per lane (texts of 4096 .. 8191 labels) spilled and is not offered; such texts go
//      through the host definition.
//   C  traceback on wave 0: per block of 8 frames ONE wave-wide read (lane i takes the word of state s - i: at most 4 states per frame,
//      32 per block), then 8 scalar steps; lane 0 writes the state of every frame and the first / last frame of every label's run.
//   D  thread k for label k: line (binary search in the line starts), start / end within it, conf = exp of the largest lp over the run.
//      Then the line scores, wave w for lines w, w + NW, ..: lane l adds the frames l, l + 64, .. of the line in ascending order into
//      one float, and the 64 partial sums go through wave_sum's DPP tree -- one fixed order of summation.
// The page's region of the workspace: [bp: ceil(sumT / 8) SP][lz: sumT][state per frame: sumT][run first: L][run last: L] words.
// Every loop is bounded by the page's tables; no spin waits, no flags, nothing waits on another workgroup, no atomics.
#pragma once
#include "ctc_lattice.hip.h"

#define COCR_PAGE_MAX_LABELS 4095       // 2 L + 1 <= 16 waves x 8 registers x 64 lanes
#define COCR_PAGE_MAX_FRAMES 65535
#define COCR_PAGE_MAX_LINES 4096
#define COCR_PAGE_MAX_WAVES 16
#define COCR_PAGE_MAX_CLASSES (1 << 22) // a state's class (as a byte offset) and its flags share a register
#define COCR_PAGE_OPTIONAL 0x40000000   // set in an uploaded label word: the label may be skipped
#define COCR_PAGE_LZ_LDS_FRAMES 24576   // lz lives in LDS (96 KB) up to this many frames per page

// the kernel form for a call whose largest page has `states` states: registers per lane, then exactly the waves it needs
static inline int page_sj_for_states(int states) {
    int sj = 1;
    while (sj < 8 && COCR_PAGE_MAX_WAVES * 64 * sj < states) sj *= 2;
    return sj;
}
static inline int page_waves_for_states(int states, int sj) { return std::max(1, (states + 64 * sj - 1) / (64 * sj)); }
// words of one page's workspace region; sp = 64 sj waves
static inline size_t page_region_words(int frames, int labels, int sp) { return (size_t)((frames + 7) / 8) * sp + 2 * (size_t)frames + 2 * (size_t)labels; }

template <int SJ>
__global__ __launch_bounds__(1024) void ctc_align_page_kernel(const float *__restrict__ logits, int T, int C, const int32_t *__restrict__ pl_off,
                                                              const int32_t *__restrict__ rows, const int32_t *__restrict__ first_all,
                                                              const int32_t *__restrict__ label_off, const int32_t *__restrict__ labels,
                                                              const uint32_t *__restrict__ ws_off, unsigned *__restrict__ ws, int lz_lds,
                                                              int32_t *__restrict__ o_line, int32_t *__restrict__ o_start, int32_t *__restrict__ o_end,
                                                              float *__restrict__ o_conf, float *__restrict__ o_score, int32_t *__restrict__ o_counts,
                                                              float *__restrict__ o_line_score) {
    enum { OFS = 0xFFFFFF, LIVE = 1 << 24, ODD3 = 1 << 25, DIFF2 = 1 << 26, OVER = 1 << 27, DIFF4 = 1 << 28 };
    auto at = [](const float *r, int f) { return *reinterpret_cast<const float *>(reinterpret_cast<const char *>(r) + (f & OFS)); };   // r[class of f]
    constexpr int PF = COCR_LATTICE_PF;                     // frames requested ahead
    extern __shared__ __attribute__((aligned(16))) unsigned char ctcp_smem[];
    __shared__ __attribute__((aligned(16))) float seam[2][COCR_PAGE_MAX_WAVES][4];
    __shared__ float fin[2];
    __shared__ int sh_ok;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), NW = nthr >> 6;
    const int SP = 64 * SJ * NW;
    const int K = pl_off[p + 1] - pl_off[p];
    const int32_t *row = rows + pl_off[p];
    const int32_t *first = first_all + pl_off[p] + p;            // K + 1 entries: first frame of every line, then sumT
    const int total = first[K];
    const int loff = label_off[p], L = label_off[p + 1] - loff;
    const int32_t *lab = labels + loff;
    const int S = 2 * L + 1;
    unsigned *bp = ws + ws_off[p];
    float *lz_ws = reinterpret_cast<float *>(bp + (size_t)((total + 7) / 8) * SP);
    int32_t *path = reinterpret_cast<int32_t *>(lz_ws + total), *run_st = path + total, *run_en = run_st + L;
    // lz through address-space-typed pointers: a pointer that may be either makes every read a flat load, which waits for ALL loads in
    // flight -- the requests the ring has out for the frames ahead included
    typedef __attribute__((address_space(3))) float lds_float;
    typedef __attribute__((address_space(1))) float global_float;
    lds_float *lz_s = (lds_float *)ctcp_smem;
    global_float *lz_g = (global_float *)lz_ws;
    auto lz = [&](int g) { return lz_lds ? (float)lz_s[g] : (float)lz_g[g]; };

    for (int k = tid; k < L; k += nthr) { run_st[k] = -1; run_en[k] = -1; }
    // ---- A: the per-frame normaliser
    for (int k = 0; k < K; ++k) {
        const int g0 = first[k], len = first[k + 1] - g0;
        const float *x = logits + (size_t)row[k] * T * C;
        for (int t = wave; t < len; t += NW) {
            const float *xt = x + (size_t)t * C;
            const float l = row_lse(xt, C, lane, row_max(xt, C, lane));
            if (lane == 0) { if (lz_lds) lz_s[g0 + t] = l; else lz_g[g0 + t] = l; }
        }
    }
    if (lane < 4) { seam[0][wave][lane] = -INFINITY; seam[1][wave][lane] = -INFINITY; }
    if (!lz_lds) __threadfence();
    __syncthreads();

    // ---- B: the recursion
    if (total > 0) {
        int cf[SJ];                                  // the byte offset of the state's class in a frame, its flags above OFS
        float a[SJ];
        unsigned acc[SJ];
        const bool odd = lane & 1;
#pragma unroll
        for (int j = 0; j < SJ; ++j) {
            const int s = (wave * SJ + j) * 64 + lane, k = s >> 1;
            const bool live = s < S, on = live && odd;
            int w0 = 0, w1 = 0, w2 = 0;
            if (on) { w0 = lab[k]; if (k >= 1) w1 = lab[k - 1]; if (k >= 2) w2 = lab[k - 2]; }
            const int c0 = w0 & ~COCR_PAGE_OPTIONAL, c1 = w1 & ~COCR_PAGE_OPTIONAL, c2 = w2 & ~COCR_PAGE_OPTIONAL;
            const bool over = on && k >= 2 && (w1 & COCR_PAGE_OPTIONAL);
            cf[j] = (c0 << 2) | (live ? LIVE : 0) | (on && k >= 1 ? ODD3 : 0) | (on && k >= 1 && c0 != c1 ? DIFF2 : 0) | (over ? OVER : 0) | (over && c0 != c2 ? DIFF4 : 0);
            a[j] = -INFINITY;
            acc[j] = 0u;
        }
        const int src1 = (lane + 63) & 63, src2 = (lane + 62) & 63, src3 = (lane + 61) & 63, src4 = (lane + 60) & 63;
        bool started = false;
        for (int k = 0; k < K; ++k) {
            const int g0 = first[k], len = first[k + 1] - g0;
            if (len == 0) continue;
            const float *x = logits + (size_t)row[k] * T * C;
            if (!started) {                          // the page's first frame
#pragma unroll
                for (int j = 0; j < SJ; ++j) {
                    const int s = (wave * SJ + j) * 64 + lane;
                    a[j] = ((cf[j] & LIVE) && s < 2) ? at(x, cf[j]) - lz(g0) : -INFINITY;
                }
                if (lane >= 60) seam[0][wave][lane - 60] = a[SJ - 1];
                __syncthreads();
            }
            // the gathered logits and lz of the next PF frames of the line, requested PF steps ahead (lattice_ring's scheme; a ring of
            // this kernel's own, as a step consumes a register of it and requests the next in place: no second array of SJ values)
            const int t_first = started ? 0 : 1;
            float nx[PF][SJ], nz[PF];
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                const int tt = min(t_first + u, len - 1);
                nz[u] = lz(g0 + tt);
#pragma unroll
                for (int j = 0; j < SJ; ++j) nx[u][j] = at(x + (size_t)tt * C, cf[j]);
            }
            for (int t0 = t_first; t0 < len; t0 += PF) {
#pragma unroll
                for (int u = 0; u < PF; ++u) {
                    const int t = t0 + u;
                    if (t < len) {                    // uniform: every wave walks the same frames
                        const int g = g0 + t, tn = min(t + PF, len - 1);
                        const bool brk = t == 0;      // (the page's first frame takes no step)
                        float p1 = -INFINITY, p2 = -INFINITY, p3 = -INFINITY, p4 = -INFINITY;
                        if (wave > 0) {               // the previous wave's top four states
                            const float4 q = *reinterpret_cast<const float4 *>(seam[(g - 1) & 1][wave - 1]);
                            p1 = q.w;
                            p2 = lane == 0 ? q.z : q.w;
                            p3 = lane == 0 ? q.y : lane == 1 ? q.z : q.w;
                            p4 = lane == 0 ? q.x : lane == 1 ? q.y : lane == 2 ? q.z : q.w;
                        }
                        const int sh = 4 * (g & 7);
                        const bool flush = (g & 7) == 7 || g == total - 1;
                        const float z = nz[u];
                        nz[u] = lz(g0 + tn);
                        const float *xn = x + (size_t)tn * C;
#pragma unroll
                        for (int j = 0; j < SJ; ++j) {
                            const float r1 = __shfl(a[j], src1, 64), r2 = __shfl(a[j], src2, 64), r3 = __shfl(a[j], src3, 64), r4 = __shfl(a[j], src4, 64);
                            const float n1 = lane >= 1 ? r1 : p1, n2 = lane >= 2 ? r2 : p2, n3 = lane >= 3 ? r3 : p3, n4 = lane >= 4 ? r4 : p4;
                            p1 = r1; p2 = r2; p3 = r3; p4 = r4;
                            const int f = cf[j];
                            const float e = nx[u][j] - z;          // lp_t(l'_s)
                            nx[u][j] = at(xn, f);
                            float best = (brk && odd) ? -INFINITY : a[j];
                            unsigned code = 0u;
                            if (n1 > best) { best = n1; code = 1u; }
                            if (((f & DIFF2) || (brk && (f & ODD3))) && n2 > best) { best = n2; code = 2u; }
                            if ((f & OVER) && n3 > best) { best = n3; code = 3u; }
                            if ((f & OVER) && ((f & DIFF4) || brk) && n4 > best) { best = n4; code = 4u; }
                            a[j] = (f & LIVE) ? best + e : -INFINITY;
                            acc[j] |= code << sh;
                            if (flush) {
                                if (f & LIVE) bp[(size_t)(g >> 3) * SP + (wave * SJ + j) * 64 + lane] = acc[j];
                                acc[j] = 0u;
                            }
                        }
                        if (lane >= 60) seam[g & 1][wave][lane - 60] = a[SJ - 1];
                        __syncthreads();
                    }
                }
            }
            started = true;
        }
#pragma unroll
        for (int j = 0; j < SJ; ++j) {
            const int s = (wave * SJ + j) * 64 + lane;
            if (s == S - 1) fin[0] = a[j];
            if (S > 1 && s == S - 2) fin[1] = a[j];
        }
    }
    __threadfence();                                 // the back-pointer words are read below by wave 0
    __syncthreads();

    // ---- C: the traceback (wave 0)
    if (wave == 0) {
        int ok = (total == 0 && L == 0) ? 1 : 0;
        float best_score = ok ? 0.f : -INFINITY;
        if (total > 0) {
            int s = S - 1;
            if (S > 1 && fin[1] > fin[0]) s = S - 2;
            best_score = s == S - 1 ? fin[0] : fin[1];
            ok = best_score != -INFINITY;
            if (ok) {
                s = __builtin_amdgcn_readfirstlane(s);
                int last = total - 1;                // last frame of the run the walk is in
                for (int blk = (total - 1) >> 3; blk >= 0; --blk) {
                    const int s0 = s, sl = s0 - lane;
                    const unsigned w = sl >= 0 ? bp[(size_t)blk * SP + sl] : 0u;
                    const int t_hi = min(total - 1, 8 * blk + 7), t_lo = max(8 * blk, 1);
                    for (int t = t_hi; t >= t_lo; --t) {
                        if (lane == 0) path[t] = s;
                        const unsigned word = (unsigned)__builtin_amdgcn_readlane((int)w, s0 - s);
                        const int code = (int)((word >> (4 * (t & 7))) & 7u);
                        if (code) {                  // frame t is the first of state s
                            if ((s & 1) && lane == 0) { run_st[s >> 1] = t; run_en[s >> 1] = last; }
                            s = __builtin_amdgcn_readfirstlane(s - code);
                            last = t - 1;
                        }
                    }
                }
                if (lane == 0) {
                    path[0] = s;
                    if (s & 1) { run_st[s >> 1] = 0; run_en[s >> 1] = last; }
                }
            }
        }
        if (lane == 0) {
            sh_ok = ok;
            o_score[p] = best_score;
            o_counts[p] = ok ? L : -1;
        }
    }
    __threadfence();                                 // the states and runs written by wave 0 are read below by every thread
    __syncthreads();

    // ---- D: the records and the line scores
    const bool ok = sh_ok != 0;
    for (int k = tid; k < L; k += nthr) {
        int ln = -1, st = -1, en = -1;
        float cf = 0.f;
        const int gs = ok ? run_st[k] : -1;
        if (gs >= 0) {
            int lo = 0, hi = K - 1;                  // the last line whose first frame is <= gs (lines of no frames before it share its start and lose)
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (first[mid] <= gs) lo = mid; else hi = mid - 1;
            }
            ln = lo;
            const int g0 = first[ln], ge = run_en[k], c = lab[k] & ~COCR_PAGE_OPTIONAL;
            const float *x = logits + (size_t)row[ln] * T * C;
            float mx = -INFINITY;
            for (int g = gs; g <= ge; ++g) mx = fmaxf(mx, x[(size_t)(g - g0) * C + c] - lz(g));
            cf = expf(mx);
            st = gs - g0; en = ge - g0;
        }
        o_line[loff + k] = ln; o_start[loff + k] = st; o_end[loff + k] = en; o_conf[loff + k] = cf;
    }
    for (int k = wave; k < K; k += NW) {
        const int g0 = first[k], len = first[k + 1] - g0;
        const float *x = logits + (size_t)row[k] * T * C;
        float sum = 0.f;
        if (ok)
            for (int t = lane; t < len; t += 64) {
                const int s = path[g0 + t];
                const int c = (s & 1) ? (lab[s >> 1] & ~COCR_PAGE_OPTIONAL) : 0;
                sum += x[(size_t)t * C + c] - lz(g0 + t);
            }
        sum = wave_sum(sum);
        if (lane == 0) o_line_score[pl_off[p] + k] = ok ? sum : -INFINITY;
    }
}

// One workgroup of `waves` waves per page; lds: the bytes of lz in dynamic LDS (0: lz in the workspace).
static inline hipError_t launch_ctc_align_page(hipStream_t s, int sj, int waves, size_t lds, const float *logits, int P, int T, int C, const int32_t *pl_off,
                                               const int32_t *rows, const int32_t *first, const int32_t *label_off, const int32_t *labels,
                                               const uint32_t *ws_off, unsigned *ws, int32_t *o_line, int32_t *o_start, int32_t *o_end, float *o_conf,
                                               float *o_score, int32_t *o_counts, float *o_line_score) {
    return with_sj(sj, [&](auto SJ) {
        auto kern = ctc_align_page_kernel<decltype(SJ)::value>;
        const hipError_t e = raise_lds_limit((const void *)kern, lds, 48 * 1024, 128 * 1024);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(P), dim3(64 * waves), lds, s, logits, T, C, pl_off, rows, first, label_off, labels, ws_off, ws, lds ? 1 : 0, o_line, o_start,
                           o_end, o_conf, o_score, o_counts, o_line_score);
        return hipSuccess;
    });
}
