// The pieces the CTC lattice kernels share (DESIGN.md "The lattice kernels' shared pieces"): the criterion (ctc_loss.hip.h), forced
// alignment (ctc_align.hip.h) and keyword spotting (ctc_spot.hip.h) walk the same machine, and the beam kernels (ctc.hip.h,
// ctc_lm.hip.h) take their frame statistics from here.
//   * a label sequence spread over ONE wave: state s on lane s & 63, register s >> 6, SJ in {1, 2, 4, 8} registers per lane;
//   * the neighbours s-1 / s-2 (backward: s+1 / s+2) of a step by two lane rotations per register (lattice_rotate) and a select at
//     the register seam (lattice_seam_fwd / _bwd): nothing goes through memory inside the T-step dependent chain;
//   * cls / skip / live of a lane's states (lattice_states);
//   * the next PF = 4 frames' gathered logits requested ahead in a register ring (lattice_ring);
//   * a frame's maximum and log-sum-exp in ONE order of summation (row_max, row_lse): what makes lp bit-identical between kernels;
//   * the SJ dispatch of the host side (sj_for_states, with_sj) and the launch that raises a kernel's LDS limit first (lattice_launch).
// Each kernel keeps its own body and its own step arithmetic (log-sum-exp of three / max + back-pointer code / max + carried start).
// Helpers take register arrays by reference and the hoisted lane indices as arguments: everything unrolls into the caller.
#pragma once
#include "common.hip.h"

#include <type_traits>

#define COCR_LATTICE_MAX_LABELS 255     // per sequence: at most 2 L + 1 <= 512 states = 8 registers of a wave
#define COCR_LATTICE_PF 4               // frames requested ahead by lattice_ring

// T four-byte values in dynamic LDS (or in a workspace region), padded to 16 bytes
__host__ __device__ static inline size_t lattice_row_bytes(int T) { return ((size_t)T * 4 + 15) & ~(size_t)15; }

// ---- frame statistics: lanes stride the classes, DPP trees (common.hip.h); the result is uniform in the wave
__device__ __forceinline__ float row_max(const float *x, int C, int lane) {
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, x[c]);
    return wave_max(mx);
}
// log sum_c exp(x[c]), given mx = row_max(x)
__device__ __forceinline__ float row_lse(const float *x, int C, int lane, float mx) {
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += expf(x[c] - mx);
    return mx + logf(wave_sum(sum));
}

// ---- neighbour exchange
// the lanes that hold state s-1 / s-2 (forward) or s+1 / s+2 (backward) of this lane's states, seams aside
__device__ __forceinline__ void lattice_src_fwd(int lane, int &src1, int &src2) { src1 = (lane + 63) & 63; src2 = (lane + 62) & 63; }
__device__ __forceinline__ void lattice_src_bwd(int lane, int &src1, int &src2) { src1 = (lane + 1) & 63; src2 = (lane + 2) & 63; }

template <int SJ, class V>
__device__ __forceinline__ void lattice_rotate(const V (&a)[SJ], V (&r1)[SJ], V (&r2)[SJ], int src1, int src2) {
#pragma unroll
    for (int j = 0; j < SJ; ++j) { r1[j] = __shfl(a[j], src1, 64); r2[j] = __shfl(a[j], src2, 64); }
}
// The seam select for register j (a constant once the caller's loop is unrolled).  r: `a` rotated down by d (1 or 2) lanes: lanes
// below d take the previous register's lanes 64 - d .., in register 0 `edge`.
template <int SJ, class V>
__device__ __forceinline__ V lattice_seam_fwd(const V (&r)[SJ], int j, int lane, int d, V edge) {
    return lane >= d ? r[j] : (j > 0 ? r[j > 0 ? j - 1 : 0] : edge);
}
// r: `a` rotated up by d lanes: lanes from 64 - d on take the next register's lanes 0 .., in the last register `edge`.
template <int SJ, class V>
__device__ __forceinline__ V lattice_seam_bwd(const V (&r)[SJ], int j, int lane, int d, V edge) {
    return lane < 64 - d ? r[j] : (j + 1 < SJ ? r[j + 1 < SJ ? j + 1 : 0] : edge);
}

// ---- a lane's states.  Labels sit on the states of parity PARITY, blanks between them: PARITY 1 with S = 2 L + 1 is the blank-extended
// sequence of the criterion and of alignment (blanks outside), PARITY 0 with S = 2 L - 1 the query of the spotter (none outside).
// cls: the state's class (0 for a blank and for a dead state); live: s < S; skip: the edge from s-2 exists (the two labels differ), or
// with `backward` the edge from s+2.
template <int SJ, int PARITY>
__device__ __forceinline__ void lattice_states(const int32_t *lab, int S, int lane, bool backward, int (&cls)[SJ], bool (&skip)[SJ], bool (&live)[SJ]) {
#pragma unroll
    for (int j = 0; j < SJ; ++j) {
        const int s = lane + 64 * j;
        live[j] = s < S;
        const int k = (s - PARITY) >> 1;
        const bool on_label = (s & 1) == PARITY;
        cls[j] = (live[j] && on_label) ? lab[k] : 0;
        if (!backward) skip[j] = live[j] && on_label && s >= 2 + PARITY && lab[k] != lab[k - 1];
        else skip[j] = on_label && s + 2 < S && lab[k] != lab[k + 1];
    }
}

// ---- the prefetch ring.  Runs step(t, cur) for t = first .. len - 1 with cur[j] = x[t, cls[j]] - stat[t].  The logits and the frame
// statistic of the next PF frames are requested PF steps ahead (a ring in registers; every lane loads, a dead state the blank's; beyond
// the line the last frame again) and subtracted only when their step begins: a step never waits for a load it has just issued.
template <int SJ, class Step>
__device__ __forceinline__ void lattice_ring(const float *x, int C, const float *stat, const int (&cls)[SJ], int first, int len, Step &&step) {
    constexpr int PF = COCR_LATTICE_PF;
    float nx[PF][SJ], nz[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const int tt = min(first + u, len - 1);
        nz[u] = stat[tt];
#pragma unroll
        for (int j = 0; j < SJ; ++j) nx[u][j] = x[(size_t)tt * C + cls[j]];
    }
    int t0 = first;
    for (; t0 + PF <= len; t0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            float cur[SJ];
#pragma unroll
            for (int j = 0; j < SJ; ++j) cur[j] = nx[u][j] - nz[u];
            const int tt = min(t0 + u + PF, len - 1);
            nz[u] = stat[tt];
#pragma unroll
            for (int j = 0; j < SJ; ++j) nx[u][j] = x[(size_t)tt * C + cls[j]];
            step(t0 + u, cur);
        }
    }
#pragma unroll
    for (int u = 0; u < PF - 1; ++u) {               // the last len - t0 < PF frames are in the ring already
        if (t0 + u < len) {
            float cur[SJ];
#pragma unroll
            for (int j = 0; j < SJ; ++j) cur[j] = nx[u][j] - nz[u];
            step(t0 + u, cur);
        }
    }
}

// ---- host side: the kernel form for `states` states, and the one switch over it.  f takes std::integral_constant<int, SJ>.
static inline int sj_for_states(int states) { return states <= 64 ? 1 : states <= 128 ? 2 : states <= 256 ? 4 : 8; }

template <class F> static inline auto with_sj(int sj, F &&f) {
    switch (sj) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 8>{});
    }
}

// One workgroup of four waves per grid entry.  The limit is raised for the very kernel that is launched; a kernel with a table in
// dynamic LDS has ~5 KB of static LDS too: the limit raised for the dynamic part stays below 160 KB - static.
template <class... P, class... A>
static inline hipError_t lattice_launch(void (*kern)(P...), dim3 grid, size_t lds, hipStream_t s, A... args) {
    const hipError_t e = raise_lds_limit((const void *)kern, lds, 48 * 1024, 150 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, args...);
    return hipSuccess;
}
