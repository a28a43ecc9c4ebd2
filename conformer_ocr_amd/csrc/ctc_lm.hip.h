// CTC prefix beam search with a character n-gram language model in the ranking (the definition is
// conformer_ocr_amd/lm.py beam_decode_host).  The recurrences, folding, creation order, starts, ends and conf are those of
// ctc_beam_kernel (ctc.hip.h); a frame's candidate classes are blank + its K best non-blank classes, every prefix carries
// lmv = sum over its labels of alpha * lm(context, label) + beta, and candidates rank by logaddexp(p_b, p_nb) + lmv.  The static
// pruning of ctc_beam_walk_kernel does not hold with a per-(prefix, class) term, so all beam x K extensions are scored.
//   * ctc_lm_topk_kernel: one wave per frame of the whole batch, any class count: max / log Z by the row_max / row_lse that
//     ctc_beam_kernel calls (so lp is bit-identical to the plain beam's), then K rounds of "largest key below the last one" for the
//     K best non-blank classes (ties: smaller class).  Record per frame: lp[blank], log Z, max, K x (class, lp).
//   * ctc_lm_walk_kernel: one workgroup of 256 threads per line, prefix state double-buffered in LDS (the last 7 labels of each
//     prefix as 16-bit values).  Per frame: extension candidate (i, r) -> one thread each (tid, tid + 256, ..): score, fold test,
//     LM lookup; barrier; the stay candidates (last wave); barrier; every candidate's rank = the number of larger 64-bit keys
//     ((score image) << 32 | ~position: unique); the candidate of rank R < beam writes next frame's prefix R; barrier.
//   * LM lookup: the first probe of every level's n-gram and context key is issued at once (the keys are the running values of
//     one multiply-add chain over the context, newest label first), then resolved from the longest level down, first hit wins;
//     only a first probe that meets a foreign key continues linearly.  Every probe loop stops at an empty slot or after `slots`
//     probes.
#pragma once
#include "ctc.hip.h"

#define COCR_LM_KMAX 64                 // candidate classes per frame
#define COCR_LM_CTX 7                   // labels of context kept per prefix (order <= 8)
#define COCR_LM_REC 132                 // dwords per frame record: lp[0], log Z, max, pad, class[64], lp[64]
#define COCR_LM_NE (COCR_BEAM_MAX * COCR_LM_KMAX)

struct cocr_lm_tables {
    const float *unigram;               // [ncls]
    const unsigned long long *nkeys;    // n-grams of order >= 2: open addressing, key 0 = empty
    const float *nlogp;
    const unsigned long long *ckeys;    // contexts of length >= 1
    const float *cbow;
    unsigned nmask, cmask;              // slots - 1
    int order;
};

// hash scheme "fnv-chain/splitmix64-v1": h_0 = offset basis, h_k = h_{k-1} * prime + (label_k + 1) with label_1 the NEWEST label of
// the context; key(level k, class c) = splitmix64 finalizer of h_k ^ c * golden ^ k * odd (c = 0: the context itself), 0 -> 1.
__host__ __device__ __forceinline__ unsigned long long lm_key(unsigned long long h, unsigned c, unsigned k) {
    unsigned long long z = h ^ ((unsigned long long)c * 0x9E3779B97F4A7C15ull) ^ ((unsigned long long)k * 0xD6E8FEB86659FD93ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z ? z : 1ull;
}

// continues a probe sequence after a first probe that met a foreign key; bounded by the slot count
__device__ __noinline__ bool lm_probe_rest(const unsigned long long *__restrict__ keys, const float *__restrict__ vals, unsigned mask,
                                           unsigned long long key, float &val) {
    unsigned slot = (unsigned)key & mask;
    for (unsigned p = 1; p <= mask; ++p) {
        slot = (slot + 1u) & mask;
        const unsigned long long g = keys[slot];
        if (g == key) { val = vals[slot]; return true; }
        if (g == 0ull) return false;
    }
    return false;
}

// lm(ctx, c): ctx[0] is the newest label, 0 = no label
__device__ __forceinline__ float lm_lookup(const cocr_lm_tables &L, const unsigned short (&ctx)[8], int c) {
    int kmax = 0;
#pragma unroll
    for (int k = 0; k < COCR_LM_CTX; ++k) kmax += (k < L.order - 1 && ctx[k] != 0) ? 1 : 0;      // (labels fill ctx from the front)
    unsigned long long kn[COCR_LM_CTX], kc[COCR_LM_CTX], gn[COCR_LM_CTX], gc[COCR_LM_CTX];
    float vn[COCR_LM_CTX], vc[COCR_LM_CTX];
    unsigned long long h = COCR_HASH_SEED;
    const float uni = L.unigram[c];
#pragma unroll
    for (int k = 0; k < COCR_LM_CTX; ++k) {
        kn[k] = kc[k] = gn[k] = gc[k] = 0ull; vn[k] = vc[k] = 0.f;
        if (k < kmax) {
            h = h * COCR_HASH_PRIME + (unsigned long long)(ctx[k] + 1);
            kn[k] = lm_key(h, (unsigned)c, (unsigned)(k + 1));
            kc[k] = lm_key(h, 0u, (unsigned)(k + 1));
            const unsigned sn = (unsigned)kn[k] & L.nmask, sc = (unsigned)kc[k] & L.cmask;
            gn[k] = L.nkeys[sn]; vn[k] = L.nlogp[sn];
            gc[k] = L.ckeys[sc]; vc[k] = L.cbow[sc];
        }
    }
    float acc = 0.f;
#pragma unroll
    for (int k = COCR_LM_CTX - 1; k >= 0; --k) {
        if (k < kmax) {
            float v = vn[k];
            bool hit = gn[k] == kn[k];
            if (!hit && gn[k] != 0ull) hit = lm_probe_rest(L.nkeys, L.nlogp, L.nmask, kn[k], v);
            if (hit) return __fadd_rn(acc, v);
            v = vc[k];
            hit = gc[k] == kc[k];
            if (!hit && gc[k] != 0ull) hit = lm_probe_rest(L.ckeys, L.cbow, L.cmask, kc[k], v);
            if (hit) acc = __fadd_rn(acc, v);
        }
    }
    return __fadd_rn(acc, uni);
}

__global__ __launch_bounds__(256) void ctc_lm_topk_kernel(const float *__restrict__ logits, int T, int C, int frames, const int32_t *__restrict__ lens,
                                                          int K, float *__restrict__ rec_all) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);          // frame index n * T + t: one wave each
    if (f >= frames) return;
    const int n = f / T, t = f - n * T;
    if (t >= min(max(lens[n], 0), T)) return;
    const float *lg = logits + (size_t)f * C;
    float *rec = rec_all + (size_t)f * COCR_LM_REC;
    const float mx = row_max(lg, C, lane), lz = row_lse(lg, C, lane, mx);
    if (lane == 0) { rec[0] = (lg[0] - mx) - (lz - mx); rec[1] = lz; rec[2] = mx; rec[3] = 0.f; }
    unsigned long long bound = ~0ull;                           // the last round's key: this round takes the largest key below it
    for (int r = 0; r < K; ++r) {
        unsigned long long best = 0ull;
        for (int c = lane; c < C; c += 64) {
            if (c == 0) continue;
            const unsigned long long key = beam_key((lg[c] - mx) - (lz - mx), (unsigned)c);
            if (key < bound && key > best) best = key;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long ok = __shfl_xor(best, o, 64);
            if (ok > best) best = ok;
        }
        bound = best;
        if (lane == 0) {
            const int c = best ? (int)(0xFFFFFFFFu - (unsigned)best) : 0;                         // 0 = no further class with a finite score
            reinterpret_cast<int32_t *>(rec)[4 + r] = c;
            rec[4 + COCR_LM_KMAX + r] = c ? (lg[c] - mx) - (lz - mx) : -INFINITY;
        }
        if (best == 0ull) {                                     // (the remaining slots stay empty)
            if (lane == 0) for (int r2 = r + 1; r2 < K; ++r2) { reinterpret_cast<int32_t *>(rec)[4 + r2] = 0; rec[4 + COCR_LM_KMAX + r2] = -INFINITY; }
            break;
        }
    }
}

struct lm_prefix_state {                                        // live prefixes of one frame, rank order; a dead slot has tot = -inf
    unsigned long long hash[COCR_BEAM_MAX];
    uint4 ctx[COCR_BEAM_MAX];                                   // 8 x u16: the last labels, newest first, 0 = none
    float pb[COCR_BEAM_MAX], pnb[COCR_BEAM_MAX], tot[COCR_BEAM_MAX], lmv[COCR_BEAM_MAX];
    int last[COCR_BEAM_MAX];
};

__global__ __launch_bounds__(256) void ctc_lm_walk_kernel(const float *__restrict__ logits, int T, int C, const int32_t *__restrict__ lens, int beam, int K,
                                                          cocr_lm_tables L, float alpha, float beta,
                                                          int32_t *__restrict__ labels, int32_t *__restrict__ starts, int32_t *__restrict__ ends,
                                                          float *__restrict__ conf, int32_t *__restrict__ counts, float *__restrict__ score, int max_per_line,
                                                          const float *__restrict__ rec_all, int32_t *__restrict__ bp_gbl, int bp_in_lds) {
    constexpr int NB = COCR_BEAM_MAX, STAY0 = 256 - NB;
    __shared__ __attribute__((aligned(16))) unsigned long long ckey[COCR_LM_NE + NB];             // extensions [0, NE), stays [NE, NE + beam), one zero pad
    __shared__ __attribute__((aligned(16))) lm_prefix_state st[2];
    __shared__ __attribute__((aligned(16))) float clmv[COCR_LM_NE], recs[2][COCR_LM_REC], spb[NB], spnb[NB], mval[NB];
    __shared__ int mpos[NB], sbp[NB], s_cnt, s_next;
    extern __shared__ __attribute__((aligned(16))) unsigned char lm_dyn[];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int len = min(max(lens[n], 0), T);
    const float *lg = logits + (size_t)n * T * C;
    const float *rec = rec_all + (size_t)n * T * COCR_LM_REC;
    int32_t *bpl = reinterpret_cast<int32_t *>(lm_dyn);                        // [T][beam]
    int32_t *bpg = bp_gbl + (size_t)n * T * NB;                                // [T][NB]
    const int NE = beam * K, NC = NE + beam, NCP = (NC + 1) & ~1;

    if (tid < NB) {
        const bool root = tid == 0;
        lm_prefix_state &s = st[0];
        s.hash[tid] = root ? COCR_HASH_SEED : 0ull; s.ctx[tid] = make_uint4(0u, 0u, 0u, 0u);
        s.pb[tid] = root ? 0.f : -INFINITY; s.pnb[tid] = -INFINITY; s.tot[tid] = root ? 0.f : -INFINITY; s.lmv[tid] = 0.f; s.last[tid] = 0;
        mval[tid] = -INFINITY; mpos[tid] = 0x7fffffff;
    }
    for (int j = tid; j < COCR_LM_NE + NB; j += 256) ckey[j] = 0ull;
    if (tid < COCR_LM_REC && len > 0) recs[0][tid] = rec[tid];
    __syncthreads();

    for (int t = 0; t < len; ++t) {
        const lm_prefix_state &cur = st[t & 1];
        lm_prefix_state &nxt = st[(t + 1) & 1];
        const float *rc = recs[t & 1];
        const int32_t *tcc = reinterpret_cast<const int32_t *>(rc) + 4;
        const float *tlc = rc + 4 + COCR_LM_KMAX;
        // next frame's record and the stay candidates' lp[last] travel while the extensions are scored
        float rnext = 0.f, lglast = 0.f;
        if (tid < COCR_LM_REC && t + 1 < len) rnext = rec[(size_t)(t + 1) * COCR_LM_REC + tid];
        if (tid >= STAY0 && tid - STAY0 < beam) { const int l = cur.last[tid - STAY0]; if (l > 0) lglast = lg[(size_t)t * C + l]; }
        if (tid < NB) {                                                        // slots no survivor writes are dead
            nxt.hash[tid] = 0ull; nxt.ctx[tid] = make_uint4(0u, 0u, 0u, 0u);
            nxt.pb[tid] = -INFINITY; nxt.pnb[tid] = -INFINITY; nxt.tot[tid] = -INFINITY; nxt.lmv[tid] = 0.f; nxt.last[tid] = 0;
        }
        // ---- extensions: prefix i by the class of rank r
        for (int j = tid; j < NE; j += 256) {
            const int i = j / K, r = j - i * K, c = tcc[r], li = cur.last[i];
            unsigned long long key = 0ull;
            const float e = c > 0 ? (c == li ? cur.pb[i] : cur.tot[i]) + tlc[r] : -INFINITY;
            if (e > -INFINITY) {
                const unsigned long long hc = cur.hash[i] * COCR_HASH_PRIME + (unsigned long long)(c + 1);
                bool folded = false;                                           // it equals live prefix q: it adds to q's stay candidate
                for (int q = 0; q < beam; ++q)
                    if (q != i && cur.hash[q] == hc && cur.tot[q] > -INFINITY) { mval[q] = e; mpos[q] = i * C + c; folded = true; break; }
                if (!folded) {
                    float term = beta;
                    if (alpha != 0.f) {
                        const uint4 cw = cur.ctx[i];
                        const unsigned short cx[8] = {(unsigned short)(cw.x & 0xffffu), (unsigned short)(cw.x >> 16), (unsigned short)(cw.y & 0xffffu),
                                                      (unsigned short)(cw.y >> 16),     (unsigned short)(cw.z & 0xffffu), (unsigned short)(cw.z >> 16),
                                                      (unsigned short)(cw.w & 0xffffu), (unsigned short)(cw.w >> 16)};
                        term = __fadd_rn(__fmul_rn(alpha, lm_lookup(L, cx, c)), beta);
                    }
                    const float lmv = __fadd_rn(cur.lmv[i], term);
                    clmv[j] = lmv;
                    key = beam_key(__fadd_rn(e, lmv), (unsigned)(i * C + c));
                }
            }
            ckey[j] = key;
        }
        __syncthreads();                                                       // (A) folds are in mval / mpos
        // ---- stay candidates, with a folded extension if there is one
        if (tid >= STAY0 && tid - STAY0 < beam) {
            const int i = tid - STAY0, li = cur.last[i];
            const float s_b = cur.tot[i] + rc[0];
            const float s_nb = lse2(li > 0 ? cur.pnb[i] + ((lglast - rc[2]) - (rc[1] - rc[2])) : -INFINITY, mval[i]);
            const float total = lse2(s_b, s_nb);
            const int mp = mpos[i];
            spb[i] = s_b; spnb[i] = s_nb;
            sbp[i] = beam_stay_bp(i, mp, C);
            ckey[NE + i] = beam_key(__fadd_rn(total, cur.lmv[i]), (unsigned)min(i * C, mp));
        }
        __syncthreads();                                                       // (B) all keys are in LDS
        if (tid < NB) { mval[tid] = -INFINITY; mpos[tid] = 0x7fffffff; }
        if (tid < COCR_LM_REC) recs[(t + 1) & 1][tid] = rnext;
        // ---- rank = the number of larger keys; the candidate of rank R < beam is next frame's prefix R
        auto settle = [&](int j) {
            const unsigned long long key = ckey[j];
            if (key == 0ull) return;
            int rank = 0;
            for (int q = 0; q < NCP; q += 2) {
                const ulonglong2 kk = *reinterpret_cast<const ulonglong2 *>(&ckey[q]);
                rank += (kk.x > key) + (kk.y > key);
            }
            if (rank >= beam) return;
            const int R = rank;
            int bpv;
            if (j >= NE) {
                const int i = j - NE;
                nxt.pb[R] = spb[i]; nxt.pnb[R] = spnb[i]; nxt.tot[R] = lse2(spb[i], spnb[i]); nxt.lmv[R] = cur.lmv[i];
                nxt.last[R] = cur.last[i]; nxt.hash[R] = cur.hash[i]; nxt.ctx[R] = cur.ctx[i];
                bpv = sbp[i];
            } else {
                const int i = j / K, r = j - i * K, c = tcc[r];
                const float e = (c == cur.last[i] ? cur.pb[i] : cur.tot[i]) + tlc[r];
                const uint4 cw = cur.ctx[i];
                nxt.pb[R] = -INFINITY; nxt.pnb[R] = e; nxt.tot[R] = e; nxt.lmv[R] = clmv[j];
                nxt.last[R] = c; nxt.hash[R] = cur.hash[i] * COCR_HASH_PRIME + (unsigned long long)(c + 1);
                nxt.ctx[R] = make_uint4((cw.x << 16) | (unsigned)c, (cw.y << 16) | (cw.x >> 16), (cw.z << 16) | (cw.y >> 16), (cw.w << 16) | (cw.z >> 16));
                bpv = (i << 16) | c;
            }
            if (bp_in_lds) bpl[t * beam + R] = bpv; else bpg[(size_t)t * NB + R] = bpv;
        };
        if (tid >= STAY0 && tid - STAY0 < beam) settle(NE + tid - STAY0);
        for (int j = tid; j < NE; j += 256) settle(j);
        __syncthreads();                                                       // (C) next frame's prefixes are in LDS
    }
    const lm_prefix_state &fin = st[len & 1];
    if (tid == 0 && score) { score[2 * n] = fin.tot[0]; score[2 * n + 1] = fin.lmv[0]; }
    // ---- best prefix: walk the back-pointers (one lane), then ends / confidences in parallel over the labels
    int32_t *olab = labels + (size_t)n * max_per_line, *ost = starts + (size_t)n * max_per_line;
    if (bp_in_lds) beam_walk_lds(bpl, beam, bpl + (size_t)T * beam, len, max_per_line, tid, olab, ost, s_cnt, s_next, counts[n]);
    else if (tid == 0) { const BeamWalk w = beam_walk_rows(bpg, len, max_per_line, olab, ost); s_cnt = w.cnt; s_next = w.next; counts[n] = w.cnt; }
    __threadfence_block();
    __syncthreads();
    beam_records<256>(lg, C, olab, ost, min(s_cnt, max_per_line), s_next, tid, ends, conf, (size_t)n * max_per_line,
                      [=](int t) { return rec[(size_t)t * COCR_LM_REC + 1]; });
}
