// What follows the forward behind the C ABI (units of the host layer: model.hip.h): the CTC decoders (greedy, beam, beam with an
// n-gram model, n-best output of both), the n-gram model itself, the CTC criterion, the distillation term, forced alignment, text-to-page alignment, keyword and pattern spotting and the search index's pack / unpack.
#include "model.hip.h"
#include "ctc.hip.h"
#include "ctc_lm.hip.h"
#include "ctc_nbest.hip.h"
#include "ctc_loss.hip.h"
#include "distill.hip.h"
#include "ctc_align.hip.h"
#include "ctc_align_page.hip.h"
#include "ctc_spot.hip.h"
#include "ctc_spot_graph.hip.h"
#include "ctc_index.hip.h"

// ------------------------------------------------------------------------------------ CTC
// The per-line lengths reach the decode kernels through a PINNED host ring: an async copy from pageable memory goes through the
// runtime's staging buffers, and a third such copy in flight (three batches on three streams, each copy queued behind its
// forward) blocked the host until the first forward had finished -- 5.5 ms per run start.  `d_lens`: the lengths on the device.
static int upload_lens(cocr_model *m, const int32_t *lens, int N, hipStream_t s, const int32_t *&d_lens) {
    int32_t *h, *d;
    HIP_TRY(m->dec.lens_ring.stage((size_t)N * 4, h, d));
    memcpy(h, lens, (size_t)N * 4);
    HIP_TRY(m->dec.lens_ring.commit((size_t)N * 4, s));
    d_lens = d;
    return COCR_OK;
}

// Host prologues of the calls that read their per-line lengths and labels before anything is launched.
static int check_out_lens(const int32_t *out_lens, int N, int T) {
    for (int n = 0; n < N; ++n)
        if (out_lens[n] < 0 || out_lens[n] > T) return fail(COCR_EINVAL, "input length %d outside [0, %d] (line %d)", out_lens[n], T, n);
    return COCR_OK;
}

// `noun`: what a label is called in the message ("target", "query label")
static int check_labels(const char *noun, const int32_t *labels, size_t total, int ncls) {
    for (size_t i = 0; i < total; ++i)
        if (labels[i] < 1 || labels[i] >= ncls) return fail(COCR_EINVAL, "%s %d outside [1, %d) (blank is 0)", noun, labels[i], ncls);
    return COCR_OK;
}

// The shape checks the entry points repeat: a batch of N lines of T frames and ncls >= min_cls classes (rows: max_per_line, where the
// call has one); frame_limit: the call's kernels hold a line's frames in LDS.
static int check_frames(int T) { return T > 8000 ? fail(COCR_EUNSUPPORTED, "more than 8000 frames per line") : COCR_OK; }
static int check_shape(int N, int T, int ncls, int min_cls, bool frame_limit, int rows = 1) {
    if (N < 1 || T < 1 || ncls < min_cls || rows < 1) return fail(COCR_EINVAL, "empty problem");
    return frame_limit ? check_frames(T) : COCR_OK;
}

// Behind a call's checks: its device, its stream, and the per-line lengths on their way to the device.
static int begin_call(cocr_model *m, const int32_t *lens, int N, void *stream, hipStream_t &s, const int32_t *&d_lens) {
    HIP_TRY(hipSetDevice(m->device));
    s = (hipStream_t)stream;
    return upload_lens(m, lens, N, s, d_lens);
}

// Where the per-line (per-pair) table of a lattice kernel lives: in dynamic LDS behind the frame statistics when all of it
// (`lds_all` bytes) fits -- the kernels have ~5 KB of static LDS of their own -- else in `ws`, grown to `ws_words`, the statistics
// (`lds_stats` bytes) alone in LDS.  `lds`: the dynamic LDS to launch with; `ws`: null for the LDS form.
struct LatticeTable { bool in_lds; size_t lds; unsigned *ws; };
static int place_lattice_table(size_t lds_stats, size_t lds_all, DevBuf<unsigned> &ws, size_t ws_words, LatticeTable &t) {
    t = {lds_all <= 144 * 1024, lds_all, nullptr};
    if (t.in_lds) return COCR_OK;
    HIP_TRY(ws.grow(ws_words));
    t.lds = lds_stats;
    t.ws = ws.p;
    return COCR_OK;
}

int ensure_ctc_scratch(cocr_model *m, size_t rows) {
    if (rows <= m->dec.ctc_lab.n && rows <= m->dec.ctc_val.n) return COCR_OK;
    HIP_TRY(hipDeviceSynchronize());                          // (captured launches that point at the old scratch are dropped with it)
    m->graphs.drop();
    m->dec.amax_logits = nullptr;
    HIP_TRY(m->dec.ctc_lab.grow(rows));
    HIP_TRY(m->dec.ctc_val.grow(rows));
    return COCR_OK;
}

extern "C" int cocr_ctc_greedy(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens, int32_t *labels,
                               int32_t *starts, int32_t *ends, float *conf, int32_t *counts, int max_per_line, void *stream) {
    if (!m || !logits || !out_lens || !labels || !starts || !ends || !conf || !counts) return fail(COCR_EINVAL, "null argument");
    int rc = check_shape(N, T, ncls, 1, true, max_per_line);
    if (rc) return rc;
    hipStream_t s;
    const int32_t *d_lens;
    if ((rc = begin_call(m, out_lens, N, stream, s, d_lens))) return rc;
    const bool have_argmax = logits == m->dec.amax_logits && N * T == m->dec.amax_rows && ncls == m->ncls;      // the decoder's epilogue computed it for these logits
    if (!have_argmax && (rc = ensure_ctc_scratch(m, (size_t)N * T))) return rc;
    ProfScope ps(m, s, FAM_GREEDY);
    if (!have_argmax) {
        m->dec.amax_logits = nullptr;                             // the scratch no longer belongs to the last forward's logits
        hipLaunchKernelGGL(ctc_argmax_kernel, dim3(ceil_div(N * T, 4)), dim3(256), 0, s, logits, T, ncls, N * T, d_lens, m->dec.ctc_lab.p, m->dec.ctc_val.p);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ctc_collapse_kernel, dim3(N), dim3(64), (size_t)T * 8, s, T, d_lens, m->dec.ctc_lab.p, m->dec.ctc_val.p, labels, starts, ends, conf, counts,
                       max_per_line);
    LAUNCH_CHECK();
    return COCR_OK;
}

// What a beam search leaves in its scratch for the n-best pass (ctc_nbest.hip.h): the back-pointers [N][T][COCR_BEAM_MAX], log Z of
// frame (n, t) at lz[(n T + t) lz_stride], and `extra` bytes of the caller's behind both (16-byte aligned).
struct BeamTrail { const int32_t *bp; const float *lz; int lz_stride; unsigned char *extra; };

// The outputs of a 1-best call.  The walk kernel's own of an n-best call, one record per line (max_per_line 1: it is asked for no more),
// sit at the head of `extra`.
struct BeamOut { int32_t *labels, *starts, *ends; float *conf; int32_t *counts; };
static size_t walk_out_bytes(int N) { return ((size_t)N * 5 * 4 + 15) / 16 * 16; }
static BeamOut walk_out_at(unsigned char *p, int N) {
    int32_t *q = reinterpret_cast<int32_t *>(p);
    return {q, q + N, q + 2 * N, reinterpret_cast<float *>(q + 3 * N), q + 4 * N};
}

// A beam search's scratch in `buf`: the back-pointers [N][T][COCR_BEAM_MAX] i32, then what the search keeps per frame (rec: so many bytes,
// log Z at byte lz_off of the first and every lz_stride floats).  `trail`: null for the 1-best call; else the back-pointers go to global
// memory over a region filled with 0xFF bytes (-1: the rank was not alive in that frame), `extra` >= walk_out_bytes(N) bytes are kept behind
// the scratch (16-byte aligned), and the kernel's 1-best outputs go to their head (the caller passes max_per_line 1 and no outputs).
// dyn: the walk kernels' dynamic LDS -- a line's back-pointers and the label stack of the final walk -- which they get when it fits.
struct BeamRec { size_t bytes, lz_off; int lz_stride; };
struct BeamScratch { int32_t *bp; unsigned char *rec; size_t dyn; int bp_in_lds; };
static int plan_beam_scratch(DevBuf<unsigned char> &buf, int N, int T, BeamRec r, int beam, hipStream_t s, size_t extra, BeamTrail *trail, BeamOut &out,
                             BeamScratch &b) {
    const size_t bp_bytes = (size_t)N * T * COCR_BEAM_MAX * 4, need = bp_bytes + (size_t)N * T * r.bytes, kept = (need + 15) / 16 * 16;
    HIP_TRY(buf.grow(trail ? kept + extra : need));
    b = {reinterpret_cast<int32_t *>(buf.p), buf.p + bp_bytes, (size_t)T * ((size_t)beam * 4 + 8), 0};
    b.bp_in_lds = !trail && b.dyn <= 96 * 1024;
    if (trail) {
        HIP_TRY(hipMemsetAsync(b.bp, 0xFF, bp_bytes, s));
        *trail = {b.bp, reinterpret_cast<const float *>(b.rec + r.lz_off), r.lz_stride, buf.p + kept};
        out = walk_out_at(trail->extra, N);
    }
    return COCR_OK;
}

// The launches of cocr_ctc_beam behind its checks; `extra` and `trail` as in plan_beam_scratch.
static int beam_launch(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *d_lens, BeamOut out, int max_per_line, int beam,
                       hipStream_t s, size_t extra, BeamTrail *trail) {
    const bool fast = ncls <= 256 && !m->sw.beam_ref;            // ctc_beam_rank_kernel + ctc_beam_walk_kernel: frames ranked in parallel, a static pruned candidate set per frame
    const int K = std::min(beam + 1, ncls - 1);
    BeamScratch b;                                               // behind the back-pointers: the frame records (fast) or log Z [N][T] (exhaustive kernel)
    const int rc = plan_beam_scratch(m->dec.beam_bp, N, T, fast ? BeamRec{COCR_BEAM_REC, COCR_BEAM_REC_LZ, COCR_BEAM_REC / 4} : BeamRec{4, 0, 1}, beam, s, extra,
                                     trail, out, b);
    if (rc) return rc;
    if (fast) {
        hipLaunchKernelGGL(ctc_beam_rank_kernel, dim3(N * T), dim3(256), 0, s, logits, T, ncls, d_lens, K, b.rec);
        auto walk = ctc_beam_walk_kernel<3>;                          // candidates per lane of a wave: <= 88 for beam <= 16, <= 184 for beam 32
        if (beam <= 16) walk = ctc_beam_walk_kernel<2>;
        // (the kernel also has ~12 KB of static LDS: the limit raised for the dynamic part stays below 160 KB - static)
        if (b.bp_in_lds) HIP_TRY(raise_lds_limit((const void *)walk, b.dyn, 48 * 1024, 96 * 1024));
        hipLaunchKernelGGL(walk, dim3(N), dim3(256), b.bp_in_lds ? b.dyn : 0, s, logits, T, ncls, d_lens, beam, K, out.labels, out.starts,
                           out.ends, out.conf, out.counts, max_per_line, b.rec, b.bp, b.bp_in_lds, m->stamps ? m->stamps + 240 : nullptr);
    } else {
        const size_t lds = ((size_t)ncls + (size_t)beam * ncls) * 4 + COCR_BEAM_MAX * (11 * 4 + 2 * 8) + 64;
        if (lds > 150 * 1024) return fail(COCR_EUNSUPPORTED, "beam x classes too large for the LDS candidate table");
        HIP_TRY(raise_lds_limit((const void *)ctc_beam_kernel, lds));
        hipLaunchKernelGGL(ctc_beam_kernel, dim3(N), dim3(64), lds, s, logits, T, ncls, d_lens, beam, out.labels, out.starts, out.ends, out.conf, out.counts,
                           max_per_line, b.bp, reinterpret_cast<float *>(b.rec));
    }
    LAUNCH_CHECK();
    return COCR_OK;
}

static int beam_check(int N, int T, int ncls, int max_per_line, int beam) {
    const int rc = check_shape(N, T, ncls, 2, false, max_per_line);
    if (rc) return rc;
    if (beam < 1 || beam > COCR_BEAM_MAX) return fail(COCR_EINVAL, "beam must be in 1..%d", COCR_BEAM_MAX);
    if (ncls > 65535) return fail(COCR_EUNSUPPORTED, "more than 65535 classes");
    return COCR_OK;
}

extern "C" int cocr_ctc_beam(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens, int32_t *labels,
                             int32_t *starts, int32_t *ends, float *conf, int32_t *counts, int max_per_line, int beam, void *stream) {
    if (!m || !logits || !out_lens || !labels || !starts || !ends || !conf || !counts) return fail(COCR_EINVAL, "null argument");
    int rc = beam_check(N, T, ncls, max_per_line, beam);
    if (rc) return rc;
    hipStream_t s;
    const int32_t *d_lens;
    if ((rc = begin_call(m, out_lens, N, stream, s, d_lens))) return rc;
    ProfScope ps(m, s, FAM_BEAM);
    return beam_launch(m, logits, N, T, ncls, d_lens, {labels, starts, ends, conf, counts}, max_per_line, beam, s, 0, nullptr);
}

// ------------------------------------------------------------------------------------ beam search with an n-gram model (ctc_lm.hip.h)
struct cocr_lm {
    int device = 0, order = 0, ncls = 0;
    int64_t nslots = 0, cslots = 0;
    DevBuf<float> unigram, nlogp, cbow;
    DevBuf<unsigned long long> nkeys, ckeys;
};

static int lm_check_table(const char *what, const int64_t *keys, const float *vals, int64_t slots) {
    if (slots < 2 || slots > (1ll << 30) || (slots & (slots - 1))) return fail(COCR_EINVAL, "%s: slot count %lld is not a power of two in 2..2^30", what, (long long)slots);
    if (!keys || !vals) return fail(COCR_EINVAL, "%s: null table", what);
    for (int64_t i = 0; i < slots; ++i)
        if (keys[i] == 0) return COCR_OK;
    return fail(COCR_EINVAL, "%s: no empty slot (a probe sequence would not end)", what);
}

extern "C" int cocr_lm_create(cocr_model *m, int order, int ncls, const float *unigram, const int64_t *ngram_keys, const float *ngram_logp,
                              int64_t ngram_slots, const int64_t *ctx_keys, const float *ctx_bow, int64_t ctx_slots, cocr_lm **out) {
    if (!m || !unigram || !out) return fail(COCR_EINVAL, "null argument");
    if (order < 1 || order > COCR_LM_CTX + 1) return fail(COCR_EINVAL, "order must be in 1..%d", COCR_LM_CTX + 1);
    if (ncls < 2 || ncls > 65535) return fail(COCR_EINVAL, "ncls must be in 2..65535");
    int rc = lm_check_table("ngram table", ngram_keys, ngram_logp, ngram_slots);
    if (rc) return rc;
    if ((rc = lm_check_table("context table", ctx_keys, ctx_bow, ctx_slots))) return rc;
    HIP_TRY(hipSetDevice(m->device));
    cocr_lm *lm = new cocr_lm();
    lm->device = m->device; lm->order = order; lm->ncls = ncls; lm->nslots = ngram_slots; lm->cslots = ctx_slots;
    hipError_t e = lm->unigram.grow((size_t)ncls);
    if (e == hipSuccess) e = lm->nkeys.grow((size_t)ngram_slots);
    if (e == hipSuccess) e = lm->nlogp.grow((size_t)ngram_slots);
    if (e == hipSuccess) e = lm->ckeys.grow((size_t)ctx_slots);
    if (e == hipSuccess) e = lm->cbow.grow((size_t)ctx_slots);
    if (e == hipSuccess) e = hipMemcpy(lm->unigram.p, unigram, (size_t)ncls * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(lm->nkeys.p, ngram_keys, (size_t)ngram_slots * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(lm->nlogp.p, ngram_logp, (size_t)ngram_slots * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(lm->ckeys.p, ctx_keys, (size_t)ctx_slots * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(lm->cbow.p, ctx_bow, (size_t)ctx_slots * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { delete lm; return fail(COCR_EHIP, "copying the language model to the device failed: %s", hipGetErrorString(e)); }
    *out = lm;
    return COCR_OK;
}

extern "C" void cocr_lm_destroy(cocr_lm *lm) {
    if (!lm) return;
    (void)hipSetDevice(lm->device);
    delete lm;
}

static int beam_lm_check(cocr_model *m, cocr_lm *lm, int N, int T, int ncls, int max_per_line, int beam, int classes, float alpha, float beta) {
    const int rc = check_shape(N, T, ncls, 2, true, max_per_line);
    if (rc) return rc;
    if (beam < 1 || beam > COCR_BEAM_MAX) return fail(COCR_EINVAL, "beam must be in 1..%d", COCR_BEAM_MAX);
    if (classes < 1 || classes > COCR_LM_KMAX) return fail(COCR_EINVAL, "classes must be in 1..%d", COCR_LM_KMAX);
    if (ncls != lm->ncls) return fail(COCR_EINVAL, "the logits have %d classes, the language model %d", ncls, lm->ncls);
    if (lm->device != m->device) return fail(COCR_EINVAL, "the language model lives on device %d, the model on %d", lm->device, m->device);
    if (!std::isfinite(alpha) || !std::isfinite(beta)) return fail(COCR_EINVAL, "alpha and beta must be finite");
    return COCR_OK;
}

static cocr_lm_tables lm_tables(const cocr_lm *lm) {
    cocr_lm_tables L;
    L.unigram = lm->unigram.p; L.nkeys = lm->nkeys.p; L.nlogp = lm->nlogp.p; L.ckeys = lm->ckeys.p; L.cbow = lm->cbow.p;
    L.nmask = (unsigned)(lm->nslots - 1); L.cmask = (unsigned)(lm->cslots - 1); L.order = lm->order;
    return L;
}

// The launches of cocr_ctc_beam_lm behind its checks; `extra` and `trail` as in beam_launch.
static int beam_lm_launch(cocr_model *m, cocr_lm *lm, const float *logits, int N, int T, int ncls, const int32_t *d_lens, BeamOut out, int max_per_line,
                          int beam, int classes, float alpha, float beta, float *score, hipStream_t s, size_t extra, BeamTrail *trail) {
    const int K = std::min(classes, ncls - 1);
    BeamScratch b;                                               // behind the back-pointers: the frame records [N][T][COCR_LM_REC] f32
    const int rc = plan_beam_scratch(m->dec.lm_scratch, N, T, BeamRec{COCR_LM_REC * 4, 4, COCR_LM_REC}, beam, s, extra, trail, out, b);
    if (rc) return rc;
    float *rec = reinterpret_cast<float *>(b.rec);
    if (b.bp_in_lds) HIP_TRY(raise_lds_limit((const void *)ctc_lm_walk_kernel, b.dyn, 16 * 1024, 96 * 1024));      // (the kernel has ~30 KB of static LDS)
    const cocr_lm_tables L = lm_tables(lm);
    hipLaunchKernelGGL(ctc_lm_topk_kernel, dim3(ceil_div(N * T, 4)), dim3(256), 0, s, logits, T, ncls, N * T, d_lens, K, rec);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(ctc_lm_walk_kernel, dim3(N), dim3(256), b.bp_in_lds ? b.dyn : 0, s, logits, T, ncls, d_lens, beam, K, L, alpha, beta, out.labels,
                       out.starts, out.ends, out.conf, out.counts, score, max_per_line, rec, b.bp, b.bp_in_lds);
    LAUNCH_CHECK();
    return COCR_OK;
}

extern "C" int cocr_ctc_beam_lm(cocr_model *m, cocr_lm *lm, const float *logits, int N, int T, int ncls, const int32_t *out_lens, int32_t *labels,
                                int32_t *starts, int32_t *ends, float *conf, int32_t *counts, int max_per_line, int beam, int classes, float alpha,
                                float beta, float *score, void *stream) {
    if (!m || !lm || !logits || !out_lens || !labels || !starts || !ends || !conf || !counts) return fail(COCR_EINVAL, "null argument");
    int rc = beam_lm_check(m, lm, N, T, ncls, max_per_line, beam, classes, alpha, beta);
    if (rc) return rc;
    hipStream_t s;
    const int32_t *d_lens;
    if ((rc = begin_call(m, out_lens, N, stream, s, d_lens))) return rc;
    ProfScope ps(m, s, FAM_BEAM);
    return beam_lm_launch(m, lm, logits, N, T, ncls, d_lens, {labels, starts, ends, conf, counts}, max_per_line, beam, classes, alpha, beta, score, s, 0, nullptr);
}

// ------------------------------------------------------------------------------------ n-best output (ctc_nbest.hip.h)
extern "C" int cocr_ctc_beam_nbest(cocr_model *m, cocr_lm *lm, const float *logits, int N, int T, int ncls, const int32_t *out_lens, int beam, int nbest,
                                   int classes, float alpha, float beta, int32_t *labels, int32_t *starts, int32_t *ends, float *conf, int32_t *counts,
                                   int32_t *nhyp, float *scores, int max_per_line, void *stream) {
    if (!m || !logits || !out_lens || !labels || !starts || !ends || !conf || !counts || !nhyp || !scores) return fail(COCR_EINVAL, "null argument");
    int rc = lm ? beam_lm_check(m, lm, N, T, ncls, max_per_line, beam, classes, alpha, beta) : beam_check(N, T, ncls, max_per_line, beam);
    if (rc) return rc;
    if (nbest < 1 || nbest > beam) return fail(COCR_EINVAL, "nbest must be in 1..beam (%d)", beam);
    if ((rc = check_frames(T))) return rc;
    if ((rc = check_out_lens(out_lens, N, T))) return rc;
    const int cap = std::max(1, (int)*std::max_element(out_lens, out_lens + N));        // frames of the longest line
    hipStream_t s;
    const int32_t *d_lens;
    if ((rc = begin_call(m, out_lens, N, stream, s, d_lens))) return rc;
    // behind the search's scratch: the walk kernel's own 1-best outputs, then the chains' label stacks [N][nbest][T] of a call whose
    // lines do not fit the LDS
    const bool in_lds = nbest_lds_bytes(cap, beam, nbest, true) <= 144 * 1024;
    const size_t walk_out = walk_out_bytes(N), extra = walk_out + (in_lds ? 0 : (size_t)N * nbest * T * 4);
    ProfScope ps(m, s, FAM_BEAM);
    BeamTrail tr;
    if (lm) rc = beam_lm_launch(m, lm, logits, N, T, ncls, d_lens, {}, 1, beam, classes, alpha, beta, nullptr, s, extra, &tr);
    else rc = beam_launch(m, logits, N, T, ncls, d_lens, {}, 1, beam, s, extra, &tr);
    if (rc) return rc;
    unsigned *stk_ws = in_lds ? nullptr : reinterpret_cast<unsigned *>(tr.extra + walk_out);
    const cocr_lm_tables L = lm ? lm_tables(lm) : cocr_lm_tables{};
    HIP_TRY(launch_ctc_nbest(s, sj_for_states(2 * std::min(cap, COCR_LATTICE_MAX_LABELS) + 1), in_lds, lm != nullptr, nbest_lds_bytes(cap, beam, nbest, in_lds), N, logits, T, ncls,
                             d_lens, beam, nbest, tr.bp, tr.lz, tr.lz_stride, L, labels, starts, ends, conf, counts, nhyp, scores, max_per_line,
                             stk_ws, cap));
    LAUNCH_CHECK();
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ CTC loss (ctc_loss.hip.h)
// The targets of a batch on the device, and the kernel form for its longest line: sj 64-state columns per lane.
struct CtcTargets { const int32_t *lens, *label_lens, *label_off, *labels; int sj; };

// Loss and forced alignment: checks the per-line lengths and the labels, then sends [lens | label lens | label offsets | labels]
// through the targets ring.  `outputs_ok`: the caller's per-label output pointers are set (asked for only where there are labels);
// `too_long`: the status for a line of more than COCR_LATTICE_MAX_LABELS labels.
static int upload_targets(cocr_model *m, int N, int T, int ncls, const int32_t *out_lens, const int32_t *targets, const int32_t *label_lens,
                          bool outputs_ok, int too_long, void *stream, CtcTargets &t) {
    size_t total = 0;
    int max_l = 0;
    int rc = check_out_lens(out_lens, N, T);
    if (rc) return rc;
    for (int n = 0; n < N; ++n) {
        if (label_lens[n] < 0) return fail(COCR_EINVAL, "negative target length (line %d)", n);
        if (label_lens[n] > COCR_LATTICE_MAX_LABELS)
            return fail(too_long, "line %d has %d labels; the kernel holds at most %d", n, label_lens[n], COCR_LATTICE_MAX_LABELS);
        max_l = std::max(max_l, (int)label_lens[n]);
        total += (size_t)label_lens[n];
    }
    if (total && (!targets || !outputs_ok)) return fail(COCR_EINVAL, "null argument");
    if ((rc = check_labels("target", targets, total, ncls))) return rc;
    HIP_TRY(hipSetDevice(m->device));
    const size_t ints = (size_t)3 * N + total;
    int32_t *h, *d;
    HIP_TRY(m->dec.target_ring.stage(ints * 4, h, d));
    int32_t off = 0;
    for (int n = 0; n < N; ++n) { h[n] = out_lens[n]; h[N + n] = label_lens[n]; h[2 * N + n] = off; off += label_lens[n]; }
    if (total) memcpy(h + 3 * N, targets, total * 4);
    HIP_TRY(m->dec.target_ring.commit(ints * 4, (hipStream_t)stream));
    t = {d, d + N, d + 2 * N, d + 3 * N, sj_for_states(2 * max_l + 1)};
    return COCR_OK;
}

extern "C" int cocr_ctc_loss(cocr_model *m, const float *probits, int N, int T, int ncls, const int32_t *out_lens, const int32_t *targets,
                             const int32_t *label_lens, float *nll, float *grad, void *stream) {
    if (!m || !probits || !out_lens || !label_lens || !nll) return fail(COCR_EINVAL, "null argument");
    int rc = check_shape(N, T, ncls, 2, false);
    if (rc) return rc;
    if (ncls > 16384) return fail(COCR_EUNSUPPORTED, "more than 16384 classes");
    CtcTargets t;
    rc = upload_targets(m, N, T, ncls, out_lens, targets, label_lens, true, COCR_EUNSUPPORTED, stream, t);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int sj = t.sj;
    const size_t need = (size_t)N * T * ((size_t)ncls + 2 * 64 * sj);
    HIP_TRY(m->dec.loss_ws.grow(need));
    ProfScope ps(m, s, FAM_LOSS);
    launch_ctc_loss(s, sj, (size_t)ncls * 4, probits, N, T, ncls, t.lens, t.label_lens, t.label_off, t.labels, nll, grad, m->dec.loss_ws.p, m->dec.loss_ws.p + (size_t)N * T * ncls);
    LAUNCH_CHECK();
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ distillation term (distill.hip.h)
// frame_ws: N T floats of the caller's for the per-frame values (the training step's planned workspace), or null: the model's own scratch
int distill_loss_on(cocr_model *m, const float *student, const float *teacher, int N, int T, int ncls, const int32_t *out_lens, float tau, float *kd, float *grad,
                    float ctc_weight, float kd_weight, int accumulate, float *frame_ws, hipStream_t s) {
    if (!m || !student || !teacher || !out_lens || !kd) return fail(COCR_EINVAL, "null argument");
    int rc = check_shape(N, T, ncls, 2, false);
    if (rc) return rc;
    if ((size_t)N * T > (size_t)1 << 30) return fail(COCR_EUNSUPPORTED, "more than 2^30 frames in one call");
    if (!std::isfinite(tau) || !(tau > 0.f)) return fail(COCR_EINVAL, "the temperature must be finite and positive, not %g", (double)tau);
    if (!std::isfinite(ctc_weight) || ctc_weight < 0.f || !std::isfinite(kd_weight) || kd_weight < 0.f)
        return fail(COCR_EINVAL, "the weights must be finite and not negative (%g, %g)", (double)ctc_weight, (double)kd_weight);
    if (accumulate != 0 && accumulate != 1) return fail(COCR_EINVAL, "accumulate must be 0 or 1");
    if ((rc = check_out_lens(out_lens, N, T))) return rc;
    if (ncls > 16384) return fail(COCR_EUNSUPPORTED, "more than 16384 classes");
    HIP_TRY(hipSetDevice(m->device));
    if (!frame_ws) {
        if ((size_t)N * T > m->dec.distill_ws.n) HIP_TRY(hipDeviceSynchronize());      // (launches in flight may still write the old scratch)
        HIP_TRY(m->dec.distill_ws.grow((size_t)N * T));
        frame_ws = m->dec.distill_ws.p;
    }
    const int32_t *d_lens;
    if ((rc = upload_lens(m, out_lens, N, s, d_lens))) return rc;
    launch_distill(s, student, teacher, N, T, ncls, d_lens, tau, frame_ws, kd, grad, ctc_weight, kd_weight, accumulate);
    LAUNCH_CHECK();
    return COCR_OK;
}

extern "C" int cocr_distill_loss(cocr_model *m, const float *student, const float *teacher, int N, int T, int ncls, const int32_t *out_lens, float tau, float *kd,
                                 float *grad, float ctc_weight, float kd_weight, int accumulate, void *stream) {
    return distill_loss_on(m, student, teacher, N, T, ncls, out_lens, tau, kd, grad, ctc_weight, kd_weight, accumulate, nullptr, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------ forced alignment (ctc_align.hip.h)
extern "C" int cocr_ctc_align(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens, const int32_t *targets,
                              const int32_t *label_lens, int32_t *starts, int32_t *ends, float *conf, float *score, int32_t *counts, void *stream) {
    if (!m || !logits || !out_lens || !label_lens || !score || !counts) return fail(COCR_EINVAL, "null argument");
    int rc = check_shape(N, T, ncls, 2, true);
    if (rc) return rc;
    CtcTargets t;
    rc = upload_targets(m, N, T, ncls, out_lens, targets, label_lens, starts && ends && conf, COCR_EINVAL, stream, t);
    if (rc) return rc;
    // the back-pointer table: beside lz, or one region per line of the workspace
    const size_t words = ctca_bp_words(T, t.sj), row = lattice_row_bytes(T);
    LatticeTable tab;
    if ((rc = place_lattice_table(row, row + words * 4, m->dec.align_ws, (size_t)N * words, tab))) return rc;
    HIP_TRY(launch_ctc_align((hipStream_t)stream, t.sj, tab.in_lds, tab.lds, logits, N, T, ncls, t.lens, t.label_lens, t.label_off, t.labels, starts, ends, conf, score,
                             counts, tab.ws, tab.in_lds ? 0 : words));
    LAUNCH_CHECK();
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ text-to-page alignment (ctc_align_page.hip.h)
extern "C" int cocr_ctc_align_page(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens, int P, const int32_t *page_line_off,
                                   const int32_t *page_lines, const int32_t *targets, const int32_t *label_lens, const uint8_t *optional, int32_t *line,
                                   int32_t *starts, int32_t *ends, float *conf, float *score, int32_t *counts, float *line_score, void *stream) {
    if (!m || !logits || !out_lens || !page_line_off || !label_lens || !score || !counts) return fail(COCR_EINVAL, "null argument");
    int rc = check_shape(N, T, ncls, 2, false);
    if (rc) return rc;
    if (P < 1) return fail(COCR_EINVAL, "no page");
    if (ncls > COCR_PAGE_MAX_CLASSES) return fail(COCR_EUNSUPPORTED, "more than %d classes", COCR_PAGE_MAX_CLASSES);
    if ((rc = check_out_lens(out_lens, N, T))) return rc;
    if (page_line_off[0] != 0) return fail(COCR_EINVAL, "the page line offsets do not begin at 0");
    for (int p = 0; p < P; ++p)
        if (page_line_off[p + 1] < page_line_off[p]) return fail(COCR_EINVAL, "page line offsets descend at page %d", p);
    const size_t lines = (size_t)page_line_off[P];
    if (lines && (!page_lines || !line_score)) return fail(COCR_EINVAL, "null argument");
    std::vector<bool> used((size_t)N, false);
    for (size_t i = 0; i < lines; ++i) {
        const int32_t r = page_lines[i];
        if (r < 0 || r >= N) return fail(COCR_EINVAL, "page line %zu names row %d outside [0, %d)", i, r, N);
        if (used[(size_t)r]) return fail(COCR_EINVAL, "row %d is named by two page lines", r);
        used[(size_t)r] = true;
    }
    size_t total = 0;
    int max_l = 0;
    for (int p = 0; p < P; ++p) {
        if (label_lens[p] < 0) return fail(COCR_EINVAL, "negative label length (page %d)", p);
        max_l = std::max(max_l, (int)label_lens[p]);
        total += (size_t)label_lens[p];
    }
    if (total && (!targets || !optional || !line || !starts || !ends || !conf)) return fail(COCR_EINVAL, "null argument");
    if ((rc = check_labels("target", targets, total, ncls))) return rc;
    for (size_t at = 0, p = 0; p < (size_t)P; at += (size_t)label_lens[p], ++p) {
        const int L = label_lens[p];
        const uint8_t *o = optional + at;
        if (L && (o[0] || o[L - 1])) return fail(COCR_EINVAL, "page %zu: the first and the last label cannot be optional", p);
        for (int k = 1; k < L; ++k)
            if (o[k] && o[k - 1]) return fail(COCR_EINVAL, "page %zu: labels %d and %d are both optional", p, k - 1, k);
    }
    if (max_l > COCR_PAGE_MAX_LABELS) return fail(COCR_EUNSUPPORTED, "a page of %d labels; the kernel holds %d", max_l, COCR_PAGE_MAX_LABELS);
    int max_frames = 0;
    std::vector<int> page_frames((size_t)P);
    for (int p = 0; p < P; ++p) {
        const int K = page_line_off[p + 1] - page_line_off[p];
        if (K > COCR_PAGE_MAX_LINES) return fail(COCR_EUNSUPPORTED, "page %d has %d lines; the kernel holds %d", p, K, COCR_PAGE_MAX_LINES);
        size_t frames = 0;
        for (int k = 0; k < K; ++k) frames += (size_t)out_lens[page_lines[page_line_off[p] + k]];
        if (frames > COCR_PAGE_MAX_FRAMES) return fail(COCR_EUNSUPPORTED, "page %d has %zu frames; the kernel holds %d", p, frames, COCR_PAGE_MAX_FRAMES);
        max_frames = std::max(max_frames, page_frames[(size_t)p] = (int)frames);
    }
    // the kernel form by the call's largest S; one workspace region per page: back-pointers, lz, the path's states, the labels' runs
    const int sj = page_sj_for_states(2 * max_l + 1), waves = page_waves_for_states(2 * max_l + 1, sj);
    size_t words = 0;
    std::vector<uint32_t> region((size_t)P);
    for (int p = 0; p < P; ++p) {
        if (words * 4 > ((size_t)1 << 31)) break;
        region[(size_t)p] = (uint32_t)words;
        words += (page_region_words(page_frames[(size_t)p], label_lens[p], 64 * sj * waves) + 3) / 4 * 4;
    }
    if (words * 4 > ((size_t)1 << 31)) return fail(COCR_EUNSUPPORTED, "the call's tables exceed 2 GiB; align fewer pages per call");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    // [page line offsets P + 1 | rows | first frames (K + 1 per page) | label offsets P + 1 | labels (+ optional bit) | region offsets P]
    const size_t ints = 3 * (size_t)P + 2 + 2 * lines + (size_t)P + total;
    int32_t *h, *d;
    HIP_TRY(m->dec.page_ring.stage(ints * 4, h, d));
    int32_t *h_off = h, *h_rows = h + P + 1, *h_first = h_rows + lines, *h_loff = h_first + lines + P, *h_lab = h_loff + P + 1, *h_reg = h_lab + total;
    memcpy(h_off, page_line_off, (size_t)(P + 1) * 4);
    if (lines) memcpy(h_rows, page_lines, lines * 4);
    int32_t lo = 0;
    for (int p = 0; p < P; ++p) {
        int32_t *f = h_first + page_line_off[p] + p;
        int32_t g = 0;
        for (int k = page_line_off[p]; k < page_line_off[p + 1]; ++k) { *f++ = g; g += out_lens[page_lines[k]]; }
        *f = g;
        h_loff[p] = lo;
        for (int k = 0; k < label_lens[p]; ++k) h_lab[lo + k] = targets[lo + k] | (optional[lo + k] ? COCR_PAGE_OPTIONAL : 0);
        lo += label_lens[p];
        h_reg[p] = (int32_t)region[(size_t)p];
    }
    h_loff[P] = lo;
    HIP_TRY(m->dec.page_ring.commit(ints * 4, s));
    HIP_TRY(m->dec.page_ws.grow(std::max(words, (size_t)4)));
    const size_t lds = max_frames <= COCR_PAGE_LZ_LDS_FRAMES ? lattice_row_bytes(max_frames) : 0;
    HIP_TRY(launch_ctc_align_page(s, sj, waves, lds, logits, P, T, ncls, d, d + (h_rows - h), d + (h_first - h), d + (h_loff - h), d + (h_lab - h),
                                  reinterpret_cast<const uint32_t *>(d + (h_reg - h)), m->dec.page_ws.p, line, starts, ends, conf, score, counts, line_score));
    LAUNCH_CHECK();
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ keyword spotting (ctc_spot.hip.h)
extern "C" int cocr_ctc_spot(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens, const int32_t *queries,
                             const int32_t *query_lens, int Q, int hits, float min_score, int32_t *starts, int32_t *ends, float *score,
                             int32_t *counts, void *stream) {
    if (!m || !logits || !out_lens || !queries || !query_lens || !starts || !ends || !score || !counts) return fail(COCR_EINVAL, "null argument");
    int rc = check_shape(N, T, ncls, 2, false);
    if (rc) return rc;
    if (Q < 1) return fail(COCR_EINVAL, "no query");
    if (hits < 1 || hits > COCR_SPOT_MAX_HITS) return fail(COCR_EINVAL, "hits must be in 1..%d", COCR_SPOT_MAX_HITS);
    if (std::isnan(min_score)) return fail(COCR_EINVAL, "min_score is NaN");
    if ((rc = check_frames(T))) return rc;
    if (N > 65535) return fail(COCR_EUNSUPPORTED, "more than 65535 lines in one call");
    if ((rc = check_out_lens(out_lens, N, T))) return rc;
    size_t total = 0;
    int max_l = 0;
    for (int q = 0; q < Q; ++q) {
        if (query_lens[q] < 1 || query_lens[q] > COCR_LATTICE_MAX_LABELS)
            return fail(COCR_EINVAL, "query %d has %d labels; a query holds 1..%d", q, query_lens[q], COCR_LATTICE_MAX_LABELS);
        max_l = std::max(max_l, (int)query_lens[q]);
        total += (size_t)query_lens[q];
    }
    if ((rc = check_labels("query label", queries, total, ncls))) return rc;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t ints = (size_t)N + 2 * (size_t)Q + total;
    int32_t *h, *d;
    HIP_TRY(m->dec.spot_ring.stage(ints * 4, h, d));
    memcpy(h, out_lens, (size_t)N * 4);
    int32_t off = 0;
    for (int q = 0; q < Q; ++q) { h[N + q] = query_lens[q]; h[N + Q + q] = off; off += query_lens[q]; }
    memcpy(h + N + 2 * Q, queries, total * 4);
    HIP_TRY(m->dec.spot_ring.commit(ints * 4, s));
    // the candidate tables (e_t, sigma_t) of the workgroup's four pairs: beside mx, or one region per pair of the workspace
    const size_t row = lattice_row_bytes(T);
    LatticeTable tab;
    if ((rc = place_lattice_table(row, 9 * row, m->dec.spot_ws, (size_t)N * Q * ctcs_pair_words(T), tab))) return rc;
    HIP_TRY(launch_ctc_spot(s, sj_for_states(2 * max_l - 1), tab.in_lds, tab.lds, logits, N, T, ncls, d, d + N, d + N + Q, d + N + 2 * Q, Q, hits, min_score, starts, ends,
                            score, counts, tab.ws));
    LAUNCH_CHECK();
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ pattern spotting (ctc_spot_graph.hip.h)
extern "C" int cocr_ctc_spot_pattern(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens, const int32_t *state_counts,
                                     const int32_t *classes, const int32_t *flags, const int32_t *pred_off, const int32_t *preds, int Q, int hits,
                                     float min_score, int32_t *starts, int32_t *ends, float *score, int32_t *finals, int32_t *counts, void *stream) {
    if (!m || !logits || !out_lens || !state_counts || !classes || !flags || !pred_off || !starts || !ends || !score || !finals || !counts)
        return fail(COCR_EINVAL, "null argument");
    int rc = check_shape(N, T, ncls, 2, false);
    if (rc) return rc;
    if (Q < 1) return fail(COCR_EINVAL, "no pattern");
    if (hits < 1 || hits > COCR_GRAPH_MAX_HITS) return fail(COCR_EINVAL, "hits must be in 1..%d", COCR_GRAPH_MAX_HITS);
    if (std::isnan(min_score)) return fail(COCR_EINVAL, "min_score is NaN");
    if ((rc = check_frames(T))) return rc;
    if (N > 65535) return fail(COCR_EUNSUPPORTED, "more than 65535 lines in one call");
    if ((rc = check_out_lens(out_lens, N, T))) return rc;
    size_t states = 0, edges = 0;
    int max_p = 0;
    for (int q = 0; q < Q; ++q) {
        const int P = state_counts[q];
        if (P < 1 || P > COCR_GRAPH_MAX_STATES) return fail(COCR_EINVAL, "pattern %d has %d label states; a pattern holds 1..%d", q, P, COCR_GRAPH_MAX_STATES);
        const int32_t *off = pred_off + states + q, *fl = flags + states;
        if (off[0] != 0) return fail(COCR_EINVAL, "pattern %d: its predecessor offsets do not begin at 0", q);
        for (int p = 0; p < P; ++p)
            if (off[p + 1] < off[p]) return fail(COCR_EINVAL, "pattern %d: predecessor offsets descend at state %d", q, p);
        const int E = off[P];
        if (E > COCR_GRAPH_MAX_EDGES) return fail(COCR_EINVAL, "pattern %d has %d edges; a pattern holds at most %d", q, E, COCR_GRAPH_MAX_EDGES);
        if (E && !preds) return fail(COCR_EINVAL, "null argument");
        bool any_first = false, any_last = false;
        for (int p = 0; p < P; ++p) {
            if (fl[p] & ~3) return fail(COCR_EINVAL, "pattern %d: flags %d of state %d (1 = first, 2 = last)", q, fl[p], p);
            any_first |= (fl[p] & 1) != 0; any_last |= (fl[p] & 2) != 0;
            for (int e = off[p]; e < off[p + 1]; ++e) {
                const int32_t pr = preds[edges + e];
                if (pr < 0 || pr >= P) return fail(COCR_EINVAL, "pattern %d: predecessor %d of state %d outside [0, %d)", q, pr, p, P);
                if (e > off[p] && pr <= preds[edges + e - 1]) return fail(COCR_EINVAL, "pattern %d: the predecessors of state %d do not ascend strictly", q, p);
            }
        }
        if (!any_first || !any_last) return fail(COCR_EINVAL, "pattern %d has no %s state", q, any_first ? "last" : "first");
        max_p = std::max(max_p, P);
        states += (size_t)P;
        edges += (size_t)E;
    }
    if ((rc = check_labels("pattern class", classes, states, ncls))) return rc;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t ints = (size_t)N + 3 * (size_t)Q + 2 * states + (states + Q) + edges;
    int32_t *h, *d;
    HIP_TRY(m->dec.pattern_ring.stage(ints * 4, h, d));
    memcpy(h, out_lens, (size_t)N * 4);
    int32_t so = 0, eo = 0;
    for (int q = 0; q < Q; ++q) {
        h[N + q] = state_counts[q]; h[N + Q + q] = so; h[N + 2 * Q + q] = eo;
        eo += pred_off[so + q + state_counts[q]];
        so += state_counts[q];
    }
    int32_t *hc = h + N + 3 * Q;
    memcpy(hc, classes, states * 4);
    memcpy(hc + states, flags, states * 4);
    memcpy(hc + 2 * states, pred_off, (states + Q) * 4);
    if (edges) memcpy(hc + 3 * states + Q, preds, edges * 4);
    HIP_TRY(m->dec.pattern_ring.commit(ints * 4, s));
    // the candidate tables (e_t, sigma_t, final_t) of the workgroup's four pairs: beside mx and the blank's row, or one region per pair of
    // the workspace.  The kernel's static graph and exchange arrays count towards what fits.
    const size_t row = lattice_row_bytes(T);
    LatticeTable tab;
    if ((rc = place_lattice_table(2 * row, COCR_GRAPH_STATIC_LDS + 14 * row, m->dec.pattern_ws, (size_t)N * Q * ctcg_pair_words(T), tab))) return rc;
    const int32_t *dc = d + N + 3 * Q;
    HIP_TRY(launch_ctc_spot_graph(s, sj_for_states(max_p), tab.in_lds, tab.in_lds ? 14 * row : 2 * row, logits, N, T, ncls, d, d + N, d + N + Q, d + N + 2 * Q, dc, dc + states,
                                  dc + 2 * states, dc + 3 * states + Q, Q, hits, min_score, starts, ends, score, finals, counts, tab.ws));
    LAUNCH_CHECK();
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ search index (ctc_index.hip.h)
extern "C" int cocr_posterior_pack(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens, int keep, float inv_step,
                                   uint16_t *classes, uint8_t *codes, void *stream) {
    if (!m || !logits || !out_lens || !classes || !codes) return fail(COCR_EINVAL, "null argument");
    int rc = check_shape(N, T, ncls, 1, false);
    if (rc) return rc;
    if (ncls > 65535) return fail(COCR_EUNSUPPORTED, "more than 65535 classes");
    if (N > 65535) return fail(COCR_EUNSUPPORTED, "more than 65535 lines in one call");
    if ((size_t)N * T > (size_t)INT_MAX) return fail(COCR_EUNSUPPORTED, "more than 2^31 - 1 frames in one call");
    if (keep < 1 || keep > std::min(ncls, COCR_INDEX_MAX_KEEP)) return fail(COCR_EINVAL, "keep must be in 1..%d", std::min(ncls, COCR_INDEX_MAX_KEEP));
    if (!std::isfinite(inv_step) || !(inv_step > 0.f)) return fail(COCR_EINVAL, "inv_step must be finite and positive, not %g", (double)inv_step);
    if ((rc = check_out_lens(out_lens, N, T))) return rc;
    hipStream_t s;
    const int32_t *d_lens;
    if ((rc = begin_call(m, out_lens, N, stream, s, d_lens))) return rc;
    HIP_TRY(launch_posterior_pack(s, logits, N, T, ncls, d_lens, keep, inv_step, classes, codes));
    return COCR_OK;
}

extern "C" int cocr_posterior_unpack(cocr_model *m, const uint16_t *classes, const uint8_t *codes, int N, int T, int keep, int ncls, float step,
                                     float *logits_out, void *stream) {
    if (!m || !classes || !codes || !logits_out) return fail(COCR_EINVAL, "null argument");
    const int rc = check_shape(N, T, ncls, 1, false);
    if (rc) return rc;
    if (ncls > 65535) return fail(COCR_EUNSUPPORTED, "more than 65535 classes");
    if ((size_t)N * T > (size_t)INT_MAX) return fail(COCR_EUNSUPPORTED, "more than 2^31 - 1 frames in one call");
    if (keep < 1 || keep > std::min(ncls, COCR_INDEX_MAX_KEEP)) return fail(COCR_EINVAL, "keep must be in 1..%d", std::min(ncls, COCR_INDEX_MAX_KEEP));
    if (!std::isfinite(step) || !(step > 0.f)) return fail(COCR_EINVAL, "step must be finite and positive, not %g", (double)step);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(launch_posterior_unpack((hipStream_t)stream, classes, codes, N, T, keep, ncls, step, logits_out));
    return COCR_OK;
}
