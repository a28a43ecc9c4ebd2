/*
 * cocr.h -- C ABI of libcocr_hip.so: the MI355X (gfx950) implementation of the
 * recognition hot path of mittagessen/conformer_ocr:
 *
 *     line batch (N,1,H,W) -> conformer encoder -> linear decoder -> CTC decode
 *
 * The reference has no FFI for this path: it is the Python class
 * `PytorchRecognitionModel` (reference conformer_ocr/pred.py:50-210).  The host
 * class `conformer_ocr_amd.pred.PytorchRecognitionModel` keeps that class's
 * surface and binds these entry points through ctypes; each entry point cites
 * the reference lines whose work it takes over.
 *
 * Conventions: plain pointers and sizes only (no torch types); every function
 * returns 0 on success or a negative COCR_E* code, with a thread-local message
 * behind cocr_last_error(); the caller owns every buffer it passes in; the
 * library owns weights and workspace; a cocr_model is bound to one device and
 * must not be used from two host threads at once.  `stream` is a hipStream_t
 * (NULL = the default stream); all device work of a call is enqueued on it and
 * the call returns without synchronising unless stated.
 */
#ifndef COCR_H
#define COCR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cocr_model cocr_model;

/* element types of buffers crossing the boundary */
enum { COCR_F32 = 0, COCR_BF16 = 1, COCR_U8 = 2, COCR_I64 = 3 };

enum {
    COCR_OK = 0,
    COCR_EINVAL = -1,      /* bad argument / shape / name   -> ValueError   */
    COCR_ESTATE = -2,      /* call out of order             -> RuntimeError */
    COCR_EHIP = -3,        /* HIP runtime error             -> RuntimeError */
    COCR_EUNSUPPORTED = -4 /* hyper-parameters outside what the kernels cover */
};

/* The shape-determining constructor arguments of PytorchRecognitionModel
 * (pred.py:51-66); dropout probabilities are inference no-ops and not passed. */
typedef struct {
    int32_t num_classes;
    int32_t height;
    int32_t encoder_dim;
    int32_t num_encoder_layers;
    int32_t num_attention_heads;
    int32_t feed_forward_expansion_factor;
    int32_t conv_expansion_factor;
    int32_t conv_kernel_size;
    int32_t half_step_residual;
    int32_t subsampling_conv_channels;
    int32_t subsampling_factor;
} cocr_hparams;

const char *cocr_last_error(void);
const char *cocr_version(void);

/* Replaces the module construction of pred.py:70-91 (ConformerEncoder + nn.Linear decoder).
 * Validates like the reference constructors do (attention.py:53, convolution.py:132-133,177-178). */
int cocr_create(const cocr_hparams *hp, int device, cocr_model **out);
void cocr_destroy(cocr_model *m);

/* Replaces nn.Module.load_state_dict (pred.py:194,209): hands one state-dict entry to the model.
 * `name` is the reference key below `nn.` ("encoder.layers.0...", "decoder.weight"); `host` is
 * read during the call (copied).  dtype COCR_F32, or COCR_I64 for num_batches_tracked (ignored). */
int cocr_set_tensor(cocr_model *m, const char *name, const void *host, int dtype, int ndim, const int64_t *shape);

/* Names of tensors still missing, '\n'-separated, into buf (for strict loading); returns the count. */
int cocr_missing_tensors(cocr_model *m, char *buf, size_t buflen);

/* Packs the weights for the kernels and uploads them: BatchNorm folded into the depthwise taps
 * (convolution.py:140-141, eval mode), positional projection P = PE Wpos^T precomputed for the full
 * 9999-row table (embedding.py:35-66, attention.py:62,85,146), GLU / flatten permutations.
 * compute_dtype: COCR_BF16 (bf16 operands, fp32 accumulate, fp32 residual stream) or COCR_F32.
 * Synchronises the device. */
int cocr_finalize(cocr_model *m, int compute_dtype);

/* Multi-GPU start-up: a rank that receives its weights by broadcast allocates the packed blob
 * without filling it, hands (ptr, bytes) to its collective library (RCCL broadcast from the rank
 * that ran cocr_finalize), and is then ready.  The blob layout depends only on (hparams, dtype). */
int cocr_finalize_empty(cocr_model *m, int compute_dtype);
/* Kernel-specific re-layouts of some matrices (MFMA-fragment order) are DERIVED from the blob on the first forward after
 * cocr_finalize, cocr_blob_import or a call of cocr_weight_blob: a caller that writes through the pointer later must call
 * cocr_weight_blob again (or use cocr_blob_import) before the next forward, or those copies stay stale. */
int cocr_weight_blob(cocr_model *m, void **device_ptr, size_t *bytes);
/* The same through a caller-owned device buffer of exactly `bytes` = blob size (stream-ordered device-to-device copies):
 * export on the root, broadcast the caller's buffer, import on the other ranks. */
int cocr_blob_export(cocr_model *m, void *dst_device, size_t bytes, void *stream);
int cocr_blob_import(cocr_model *m, const void *src_device, size_t bytes, void *stream);

/* calc_length (convolution.py:240-247) with k=3, s=2, p=1 repeated log2(subsampling_factor) times. */
int32_t cocr_out_len(int32_t in_len, int32_t subsampling_factor);

/* Several packed copies of ONE model (one per stream of a caller that keeps several batches in flight) need one set of weights: after
 * this call `m` -- same hyper-parameters, same device -- reads `owner`'s packed weights, fragment-major copies and positional tables
 * and keeps only a workspace and captured launch sequences of its own.  (Four private copies of the cfg2 model are 4 x ~100 MB, more than
 * the 256 MB Infinity Cache: every forward then streamed its weights from HBM, cycling four copies on one stream ran 30 % slower than one.)
 * `owner` must outlive `m` and must not itself share; weights are changed through the owner (set_tensor + finalize, blob import, the
 * training entry points), `m` sees them at its next forward; finalizing `m` gives it weights of its own again.  Every entry point of
 * a sharing model reads the owner's current weights, not only its next forward; one that outlives its owner is not finalized. */
int cocr_share_weights(cocr_model *m, cocr_model *owner);

/* Host-side collation of a line batch: what kraken's `collate_sequences` does for the reference's loaders (cli/test.py:186-189, the
 * `DataLoader(..., collate_fn=collate_sequences)`): N lines of H rows each, line i `widths[i]` elements wide and C-contiguous, are
 * copied left-aligned into the (N,H,W) batch `dst` and the rest of every row is zeroed.  Plain host memory on both sides (dst is
 * typically a pinned staging buffer the caller uploads with one copy); elem_size 1 (uint8 lines) or 4 (float32); the rows are split
 * over `threads` host threads (<= 1: the calling thread alone).  No GPU call is made. */
int cocr_collate_lines(const void *const *lines, const int32_t *widths, int N, int H, int elem_size, void *dst, int W, int threads);

/* Pre-allocates workspace for batches up to N lines of width W (otherwise cocr_forward grows it on
 * demand, which synchronises and must not happen inside a stream capture). */
int cocr_reserve(cocr_model *m, int N, int W);

/* PytorchRecognitionModel.forward (pred.py:101-122): lines (N,H,W) [the (N,1,H,W) batch with the
 * singleton channel dropped; W fastest], DEVICE memory of type line_dtype (COCR_F32 in [0,1] or
 * COCR_U8, read as u8/255).  in_lens (N) HOST int32 pixel widths.  logits: DEVICE float32
 * (N,T,num_classes) with T = cocr_out_len(W).  out_lens: HOST int32 (N), written before return.
 * The padded region is processed like the reference does: no masking. */
int cocr_forward(cocr_model *m, const void *lines, int line_dtype, int N, int H, int W,
                 const int32_t *in_lens, float *logits, int32_t *out_lens, void *stream);

/* Replaces the per-line host loop `self.ctc_decoder(seq[:, :seq_len])` with
 * kraken.lib.ctc_decoder.greedy_decoder (pred.py:138-145,158-164,173-178; model.py:163-168):
 * per line argmax over classes (first index on ties), merge runs, drop blank (0).
 * logits DEVICE float32 (N,T,ncls); out_lens HOST int32 (N).  Outputs DEVICE, caller-owned:
 * labels/starts/ends int32 (N,max_per_line), conf float32 (N,max_per_line) = max over the run of the
 * label's logit, counts int32 (N).  A line emits at most ceil(len/1) runs; max_per_line >= T is safe;
 * excess runs are counted but not stored.
 * When `logits` is the buffer the model's LAST cocr_forward wrote (same pointer, same N*T; models of up to 128
 * classes), the per-frame argmax was already taken in the decoder product's epilogue and only the run merge is
 * launched.  A caller that edits those logits in place before decoding calls cocr_forget_argmax first. */
int cocr_ctc_greedy(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens,
                    int32_t *labels, int32_t *starts, int32_t *ends, float *conf, int32_t *counts,
                    int max_per_line, void *stream);
int cocr_forget_argmax(cocr_model *m);

/* CTC prefix beam search (kraken.lib.ctc_decoder.beam_decoder's algorithm on log-softmax(logits);
 * semantics fixed in oracle/ctc_ref.py::beam_decoder).  Same buffers as cocr_ctc_greedy; conf is a
 * softmax probability.  beam <= 32. */
int cocr_ctc_beam(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens,
                  int32_t *labels, int32_t *starts, int32_t *ends, float *conf, int32_t *counts,
                  int max_per_line, int beam, void *stream);

/* A character n-gram language model on the device (built by conformer_ocr_amd/lm.py).  All arrays HOST, copied
 * before return: unigram float32 (ncls), natural logs, entry 0 (blank) unused; two open-addressing tables with linear probing and key 0
 * = empty: (ngram_keys int64, ngram_logp float32) of ngram_slots entries for the n-grams of order >= 2, (ctx_keys, ctx_bow) of ctx_slots
 * entries for the back-off weights of the contexts.  COCR_EINVAL: a slot count that is no power of two, a table without an empty slot,
 * order outside 1..8, ncls outside 2..65535.  The model is bound to `m`'s device, not to `m`. */
typedef struct cocr_lm cocr_lm;
int cocr_lm_create(cocr_model *m, int order, int ncls, const float *unigram, const int64_t *ngram_keys, const float *ngram_logp,
                   int64_t ngram_slots, const int64_t *ctx_keys, const float *ctx_bow, int64_t ctx_slots, cocr_lm **lm);
void cocr_lm_destroy(cocr_lm *lm);

/* cocr_ctc_beam with the language model in the ranking (shallow fusion; the definition is conformer_ocr_amd/lm.py beam_decode_host):
 * a frame's candidate classes are blank + its min(classes, ncls - 1) best non-blank classes (ties: smaller class); a prefix created as
 * parent + (s,) carries lmv = lmv(parent) + (alpha * lm(parent, s) + beta); candidates rank by logaddexp(p_b, p_nb) + lmv.  Buffers and
 * ownership as for cocr_ctc_beam.  score: (N,2) float32, DEVICE or pinned host, or NULL: the CTC log-probability logaddexp(p_b, p_nb)
 * of the returned prefix and its lmv.  beam <= 32, 1 <= classes <= 64, ncls = the language model's.  With alpha = beta = 0 and
 * classes >= beam + 1 every output equals cocr_ctc_beam's.  A damaged table may give wrong text, never a hang: every probe sequence ends
 * at an empty slot or after `slots` probes.  Deterministic (no atomics).  Stream-ordered, does not synchronise (workspace growth does). */
int cocr_ctc_beam_lm(cocr_model *m, cocr_lm *lm, const float *logits, int N, int T, int ncls, const int32_t *out_lens,
                     int32_t *labels, int32_t *starts, int32_t *ends, float *conf, int32_t *counts, int max_per_line,
                     int beam, int classes, float alpha, float beta, float *score, void *stream);

/* N-best output (the definition is conformer_ocr_amd/nbest.py nbest_host): the search of cocr_ctc_beam (lm NULL;
 * classes, alpha, beta ignored) or of cocr_ctc_beam_lm, returning the first min(nbest, live) prefixes of the final beam in beam order,
 * live = the prefixes alive after the last frame (a line of length 0: the empty prefix alone).  labels / starts / ends / conf:
 * (N, nbest, max_per_line), records as the 1-best decoders write them; counts (N, nbest): the full label count of each hypothesis
 * (rows truncated at max_per_line); nhyp (N): min(nbest, live); scores (N, nbest, 2) float32:
 *     [0] the exact CTC log-probability of the label sequence over ALL alignments (the forward recursion of the criterion on
 *         log_softmax(logits), float32) -- not the beam's pruned logaddexp(p_b, p_nb); NaN for a hypothesis of more than 255 labels
 *         (COCR_LATTICE_MAX_LABELS, the criterion's limit); 0 for the empty hypothesis of a line of length 0;
 *     [1] the float32 sum, in label order, of lm(context, label): raw, without alpha or beta, so that a caller can re-weight; 0 without lm.
 * Slots j >= nhyp[n] have counts 0 and both scores -inf.  Hypothesis 0 of every line is what cocr_ctc_beam (cocr_ctc_beam_lm) writes
 * for it, bit for bit.  All outputs DEVICE or pinned host, like the other decoders'.  Errors and limits: those of cocr_ctc_beam /
 * cocr_ctc_beam_lm, 1 <= nbest <= beam (COCR_EINVAL), out_lens within [0, T] (COCR_EINVAL), T <= 8000 (COCR_EUNSUPPORTED).
 * Deterministic (no atomics).  Stream-ordered, does not synchronise (workspace growth does). */
int cocr_ctc_beam_nbest(cocr_model *m, cocr_lm *lm /* may be NULL */, const float *logits, int N, int T, int ncls, const int32_t *out_lens,
                        int beam, int nbest, int classes, float alpha, float beta, int32_t *labels, int32_t *starts, int32_t *ends,
                        float *conf, int32_t *counts, int32_t *nhyp, float *scores, int max_per_line, void *stream);

/* The loss of the reference's training / validation step, RecognitionModel._step (model.py:119,136-142):
 *     nn.CTCLoss(reduction='sum', zero_infinity=True)(log_softmax(probits, -1).transpose(0, 1), target, encoder_lens, label_lens)
 * and its gradient with respect to `probits` (what autograd hands to the decoder's backward).  probits DEVICE float32 (N,T,ncls), the
 * output of cocr_forward; out_lens HOST (N) valid frames; targets HOST int32, the batch's labels concatenated (the reference's 1-D
 * `target`), label_lens HOST (N); blank = 0, labels in [1, ncls), at most 255 per line.  nll (N) float32, DEVICE or pinned host:
 * per-line negative log-likelihoods, 0 where no alignment exists (zero_infinity) -- the reference's scalar is their plain sum.
 * grad (N,T,ncls) DEVICE float32 or NULL (validation: loss only): d sum(nll) / d probits, zero for frames >= out_lens[n].
 * Deterministic (no floating-point atomics).  Stream-ordered, does not synchronise (workspace growth does). */
int cocr_ctc_loss(cocr_model *m, const float *probits, int N, int T, int ncls, const int32_t *out_lens, const int32_t *targets,
                  const int32_t *label_lens, float *nll, float *grad, void *stream);

/* Knowledge distillation (the definition is conformer_ocr_amd/distill.py kd_loss_host): the Kullback-Leibler term
 * between a teacher's and a student's per-frame posteriors at temperature tau,
 *     p = softmax(teacher / tau), q = softmax(student / tau) over the classes of a frame,
 *     kd[n] = tau^2 sum_{t < out_lens[n]} sum_c p(c) (log p(c) - log q(c)),        d kd[n] / d student[n,t,:] = tau (q - p),
 * i.e. tau^2 F.kl_div(log_softmax(student / tau), log_softmax(teacher / tau), reduction='sum', log_target=True) on the valid frames.
 * student, teacher DEVICE float32 (N,T,ncls); out_lens HOST (N); kd (N) float32, DEVICE or pinned host (0 for a line of length 0);
 * grad (N,T,ncls) DEVICE float32 or NULL (loss only).  accumulate = 0: grad = kd_weight tau (q - p), zero for frames >= out_lens[n];
 * accumulate = 1: grad = ctc_weight grad + kd_weight tau (q - p), frames >= out_lens[n] multiplied by ctc_weight only (the two-term
 * criterion on the gradient the CTC loss left there).  Log-probabilities come from log-softmax, so a teacher probability that underflows
 * to 0 contributes exactly 0; equal student and teacher rows give exactly 0 in kd and grad.  The logits must be finite: anything else is
 * unspecified.  Checked before any launch: N, T < 1, ncls < 2, out_lens[n] outside [0, T], a tau that is not finite and positive, a
 * weight that is not finite or is negative, accumulate other than 0 / 1 (COCR_EINVAL); ncls > 16384 (COCR_EUNSUPPORTED).  Deterministic
 * (no floating-point atomics: per-frame values, then each line's sum in index order in double).  Stream-ordered, does not synchronise
 * (scratch growth does). */
int cocr_distill_loss(cocr_model *m, const float *student, const float *teacher, int N, int T, int ncls, const int32_t *out_lens,
                      float tau, float *kd, float *grad, float ctc_weight, float kd_weight, int accumulate, void *stream);

/* Forced alignment (the definition is conformer_ocr_amd/align.py viterbi_align): the best path of each line's KNOWN
 * label sequence through log_softmax(logits) -- the CTC lattice with max in place of the sum; ties keep the earlier of (stay, from s-1,
 * from s-2); the path ends in the last label or the blank after it, the blank unless the label scores strictly higher.
 * Arguments as for cocr_ctc_loss: logits DEVICE float32 (N,T,ncls); out_lens, targets (concatenated), label_lens HOST, checked before
 * any launch (COCR_EINVAL: a label outside [1, ncls), out_lens[n] > T, more than 255 labels in a line).  Outputs DEVICE or device-visible
 * pinned host memory: starts / ends int32 and conf float32, sum(label_lens) each, packed in target order -- first and last frame of the
 * label's run and the largest softmax probability of the label over it; score (N) float32, the path's log-probability; counts (N) int32
 * = label_lens[n], or -1 where no alignment fits (score -inf; the line's starts / ends are -1, conf 0).
 * Deterministic (no atomics).  Stream-ordered, does not synchronise (workspace growth does). */
int cocr_ctc_align(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens, const int32_t *targets,
                   const int32_t *label_lens, int32_t *starts, int32_t *ends, float *conf, float *score, int32_t *counts, void *stream);

/* Text-to-page alignment (the definition is conformer_ocr_amd/align.py viterbi_align_page): the best path of each
 * page's running text through the frames of its lines in reading order -- forced alignment over the concatenated frames, where a label
 * never spans a line break, equal neighbours on the two sides of a break need no blank, and an optional label (a space of the text) may
 * be absent.  Ties keep the earlier of (stay, from s-1, s-2, s-3, s-4).
 * logits DEVICE float32 (N,T,ncls).  HOST, checked before any launch: out_lens (N); P pages; page_line_off (P+1) into page_lines, the rows
 * of logits that are each page's lines in reading order, every row in at most one page; targets (concatenated) and label_lens (P);
 * optional, one byte per label.  COCR_EINVAL: a label outside [1, ncls), out_lens[n] outside [0, T], a row outside [0, N) or named
 * twice, two adjacent optional labels or an optional first / last label, descending offsets, P < 1.  COCR_EUNSUPPORTED: a page of more
 * than 4095 labels (8191 states: 16 waves x 8 registers per lane; the form of 16 registers does not fit the register file without
 * scratch and is not offered -- longer texts go through the host definition), 65535 frames or 4096 lines; a call whose tables exceed
 * 2 GiB (then align fewer pages per call); more than 2^22 classes (a state's class travels as a byte offset beside its flags).
 * Outputs DEVICE or device-visible pinned host memory.  Per label, packed in target order: line int32 (index within the page's lines),
 * starts / ends int32 (frames within that line), conf float32; a skipped optional label has -1, -1, -1 and 0.  Per page: score float32,
 * counts int32 = label_lens[p], or -1 where the text does not fit (score -inf; the page's line / starts / ends are -1, conf 0, its line
 * scores -inf).  Per page line, packed as page_lines: line_score float32, the sum of the path's log-probabilities over the line's frames.
 * Deterministic (no atomics).  Stream-ordered, does not synchronise (ring or workspace growth does).  Leaves the greedy decoder's
 * per-frame argmax alone. */
int cocr_ctc_align_page(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens, int P, const int32_t *page_line_off,
                        const int32_t *page_lines, const int32_t *targets, const int32_t *label_lens, const uint8_t *optional, int32_t *line,
                        int32_t *starts, int32_t *ends, float *conf, float *score, int32_t *counts, float *line_score, void *stream);

/* Keyword spotting (the definition is conformer_ocr_amd/search.py spot_host): where each of Q label sequences
 * occurs in each of N lines.  With r_t(c) = logits[t, c] - max_c' logits[t, c'], a candidate ending at frame t is the best path that
 * spells the query over some window [start, t] -- first frame on the first label, last frame on the last label, blanks between labels
 * optional except between equal ones -- and its score the sum of r over the window: the log-ratio to the unconstrained best path
 * there, 0 exactly when the query's path is the frame-wise argmax.  Ties keep the earlier of (stay, from s-1, from s-2, fresh start).
 * Up to `hits` non-overlapping candidates are selected per (line, query), best first (ties: the later end); the selection stops at
 * the first candidate below min_score (-inf: none).
 * logits DEVICE float32 (N,T,ncls); out_lens (N), queries (concatenated) and query_lens (Q) HOST, checked before any launch:
 * COCR_EINVAL for a label outside [1, ncls), a query length outside 1..255, out_lens[n] outside [0, T], hits outside 1..8, Q < 1 or a
 * NaN min_score; COCR_EUNSUPPORTED for T > 8000.  Outputs DEVICE or device-visible pinned host memory: starts / ends int32 and score
 * float32 (N,Q,hits), counts int32 (N,Q); entries past the count are -1 / -1 / -inf.  Does not touch the greedy decoder's argmax
 * scratch.  Deterministic (no atomics).  Stream-ordered, does not synchronise (ring or workspace growth does). */
int cocr_ctc_spot(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens, const int32_t *queries,
                  const int32_t *query_lens, int Q, int hits, float min_score, int32_t *starts, int32_t *ends, float *score,
                  int32_t *counts, void *stream);

/* Pattern spotting (the definition is conformer_ocr_amd/pattern.py spot_pattern_host): where each of Q patterns
 * -- graphs of label states, compiled from regular expressions by pattern.compile_pattern -- matches in each of N lines.  Pattern i has
 * state_counts[i] = P label states; state p has class classes[p] in [1, ncls), flags[p] (1: a match may begin in it, 2: a match may end
 * in it) and the strictly ascending predecessors preds[pred_off[p] .. pred_off[p + 1]) (a state may precede itself); a blank state
 * follows every label state.  The tables of the patterns are concatenated: classes and flags sum(P) entries, pred_off P + 1 entries per
 * pattern, each list beginning at 0, preds sum(edges).  Scores, ties within a state (stay, the predecessors in list order -- blank
 * state first, then the label state if the classes differ --, fresh start) and the selection are cocr_ctc_spot's; among the last
 * states of equal score the lowest wins and is reported in `finals`.  A pattern that is a plain chain gives cocr_ctc_spot's results.
 * logits DEVICE float32 (N,T,ncls); out_lens and the tables HOST, checked before any launch: COCR_EINVAL for a class outside
 * [1, ncls), P outside 1..256, more than 4096 edges, a predecessor outside [0, P) or a list not strictly ascending, a pattern without a
 * first or without a last state, out_lens[n] outside [0, T], hits outside 1..8, Q < 1 or a NaN min_score; COCR_EUNSUPPORTED for
 * T > 8000 or more than 65535 lines.  Outputs DEVICE or device-visible pinned host memory: starts / ends / finals int32 and score
 * float32 (N,Q,hits), counts int32 (N,Q); entries past the count are -1 / -1 / -1 / -inf.  Does not touch the greedy decoder's argmax
 * scratch.  Deterministic (no atomics).  Stream-ordered, does not synchronise (ring or workspace growth does). */
int cocr_ctc_spot_pattern(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens, const int32_t *state_counts,
                          const int32_t *classes, const int32_t *flags, const int32_t *pred_off, const int32_t *preds, int Q, int hits,
                          float min_score, int32_t *starts, int32_t *ends, float *score, int32_t *finals, int32_t *counts, void *stream);

/* The search index (the definition is conformer_ocr_amd/index.py pack_host / expand_host): pruned, quantised
 * frame posteriors that cocr_ctc_spot can be run on later, without the model.
 * cocr_posterior_pack: per frame the `keep` classes of the largest logit, ties to the lower class, stored in that order (entry 0 is the
 * frame's argmax), each with code = min(255, ceil(float32(float32(max - logit) * inv_step))): one float32 subtraction, one float32
 * multiply (never fused), ceil -- so code == 0 exactly where the logit equals the frame's maximum; a difference of +inf codes as 255.
 * Logits are finite, or -inf beside a finite row maximum; NaN is outside the contract.
 * logits DEVICE float32 (N,T,ncls); out_lens (N) HOST, checked before any launch: COCR_EINVAL for out_lens[n] outside [0, T], keep
 * outside 1..min(ncls, 32) or an inv_step that is not finite and positive; COCR_EUNSUPPORTED for ncls > 65535, N > 65535 or more than
 * 2^31 - 1 frames.  classes uint16 and codes uint8 (N,T,keep): DEVICE or device-visible pinned host memory; the entries of frames at
 * or beyond out_lens[n] are written as class 0 / code 255, so the buffers are fully defined.  Does not touch the greedy decoder's
 * argmax scratch.  Deterministic (no atomics).  Stream-ordered, does not synchronise (ring growth does).
 * cocr_posterior_unpack: classes / codes DEVICE (N,T,keep) -> logits_out DEVICE float32 (N,T,ncls), the table cocr_ctc_spot takes:
 * -(float32(code) * step) for the stored classes (one float32 multiply), -(255 * step) for every other class; each row's maximum is
 * 0 when entry 0 has code 0, as cocr_posterior_pack writes it.  A frame of all-255 codes comes out as a row of floors.  The stored
 * classes cannot be checked on the host without a copy: an entry whose class is >= ncls is IGNORED by the kernel (no store leaves the
 * row); of two entries of one class the later one wins.  COCR_EINVAL for keep outside 1..min(ncls, 32) or a step that is not finite
 * and positive; COCR_EUNSUPPORTED for ncls > 65535 or more than 2^31 - 1 frames.  Deterministic.  Stream-ordered, does not synchronise. */
int cocr_posterior_pack(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens, int keep, float inv_step,
                        uint16_t *classes, uint8_t *codes, void *stream);
int cocr_posterior_unpack(cocr_model *m, const uint16_t *classes, const uint8_t *codes, int N, int T, int keep, int ncls, float step,
                          float *logits_out, void *stream);

/* Training step of the output layer: the part of the reference's `training_step` (model.py:147-152, autograd through
 * `nn['decoder'] = nn.Linear(encoder_dim, num_classes)`, model.py:115) between the encoder output and the criterion, and the
 * reference's default optimizer (`torch.optim.AdamW`, model.py:47,283-284).  The encoder's backward is not in this library yet;
 * with these calls the output layer trains on a frozen backbone (`freeze_backbone`, default_specs.py:47).
 * cocr_decoder_backward: grad_probits DEVICE float32 (N,T,ncls) = d loss / d probits (cocr_ctc_loss) for the LAST cocr_forward on this
 * model (N, T must match it: the encoder output it multiplied is still in the workspace) ->
 *   grad_weight (ncls, encoder_dim), grad_bias (ncls): DEVICE float32, the `.grad` of decoder.weight / decoder.bias;
 *   grad_output (N,T,encoder_dim) DEVICE float32 or NULL: d loss / d encoder output (what the encoder's backward would receive).
 * Deterministic (fixed-order reductions).  Stream-ordered.
 * cocr_decoder_adamw: one torch.optim.AdamW step (decoupled weight decay, no amsgrad) on decoder.weight / decoder.bias with the given
 * gradients (after the caller's all-reduce across ranks, if any); keeps an fp32 master copy and the two moment buffers inside the
 * model (created on the first call: step counter 1), and writes the updated values where the next cocr_forward reads them.
 * cocr_finalize / cocr_blob_import discard that state.
 * cocr_get_tensor: decoder.weight / decoder.bias as float32 into HOST memory (the trained master copy if training has started, else
 * the tensor given to cocr_set_tensor) -- for writing checkpoints.  Synchronises `stream`. */
int cocr_decoder_backward(cocr_model *m, const float *grad_probits, int N, int T, float *grad_weight, float *grad_bias, float *grad_output,
                          void *stream);
int cocr_decoder_adamw(cocr_model *m, const float *grad_weight, const float *grad_bias, float lr, float beta1, float beta2, float eps,
                       float weight_decay, void *stream);
int cocr_get_tensor(cocr_model *m, const char *name, float *host_out, int64_t max_elems, void *stream);

/* Line pre-processing in front of the path -- the step the reference delegates to kraken's
 * ImageInputTransforms(1, 96, 0, 1, (16, 0), valid_norm=False) (reference dataset.py:89, cli/test.py:156): grayscale, scale to
 * height `out_h` keeping the aspect ratio (Pillow's 8-bit LANCZOS resampler, bit for bit), `pad` zero columns left and right,
 * right-zero-filled to the batch width.  Input: N raw 8-bit line crops packed in one DEVICE buffer `pixels` (line i starts at
 * byte offsets[i], heights[i] rows of widths[i] pixels of channels[i] = 1 (L) or 3 (RGB, converted like Pillow) bytes;
 * channels == NULL: all 1).  Output: `out` (N, out_h, out_w) uint8 on the device -- the COCR_U8 line batch of cocr_forward
 * (pixel / 255 are the reference's [0, 1] floats) -- and out_widths[i] (HOST) = scaled width + 2 pad, the batch's `seq_lens`.
 * Errors: COCR_EINVAL if a scaled line does not fit out_w.  Synchronises `stream` once (tap tables are built on the host).
 * cocr_preproc_width: the width line (h, w) will have, for choosing out_w / bucketing before the call. */
int32_t cocr_preproc_width(int32_t h, int32_t w, int32_t out_h, int32_t pad);
int cocr_preproc_lines(cocr_model *m, const uint8_t *pixels, const int64_t *offsets, const int32_t *heights, const int32_t *widths,
                       const int32_t *channels, int N, int out_h, int pad, int out_w, uint8_t *out, int32_t *out_widths, void *stream);

/* Baseline line extraction in front of cocr_preproc_lines -- the step kraken's `extract_polygons` performs for the reference's
 * `cocr ocr` (README.rst:32-39), with this library's own definition (not pinned against kraken): every text line
 * of a page is masked by its boundary polygon and resampled along its baseline into a straight grayscale strip.
 * Pages: P 8-bit images in DEVICE memory, page p at pages[p] (a HOST array of device pointers), page_dims[3p..3p+2] = rows, columns,
 * channels (1 = L, 3 = RGB, converted like Pillow).  Lines (all arrays HOST): line i lies on page line_page[i];
 * line_dims[3i..3i+2] = strip rows H_s (<= 4096), columns W_s (<= 65535), baseline row T; its W_s column frames follow the previous
 * lines' in `cols` as (Bx, By, Nx, Ny) int64 in 1/65536 px; its nverts[i] (3 .. 4096) integer boundary vertices follow theirs in
 * `verts` as (x, y) pairs.  Strip pixel (r, c) = bilinear sample (1/256 px, integer blend) of the page at B(c) + (r - T) N(c);
 * neighbours outside the page or the polygon (even-odd rule, half-open spans) count as `fill` (0 .. 255).  Output: strip i as
 * H_s rows of W_s bytes at byte out_offsets[i] of the DEVICE buffer `out` -- the packed input of cocr_preproc_lines (channels 1).
 * Errors: COCR_EINVAL naming the line index for a line over a limit or with coordinates beyond +-2^24 px.  Synchronises `stream`
 * once (the tables are uploaded from host memory). */
int cocr_extract_lines(cocr_model *m, const uint8_t *const *pages, const int32_t *page_dims, int P, const int32_t *line_page,
                       const int32_t *line_dims, const int64_t *cols, const int32_t *verts, const int32_t *nverts, int N, int fill,
                       uint8_t *out, const int64_t *out_offsets, void *stream);

/* Training-time augmentation of a pre-processed line batch -- the step the reference hands to kraken's default augmenter
 * (albumentations, on the host, after scaling each line; reference dataset.py), with this library's own definition (DESIGN.md
 * section 7b; not pinned against kraken): `in` (N, H, W) uint8 DEVICE, the batch cocr_preproc_lines wrote, seq_lens HOST int32 (N) its
 * line widths; `out` a DEVICE buffer of the same shape (not `in`).  params DEVICE int64 (N, 16): per line seq_len, stage flags
 * (1 geometry, 2 control-grid displacement, 4 blur, 8 pixel dropout), the inverse affine map (a0 .. a5, 1/65536 px), blur kind
 * (1 box 3x3, 2 median 3x3, 3 motion), motion length and direction, dropout threshold (of 65536) and hash key; the table's seq_len must
 * equal seq_lens[i] (the kernel clamps it to [0, W]).  grid DEVICE int32 (N, grid_cols, 3): (dx, dy, shear) in 1/65536 px at columns
 * 0, 32, 64, ...; grid_cols >= (W - 1) / 32 + 2.  Pixels of a line read only [0, H) x [0, seq_len) of `in` (anything else is 0);
 * columns >= seq_len are copied unchanged.  Integer arithmetic throughout.  Errors: COCR_EINVAL before any launch for a shape over
 * the limits (H <= 4096, W <= 65535), seq_lens[i] > W, or a grid too small for W.  Never synchronises `stream`. */
int cocr_augment_lines(cocr_model *m, const uint8_t *in, uint8_t *out, int N, int H, int W, const int32_t *seq_lens, const int64_t *params,
                       const int32_t *grid, int grid_cols, void *stream);

/* Batched edit-distance alignment -- the scoring behind CER / WER and the confusion report (evaluate.global_align is the definition,
 * tie-breaking included): unit costs, cost[i][0] = i, cost[0][j] = j; the traceback from (n, m) prefers the diagonal
 * step when cost[i][j] == cost[i-1][j-1] + (a[i-1] != b[j-1]), else the deletion when cost[i][j] == cost[i-1][j] + 1, else the insertion.
 * P pairs of int32 symbol sequences (compared for equality only), packed: pair p is a[a_offs[p] .. a_offs[p+1]) (the ground truth) against
 * b[b_offs[p] .. b_offs[p+1]) (the prediction).  a, b DEVICE; a_offs, b_offs HOST int64 (P + 1): they are checked here, decide the
 * launches, and reach the kernels through a pinned ring of the model.  Outputs, all DEVICE (or device-visible pinned memory):
 * counts int32 (P, 4), 16-byte aligned = (distance, insertions, deletions, substitutions) per pair; ops (optional, NULL: counts only), one
 * byte per alignment column: 0 equal, 1 substitution, 2 deletion (a symbol of a against a gap), 3 insertion (a gap against a symbol of b).
 * Pair p owns the slot of len_a + len_b bytes starting at byte (a_offs[p] - a_offs[0]) + (b_offs[p] - b_offs[0]); its alignment, in
 * forward order, fills the LAST ops_len[p] bytes of the slot (ops_len int32 (P), required with ops), the bytes before are left as they
 * were.  Limits, COCR_EINVAL before any launch: a sequence longer than 4096 symbols, negative or decreasing offsets, P < 0.  P = 0 and
 * empty sequences are valid.  Stream-ordered; does not synchronise `stream` (a growth of the ring or of the workspace waits for the
 * device once).  cocr_edit_align_lds: the bytes of LDS a pair of these lengths takes when its op-code table is kept in LDS, 0 when the
 * table goes to the model's global workspace (more than 64 KB, or more than COCR_SCORE_LDS_MAX); negative on an error. */
int cocr_edit_align(cocr_model *m, const int32_t *a, const int64_t *a_offs, const int32_t *b, const int64_t *b_offs, int P, int32_t *counts,
                    uint8_t *ops, int32_t *ops_len, void *stream);
int64_t cocr_edit_align_lds(cocr_model *m, int len_a, int len_b);

/* Launch-overhead control: with graph replay on, cocr_forward captures its ~40 kernel launches into a hipGraph and
 * replays it.  A caller that reuses (lines, logits, N, W, dtype, stream) gets a graph on its own buffers (second
 * identical call captures, later ones replay; contents may change, addresses not).  A caller with fresh buffers per
 * call gets a graph keyed by (N, W, dtype, stream) on library-owned staging buffers: one device-to-device copy of the
 * lines in and of the logits out per call.  Off by default. */
int cocr_set_graph(cocr_model *m, int on);

/* Rows of the (N*T, D) activation one workgroup of the row-chain kernels owns (bf16 mode, encoder_dim 256 / 512).
 * 0 (default): by the batch's row count and by how many batches this process can really overlap (cocr_get_chain_rows) -- the
 * largest block that keeps the chip covered (up to 96 rows at D = 256, 64 at D = 512: every weight byte is streamed once per
 * block, the cheapest form when several batches are in flight).  A caller with ONE batch in flight
 * gets a shorter forward from smaller blocks (e.g. 48: twice the workgroups, 32 lines x 300 frames = 200 workgroups).
 * Same results bit for bit (a row's arithmetic does not depend on the block it is in). */
int cocr_set_chain_rows(cocr_model *m, int rows);

/* The rows per workgroup the next cocr_forward of an (N, H, W) batch would run its row-chain launches with (0: this model's
 * forward does not use them).  Host arithmetic, no GPU call.  A value set with cocr_set_chain_rows (or COCR_CHAIN_ROWS) is
 * mapped to the nearest built form (D = 256: 96, 64, 48, 32; D = 512: 64, 32).  Otherwise a model alone on its weights gets
 * the tallest form from 50 workgroups on, else 32.  Models that share one set of weights (cocr_share_weights: S of them, the
 * owner included) are taken for S batches in flight: their streams run on max(1, GPU_MAX_HW_QUEUES - 1) hardware queues
 * (the variable as read once by this library: 4 when unset, 1..32), streams on one queue run in turn, so
 * c = S / ceil(S / queues) forwards overlap; the tallest form with at least 50 workgroups whose workgroups x c cover the 256
 * CUs is chosen, else the shortest such form.  32 x 300 frames, four models: 64 rows on 4 queues, 96 on 8. */
int cocr_get_chain_rows(cocr_model *m, int N, int W, int *rows);

/* Test taps: with debug on, cocr_forward keeps a float32 copy of every stage output
 * ("front.z2", "front.z3", "front.y", "l<i>.ffn1|mhsa|conv|ffn2|out", "l<i>.q|k|v|ctx|glu|dw").
 * cocr_debug_tap copies one to HOST memory; *n_elems receives its element count. */
int cocr_set_debug(cocr_model *m, int on);
int cocr_debug_tap(cocr_model *m, const char *name, float *host_out, int64_t max_elems, int64_t *n_elems);

/* Test entry: block `layer`'s attention core alone -- the one launch cocr_forward makes between the q / k / v projection and the
 * out-projection -- on the caller's DEVICE tensors in the model's compute type.  q, k, v: [N][heads][Tp][dhp] (Tp = T rounded up to 64,
 * dhp = the engine's d_head rounded up to 32), ZERO in the rows beyond T and the columns beyond d_head: the kernels read whole tiles.
 * ctx: [N][T][heads * dh], dh the engine's d_head (a zero-padded narrow model: its slot, the model's own columns first).  The
 * positional table, u / v biases, scale and the kernel form (COCR_ATT_TILED, COCR_ATT_RESIDENT_MIN, COCR_ATT_RESIDENT_LONG) are
 * those of a forward of N lines of T frames.  qkv_elems / ctx_elems: the element counts of the buffers, checked against the layout.
 * dims (may be null) receives {heads, dh, dhp, Tp}; with q, k, v and ctx all null nothing is launched (the layout alone). */
int cocr_debug_attention(cocr_model *m, int layer, int N, int T, const void *q, const void *k, const void *v, int64_t qkv_elems, void *ctx,
                         int64_t ctx_elems, int32_t *dims, void *stream);

/* Kernel timing hook for bench.py's roofline leg: average device time (ms) per launch of each
 * kernel family over the forwards run since cocr_profile(m,1), measured with HIP events on the
 * forward's own stream.  Names are '\n'-separated in `names`; ms[i], launches[i] per family. */
int cocr_profile(cocr_model *m, int on);
int cocr_profile_read(cocr_model *m, char *names, size_t names_len, double *ms, int64_t *launches, int max_entries);

/* ---- Training step of the whole network: RecognitionModel.training_step (model.py:129-152) + torch.optim.AdamW (model.py:283-284).
 * fp32.  cocr_train_begin copies every parameter / buffer given through cocr_set_tensor to the device (optimizer state zeroed);
 * cocr_train_step runs the TRAIN-mode forward (BatchNorm1d batch statistics over all positions of the padded batch + running-statistics
 * update, dropout at the reference's six sites with probabilities dropout_p = {input, feed_forward, attention, conv}, masks from
 * (seed, site, index)), the criterion nn.CTCLoss(reduction='sum', zero_infinity=True) on log_softmax(probits), and the backward through
 * decoder and encoder: afterwards cocr_train_get(name, kind = 1) returns d loss / d parameter for every reference state-dict name
 * (kind = 0: the current value of a parameter / buffer).  lines as for cocr_forward; in_lens, targets (concatenated labels),
 * label_lens HOST int32; *loss_out HOST.  cocr_train_adamw applies one AdamW step to all parameters; cocr_train_end copies the trained
 * values back into the model's state (call cocr_finalize again to serve them) and frees the training state. */
int cocr_train_begin(cocr_model *m);
int cocr_train_step(cocr_model *m, const void *lines, int line_dtype, int N, int H, int W, const int32_t *in_lens, const int32_t *targets,
                    const int32_t *label_lens, const float *dropout_p, uint64_t seed, float *loss_out, void *stream);
/* The step with a teacher: the criterion is (1 - weight) sum CTC + weight sum KD, KD as cocr_distill_loss defines
 * it at temperature tau between the step's own logits and teacher_logits, DEVICE float32 (N, T, ncls) with T = cocr_out_len(W) -- the
 * teacher's eval-mode forward on the same batch.  loss_out HOST [2]: the summed CTC loss and the summed KD, both unweighted.  Everything
 * else is the step above, which keeps its launches and its bits; with weight = 0 the gradient is that step's gradient bit for bit and KD
 * is still reported.  COCR_EINVAL: teacher_logits NULL, weight outside [0, 1], tau not finite and positive. */
int cocr_train_step_distill(cocr_model *m, const void *lines, int line_dtype, int N, int H, int W, const int32_t *in_lens,
                            const int32_t *targets, const int32_t *label_lens, const float *dropout_p, uint64_t seed,
                            const float *teacher_logits, float tau, float weight, float *loss_out, void *stream);
int cocr_train_get(cocr_model *m, const char *name, int kind, float *host_out, int64_t n_elems, void *stream);
int cocr_train_adamw(cocr_model *m, float lr, float beta1, float beta2, float eps, float weight_decay, void *stream);
int cocr_train_end(cocr_model *m);
/* Matmul precision of the training step's Linear / pointwise-conv products (forward, input and weight gradients): 0 (default) exact fp32
 * on the matrix cores; 1 = both operands rounded to bf16, fp32 accumulation -- what the reference trains under
 * (torch.set_float32_matmul_precision('medium'), cli/train.py:252).  Parameters, activations, gradients and the optimizer stay fp32. */
int cocr_train_set_matmul(cocr_model *m, int bf16_operands);
/* The flat device gradient vector (float32, all parameters): a data-parallel job all-reduces it between cocr_train_step and cocr_train_adamw. */
int cocr_train_grad_buffer(cocr_model *m, void **device_ptr, size_t *n_floats);
/* The flat device VALUE vector in the same layout (parameters [0, *n_params), then the BatchNorm running statistics up to *n_total) and
 * the place of a reference state-dict name in both vectors.  This is what puts the step behind torch autograd (reference
 * model.py:129-152: `loss.backward()`, then any torch optimizer, model.py:283-289): the host copies `net.nn.parameters()` in, runs
 * cocr_train_step, hands slices of the gradient vector to autograd and copies the running statistics out -- conformer_ocr_amd/autograd.py. */
int cocr_train_param_buffer(cocr_model *m, void **device_ptr, size_t *n_total, size_t *n_params);
int cocr_train_layout(cocr_model *m, const char *name, int64_t *offset, int64_t *n_elems, int *is_param);
/* Hand-over from a frozen-backbone phase: the output layer of `src` as cocr_decoder_adamw left it -- fp32 master copy of decoder.weight /
 * decoder.bias, both AdamW moments and the step count k -- moves into the training state of `dst` (the tensors' cocr_train_layout offsets),
 * device to device and ordered on `stream`.  cocr_train_adamw keeps PER-TENSOR step counts from then on: the adopted layer continues
 * with the bias corrections of step k + 1, every other parameter with its own count (torch.optim.AdamW's state['step'] per parameter);
 * with equal counts the step is the one it was.  A `src` that never took an optimizer step hands over its values, zero moments and
 * k = 0.  COCR_ESTATE: `dst` has no training state; COCR_EINVAL: the two output layers differ in shape or device. */
int cocr_train_adopt_decoder(cocr_model *dst, cocr_model *src, void *stream);

/* One optimizer step of any of the reference's four kinds (`--optimizer`, model.py:283-289) on the gradients of the last cocr_train_step:
 * cocr_train_optim_step over all parameters, cocr_decoder_optim_step on the output layer of a finalized model (the frozen-backbone
 * phase; as cocr_decoder_adamw it keeps an fp32 master copy and writes the values where the next cocr_forward reads them).
 * Per element, in fp32, torch's single-tensor definitions; g' = g + weight_decay p for every kind but AdamW:
 *   AdamW    p *= 1 - lr weight_decay;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;
 *            p -= lr / (1 - beta1^t) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)         -- bit for bit what cocr_train_adamw computes
 *   Adam     the same moments and update on g', no decoupled decay (L2 decay folded into the gradient)
 *   SGD      buf = momentum buf + g';  p -= lr buf;  momentum = 0: p -= lr g' (dampening 0, no Nesterov, as the reference constructs it)
 *   RMSprop  sq = alpha sq + (1 - alpha) g'^2;  a = sqrt(sq) + eps;  momentum > 0: buf = momentum buf + g' / a, p -= lr buf;
 *            else p -= lr g' / a                                                       (not centered)
 * The optimizer state is two float vectors ("slots") beside the parameters, zeroed by cocr_train_begin; their meaning depends on the kind:
 *   AdamW, Adam: slot 0 exp_avg, slot 1 exp_avg_sq;   SGD: slot 0 momentum buffer;   RMSprop: slot 0 square_avg, slot 1 momentum buffer.
 * A state remembers the kind of its first step: a step of another kind is COCR_ESTATE (cocr_train_adamw / cocr_decoder_adamw count as
 * AdamW steps).  Hyper-parameters outside torch's own checks (negative lr, weight_decay, eps, momentum or alpha, a beta outside [0, 1))
 * are COCR_EINVAL.  Unused fields of cocr_optim are ignored (torch's defaults: beta 0.9 / 0.999, eps 1e-8, alpha 0.99).
 * cocr_train_adopt_decoder hands over slots and step count whatever the kind and refuses (COCR_EINVAL) two states that have taken
 * steps of different kinds; the per-tensor step counts matter to AdamW and Adam only.  Stream-ordered, no synchronisation. */
enum { COCR_OPT_ADAMW = 0, COCR_OPT_ADAM = 1, COCR_OPT_SGD = 2, COCR_OPT_RMSPROP = 3 };
typedef struct { int kind; float lr, weight_decay, beta1, beta2, eps, momentum, alpha; } cocr_optim;
int cocr_train_optim_step(cocr_model *m, const cocr_optim *o, void *stream);
int cocr_decoder_optim_step(cocr_model *m, const float *grad_weight, const float *grad_bias, const cocr_optim *o, void *stream);

/* The gradient window: accumulation over several cocr_train_step calls, the global L2 norm, and the clipped step.
 * The first two work on raw DEVICE vectors of floats (any float offset of an allocation) on `device` and belong to no model: they serve
 * the whole-network gradient vector and the frozen phase's two small output-layer gradients alike.
 * cocr_grad_accumulate: per element t = fl(scale src[i]), then dst[i] = overwrite ? t : fl(dst[i] + t) -- two fp32 operations, each
 * rounded on its own, torch's acc.add_(g * s) bit for bit.  dst == src is legal with overwrite: the in-place scale.  16 bytes per lane
 * where dst and src are aligned alike, one float at a time before, behind and otherwise.  Stream-ordered, no synchronisation, no
 * allocation.
 * cocr_grad_norm: *norm_out (HOST) = sqrt(sum g[i]^2), every square formed and every sum taken in double: partial sums over a number of
 * contiguous chunks that depends on n only, added in index order by a second small kernel -- no atomics, so the result is a function of
 * the values and n alone, the same bits on every call and at every alignment of g.  Relative error <= n 2^-53.  IEEE on non-finite
 * input: an Inf gives +Inf, a NaN (with or without an Inf) NaN.  n = 0 gives 0 and launches nothing.  Squares of 1e30 or 1e-30 neither
 * overflow nor vanish.  The result comes back through pinned host memory; the call SYNCHRONISES `stream`.  Its scratch (8 KB per device)
 * is allocated on the first call on a device and kept.
 * cocr_train_optim_step_ex: cocr_train_optim_step with the gradient read from `grad` (DEVICE, the layout of cocr_train_grad_buffer; NULL:
 * the state's own vector) and every gradient element entering the step as fl(grad_scale g).  cocr_train_optim_step IS
 * cocr_train_optim_step_ex(m, o, NULL, 1.0f, stream): fl(1.0f g) == g for every float, so it keeps its bits.  grad_scale must be finite
 * and >= 0 (else COCR_EINVAL), with one exception: NaN is taken, because torch's clip makes a NaN coefficient of a NaN norm; the
 * Python Trainer never passes one (it skips or refuses a window whose norm is not finite).  Stream-ordered, no synchronisation. */
int cocr_grad_accumulate(float *dst, const float *src, size_t n, float scale, int overwrite, int device, void *stream);
int cocr_grad_norm(const float *g, size_t n, int device, double *norm_out, void *stream);
int cocr_train_optim_step_ex(cocr_model *m, const cocr_optim *o, const float *grad, float grad_scale, void *stream);

/* The optimizer state out of the library and back, for continuing an interrupted fit.
 * cocr_train_optim_state: the kind (-1 before the first step), the step count, the steps an adopted output layer is ahead, and DEVICE
 * pointers to the two slots (*n_floats each: the layout of cocr_train_grad_buffer).  The caller copies them out; to restore it writes
 * values (cocr_train_param_buffer) and slots back and then calls cocr_train_optim_restore with the three counters.
 * cocr_decoder_optim_state: the output layer's state of a finalized model, *state a DEVICE pointer to *n_floats floats
 * [master copy | slot 0 | slot 1] in the engine's layout, NULL before the first step (*n_floats is set either way).
 * cocr_decoder_optim_restore copies such a vector in (device to device, ordered on `stream`), sets kind and step count, and writes the
 * master copy's values where cocr_forward reads them.  COCR_EINVAL: n_floats does not fit the model, or invalid counters. */
int cocr_train_optim_state(cocr_model *m, int *kind, int64_t *step, int64_t *dec_steps, void **slot0, void **slot1, size_t *n_floats);
int cocr_train_optim_restore(cocr_model *m, int kind, int64_t step, int64_t dec_steps);
int cocr_decoder_optim_state(cocr_model *m, int *kind, int64_t *step, void **state, size_t *n_floats);
int cocr_decoder_optim_restore(cocr_model *m, int kind, int64_t step, const float *state_device, size_t n_floats, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* COCR_H */
