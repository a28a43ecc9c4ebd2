// One set of weights and everything derived from it (Weights), and a model's captured launch sequences (GraphCache): the host-side
// bookkeeping of the host layer (model.hip.h) that is plain C++.  The two HIP calls it makes go through the macros below, so that
// tools/weights_lifecycle.cpp can drive it on the CPU under a sanitizer.
#pragma once

#include <algorithm>
#include <cstddef>
#include <memory>
#include <vector>

#ifndef COCR_DEVICE_FREE
#define COCR_DEVICE_FREE(p) (void)hipFree(p)
#define COCR_GRAPH_EXEC_DESTROY(e) (void)hipGraphExecDestroy(e)
#endif

struct FfnW { size_t ln_g, ln_b, w1, b1, w2, b2; };
struct LayerW {
    FfnW ffn[2];
    size_t a_ln_g, a_ln_b, wqkv, bqkv, ub, vb, wpos, wo, bo;       // wpos: pos_proj weight, fp32 (D, D): the positional tables are DERIVED from it
    size_t c_ln_g, c_ln_b, wpw1, bpw1, dww, dwb, wpw2, bpw2;
    size_t f_ln_g, f_ln_b;
};
struct StageW { size_t dw_w, dw_b, pw_w, pw_b; };   // one (depthwise, pointwise) frontend stage
struct BlobPlan {
    size_t w0, b0;                 // frontend conv.0 taps [C][9], bias
    std::vector<StageW> stages;    // sampling_num - 1 stages; stage 0's depthwise is fused with conv.0
    size_t wout, bout;
    std::vector<LayerW> layers;
    size_t wdec, bdec;
    size_t total = 0;
};

struct cocr_model;
struct Form;

// The packed blob of one finalize and what is derived from it, on one device.  Every model holds a counted reference to exactly one
// Weights and reads every pointer through it; nobody keeps copies.  `users` are the models that read this set, its owner first: the
// model that finalized it, the only one that may change it.  The others joined through cocr_share_weights (several packed copies of
// one model, each with its workspace, for callers that keep several batches in flight: four private copies are 4 x ~100 MB, more than
// the 256 MB Infinity Cache -- every forward then streamed its weights from HBM).
//   * The device buffers are released by the owner alone: when it finalizes again (the same object gets new buffers, the other users
//     follow) and when it leaves (destroyed, or made a sharer of another set).  `blob == nullptr` reads as "not finalized", so users
//     that outlive their owner fail cleanly.  The struct itself lives until its last user lets go.
//   * `gen` is bumped whenever a buffer may have moved or been rebuilt; a model that last ran at another generation drops its captured
//     launches (sync_weights).
struct Weights {
    int device = 0;
    int dtype = -1;                  // compute dtype of the blob (COCR_BF16 / COCR_F32); -1: never allocated
    BlobPlan plan;
    unsigned char *blob = nullptr;
    // fragment-major copies of the row-chain kernels' weight matrices (rowchain.hip.h), at the blob's offsets; derived from the blob,
    // rebuilt before the next forward whenever the blob may have changed (finalize, import, cocr_weight_blob handed out)
    unsigned char *packed = nullptr;
    bf16_t *fpack = nullptr;         // fused frontend kernel (frontend.hip.h): conv.0 A-fragments, then the depthwise block-diagonal B-fragments
    bool packed_stale = true;
    // positional tables P_l = PE Wpos_l^T, [layer][2 pos_maxlen - 1][heads][dhp] in the compute dtype: derived from the blob's wpos matrices on this
    // device -- 61 of the former 104 MB of the cfg2 blob, which every rank can compute for itself
    unsigned char *ptab = nullptr;
    size_t ptab_stride = 0;
    int pos_maxlen = COCR_POS_MAXLEN;                  // relative positions the tables cover: -(max_len - 1) .. max_len - 1
    bool ptab_stale = true;
    unsigned long long gen = 1;
    std::vector<cocr_model *> users;

    explicit Weights(int device_) : device(device_) {}
    Weights(const Weights &) = delete;
    Weights &operator=(const Weights &) = delete;
    ~Weights() { release(); }

    bool owned_by(const cocr_model *m) const { return !users.empty() && users.front() == m; }
    bool stale() const { return packed_stale || ptab_stale; }
    void invalidate() { packed_stale = ptab_stale = true; }       // the blob's values may have changed: derived copies are rebuilt by the next forward
    void release() {                                               // the device buffers go; the users read "not finalized"
        for (void *p : {(void *)blob, (void *)packed, (void *)ptab, (void *)fpack})
            if (p) COCR_DEVICE_FREE(p);
        blob = packed = ptab = nullptr;
        fpack = nullptr;
        invalidate();
        ++gen;
    }
    // (the layout's dimensions are the owner's.  ensure_packed: forward.hip, the one unit that knows a Form; the positional tables: cocr_api.hip)
    int ensure_packed(const Form &f, hipStream_t s);
    int ensure_ptab(hipStream_t s);
    template <typename T> int compute_pos_tables(hipStream_t s);
    int cover_positions(int Tp64);
};
typedef std::shared_ptr<Weights> WeightsRef;

// `m` stops reading the set `w` points at.  A sharer leaves the group; an owner takes the device buffers with it, and the set has no
// users from then on: the models that still point at it are not finalized until they get weights of their own or join another set.
static void weights_leave(WeightsRef &w, cocr_model *m) {
    if (w->owned_by(m)) {
        w->release();
        w->users.clear();
    } else {
        w->users.erase(std::remove(w->users.begin(), w->users.end(), m), w->users.end());
    }
}
// `w` becomes a set that `m` owns, without device buffers: the one it owns already (the models that share it follow), else a new one
static void weights_own(WeightsRef &w, cocr_model *m, int device) {
    if (w && w->owned_by(m)) { w->release(); return; }
    if (w) weights_leave(w, m);
    w = std::make_shared<Weights>(device);
    w->users.push_back(m);
}
// `m` reads `set`, another model's, from now on
static void weights_join(WeightsRef &w, cocr_model *m, const WeightsRef &set) {
    weights_leave(w, m);
    w = set;
    w->users.push_back(m);
}

// hipGraph replay of a model's forward: the instantiated launch sequences and the calls seen so far.  A sequence points at the
// model's workspace, at the weights' buffers and at launch shapes, so the cache is dropped whenever one of them changes.
// Two kinds of captured sequences:
//   * keyed by the caller's buffers (lines, logits, N, W, dtype): a loop that reuses its buffers replays with no extra copy;
//   * STAGED, keyed by (N, W, dtype) only: a caller that hands over fresh buffers every call (a data loader's batches, torch's
//     allocator) gets one device-to-device copy of the lines into a library-owned staging buffer, the replay, and one copy of the
//     logits out (~20 MB at 32 x 96 x 1200 f32: a few microseconds) instead of ~40 host-side launches.
// (The stream is not part of either key: an instantiated graph launches on any stream, and one model serves one stream at a time anyway.)
struct GraphCache {
    struct Call { const void *lines; float *logits; int N, W, dtype; int rows; };      // lines == nullptr: staged; rows: Form::chain_rows of the launches
    struct Entry { Call c; hipGraphExec_t exec; };
    enum Action { REPLAY, CAPTURE, STAGED_REPLAY, STAGED_CAPTURE, PLAIN };
    std::vector<Entry> graphs;       // at most 16, oldest first
    std::vector<Call> seen;          // calls that ran plain; about 32, oldest first
    GraphCache() = default;
    GraphCache(const GraphCache &) = delete;
    GraphCache &operator=(const GraphCache &) = delete;
    ~GraphCache() { drop(); }

    void drop() {
        for (Entry &g : graphs) COCR_GRAPH_EXEC_DESTROY(g.exec);
        graphs.clear();
        seen.clear();
    }
    static bool same(const Call &a, const Call &b) { return a.lines == b.lines && a.logits == b.logits && a.N == b.N && a.W == b.W && a.dtype == b.dtype; }
    static Call staged(const Call &c) { return {nullptr, nullptr, c.N, c.W, c.dtype, c.rows}; }
    // What the call `c` does, and with which sequence.  The second identical call captures, later ones replay; `shape_ready`: the
    // shape's one-time attribute / zeroing work is done (its first call runs plain whatever was seen).
    Action next(const Call &c, bool shape_ready, hipGraphExec_t *exec) {
        for (const Entry &g : graphs)
            if (g.c.N == c.N && g.c.W == c.W && g.c.rows != c.rows) {      // captured with another grid (a model joined or left the group since): as cocr_set_chain_rows
                drop();
                break;
            }
        for (const Entry &g : graphs)
            if (same(g.c, c)) { *exec = g.exec; return REPLAY; }
        const Call st = staged(c);
        bool was_seen = false, seen_shape = false;
        for (const Call &g : seen) { was_seen = was_seen || same(g, c); seen_shape = seen_shape || same(g, st); }
        if (was_seen && shape_ready) return CAPTURE;      // the caller reuses its buffers: capture on them
        if (seen.size() >= 32) seen.erase(seen.begin());
        seen.push_back(c);
        for (const Entry &g : graphs)
            if (same(g.c, st)) { *exec = g.exec; return STAGED_REPLAY; }
        if (seen_shape && shape_ready) return STAGED_CAPTURE;      // second call of the shape with other buffers
        seen.push_back(st);                               // first call of this shape: plain, on the caller's buffers
        return PLAIN;
    }
    void add(const Call &c, hipGraphExec_t exec) {
        if (graphs.size() >= 16) { COCR_GRAPH_EXEC_DESTROY(graphs.front().exec); graphs.erase(graphs.begin()); }
        graphs.push_back({c, exec});
    }
};
