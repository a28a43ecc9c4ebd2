// What every unit of the host layer sees: the error path, the grow-only buffers and upload rings, the profiler's brackets, the
// model (struct cocr_model, its state grouped by the unit that writes it) and the few functions that cross units.  The units:
//     cocr_api.hip   error buffer, model lifetime, layout, finalize / share / blob, positional tables, workspace, taps, profiler
//     forward.hip    the forward: its form, its stages, the graph cache's use, the entry point; the GEMM micro-benchmark
//     decode.hip     CTC decoders, n-gram model, criterion, distillation term, forced alignment, keyword spotting
//     lines.hip      line collation, pre-processing, page extraction, augmentation
//     score.hip      edit-distance alignment
//     train.hip      output-layer training and the training step of the whole network
// A kernel header is included by the one unit that launches from it (non-template kernels have external linkage).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/cocr.h"
#include "common.hip.h"
#include "weights.hip.h"

// not exported from the library: the functions one unit defines and another calls (declared once, at the end of this file) and the
// groups of the model's state
#define COCR_INTERNAL __attribute__((visibility("hidden")))

// ------------------------------------------------------------------------------------ errors
// One message buffer per thread, in cocr_api.hip; every unit writes it through fail() alone.
COCR_INTERNAL int fail(int code, const char *fmt, ...);
#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) return fail(COCR_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define LAUNCH_CHECK() HIP_TRY(hipGetLastError())

#define GEMM_TRY(call)                                                                                 \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return fail(COCR_EHIP, "kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// ------------------------------------------------------------------------------------ model
struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
    bool set = false;
};

// A grow-only scratch buffer of E: device memory, or pinned host memory.  grow() releases the old memory and records capacity 0
// before it allocates, so a failed allocation leaves an empty buffer, never a stale capacity.  Work still in flight that reads the
// old memory is the caller's to finish first.  The destructor releases the buffer.
template <typename E> struct DevBuf {
    E *p = nullptr;
    size_t n = 0;                       // capacity in elements
    const bool pinned;
    explicit DevBuf(bool pinned_ = false) : pinned(pinned_) {}
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr; n = 0;
    }
    hipError_t grow(size_t need, size_t alloc = 0) {     // at least `need` elements; a growth allocates max(need, alloc)
        if (need <= n) return hipSuccess;
        release();
        alloc = std::max(need, alloc);
        void *q = nullptr;
        const hipError_t e = pinned ? hipHostMalloc(&q, alloc * sizeof(E)) : hipMalloc(&q, alloc * sizeof(E));
        if (e != hipSuccess) return e;
        p = static_cast<E *>(q); n = alloc;
        return hipSuccess;
    }
};
// a device buffer and its pinned host staging, grown together to one capacity: both or neither
template <typename E> static hipError_t grow_pair(DevBuf<E> &dev, DevBuf<E> &host, size_t need, size_t alloc = 0) {
    if (need <= dev.n && need <= host.n) return hipSuccess;
    dev.release(); host.release();
    hipError_t e = dev.grow(need, alloc);
    if (e == hipSuccess && (e = host.grow(need, alloc)) != hipSuccess) dev.release();
    return e;
}

// A ring of COCR_RING_SLOTS slots for the small host tables an entry point sends ahead of its kernels: a device buffer and its pinned
// host twin (an async copy from pageable memory can block the host).  stage() hands out the next slot, 16-byte
// aligned, once the upload that last used it has run (one event per slot; a wait only for a caller more than COCR_RING_SLOTS calls
// ahead of the device); commit() enqueues the slot's copy and records its event.  A slot too small regrows the ring by half again as
// much, both buffers or neither, after a device synchronise: uploads of earlier calls still read the old buffers.
#define COCR_RING_SLOTS 16
struct UploadRing {
    DevBuf<unsigned char> dev, host{true};
    hipEvent_t ev[COCR_RING_SLOTS] = {};
    int slot = 0;                       // the slot stage() handed out last, and its byte offset in both buffers
    size_t at = 0;
    ~UploadRing() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    template <typename E> hipError_t stage(size_t bytes, E *&h, E *&d) {
        const size_t need = (bytes + 15) / 16 * 16 * COCR_RING_SLOTS;
        hipError_t e = hipSuccess;
        if (need > dev.n || need > host.n) {
            if ((e = hipDeviceSynchronize()) != hipSuccess) return e;
            if ((e = grow_pair(dev, host, need, (bytes + bytes / 2 + 15) / 16 * 16 * COCR_RING_SLOTS)) != hipSuccess) return e;
        }
        slot = (slot + 1) % COCR_RING_SLOTS;
        e = ev[slot] ? hipEventSynchronize(ev[slot]) : hipEventCreateWithFlags(&ev[slot], hipEventDisableTiming);
        at = dev.n / COCR_RING_SLOTS / 16 * 16 * (size_t)slot;
        h = reinterpret_cast<E *>(host.p + at); d = reinterpret_cast<E *>(dev.p + at);
        return e;
    }
    hipError_t commit(size_t bytes, hipStream_t s) {
        const hipError_t e = hipMemcpyAsync(dev.p + at, host.p + at, bytes, hipMemcpyHostToDevice, s);
        return e != hipSuccess ? e : hipEventRecord(ev[slot], s);
    }
};

struct ProfRec { int fam; hipEvent_t a, b; };
struct TrainState;

// The forward's workspace for (capN, capW).  Written by cocr_reserve / free_workspace (cocr_api.hip) and by the forward (forward.hip).
struct COCR_INTERNAL Workspace {
    int capN = 0, capW = 0;
    std::vector<void *> ws_allocs;
    void *z_a = nullptr, *z_b = nullptr;
    float *x = nullptr, *x2 = nullptr;  // the fp32 stream; its second buffer (the chains with the out-proj -> GLU head read one and write the other)
    void *g_lines = nullptr;           // staged graph replay (cocr_forward): library-owned copies of the caller's lines / logits
    float *g_logits = nullptr;
    void *xn = nullptr, *hid = nullptr, *q = nullptr, *k = nullptr, *vt = nullptr, *ctx = nullptr, *glu = nullptr, *dwo = nullptr;
    size_t qkv_bytes = 0;
    int vtN = -1, vtT = -1;    // shape the q/k/vt buffers were last zeroed for
    int lastN = 0, lastT = 0;                          // shape of the last forward: its encoder output is still in `xn`
};

// What the caller switches: the COCR_* environment switches (SWITCHES[], read by cocr_create) and the setters' flags.  Written by
// cocr_api.hip (cocr_create, cocr_set_debug, cocr_profile) and by forward.hip's setters (cocr_set_chain_rows, cocr_set_graph).
struct COCR_INTERNAL Switches {
    bool use_graph = false;      // cocr_set_graph: hipGraph replay of the forward's launch sequence
    bool debug = false;
    bool profile = false;
    bool no_pad = false;         // COCR_NO_PAD=1: never run a narrow model as a zero-padded 256-wide one
    bool beam_ref = false;       // COCR_BEAM_REF=1: the exhaustive beam kernel (all beam x C candidates per frame) also for <= 256 classes
    bool no_front96 = false;     // COCR_NO_FRONT96=1: frontend conv stages as separate kernels (A/B)
    bool no_front32 = false;     // COCR_NO_FRONT32=1: 32 conv channels: the pointwise conv as a GEMM launch of its own (A/B)
    bool no_dw_fuse = false;     // COCR_NO_DW_FUSE=1: depthwise conv as its own launch (A/B)
    bool no_a_fuse = false;      // COCR_NO_A_FUSE=1: out-proj -> GLU (chain A) as a launch of its own in front of chain B instead of chain B's head (A/B)
    int chain_rows = 0;          // rows per workgroup of the row-chain kernels (cocr_set_chain_rows / COCR_CHAIN_ROWS); 0 = by the number of rows
    bool no_front_chain = false; // COCR_NO_FRONT_CHAIN=1: the frontend's output linear as a split-K GEMM + reduction in front of the first chain launch (A/B)
    bool ffn_probe = false;      // COCR_FFN_PROBE=1: one extra FFN-only row-chain launch per forward (measurement; results discarded)
    int att_resident_min = 192;  // COCR_ATT_RESIDENT_MIN: fewest workgroups for which the LDS-resident attention kernel is chosen (tests: 1)
    bool att_resident_long = false;   // COCR_ATT_RESIDENT_LONG=1: the LDS-resident attention kernel also for lines of more than 320 frames (key passes; A/B)
    bool att_tiled = false;      // COCR_ATT_TILED=1: the tiled attention kernel also for lines of <= 320 frames (A/B against the LDS-resident one)
    bool no_kskip = false;       // COCR_NO_KSKIP=1: zero-padded narrow models multiply their zero k-steps too (A/B)
    bool chain_xcd = true;       // COCR_CHAIN_XCD=0: row blocks in plain workgroup order (A/B)
    bool no_chain = false;       // COCR_NO_CHAIN=1: one kernel per GEMM / FFN instead of the row-local chains (A/B measurements)
    int score_lds_max = 64 * 1024;   // COCR_SCORE_LDS_MAX: bytes of LDS one pair may take (tests / A/B: 0 puts every op-code table in the global workspace)
};

// Scratch of the decode entry points.  Written by decode.hip -- with one exception: ctc_lab / ctc_val / amax_* are filled by the
// forward's decoder epilogue (forward.hip) and read by cocr_ctc_greedy; ensure_ctc_scratch (decode.hip) is their one grower, and
// whoever moves the weights or the logits under them forgets amax_logits.
struct COCR_INTERNAL DecodeScratch {
    UploadRing lens_ring;                  // per-line lengths of the decode entry points (upload_lens)
    DevBuf<int32_t> ctc_lab;                // per-frame argmax / maximum of the greedy decoder (ensure_ctc_scratch)
    DevBuf<float> ctc_val;
    const float *amax_logits = nullptr;     // the logits buffer whose per-frame argmax / maximum the last forward left in ctc_lab / ctc_val (decoder epilogue)
    int amax_rows = 0;
    bool amax_ok = false;                   // the forward's launch sequence (plain or captured) ends with the argmax epilogue
    DevBuf<unsigned char> beam_bp;          // cocr_ctc_beam: back-pointers, then log Z or the frame records
    DevBuf<unsigned char> lm_scratch;       // cocr_ctc_beam_lm: back-pointers, then the frame records
    UploadRing target_ring;                 // cocr_ctc_loss, cocr_ctc_align: [lens | label lens | label offsets | labels] (upload_targets)
    DevBuf<float> loss_ws;                  // log-softmax + alpha / beta tables
    DevBuf<float> distill_ws;               // cocr_distill_loss: the per-frame KL values
    DevBuf<unsigned> align_ws;              // back-pointer tables of the lines too long for the LDS
    UploadRing page_ring;                   // cocr_ctc_align_page: [page line offsets | rows | first frames | label offsets | labels | region offsets]
    DevBuf<unsigned> page_ws;               // cocr_ctc_align_page: per page the back-pointers, lz, the path's states and the labels' runs
    UploadRing spot_ring;                   // cocr_ctc_spot: [lens | query lens | query offsets | queries]
    DevBuf<unsigned> spot_ws;               // cocr_ctc_spot: per (line, query) the candidate scores and starts of lines too long for the LDS
    UploadRing pattern_ring;                // cocr_ctc_spot_pattern: [lens | state counts | state offsets | edge offsets | classes | flags | predecessor offsets | predecessors]
    DevBuf<unsigned> pattern_ws;            // cocr_ctc_spot_pattern: per (line, pattern) the candidate scores, starts and final states of lines too long for the LDS
};

// Written by lines.hip.
struct COCR_INTERNAL LinesScratch {
    DevBuf<unsigned char> pre_buf;         // line pre-processing: descriptors, tap tables, intermediates
    DevBuf<unsigned char> page_buf;        // line extraction: descriptors, column frames, polygons, span table
};

// Written by score.hip.  cocr_edit_align: the ring of [a offsets | b offsets | launch order] and the op-code workspace of the pairs
// too large for the LDS (the LDS budget of one pair is a switch: score_lds_max)
struct COCR_INTERNAL ScoreScratch {
    UploadRing score_ring;
    DevBuf<unsigned> score_ws;
};

// The output layer's own training state (the frozen-backbone phase).  Written by train.hip; cocr_api.hip releases tr_state where the
// weights it belongs to go (forget_decoder_state, cocr_destroy).
struct COCR_INTERNAL DecoderTrain {
    DevBuf<float> tr_pad;                   // padded models: engine-layout staging of the output layer's gradient tensors
    DevBuf<float> tr_part;                  // decoder backward: per-chunk partial sums of dW | db
    float *tr_state = nullptr;                         // decoder AdamW: fp32 master [W | b], then exp_avg, then exp_avg_sq
    long tr_step = 0;
    int tr_kind = -1;                       // the optimizer kind (COCR_OPT_*) the output layer's steps were taken with; -1: none yet
};

struct cocr_model {
    cocr_hparams hp;
    int device = 0;
    // derived
    int D, C, L, heads, dh, dhp, ff, ksz, ncls, H, snum;      // D / ff / dh / dhp: the ENGINE's dimensions (zero-padded when `padded`)
    int rD = 0, rff = 0, rdh = 0;                      // the model's own encoder_dim, feed-forward width, d_head (tensor shapes, LayerNorm width, 1/sqrt(d_head))
    bool padded = false;                               // bf16, 128 <= encoder_dim < 512 other than 256: the model runs as a zero-padded 256- / 512-wide one (set_engine_dims)
    std::vector<int> feats;   // height after each stride-2 stage: feats[0] = F1, ...
    std::map<std::string, HostTensor> host;
    std::vector<std::string> names;
    // the weights this model reads, its own or another model's (weights.hip.h): never null.  `dtype`, the engine dimensions above and
    // `padded` mirror that set's layout and are written by adopt_layout alone; `seen_gen`: the set's generation at this model's last forward
    WeightsRef w;
    int dtype = -1;
    unsigned long long seen_gen = 0;
    Workspace ws;
    Switches sw;
    DecodeScratch dec;
    LinesScratch lines;
    ScoreScratch score;
    DecoderTrain dtr;
    TrainState *train = nullptr;   // cocr_train_begin .. cocr_train_end (train.hip); opaque outside that unit
    // captured launches (forward.hip; dropped by whoever moves what they point at), debug taps and profile (cocr_api.hip; the forward records into them)
    GraphCache graphs;
    unsigned long long *stamps = nullptr;   // COCR_CHAIN_STAMPS=1 (dev builds): host-visible cycle stamps of the frontend / attention / beam kernels, printed at destroy
    std::map<std::string, std::pair<float *, int64_t>> taps;
    DevBuf<float> tapbuf;        // debug: 5 fp32 (M, D) tap targets of the chain kernels' TAPS instantiation + one bf16 (M, D)
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> ev_pool;
};

static const char *FAMILIES[] = {"frontend_fused", "frontend_conv12", "frontend_dw", "gemm_front_pw", "gemm_front_out", "layernorm",
                                 "gemm_ffn_up", "gemm_ffn_down", "ffn_fused", "chain_ffn_qkv", "chain_front_ffn_qkv", "chain_attn_out_glu", "chain_pw2_ffn_ffn_qkv", "chain_pw2_ffn", "gemm_qkv", "attention", "gemm_attn_out", "gemm_glu",
                                 "dwconv", "gemm_pw2", "gemm_decoder", "ctc_greedy", "ctc_beam", "ctc_loss", "ffn_probe", "event_pair_overhead"};
enum { FAM_FRONT96, FAM_CONV12, FAM_FDW, FAM_FPW, FAM_FOUT, FAM_LN, FAM_FFN_UP, FAM_FFN_DOWN, FAM_FFN_FUSED, FAM_CH_FIRST, FAM_CH_FRONT, FAM_CH_A, FAM_CH_B, FAM_CH_LAST, FAM_QKV, FAM_ATTN, FAM_AOUT, FAM_GLU,
       FAM_DW, FAM_PW2, FAM_DEC, FAM_GREEDY, FAM_BEAM, FAM_LOSS, FAM_FFN_PROBE, FAM_EMPTY, FAM_COUNT };

static int out_len1(int l) { return l >= 1 ? (l - 1) / 2 + 1 : 0; }
static size_t esize(int dtype) { return dtype == COCR_BF16 ? 2 : 4; }

struct ProfScope {
    cocr_model *m; hipStream_t s; ProfRec r; bool on;
    ProfScope(cocr_model *m_, hipStream_t s_, int fam) : m(m_), s(s_), on(m_->sw.profile) {
        if (!on) return;
        r.fam = fam;
        auto get = [&]() { hipEvent_t e; if (m->ev_pool.empty()) { (void)hipEventCreate(&e); } else { e = m->ev_pool.back(); m->ev_pool.pop_back(); } return e; };
        r.a = get(); r.b = get();
        (void)hipEventRecord(r.a, s);
    }
    ~ProfScope() { if (on) { (void)hipEventRecord(r.b, s); m->prof.push_back(r); } }
};

// ------------------------------------------------------------------------------------ functions that cross units
// cocr_api.hip
COCR_INTERNAL int adopt_layout(cocr_model *m);
template <typename T> COCR_INTERNAL int tap(cocr_model *m, hipStream_t s, const std::string &name, const T *src, size_t n);      // T: float, bf16_t
COCR_INTERNAL void blob_to_f32(const cocr_model *m, size_t off, float *dst, size_t n, hipStream_t s);      // owns to_f32_kernel with the taps
// forward.hip
COCR_INTERNAL int attention_core_on(cocr_model *m, int l, int N, int Tn, const void *q, const void *k, const void *v, void *ctx, hipStream_t s);      // block l's attention launch alone
// decode.hip
COCR_INTERNAL int ensure_ctc_scratch(cocr_model *m, size_t rows);
COCR_INTERNAL int distill_loss_on(cocr_model *m, const float *student, const float *teacher, int N, int T, int ncls, const int32_t *out_lens, float tau, float *kd,
                                  float *grad, float ctc_weight, float kd_weight, int accumulate, float *frame_ws, hipStream_t s);
// train.hip
COCR_INTERNAL void train_free(cocr_model *m);
