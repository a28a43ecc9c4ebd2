// libcocr_hip.so -- C ABI (include/cocr.h) and host orchestration of the gfx950 kernels.
//
// A model is: the reference state dict (fp32, host) -> one packed device blob in the compute dtype
// (cocr_finalize) -> a workspace sized for (N, W) -> a fixed sequence of kernel launches on the
// caller's stream (cocr_forward).  Nothing here falls back to the CPU: without a GPU every compute
// entry point fails with COCR_EHIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cocr.h"
#include "attention.hip.h"
#include "common.hip.h"
#include "conv.hip.h"
#include "ctc.hip.h"
#include "ctc_lm.hip.h"
#include "ctc_loss.hip.h"
#include "ctc_align.hip.h"
#include "train.hip.h"
#include "train_enc.hip.h"
#include "gemm.hip.h"
#include "ffn.hip.h"
#include "rowchain_args.hip.h"
#include "pack.hip.h"
#include "frontend.hip.h"
#include "norm.hip.h"
#include "preproc.hip.h"
#include "page.hip.h"
#include "augment.hip.h"
#include "score.hip.h"
#include "weights.hip.h"

// ------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) return fail(COCR_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

extern "C" const char *cocr_last_error(void) { return g_err; }
#ifndef COCR_SRC_HASH
#define COCR_SRC_HASH "unknown"
#endif
extern "C" const char *cocr_version(void) { return "cocr-hip 0.2 (gfx950) src=" COCR_SRC_HASH; }

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
    // workspace
    int capN = 0, capW = 0;
    std::vector<void *> ws_allocs;
    void *z_a = nullptr, *z_b = nullptr;
    float *x = nullptr, *x2 = nullptr;  // the fp32 stream; its second buffer (the chains with the out-proj -> GLU head read one and write the other)
    void *g_lines = nullptr;           // staged graph replay (cocr_forward): library-owned copies of the caller's lines / logits
    float *g_logits = nullptr;
    void *xn = nullptr, *hid = nullptr, *q = nullptr, *k = nullptr, *vt = nullptr, *ctx = nullptr, *glu = nullptr, *dwo = nullptr;
    size_t qkv_bytes = 0;
    int vtN = -1, vtT = -1;    // shape the q/k/vt buffers were last zeroed for
    DevBuf<unsigned char> pre_buf;         // line pre-processing: descriptors, tap tables, intermediates
    DevBuf<unsigned char> page_buf;        // line extraction: descriptors, column frames, polygons, span table
    UploadRing lens_ring;                  // per-line lengths of the decode entry points (upload_lens)
    DevBuf<int32_t> ctc_lab;                // per-frame argmax / maximum of the greedy decoder (ensure_ctc_scratch)
    DevBuf<float> ctc_val;
    const float *amax_logits = nullptr;     // the logits buffer whose per-frame argmax / maximum the last forward left in ctc_lab / ctc_val (decoder epilogue)
    int amax_rows = 0;
    bool amax_ok = false;                   // the forward's launch sequence (plain or captured) ends with the argmax epilogue
    DevBuf<float> tr_pad;                   // padded models: engine-layout staging of the output layer's gradient tensors
    DevBuf<unsigned char> beam_bp;          // cocr_ctc_beam: back-pointers, then log Z or the frame records
    DevBuf<unsigned char> lm_scratch;       // cocr_ctc_beam_lm: back-pointers, then the frame records
    UploadRing target_ring;                 // cocr_ctc_loss, cocr_ctc_align: [lens | label lens | label offsets | labels] (upload_targets)
    DevBuf<float> loss_ws;                  // log-softmax + alpha / beta tables
    DevBuf<unsigned> align_ws;              // back-pointer tables of the lines too long for the LDS
    // cocr_edit_align: the ring of [a offsets | b offsets | launch order], the op-code workspace of the pairs too large for the LDS,
    // and the LDS budget of one pair
    UploadRing score_ring;
    DevBuf<unsigned> score_ws;
    int score_lds_max = 64 * 1024;   // COCR_SCORE_LDS_MAX: bytes of LDS one pair may take (tests / A/B: 0 puts every op-code table in the global workspace)
    int lastN = 0, lastT = 0;                          // shape of the last forward: its encoder output is still in `xn`
    DevBuf<float> tr_part;                  // decoder backward: per-chunk partial sums of dW | db
    float *tr_state = nullptr;                         // decoder AdamW: fp32 master [W | b], then exp_avg, then exp_avg_sq
    long tr_step = 0;
    int tr_kind = -1;                       // the optimizer kind (COCR_OPT_*) the output layer's steps were taken with; -1: none yet
    // debug / profile
    bool use_graph = false;      // cocr_set_graph: hipGraph replay of the forward's launch sequence
    GraphCache graphs;
    bool debug = false;
    unsigned long long *stamps = nullptr;   // COCR_CHAIN_STAMPS=1 (dev builds): host-visible cycle stamps of the frontend / attention / beam kernels, printed at destroy
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
    std::map<std::string, std::pair<float *, int64_t>> taps;
    DevBuf<float> tapbuf;        // debug: 5 fp32 (M, D) tap targets of the chain kernels' TAPS instantiation + one bf16 (M, D)
    TrainState *train = nullptr;   // cocr_train_begin .. cocr_train_end (train_api.hip.h)
    bool profile = false;
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> ev_pool;
};

static const char *FAMILIES[] = {"frontend_fused", "frontend_conv12", "frontend_dw", "gemm_front_pw", "gemm_front_out", "layernorm",
                                 "gemm_ffn_up", "gemm_ffn_down", "ffn_fused", "chain_ffn_qkv", "chain_front_ffn_qkv", "chain_attn_out_glu", "chain_pw2_ffn_ffn_qkv", "chain_pw2_ffn", "gemm_qkv", "attention", "gemm_attn_out", "gemm_glu",
                                 "dwconv", "gemm_pw2", "gemm_decoder", "ctc_greedy", "ctc_beam", "ctc_loss", "ffn_probe", "event_pair_overhead"};
enum { FAM_FRONT96, FAM_CONV12, FAM_FDW, FAM_FPW, FAM_FOUT, FAM_LN, FAM_FFN_UP, FAM_FFN_DOWN, FAM_FFN_FUSED, FAM_CH_FIRST, FAM_CH_FRONT, FAM_CH_A, FAM_CH_B, FAM_CH_LAST, FAM_QKV, FAM_ATTN, FAM_AOUT, FAM_GLU,
       FAM_DW, FAM_PW2, FAM_DEC, FAM_GREEDY, FAM_BEAM, FAM_LOSS, FAM_FFN_PROBE, FAM_EMPTY, FAM_COUNT };

static int out_len1(int l) { return l >= 1 ? (l - 1) / 2 + 1 : 0; }

extern "C" int32_t cocr_out_len(int32_t in_len, int32_t subsampling_factor) {
    int n = 0;
    for (int f = subsampling_factor; f > 1; f >>= 1) ++n;
    for (int i = 0; i < n; ++i) in_len = out_len1(in_len);
    return in_len;
}

static void add_name(cocr_model *m, const std::string &n) { m->names.push_back(n); m->host[n]; }

// The COCR_* environment switches, read when a model is created.  A flag switch flips its default: '1' turns a
// default-off flag on, '0' turns a default-on one off.  A count takes the value's integer.
struct Switch { const char *name; bool cocr_model::*flag; int cocr_model::*count; };
static const Switch SWITCHES[] = {
    {"COCR_NO_PAD", &cocr_model::no_pad, nullptr},
    {"COCR_NO_CHAIN", &cocr_model::no_chain, nullptr},
    {"COCR_NO_FRONT_CHAIN", &cocr_model::no_front_chain, nullptr},
    {"COCR_FFN_PROBE", &cocr_model::ffn_probe, nullptr},
    {"COCR_ATT_TILED", &cocr_model::att_tiled, nullptr},
    {"COCR_ATT_RESIDENT_LONG", &cocr_model::att_resident_long, nullptr},
    {"COCR_CHAIN_XCD", &cocr_model::chain_xcd, nullptr},
    {"COCR_NO_KSKIP", &cocr_model::no_kskip, nullptr},
    {"COCR_NO_DW_FUSE", &cocr_model::no_dw_fuse, nullptr},
    {"COCR_NO_A_FUSE", &cocr_model::no_a_fuse, nullptr},
    {"COCR_NO_FRONT96", &cocr_model::no_front96, nullptr},
    {"COCR_NO_FRONT32", &cocr_model::no_front32, nullptr},
    {"COCR_BEAM_REF", &cocr_model::beam_ref, nullptr},
    {"COCR_ATT_RESIDENT_MIN", nullptr, &cocr_model::att_resident_min},
    {"COCR_CHAIN_ROWS", nullptr, &cocr_model::chain_rows},
    {"COCR_SCORE_LDS_MAX", nullptr, &cocr_model::score_lds_max},
};

extern "C" int cocr_create(const cocr_hparams *hp, int device, cocr_model **out) {
    if (!hp || !out) return fail(COCR_EINVAL, "null argument");
    if (hp->num_classes < 1 || hp->height < 1 || hp->encoder_dim < 1 || hp->num_encoder_layers < 1 || hp->num_attention_heads < 1)
        return fail(COCR_EINVAL, "non-positive hyper-parameter");
    if (hp->encoder_dim % hp->num_attention_heads) return fail(COCR_EINVAL, "d_model %% num_heads should be zero.");
    if ((hp->conv_kernel_size - 1) % 2 || hp->conv_kernel_size < 1) return fail(COCR_EINVAL, "kernel_size should be a odd number for 'SAME' padding");
    if (hp->conv_expansion_factor != 2) return fail(COCR_EINVAL, "Currently, Only Supports expansion_factor 2");
    int sf = hp->subsampling_factor, snum = 0;
    if (sf < 2 || (sf & (sf - 1))) return fail(COCR_EINVAL, "Sampling factor should be a power of 2.");
    for (int f = sf; f > 1; f >>= 1) ++snum;
    if (snum < 1) return fail(COCR_EINVAL, "subsampling_factor must be at least 2");
    if (hp->encoder_dim % 16) return fail(COCR_EUNSUPPORTED, "encoder_dim must be a multiple of 16 (GLU tile pairing, 16-byte rows)");
    if (hp->subsampling_conv_channels % 8) return fail(COCR_EUNSUPPORTED, "subsampling_conv_channels must be a multiple of 8");
    if (hp->encoder_dim > COCR_LN_MAX_D) return fail(COCR_EUNSUPPORTED, "encoder_dim > 1024");
    const int dh = hp->encoder_dim / hp->num_attention_heads;
    if (dh > 128) return fail(COCR_EUNSUPPORTED, "d_head > 128");
    cocr_model *m = new cocr_model();
    m->hp = *hp;
    m->device = device;
    m->D = hp->encoder_dim; m->C = hp->subsampling_conv_channels; m->L = hp->num_encoder_layers;
    m->heads = hp->num_attention_heads; m->dh = dh; m->dhp = round_up(dh, 32);
    m->ff = hp->feed_forward_expansion_factor * hp->encoder_dim; m->ksz = hp->conv_kernel_size;
    m->rD = m->D; m->rff = m->ff; m->rdh = m->dh;
    m->ncls = hp->num_classes; m->H = hp->height; m->snum = snum;
    weights_own(m->w, m, device);                       // (an empty set: not finalized)
    for (const Switch &w : SWITCHES) {
        const char *e = getenv(w.name);
        if (!e) continue;
        if (w.count) m->*w.count = atoi(e);
        else m->*w.flag = m->*w.flag ? e[0] != '0' : e[0] == '1';
    }
    { const char *e = getenv("COCR_CHAIN_STAMPS"); if (e && e[0] == '1') { (void)hipHostMalloc((void **)&m->stamps, 4096 * 8); memset(m->stamps, 0, 4096 * 8); } }
    int f = hp->height;
    for (int i = 0; i < snum; ++i) { f = out_len1(f); m->feats.push_back(f); }
    // expected state-dict entries, reference key names
    char buf[256];
    add_name(m, "encoder.conv_subsample.conv.0.weight");
    add_name(m, "encoder.conv_subsample.conv.0.bias");
    for (int s = 0, idx = 2; s < snum - 1; ++s, idx += 3) {
        for (int j = 0; j < 2; ++j) {
            snprintf(buf, sizeof buf, "encoder.conv_subsample.conv.%d.weight", idx + j); add_name(m, buf);
            snprintf(buf, sizeof buf, "encoder.conv_subsample.conv.%d.bias", idx + j); add_name(m, buf);
        }
    }
    add_name(m, "encoder.conv_subsample.out.0.weight");
    add_name(m, "encoder.conv_subsample.out.0.bias");
    for (int l = 0; l < m->L; ++l) {
        auto nm = [&](const char *suffix) { snprintf(buf, sizeof buf, "encoder.layers.%d.sequential.%s", l, suffix); add_name(m, buf); };
        for (int w = 0; w < 2; ++w) {
            const char *pre = w == 0 ? "0" : "3";
            for (const char *s : {"module.sequential.0.weight", "module.sequential.0.bias", "module.sequential.1.linear.weight",
                                  "module.sequential.1.linear.bias", "module.sequential.4.linear.weight", "module.sequential.4.linear.bias"}) {
                char b2[200]; snprintf(b2, sizeof b2, "%s.%s", pre, s); nm(b2);
            }
        }
        for (const char *s : {"1.module.layer_norm.weight", "1.module.layer_norm.bias", "1.module.attention.u_bias", "1.module.attention.v_bias",
                              "1.module.attention.query_proj.linear.weight", "1.module.attention.query_proj.linear.bias",
                              "1.module.attention.key_proj.linear.weight", "1.module.attention.key_proj.linear.bias",
                              "1.module.attention.value_proj.linear.weight", "1.module.attention.value_proj.linear.bias",
                              "1.module.attention.pos_proj.linear.weight", "1.module.attention.out_proj.linear.weight",
                              "1.module.attention.out_proj.linear.bias",
                              "2.module.sequential.0.weight", "2.module.sequential.0.bias", "2.module.sequential.2.conv.weight",
                              "2.module.sequential.2.conv.bias", "2.module.sequential.4.conv.weight", "2.module.sequential.5.weight",
                              "2.module.sequential.5.bias", "2.module.sequential.5.running_mean", "2.module.sequential.5.running_var",
                              "2.module.sequential.7.conv.weight", "2.module.sequential.7.conv.bias", "4.weight", "4.bias"})
            nm(s);
    }
    add_name(m, "decoder.weight");
    add_name(m, "decoder.bias");
    *out = m;
    return COCR_OK;
}

static void free_workspace(cocr_model *m) {
    for (void *p : m->ws_allocs) (void)hipFree(p);
    m->ws_allocs.clear();
    m->capN = m->capW = 0;
    m->vtN = m->vtT = -1;
    m->lastN = m->lastT = 0;                            // (the last forward's encoder output went with it)
}
static void clear_taps(cocr_model *m) {
    for (auto &kv : m->taps) (void)hipFree(kv.second.first);
    m->taps.clear();
    m->tapbuf.release();
}

// COCR_CHAIN_STAMPS=1 (dev builds): what the stamped kernels left
static void print_stamps(const cocr_model *m) {
    if (m->stamps[1024]) {                          // row-chain kernel (dominant form), workgroup 7: per wave, cycles between stamps
        for (int w = 0; w < 8; ++w) {
            const unsigned long long *q = m->stamps + 1024 + 64 * w;
            fprintf(stderr, "chain wave %d (start +%llu):", w, q[0] - m->stamps[1024]);
            for (int i = 1; i < 64 && q[i]; ++i) fprintf(stderr, " %llu", q[i] - q[i - 1]);
            fprintf(stderr, "  total %llu\n", [&] { int i = 1; while (i < 64 && q[i]) ++i; return q[i - 1] - q[0]; }());
        }
    }
    fprintf(stderr, "frontend stamps:");
    for (int i = 129; i < 192 && m->stamps[i]; ++i) fprintf(stderr, " %llu", m->stamps[i] - m->stamps[128]);
    fprintf(stderr, "\nbeam walk cycles of the stay wave, then of extension wave 0 (pairs + reads, keys, barrier + ranks, update, tail):");
    for (int i = 240; i < 250 && m->stamps[i]; ++i) fprintf(stderr, " %llu", m->stamps[i]);
    fprintf(stderr, "\nattention stamps:");
    for (int i = 193; i < 240 && m->stamps[i]; ++i) fprintf(stderr, " %llu", m->stamps[i] - m->stamps[192]);
    fprintf(stderr, "\n");
    {   // per-workgroup (start, end, hardware id) of the stamped attention launch: residency and tail
        const unsigned long long *w = m->stamps + 192 + 64;
        unsigned long long t0 = ~0ull, t1 = 0;
        int nwg = 0;
        for (int i = 0; i < 1200 && w[3 * i]; ++i) { t0 = std::min(t0, w[3 * i]); t1 = std::max(t1, w[3 * i + 1]); nwg = i + 1; }
        if (nwg) {
            fprintf(stderr, "attention workgroups %d, span %.2f us (100 MHz ticks)\n", nwg, (t1 - t0) * 0.01);
            std::map<unsigned long long, int> per_cu;
            int hist_start[32] = {0};
            double dur = 0;
            for (int i = 0; i < nwg; ++i) {
                const unsigned long long hw = w[3 * i + 2];
                const unsigned long long cu = ((hw >> 32) << 16) | ((hw >> 8) & 0xff) | (((hw >> 13) & 7) << 8);
                per_cu[cu]++;
                hist_start[std::min<unsigned long long>((w[3 * i] - t0) / 100, 31)]++;
                dur += (w[3 * i + 1] - w[3 * i]) * 0.01;
            }
            fprintf(stderr, "  mean workgroup duration %.2f us; distinct CUs %zu; start-time histogram (1 us bins):", dur / nwg, per_cu.size());
            for (int b = 0; b < 32; ++b) fprintf(stderr, " %d", hist_start[b]);
            int cnt[8] = {0};
            for (auto &kv : per_cu) cnt[std::min(kv.second, 7)]++;
            fprintf(stderr, "\n  CUs by number of workgroups received (0..7+):");
            for (int b = 0; b < 8; ++b) fprintf(stderr, " %d", cnt[b]);
            fprintf(stderr, "\n");
        }
    }
}

static void train_free(cocr_model *m);
extern "C" void cocr_destroy(cocr_model *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    train_free(m);
    free_workspace(m);
    clear_taps(m);
    weights_leave(m->w, m);                             // (an owner: the models that still read its weights are left unfinalized)
    if (m->stamps) {
        (void)hipDeviceSynchronize();
        print_stamps(m);
        (void)hipHostFree(m->stamps);
    }
    if (m->tr_state) (void)hipFree(m->tr_state);
    for (auto &r : m->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : m->ev_pool) (void)hipEventDestroy(e);
    delete m;                                           // (its scratch buffers and captured launches release themselves)
}

extern "C" int cocr_set_tensor(cocr_model *m, const char *name, const void *host, int dtype, int ndim, const int64_t *shape) {
    if (!m || !name || !host) return fail(COCR_EINVAL, "null argument");
    std::string n(name);
    if (n.size() > 20 && n.compare(n.size() - 19, 19, "num_batches_tracked") == 0) return COCR_OK;   // BatchNorm counter: unused in eval
    auto it = m->host.find(n);
    if (it == m->host.end()) return fail(COCR_EINVAL, "unexpected key '%s'", name);
    if (dtype != COCR_F32) return fail(COCR_EINVAL, "tensor '%s': only float32 state is accepted", name);
    int64_t cnt = 1;
    for (int i = 0; i < ndim; ++i) cnt *= shape[i];
    it->second.shape.assign(shape, shape + ndim);
    it->second.data.assign((const float *)host, (const float *)host + cnt);
    it->second.set = true;
    return COCR_OK;
}

extern "C" int cocr_missing_tensors(cocr_model *m, char *buf, size_t buflen) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    int cnt = 0;
    std::string s;
    for (auto &n : m->names)
        if (!m->host[n].set) { ++cnt; s += n; s += '\n'; }
    if (buf && buflen) { strncpy(buf, s.c_str(), buflen - 1); buf[buflen - 1] = 0; }
    return cnt;
}

// ------------------------------------------------------------------------------------ blob
static size_t esize(int dtype) { return dtype == COCR_BF16 ? 2 : 4; }

// The row-chain kernels exist for encoder_dim 256 and 512.  A narrower model (the reference's default: encoder_dim 144, 4 heads of 36,
// feed-forward 576) ran one kernel per product and was SLOWER than the 256-wide model.  In bf16 mode such a model (and one between 256
// and 512 wide) is run as a zero-padded 256-wide (512-wide) one: every tensor is embedded in the 256 / 768-wide layout at pack time (model dimension: identity + zeros; head dimension:
// head h at columns [64 h, 64 h + d_head); feed-forward: identity + zeros), so every padded activation column is exactly zero at every
// stage (zero weights and biases, zero LayerNorm gain and shift, silu(0) = 0, 0 * sigmoid(0) = 0) and the real columns see the same
// sums.  What does not follow from the padding is stated separately: LayerNorm divides by the REAL width (the statistics are raw
// moments: zeros add nothing), the attention scale is 1 / sqrt(real d_head), the sinusoids use the real encoder_dim.
struct EngineDims { int D, ff, dh, dhp; bool padded; };
static EngineDims engine_dims(const cocr_model *m, int dtype) {
    const int wide = m->rD < 256 ? 256 : 512;            // 128 <= encoder_dim < 256 -> 256; 256 < encoder_dim < 512 -> 512
    const int slot = m->heads > 0 && wide % m->heads == 0 ? wide / m->heads : 0;
    const bool pad = dtype == COCR_BF16 && !m->no_pad && m->rD >= 128 && m->rD < 512 && m->rD != 256 && slot >= m->rdh && slot % 32 == 0 && slot <= 128 &&
                     round_up(m->rff, 256) <= (wide == 256 ? 1024 : 2048);
    return {pad ? wide : m->rD, pad ? round_up(m->rff, 256) : m->rff, pad ? slot : m->rdh, pad ? slot : round_up(m->rdh, 32), pad};
}

static BlobPlan make_plan(const cocr_model *m, int dtype) {
    BlobPlan p;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t es = esize(dtype);
    const EngineDims e = engine_dims(m, dtype);
    const int D = e.D, C = m->C, ff = e.ff;
    p.w0 = take((size_t)C * 9 * 4); p.b0 = take((size_t)C * 4);
    for (int s = 0; s < m->snum - 1; ++s) {
        StageW st;
        st.dw_w = take((size_t)C * 9 * 4); st.dw_b = take((size_t)C * 4);
        st.pw_w = take((size_t)C * C * es); st.pw_b = take((size_t)C * 4);
        p.stages.push_back(st);
    }
    const int F = m->feats.back();
    p.wout = take((size_t)D * F * C * es); p.bout = take((size_t)D * 4);
    for (int l = 0; l < m->L; ++l) {
        LayerW w;
        for (int i = 0; i < 2; ++i) {
            w.ffn[i].ln_g = take(D * 4); w.ffn[i].ln_b = take(D * 4);
            w.ffn[i].w1 = take((size_t)ff * D * es); w.ffn[i].b1 = take((size_t)ff * 4);
            w.ffn[i].w2 = take((size_t)D * ff * es); w.ffn[i].b2 = take(D * 4);
        }
        w.a_ln_g = take(D * 4); w.a_ln_b = take(D * 4);
        w.wqkv = take((size_t)3 * D * D * es); w.bqkv = take((size_t)3 * D * 4);
        w.ub = take(D * 4); w.vb = take(D * 4);
        w.wpos = take((size_t)D * D * 4);
        w.wo = take((size_t)D * D * es); w.bo = take(D * 4);
        w.c_ln_g = take(D * 4); w.c_ln_b = take(D * 4);
        w.wpw1 = take((size_t)2 * D * D * es); w.bpw1 = take((size_t)2 * D * 4);
        w.dww = take((size_t)m->ksz * D * 4); w.dwb = take(D * 4);
        w.wpw2 = take((size_t)D * D * es); w.bpw2 = take(D * 4);
        w.f_ln_g = take(D * 4); w.f_ln_b = take(D * 4);
        p.layers.push_back(w);
    }
    p.wdec = take((size_t)m->ncls * D * es); p.bdec = take((size_t)m->ncls * 4);
    p.total = off;
    return p;
}

static uint16_t f32_to_bf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// writes rows x cols of src (row i taken from src row map(i)) as compute dtype
static void put_matrix(unsigned char *dst, int dtype, const float *src, int rows, int cols, const std::vector<int> *rowmap = nullptr,
                       const std::vector<int> *colmap = nullptr) {
    for (int r = 0; r < rows; ++r) {
        const float *s = src + (size_t)(rowmap ? (*rowmap)[r] : r) * cols;
        for (int c = 0; c < cols; ++c) {
            const float v = s[colmap ? (*colmap)[c] : c];
            if (dtype == COCR_BF16) ((uint16_t *)dst)[(size_t)r * cols + c] = f32_to_bf16(v);
            else ((float *)dst)[(size_t)r * cols + c] = v;
        }
    }
}
static void put_f32(unsigned char *dst, const float *src, size_t n) { memcpy(dst, src, n * 4); }

static int expect_shape(const cocr_model *m, const std::string &name, std::initializer_list<int64_t> shape, const HostTensor **out) {
    auto it = m->host.find(name);
    if (it == m->host.end() || !it->second.set) return fail(COCR_ESTATE, "missing tensor '%s'", name.c_str());
    if (it->second.shape != std::vector<int64_t>(shape)) {
        std::string got;
        for (auto v : it->second.shape) got += std::to_string(v) + ",";
        return fail(COCR_EINVAL, "size mismatch for %s: got (%s)", name.c_str(), got.c_str());
    }
    *out = &it->second;
    return COCR_OK;
}

static void free_workspace(cocr_model *m);
// A model's compute dtype and engine dimensions (engine_dims) mirror the layout of the weights it reads; adopt_layout, through this
// function, is the only writer.
static void set_engine_dims(cocr_model *m, int dtype) {
    const EngineDims e = engine_dims(m, dtype);
    m->D = e.D; m->ff = e.ff; m->dh = e.dh; m->dhp = e.dhp; m->padded = e.padded;
    m->dtype = dtype;
}
static void forget_decoder_state(cocr_model *m) {     // the output layer's optimizer state belongs to the old weights
    if (m->tr_state) { (void)hipFree(m->tr_state); m->tr_state = nullptr; m->tr_step = 0; }
}
// Brings `m` to the layout of the set it reads; every entry point that reads the blob or sizes anything from the plan calls this first.
// Where the layouts differ -- the set was (re)finalized in another compute dtype since `m` last looked -- the model's workspace,
// captured launches, last forward and output-layer optimizer state describe the old layout and go.
static int adopt_layout(cocr_model *m) {
    if (m->dtype == m->w->dtype) return COCR_OK;
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    m->graphs.drop();
    free_workspace(m);
    m->amax_logits = nullptr;
    forget_decoder_state(m);
    set_engine_dims(m, m->w->dtype);
    return COCR_OK;
}

// an empty (zeroed) blob of `dtype` that `m` owns: in the set it owns already, else in a new one (weights of its own again)
static int alloc_blob(cocr_model *m, int dtype) {
    if (dtype != COCR_BF16 && dtype != COCR_F32) return fail(COCR_EINVAL, "compute dtype must be COCR_BF16 or COCR_F32");
    HIP_TRY(hipSetDevice(m->device));
    weights_own(m->w, m, m->device);
    m->graphs.drop();
    m->seen_gen = 0;
    forget_decoder_state(m);
    Weights &w = *m->w;
    w.dtype = dtype;
    w.plan = make_plan(m, dtype);
    HIP_TRY(hipMalloc((void **)&w.blob, w.plan.total));
    HIP_TRY(hipMemset(w.blob, 0, w.plan.total));
    return adopt_layout(m);
}

extern "C" int cocr_finalize_empty(cocr_model *m, int compute_dtype) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    int rc = alloc_blob(m, compute_dtype);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return COCR_OK;
}

extern "C" int cocr_share_weights(cocr_model *m, cocr_model *owner) {
    if (!m || !owner || m == owner) return fail(COCR_EINVAL, "two different models expected");
    if (owner->w->blob && !owner->w->owned_by(owner)) return fail(COCR_EINVAL, "the owner itself shares another model's weights");
    if (!owner->w->blob) return fail(COCR_ESTATE, "the owner is not finalized");
    if (m->device != owner->device || memcmp(&m->hp, &owner->hp, sizeof m->hp) != 0) return fail(COCR_EINVAL, "models of the same hyper-parameters on the same device expected");
    if (m->train || owner->train) return fail(COCR_ESTATE, "not while a training state exists");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    weights_join(m->w, m, owner->w);
    m->graphs.drop();
    m->seen_gen = 0;
    forget_decoder_state(m);
    return adopt_layout(m);
}

extern "C" int cocr_weight_blob(cocr_model *m, void **device_ptr, size_t *bytes) {
    if (!m || !device_ptr || !bytes) return fail(COCR_EINVAL, "null argument");
    if (!m->w->blob) return fail(COCR_ESTATE, "model not finalized");
    if (!m->w->owned_by(m)) return fail(COCR_ESTATE, "this model shares another model's weights: address the owner");
    *device_ptr = m->w->blob;
    *bytes = m->w->plan.total;
    m->w->invalidate();          // the caller may write through the pointer
    return COCR_OK;
}

// Copies between the packed blob and a caller-owned device buffer (a collective library's registered / framework-owned
// memory): rank 0 exports, broadcasts, the other ranks import.  Stream-ordered on `stream`.
extern "C" int cocr_blob_export(cocr_model *m, void *dst_device, size_t bytes, void *stream) {
    if (!m || !dst_device) return fail(COCR_EINVAL, "null argument");
    if (!m->w->blob) return fail(COCR_ESTATE, "model not finalized");
    if (!m->w->owned_by(m)) return fail(COCR_ESTATE, "this model shares another model's weights: address the owner");
    if (bytes != m->w->plan.total) return fail(COCR_EINVAL, "blob is %zu bytes, buffer %zu", m->w->plan.total, bytes);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemcpyAsync(dst_device, m->w->blob, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return COCR_OK;
}
extern "C" int cocr_blob_import(cocr_model *m, const void *src_device, size_t bytes, void *stream) {
    if (!m || !src_device) return fail(COCR_EINVAL, "null argument");
    if (!m->w->blob) return fail(COCR_ESTATE, "model not finalized");
    if (bytes != m->w->plan.total) return fail(COCR_EINVAL, "blob is %zu bytes, buffer %zu", m->w->plan.total, bytes);
    if (!m->w->owned_by(m)) return fail(COCR_ESTATE, "this model shares another model's weights: address the owner");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemcpyAsync(m->w->blob, src_device, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    m->w->invalidate();
    forget_decoder_state(m);
    return COCR_OK;
}

// dst (vrows x vcols, compute dtype) <- src (.. x src_cols): element (r, c) = src[rmap[r]][cmap[c]], zero where a map says -1
static void put_mapped(unsigned char *dst, int dtype, const float *src, int src_cols, const std::vector<int> &rmap, const std::vector<int> &cmap) {
    const size_t vcols = cmap.size();
    for (size_t r = 0; r < rmap.size(); ++r)
        for (size_t c = 0; c < vcols; ++c) {
            const float v = (rmap[r] >= 0 && cmap[c] >= 0) ? src[(size_t)rmap[r] * src_cols + cmap[c]] : 0.0f;
            if (dtype == COCR_BF16) ((uint16_t *)dst)[r * vcols + c] = f32_to_bf16(v);
            else ((float *)dst)[r * vcols + c] = v;
        }
}
static void put_vec(unsigned char *dst, const float *src, const std::vector<int> &map) {
    for (size_t i = 0; i < map.size(); ++i) ((float *)dst)[i] = map[i] >= 0 ? src[map[i]] : 0.0f;
}

extern "C" int cocr_finalize(cocr_model *m, int dtype) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    if (dtype != COCR_BF16 && dtype != COCR_F32) return fail(COCR_EINVAL, "compute dtype must be COCR_BF16 or COCR_F32");
    HIP_TRY(hipSetDevice(m->device));
    int rc;
    // tensor shapes: the model's own (rD, rff, h x rdh); blob layout: the engine's (D, ff, h x dh) -- the same unless the model is padded
    const EngineDims e = engine_dims(m, dtype);
    const int rD = m->rD, rff = m->rff, rdh = m->rdh, D = e.D, C = m->C, ff = e.ff, k = m->ksz, h = m->heads, dh = e.dh;
    std::vector<int> Mm(D), Fm(ff), Am(D), Gm((size_t)2 * D), ident_cls(m->ncls);      // engine index -> model index (-1: zero)
    for (int c = 0; c < D; ++c) Mm[c] = c < rD ? c : -1;                                // model dimension
    for (int c = 0; c < ff; ++c) Fm[c] = c < rff ? c : -1;                              // feed-forward dimension
    for (int c = 0; c < D; ++c) Am[c] = (c / dh < h && c % dh < rdh) ? (c / dh) * rdh + c % dh : -1;      // head-major dimension: head hh at [dh hh, dh hh + rdh)
    for (int n = 0; n < 2 * D; ++n) {   // GLU interleave: packed row 32j + c <- value row 16j + c ; packed row 32j + 16 + c <- gate row D + 16j + c
        const int tn = n >> 4, c = n & 15, j = tn >> 1, v = 16 * j + c;
        Gm[n] = v < rD ? ((tn & 1) ? rD + v : v) : -1;
    }
    for (int c = 0; c < m->ncls; ++c) ident_cls[c] = c;
    const BlobPlan plan = make_plan(m, dtype);
    std::vector<unsigned char> stage(plan.total, 0);
    unsigned char *st = stage.data();
    const HostTensor *t = nullptr;
    char buf[256];
#define GET(NAME, ...)                                          \
    if ((rc = expect_shape(m, NAME, {__VA_ARGS__}, &t))) return rc;
    GET("encoder.conv_subsample.conv.0.weight", C, 1, 3, 3); put_f32(st + plan.w0, t->data.data(), (size_t)C * 9);
    GET("encoder.conv_subsample.conv.0.bias", C); put_f32(st + plan.b0, t->data.data(), C);
    for (int s = 0, idx = 2; s < m->snum - 1; ++s, idx += 3) {
        snprintf(buf, sizeof buf, "encoder.conv_subsample.conv.%d.weight", idx); GET(buf, C, 1, 3, 3); put_f32(st + plan.stages[s].dw_w, t->data.data(), (size_t)C * 9);
        snprintf(buf, sizeof buf, "encoder.conv_subsample.conv.%d.bias", idx); GET(buf, C); put_f32(st + plan.stages[s].dw_b, t->data.data(), C);
        snprintf(buf, sizeof buf, "encoder.conv_subsample.conv.%d.weight", idx + 1); GET(buf, C, C, 1, 1); put_matrix(st + plan.stages[s].pw_w, dtype, t->data.data(), C, C);
        snprintf(buf, sizeof buf, "encoder.conv_subsample.conv.%d.bias", idx + 1); GET(buf, C); put_f32(st + plan.stages[s].pw_b, t->data.data(), C);
    }
    {   // flatten order: the reference's feature index is c*F + f (convolution.py:235-236); ours is f*C + c
        const int F = m->feats.back();
        GET("encoder.conv_subsample.out.0.weight", rD, (int64_t)C * F);
        std::vector<int> colmap((size_t)F * C);
        for (int f = 0; f < F; ++f) for (int c = 0; c < C; ++c) colmap[(size_t)f * C + c] = c * F + f;
        put_mapped(st + plan.wout, dtype, t->data.data(), F * C, Mm, colmap);
        GET("encoder.conv_subsample.out.0.bias", rD); put_vec(st + plan.bout, t->data.data(), Mm);
    }
    for (int l = 0; l < m->L; ++l) {
        const LayerW &w = plan.layers[l];
        auto key = [&](const char *suffix) { snprintf(buf, sizeof buf, "encoder.layers.%d.sequential.%s", l, suffix); return std::string(buf); };
        for (int i = 0; i < 2; ++i) {
            const std::string pre = std::string(i == 0 ? "0" : "3") + ".module.sequential.";
            GET(key((pre + "0.weight").c_str()), rD); put_vec(st + w.ffn[i].ln_g, t->data.data(), Mm);
            GET(key((pre + "0.bias").c_str()), rD); put_vec(st + w.ffn[i].ln_b, t->data.data(), Mm);
            GET(key((pre + "1.linear.weight").c_str()), rff, rD); put_mapped(st + w.ffn[i].w1, dtype, t->data.data(), rD, Fm, Mm);
            GET(key((pre + "1.linear.bias").c_str()), rff); put_vec(st + w.ffn[i].b1, t->data.data(), Fm);
            GET(key((pre + "4.linear.weight").c_str()), rD, rff); put_mapped(st + w.ffn[i].w2, dtype, t->data.data(), rff, Mm, Fm);
            GET(key((pre + "4.linear.bias").c_str()), rD); put_vec(st + w.ffn[i].b2, t->data.data(), Mm);
        }
        GET(key("1.module.layer_norm.weight"), rD); put_vec(st + w.a_ln_g, t->data.data(), Mm);
        GET(key("1.module.layer_norm.bias"), rD); put_vec(st + w.a_ln_b, t->data.data(), Mm);
        const char *proj[3] = {"query", "key", "value"};
        for (int j = 0; j < 3; ++j) {
            snprintf(buf, sizeof buf, "encoder.layers.%d.sequential.1.module.attention.%s_proj.linear.weight", l, proj[j]);
            GET(std::string(buf), rD, rD); put_mapped(st + w.wqkv + (size_t)j * D * D * esize(dtype), dtype, t->data.data(), rD, Am, Mm);
            snprintf(buf, sizeof buf, "encoder.layers.%d.sequential.1.module.attention.%s_proj.linear.bias", l, proj[j]);
            GET(std::string(buf), rD); put_vec(st + w.bqkv + (size_t)j * D * 4, t->data.data(), Am);
        }
        GET(key("1.module.attention.u_bias"), h, rdh); put_vec(st + w.ub, t->data.data(), Am);
        GET(key("1.module.attention.v_bias"), h, rdh); put_vec(st + w.vb, t->data.data(), Am);
        GET(key("1.module.attention.pos_proj.linear.weight"), rD, rD); put_mapped(st + w.wpos, COCR_F32, t->data.data(), rD, Am, Mm);
        GET(key("1.module.attention.out_proj.linear.weight"), rD, rD); put_mapped(st + w.wo, dtype, t->data.data(), rD, Mm, Am);
        GET(key("1.module.attention.out_proj.linear.bias"), rD); put_vec(st + w.bo, t->data.data(), Mm);
        GET(key("2.module.sequential.0.weight"), rD); put_vec(st + w.c_ln_g, t->data.data(), Mm);
        GET(key("2.module.sequential.0.bias"), rD); put_vec(st + w.c_ln_b, t->data.data(), Mm);
        GET(key("2.module.sequential.2.conv.weight"), 2 * rD, rD, 1); put_mapped(st + w.wpw1, dtype, t->data.data(), rD, Gm, Mm);
        GET(key("2.module.sequential.2.conv.bias"), 2 * rD); put_vec(st + w.bpw1, t->data.data(), Gm);
        {   // BatchNorm (eval) folded into the depthwise taps: s = gamma / sqrt(var + eps)
            const HostTensor *wd, *g, *b, *mu, *var;
            if ((rc = expect_shape(m, key("2.module.sequential.4.conv.weight"), {rD, 1, k}, &wd))) return rc;
            if ((rc = expect_shape(m, key("2.module.sequential.5.weight"), {rD}, &g))) return rc;
            if ((rc = expect_shape(m, key("2.module.sequential.5.bias"), {rD}, &b))) return rc;
            if ((rc = expect_shape(m, key("2.module.sequential.5.running_mean"), {rD}, &mu))) return rc;
            if ((rc = expect_shape(m, key("2.module.sequential.5.running_var"), {rD}, &var))) return rc;
            float *tw = (float *)(st + w.dww), *tb = (float *)(st + w.dwb);      // (padded channels: taps and bias stay zero)
            for (int c = 0; c < rD; ++c) {
                const float s = g->data[c] / sqrtf(var->data[c] + 1e-5f);
                for (int tau = 0; tau < k; ++tau) tw[(size_t)tau * D + c] = wd->data[(size_t)c * k + tau] * s;
                tb[c] = b->data[c] - mu->data[c] * s;
            }
        }
        GET(key("2.module.sequential.7.conv.weight"), rD, rD, 1); put_mapped(st + w.wpw2, dtype, t->data.data(), rD, Mm, Mm);
        GET(key("2.module.sequential.7.conv.bias"), rD); put_vec(st + w.bpw2, t->data.data(), Mm);
        GET(key("4.weight"), rD); put_vec(st + w.f_ln_g, t->data.data(), Mm);
        GET(key("4.bias"), rD); put_vec(st + w.f_ln_b, t->data.data(), Mm);
    }
    GET("decoder.weight", m->ncls, rD); put_mapped(st + plan.wdec, dtype, t->data.data(), rD, ident_cls, Mm);
    GET("decoder.bias", m->ncls); put_f32(st + plan.bdec, t->data.data(), m->ncls);
#undef GET
    if ((rc = alloc_blob(m, dtype))) return rc;
    HIP_TRY(hipMemcpy(m->w->blob, st, plan.total, hipMemcpyHostToDevice));
    if ((rc = m->w->ensure_ptab(nullptr))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return COCR_OK;
}

// P_l = PE Wpos_l^T for all 2 max_len - 1 relative positions (max_len 5000 as in the reference, longer once a longer line has come) (embedding.py:35-56 table, attention.py:62,85 projection), computed on the device in
// fp32 from the blob's own wpos matrices and stored head-padded in the compute dtype.  Runs on `s` ahead of a forward's launches (stream
// order covers a blob import issued on the same stream), never inside a graph capture; the same kernel on the same inputs on every rank,
// so a rank that received the blob by broadcast holds bit-identical tables.
template <typename T> int Weights::compute_pos_tables(hipStream_t s) {
    const cocr_model *m = users.front();
    const int D = m->D, rD = m->rD, maxlen = pos_maxlen, R = 2 * maxlen - 1;      // (a padded model: rD sinusoids, zeros behind them)
    std::vector<float> pe((size_t)R * D, 0.0f);
    for (int r = 0; r < R; ++r) {
        const float pos = (float)(maxlen - 1 - r);           // +(max_len - 1) ... -(max_len - 1)
        for (int i = 0; i < rD; i += 2) {
            const float div = expf((float)i * (float)(-(log(10000.0) / rD)));
            const float ang = pos * div;
            pe[(size_t)r * D + i] = sinf(ang);
            if (i + 1 < rD) pe[(size_t)r * D + i + 1] = cosf(ang);
        }
    }
    float *d_pe = nullptr;
    HIP_TRY(hipMalloc((void **)&d_pe, pe.size() * 4));
    HIP_TRY(hipMemcpyAsync(d_pe, pe.data(), pe.size() * 4, hipMemcpyHostToDevice, s));
    for (int l = 0; l < m->L; ++l) {
        EpiPosTable<T> epi{(T *)(ptab + (size_t)l * ptab_stride), m->dh, m->dhp, m->heads};
        HIP_TRY(launch_gemm<float>(s, d_pe, D, (const float *)(blob + plan.layers[l].wpos), D, R, D, D, epi));
    }
    HIP_TRY(hipStreamSynchronize(s));            // (pe is host memory of this call; one-time start-up work)
    HIP_TRY(hipFree(d_pe));
    return COCR_OK;
}
int Weights::ensure_ptab(hipStream_t s) {
    if (!ptab_stale) return COCR_OK;
    const cocr_model *m = users.front();
    ptab_stride = (size_t)(2 * pos_maxlen - 1) * m->heads * m->dhp * esize(dtype);
    if (!ptab) {
        HIP_TRY(hipMalloc((void **)&ptab, ptab_stride * m->L));
        HIP_TRY(hipMemsetAsync(ptab, 0, ptab_stride * m->L, s));          // padded head dims read as zero
    }
    int rc = dtype == COCR_BF16 ? compute_pos_tables<bf16_t>(s) : compute_pos_tables<float>(s);
    if (rc) return rc;
    ptab_stale = false;
    return COCR_OK;
}
// The attention core reads the band of whole 64-key tiles unclamped: the tables must cover |relative position| < Tp64 = round_up(T, 64).
// A longer line than the tables hold: rebuilt longer by the next ensure_ptab (the reference's RelPositionalEncoding.extend_pe,
// embedding.py:35-41; a position's encoding does not depend on the table length, so shorter lines keep their results)
int Weights::cover_positions(int Tp64) {
    if (Tp64 + 64 <= pos_maxlen) return COCR_OK;
    HIP_TRY(hipDeviceSynchronize());
    if (ptab) { (void)hipFree(ptab); ptab = nullptr; }
    pos_maxlen = round_up(Tp64 + 64, 1024);
    ptab_stale = true;
    ++gen;                                       // captured launches point at the old tables
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ workspace
static int ws_alloc(cocr_model *m, void **p, size_t bytes) {
    HIP_TRY(hipMalloc(p, bytes ? bytes : 256));
    m->ws_allocs.push_back(*p);
    return COCR_OK;
}

extern "C" int cocr_reserve(cocr_model *m, int N, int W) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    if (!m->w->blob) return fail(COCR_ESTATE, "model not finalized");
    if (N < 1 || W < 1) return fail(COCR_EINVAL, "empty batch");
    { const int rc = adopt_layout(m); if (rc) return rc; }
    if (N <= m->capN && W <= m->capW) return COCR_OK;
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    N = std::max(N, m->capN); W = std::max(W, m->capW);
    m->graphs.drop();     // captured launches point into the old workspace
    free_workspace(m);
    const size_t es = esize(m->dtype);
    int T = W;
    for (int i = 0; i < m->snum; ++i) T = out_len1(T);
    const int Tz = m->snum >= 2 ? out_len1(out_len1(W)) : out_len1(W);      // frames after the fused first two stages (factor 2: after conv.0)
    const size_t M = (size_t)N * T, Tp = round_up(T, 64);      // q / k / v rows per (line, head): whole 64-key tiles (attention.hip.h reads them unclamped)
    int rc;
    const size_t zbytes = (size_t)N * Tz * m->feats[m->snum >= 2 ? 1 : 0] * m->C * es;
    if ((rc = ws_alloc(m, &m->z_a, zbytes))) return rc;
    if ((rc = ws_alloc(m, &m->z_b, zbytes))) return rc;
    if ((rc = ws_alloc(m, (void **)&m->x, (M + 128) * m->D * 4))) return rc;      // (+ 128 rows: the row-chain kernels keep the stream in whole row blocks of up to 96 rows)
    if ((rc = ws_alloc(m, (void **)&m->x2, (M + 128) * m->D * 4))) return rc;
    if ((rc = ws_alloc(m, &m->xn, M * m->D * es))) return rc;
    if ((rc = ws_alloc(m, &m->hid, M * m->ff * es))) return rc;
    m->qkv_bytes = (size_t)N * m->heads * Tp * m->dhp * es;
    if ((rc = ws_alloc(m, &m->q, m->qkv_bytes))) return rc;
    if ((rc = ws_alloc(m, &m->k, m->qkv_bytes))) return rc;
    if ((rc = ws_alloc(m, &m->vt, m->qkv_bytes))) return rc;
    if ((rc = ws_alloc(m, &m->ctx, M * m->D * es))) return rc;
    if ((rc = ws_alloc(m, &m->glu, M * m->D * es))) return rc;
    if ((rc = ws_alloc(m, &m->dwo, M * m->D * es))) return rc;
    if ((rc = ws_alloc(m, &m->g_lines, (size_t)N * m->H * W * 4))) return rc;
    if ((rc = ws_alloc(m, (void **)&m->g_logits, M * m->ncls * 4))) return rc;
    m->capN = N; m->capW = W;
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ debug / profile
template <typename T> __global__ void to_f32_kernel(const T *in, float *out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = to_f32(in[i]);
}
// rows of the engine's (padded) width D -> rows of the model's own width rD: column c of the output is engine column c (model
// dimension) or, head-major, engine column (c / rdh) * dh + c % rdh
template <typename T> __global__ void tap_narrow_kernel(const T *in, float *out, size_t rows, int D, int rD, int dh, int rdh, int head_major) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * rD; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / rD;
        const int c = (int)(i - r * rD);
        out[i] = to_f32(in[r * D + (head_major ? (c / rdh) * dh + c % rdh : c)]);
    }
}
template <typename T> static int tap(cocr_model *m, hipStream_t s, const std::string &name, const T *src, size_t n) {
    if (!m->debug) return COCR_OK;
    // a padded model (set_engine_dims): the taps show the model's own columns.  Which taps are rows of D, and in which column order,
    // follows from their names: q / k / v and the frontend's channel-last tensors have layouts of their own
    auto ends = [&](const char *suf) { const size_t l = strlen(suf); return name.size() >= l && name.compare(name.size() - l, l, suf) == 0; };
    const bool own_layout = ends(".q") || ends(".k") || ends(".v") || ends(".z2") || ends(".z3");
    const bool narrow = m->padded && !own_layout && n % (size_t)m->D == 0;
    const size_t nout = narrow ? n / m->D * m->rD : n;
    float *dst = nullptr;
    HIP_TRY(hipMalloc((void **)&dst, nout * 4));
    if (narrow) hipLaunchKernelGGL((tap_narrow_kernel<T>), dim3(256), dim3(256), 0, s, src, dst, n / m->D, m->D, m->rD, m->dh, m->rdh, ends(".ctx") ? 1 : 0);
    else hipLaunchKernelGGL((to_f32_kernel<T>), dim3(256), dim3(256), 0, s, src, dst, n);
    HIP_TRY(hipStreamSynchronize(s));
    auto it = m->taps.find(name);
    if (it != m->taps.end()) (void)hipFree(it->second.first);
    m->taps[name] = {dst, (int64_t)nout};
    return COCR_OK;
}

extern "C" int cocr_set_debug(cocr_model *m, int on) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    m->debug = on != 0;
    if (!on) clear_taps(m);
    return COCR_OK;
}
extern "C" int cocr_debug_tap(cocr_model *m, const char *name, float *host_out, int64_t max_elems, int64_t *n_elems) {
    if (!m || !name) return fail(COCR_EINVAL, "null argument");
    auto it = m->taps.find(name);
    if (it == m->taps.end()) return fail(COCR_EINVAL, "no tap '%s' (debug off, or stage not run)", name);
    if (n_elems) *n_elems = it->second.second;
    if (host_out) {
        if (max_elems < it->second.second) return fail(COCR_EINVAL, "tap '%s' has %lld elements", name, (long long)it->second.second);
        HIP_TRY(hipMemcpy(host_out, it->second.first, it->second.second * 4, hipMemcpyDeviceToHost));
    }
    return COCR_OK;
}

struct ProfScope {
    cocr_model *m; hipStream_t s; ProfRec r; bool on;
    ProfScope(cocr_model *m_, hipStream_t s_, int fam) : m(m_), s(s_), on(m_->profile) {
        if (!on) return;
        r.fam = fam;
        auto get = [&]() { hipEvent_t e; if (m->ev_pool.empty()) { (void)hipEventCreate(&e); } else { e = m->ev_pool.back(); m->ev_pool.pop_back(); } return e; };
        r.a = get(); r.b = get();
        (void)hipEventRecord(r.a, s);
    }
    ~ProfScope() { if (on) { (void)hipEventRecord(r.b, s); m->prof.push_back(r); } }
};

extern "C" int cocr_profile(cocr_model *m, int on) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    m->profile = on != 0;
    for (auto &r : m->prof) { m->ev_pool.push_back(r.a); m->ev_pool.push_back(r.b); }
    m->prof.clear();
    return COCR_OK;
}
extern "C" int cocr_profile_read(cocr_model *m, char *names, size_t names_len, double *ms, int64_t *launches, int max_entries) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    double sum[FAM_COUNT] = {0};
    int64_t cnt[FAM_COUNT] = {0};
    for (auto &r : m->prof) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, r.a, r.b));
        sum[r.fam] += t; cnt[r.fam]++;
    }
    std::string s;
    int n = 0;
    for (int f = 0; f < FAM_COUNT && n < max_entries; ++f) {
        if (!cnt[f]) continue;
        s += FAMILIES[f]; s += '\n';
        ms[n] = sum[f] / (double)cnt[f]; launches[n] = cnt[f];
        ++n;
    }
    if (names && names_len) { strncpy(names, s.c_str(), names_len - 1); names[names_len - 1] = 0; }
    return n;
}

// ------------------------------------------------------------------------------------ forward
#define LAUNCH_CHECK() HIP_TRY(hipGetLastError())

#define GEMM_TRY(call)                                                                                 \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return fail(COCR_EHIP, "kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

template <typename T, int DHP>
static hipError_t launch_attention(hipStream_t s, int N, const T *q, const T *k, const T *v, const T *ptab, const float *ub,
                                   const float *vb, T *ctx, int Tn, int Tp, int heads, int dh, float scale, int pos_center, unsigned long long *stamps = nullptr,
                                   bool tiled_only = false, int resident_min = 192, bool resident_long = false) {
    if constexpr (sizeof(T) == 2 && DHP == 64) {
        // lines of at most 320 frames (the metric's: 300): K, V and the band of a (line, head) resident in LDS, no barriers in the key loop
        // ... when there are enough (line, head) pairs to give most CUs one of its workgroups: a small batch is served faster by the tiled
        // kernel's five workgroups per (line, head) on CUs of their own (B = 1: 0.83 ms per forward with this kernel against 0.76 ms)
        const int ntiles = ceil_div(Tn, 16), nqb = ceil_div(ntiles, AF_QT);
        // Longer lines (`resident_long`, COCR_ATT_RESIDENT_LONG=1: measured, not the default) walk their keys in passes of at most AF_TK: at the wide
        // model's 600-frame lines the tiled kernel is the faster one (83 us against 91 us per launch of 32 lines x 8 heads: its staging is
        // amortised over ten key tiles there and three of its workgroups share a CU; 4.6 k against 4.2 k query-key pairs per us and CU).
        if (dh == DHP && (Tn <= AF_TK || resident_long) && !tiled_only && !stamps && nqb * N * heads >= resident_min) {
            // (lines of more than AF_TK frames: their keys in passes of at most AF_TK, balanced -- 600 frames = 2 x 320, 700 = 3 x 256)
            const int Tk0 = round_up(Tn, 64), npass = ceil_div(Tk0, AF_TK), Tk = round_up(ceil_div(Tk0, npass), 64);
            const int ntw = ceil_div(ntiles, nqb);
            const size_t lds = (size_t)(2 * Tk + 16 * ntw + Tk) * 128 + AF_WAVES * AF_SROWS * AF_SK * sizeof(float);
            auto kern = npass > 1 ? relpos_attention_full_kernel<true> : relpos_attention_full_kernel<false>;
            hipError_t e = raise_lds_limit((const void *)kern, lds);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(kern, dim3(nqb, N * heads), dim3(64 * AF_WAVES), lds, s, (const bf16_t *)q, (const bf16_t *)k, (const bf16_t *)v,
                               (const bf16_t *)ptab, ub, vb, (bf16_t *)ctx, Tn, Tp, heads, scale * 1.44269504088896340736f, pos_center, ntw, Tk);
            return hipGetLastError();
        }
    }
    const size_t lds = attention_lds_bytes<T, DHP>();
    auto kern = relpos_attention_kernel<T, DHP>;
    hipError_t e = raise_lds_limit((const void *)kern, lds);
    if (e != hipSuccess) return e;
    // log2(e) rides on the 1/sqrt(d_head) factor folded into the query operands: the kernel's scores are in log2 units and its
    // softmax uses v_exp_f32 (2^x) directly -- one multiply per score less.
    // (80-query tiles -- 5 waves, 512 workgroups = one round of 2 per CU at cfg2 instead of 1280 in two rounds -- measured SLOWER:
    // 19.4 us against 16.3 us per launch)
    hipLaunchKernelGGL(kern, dim3(ceil_div(Tn, 64), N * heads), dim3(256), lds, s, q, k, v, ptab, ub, vb, ctx, Tn, Tp, heads, dh,
                       scale * 1.44269504088896340736f, pos_center, stamps);
    return hipGetLastError();
}

static int ensure_ctc_scratch(cocr_model *m, size_t rows);

// ------------------------------------------------------------------------------------ forward: its form
// How each stage of a forward runs, decided in one place (forward_form) from the model, the compute type, the batch shape, the
// debug-tap state and the switches.  forward_impl launches that form; ensure_packed packs the weights it reads.
enum FrontForm {
    FRONT_96,      // bf16, two stages, frontend96_supported: conv.0 + ReLU + depthwise conv.2 + pointwise conv.3 + ReLU in one kernel (frontend.hip.h)
    FRONT_CONV0,   // subsampling factor 2: conv.0 + ReLU, then the output linear
    FRONT_PW32,    // bf16, 32 conv channels, no taps: conv.0 .. conv.3 in one launch (conv.hip.h: frontend_conv12pw32_kernel; Z2 stays on chip)
    FRONT_MFMA,    // bf16, conv channels a multiple of 64: conv.0 on the matrix cores + depthwise conv.2 (conv.hip.h), pointwise conv.3 as a GEMM
    FRONT_VALU,    // conv.0 + depthwise conv.2 on the vector units, pointwise conv.3 as a GEMM
};
enum OutForm {     // the frontend's output linear (K = F C) and the first block's first LayerNorm
    OUT_IN_CHAIN,  // the first stage of the first row-chain launch (rowchain.hip.h: FRONT stage)
    OUT_SPLITK,    // split-K GEMM into the idle frontend buffer, then one pass sums the parts, adds the bias and applies the LayerNorm
    OUT_GEMM,      // one GEMM, the LayerNorm in its epilogue (rowln) or as a launch of its own
};
struct Form {
    FrontForm front;
    OutForm out;
    bool rowln;        // N == D products own whole rows: residual + LayerNorm in their epilogue
    bool chain;        // encoder as row-local chains (rowchain.hip.h), else one kernel per product
    bool ffn_fused;    // per product: the feed-forward module in one kernel, its hidden tensor on chip (ffn.hip.h)
    bool dw_fused;     // chains: the depthwise conv as the prologue of chain B, else a launch of its own
    bool a_fused;      // chains: chain A (out-proj -> GLU) as the head of chain B (rowchain.hip.h: one row tile of halo), else a launch of its own
    bool taps;         // debug taps (cocr_set_debug): the chains run their TAPS instantiation; per product, the second feed-forward module
                       // runs as two GEMMs with its closing LayerNorm apart (the stream is tapped before and after it)
    bool argmax;       // the decoder product's epilogue also leaves the per-frame argmax / maximum for cocr_ctc_greedy
    int chain_rows;    // chains: rows of the (M, D) activation one workgroup owns (chain_rows_for); 0 without chains
};

// Hardware queues the runtime multiplexes this process's streams onto: GPU_MAX_HW_QUEUES as the runtime reads it (once; 4 when unset or
// not a number), 1..32.
static int hw_queue_count() {
    static const int n = [] {
        const char *e = getenv("GPU_MAX_HW_QUEUES");
        char *end = nullptr;
        long v = e ? strtol(e, &end, 10) : 4;
        if (e && (end == e || *end)) v = 4;
        return (int)std::min(32L, std::max(1L, v));
    }();
    return n;
}

// Rows per workgroup of the chain launches of a forward over M rows, an instantiated form (rowchain_pick_mt).
//   * cocr_set_chain_rows / COCR_CHAIN_ROWS: the caller's choice, mapped to the nearest form.
//   * A model alone on its weights (S = 1): by M as ever -- the tallest form from 50 workgroups on, else 32 rows.
//   * S >= 2 models on one set of weights (cocr_share_weights: one per batch a caller keeps in flight): their streams share
//     Q = queues - 1 hardware queues (one serves the null stream), and streams on one queue run in turn, so S forwards take
//     ceil(S / Q) turns and c = S / ceil(S / Q) of them overlap.  The tallest form (fewest weight bytes streamed per row) whose
//     workgroups x c still cover the chip's 256 CUs: with fewer, CUs idle while every forward waits for its tall blocks (two 96-row
//     launches of 9600 rows put 200 workgroups on 256 CUs; 64 rows: 300).  Among the forms with at least 50 workgroups, as above; when
//     none of them covers the chip, the shortest.  DESIGN.md "Hardware queues and the rows per workgroup" has the measurements.
static int chain_rows_for(const cocr_model *m, int M) {
    const bool d256 = m->D == 256;
    auto form = [&](int hint) { return 16 * (d256 ? rowchain_pick_mt<256>(M, hint) : rowchain_pick_mt<512>(M, hint)); };
    if (m->chain_rows > 0) return form(m->chain_rows);
    const int S = (int)m->w->users.size();
    if (S < 2) return form(0);
    const int Q = std::max(1, hw_queue_count() - 1), turns = ceil_div(S, Q);      // c = S / turns
    static const int forms256[] = {96, 64, 48}, forms512[] = {64};
    const int *forms = d256 ? forms256 : forms512, nforms = d256 ? 3 : 1;
    int rows = 32;
    for (int i = 0; i < nforms; ++i) {
        if (M < 50 * forms[i]) continue;
        rows = forms[i];
        if ((long)ceil_div(M, rows) * S >= 256L * turns) break;
    }
    return rows;
}

// split-K over 2 workgroup groups (2 measured best of 2, 4, 8: 63 vs 74 vs 91 us for product + reduction)
#ifndef COCR_FO_SPLITS
#define COCR_FO_SPLITS 2
#endif
static Form forward_form(const cocr_model *m, int N, int W) {
    const bool bf16 = m->dtype == COCR_BF16, f2only = m->snum == 1;
    const int es = bf16 ? 2 : 4, D = m->D, C = m->C, H = m->H;
    const int T1 = out_len1(W), T2 = f2only ? T1 : out_len1(T1), F2 = m->feats[f2only ? 0 : 1];
    const int Kf = m->feats.back() * C, M = N * cocr_out_len(W, m->hp.subsampling_factor);
    const size_t lds32 = (size_t)(4 * 16 + 3) * ((H + 11) & ~3) * 4 + (size_t)16 * F2 * 80;      // FRONT_PW32: line tile + Z2 rows of 16 frames
    Form f{};
    f.taps = m->debug;
    f.rowln = bf16 ? gemm_rowln_supported<bf16_t>(D) : gemm_rowln_supported<float>(D);
    f.chain = bf16 && rowchain_supported(D, m->ff, m->dh) && !m->no_chain;
    if (bf16 && m->snum == 2 && frontend96_supported(C, m->feats[0], m->feats[1], H) && !m->no_front96) f.front = FRONT_96;
    else if (f2only) f.front = FRONT_CONV0;
    else if (bf16 && C == 32 && F2 <= 32 && lds32 <= 160 * 1024 && !f.taps && !m->no_front32) f.front = FRONT_PW32;
    else f.front = bf16 && C % 64 == 0 ? FRONT_MFMA : FRONT_VALU;
    if (f.chain && Kf % 256 == 0 && !m->no_front_chain) f.out = OUT_IN_CHAIN;
    else if (f.rowln && Kf % (COCR_FO_SPLITS * (128 / es)) == 0 && D <= 256 && (size_t)COCR_FO_SPLITS * M * D * 4 <= (size_t)N * T2 * F2 * C * es)
        f.out = OUT_SPLITK;     // (the parts fit the idle frontend buffer)
    else f.out = OUT_GEMM;
    f.ffn_fused = bf16 && f.rowln && ffn_fused_supported<int>(D, m->ff);
    f.dw_fused = m->ksz == 31 && (!m->no_dw_fuse || f.taps);
    f.argmax = m->ncls <= 128 && D % (128 / es) == 0;       // (whole k-steps of the decoder product)
    f.chain_rows = f.chain ? chain_rows_for(m, M) : 0;
    f.a_fused = f.chain && f.dw_fused && !m->no_a_fuse && rowchain_head_supported(D, m->ksz, f.chain_rows);
    return f;
}

// ------------------------------------------------------------------------------------ forward
// What every stage of one forward reads: the model, its form, the stream, the plan, the dimensions and the workspace
template <typename T> struct Fwd {
    cocr_model *m;
    const Form &f;
    hipStream_t s;
    const BlobPlan &P;
    const int N, W, D, T1, T2, F1, F2, Tn, M, Tp;        // T1 / F1, T2 / F2: frames / height after the first, second stride-2 stage
    const float ffr, scale;     // feed-forward residual factor; 1/sqrt(d_head) of the model (a padded model's engine d_head is its 64-wide slot)
    T *const za, *const zb;     // frontend: each stage's output in zb, its intermediate in za
    float *const x;             // the fp32 residual stream
    T *const xn, *const hid, *const q, *const k, *const v, *const ctx, *const glu, *const dwo;
    Fwd(cocr_model *m_, const Form &f_, int N_, int W_, hipStream_t s_)
        : m(m_), f(f_), s(s_), P(m_->w->plan), N(N_), W(W_), D(m_->D), T1(out_len1(W_)), T2(m_->snum == 1 ? T1 : out_len1(T1)), F1(m_->feats[0]),
          F2(m_->feats[m_->snum == 1 ? 0 : 1]), Tn(cocr_out_len(W_, m_->hp.subsampling_factor)), M(N_ * Tn), Tp(round_up(Tn, 64)),
          ffr(m_->hp.half_step_residual ? 0.5f : 1.0f), scale(1.0f / sqrtf((float)m_->rdh)), za((T *)m_->z_a), zb((T *)m_->z_b), x(m_->x),
          xn((T *)m_->xn), hid((T *)m_->hid), q((T *)m_->q), k((T *)m_->k), v((T *)m_->vt), ctx((T *)m_->ctx), glu((T *)m_->glu), dwo((T *)m_->dwo) {}
    const float *F32(size_t off) const { return (const float *)(m->w->blob + off); }
    const T *WT(size_t off) const { return (const T *)(m->w->blob + off); }
    template <typename S> int tap(int l, const char *what, const S *src, size_t n) const {      // debug tap "what" (l < 0) or "l<l>.what"
        if (!f.taps) return COCR_OK;
        char nm[64];
        if (l < 0) snprintf(nm, sizeof nm, "%s", what);
        else snprintf(nm, sizeof nm, "l%d.%s", l, what);
        return ::tap<S>(m, s, nm, src, n);
    }
    int tap_x(int l, const char *what, const float *src) const { return tap<float>(l, what, src, (size_t)M * D); }
    int tap_qkv(int l) const {
        const size_t n = m->qkv_bytes / sizeof(T);
        int rc;
        if ((rc = tap<T>(l, "q", q, n)) || (rc = tap<T>(l, "k", k, n)) || (rc = tap<T>(l, "v", v, n))) return rc;
        return COCR_OK;
    }
};

// ---- frontend: conv.0 + ReLU [+ depthwise conv.2 + pointwise conv.3 + ReLU] in the form's kernels, then the further (depthwise s2,
// pointwise, ReLU) stages.  The output is channel-last in zb: the flatten (b, t, (f, c)) of the output linear is a view of it.
template <typename T, typename TIn> static int frontend(const Fwd<T> &c, const TIn *lines) {
    cocr_model *m = c.m;
    const BlobPlan &P = c.P;
    const hipStream_t s = c.s;
    const int N = c.N, H = m->H, W = c.W, C = m->C, T1 = c.T1, F1 = c.F1, T2 = c.T2, F2 = c.F2;
    const FrontForm form = c.f.front;
    T *za = c.za, *zb = c.zb;
    int rc;
    if (form == FRONT_CONV0) {
        ProfScope ps(m, s, FAM_CONV12);
        const size_t npos = (size_t)N * T1 * F1;
        hipLaunchKernelGGL((frontend_conv0_kernel<T, TIn>), dim3((unsigned)((npos * (size_t)(C / 2) + 255) / 256)), dim3(256), 0, s, lines, H, W, T1, F1, C, npos,
                           c.F32(P.w0), c.F32(P.b0), zb);
        LAUNCH_CHECK();
        return COCR_OK;
    }
    if (form == FRONT_96) {
        ProfScope ps(m, s, FAM_FRONT96);
        const size_t n0 = (size_t)(C / 16) * 64 * 4;
        GEMM_TRY(launch_frontend96<TIn>(s, lines, N, H, W, T1, F1, T2, m->w->fpack, c.F32(P.b0), m->w->fpack + n0, c.F32(P.stages[0].dw_b),
                                        (const bf16_t *)(m->w->packed + P.stages[0].pw_w), c.F32(P.stages[0].pw_b), (bf16_t *)zb, m->stamps ? m->stamps + 128 : nullptr));
    } else if (form == FRONT_PW32) {
        ProfScope ps(m, s, FAM_CONV12);
        const size_t lds = (size_t)(4 * 16 + 3) * ((H + 11) & ~3) * 4 + (size_t)16 * F2 * 80;      // line tile + Z2 rows of 16 frames
        auto kern = frontend_conv12pw32_kernel<TIn>;
        GEMM_TRY(raise_lds_limit((const void *)kern, lds));
        hipLaunchKernelGGL(kern, dim3(ceil_div(T2, 16), N), dim3(256), lds, s, lines, H, W, T1, F1, T2, F2, c.F32(P.w0), c.F32(P.b0),
                           c.F32(P.stages[0].dw_w), c.F32(P.stages[0].dw_b), (const bf16_t *)c.WT(P.stages[0].pw_w), c.F32(P.stages[0].pw_b), (bf16_t *)zb);
        LAUNCH_CHECK();
    } else {
        {
            ProfScope ps(m, s, FAM_CONV12);
            if (form == FRONT_MFMA) {
                GEMM_TRY(launch_conv12_mfma<TIn>(s, lines, N, H, W, T1, F1, T2, F2, C, c.F32(P.w0), c.F32(P.b0), c.F32(P.stages[0].dw_w), c.F32(P.stages[0].dw_b),
                                                 (bf16_t *)za));
            } else {
                const int TB = std::max(1, 512 / C);                 // 256 threads = TB time steps x C/2 channel pairs
                const size_t lds = (size_t)(4 * TB + 3) * ((H + 11) & ~3) * 4;
                hipLaunchKernelGGL((frontend_conv12_kernel<T, TIn>), dim3(ceil_div(T2, TB), N), dim3(256), lds, s, lines, H, W, T1, F1, T2, F2, C,
                                   c.F32(P.w0), c.F32(P.b0), c.F32(P.stages[0].dw_w), c.F32(P.stages[0].dw_b), za, TB);
                LAUNCH_CHECK();
            }
        }
        if ((rc = c.tap(-1, "front.z2", za, (size_t)N * T2 * F2 * C))) return rc;
        ProfScope ps(m, s, FAM_FPW);
        EpiBiasAct<T, ACT_RELU> epi{zb, C, c.F32(P.stages[0].pw_b), C};
        GEMM_TRY(launch_gemm<T>(s, za, C, c.WT(P.stages[0].pw_w), C, N * T2 * F2, C, C, epi));
    }
    if ((rc = c.tap(-1, "front.z3", zb, (size_t)N * T2 * F2 * C))) return rc;      // (FRONT_96: Z2 does not exist)
    int Tc = T2, Fc = F2;
    for (int st = 1; st < m->snum - 1; ++st) {
        const int To = out_len1(Tc), Fo = m->feats[st + 1];
        {
            ProfScope ps(m, s, FAM_FDW);
            hipLaunchKernelGGL((dw3x3s2_kernel<T>), dim3(1024), dim3(256), 0, s, zb, N, Tc, Fc, To, Fo, C, c.F32(P.stages[st].dw_w),
                               c.F32(P.stages[st].dw_b), za);
            LAUNCH_CHECK();
        }
        {
            ProfScope ps(m, s, FAM_FPW);
            EpiBiasAct<T, ACT_RELU> epi{zb, C, c.F32(P.stages[st].pw_b), C};
            GEMM_TRY(launch_gemm<T>(s, za, C, c.WT(P.stages[st].pw_w), C, N * To * Fo, C, C, epi));
        }
        Tc = To; Fc = Fo;
    }
    return COCR_OK;
}

// xn <- LN1(x); g2 >= 0: x <- LN1(x), xn <- LN2(x) (a block-final LayerNorm chained with the next block's first); write_f32: x <- LN1(x)
template <typename T> static int layernorm(const Fwd<T> &c, size_t g1, size_t b1, bool write_f32, long g2, long b2) {
    ProfScope ps(c.m, c.s, FAM_LN);
    launch_layernorm<T>(c.s, c.x, c.M, c.D, c.F32(g1), c.F32(b1), write_f32 ? c.x : nullptr, g2 >= 0 ? c.F32((size_t)g2) : nullptr,
                        b2 >= 0 ? c.F32((size_t)b2) : nullptr, c.xn, c.m->rD);
    LAUNCH_CHECK();
    return COCR_OK;
}

// x <- [x +] alpha (A W^T + bias); then the LayerNorm(s) that follow in the reference (layernorm)
template <typename T> static int gemm_to_stream(const Fwd<T> &c, int fam, const T *A, int K, size_t w, size_t bias, float alpha, bool resid,
                                                size_t g1, size_t b1, long g2, long b2) {
    const int M = c.M, D = c.D;
    {
        ProfScope ps(c.m, c.s, fam);
        if (c.f.rowln) {
            EpiResidualLN<T, 1> e{c.x, D, c.F32(bias), alpha, D, resid ? 1 : 0, c.F32(g1), c.F32(b1), g2 >= 0 ? c.F32((size_t)g2) : nullptr,
                                  b2 >= 0 ? c.F32((size_t)b2) : nullptr, c.xn};
            e.Dn = c.m->rD;
            GEMM_TRY(launch_gemm_rowln<T>(c.s, A, K, c.WT(w), K, M, D, K, e));
            return COCR_OK;
        }
        if (resid) { EpiResidual e{c.x, D, c.F32(bias), alpha, D}; GEMM_TRY(launch_gemm<T>(c.s, A, K, c.WT(w), K, M, D, K, e)); }
        else { EpiStoreF32 e{c.x, D, c.F32(bias), D}; GEMM_TRY(launch_gemm<T>(c.s, A, K, c.WT(w), K, M, D, K, e)); }
    }
    return layernorm(c, g1, b1, g2 >= 0, g2, b2);
}

// ---- the frontend's output linear into the fp32 residual stream, and the first block's first LayerNorm
template <typename T> static int front_out(const Fwd<T> &c) {
    cocr_model *m = c.m;
    const BlobPlan &P = c.P;
    const FfnW &f0 = P.layers[0].ffn[0];
    const int Kf = m->feats.back() * m->C, M = c.M, D = c.D;
    if (c.f.out == OUT_IN_CHAIN) return COCR_OK;                  // (encoder_chains; front.y is tapped there)
    if (c.f.out == OUT_SPLITK) {
        float *partial = reinterpret_cast<float *>(c.za);          // the other frontend buffer is free now
        { ProfScope ps(m, c.s, FAM_FOUT); GEMM_TRY(launch_gemm_splitk<T>(c.s, c.zb, Kf, c.WT(P.wout), Kf, M, D, Kf, COCR_FO_SPLITS, partial)); }
        ProfScope ps(m, c.s, FAM_LN);
        hipLaunchKernelGGL((splitk_reduce_ln_kernel<T>), dim3(ceil_div(M, 16)), dim3(256), 0, c.s, partial, COCR_FO_SPLITS, (size_t)M * D, c.F32(P.bout), M, D,
                           m->rD, c.F32(f0.ln_g), c.F32(f0.ln_b), c.x, c.xn);
        LAUNCH_CHECK();
    } else {
        const int rc = gemm_to_stream(c, FAM_FOUT, c.zb, Kf, P.wout, P.bout, 1.0f, false, f0.ln_g, f0.ln_b, -1, -1);
        if (rc) return rc;
    }
    return c.tap_x(-1, "front.y", c.x);
}

template <typename T> static int ffn_up(const Fwd<T> &c, const FfnW &fw) {
    ProfScope ps(c.m, c.s, FAM_FFN_UP);
    EpiBiasAct<T, ACT_SILU> e{c.hid, c.m->ff, c.F32(fw.b1), c.m->ff};
    GEMM_TRY(launch_gemm<T>(c.s, c.xn, c.D, c.WT(fw.w1), c.D, c.M, c.m->ff, c.D, e));
    return COCR_OK;
}
// feed-forward module + the LayerNorm(s) that follow it (layernorm)
template <typename T> static int ffn(const Fwd<T> &c, const FfnW &fw, size_t g1, size_t b1, long g2, long b2) {
    if constexpr (sizeof(T) == 2) {
        if (c.f.ffn_fused) {
            ProfScope ps(c.m, c.s, FAM_FFN_FUSED);
            EpiResidualLN<T, 1> e{c.x, c.D, c.F32(fw.b2), c.ffr, c.D, 1, c.F32(g1), c.F32(b1), g2 >= 0 ? c.F32((size_t)g2) : nullptr,
                                  b2 >= 0 ? c.F32((size_t)b2) : nullptr, c.xn};
            GEMM_TRY(launch_ffn_fused(c.s, (const bf16_t *)c.xn, (const bf16_t *)c.WT(fw.w1), c.F32(fw.b1), (const bf16_t *)c.WT(fw.w2), c.M, c.D, c.m->ff, e));
            return COCR_OK;
        }
    }
    const int rc = ffn_up(c, fw);
    return rc ? rc : gemm_to_stream(c, FAM_FFN_DOWN, c.hid, c.m->ff, fw.w2, fw.b2, c.ffr, true, g1, b1, g2, b2);
}

template <typename T, int DHP> static hipError_t attention_dhp(const Fwd<T> &c, int l, unsigned long long *stamps) {
    const cocr_model *m = c.m;
    const LayerW &w = c.P.layers[l];
    return launch_attention<T, DHP>(c.s, c.N, c.q, c.k, c.v, (const T *)(m->w->ptab + (size_t)l * m->w->ptab_stride), c.F32(w.ub), c.F32(w.vb), c.ctx, c.Tn,
                                    c.Tp, m->heads, m->dh, c.scale, m->w->pos_maxlen - 1, stamps, m->att_tiled, m->att_resident_min, m->att_resident_long);
}
// block l's attention core: ctx <- attention(q, k, v) (launch_attention chooses the kernel)
template <typename T> static int attention(const Fwd<T> &c, int l, unsigned long long *stamps) {
    ProfScope ps(c.m, c.s, FAM_ATTN);
    const int dhp = c.m->dhp;
    GEMM_TRY((dhp == 32   ? attention_dhp<T, 32>(c, l, stamps)
              : dhp == 64 ? attention_dhp<T, 64>(c, l, stamps)
              : dhp == 96 ? attention_dhp<T, 96>(c, l, stamps)
                          : attention_dhp<T, 128>(c, l, stamps)));
    return COCR_OK;
}

template <typename T> static int dwconv(const Fwd<T> &c, const LayerW &w) {
    ProfScope ps(c.m, c.s, FAM_DW);
    launch_dwconv<T>(c.s, c.glu, c.N, c.Tn, c.D, c.m->ksz, c.F32(w.dww), c.F32(w.dwb), c.dwo);
    LAUNCH_CHECK();
    return COCR_OK;
}

// ---- encoder, one kernel per product
template <typename T> static int encoder_products(const Fwd<T> &c) {
    cocr_model *m = c.m;
    const hipStream_t s = c.s;
    const int M = c.M, D = c.D;
    const size_t MD = (size_t)M * D;
    int rc;
    for (int l = 0; l < m->L; ++l) {
        const LayerW &w = c.P.layers[l];
        const bool last = l + 1 == m->L;
        const long g_next = last ? -1 : (long)c.P.layers[l + 1].ffn[0].ln_g, b_next = last ? -1 : (long)c.P.layers[l + 1].ffn[0].ln_b;
        // FFN, half-step residual (feed_forward.py:45-52, encoder.py:68-75); epilogue: LayerNorm of the attention module
        if ((rc = ffn(c, w.ffn[0], w.a_ln_g, w.a_ln_b, -1, -1)) || (rc = c.tap_x(l, "ffn1", c.x))) return rc;
        // MHSA (attention.py:143-151)
        { ProfScope ps(m, s, FAM_QKV); EpiQKV<T> e{c.q, c.k, c.v, c.F32(w.bqkv), D, m->dh, m->dhp, m->heads, c.Tn, c.Tp, 3 * D}; GEMM_TRY(launch_gemm<T>(s, c.xn, D, c.WT(w.wqkv), D, M, 3 * D, D, e)); }
        if ((rc = attention(c, l, nullptr)) || (rc = c.tap_qkv(l)) || (rc = c.tap(l, "ctx", c.ctx, MD))) return rc;
        if ((rc = gemm_to_stream(c, FAM_AOUT, c.ctx, D, w.wo, w.bo, 1.0f, true, w.c_ln_g, w.c_ln_b, -1, -1)) || (rc = c.tap_x(l, "mhsa", c.x))) return rc;
        // conv module (convolution.py:135-148)
        { ProfScope ps(m, s, FAM_GLU); EpiGLU<T> e{c.glu, D, c.F32(w.bpw1), 2 * D}; GEMM_TRY(launch_gemm<T>(s, c.xn, D, c.WT(w.wpw1), D, M, 2 * D, D, e)); }
        if ((rc = dwconv(c, w)) || (rc = c.tap(l, "glu", c.glu, MD)) || (rc = c.tap(l, "dw", c.dwo, MD))) return rc;
        if ((rc = gemm_to_stream(c, FAM_PW2, c.dwo, D, w.wpw2, w.bpw2, 1.0f, true, w.ffn[1].ln_g, w.ffn[1].ln_b, -1, -1)) || (rc = c.tap_x(l, "conv", c.x))) return rc;
        // second FFN; its epilogue applies the block-final LayerNorm (encoder.py:99) chained with the next block's first
        if (!c.f.taps) {
            if ((rc = ffn(c, w.ffn[1], w.f_ln_g, w.f_ln_b, g_next, b_next))) return rc;
            continue;
        }
        if ((rc = ffn_up(c, w.ffn[1]))) return rc;
        { ProfScope ps(m, s, FAM_FFN_DOWN); EpiResidual e{c.x, D, c.F32(w.ffn[1].b2), c.ffr, D}; GEMM_TRY(launch_gemm<T>(s, c.hid, m->ff, c.WT(w.ffn[1].w2), m->ff, M, D, m->ff, e)); }
        if ((rc = c.tap_x(l, "ffn2", c.x)) || (rc = layernorm(c, w.f_ln_g, w.f_ln_b, true, g_next, b_next)) || (rc = c.tap_x(l, "out", c.x))) return rc;
    }
    return COCR_OK;
}

// ---- encoder as row-local chains (rowchain.hip.h, bf16): 3 launches per block (attention core, chain A, chain B), or 2 where chain A runs
// as chain B's head (Form::a_fused).  Debug taps: the
// TAPS instantiation of the SAME kernels copies what never leaves the chip (or is overwritten inside the launch) into tapbuf; everything
// else is read from the buffers the launches leave behind.
template <typename T> static int encoder_chains(const Fwd<T> &c) {
    cocr_model *m = c.m;
    const BlobPlan &P = c.P;
    const int D = c.D, M = c.M;
    const size_t MD = (size_t)M * D;
    const bool taps = c.f.taps;
    int rc;
    float *tp[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};      // (tp[4]: the head's "mhsa" -- a fused launch writes the four others too)
    bf16_t *tap_dw = nullptr;
    if (taps) {
        HIP_TRY(m->tapbuf.grow(MD * 5 + MD / 2));
        for (int i = 0; i < 5; ++i) tp[i] = m->tapbuf.p + (size_t)i * MD;
        tap_dw = reinterpret_cast<bf16_t *>(m->tapbuf.p + 5 * MD);
    }
    auto CW = [&](size_t off) { return (const bf16_t *)(m->w->packed + off); };      // chain weights: fragment-major copies (ensure_packed)
    auto launch = [&](const ChainArgs &a, int fam) -> int {
        ProfScope ps(m, c.s, fam);
        GEMM_TRY(a.nhead ? launch_rowchain_256_head(c.s, a, taps, c.f.chain_rows) : D == 256 ? launch_rowchain_256(c.s, a, taps, c.f.chain_rows) : launch_rowchain_512(c.s, a, taps, c.f.chain_rows));
        return COCR_OK;
    };
    // the fp32 stream between the chain launches: in the kernels' register order (ChainArgs::x_in_blocked); the first launch reads
    // the row-major stream the frontend's reduction wrote
    auto base = [&](const T *A0, int nstages) {
        ChainArgs a{}; a.x = c.x; a.x_in_blocked = 1; a.x_out_blocked = 1; a.xn = (bf16_t *)c.xn; a.M = M; a.dh = m->dh; a.dhp = m->dhp; a.heads = m->heads; a.T_ = c.Tn; a.Tp = c.Tp; a.inv_d = 1.0f / (float)m->rD; a.xcd_order = m->chain_xcd ? 1 : 0;
        a.kd = (m->padded && !m->no_kskip) ? ceil_div(m->rD, 32) : 8; a.kl = (m->padded && !m->no_kskip) ? ((m->rff - 1) % 256) / 32 + 1 : 8;
        a.A0 = (const bf16_t *)A0; a.nstages = nstages; return a; };
    auto st_rowln = [&](size_t wgt, size_t bias, float alpha, size_t g1, size_t b1) {
        ChainStage st{}; st.kind = ST_ROWLN; st.W = CW(wgt); st.bias = c.F32(bias); st.N = D; st.alpha = alpha;
        st.g1 = c.F32(g1); st.b1 = c.F32(b1); return st; };
    auto st_ffn = [&](const FfnW &fw, size_t g1, size_t b1, long g2, long b2) {
        ChainStage st{}; st.kind = ST_FFN; st.W = CW(fw.w1); st.W2 = CW(fw.w2); st.bias = c.F32(fw.b1); st.bias2 = c.F32(fw.b2);
        st.N = m->ff; st.alpha = c.ffr; st.g1 = c.F32(g1); st.b1 = c.F32(b1);      // (W2's fragment-major copy is pre-scaled by ffr: ensure_packed)
        st.g2 = g2 >= 0 ? c.F32((size_t)g2) : nullptr; st.b2 = b2 >= 0 ? c.F32((size_t)b2) : nullptr; return st; };
    auto st_qkv = [&](const LayerW &lw) {
        ChainStage st{}; st.kind = ST_QKV; st.W = CW(lw.wqkv); st.bias = c.F32(lw.bqkv); st.N = 3 * D;
        st.q = (bf16_t *)c.q; st.k = (bf16_t *)c.k; st.v = (bf16_t *)c.v; return st; };
    const LayerW &w0 = P.layers[0];
    if (c.f.out == OUT_IN_CHAIN) {   // frontend output linear + first LayerNorm -> first block's FFN -> its q/k/v projection
        ChainArgs a = base(c.zb, 3); a.x_in_blocked = 0;
        ChainStage f{}; f.kind = ST_FRONT; f.W = CW(P.wout); f.bias = c.F32(P.bout); f.N = D; f.K = m->feats.back() * m->C; f.alpha = 1.0f;
        f.g1 = c.F32(w0.ffn[0].ln_g); f.b1 = c.F32(w0.ffn[0].ln_b);
        a.st[0] = f;
        a.st[1] = st_ffn(w0.ffn[0], w0.a_ln_g, w0.a_ln_b, -1, -1); a.st[1].store_x = 1;
        a.st[2] = st_qkv(w0);
        a.st[0].tap_pre = tp[1]; a.st[1].tap_pre = tp[0];
        if ((rc = launch(a, FAM_CH_FRONT)) || (rc = c.tap_x(-1, "front.y", tp[1])) || (rc = c.tap_x(0, "ffn1", tp[0])) || (rc = c.tap_qkv(0))) return rc;
    } else {   // first block's FFN + q/k/v projection on the frontend output
        ChainArgs a = base(c.xn, 2); a.x_in_blocked = 0;
        a.st[0] = st_ffn(w0.ffn[0], w0.a_ln_g, w0.a_ln_b, -1, -1); a.st[0].store_x = 1;
        a.st[1] = st_qkv(w0);
        a.st[0].tap_pre = tp[0];
        if ((rc = launch(a, FAM_CH_FIRST)) || (rc = c.tap_x(0, "ffn1", tp[0])) || (rc = c.tap_qkv(0))) return rc;
    }
    if (m->ffn_probe) {
        // measurement only (COCR_FFN_PROBE=1): block 0's first feed-forward module as a launch of its own on real operands (the
        // frontend output's first M x D values, the stream the launch above left), results discarded (no store flags) -- so that
        // rocprofv3's matrix-pipe counters can be read for the FFN products alone (tools/ffn_probe.py, profiles/r03_ffn_probe_*)
        ChainArgs a = base(c.zb, 1);
        a.st[0] = st_ffn(w0.ffn[0], w0.a_ln_g, w0.a_ln_b, -1, -1);
        if ((rc = launch(a, FAM_FFN_PROBE))) return rc;
    }
    for (int l = 0; l < m->L; ++l) {
        const LayerW &w = P.layers[l];
        const bool last = l + 1 == m->L;
        if ((rc = attention(c, l, (m->stamps && l == 5) ? m->stamps + 192 : nullptr))) return rc;
        // out-proj + residual + conv-module LayerNorm -> pointwise conv 1 + GLU: a launch of its own, or the head of the next one
        ChainStage ha = st_rowln(w.wo, w.bo, 1.0f, w.c_ln_g, w.c_ln_b);
        ChainStage hg{}; hg.kind = ST_GLU; hg.W = CW(w.wpw1); hg.bias = c.F32(w.bpw1); hg.N = 2 * D; hg.out = (bf16_t *)c.glu;
        ha.tap_pre = tp[4];
        if (!c.f.a_fused) {
            ChainArgs a = base(c.ctx, 2);
            a.st[0] = ha; a.st[0].store_x = 1; a.st[0].tap_pre = tp[0];
            a.st[1] = hg;
            if ((rc = c.tap(l, "ctx", c.ctx, MD)) || (rc = launch(a, FAM_CH_A)) || (rc = c.tap_x(l, "mhsa", tp[0])) || (rc = c.tap(l, "glu", c.glu, MD))) return rc;
        } else if ((rc = c.tap(l, "ctx", c.ctx, MD))) return rc;
        if (!c.f.dw_fused && (rc = dwconv(c, w))) return rc;
        // [depthwise conv + BN + SiLU ->] pointwise conv 2 + residual + LayerNorm -> FFN 2 (+ closing LayerNorm [+ next block's]) [-> next block's FFN 1 -> its q/k/v]
        ChainArgs a = base(c.dwo, 2);
        if (c.f.dw_fused) { a.dw_in = (const bf16_t *)c.glu; a.dw_w = c.F32(w.dww); a.dw_b = c.F32(w.dwb); a.tap_dw = tap_dw; }
        if (c.f.a_fused) {      // the head reads the stream (with its halo rows) from one buffer, the launch writes the other
            a.A0 = (const bf16_t *)c.ctx; a.dw_in = nullptr; a.nhead = 2; a.st[4] = ha; a.st[5] = hg;
            a.xh = (l & 1) ? m->x2 : c.x; a.x = (l & 1) ? c.x : m->x2;
            if (!taps) a.st[5].out = nullptr;
        }
        a.st[0] = st_rowln(w.wpw2, w.bpw2, 1.0f, w.ffn[1].ln_g, w.ffn[1].ln_b);
        a.st[0].tap_pre = tp[0];
        if (!last) {
            const LayerW &nx = P.layers[l + 1];
            a.st[1] = st_ffn(w.ffn[1], w.f_ln_g, w.f_ln_b, (long)nx.ffn[0].ln_g, (long)nx.ffn[0].ln_b);
            a.st[2] = st_ffn(nx.ffn[0], nx.a_ln_g, nx.a_ln_b, -1, -1); a.st[2].store_x = 1;
            a.st[3] = st_qkv(nx);
            a.nstages = 4;
            a.st[1].tap_pre = tp[1]; a.st[1].tap_post = tp[2]; a.st[2].tap_pre = tp[3];
            a.stamps = (m->stamps && l == 5) ? m->stamps + 1024 : nullptr;
            if ((rc = launch(a, FAM_CH_B))) return rc;
        } else {
            a.st[1] = st_ffn(w.ffn[1], w.f_ln_g, w.f_ln_b, -1, -1); a.st[1].store_x = 1; a.st[1].store_xn = 1;
            a.st[1].tap_pre = tp[1];
            if ((rc = launch(a, FAM_CH_LAST))) return rc;
        }
        if (c.f.a_fused && ((rc = c.tap_x(l, "mhsa", tp[4])) || (rc = c.tap(l, "glu", c.glu, MD)))) return rc;
        // every chain B: the depthwise output, the stream after the conv module and after FFN 2
        if ((rc = c.tap(l, "dw", c.f.dw_fused ? (const T *)tap_dw : (const T *)c.dwo, MD)) || (rc = c.tap_x(l, "conv", tp[0])) || (rc = c.tap_x(l, "ffn2", tp[1])))
            return rc;
        if (!last && ((rc = c.tap_x(l, "out", tp[2])) || (rc = c.tap_x(l + 1, "ffn1", tp[3])) || (rc = c.tap_qkv(l + 1)))) return rc;
        if (last && (rc = c.tap(l, "out", c.xn, MD))) return rc;     // (the closing LayerNorm's output exists only as the bf16 decoder operand xn here)
    }
    return COCR_OK;
}

// ---- decoder nn.Linear (pred.py:90,121): logits fp32.  The argmax form's epilogue also leaves the greedy decoder's per-frame argmax /
// maximum (ctc_lab / ctc_val): cocr_ctc_greedy on these logits then only merges runs.
template <typename T> static int decoder(const Fwd<T> &c, float *logits) {
    cocr_model *m = c.m;
    const int M = c.M, D = c.D;
    ProfScope ps(m, c.s, FAM_DEC);
    if (c.f.argmax) {
        const int rc = ensure_ctc_scratch(m, (size_t)M);
        if (rc) return rc;
        EpiLogitsArgmax e{logits, m->ncls, c.F32(c.P.bdec), m->ncls, m->ctc_lab.p, m->ctc_val.p};
        GemmArgs<T> a{c.xn, D, c.WT(c.P.wdec), D, M, m->ncls, D, 0};
        GEMM_TRY((launch_ring_cfg<T, 64, 128, 3, EpiLogitsArgmax>(c.s, a, e)));
        m->amax_ok = true; m->amax_rows = M;
        return COCR_OK;
    }
    EpiStoreF32 e{logits, m->ncls, c.F32(c.P.bdec), m->ncls};
    GEMM_TRY(launch_gemm<T>(c.s, c.xn, D, c.WT(c.P.wdec), D, M, m->ncls, D, e));
    m->amax_ok = false;
    return COCR_OK;
}

// frontend -> output linear -> encoder -> decoder, in the form `f`
template <typename T, typename TIn>
static int forward_impl(cocr_model *m, const Form &f, const TIn *lines, int N, int W, float *logits, hipStream_t s) {
    const Fwd<T> c(m, f, N, W, s);
    // profiling: one EMPTY event pair per forward = the fixed cost of a bracket (record -> record with nothing between), which
    // bench.py subtracts from every family's average so that the event timings line up with rocprofv3's dispatch durations
    { ProfScope ps(m, s, FAM_EMPTY); }
    int rc;
    if ((rc = frontend<T, TIn>(c, lines)) || (rc = front_out(c))) return rc;
    if (m->vtN != N || m->vtT != c.Tn) {   // pad dims of q, k, v must read as zero for this shape
        for (T *p : {c.q, c.k, c.v}) HIP_TRY(hipMemsetAsync(p, 0, m->qkv_bytes, s));
        m->vtN = N; m->vtT = c.Tn;
    }
    if constexpr (sizeof(T) == 2) rc = f.chain ? encoder_chains(c) : encoder_products(c);
    else rc = encoder_products(c);
    return rc ? rc : decoder(c, logits);
}

// (Re)builds the fragment-major weight copies that the form's row chains and fused frontend read.  Runs on `s` ahead of the forward's
// launches (stream order covers a blob import issued on the same stream), never inside a graph capture.  What it packs does not depend
// on the batch shape (forward_form).
int Weights::ensure_packed(const Form &f, hipStream_t s) {
    if ((!f.chain && f.front != FRONT_96) || !packed_stale) return COCR_OK;
    const cocr_model *m = users.front();
    if (!packed) HIP_TRY(hipMalloc((void **)&packed, plan.total));
    const int D = m->D, ff = m->ff, C = m->C;
    auto pack = [&](size_t off, int N, int K, float scale = 1.0f) {
        hipLaunchKernelGGL(pack_frag_kernel, dim3(std::min(1024, ceil_div(N * K / 8, 256))), dim3(256), 0, s, (const bf16_t *)(blob + off),
                           (bf16_t *)(packed + off), N, K, scale);
    };
    const float ffr = m->hp.half_step_residual ? 0.5f : 1.0f;       // the FFN's residual factor rides on the packed copy of its second matrix (exact)
    if (f.chain)
        for (const LayerW &w : plan.layers) {
            for (int i = 0; i < 2; ++i) { pack(w.ffn[i].w1, ff, D); pack(w.ffn[i].w2, D, ff, ffr); }
            pack(w.wqkv, 3 * D, D); pack(w.wo, D, D); pack(w.wpw1, 2 * D, D); pack(w.wpw2, D, D);
        }
    if (f.out == OUT_IN_CHAIN) pack(plan.wout, D, m->feats.back() * C);      // the FRONT stage's matrix
    if (f.front == FRONT_96) {
        pack(plan.stages[0].pw_w, C, C);
        const size_t n0 = (size_t)(C / 16) * 64 * 4, n2 = (size_t)(C / 16) * 5 * 64 * 8;
        if (!fpack) HIP_TRY(hipMalloc((void **)&fpack, (n0 + n2) * sizeof(bf16_t)));
        hipLaunchKernelGGL(frontend_pack_kernel, dim3(ceil_div((int)n2, 256)), dim3(256), 0, s, (const float *)(blob + plan.w0),
                           (const float *)(blob + plan.stages[0].dw_w), fpack, fpack + n0, C);
    }
    LAUNCH_CHECK();
    packed_stale = false;
    return COCR_OK;
}

static int forward_entry(cocr_model *m, const void *lines, int line_dtype, int N, int H, int W, const int32_t *in_lens,
                         float *logits, int32_t *out_lens, void *stream);
extern "C" int cocr_forward(cocr_model *m, const void *lines, int line_dtype, int N, int H, int W, const int32_t *in_lens,
                            float *logits, int32_t *out_lens, void *stream) {
    if (m) m->amax_logits = nullptr;
    const int rc = forward_entry(m, lines, line_dtype, N, H, W, in_lens, logits, out_lens, stream);
    if (rc == COCR_OK && m->amax_ok) m->amax_logits = logits;      // (plain run, replay or staged replay: the sequence ended with the argmax epilogue)
    return rc;
}
extern "C" int cocr_forget_argmax(cocr_model *m) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    m->amax_logits = nullptr;
    return COCR_OK;
}
static int run_forward(cocr_model *m, const Form &form, const void *in, int line_dtype, int N, int W, float *out, hipStream_t s) {
    if (m->dtype == COCR_BF16) {
        if (line_dtype == COCR_F32) return forward_impl<bf16_t, float>(m, form, (const float *)in, N, W, out, s);
        if (line_dtype == COCR_U8) return forward_impl<bf16_t, uint8_t>(m, form, (const uint8_t *)in, N, W, out, s);
    } else {
        if (line_dtype == COCR_F32) return forward_impl<float, float>(m, form, (const float *)in, N, W, out, s);
        if (line_dtype == COCR_U8) return forward_impl<float, uint8_t>(m, form, (const uint8_t *)in, N, W, out, s);
    }
    return fail(COCR_EINVAL, "line dtype must be COCR_F32 or COCR_U8");
}

// The derived copies that the form reads, rebuilt where they are stale (rarely: new weights, longer tables), and this model brought up to
// the set's generation.  A set with several users, or one that has been rebuilt before, is rebuilt with the device idle: other models
// may read it on other streams.  (Any user packs what every user's form reads: models that share weights share the switches.)
static int sync_weights(cocr_model *m, const Form &form, hipStream_t s) {
    Weights &w = *m->w;
    if (w.stale()) {
        const bool idle = w.users.size() > 1 || w.gen > 1;
        int rc;
        if (idle) HIP_TRY(hipDeviceSynchronize());
        if ((rc = w.ensure_packed(form, s)) || (rc = w.ensure_ptab(s))) return rc;
        HIP_TRY(idle ? hipDeviceSynchronize() : hipStreamSynchronize(s));
        ++w.gen;
    }
    if (m->seen_gen != w.gen) {      // captured launches may point at moved buffers, or run ahead of a rebuild
        m->graphs.drop();
        m->seen_gen = w.gen;
    }
    return COCR_OK;
}

// Launch-bound regime (~120 kernels of 10-40 us per forward): the second identical call captures the launch sequence into a
// hipGraph, later identical calls replay it (one host call instead of ~120).  GraphCache says which sequence a call gets.
static int forward_graphed(cocr_model *m, const Form &form, const void *lines, int line_dtype, int N, int W, float *logits, hipStream_t s) {
    const int Tn = cocr_out_len(W, m->hp.subsampling_factor);
    const GraphCache::Call call{lines, logits, N, W, line_dtype, form.chain_rows};
    hipGraphExec_t exec = nullptr;
    const GraphCache::Action act = m->graphs.next(call, m->vtN == N && m->vtT == Tn, &exec);
    if (act == GraphCache::PLAIN) return run_forward(m, form, lines, line_dtype, N, W, logits, s);
    const bool staged = act == GraphCache::STAGED_REPLAY || act == GraphCache::STAGED_CAPTURE;
    if (act == GraphCache::CAPTURE || act == GraphCache::STAGED_CAPTURE) {
        hipGraph_t graph = nullptr;
        HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int r = run_forward(m, form, staged ? m->g_lines : lines, line_dtype, N, W, staged ? m->g_logits : logits, s);
        const hipError_t ce = hipStreamEndCapture(s, &graph);
        if (r) { if (graph) (void)hipGraphDestroy(graph); return r; }
        if (ce != hipSuccess) return fail(COCR_EHIP, "hipStreamEndCapture failed: %s", hipGetErrorString(ce));
        HIP_TRY(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        (void)hipGraphDestroy(graph);
        m->graphs.add(staged ? GraphCache::staged(call) : call, exec);
    }
    if (staged) HIP_TRY(hipMemcpyAsync(m->g_lines, lines, (size_t)N * m->H * W * (line_dtype == COCR_F32 ? 4 : 1), hipMemcpyDefault, s));
    HIP_TRY(hipGraphLaunch(exec, s));
    if (staged) HIP_TRY(hipMemcpyAsync(logits, m->g_logits, (size_t)N * Tn * m->ncls * 4, hipMemcpyDeviceToDevice, s));
    return COCR_OK;
}

static int forward_entry(cocr_model *m, const void *lines, int line_dtype, int N, int H, int W, const int32_t *in_lens,
                         float *logits, int32_t *out_lens, void *stream) {
    if (!m || !lines || !logits) return fail(COCR_EINVAL, "null argument");
    if (!m->w->blob) return fail(COCR_ESTATE, "model not finalized");
    if (H != m->H) return fail(COCR_EINVAL, "line height %d does not match the model's height %d", H, m->H);
    if (N < 1 || W < 1) return fail(COCR_EINVAL, "empty batch");
    if (line_dtype != COCR_F32 && line_dtype != COCR_U8) return fail(COCR_EINVAL, "line dtype must be COCR_F32 or COCR_U8");
    const int Tn = cocr_out_len(W, m->hp.subsampling_factor);
    if (round_up(Tn, 64) > 65536) return fail(COCR_EUNSUPPORTED, "more than 65536 output frames");
    HIP_TRY(hipSetDevice(m->device));
    int rc;
    if ((rc = adopt_layout(m)) || (rc = m->w->cover_positions(round_up(Tn, 64))) || (rc = cocr_reserve(m, N, W))) return rc;
    if (in_lens && out_lens)
        for (int i = 0; i < N; ++i) out_lens[i] = cocr_out_len(in_lens[i], m->hp.subsampling_factor);
    hipStream_t s = (hipStream_t)stream;
    const Form form = forward_form(m, N, W);
    if ((rc = sync_weights(m, form, s))) return rc;
    m->lastN = N;
    m->lastT = Tn;
    if (!m->use_graph || m->debug || m->profile || s == nullptr) return run_forward(m, form, lines, line_dtype, N, W, logits, s);
    return forward_graphed(m, form, lines, line_dtype, N, W, logits, s);
}

// ------------------------------------------------------------------------------------ host-side collation
extern "C" int cocr_collate_lines(const void *const *lines, const int32_t *widths, int N, int H, int elem_size, void *dst, int W, int threads) {
    if (N < 0 || H <= 0 || W <= 0 || (elem_size != 1 && elem_size != 4)) return fail(COCR_EINVAL, "collate: bad shape or element size");
    if (N == 0) return COCR_OK;
    if (!lines || !widths || !dst) return fail(COCR_EINVAL, "collate: null argument");
    for (int i = 0; i < N; ++i)
        if (!lines[i] || widths[i] < 0 || widths[i] > W) return fail(COCR_EINVAL, "collate: line %d is %d wide, the batch %d", i, widths[i], W);
    const long rows = (long)N * H;
    auto span = [=](long r0, long r1) {
        for (long r = r0; r < r1; ++r) {
            const int i = (int)(r / H), y = (int)(r % H);
            const size_t wb = (size_t)widths[i] * elem_size, Wb = (size_t)W * elem_size;
            char *d = (char *)dst + (size_t)r * Wb;
            memcpy(d, (const char *)lines[i] + (size_t)y * wb, wb);
            memset(d + wb, 0, Wb - wb);
        }
    };
    const int nt = (int)std::max(1L, std::min<long>(std::min(threads, 64), rows / 64));
    if (nt <= 1) { span(0, rows); return COCR_OK; }
    std::vector<std::thread> pool;
    pool.reserve(nt - 1);
    for (int t = 1; t < nt; ++t) pool.emplace_back(span, rows * t / nt, rows * (t + 1) / nt);
    span(0, rows / nt);
    for (auto &t : pool) t.join();
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ CTC
// The per-line lengths reach the decode kernels through a PINNED host ring: an async copy from pageable memory goes through the
// runtime's staging buffers, and a third such copy in flight (three batches on three streams, each copy queued behind its
// forward) blocked the host until the first forward had finished -- 5.5 ms per run start.  `d_lens`: the lengths on the device.
static int upload_lens(cocr_model *m, const int32_t *lens, int N, hipStream_t s, const int32_t *&d_lens) {
    int32_t *h, *d;
    HIP_TRY(m->lens_ring.stage((size_t)N * 4, h, d));
    memcpy(h, lens, (size_t)N * 4);
    HIP_TRY(m->lens_ring.commit((size_t)N * 4, s));
    d_lens = d;
    return COCR_OK;
}

static int ensure_ctc_scratch(cocr_model *m, size_t rows) {
    if (rows <= m->ctc_lab.n && rows <= m->ctc_val.n) return COCR_OK;
    HIP_TRY(hipDeviceSynchronize());                          // (captured launches that point at the old scratch are dropped with it)
    m->graphs.drop();
    m->amax_logits = nullptr;
    HIP_TRY(m->ctc_lab.grow(rows));
    HIP_TRY(m->ctc_val.grow(rows));
    return COCR_OK;
}

extern "C" int cocr_ctc_greedy(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens, int32_t *labels,
                               int32_t *starts, int32_t *ends, float *conf, int32_t *counts, int max_per_line, void *stream) {
    if (!m || !logits || !out_lens || !labels || !starts || !ends || !conf || !counts) return fail(COCR_EINVAL, "null argument");
    if (N < 1 || T < 1 || ncls < 1 || max_per_line < 1) return fail(COCR_EINVAL, "empty problem");
    if (T > 8000) return fail(COCR_EUNSUPPORTED, "more than 8000 frames per line");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const int32_t *d_lens;
    int rc = upload_lens(m, out_lens, N, s, d_lens);
    if (rc) return rc;
    const bool have_argmax = logits == m->amax_logits && N * T == m->amax_rows && ncls == m->ncls;      // the decoder's epilogue computed it for these logits
    if (!have_argmax && (rc = ensure_ctc_scratch(m, (size_t)N * T))) return rc;
    ProfScope ps(m, s, FAM_GREEDY);
    if (!have_argmax) {
        m->amax_logits = nullptr;                             // the scratch no longer belongs to the last forward's logits
        hipLaunchKernelGGL(ctc_argmax_kernel, dim3(ceil_div(N * T, 4)), dim3(256), 0, s, logits, T, ncls, N * T, d_lens, m->ctc_lab.p, m->ctc_val.p);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ctc_collapse_kernel, dim3(N), dim3(64), (size_t)T * 8, s, T, d_lens, m->ctc_lab.p, m->ctc_val.p, labels, starts, ends, conf, counts,
                       max_per_line);
    LAUNCH_CHECK();
    return COCR_OK;
}

extern "C" int cocr_ctc_beam(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens, int32_t *labels,
                             int32_t *starts, int32_t *ends, float *conf, int32_t *counts, int max_per_line, int beam, void *stream) {
    if (!m || !logits || !out_lens || !labels || !starts || !ends || !conf || !counts) return fail(COCR_EINVAL, "null argument");
    if (N < 1 || T < 1 || ncls < 2 || max_per_line < 1) return fail(COCR_EINVAL, "empty problem");
    if (beam < 1 || beam > COCR_BEAM_MAX) return fail(COCR_EINVAL, "beam must be in 1..%d", COCR_BEAM_MAX);
    if (ncls > 65535) return fail(COCR_EUNSUPPORTED, "more than 65535 classes");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const int32_t *d_lens;
    int rc = upload_lens(m, out_lens, N, s, d_lens);
    if (rc) return rc;
    const bool fast = ncls <= 256 && !m->beam_ref;            // ctc_beam_rank_kernel + ctc_beam_walk_kernel: frames ranked in parallel, a static pruned candidate set per frame
    const int K = std::min(beam + 1, ncls - 1);
    // scratch: back-pointers [N][T][COCR_BEAM_MAX] i32, then log Z [N][T] (exhaustive kernel) or the frame records (fast)
    const size_t need = (size_t)N * T * ((size_t)COCR_BEAM_MAX * 4 + (fast ? (size_t)COCR_BEAM_REC : 4));
    HIP_TRY(m->beam_bp.grow(need));
    int32_t *bp = reinterpret_cast<int32_t *>(m->beam_bp.p);
    ProfScope ps(m, s, FAM_BEAM);
    if (fast) {
        unsigned char *rec = reinterpret_cast<unsigned char *>(bp + (size_t)N * T * COCR_BEAM_MAX);
        const size_t dyn = (size_t)T * ((size_t)beam * 4 + 8);                 // back-pointers + the label stack of the final walk, in LDS when they fit
        const int bp_in_lds = dyn <= 96 * 1024;
        hipLaunchKernelGGL(ctc_beam_rank_kernel, dim3(N * T), dim3(256), 0, s, logits, T, ncls, d_lens, K, rec);
        auto walk = ctc_beam_walk_kernel<3>;                          // candidates per lane of a wave: <= 88 for beam <= 16, <= 184 for beam 32
        if (beam <= 16) walk = ctc_beam_walk_kernel<2>;
        // (the kernel also has ~12 KB of static LDS: the limit raised for the dynamic part stays below 160 KB - static)
        if (bp_in_lds) HIP_TRY(raise_lds_limit((const void *)walk, dyn, 48 * 1024, 96 * 1024));
        hipLaunchKernelGGL(walk, dim3(N), dim3(256), bp_in_lds ? dyn : 0, s, logits, T, ncls, d_lens, beam, K, labels, starts,
                           ends, conf, counts, max_per_line, rec, bp, bp_in_lds, m->stamps ? m->stamps + 240 : nullptr);
    } else {
        float *logz = reinterpret_cast<float *>(bp + (size_t)N * T * COCR_BEAM_MAX);
        const size_t lds = ((size_t)ncls + (size_t)beam * ncls) * 4 + COCR_BEAM_MAX * (11 * 4 + 2 * 8) + 64;
        if (lds > 150 * 1024) return fail(COCR_EUNSUPPORTED, "beam x classes too large for the LDS candidate table");
        HIP_TRY(raise_lds_limit((const void *)ctc_beam_kernel, lds));
        hipLaunchKernelGGL(ctc_beam_kernel, dim3(N), dim3(64), lds, s, logits, T, ncls, d_lens, beam, labels, starts, ends, conf, counts,
                           max_per_line, bp, logz);
    }
    LAUNCH_CHECK();
    return COCR_OK;
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

extern "C" int cocr_ctc_beam_lm(cocr_model *m, cocr_lm *lm, const float *logits, int N, int T, int ncls, const int32_t *out_lens, int32_t *labels,
                                int32_t *starts, int32_t *ends, float *conf, int32_t *counts, int max_per_line, int beam, int classes, float alpha,
                                float beta, float *score, void *stream) {
    if (!m || !lm || !logits || !out_lens || !labels || !starts || !ends || !conf || !counts) return fail(COCR_EINVAL, "null argument");
    if (N < 1 || T < 1 || ncls < 2 || max_per_line < 1) return fail(COCR_EINVAL, "empty problem");
    if (T > 8000) return fail(COCR_EUNSUPPORTED, "more than 8000 frames per line");
    if (beam < 1 || beam > COCR_BEAM_MAX) return fail(COCR_EINVAL, "beam must be in 1..%d", COCR_BEAM_MAX);
    if (classes < 1 || classes > COCR_LM_KMAX) return fail(COCR_EINVAL, "classes must be in 1..%d", COCR_LM_KMAX);
    if (ncls != lm->ncls) return fail(COCR_EINVAL, "the logits have %d classes, the language model %d", ncls, lm->ncls);
    if (lm->device != m->device) return fail(COCR_EINVAL, "the language model lives on device %d, the model on %d", lm->device, m->device);
    if (!std::isfinite(alpha) || !std::isfinite(beta)) return fail(COCR_EINVAL, "alpha and beta must be finite");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const int32_t *d_lens;
    int rc = upload_lens(m, out_lens, N, s, d_lens);
    if (rc) return rc;
    const int K = std::min(classes, ncls - 1);
    // scratch: back-pointers [N][T][COCR_BEAM_MAX] i32, then the frame records [N][T][COCR_LM_REC] f32
    const size_t bp_bytes = (size_t)N * T * COCR_BEAM_MAX * 4;
    HIP_TRY(m->lm_scratch.grow(bp_bytes + (size_t)N * T * COCR_LM_REC * 4));
    int32_t *bp = reinterpret_cast<int32_t *>(m->lm_scratch.p);
    float *rec = reinterpret_cast<float *>(m->lm_scratch.p + bp_bytes);
    const size_t dyn = (size_t)T * ((size_t)beam * 4 + 8);                     // back-pointers + the label stack of the final walk, in LDS when they fit
    const int bp_in_lds = dyn <= 96 * 1024;
    if (bp_in_lds) HIP_TRY(raise_lds_limit((const void *)ctc_lm_walk_kernel, dyn, 16 * 1024, 96 * 1024));      // (the kernel has ~30 KB of static LDS)
    cocr_lm_tables L;
    L.unigram = lm->unigram.p; L.nkeys = lm->nkeys.p; L.nlogp = lm->nlogp.p; L.ckeys = lm->ckeys.p; L.cbow = lm->cbow.p;
    L.nmask = (unsigned)(lm->nslots - 1); L.cmask = (unsigned)(lm->cslots - 1); L.order = lm->order;
    ProfScope ps(m, s, FAM_BEAM);
    hipLaunchKernelGGL(ctc_lm_topk_kernel, dim3(ceil_div(N * T, 4)), dim3(256), 0, s, logits, T, ncls, N * T, d_lens, K, rec);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(ctc_lm_walk_kernel, dim3(N), dim3(256), bp_in_lds ? dyn : 0, s, logits, T, ncls, d_lens, beam, K, L, alpha, beta, labels, starts,
                       ends, conf, counts, score, max_per_line, rec, bp, bp_in_lds);
    LAUNCH_CHECK();
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ CTC loss (ctc_loss.hip.h)
// The targets of a batch on the device, and the kernel form for its longest line: sj 64-state columns per lane.
struct CtcTargets { const int32_t *lens, *label_lens, *label_off, *labels; int sj; };

// Loss and forced alignment: checks the per-line lengths and the labels, then sends [lens | label lens | label offsets | labels]
// through the targets ring.  `outputs_ok`: the caller's per-label output pointers are set (asked for only where there are labels);
// `too_long`: the status for a line of more than COCR_CTCL_MAX_LABELS labels.
static int upload_targets(cocr_model *m, int N, int T, int ncls, const int32_t *out_lens, const int32_t *targets, const int32_t *label_lens,
                          bool outputs_ok, int too_long, void *stream, CtcTargets &t) {
    size_t total = 0;
    int max_l = 0;
    for (int n = 0; n < N; ++n) {
        if (label_lens[n] < 0) return fail(COCR_EINVAL, "negative target length (line %d)", n);
        if (label_lens[n] > COCR_CTCL_MAX_LABELS) return fail(too_long, "line %d has %d labels; the kernel holds at most %d", n, label_lens[n], COCR_CTCL_MAX_LABELS);
        if (out_lens[n] < 0 || out_lens[n] > T) return fail(COCR_EINVAL, "input length %d outside [0, %d] (line %d)", out_lens[n], T, n);
        max_l = std::max(max_l, (int)label_lens[n]);
        total += (size_t)label_lens[n];
    }
    if (total && (!targets || !outputs_ok)) return fail(COCR_EINVAL, "null argument");
    for (size_t i = 0; i < total; ++i)
        if (targets[i] < 1 || targets[i] >= ncls) return fail(COCR_EINVAL, "target %d outside [1, %d) (blank is 0)", targets[i], ncls);
    HIP_TRY(hipSetDevice(m->device));
    const size_t ints = (size_t)3 * N + total;
    int32_t *h, *d;
    HIP_TRY(m->target_ring.stage(ints * 4, h, d));
    int32_t off = 0;
    for (int n = 0; n < N; ++n) { h[n] = out_lens[n]; h[N + n] = label_lens[n]; h[2 * N + n] = off; off += label_lens[n]; }
    if (total) memcpy(h + 3 * N, targets, total * 4);
    HIP_TRY(m->target_ring.commit(ints * 4, (hipStream_t)stream));
    const int states = 2 * max_l + 1;
    t = {d, d + N, d + 2 * N, d + 3 * N, states <= 64 ? 1 : states <= 128 ? 2 : states <= 256 ? 4 : 8};
    return COCR_OK;
}

extern "C" int cocr_ctc_loss(cocr_model *m, const float *probits, int N, int T, int ncls, const int32_t *out_lens, const int32_t *targets,
                             const int32_t *label_lens, float *nll, float *grad, void *stream) {
    if (!m || !probits || !out_lens || !label_lens || !nll) return fail(COCR_EINVAL, "null argument");
    if (N < 1 || T < 1 || ncls < 2) return fail(COCR_EINVAL, "empty problem");
    if (ncls > 16384) return fail(COCR_EUNSUPPORTED, "more than 16384 classes");
    CtcTargets t;
    const int rc = upload_targets(m, N, T, ncls, out_lens, targets, label_lens, true, COCR_EUNSUPPORTED, stream, t);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int sj = t.sj;
    const size_t need = (size_t)N * T * ((size_t)ncls + 2 * 64 * sj);
    HIP_TRY(m->loss_ws.grow(need));
    ProfScope ps(m, s, FAM_LOSS);
    launch_ctc_loss(s, sj, (size_t)ncls * 4, probits, N, T, ncls, t.lens, t.label_lens, t.label_off, t.labels, nll, grad, m->loss_ws.p, m->loss_ws.p + (size_t)N * T * ncls);
    LAUNCH_CHECK();
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ forced alignment (ctc_align.hip.h)
extern "C" int cocr_ctc_align(cocr_model *m, const float *logits, int N, int T, int ncls, const int32_t *out_lens, const int32_t *targets,
                              const int32_t *label_lens, int32_t *starts, int32_t *ends, float *conf, float *score, int32_t *counts, void *stream) {
    if (!m || !logits || !out_lens || !label_lens || !score || !counts) return fail(COCR_EINVAL, "null argument");
    if (N < 1 || T < 1 || ncls < 2) return fail(COCR_EINVAL, "empty problem");
    if (T > 8000) return fail(COCR_EUNSUPPORTED, "more than 8000 frames per line");
    CtcTargets t;
    const int rc = upload_targets(m, N, T, ncls, out_lens, targets, label_lens, starts && ends && conf, COCR_EINVAL, stream, t);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int sj = t.sj;
    // the back-pointer table: in LDS beside lz when both fit (the kernel has ~5 KB of static LDS), else one region per line of the workspace
    const size_t words = ctca_bp_words(T, sj), lds_all = ctca_lz_bytes(T) + words * 4;
    if (lds_all <= 144 * 1024) {
        auto kern = ctc_align_kernel<8, true>;
        switch (sj) { case 1: kern = ctc_align_kernel<1, true>; break; case 2: kern = ctc_align_kernel<2, true>; break; case 4: kern = ctc_align_kernel<4, true>; break; }
        // (the kernel also has ~5 KB of static LDS: the limit raised for the dynamic part stays below 160 KB - static)
        HIP_TRY(raise_lds_limit((const void *)kern, lds_all, 48 * 1024, 150 * 1024));
        launch_ctc_align<true>(s, sj, lds_all, logits, N, T, ncls, t.lens, t.label_lens, t.label_off, t.labels, starts, ends, conf, score, counts, nullptr, 0);
    } else {
        HIP_TRY(m->align_ws.grow((size_t)N * words));
        launch_ctc_align<false>(s, sj, ctca_lz_bytes(T), logits, N, T, ncls, t.lens, t.label_lens, t.label_off, t.labels, starts, ends, conf, score, counts,
                                m->align_ws.p, words);
    }
    LAUNCH_CHECK();
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ output-layer training step (train.hip.h)
extern "C" int cocr_decoder_backward(cocr_model *m, const float *grad_probits, int N, int T, float *grad_weight, float *grad_bias, float *grad_output,
                                     void *stream) {
    if (!m || !grad_probits || !grad_weight || !grad_bias) return fail(COCR_EINVAL, "null argument");
    if (!m->w->blob) return fail(COCR_ESTATE, "model not finalized");
    { const int rc = adopt_layout(m); if (rc) return rc; }
    if (N != m->lastN || T != m->lastT || !m->xn) return fail(COCR_ESTATE, "no forward of shape (%d lines, %d frames) precedes this call (last forward: %d, %d)", N, T, m->lastN, m->lastT);
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const int M = N * T, C = m->ncls, D = m->D, chunks = ceil_div(M, COCR_TR_ROWS);
    const size_t per = (size_t)C * D + C, need = per * chunks;
    HIP_TRY(m->tr_part.grow(need));
    float *part_w = m->tr_part.p, *part_b = m->tr_part.p + (size_t)chunks * C * D;
    // A padded model (set_engine_dims): the kernels work on the engine's D-wide rows (the padded columns of the encoder output and of
    // the weight are zero, so are their gradients); the caller's tensors have the model's own width rD: strided copies at the boundary.
    const int rD = m->rD;
    float *gw_dst = grad_weight, *go_dst = grad_output;
    if (m->padded) {
        const size_t need_pad = (size_t)C * D + (grad_output ? (size_t)M * D : 0);
        HIP_TRY(m->tr_pad.grow(need_pad));
        gw_dst = m->tr_pad.p;
        if (grad_output) go_dst = m->tr_pad.p + (size_t)C * D;
    }
    const dim3 grid(chunks, ceil_div(C, COCR_TR_CT));
    if (m->dtype == COCR_BF16) hipLaunchKernelGGL((decoder_wgrad_kernel<bf16_t>), grid, dim3(256), 0, s, grad_probits, (const bf16_t *)m->xn, M, C, D, part_w, part_b);
    else hipLaunchKernelGGL((decoder_wgrad_kernel<float>), grid, dim3(256), 0, s, grad_probits, (const float *)m->xn, M, C, D, part_w, part_b);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(chunk_reduce_kernel, dim3(ceil_div(C * D, 256)), dim3(256), 0, s, part_w, chunks, (size_t)C * D, gw_dst);
    hipLaunchKernelGGL(chunk_reduce_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, s, part_b, chunks, (size_t)C, grad_bias);
    LAUNCH_CHECK();
    if (grad_output) {
        if (m->dtype == COCR_BF16) hipLaunchKernelGGL((decoder_igrad_kernel<bf16_t>), dim3(ceil_div(M, 16)), dim3(256), 0, s, grad_probits, (const bf16_t *)(m->w->blob + m->w->plan.wdec), M, C, D, go_dst);
        else hipLaunchKernelGGL((decoder_igrad_kernel<float>), dim3(ceil_div(M, 16)), dim3(256), 0, s, grad_probits, (const float *)(m->w->blob + m->w->plan.wdec), M, C, D, go_dst);
        LAUNCH_CHECK();
    }
    if (m->padded) {
        HIP_TRY(hipMemcpy2DAsync(grad_weight, (size_t)rD * 4, gw_dst, (size_t)D * 4, (size_t)rD * 4, C, hipMemcpyDeviceToDevice, s));
        if (grad_output) HIP_TRY(hipMemcpy2DAsync(grad_output, (size_t)rD * 4, go_dst, (size_t)D * 4, (size_t)rD * 4, M, hipMemcpyDeviceToDevice, s));
    }
    return COCR_OK;
}

// fp32 master copy [W | b] of the output layer + zeroed moments: the state-dict tensors when this rank has them, else (weights received by
// broadcast) the blob's values
static int decoder_master_init(cocr_model *m, hipStream_t s) {
    const size_t nw = (size_t)m->ncls * m->D, nb = (size_t)m->ncls, n = nw + nb, nw_model = (size_t)m->ncls * m->rD;
    const size_t row_e = (size_t)m->D * 4, row_m = (size_t)m->rD * 4;      // engine / model row bytes of the decoder weight (equal unless padded)
    HIP_TRY(hipMalloc((void **)&m->tr_state, 3 * n * 4));
    HIP_TRY(hipMemsetAsync(m->tr_state + n, 0, 2 * n * 4, s));
    auto w = m->host.find("decoder.weight"), b = m->host.find("decoder.bias");
    if (w != m->host.end() && w->second.set && w->second.data.size() == nw_model && b != m->host.end() && b->second.set && b->second.data.size() == nb) {
        HIP_TRY(hipMemsetAsync(m->tr_state, 0, nw * 4, s));
        HIP_TRY(hipMemcpy2DAsync(m->tr_state, row_e, w->second.data.data(), row_m, row_m, m->ncls, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(m->tr_state + nw, b->second.data.data(), nb * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));                                   // pageable sources
    } else {
        if (m->dtype == COCR_BF16) hipLaunchKernelGGL((to_f32_kernel<bf16_t>), dim3(64), dim3(256), 0, s, (const bf16_t *)(m->w->blob + m->w->plan.wdec), m->tr_state, nw);
        else hipLaunchKernelGGL((to_f32_kernel<float>), dim3(64), dim3(256), 0, s, (const float *)(m->w->blob + m->w->plan.wdec), m->tr_state, nw);
        HIP_TRY(hipMemcpyAsync(m->tr_state + nw, m->w->blob + m->w->plan.bdec, nb * 4, hipMemcpyDeviceToDevice, s));
        LAUNCH_CHECK();
    }
    m->tr_step = 0;
    m->tr_kind = -1;
    return COCR_OK;
}

extern "C" int cocr_get_tensor(cocr_model *m, const char *name, float *host_out, int64_t max_elems, void *stream) {
    if (!m || !name || !host_out) return fail(COCR_EINVAL, "null argument");
    const bool is_w = !strcmp(name, "decoder.weight"), is_b = !strcmp(name, "decoder.bias");
    if (!is_w && !is_b) return fail(COCR_EINVAL, "only decoder.weight / decoder.bias are trained by this library (got '%s')", name);
    const size_t nw = (size_t)m->ncls * m->D, nb = (size_t)m->ncls, n = is_w ? (size_t)m->ncls * m->rD : nb;      // nw: the engine's (maybe padded) copy
    if ((int64_t)n > max_elems) return fail(COCR_EINVAL, "%s has %zu elements, buffer %lld", name, n, (long long)max_elems);
    auto it = m->host.find(name);
    if (m->tr_state) {
        HIP_TRY(hipSetDevice(m->device));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        if (is_w) HIP_TRY(hipMemcpy2D(host_out, (size_t)m->rD * 4, m->tr_state, (size_t)m->D * 4, (size_t)m->rD * 4, m->ncls, hipMemcpyDeviceToHost));
        else HIP_TRY(hipMemcpy(host_out, m->tr_state + nw, n * 4, hipMemcpyDeviceToHost));
        if (it != m->host.end() && it->second.data.size() == n) memcpy(it->second.data.data(), host_out, n * 4);      // a later cocr_finalize keeps the trained values
        return COCR_OK;
    }
    if (it == m->host.end() || !it->second.set || it->second.data.size() != n) return fail(COCR_ESTATE, "%s was never set on this model", name);
    memcpy(host_out, it->second.data.data(), n * 4);
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ line pre-processing (preproc.hip.h)
extern "C" int32_t cocr_preproc_width(int32_t h, int32_t w, int32_t out_h, int32_t pad) {
    if (h < 1 || w < 1 || out_h < 1 || pad < 0) return -1;
    return pre_scaled_width(h, w, out_h) + 2 * pad;
}

extern "C" int cocr_preproc_lines(cocr_model *m, const uint8_t *pixels, const int64_t *offsets, const int32_t *heights, const int32_t *widths,
                                  const int32_t *channels, int N, int out_h, int pad, int out_w, uint8_t *out, int32_t *out_widths, void *stream) {
    if (!m || !pixels || !offsets || !heights || !widths || !out || !out_widths) return fail(COCR_EINVAL, "null argument");
    if (N < 1 || out_h < 1 || pad < 0 || out_w < 1) return fail(COCR_EINVAL, "empty problem");
    std::vector<PreLine> lines((size_t)N);
    std::vector<int> tab;
    size_t tmp_bytes = 0;
    int max_h = 0, max_ow = 0;
    for (int i = 0; i < N; ++i) {
        const int h = heights[i], w = widths[i], cpp = channels ? channels[i] : 1;
        if (h < 1 || w < 1 || (cpp != 1 && cpp != 3)) return fail(COCR_EINVAL, "line %d: %d x %d pixels, %d channels", i, h, w, cpp);
        PreLine &L = lines[(size_t)i];
        L.in_off = offsets[i]; L.h = h; L.w = w; L.cpp = cpp; L.ow = pre_scaled_width(h, w, out_h);
        if (L.ow + 2 * pad > out_w) return fail(COCR_EINVAL, "size mismatch: line %d is %d px wide after scaling and padding, the batch %d", i, L.ow + 2 * pad, out_w);
        pre_coeffs(w, L.ow, tab, &L.hb, &L.hk, &L.hks);
        pre_coeffs(h, out_h, tab, &L.vb, &L.vk, &L.vks);
        L.tmp_off = (long long)tmp_bytes;
        tmp_bytes += (size_t)h * L.ow;
        out_widths[i] = L.ow + 2 * pad;
        max_h = std::max(max_h, h); max_ow = std::max(max_ow, L.ow);
    }
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t lines_b = round_up((int)(lines.size() * sizeof(PreLine)), 256), tab_b = (size_t)round_up((int)(tab.size() * 4), 256);
    const size_t need = lines_b + tab_b + tmp_bytes;
    if (need > m->pre_buf.n) HIP_TRY(hipStreamSynchronize(s));      // an earlier call on this stream may still read the old buffer
    HIP_TRY(m->pre_buf.grow(need, need + need / 4));
    PreLine *d_lines = reinterpret_cast<PreLine *>(m->pre_buf.p);
    int *d_tab = reinterpret_cast<int *>(m->pre_buf.p + lines_b);
    unsigned char *d_tmp = m->pre_buf.p + lines_b + tab_b;
    HIP_TRY(hipMemcpyAsync(d_lines, lines.data(), lines.size() * sizeof(PreLine), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                      // the host tables go out of scope; also orders reuse of pre_buf by the next call
    hipLaunchKernelGGL(preproc_h_kernel, dim3(ceil_div(max_ow, 256), max_h, N), dim3(256), 0, s, pixels, d_lines, d_tab, d_tmp);
    hipLaunchKernelGGL(preproc_v_kernel, dim3(ceil_div(out_w, 256), out_h, N), dim3(256), 0, s, d_tmp, d_lines, d_tab, out, out_h, out_w, pad);
    LAUNCH_CHECK();
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ baseline line extraction (page.hip.h)
extern "C" int cocr_extract_lines(cocr_model *m, const uint8_t *const *pages, const int32_t *page_dims, int P, const int32_t *line_page,
                                  const int32_t *line_dims, const int64_t *cols, const int32_t *verts, const int32_t *nverts, int N, int fill,
                                  uint8_t *out, const int64_t *out_offsets, void *stream) {
    if (!m || !pages || !page_dims || !line_page || !line_dims || !cols || !verts || !nverts || !out || !out_offsets)
        return fail(COCR_EINVAL, "null argument");
    if (N < 1 || P < 1) return fail(COCR_EINVAL, "empty problem: %d lines on %d pages", N, P);
    if (N > 65535) return fail(COCR_EINVAL, "%d lines in one call (at most 65535)", N);
    if (fill < 0 || fill > 255) return fail(COCR_EINVAL, "fill %d is not a byte value", fill);
    for (int p = 0; p < P; ++p) {
        const int h = page_dims[3 * p], w = page_dims[3 * p + 1], c = page_dims[3 * p + 2];
        if (!pages[p] || h < 1 || w < 1 || (c != 1 && c != 3)) return fail(COCR_EINVAL, "page %d: %d x %d pixels, %d channels", p, h, w, c);
    }
    const long long kCoord = 1ll << 24;                    // |coordinate| bound: every product of the kernels stays inside int64 / int32
    std::vector<PageLine> lines((size_t)N);
    std::vector<long long> row_start;
    std::vector<long long> cnt;
    long long ncols = 0, nthr = 0, nv = 0;
    int max_ws = 0, max_hs = 0, max_rows = 0;
    for (int i = 0; i < N; ++i) {
        PageLine &L = lines[(size_t)i];
        const int p = line_page[i], hs = line_dims[3 * i], ws = line_dims[3 * i + 1], t = line_dims[3 * i + 2], V = nverts[i];
        if (p < 0 || p >= P) return fail(COCR_EINVAL, "line %d: page %d of %d", i, p, P);
        if (hs < 1 || hs > 4096 || ws < 1 || ws > 65535 || t < 0 || t >= hs)
            return fail(COCR_EINVAL, "line %d: strip %d x %d with the baseline on row %d (limits 4096 x 65535)", i, hs, ws, t);
        if (V < 3 || V > 4096) return fail(COCR_EINVAL, "line %d: %d boundary vertices (3 .. 4096)", i, V);
        if (out_offsets[i] < 0) return fail(COCR_EINVAL, "line %d: negative output offset", i);
        const int64_t *cr = cols + 4 * ncols;
        for (int c = 0; c < ws; ++c) {
            const int64_t *q = cr + 4 * c;
            if (llabs(q[0]) > (kCoord << 16) || llabs(q[1]) > (kCoord << 16) || llabs(q[2]) > 65536 || llabs(q[3]) > 65536)
                return fail(COCR_EINVAL, "line %d: column %d frame out of range", i, c);
        }
        const int32_t *v = verts + 2 * nv;
        int ymin = v[1], ymax = v[1];
        for (int k = 0; k < V; ++k) {
            if (llabs(v[2 * k]) > kCoord || llabs(v[2 * k + 1]) > kCoord) return fail(COCR_EINVAL, "line %d: boundary vertex %d out of range", i, k);
            ymin = std::min(ymin, (int)v[2 * k + 1]); ymax = std::max(ymax, (int)v[2 * k + 1]);
        }
        const int nrows = ymax - ymin;
        if (nrows > (1 << 17)) return fail(COCR_EINVAL, "line %d: the boundary spans %d rows (at most %d)", i, nrows, 1 << 17);
        cnt.assign((size_t)nrows + 1, 0);                  // thresholds per source row: each edge straddles the rows [min y, max y)
        for (int k = 0; k < V; ++k) {
            const int ay = v[2 * k + 1], by = v[2 * ((k + 1) % V) + 1];
            if (ay == by) continue;
            ++cnt[(size_t)(std::min(ay, by) - ymin)];
            --cnt[(size_t)(std::max(ay, by) - ymin)];
        }
        L.page = pages[p]; L.ph = page_dims[3 * p]; L.pw = page_dims[3 * p + 1]; L.cpp = page_dims[3 * p + 2];
        L.out_off = out_offsets[i]; L.col_off = ncols; L.row_off = (long long)row_start.size();
        L.hs = hs; L.ws = ws; L.t = t; L.vert_off = (int)nv; L.nverts = V; L.ymin = ymin; L.nrows = nrows; L.fill = fill;
        long long run = 0;
        for (int r = 0; r <= nrows; ++r) {
            row_start.push_back(nthr);
            if (r < nrows) { run += cnt[(size_t)r]; nthr += run; }
        }
        ncols += ws; nv += V;
        max_ws = std::max(max_ws, ws); max_hs = std::max(max_hs, hs); max_rows = std::max(max_rows, nrows);
    }
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t lines_b = al(lines.size() * sizeof(PageLine)), cols_b = al((size_t)ncols * 32), verts_b = al((size_t)nv * 8),
                 rows_b = al(row_start.size() * 8), thr_b = al((size_t)std::max(nthr, 1ll) * 4);
    const size_t need = lines_b + cols_b + verts_b + rows_b + thr_b;
    if (need > m->page_buf.n) HIP_TRY(hipStreamSynchronize(s));     // an earlier call on this stream may still read the old buffer
    HIP_TRY(m->page_buf.grow(need, need + need / 4));
    unsigned char *b = m->page_buf.p;
    PageLine *d_lines = reinterpret_cast<PageLine *>(b);
    long long *d_cols = reinterpret_cast<long long *>(b + lines_b);
    int *d_verts = reinterpret_cast<int *>(b + lines_b + cols_b);
    long long *d_rows = reinterpret_cast<long long *>(b + lines_b + cols_b + verts_b);
    int *d_thr = reinterpret_cast<int *>(b + lines_b + cols_b + verts_b + rows_b);
    HIP_TRY(hipMemcpyAsync(d_lines, lines.data(), lines.size() * sizeof(PageLine), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_cols, cols, (size_t)ncols * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_verts, verts, (size_t)nv * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_rows, row_start.data(), row_start.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                      // the host tables go out of scope; also orders reuse of page_buf by the next call
    if (max_rows > 0) hipLaunchKernelGGL(page_spans_kernel, dim3(ceil_div(max_rows, 256), N), dim3(256), 0, s, d_lines, d_verts, d_rows, d_thr);
    hipLaunchKernelGGL(page_sample_kernel, dim3(ceil_div(max_ws, 256), N, ceil_div(max_hs, PAGE_ROWS_PER_THREAD)), dim3(256), 0, s,
                       d_lines, d_cols, d_rows, d_thr, out);
    LAUNCH_CHECK();
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ training augmentation
extern "C" int cocr_augment_lines(cocr_model *m, const uint8_t *in, uint8_t *out, int N, int H, int W, const int32_t *seq_lens,
                                  const int64_t *params, const int32_t *grid, int grid_cols, void *stream) {
    if (!m || !in || !out || !seq_lens || !params || !grid) return fail(COCR_EINVAL, "null argument");
    if (in == out) return fail(COCR_EINVAL, "the output must be a buffer of its own");
    if (N < 1 || N > 65535) return fail(COCR_EINVAL, "%d lines in one call (1 .. 65535)", N);
    if (H < 1 || H > 4096 || W < 1 || W > 65535) return fail(COCR_EINVAL, "batch of %d x %d px (limits 4096 x 65535)", H, W);
    const int need_cols = (W - 1) / AUG_GRID_STEP + 2;
    if (grid_cols < need_cols) return fail(COCR_EINVAL, "control grid of %d columns, a batch %d px wide needs %d", grid_cols, W, need_cols);
    for (int i = 0; i < N; ++i)
        if (seq_lens[i] < 0 || seq_lens[i] > W) return fail(COCR_EINVAL, "line %d: seq_len %d outside the batch width %d", i, seq_lens[i], W);
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(augment_kernel, dim3(ceil_div(W, AUG_TW), ceil_div(H, AUG_TH), N), dim3(256), 0, s, (const unsigned char *)in,
                       (unsigned char *)out, (const long long *)params, (const int *)grid, grid_cols, H, W);
    LAUNCH_CHECK();
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ scoring: edit-distance alignment
// Where one pair's op-code table lives: the dynamic LDS it needs when that fits the budget, else 0 (the global workspace).
static size_t score_lds_need(const cocr_model *m, int n, int mm) {
    const size_t need = score_carry_bytes(n) + score_dir_words(n, mm) * 4;
    return need <= (size_t)std::min(std::max(m->score_lds_max, 0), 64 * 1024) ? need : 0;
}

extern "C" int64_t cocr_edit_align_lds(cocr_model *m, int len_a, int len_b) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    if (len_a < 0 || len_b < 0 || len_a > SCORE_MAX_LEN || len_b > SCORE_MAX_LEN)
        return fail(COCR_EINVAL, "sequences of %d and %d symbols (0 .. %d)", len_a, len_b, SCORE_MAX_LEN);
    return (int64_t)score_lds_need(m, len_a, len_b);
}

extern "C" int cocr_edit_align(cocr_model *m, const int32_t *a, const int64_t *a_offs, const int32_t *b, const int64_t *b_offs, int P,
                               int32_t *counts, uint8_t *ops, int32_t *ops_len, void *stream) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    if (P < 0) return fail(COCR_EINVAL, "%d pairs", P);
    if (P == 0) return COCR_OK;
    if (!a_offs || !b_offs || !counts || (ops && !ops_len)) return fail(COCR_EINVAL, "null argument");
    if (a_offs[0] < 0 || b_offs[0] < 0) return fail(COCR_EINVAL, "negative offset");
    for (int p = 0; p < P; ++p) {
        const int64_t n = a_offs[p + 1] - a_offs[p], mm = b_offs[p + 1] - b_offs[p];
        if (n < 0 || mm < 0) return fail(COCR_EINVAL, "pair %d: offsets decrease", p);
        if (n > SCORE_MAX_LEN || mm > SCORE_MAX_LEN)
            return fail(COCR_EINVAL, "pair %d: sequences of %lld and %lld symbols (at most %d)", p, (long long)n, (long long)mm, SCORE_MAX_LEN);
    }
    if ((a_offs[P] > a_offs[0] && !a) || (b_offs[P] > b_offs[0] && !b)) return fail(COCR_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    // launches: three LDS classes (a short pair does not pay for a long one's table), then the pairs whose table goes to the workspace;
    // inside a launch the largest matrices first
    static const size_t CLASS_MAX[3] = {2 * 1024, 8 * 1024, 64 * 1024};
    std::vector<int> cls[4];
    size_t cls_lds[4] = {0, 0, 0, 0}, ws_words = 0;
    std::vector<int64_t> cells((size_t)P);
    for (int p = 0; p < P; ++p) {
        const int n = (int)(a_offs[p + 1] - a_offs[p]), mm = (int)(b_offs[p + 1] - b_offs[p]);
        cells[p] = (int64_t)n * mm;
        const size_t need = score_lds_need(m, n, mm);
        int c = 3;
        if (need) c = need <= CLASS_MAX[0] ? 0 : need <= CLASS_MAX[1] ? 1 : 2;
        else ws_words = std::max(ws_words, score_dir_words(n, mm));
        cls[c].push_back(p);
        cls_lds[c] = std::max(cls_lds[c], need ? need : score_carry_bytes(n));
    }
    const int ws_groups = (int)std::min<size_t>(cls[3].size(), 32);      // workgroups of the workspace launch, one region each
    if (ws_groups) HIP_TRY(m->score_ws.grow((size_t)ws_groups * ws_words));
    // the tables of this call, through the pinned ring
    const size_t offs_bytes = (size_t)(P + 1) * 8, bytes = 2 * offs_bytes + (size_t)P * 4;
    unsigned char *h, *d;
    HIP_TRY(m->score_ring.stage(bytes, h, d));
    memcpy(h, a_offs, offs_bytes);
    memcpy(h + offs_bytes, b_offs, offs_bytes);
    int *order = reinterpret_cast<int *>(h + 2 * offs_bytes);
    size_t at = 0, first[4];
    for (int c = 0; c < 4; ++c) {
        std::sort(cls[c].begin(), cls[c].end(), [&](int x, int y) { return cells[x] != cells[y] ? cells[x] > cells[y] : x < y; });
        first[c] = at;
        for (int p : cls[c]) order[at++] = p;
    }
    HIP_TRY(m->score_ring.commit(bytes, s));
    const long long *d_ao = reinterpret_cast<const long long *>(d), *d_bo = reinterpret_cast<const long long *>(d + offs_bytes);
    const int *d_order = reinterpret_cast<const int *>(d + 2 * offs_bytes);
    for (int c = 0; c < 3; ++c) {
        if (cls[c].empty()) continue;
        hipLaunchKernelGGL(edit_align_kernel<true>, dim3((unsigned)cls[c].size()), dim3(64), (cls_lds[c] + 15) & ~(size_t)15, s, a, b, d_ao, d_bo,
                           d_order + first[c], (int)cls[c].size(), counts, ops, ops_len, (unsigned *)nullptr, (size_t)0);
        LAUNCH_CHECK();
    }
    if (ws_groups) {
        hipLaunchKernelGGL(edit_align_kernel<false>, dim3(ws_groups), dim3(64), (cls_lds[3] + 15) & ~(size_t)15, s, a, b, d_ao, d_bo,
                           d_order + first[3], (int)cls[3].size(), counts, ops, ops_len, m->score_ws.p, ws_words);
        LAUNCH_CHECK();
    }
    return COCR_OK;
}

// ------------------------------------------------------------------------------------ kernel micro-benchmarks (development hook)
__global__ void fill_kernel(unsigned short *p, size_t n, unsigned seed, int as_f32) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned h = (unsigned)i * 2654435761u + seed;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        const float v = ((float)(h & 0xffff) / 65536.0f - 0.5f);
        if (as_f32) ((float *)p)[i] = v; else ((bf16_t *)p)[i] = (bf16_t)v;
    }
}

struct EpiNull {   // ablation: keeps the accumulators alive, stores (almost) nothing
    typedef float stage_t;
    static constexpr bool GLU = false;
    static constexpr bool ROWWISE = false;
    float *sink;
    __device__ __forceinline__ void transform(int n, const float *v, float *r) const { for (int i = 0; i < 4; ++i) r[i] = v[i]; }
    __device__ __forceinline__ void store(int m, int c, const float *src, int cnt) const { if (src[0] == 123.456f) sink[0] = 1.0f; }
};

// Times one GEMM variant on random operands: returns the average device time per launch in microseconds.
extern "C" int cocr_dev_bench_gemm(int variant, int M, int N, int K, int iters, double *us_out) {
    typedef bf16_t T;
    void *A = nullptr, *W = nullptr, *O = nullptr;
    float *X = nullptr, *bias = nullptr, *gam = nullptr;
    HIP_TRY(hipMalloc(&A, (size_t)M * K * 2)); HIP_TRY(hipMalloc(&W, (size_t)N * K * 2)); HIP_TRY(hipMalloc(&O, (size_t)M * N * 4));
    HIP_TRY(hipMalloc((void **)&X, (size_t)M * K * 4)); HIP_TRY(hipMalloc((void **)&bias, (size_t)N * 4)); HIP_TRY(hipMalloc((void **)&gam, (size_t)K * 4));
    hipLaunchKernelGGL(fill_kernel, dim3(1024), dim3(256), 0, 0, (unsigned short *)A, (size_t)M * K, 1u, 0);
    hipLaunchKernelGGL(fill_kernel, dim3(1024), dim3(256), 0, 0, (unsigned short *)W, (size_t)N * K, 2u, 0);
    hipLaunchKernelGGL(fill_kernel, dim3(1024), dim3(256), 0, 0, (unsigned short *)X, (size_t)M * K, 3u, 1);
    hipLaunchKernelGGL(fill_kernel, dim3(64), dim3(256), 0, 0, (unsigned short *)bias, (size_t)N, 4u, 1);
    hipLaunchKernelGGL(fill_kernel, dim3(64), dim3(256), 0, 0, (unsigned short *)gam, (size_t)K, 5u, 1);
    HIP_TRY(hipMemset(O, 0, (size_t)M * N * 4));
    GemmArgs<T> a{(const T *)A, K, (const T *)W, K, M, N, K, 0};
    EpiBiasAct<T, ACT_SILU> eh{(T *)O, N, bias, N};
    EpiResidual er{(float *)O, N, bias, 0.5f, N};
    EpiNull en{(float *)O};
    const bool resid = N <= 256;
    auto run = [&]() -> hipError_t {
#define RING(BM, BN, NST) (resid ? launch_ring_cfg<T, BM, BN, NST>(0, a, er) : launch_ring_cfg<T, BM, BN, NST>(0, a, eh))
        switch (variant) {
            case 0: return resid ? launch_gemm<T>(0, a.A, K, a.W, K, M, N, K, er) : launch_gemm<T>(0, a.A, K, a.W, K, M, N, K, eh);
            case 1: return RING(64, 64, 3);
            case 2: return RING(64, 64, 4);
            case 3: return RING(64, 128, 3);
            case 4: return RING(128, 128, 2);
            case 5: return RING(128, 128, 3);
            case 6: return RING(128, 64, 3);
            case 7: return RING(64, 128, 2);
            case 8: return RING(64, 64, 2);
            case 9: return resid ? launch_stream_cfg<T, 64, 64>(0, a, er) : launch_stream_cfg<T, 64, 64>(0, a, eh);
            case 30: return launch_ring_cfg<T, 128, 128, 2>(0, a, en);
            case 31: return launch_ring_cfg<T, 64, 64, 3>(0, a, en);
            case 40: {   // fused FFN on (M, D=256, FF=N): A = xn [M][256], W = W1 [N][256], O reused as W2 [256][N]
                EpiResidualLN<T, 1> e{X, 256, bias, 0.5f, 256, 1, gam, gam, nullptr, nullptr, (T *)A};
                return launch_ffn_fused<EpiResidualLN<T, 1>>(0, (const T *)A, (const T *)W, bias, (const T *)O, M, 256, N, e);
            }
            case 20: launch_layernorm<T>(0, X, M, K, gam, gam, nullptr, nullptr, nullptr, (T *)A); return hipGetLastError();
            case 21: launch_layernorm<T>(0, X, M, K, gam, gam, X, gam, gam, (T *)A); return hipGetLastError();
            default: return hipErrorInvalidValue;
        }
#undef RING
    };
    for (int i = 0; i < 3; ++i) HIP_TRY(run());
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, 0));
    for (int i = 0; i < iters; ++i) HIP_TRY(run());
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    *us_out = (double)ms * 1e3 / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(A); (void)hipFree(W); (void)hipFree(O); (void)hipFree(X); (void)hipFree(bias); (void)hipFree(gam);
    return COCR_OK;
}

extern "C" int cocr_set_chain_rows(cocr_model *m, int rows) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    if (rows < 0 || rows > 96) return fail(COCR_EINVAL, "rows per workgroup must be in 0..96");
    if (rows != m->chain_rows) {          // captured launch sequences use the old grid
        m->graphs.drop();
    }
    m->chain_rows = rows;
    return COCR_OK;
}

extern "C" int cocr_get_chain_rows(cocr_model *m, int N, int W, int *rows) {
    if (!m || !rows) return fail(COCR_EINVAL, "null argument");
    if (!m->w->blob) return fail(COCR_ESTATE, "model not finalized");
    if (N < 1 || W < 1) return fail(COCR_EINVAL, "empty batch");
    { const int rc = adopt_layout(m); if (rc) return rc; }
    *rows = forward_form(m, N, W).chain_rows;
    return COCR_OK;
}

extern "C" int cocr_set_graph(cocr_model *m, int on) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    m->use_graph = on != 0;
    return COCR_OK;
}

#include "train_api.hip.h"
