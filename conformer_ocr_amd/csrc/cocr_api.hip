// libcocr_hip.so -- C ABI (include/cocr.h) and host orchestration of the gfx950 kernels.  This unit: the error buffer, a model's
// lifetime and layout, finalize / share / blob, the positional tables, the workspace, debug taps and the profiler; the other units
// of the host layer are listed in model.hip.h.
//
// A model is: the reference state dict (fp32, host) -> one packed device blob in the compute dtype
// (cocr_finalize) -> a workspace sized for (N, W) -> a fixed sequence of kernel launches on the
// caller's stream (cocr_forward).  Nothing here falls back to the CPU: without a GPU every compute
// entry point fails with COCR_EHIP.
#include <cstdarg>

#include "model.hip.h"
#include "gemm.hip.h"

// ------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char *cocr_last_error(void) { return g_err; }
#ifndef COCR_SRC_HASH
#define COCR_SRC_HASH "unknown"
#endif
extern "C" const char *cocr_version(void) { return "cocr-hip 0.2 (gfx950) src=" COCR_SRC_HASH; }

extern "C" int32_t cocr_out_len(int32_t in_len, int32_t subsampling_factor) {
    int n = 0;
    for (int f = subsampling_factor; f > 1; f >>= 1) ++n;
    for (int i = 0; i < n; ++i) in_len = out_len1(in_len);
    return in_len;
}

static void add_name(cocr_model *m, const std::string &n) { m->names.push_back(n); m->host[n]; }

// The COCR_* environment switches, read when a model is created.  A flag switch flips its default: '1' turns a
// default-off flag on, '0' turns a default-on one off.  A count takes the value's integer.
struct Switch { const char *name; bool Switches::*flag; int Switches::*count; };
static const Switch SWITCHES[] = {
    {"COCR_NO_PAD", &Switches::no_pad, nullptr},
    {"COCR_NO_CHAIN", &Switches::no_chain, nullptr},
    {"COCR_NO_FRONT_CHAIN", &Switches::no_front_chain, nullptr},
    {"COCR_FFN_PROBE", &Switches::ffn_probe, nullptr},
    {"COCR_ATT_TILED", &Switches::att_tiled, nullptr},
    {"COCR_ATT_RESIDENT_LONG", &Switches::att_resident_long, nullptr},
    {"COCR_CHAIN_XCD", &Switches::chain_xcd, nullptr},
    {"COCR_NO_KSKIP", &Switches::no_kskip, nullptr},
    {"COCR_NO_DW_FUSE", &Switches::no_dw_fuse, nullptr},
    {"COCR_NO_A_FUSE", &Switches::no_a_fuse, nullptr},
    {"COCR_NO_FRONT96", &Switches::no_front96, nullptr},
    {"COCR_NO_FRONT32", &Switches::no_front32, nullptr},
    {"COCR_BEAM_REF", &Switches::beam_ref, nullptr},
    {"COCR_ATT_RESIDENT_MIN", nullptr, &Switches::att_resident_min},
    {"COCR_CHAIN_ROWS", nullptr, &Switches::chain_rows},
    {"COCR_SCORE_LDS_MAX", nullptr, &Switches::score_lds_max},
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
        if (w.count) m->sw.*w.count = atoi(e);
        else m->sw.*w.flag = m->sw.*w.flag ? e[0] != '0' : e[0] == '1';
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
    for (void *p : m->ws.ws_allocs) (void)hipFree(p);
    m->ws.ws_allocs.clear();
    m->ws.capN = m->ws.capW = 0;
    m->ws.vtN = m->ws.vtT = -1;
    m->ws.lastN = m->ws.lastT = 0;                            // (the last forward's encoder output went with it)
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
    if (m->dtr.tr_state) (void)hipFree(m->dtr.tr_state);
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
    const bool pad = dtype == COCR_BF16 && !m->sw.no_pad && m->rD >= 128 && m->rD < 512 && m->rD != 256 && slot >= m->rdh && slot % 32 == 0 && slot <= 128 &&
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

// A model's compute dtype and engine dimensions (engine_dims) mirror the layout of the weights it reads; adopt_layout, through this
// function, is the only writer.
static void set_engine_dims(cocr_model *m, int dtype) {
    const EngineDims e = engine_dims(m, dtype);
    m->D = e.D; m->ff = e.ff; m->dh = e.dh; m->dhp = e.dhp; m->padded = e.padded;
    m->dtype = dtype;
}
static void forget_decoder_state(cocr_model *m) {     // the output layer's optimizer state belongs to the old weights
    if (m->dtr.tr_state) { (void)hipFree(m->dtr.tr_state); m->dtr.tr_state = nullptr; m->dtr.tr_step = 0; }
}
// Brings `m` to the layout of the set it reads; every entry point that reads the blob or sizes anything from the plan calls this first.
// Where the layouts differ -- the set was (re)finalized in another compute dtype since `m` last looked -- the model's workspace,
// captured launches, last forward and output-layer optimizer state describe the old layout and go.
int adopt_layout(cocr_model *m) {
    if (m->dtype == m->w->dtype) return COCR_OK;
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    m->graphs.drop();
    free_workspace(m);
    m->dec.amax_logits = nullptr;
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
    m->ws.ws_allocs.push_back(*p);
    return COCR_OK;
}

extern "C" int cocr_reserve(cocr_model *m, int N, int W) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    if (!m->w->blob) return fail(COCR_ESTATE, "model not finalized");
    if (N < 1 || W < 1) return fail(COCR_EINVAL, "empty batch");
    { const int rc = adopt_layout(m); if (rc) return rc; }
    if (N <= m->ws.capN && W <= m->ws.capW) return COCR_OK;
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    N = std::max(N, m->ws.capN); W = std::max(W, m->ws.capW);
    m->graphs.drop();     // captured launches point into the old workspace
    free_workspace(m);
    const size_t es = esize(m->dtype);
    int T = W;
    for (int i = 0; i < m->snum; ++i) T = out_len1(T);
    const int Tz = m->snum >= 2 ? out_len1(out_len1(W)) : out_len1(W);      // frames after the fused first two stages (factor 2: after conv.0)
    const size_t M = (size_t)N * T, Tp = round_up(T, 64);      // q / k / v rows per (line, head): whole 64-key tiles (attention.hip.h reads them unclamped)
    int rc;
    const size_t zbytes = (size_t)N * Tz * m->feats[m->snum >= 2 ? 1 : 0] * m->C * es;
    if ((rc = ws_alloc(m, &m->ws.z_a, zbytes))) return rc;
    if ((rc = ws_alloc(m, &m->ws.z_b, zbytes))) return rc;
    if ((rc = ws_alloc(m, (void **)&m->ws.x, (M + 128) * m->D * 4))) return rc;      // (+ 128 rows: the row-chain kernels keep the stream in whole row blocks of up to 96 rows)
    if ((rc = ws_alloc(m, (void **)&m->ws.x2, (M + 128) * m->D * 4))) return rc;
    if ((rc = ws_alloc(m, &m->ws.xn, M * m->D * es))) return rc;
    if ((rc = ws_alloc(m, &m->ws.hid, M * m->ff * es))) return rc;
    m->ws.qkv_bytes = (size_t)N * m->heads * Tp * m->dhp * es;
    if ((rc = ws_alloc(m, &m->ws.q, m->ws.qkv_bytes))) return rc;
    if ((rc = ws_alloc(m, &m->ws.k, m->ws.qkv_bytes))) return rc;
    if ((rc = ws_alloc(m, &m->ws.vt, m->ws.qkv_bytes))) return rc;
    if ((rc = ws_alloc(m, &m->ws.ctx, M * m->D * es))) return rc;
    if ((rc = ws_alloc(m, &m->ws.glu, M * m->D * es))) return rc;
    if ((rc = ws_alloc(m, &m->ws.dwo, M * m->D * es))) return rc;
    if ((rc = ws_alloc(m, &m->ws.g_lines, (size_t)N * m->H * W * 4))) return rc;
    if ((rc = ws_alloc(m, (void **)&m->ws.g_logits, M * m->ncls * 4))) return rc;
    m->ws.capN = N; m->ws.capW = W;
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
template <typename T> int tap(cocr_model *m, hipStream_t s, const std::string &name, const T *src, size_t n) {
    if (!m->sw.debug) return COCR_OK;
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
template int tap<float>(cocr_model *, hipStream_t, const std::string &, const float *, size_t);      // (the forward's instantiations)
template int tap<bf16_t>(cocr_model *, hipStream_t, const std::string &, const bf16_t *, size_t);
// n values of the blob at `off`, compute dtype -> fp32 (the output layer's master copy, train.hip)
void blob_to_f32(const cocr_model *m, size_t off, float *dst, size_t n, hipStream_t s) {
    if (m->dtype == COCR_BF16) hipLaunchKernelGGL((to_f32_kernel<bf16_t>), dim3(64), dim3(256), 0, s, (const bf16_t *)(m->w->blob + off), dst, n);
    else hipLaunchKernelGGL((to_f32_kernel<float>), dim3(64), dim3(256), 0, s, (const float *)(m->w->blob + off), dst, n);
}

extern "C" int cocr_set_debug(cocr_model *m, int on) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    m->sw.debug = on != 0;
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

extern "C" int cocr_debug_attention(cocr_model *m, int layer, int N, int T, const void *q, const void *k, const void *v, int64_t qkv_elems, void *ctx,
                                    int64_t ctx_elems, int32_t *dims, void *stream) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    if (!m->w->blob) return fail(COCR_ESTATE, "model not finalized");
    { const int rc = adopt_layout(m); if (rc) return rc; }
    if (layer < 0 || layer >= m->L) return fail(COCR_EINVAL, "block %d of a model with %d blocks", layer, m->L);
    if (N < 1 || T < 1) return fail(COCR_EINVAL, "empty batch");
    const int Tp = round_up(T, 64);
    if (Tp > 65536) return fail(COCR_EUNSUPPORTED, "more than 65536 output frames");
    if ((int64_t)N * m->heads > 65535) return fail(COCR_EUNSUPPORTED, "more than 65535 (line, head) pairs");
    if (dims) { dims[0] = m->heads; dims[1] = m->dh; dims[2] = m->dhp; dims[3] = Tp; }
    if (!q && !k && !v && !ctx) return dims ? COCR_OK : fail(COCR_EINVAL, "null argument");      // the layout alone
    if (!q || !k || !v || !ctx) return fail(COCR_EINVAL, "null argument");
    const int64_t want_qkv = (int64_t)N * m->heads * Tp * m->dhp, want_ctx = (int64_t)N * T * m->heads * m->dh;
    if (qkv_elems != want_qkv) return fail(COCR_EINVAL, "q, k, v hold [%d][%d][%d][%d] = %lld elements each, not %lld", N, m->heads, Tp, m->dhp, (long long)want_qkv, (long long)qkv_elems);
    if (ctx_elems != want_ctx) return fail(COCR_EINVAL, "ctx holds [%d][%d][%d] = %lld elements, not %lld", N, T, m->heads * m->dh, (long long)want_ctx, (long long)ctx_elems);
    for (const void *p : {q, k, v, (const void *)ctx})
        if ((uintptr_t)p % 16) return fail(COCR_EINVAL, "q, k, v and ctx must be 16-byte aligned");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = m->w->cover_positions(Tp)) || (rc = m->w->ensure_ptab(s))) return rc;
    return attention_core_on(m, layer, N, T, q, k, v, ctx, s);
}

extern "C" int cocr_profile(cocr_model *m, int on) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    m->sw.profile = on != 0;
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
