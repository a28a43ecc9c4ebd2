// The forward behind the C ABI (units of the host layer: model.hip.h): its form (forward_form), its stages, the weights' packed copies,
// the hipGraph replay, the entry point; the setters that change its launches.
#include "model.hip.h"
#include "attention.hip.h"
#include "conv.hip.h"
#include "gemm.hip.h"
#include "ffn.hip.h"
#include "rowchain_args.hip.h"
#include "pack.hip.h"
#include "frontend.hip.h"
#include "norm.hip.h"

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
            const size_t lds = attention_full_lds_bytes(Tk, ntw);
            auto kern = npass > 1 ? relpos_attention_full_kernel<true> : relpos_attention_full_kernel<false>;
            return launch_lds(kern, dim3(nqb, N * heads), dim3(64 * AF_WAVES), lds, s, (const bf16_t *)q, (const bf16_t *)k, (const bf16_t *)v,
                              (const bf16_t *)ptab, ub, vb, (bf16_t *)ctx, Tn, Tp, heads, scale * 1.44269504088896340736f, pos_center, ntw, Tk);
        }
    }
    const size_t lds = attention_lds_bytes<T, DHP>();
    // log2(e) rides on the 1/sqrt(d_head) factor folded into the query operands: the kernel's scores are in log2 units and its
    // softmax uses v_exp_f32 (2^x) directly -- one multiply per score less.
    // (80-query tiles -- 5 waves, 512 workgroups = one round of 2 per CU at cfg2 instead of 1280 in two rounds -- measured SLOWER:
    // 19.4 us against 16.3 us per launch)
    return launch_lds(relpos_attention_kernel<T, DHP>, dim3(ceil_div(Tn, 64), N * heads), dim3(256), lds, s, q, k, v, ptab, ub, vb, ctx, Tn, Tp, heads, dh,
                      scale * 1.44269504088896340736f, pos_center, stamps);
}

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
    if (m->sw.chain_rows > 0) return form(m->sw.chain_rows);
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
constexpr int FRONT_OUT_SPLITS = 2;
static Form forward_form(const cocr_model *m, int N, int W) {
    const bool bf16 = m->dtype == COCR_BF16, f2only = m->snum == 1;
    const int es = bf16 ? 2 : 4, D = m->D, C = m->C, H = m->H;
    const int T1 = out_len1(W), T2 = f2only ? T1 : out_len1(T1), F2 = m->feats[f2only ? 0 : 1];
    const int Kf = m->feats.back() * C, M = N * cocr_out_len(W, m->hp.subsampling_factor);
    const size_t lds32 = (size_t)(4 * 16 + 3) * ((H + 11) & ~3) * 4 + (size_t)16 * F2 * 80;      // FRONT_PW32: line tile + Z2 rows of 16 frames
    Form f{};
    f.taps = m->sw.debug;
    f.rowln = bf16 ? gemm_rowln_supported<bf16_t>(D) : gemm_rowln_supported<float>(D);
    f.chain = bf16 && rowchain_supported(D, m->ff, m->dh) && !m->sw.no_chain;
    if (bf16 && m->snum == 2 && frontend96_supported(C, m->feats[0], m->feats[1], H) && !m->sw.no_front96) f.front = FRONT_96;
    else if (f2only) f.front = FRONT_CONV0;
    else if (bf16 && C == 32 && F2 <= 32 && lds32 <= 160 * 1024 && !f.taps && !m->sw.no_front32) f.front = FRONT_PW32;
    else f.front = bf16 && C % 64 == 0 ? FRONT_MFMA : FRONT_VALU;
    if (f.chain && Kf % 256 == 0 && !m->sw.no_front_chain) f.out = OUT_IN_CHAIN;
    else if (f.rowln && Kf % (FRONT_OUT_SPLITS * (128 / es)) == 0 && D <= 256 && (size_t)FRONT_OUT_SPLITS * M * D * 4 <= (size_t)N * T2 * F2 * C * es)
        f.out = OUT_SPLITK;     // (the parts fit the idle frontend buffer)
    else f.out = OUT_GEMM;
    f.ffn_fused = bf16 && f.rowln && ffn_fused_supported<int>(D, m->ff);
    f.dw_fused = m->ksz == 31 && (!m->sw.no_dw_fuse || f.taps);
    f.argmax = m->ncls <= 128 && D % (128 / es) == 0;       // (whole k-steps of the decoder product)
    f.chain_rows = f.chain ? chain_rows_for(m, M) : 0;
    f.a_fused = f.chain && f.dw_fused && !m->sw.no_a_fuse && rowchain_head_supported(D, m->ksz, f.chain_rows);
    return f;
}

// ------------------------------------------------------------------------------------ forward
// the attention scores' 1/sqrt(d_head): of the model's own d_head (a padded model's engine d_head is its 64-wide slot)
static float attention_scale(const cocr_model *m) { return 1.0f / sqrtf((float)m->rdh); }

// What every stage of one forward reads: the model, its form, the stream, the plan, the dimensions and the workspace
template <typename T> struct Fwd {
    cocr_model *m;
    const Form &f;
    hipStream_t s;
    const BlobPlan &P;
    const int N, W, D, T1, T2, F1, F2, Tn, M, Tp;        // T1 / F1, T2 / F2: frames / height after the first, second stride-2 stage
    const float ffr;            // feed-forward residual factor
    T *const za, *const zb;     // frontend: each stage's output in zb, its intermediate in za
    float *const x;             // the fp32 residual stream
    T *const xn, *const hid, *const q, *const k, *const v, *const ctx, *const glu, *const dwo;
    Fwd(cocr_model *m_, const Form &f_, int N_, int W_, hipStream_t s_)
        : m(m_), f(f_), s(s_), P(m_->w->plan), N(N_), W(W_), D(m_->D), T1(out_len1(W_)), T2(m_->snum == 1 ? T1 : out_len1(T1)), F1(m_->feats[0]),
          F2(m_->feats[m_->snum == 1 ? 0 : 1]), Tn(cocr_out_len(W_, m_->hp.subsampling_factor)), M(N_ * Tn), Tp(round_up(Tn, 64)),
          ffr(m_->hp.half_step_residual ? 0.5f : 1.0f), za((T *)m_->ws.z_a), zb((T *)m_->ws.z_b), x(m_->ws.x),
          xn((T *)m_->ws.xn), hid((T *)m_->ws.hid), q((T *)m_->ws.q), k((T *)m_->ws.k), v((T *)m_->ws.vt), ctx((T *)m_->ws.ctx), glu((T *)m_->ws.glu), dwo((T *)m_->ws.dwo) {}
    const float *F32(size_t off) const { return (const float *)(m->w->blob + off); }
    const float *F32_opt(long off) const { return off >= 0 ? F32((size_t)off) : nullptr; }      // (an optional second LayerNorm's parameters: -1 without)
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
        const size_t n = m->ws.qkv_bytes / sizeof(T);
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
        GEMM_TRY(launch_lds(frontend_conv12pw32_kernel<TIn>, dim3(ceil_div(T2, 16), N), dim3(256), lds, s, lines, H, W, T1, F1, T2, F2, c.F32(P.w0), c.F32(P.b0),
                            c.F32(P.stages[0].dw_w), c.F32(P.stages[0].dw_b), (const bf16_t *)c.WT(P.stages[0].pw_w), c.F32(P.stages[0].pw_b), (bf16_t *)zb));
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
    launch_layernorm<T>(c.s, c.x, c.M, c.D, c.m->rD, c.F32(g1), c.F32(b1), write_f32 ? c.x : nullptr, c.F32_opt(g2), c.F32_opt(b2), c.xn);
    LAUNCH_CHECK();
    return COCR_OK;
}

// The row-complete epilogue of a product into the stream (Form::rowln): x <- [x +] alpha (acc + bias), then the LayerNorm(s) that follow in the
// reference, over the model's own width (layernorm)
template <typename T> static EpiResidualLN<T> stream_ln_epi(const Fwd<T> &c, size_t bias, float alpha, bool resid, size_t g1, size_t b1, long g2, long b2) {
    return {c.x, c.D, c.F32(bias), alpha, c.D, resid ? 1 : 0, c.F32(g1), c.F32(b1), c.F32_opt(g2), c.F32_opt(b2), c.xn, c.m->rD};
}

// x <- [x +] alpha (A W^T + bias); then the LayerNorm(s) that follow in the reference (layernorm)
template <typename T> static int gemm_to_stream(const Fwd<T> &c, int fam, const T *A, int K, size_t w, size_t bias, float alpha, bool resid,
                                                size_t g1, size_t b1, long g2, long b2) {
    const int M = c.M, D = c.D;
    {
        ProfScope ps(c.m, c.s, fam);
        if (c.f.rowln) {
            GEMM_TRY(launch_gemm_rowln<T>(c.s, A, K, c.WT(w), K, M, D, K, stream_ln_epi(c, bias, alpha, resid, g1, b1, g2, b2)));
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
        { ProfScope ps(m, c.s, FAM_FOUT); GEMM_TRY(launch_gemm_splitk<T>(c.s, c.zb, Kf, c.WT(P.wout), Kf, M, D, Kf, FRONT_OUT_SPLITS, partial)); }
        ProfScope ps(m, c.s, FAM_LN);
        hipLaunchKernelGGL((splitk_reduce_ln_kernel<T>), dim3(ceil_div(M, 16)), dim3(256), 0, c.s, partial, FRONT_OUT_SPLITS, (size_t)M * D, c.F32(P.bout), M, D,
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
            GEMM_TRY(launch_ffn_fused(c.s, (const bf16_t *)c.xn, (const bf16_t *)c.WT(fw.w1), c.F32(fw.b1), (const bf16_t *)c.WT(fw.w2), c.M, c.D, c.m->ff,
                                      stream_ln_epi(c, fw.b2, c.ffr, true, g1, b1, g2, b2)));
            return COCR_OK;
        }
    }
    const int rc = ffn_up(c, fw);
    return rc ? rc : gemm_to_stream(c, FAM_FFN_DOWN, c.hid, c.m->ff, fw.w2, fw.b2, c.ffr, true, g1, b1, g2, b2);
}

// block l's attention core on the given operands: the launch of a forward and of cocr_debug_attention (launch_attention chooses the kernel
// from the head geometry, the batch shape and the switches)
template <typename T, int DHP> static hipError_t attention_dhp(const cocr_model *m, hipStream_t s, int l, int N, const T *q, const T *k, const T *v, T *ctx, int Tn,
                                                               int Tp, unsigned long long *stamps) {
    const LayerW &w = m->w->plan.layers[l];
    return launch_attention<T, DHP>(s, N, q, k, v, (const T *)(m->w->ptab + (size_t)l * m->w->ptab_stride), (const float *)(m->w->blob + w.ub),
                                    (const float *)(m->w->blob + w.vb), ctx, Tn, Tp, m->heads, m->dh, attention_scale(m), m->w->pos_maxlen - 1, stamps,
                                    m->sw.att_tiled, m->sw.att_resident_min, m->sw.att_resident_long);
}
template <typename T> static hipError_t attention_on(const cocr_model *m, hipStream_t s, int l, int N, const T *q, const T *k, const T *v, T *ctx, int Tn, int Tp,
                                                     unsigned long long *stamps) {
    const int dhp = m->dhp;
    return dhp == 32   ? attention_dhp<T, 32>(m, s, l, N, q, k, v, ctx, Tn, Tp, stamps)
           : dhp == 64 ? attention_dhp<T, 64>(m, s, l, N, q, k, v, ctx, Tn, Tp, stamps)
           : dhp == 96 ? attention_dhp<T, 96>(m, s, l, N, q, k, v, ctx, Tn, Tp, stamps)
                       : attention_dhp<T, 128>(m, s, l, N, q, k, v, ctx, Tn, Tp, stamps);
}
template <typename T> static int attention(const Fwd<T> &c, int l, unsigned long long *stamps) {
    ProfScope ps(c.m, c.s, FAM_ATTN);
    GEMM_TRY(attention_on<T>(c.m, c.s, l, c.N, c.q, c.k, c.v, c.ctx, c.Tn, c.Tp, stamps));
    return COCR_OK;
}
// cocr_debug_attention (cocr_api.hip): that launch alone, on the caller's device tensors in the model's compute type
int attention_core_on(cocr_model *m, int l, int N, int Tn, const void *q, const void *k, const void *v, void *ctx, hipStream_t s) {
    const int Tp = round_up(Tn, 64);
    if (m->dtype == COCR_BF16) GEMM_TRY(attention_on<bf16_t>(m, s, l, N, (const bf16_t *)q, (const bf16_t *)k, (const bf16_t *)v, (bf16_t *)ctx, Tn, Tp, nullptr));
    else GEMM_TRY(attention_on<float>(m, s, l, N, (const float *)q, (const float *)k, (const float *)v, (float *)ctx, Tn, Tp, nullptr));
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
        ChainArgs a{}; a.x = c.x; a.x_in_blocked = 1; a.x_out_blocked = 1; a.xn = (bf16_t *)c.xn; a.M = M; a.dh = m->dh; a.dhp = m->dhp; a.heads = m->heads; a.T_ = c.Tn; a.Tp = c.Tp; a.inv_d = 1.0f / (float)m->rD; a.xcd_order = m->sw.chain_xcd ? 1 : 0;
        a.kd = (m->padded && !m->sw.no_kskip) ? ceil_div(m->rD, 32) : 8; a.kl = (m->padded && !m->sw.no_kskip) ? ((m->rff - 1) % 256) / 32 + 1 : 8;
        a.A0 = (const bf16_t *)A0; a.nstages = nstages; return a; };
    auto st_rowln = [&](size_t wgt, size_t bias, float alpha, size_t g1, size_t b1) {
        ChainStage st{}; st.kind = ST_ROWLN; st.W = CW(wgt); st.bias = c.F32(bias); st.N = D; st.alpha = alpha;
        st.g1 = c.F32(g1); st.b1 = c.F32(b1); return st; };
    auto st_ffn = [&](const FfnW &fw, size_t g1, size_t b1, long g2, long b2) {
        ChainStage st{}; st.kind = ST_FFN; st.W = CW(fw.w1); st.W2 = CW(fw.w2); st.bias = c.F32(fw.b1); st.bias2 = c.F32(fw.b2);
        st.N = m->ff; st.alpha = c.ffr; st.g1 = c.F32(g1); st.b1 = c.F32(b1);      // (W2's fragment-major copy is pre-scaled by ffr: ensure_packed)
        st.g2 = c.F32_opt(g2); st.b2 = c.F32_opt(b2); return st; };
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
    if (m->sw.ffn_probe) {
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
            a.xh = (l & 1) ? m->ws.x2 : c.x; a.x = (l & 1) ? c.x : m->ws.x2;
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
        EpiLogitsArgmax e{logits, m->ncls, c.F32(c.P.bdec), m->ncls, m->dec.ctc_lab.p, m->dec.ctc_val.p};
        GemmArgs<T> a{c.xn, D, c.WT(c.P.wdec), D, M, m->ncls, D, 0};
        GEMM_TRY((launch_ring_cfg<T, 64, 128, 3, EpiLogitsArgmax>(c.s, a, e)));
        m->dec.amax_ok = true; m->dec.amax_rows = M;
        return COCR_OK;
    }
    EpiStoreF32 e{logits, m->ncls, c.F32(c.P.bdec), m->ncls};
    GEMM_TRY(launch_gemm<T>(c.s, c.xn, D, c.WT(c.P.wdec), D, M, m->ncls, D, e));
    m->dec.amax_ok = false;
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
    if (m->ws.vtN != N || m->ws.vtT != c.Tn) {   // pad dims of q, k, v must read as zero for this shape
        for (T *p : {c.q, c.k, c.v}) HIP_TRY(hipMemsetAsync(p, 0, m->ws.qkv_bytes, s));
        m->ws.vtN = N; m->ws.vtT = c.Tn;
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
    const GraphCache::Action act = m->graphs.next(call, m->ws.vtN == N && m->ws.vtT == Tn, &exec);
    if (act == GraphCache::PLAIN) return run_forward(m, form, lines, line_dtype, N, W, logits, s);
    const bool staged = act == GraphCache::STAGED_REPLAY || act == GraphCache::STAGED_CAPTURE;
    if (act == GraphCache::CAPTURE || act == GraphCache::STAGED_CAPTURE) {
        hipGraph_t graph = nullptr;
        HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int r = run_forward(m, form, staged ? m->ws.g_lines : lines, line_dtype, N, W, staged ? m->ws.g_logits : logits, s);
        const hipError_t ce = hipStreamEndCapture(s, &graph);
        if (r) { if (graph) (void)hipGraphDestroy(graph); return r; }
        if (ce != hipSuccess) return fail(COCR_EHIP, "hipStreamEndCapture failed: %s", hipGetErrorString(ce));
        HIP_TRY(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        (void)hipGraphDestroy(graph);
        m->graphs.add(staged ? GraphCache::staged(call) : call, exec);
    }
    if (staged) HIP_TRY(hipMemcpyAsync(m->ws.g_lines, lines, (size_t)N * m->H * W * (line_dtype == COCR_F32 ? 4 : 1), hipMemcpyDefault, s));
    HIP_TRY(hipGraphLaunch(exec, s));
    if (staged) HIP_TRY(hipMemcpyAsync(logits, m->ws.g_logits, (size_t)N * Tn * m->ncls * 4, hipMemcpyDeviceToDevice, s));
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
    m->ws.lastN = N;
    m->ws.lastT = Tn;
    if (!m->sw.use_graph || m->sw.debug || m->sw.profile || s == nullptr) return run_forward(m, form, lines, line_dtype, N, W, logits, s);
    return forward_graphed(m, form, lines, line_dtype, N, W, logits, s);
}

extern "C" int cocr_forward(cocr_model *m, const void *lines, int line_dtype, int N, int H, int W, const int32_t *in_lens,
                            float *logits, int32_t *out_lens, void *stream) {
    if (m) m->dec.amax_logits = nullptr;
    const int rc = forward_entry(m, lines, line_dtype, N, H, W, in_lens, logits, out_lens, stream);
    if (rc == COCR_OK && m->dec.amax_ok) m->dec.amax_logits = logits;      // (plain run, replay or staged replay: the sequence ended with the argmax epilogue)
    return rc;
}
extern "C" int cocr_forget_argmax(cocr_model *m) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    m->dec.amax_logits = nullptr;
    return COCR_OK;
}

extern "C" int cocr_set_chain_rows(cocr_model *m, int rows) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    if (rows < 0 || rows > 96) return fail(COCR_EINVAL, "rows per workgroup must be in 0..96");
    if (rows != m->sw.chain_rows) {          // captured launch sequences use the old grid
        m->graphs.drop();
    }
    m->sw.chain_rows = rows;
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
    m->sw.use_graph = on != 0;
    return COCR_OK;
}
