// What cocr_train_step (train.hip) is made of:
//     TrainW      the float offset of every tensor the step touches, resolved from the reference's state-dict names ONCE (train_resolve)
//     TrainPlan   one shape's derived dimensions, every workspace offset (activations per stage / block, scratch grouped by role) and the
//                 sizes of the three per-step arenas (train_plan)
//     Train       the context of one step: plan + model, state, stream, seed, dropout; the primitives (products, Linear forward / backward,
//                 LayerNorm, column sums, deferred finals) and above them one function per stage and direction
// The launches, their order and their arguments are those of the step before it was split: nothing here decides what a kernel computes.
#pragma once

struct TrainEntry { size_t off = 0, n = 0; bool param = false; };

constexpr size_t TRAIN_NONE = ~(size_t)0;
// A Linear / pointwise conv: float offsets of weight and bias (TRAIN_NONE: no bias) in P / G, and its slot in TrainState::Xb_off
struct TrainLin { size_t w = 0, b = TRAIN_NONE; int x = 0; };
struct TrainFfnW { size_t ln_g, ln_b; TrainLin up, down; };
struct TrainStageW { size_t dw_w, dw_b; TrainLin pw; };                  // one (depthwise, pointwise) frontend stage
struct TrainBlockW {
    TrainFfnW ffn[2];
    size_t a_ln_g, a_ln_b, ub, vb; TrainLin q, k, v, pos, out;
    size_t c_ln_g, c_ln_b, dww, bn_g, bn_b, bn_mean, bn_var; TrainLin pw1, pw2;
    size_t f_ln_g, f_ln_b;
};
struct TrainW {
    size_t w0 = 0, b0 = 0;                  // frontend conv.0
    std::vector<TrainStageW> stages;        // sampling_num - 1
    TrainLin out;                           // frontend output linear
    std::vector<TrainBlockW> blocks;
    TrainLin dec;
    int nlin = 0;                           // Linears in all: the length of TrainState::Xb_off
};

struct TrainState {
    std::map<std::string, TrainEntry> idx;    // by name: cocr_train_get / _layout, the optimizer entry points (the step reads W)
    std::vector<std::string> order;
    TrainW W;
    size_t nparam = 0, ntotal = 0;            // floats: parameters first (the optimizer's range), then buffers (BatchNorm running statistics)
    float *P = nullptr, *G = nullptr, *Mo = nullptr, *Vo = nullptr;      // Mo / Vo: the optimizer's slot 0 / slot 1 (their meaning per kind: k_optim_flat)
    long step = 0;
    int kind = -1;                            // the optimizer kind (COCR_OPT_*) of the steps taken so far; -1: none yet
    long dec_steps = 0;                       // optimizer steps the output layer took BEFORE it was adopted (cocr_train_adopt_decoder): its own step count is step + dec_steps
    DevBuf<unsigned char> ws;                 // activations + scratch of one step (TrainPlan's offsets)
    DevBuf<float> pe;                         // sinusoid rows for relative positions T-1 ... -(T-1), (2T-1, D)
    int peT = 0;
    bool matmul_bf16 = false;                 // cocr_train_set_matmul: the Linear / pointwise-conv products on bf16-rounded operands (fp32 accumulate)
    DevBuf<float> parts;                           // partial column sums of the step's deferred finals (k_colsum_final_jobs), bump-allocated per step
    size_t parts_used = 0;
    std::vector<ColsumJob> jobs;
    DevBuf<ColsumJob> jobs_dev, jobs_host{true};   // device copy + pinned staging of the job table (COCR_MAX_COLSUM_JOBS entries)
    bool no_tn = false;                            // COCR_TRAIN_NO_TN=1 (read at cocr_train_set_matmul): weight gradients on transposed copies (A/B)
    DevBuf<unsigned char> Xb;                      // 'medium': the bf16 copy of every Linear's input (rows zero-padded to the weight-gradient product's depth), written by the
    size_t Xb_used = 0;                            // forward, read by the backward as a K-major operand (gemm_tn_kernel): TrainPlan::xb_bytes exactly, bump-allocated per
    std::vector<size_t> Xb_off;                    // step; byte offset per Linear (TrainLin::x), TRAIN_NONE: none kept this step
    DevBuf<unsigned char> Wb, WTb;                 // 'medium': bf16 copies of every Linear weight (N, K) and of its transpose (K, N), written by the forward, read by the
                                              // backward (byte offset of a tensor = its float offset x 4: 16-byte aligned like the fp32 tensors)
};

// The one place that knows the reference's state-dict names of what the step reads (cocr_train_begin, after idx is filled).  Linears get their
// slots in the forward's order.
static int train_resolve(TrainState *t, int snum, int L) {
    std::string missing;
    auto off = [&](const std::string &n) -> size_t {
        const auto it = t->idx.find(n);
        if (it != t->idx.end()) return it->second.off;
        if (missing.empty()) missing = n;
        return 0;
    };
    TrainW &w = t->W;
    w = TrainW();
    auto lin = [&](const std::string &stem, bool bias = true) { TrainLin l; l.w = off(stem + ".weight"); if (bias) l.b = off(stem + ".bias"); l.x = w.nlin++; return l; };
    const std::string conv = "encoder.conv_subsample.conv.";
    w.w0 = off(conv + "0.weight"); w.b0 = off(conv + "0.bias");
    for (int i = 0, idx = 2; i + 1 < snum; ++i, idx += 3) {
        const std::string dw = conv + std::to_string(idx);
        w.stages.push_back({off(dw + ".weight"), off(dw + ".bias"), lin(conv + std::to_string(idx + 1))});
    }
    w.out = lin("encoder.conv_subsample.out.0");
    for (int l = 0; l < L; ++l) {
        const std::string blk = "encoder.layers." + std::to_string(l) + ".sequential.", att = blk + "1.module.attention.", cv = blk + "2.module.sequential.";
        auto ffn = [&](const char *which) { const std::string f = blk + which + ".module.sequential."; return TrainFfnW{off(f + "0.weight"), off(f + "0.bias"), lin(f + "1.linear"), lin(f + "4.linear")}; };
        TrainBlockW b;
        b.ffn[0] = ffn("0");
        b.a_ln_g = off(blk + "1.module.layer_norm.weight"); b.a_ln_b = off(blk + "1.module.layer_norm.bias");
        b.q = lin(att + "query_proj.linear"); b.k = lin(att + "key_proj.linear"); b.v = lin(att + "value_proj.linear"); b.pos = lin(att + "pos_proj.linear", false);
        b.ub = off(att + "u_bias"); b.vb = off(att + "v_bias"); b.out = lin(att + "out_proj.linear");
        b.c_ln_g = off(cv + "0.weight"); b.c_ln_b = off(cv + "0.bias"); b.pw1 = lin(cv + "2.conv"); b.dww = off(cv + "4.conv.weight");
        b.bn_g = off(cv + "5.weight"); b.bn_b = off(cv + "5.bias"); b.bn_mean = off(cv + "5.running_mean"); b.bn_var = off(cv + "5.running_var");
        b.pw2 = lin(cv + "7.conv");
        b.ffn[1] = ffn("3");
        b.f_ln_g = off(blk + "4.weight"); b.f_ln_b = off(blk + "4.bias");
        w.blocks.push_back(b);
    }
    w.dec = lin("decoder");
    return missing.empty() ? COCR_OK : fail(COCR_ESTATE, "missing tensor '%s'", missing.c_str());
}

// Dropout masks are a function of (seed, site, index): the site numbers, for the forward and the backward alike
enum DropSite { DROP_FF_HIDDEN = 2, DROP_FF_OUT = 3, DROP_ATTN_WEIGHTS = 4, DROP_ATTN_OUT = 5, DROP_CONV_OUT = 6 };
constexpr unsigned DROP_SITE_INPUT = 1;                                            // after the frontend's output linear
static unsigned drop_site(int l, DropSite k, int which = 0) { return (unsigned)(16 * l + k + 8 * which); }      // which: the block's first / second feed-forward module

// weight gradients are tall-K products (K = rows): split-K partial sums [splits][out x in], in the tiles of launch_gemm_splitk (launch_gemm_tn's are as large)
static int train_wg_splits(int Nc, int Kr) { const int tiles = ceil_div(Nc, SPLITK_BM) * ceil_div(Kr, SPLITK_BN); return std::max(1, std::min(32, 512 / tiles)); }
// 'medium': does this Linear run on bf16 copies (and keep its input's for the backward)?
static bool train_lin_bf16(const TrainState *t, int Nc, int Kr) { return t->matmul_bf16 && t->Wb.p && t->WTb.p && Nc % 8 == 0 && Kr % 8 == 0; }
static dim3 grid1(size_t n) { return dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192)); }

// ---- the plan of one shape -------------------------------------------------------------------------------------------------------------------
struct TrainPlan {
    int N, H, W, D, C, L, Hh, dh, ff, K, ncls, snum;      // (the model's own dimensions: the engine's may be padded)
    std::vector<int> Ts, Fs;                              // frames / height after each stride-2 frontend stage
    int T, F, M, Mp, R, Rp, Tk, Rk, Z, nclp, wide;        // Mp / Rp: row counts of split-K weight gradients (32 or 64 x <= 32 splits); Tk / Rk: whole 32-wide k-chunks
    bool attn_gemm;      // attention as batched exact-fp32 GEMMs (train_enc.hip.h) when d_head is a whole number of 32-wide k-chunks; else one wave per row
    size_t big_rows, MD;
    // Activations: written by the forward stage that owns them, read-only for the backward (except the in-place ReLU masks of the frontend)
    struct Stage { size_t z2, z3; };
    struct Ffn { size_t xn, mu, rs, h, a, out; };
    struct Lay { size_t x_in; Ffn f0; size_t xn2, mu2, rs2, q, k, v, P, attn, ctx, x2, xn3, mu3, rs3, ga, g, dwo, bnm, bnr, xhat, bny, sact, x3; Ffn f1; size_t mu5, rs5; };
    size_t X, Z1, Zt, Xout, Logits, Dlog, Nll;            // Xout: encoder output (after the last block's LayerNorm)
    std::vector<Stage> stg;
    std::vector<Lay> lay;
    // GEMM operand staging.  Written ONLY by the product primitives (gemm, lin_fwd, lin_bwd) and dead when they return: TA / TB transposed
    // operands of a weight gradient ('medium': TA = dY's bf16 rows), TW a transposed weight, BfA / BfW bf16 copies of a product's two operands,
    // Split the split-K partial sums, PadY dY with its columns padded to a multiple of 4.
    struct { size_t TA, TB, TW, BfA, BfW, Split, PadY; } op;
    // Gradients of the stream (each M x D; wide / wide2: M x max(ff, 2 D)).  Written by the STAGES, never by a primitive, except that ln_bwd
    // puts its dy * xhat product into wide2 (so no LayerNorm's input gradient may live there):
    //   b  d(block output), from the decoder / the block above          d  the stream's gradient inside a block
    //   a  a branch's output (forward: before the residual add; backward: its masked gradient; attention: dV)
    //   c  a branch's inner gradients, ending as d(LayerNorm output)     e  d(depthwise output), attention: dK
    //   wide  d(hidden) of a feed-forward / GLU input, attention: d(q + u) | d(q + v)      wide2  dX of the key / value projections
    struct { size_t a, b, c, d, e, wide, wide2; } g;
    // Attention scratch, written by the attention stages only: Dsb d(scores), DP d(positional rows), and (batched form) q + u, q + v, the
    // positional scores, the dropped weights, per-head transposes
    struct { size_t Dsb, DP, Qu, Qv, Rm, Ad, HT, TT, DRT, PmT; } at;
    // Frontend gradients, written by front_bwd only
    struct { size_t Zg, Za, Zb, Z1g; } fg;
    // Reduction scratch, each consumed by the launch right after the one that wrote it: Part chunk partial sums (colsum, BatchNorm statistics,
    // LayerNorm / frontend weight gradients when not deferred), Vec the BatchNorm sums, LinePart per-line partial sums (depthwise weight
    // gradient, d positional rows)
    struct { size_t Part, Vec, LinePart; } rd;
    // The distillation term (cocr_train_step_distill): per-frame KL values (M) and the per-line sums (N), written by the criterion alone
    struct { size_t Frame, Kd; } kd;
    size_t ws_bytes, parts_floats, xb_bytes;              // the sizes of TrainState::ws / parts / Xb for this shape
};

static TrainPlan train_plan(const cocr_model *m, const TrainState *t, int N, int H, int W) {
    TrainPlan p{};
    p.N = N; p.H = H; p.W = W; p.D = m->rD; p.C = m->C; p.L = m->L; p.Hh = m->heads; p.dh = m->rdh; p.ff = m->rff; p.K = m->ksz; p.ncls = m->ncls; p.snum = m->snum;
    const int D = p.D, C = p.C, L = p.L, Hh = p.Hh, dh = p.dh, ff = p.ff, K = p.K, ncls = p.ncls, snum = p.snum;
    p.Ts.resize(snum); p.Fs.resize(snum);
    { int tt = W, f = H; for (int i = 0; i < snum; ++i) { tt = out_len1(tt); f = out_len1(f); p.Ts[i] = tt; p.Fs[i] = f; } }
    const std::vector<int> &Ts = p.Ts, &Fs = p.Fs;
    const int T = p.T = Ts.back(), F = p.F = Fs.back(), M = p.M = N * T, Mp = p.Mp = round_up(M, 2048), R = p.R = 2 * T - 1, Rp = p.Rp = round_up(R, 2048);
    const int nclp = p.nclp = round_up(ncls, 4), Tk = p.Tk = round_up(T, 32), Rk = p.Rk = round_up(R, 32), Z = p.Z = N * Hh;
    const bool attn_gemm = p.attn_gemm = dh % 32 == 0 && !getenv("COCR_TRAIN_ATTN_NAIVE");
    const size_t MD = p.MD = (size_t)M * D;

    // ---- workspace: one bump allocation
    size_t need = 0;
    auto rsv = [&](size_t floats) { size_t o = need; need += (floats * 4 + 255) / 256 * 256; return o; };
    auto rsv_ffn = [&](TrainPlan::Ffn &f) { f.xn = rsv(MD); f.mu = rsv(M); f.rs = rsv(M); f.h = rsv((size_t)M * ff); f.a = rsv((size_t)M * ff); f.out = rsv(MD); };
    p.X = rsv((size_t)N * H * W);
    p.Z1 = rsv((size_t)N * Ts[0] * Fs[0] * C);
    p.stg.resize(snum - 1);
    for (int i = 0; i + 1 < snum; ++i) { const size_t rows = (size_t)N * Ts[i + 1] * Fs[i + 1]; p.stg[i].z2 = rsv(rows * C); p.stg[i].z3 = rsv(rows * C); }
    p.Zt = rsv((size_t)M * C * F);
    p.lay.resize(L);
    for (TrainPlan::Lay &a : p.lay) {
        a.x_in = rsv(MD); rsv_ffn(a.f0);
        a.xn2 = rsv(MD); a.mu2 = rsv(M); a.rs2 = rsv(M); a.q = rsv(MD); a.k = rsv(MD); a.v = rsv(MD); a.P = rsv((size_t)R * D);
        a.attn = rsv((size_t)N * Hh * T * (attn_gemm ? Tk : T)); a.ctx = rsv(MD); a.x2 = rsv(MD);
        a.xn3 = rsv(MD); a.mu3 = rsv(M); a.rs3 = rsv(M); a.ga = rsv(2 * MD); a.g = rsv(MD); a.dwo = rsv(MD); a.bnm = rsv(D); a.bnr = rsv(D); a.xhat = rsv(MD);
        a.bny = rsv(MD); a.sact = rsv(MD); a.x3 = rsv(MD);
        rsv_ffn(a.f1); a.mu5 = rsv(M); a.rs5 = rsv(M);
    }
    p.Xout = rsv(MD);
    p.Logits = rsv((size_t)M * ncls); p.Dlog = rsv((size_t)M * ncls); p.op.PadY = rsv((size_t)M * nclp); p.Nll = rsv(N);
    // backward scratch
    size_t big_rows = (size_t)M;
    for (int i = 0; i + 1 < snum; ++i) big_rows = std::max(big_rows, (size_t)N * Ts[i + 1] * Fs[i + 1]);
    p.big_rows = big_rows;
    const size_t big_rows_p = (big_rows + 2047) / 2048 * 2048;
    const int wide = p.wide = std::max(std::max(ff, 3 * D), std::max(C * F, std::max(2 * D, nclp)));
    const size_t tr_floats = std::max((size_t)wide * Mp, big_rows_p * (size_t)C);
    p.op.TA = rsv(tr_floats); p.op.TB = rsv(tr_floats);
    p.op.TW = rsv((size_t)std::max(std::max((size_t)ff * D, (size_t)C * F * D), (size_t)std::max(C * C, D * nclp)) + 1024);
    p.op.BfA = rsv(t->matmul_bf16 ? tr_floats / 2 + 64 : 0); p.op.BfW = rsv(t->matmul_bf16 ? tr_floats / 2 + 64 : 0);
    p.g.a = rsv(MD); p.g.b = rsv(MD); p.g.c = rsv(MD); p.g.d = rsv(MD); p.g.e = rsv(MD);
    p.g.wide = rsv((size_t)M * std::max(ff, 2 * D)); p.g.wide2 = rsv((size_t)M * std::max(ff, 2 * D));
    p.at.Dsb = rsv((size_t)N * Hh * T * (attn_gemm ? Tk : T)); p.at.DP = rsv((size_t)Rp * D);
    if (attn_gemm) {
        p.at.Qu = rsv(MD); p.at.Qv = rsv(MD); p.at.Rm = rsv((size_t)Z * T * Rk); p.at.Ad = rsv((size_t)Z * T * Tk); p.at.HT = rsv((size_t)Z * dh * Tk);
        p.at.TT = rsv((size_t)Z * T * Tk); p.at.DRT = rsv((size_t)Z * R * Tk); p.at.PmT = rsv((size_t)Hh * dh * Rk);
    }
    p.fg.Zg = rsv((size_t)M * C * F); p.fg.Za = rsv(big_rows * C); p.fg.Zb = rsv(big_rows * C); p.fg.Z1g = rsv((size_t)N * Ts[0] * Fs[0] * C);
    const size_t part_floats = std::max(std::max<size_t>(1024, (size_t)ceil_div((int)std::min<size_t>(big_rows, 1u << 30), 256)) * (size_t)std::max(wide, C * 10),
                                        (size_t)ceil_div(N * Ts[0], COCR_CV_ROWS) * 10 * (size_t)C);
    p.rd.Part = rsv(part_floats + 4096); p.rd.Vec = rsv(4 * (size_t)std::max(D, C) + 64);
    size_t split_floats = 0;
    for (auto nk : {std::pair<int, int>{ff, D}, {D, ff}, {D, D}, {2 * D, D}, {C, C}, {D, C * F}, {ncls, D}})
        split_floats = std::max(split_floats, (size_t)train_wg_splits(nk.first, nk.second) * nk.first * nk.second);
    p.op.Split = rsv(split_floats);
    p.rd.LinePart = rsv((size_t)N * std::max((size_t)R * D, (size_t)ceil_div(T, COCR_DW_WC) * D * K));
    p.kd.Frame = rsv(M); p.kd.Kd = rsv(N);
    p.ws_bytes = need;
    // deferred column-sum finals: at most 12 jobs per block + the frontend's and the decoder's, each up to ceil(M / 32) x (widest matrix) partial sums
    p.parts_floats = (size_t)(12 * L + 16) * (size_t)ceil_div(M, 32) * (size_t)std::max(wide, 2 * D) + 4096;

    // ---- 'medium': the kept bf16 inputs, exactly -- the forward's Linears in its order under lin_fwd's own rule (a Linear that reads what the
    // one before it read -- the query / key / value projections -- shares that copy)
    int kept_in = -1, kept_rows = 0, kept_k = 0, kept_rp = 0, input = 0;
    auto keep = [&](int in, int rows, int Nc, int Kr) {
        if (!train_lin_bf16(t, Nc, Kr)) return;
        const int rp = round_up(rows, 64 * train_wg_splits(Nc, Kr));
        if (in == kept_in && rows == kept_rows && Kr == kept_k && rp <= kept_rp) return;
        p.xb_bytes += ((size_t)rp * Kr * 2 + 255) / 256 * 256;
        kept_in = in; kept_rows = rows; kept_k = Kr; kept_rp = rp;
    };
    for (int i = 0; i + 1 < snum; ++i) keep(input++, N * Ts[i + 1] * Fs[i + 1], C, C);
    keep(input++, M, D, C * F);
    for (int l = 0; l < L; ++l) {
        keep(input++, M, ff, D); keep(input++, M, D, ff);                                       // feed-forward 0
        keep(input, M, D, D); keep(input, M, D, D); keep(input++, M, D, D);                     // query, key, value: one LayerNorm output
        keep(input++, R, D, D); keep(input++, M, D, D);                                         // positional rows, attention output
        keep(input++, M, 2 * D, D); keep(input++, M, D, D);                                     // conv module's two pointwise convs
        keep(input++, M, ff, D); keep(input++, M, D, ff);                                       // feed-forward 1
    }
    keep(input++, M, ncls, D);
    return p;
}

// ---- the context of one step -----------------------------------------------------------------------------------------------------------------
struct Train : TrainPlan {
    cocr_model *const m;
    TrainState *const t;
    const TrainW &w;
    const hipStream_t s;
    const unsigned long long seed;
    const float p_in, p_ff, p_at, p_cv;      // the reference's four dropout probabilities (encoder.py:144-147)
    const float ffr, scale;                  // feed-forward residual factor; 1/sqrt(d_head)
    const long long sTD, sTT, sTR, sHT, arows;
    const size_t cw_lds;                     // conv_w_block_sum: [position phases][10][C]
    // 'medium': the input of the last lin_fwd that kept a copy and where that copy lies -- a Linear reading the same input shares it
    struct { const float *x = nullptr; int rows = 0, k = 0, rp = 0; size_t xo = 0; } kept;
    float *dx = nullptr;                     // backward: the gradient of the stream entering the current point

    Train(cocr_model *m_, const TrainPlan &p, hipStream_t s_, uint64_t seed_, const float *drop)
        : TrainPlan(p), m(m_), t(m_->train), w(m_->train->W), s(s_), seed(seed_), p_in(drop[0]), p_ff(drop[1]), p_at(drop[2]), p_cv(drop[3]),
          ffr(m_->hp.half_step_residual ? 0.5f : 1.0f), scale(1.0f / sqrtf((float)p.dh)), sTD((long long)T * D), sTT((long long)T * Tk), sTR((long long)T * Rk),
          sHT((long long)dh * Tk), arows((long long)N * Hh * T), cw_lds((size_t)(256 / (C / 4)) * 10 * C * sizeof(float)) {}
    float *WS(size_t off) const { return reinterpret_cast<float *>(t->ws.p + off); }
    float *P(size_t off) const { return t->P + off; }
    float *G(size_t off) const { return t->G + off; }

    // ---- primitives
    // 'medium' matmul precision (cocr_train_set_matmul; the reference trains under torch.set_float32_matmul_precision('medium'),
    // cli/train.py:252): both operands rounded to bf16, products on the bf16 matrix cores, fp32 accumulation and output
    const bf16_t *to_bf16(const float *in, size_t off, size_t n) {
        bf16_t *dst = reinterpret_cast<bf16_t *>(t->ws.p + off);
        hipLaunchKernelGGL(k_f32_to_bf16, grid1((n + 3) / 4), dim3(256), 0, s, in, dst, (n + 3) / 4);
        return dst;
    }
    int gemm(const float *A, int lda, const float *Wt, int ldw, int Mr, int Nc, int Kr, float *out, int ldo, const float *bias) {
        EpiStoreF32 e{out, ldo, bias, Nc};
        if (t->matmul_bf16 && (lda & 7) == 0 && (ldw & 7) == 0 && (Kr & 7) == 0) {
            const bf16_t *Ab = to_bf16(A, op.BfA, (size_t)Mr * lda), *Wb = to_bf16(Wt, op.BfW, (size_t)Nc * ldw);
            GEMM_TRY(launch_gemm<bf16_t>(s, Ab, lda, Wb, ldw, Mr, Nc, Kr, e));
            return COCR_OK;
        }
        GEMM_TRY(launch_gemm<float>(s, A, lda, Wt, ldw, Mr, Nc, Kr, e));
        return COCR_OK;
    }
    void transpose(const float *in, float *out, int Rr, int Cc, int ldo) {      // out (Cc, ldo) zero-padded beyond Rr
        hipLaunchKernelGGL(k_transpose, dim3(ceil_div(Cc, 32), ceil_div(ldo, 32)), dim3(256), 0, s, in, out, Rr, Cc, ldo);
    }
    // out_z (Mr x Nc, stride ldo) = A_z (Mr x Kr) W_z (Nc x Kr)^T over the Z = N * heads (line, head) batches: offsets per (line, head)
    int bgemm(const float *A, int lda, long long azb, long long azh, const float *Wm, int ldw, long long wzb, long long wzh, int Mr, int Nc, int Kr,
              float *out, int ldo, long long ozb, long long ozh) {
        GemmArgs<float> a{A, lda, Wm, ldw, Mr, Nc, Kr, 0};
        a.z_div = Hh; a.a_zb = azb; a.a_zh = azh; a.w_zb = wzb; a.w_zh = wzh; a.o_zb = ozb; a.o_zh = ozh;
        GEMM_TRY(launch_gemm_batched_f32(s, a, out, ldo, Z));
        return COCR_OK;
    }
    // head h of an (M, D) activation as (T x dh) matrices -> [z][dh][Tk] (transposed, zero-padded)
    void head_T(const float *in, float *out) {
        hipLaunchKernelGGL(k_btranspose, dim3(ceil_div(Tk, 32), ceil_div(dh, 32), Z), dim3(256), 0, s, in, out, T, dh, (long long)D, (long long)Tk, Tk, Hh, sTD, (long long)dh, sHT,
                           0, 0.f, 0ull, 0u);
    }
    // [z][T][Tk] -> its transpose [z][T][Tk]; drop: the attention weights' dropout applied to the input
    void square_T(const float *in, float *out, bool drop, float p, unsigned site) {
        hipLaunchKernelGGL(k_btranspose, dim3(ceil_div(Tk, 32), ceil_div(T, 32), Z), dim3(256), 0, s, in, out, T, T, (long long)Tk, (long long)Tk, Tk, 1, sTT, 0ll, sTT,
                           drop ? T : 0, p, seed, site);
    }
    // Deferred finals: `part_alloc` hands out a region of this step's partial-sum arena (null: arena or job table full -> the caller does the
    // final at once), `defer_final` queues "out[n] = sum over chunks of part[chunk * stride + n]"; `flush_finals` (end of the backward pass)
    // runs them all in one launch.
    float *part_alloc(size_t n) {
        n = (n + 63) / 64 * 64;
        if (t->parts_used + n > t->parts.n || t->jobs.size() + 2 > COCR_MAX_COLSUM_JOBS) return nullptr;
        float *p0 = t->parts.p + t->parts_used;
        t->parts_used += n;
        return p0;
    }
    void defer_final(const float *part, int stride, int chunks, int Nc, float *out) {
        const int fb = t->jobs.empty() ? 0 : t->jobs.back().first_block + ceil_div(t->jobs.back().N, 64);
        t->jobs.push_back(ColsumJob{part, out, stride, chunks, Nc, fb});
    }
    int flush_finals() {
        if (t->jobs.empty()) return COCR_OK;
        const int total = t->jobs.back().first_block + ceil_div(t->jobs.back().N, 64);
        memcpy(t->jobs_host.p, t->jobs.data(), t->jobs.size() * sizeof(ColsumJob));
        HIP_TRY(hipMemcpyAsync(t->jobs_dev.p, t->jobs_host.p, t->jobs.size() * sizeof(ColsumJob), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_colsum_final_jobs, dim3(total), dim3(256), 0, s, t->jobs_dev.p, (int)t->jobs.size());
        t->jobs.clear();
        return COCR_OK;
    }
    // The final of partial sums part[chunk][Nc] at once: out[n] = sum over the chunks.  groups16 (and Nc % 4 == 0): 16 chunk groups, else 4 --
    // the order of the additions differs, so who sums what keeps its form
    void colsum_final(const float *part, int chunks, int Nc, float *out, bool groups16 = false) {
        if (groups16 && Nc % 4 == 0) hipLaunchKernelGGL(k_colsum_final4, dim3(ceil_div(Nc, 64)), dim3(256), 0, s, part, out, chunks, Nc);
        else hipLaunchKernelGGL(k_colsum_final, dim3(ceil_div(Nc, 64)), dim3(256), 0, s, part, out, chunks, Nc);
    }
    // Column sums over the Mr rows of an (Mr, Nc) source (ColsumKind, train_enc.hip.h) -- CS_ONE: a, or a .* b, -> out; CS_PAIR a | b, CS_SQ
    // a | a .* a, CS_AB a | a .* b -> out | out2.  Owns the chunk rule, the choice of the 16-byte forms (Nc % 4 == 0, aligned operands; a pair
    // form and a deferred final store 16 bytes too) and where the final runs: at once (out is read next), or -- DEFER, gradients only -- with the
    // step's other finals when the arena has room.  A pair the 16-byte forms cannot take is its two single sums, at once.
    enum { NOW = 0, DEFER = 1 };
    void colsum(ColsumKind kind, const float *a, const float *b, int Mr, int Nc, float *out, float *out2 = nullptr, int when = NOW) {
        const int rows = colsum_chunk_rows(Mr), chunks = ceil_div(Mr, rows), wide = kind == CS_ONE ? 1 : 2;
        const bool vec = Nc % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0, vec_out = (((uintptr_t)out | (uintptr_t)out2) & 15) == 0;
        if (kind != CS_ONE && !(vec && vec_out)) {
            colsum(CS_ONE, a, nullptr, Mr, Nc, out);
            colsum(CS_ONE, kind == CS_PAIR ? b : a, kind == CS_PAIR ? nullptr : kind == CS_SQ ? a : b, Mr, Nc, out2);
            return;
        }
        float *arena = (when == DEFER && vec && vec_out) ? part_alloc((size_t)chunks * wide * Nc) : nullptr, *part = arena ? arena : WS(rd.Part);
        const auto partial = !vec ? k_colsum_partial<CS_ONE, float> : kind == CS_ONE ? k_colsum_partial<CS_ONE, f32x4> : kind == CS_PAIR ? k_colsum_partial<CS_PAIR, f32x4>
                             : kind == CS_SQ ? k_colsum_partial<CS_SQ, f32x4> : k_colsum_partial<CS_AB, f32x4>;
        hipLaunchKernelGGL(partial, dim3(ceil_div(wide * Nc, vec ? 256 : 64), chunks), dim3(256), 0, s, a, b, part, Mr, Nc, rows);
        if (arena) {
            defer_final(arena, wide * Nc, chunks, Nc, out);
            if (out2) defer_final(arena + Nc, wide * Nc, chunks, Nc, out2);
        } else if (kind != CS_ONE) hipLaunchKernelGGL(k_colsum_final_2, dim3(ceil_div(2 * Nc, 64)), dim3(256), 0, s, part, out, out2, chunks, Nc);
        else colsum_final(part, chunks, Nc, out, vec && chunks > 32);
    }
    // A bias gradient whose partial sums another kernel writes on its way, a 32-row tile each (k_rows_bf16, k_transpose_bf16): where that kernel
    // puts them, their final queued -- or null (32 rows are not this height's chunk, out is not 16-byte aligned, the arena is full): `colsum` then
    float *defer_tile_sums(int rows, int Nc, float *out) {
        float *part = (colsum_chunk_rows(rows) == 32 && ((uintptr_t)out & 15) == 0) ? part_alloc((size_t)ceil_div(rows, 32) * Nc) : nullptr;
        if (part) defer_final(part, Nc, ceil_div(rows, 32), Nc, out);
        return part;
    }
    // Y (rows, Nc) = X (rows, Kr) W(Nc, Kr)^T + b
    int lin_fwd(const float *X, const TrainLin &ln, int rows, int Nc, int Kr, float *Y) {
        const float *bias = ln.b == TRAIN_NONE ? nullptr : P(ln.b);
        if (!train_lin_bf16(t, Nc, Kr)) return gemm(X, Kr, P(ln.w), Kr, rows, Nc, Kr, Y, Nc, bias);
        // 'medium': the weight's bf16 copy AND its bf16 transpose (the input-gradient product's operand) in one pass, kept for the backward
        bf16_t *Wb = reinterpret_cast<bf16_t *>(t->Wb.p + ln.w * 4), *WT = reinterpret_cast<bf16_t *>(t->WTb.p + ln.w * 4);
        hipLaunchKernelGGL(k_transpose_bf16, dim3(ceil_div(Kr, 32), ceil_div(Nc, 32)), dim3(256), 0, s, P(ln.w), WT, Wb, nullptr, Nc, Kr, Nc);
        // the input's bf16 copy is kept for the backward (K-major operand of dW = dY^T X: rows zero-padded to that product's depth)
        const int rp = round_up(rows, 64 * train_wg_splits(Nc, Kr));
        if (!(X == kept.x && rows == kept.rows && Kr == kept.k && rp <= kept.rp)) {
            const size_t xo = t->Xb_used, xbytes = ((size_t)rp * Kr * 2 + 255) / 256 * 256;
            if (xo + xbytes > xb_bytes || xo + xbytes > t->Xb.n)
                return fail(COCR_ESTATE, "training plan: the kept Linear inputs need more than the %zu bytes planned (%d x %d at %zu)", xb_bytes, rows, Kr, xo);
            t->Xb_used += xbytes;
            hipLaunchKernelGGL(k_rows_bf16, dim3(ceil_div(Kr, 256), ceil_div(rp, 32)), dim3(256), 0, s, X, reinterpret_cast<bf16_t *>(t->Xb.p + xo), nullptr, rows, Kr, rp);
            kept.x = X; kept.rows = rows; kept.k = Kr; kept.rp = rp; kept.xo = xo;
        }
        t->Xb_off[ln.x] = kept.xo;
        EpiStoreF32 e{Y, Nc, bias, Nc};
        GEMM_TRY(launch_gemm<bf16_t>(s, reinterpret_cast<const bf16_t *>(t->Xb.p + kept.xo), Kr, Wb, Kr, rows, Nc, Kr, e));
        return COCR_OK;
    }
    // 'medium' lin_bwd: dY is read ONCE in fp32 and leaves as the bf16 row-major copy both products take (k_rows_bf16: rows zero-padded to the
    // weight-gradient product's depth, the bias gradient's partial sums on the way); X's copy is the forward's; the weight gradient
    // dW = dY^T X reads both K-major (gemm_tn_kernel: no transposed copies), the input gradient takes the forward's W^T.
    int lin_bwd_bf16(const float *dY, const float *X, const TrainLin &ln, int rows, int Nc, int Kr, float *dX) {
        const int splits = train_wg_splits(Nc, Kr), rp = round_up(rows, 64 * splits);
        const bool has_b = ln.b != TRAIN_NONE;
        bf16_t *dYR = reinterpret_cast<bf16_t *>(WS(op.TA));
        const bf16_t *WT = reinterpret_cast<const bf16_t *>(t->WTb.p + ln.w * 4);          // written by lin_fwd of this step
        float *bpart = has_b ? defer_tile_sums(rows, Nc, G(ln.b)) : nullptr;
        if (t->no_tn) {
            // COCR_TRAIN_NO_TN=1 (A/B of the test): the weight-gradient product on transposed bf16 copies, as before gemm_tn_kernel existed
            bf16_t *dYT = reinterpret_cast<bf16_t *>(t->ws.p + op.BfA), *XT = reinterpret_cast<bf16_t *>(t->ws.p + op.BfW);
            hipLaunchKernelGGL(k_transpose_bf16, dim3(ceil_div(Nc, 32), ceil_div(rp, 32)), dim3(256), 0, s, dY, dYT, dX ? dYR : nullptr, bpart, rows, Nc, rp);
            hipLaunchKernelGGL(k_transpose_bf16, dim3(ceil_div(Kr, 32), ceil_div(rp, 32)), dim3(256), 0, s, X, XT, nullptr, nullptr, rows, Kr, rp);
            if (splits == 1) {
                EpiStoreF32 e{G(ln.w), Kr, nullptr, Kr};
                GEMM_TRY(launch_gemm<bf16_t>(s, dYT, rp, XT, rp, Nc, Kr, rp, e));
            } else {
                GEMM_TRY(launch_gemm_splitk<bf16_t>(s, dYT, rp, XT, rp, Nc, Kr, rp, splits, WS(op.Split)));
            }
        } else {
            if (t->Xb_off[ln.x] == TRAIN_NONE) return fail(COCR_ESTATE, "training step: the forward kept no bf16 input for Linear %d (%d x %d)", ln.x, rows, Kr);
            const bf16_t *XR = reinterpret_cast<const bf16_t *>(t->Xb.p + t->Xb_off[ln.x]);
            hipLaunchKernelGGL(k_rows_bf16, dim3(ceil_div(Nc, 256), ceil_div(rp, 32)), dim3(256), 0, s, dY, dYR, bpart, rows, Nc, rp);
            GEMM_TRY(launch_gemm_tn(s, dYR, Nc, XR, Kr, Nc, Kr, rp, splits, splits == 1 ? G(ln.w) : WS(op.Split)));
        }
        if (splits > 1) colsum_final(WS(op.Split), splits, Nc * Kr, G(ln.w));
        if (has_b && !bpart) colsum(CS_ONE, dY, nullptr, rows, Nc, G(ln.b), nullptr, DEFER);
        if (dX) {
            EpiStoreF32 e{dX, Kr, nullptr, Kr};
            GEMM_TRY(launch_gemm<bf16_t>(s, dYR, Nc, WT, Nc, rows, Kr, Nc, e));
        }
        return COCR_OK;
    }
    // dW += dY^T X, db += colsum(dY), dX = dY W   (dX null: not wanted).  dY (rows, Nc), X (rows, Kr).  Not 'medium': dX = dY (W^T)^T and
    // dW = dY^T (X^T)^T through explicit transposes
    int lin_bwd(const float *dY, const float *X, const TrainLin &ln, int rows, int Nc, int Kr, float *dX) {
        if (train_lin_bf16(t, Nc, Kr)) return lin_bwd_bf16(dY, X, ln, rows, Nc, Kr, dX);
        const int splits = train_wg_splits(Nc, Kr), rp = round_up(rows, (t->matmul_bf16 ? 64 : 32) * splits);
        int r;
        transpose(dY, WS(op.TA), rows, Nc, rp);
        transpose(X, WS(op.TB), rows, Kr, rp);
        if (splits == 1) {
            if ((r = gemm(WS(op.TA), rp, WS(op.TB), rp, Nc, Kr, rp, G(ln.w), Kr, nullptr))) return r;
        } else {
            if (t->matmul_bf16) {
                const bf16_t *Ab = to_bf16(WS(op.TA), op.BfA, (size_t)Nc * rp), *Wb = to_bf16(WS(op.TB), op.BfW, (size_t)Kr * rp);
                GEMM_TRY(launch_gemm_splitk<bf16_t>(s, Ab, rp, Wb, rp, Nc, Kr, rp, splits, WS(op.Split)));
            } else {
                GEMM_TRY(launch_gemm_splitk<float>(s, WS(op.TA), rp, WS(op.TB), rp, Nc, Kr, rp, splits, WS(op.Split)));
            }
            colsum_final(WS(op.Split), splits, Nc * Kr, G(ln.w));
        }
        if (ln.b != TRAIN_NONE) colsum(CS_ONE, dY, nullptr, rows, Nc, G(ln.b), nullptr, DEFER);
        if (dX) {
            const int np = round_up(Nc, 4);
            const float *dYp = dY;
            if (np != Nc) { hipLaunchKernelGGL(k_pad_cols, grid1((size_t)rows * np), dim3(256), 0, s, dY, WS(op.PadY), rows, Nc, np); dYp = WS(op.PadY); }
            transpose(P(ln.w), WS(op.TW), Nc, Kr, np);                      // W^T (Kr, np)
            if ((r = gemm(dYp, np, WS(op.TW), np, rows, Kr, np, dX, Kr, nullptr))) return r;
        }
        return COCR_OK;
    }
    void ln_fwd(const float *x, size_t gamma, size_t beta, float *y, float *mu, float *rs) {
        hipLaunchKernelGGL(k_ln_fwd, dim3(ceil_div(M, 4)), dim3(256), 0, s, x, P(gamma), P(beta), y, mu, rs, M, D);
    }
    // dx (+)= LayerNorm backward of dy; d gamma, d beta.  (Its dy * xhat product goes through g.wide2.)
    void ln_bwd(const float *dy, const float *x, const float *mu, const float *rs, size_t gamma, size_t beta, float *dxo, int accumulate) {
        hipLaunchKernelGGL(k_ln_bwd, dim3(ceil_div(M, 4)), dim3(256), 0, s, dy, x, mu, rs, P(gamma), dxo, WS(g.wide2), M, D, accumulate);
        colsum(CS_PAIR, WS(g.wide2), dy, M, D, G(gamma), G(beta), DEFER);
    }
    void dropout(float *x, size_t n, float p, unsigned site) {
        if (p > 0.f) hipLaunchKernelGGL(k_dropout, grid1(n), dim3(256), 0, s, x, n, p, seed, site);
    }
    int copy(float *dst, const float *src, size_t n) {
        HIP_TRY(hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, s));
        return COCR_OK;
    }
    void tfc(const float *in, float *out, int reverse) {                       // (n, t, f, c) <-> (n, t, c, f), a row per block through LDS
        const size_t lds = (size_t)F * (C + 1) * sizeof(float);
        if (lds <= 64 * 1024) hipLaunchKernelGGL(k_tfc_to_tcf, dim3(M), dim3(256), lds, s, in, out, (size_t)M, F, C, reverse);
        else hipLaunchKernelGGL(k_tfc_to_tcf_flat, grid1((size_t)M * F * C), dim3(256), 0, s, in, out, (size_t)M, F, C, reverse);
    }
    const Ffn &ffn_act(int l, int which) const { return which == 0 ? lay[l].f0 : lay[l].f1; }

    // ============================================================================================ forward (train mode)
    // lines -> conv.0 -> (depthwise, pointwise, ReLU) stages -> (n, t, (c, f)) -> output linear -> input dropout: block 0's input
    int front_fwd(const void *lines, int line_dtype) {
        int rc;
        if (line_dtype == COCR_U8) hipLaunchKernelGGL(k_u8_to_f32, grid1((size_t)N * H * W), dim3(256), 0, s, (const uint8_t *)lines, WS(X), (size_t)N * H * W);
        else if ((rc = copy(WS(X), (const float *)lines, (size_t)N * H * W))) return rc;
        hipLaunchKernelGGL(k_conv0_fwd, dim3(N * Ts[0]), dim3(256), 0, s, WS(X), P(w.w0), P(w.b0), WS(Z1), N, H, W, Ts[0], Fs[0], C);
        const float *zin = WS(Z1);
        for (int i = 0; i + 1 < snum; ++i) {
            const size_t rows = (size_t)N * Ts[i + 1] * Fs[i + 1];
            hipLaunchKernelGGL(k_dw3_fwd, dim3(N * Ts[i + 1]), dim3(256), 0, s, zin, P(w.stages[i].dw_w), P(w.stages[i].dw_b), WS(stg[i].z2), N, Ts[i], Fs[i], Ts[i + 1], Fs[i + 1], C);
            if ((rc = lin_fwd(WS(stg[i].z2), w.stages[i].pw, (int)rows, C, C, WS(stg[i].z3)))) return rc;
            hipLaunchKernelGGL(k_relu, grid1(rows * C), dim3(256), 0, s, WS(stg[i].z3), rows * C);
            zin = WS(stg[i].z3);
        }
        tfc(zin, WS(Zt), 0);
        if ((rc = lin_fwd(WS(Zt), w.out, M, D, C * F, WS(lay[0].x_in)))) return rc;
        dropout(WS(lay[0].x_in), MD, p_in, DROP_SITE_INPUT);
        return COCR_OK;
    }
    // x_out = x_in + ffr drop(W2 drop(silu(W1 LN(x_in) + b1)) + b2)
    int ffn_fwd(int l, int which) {
        const Ffn &f = ffn_act(l, which);
        const TrainFfnW &fw = w.blocks[l].ffn[which];
        const float *xin = WS(which == 0 ? lay[l].x_in : lay[l].x3);
        int r;
        ln_fwd(xin, fw.ln_g, fw.ln_b, WS(f.xn), WS(f.mu), WS(f.rs));
        if ((r = lin_fwd(WS(f.xn), fw.up, M, ff, D, WS(f.h)))) return r;
        hipLaunchKernelGGL(k_silu_fwd_drop, grid1((size_t)M * ff), dim3(256), 0, s, WS(f.h), WS(f.a), (size_t)M * ff, p_ff, seed, drop_site(l, DROP_FF_HIDDEN, which));
        if ((r = lin_fwd(WS(f.a), fw.down, M, D, ff, WS(g.a)))) return r;
        hipLaunchKernelGGL(k_add3_drop, grid1(MD), dim3(256), 0, s, WS(f.out), xin, WS(g.a), ffr, MD, p_ff, seed, drop_site(l, DROP_FF_OUT, which));
        return COCR_OK;
    }
    // x2 = x1 + drop(out_proj(attention(LN(x1))))
    int attn_fwd(int l) {
        const Lay &a = lay[l];
        const TrainBlockW &b = w.blocks[l];
        const unsigned site = drop_site(l, DROP_ATTN_WEIGHTS);
        int rc;
        ln_fwd(WS(a.f0.out), b.a_ln_g, b.a_ln_b, WS(a.xn2), WS(a.mu2), WS(a.rs2));
        if ((rc = lin_fwd(WS(a.xn2), b.q, M, D, D, WS(a.q)))) return rc;
        if ((rc = lin_fwd(WS(a.xn2), b.k, M, D, D, WS(a.k)))) return rc;
        if ((rc = lin_fwd(WS(a.xn2), b.v, M, D, D, WS(a.v)))) return rc;
        if ((rc = lin_fwd(t->pe.p, b.pos, R, D, D, WS(a.P)))) return rc;
        if (attn_gemm) {
            hipLaunchKernelGGL(k_attn_qu_qv, grid1(MD), dim3(256), 0, s, WS(a.q), P(b.ub), P(b.vb), WS(at.Qu), WS(at.Qv), MD, D);
            // S = (q + u) K^T -> attn buffer; Rm = (q + vb) P_h^T for all 2T - 1 relative positions
            if ((rc = bgemm(WS(at.Qu), D, sTD, dh, WS(a.k), D, sTD, dh, T, T, dh, WS(a.attn), Tk, (long long)Hh * sTT, sTT))) return rc;
            if ((rc = bgemm(WS(at.Qv), D, sTD, dh, WS(a.P), D, 0, dh, T, R, dh, WS(at.Rm), Rk, (long long)Hh * sTR, sTR))) return rc;
            hipLaunchKernelGGL(k_attn_softmax, dim3((unsigned)((arows + 3) / 4)), dim3(256), 0, s, WS(a.attn), WS(at.Rm), p_at > 0.f ? WS(at.Ad) : (float *)nullptr, arows, T, Tk,
                               Rk, scale, p_at, seed, site);
            head_T(WS(a.v), WS(at.HT));                                   // V^T per (line, head)
            if ((rc = bgemm(p_at > 0.f ? WS(at.Ad) : WS(a.attn), Tk, (long long)Hh * sTT, sTT, WS(at.HT), Tk, (long long)Hh * sHT, sHT, T, dh, Tk, WS(a.ctx), D, sTD, dh)))
                return rc;
        } else {
            hipLaunchKernelGGL(k_attn_fwd, dim3((unsigned)((arows + 3) / 4)), dim3(256), 4 * 2 * dh * 4, s, WS(a.q), WS(a.k), WS(a.v), WS(a.P), P(b.ub), P(b.vb), WS(a.attn),
                               WS(a.ctx), arows, T, Hh, dh, scale, p_at, seed, site);
        }
        if ((rc = lin_fwd(WS(a.ctx), b.out, M, D, D, WS(g.a)))) return rc;
        hipLaunchKernelGGL(k_add3_drop, grid1(MD), dim3(256), 0, s, WS(a.x2), WS(a.f0.out), WS(g.a), 1.0f, MD, p_at, seed, drop_site(l, DROP_ATTN_OUT));
        return COCR_OK;
    }
    // x3 = x2 + drop(pw2(silu(bn(dw(glu(pw1(LN(x2)))))))), BatchNorm on the batch's statistics (the running ones move)
    int conv_fwd(int l) {
        const Lay &a = lay[l];
        const TrainBlockW &b = w.blocks[l];
        int rc;
        ln_fwd(WS(a.x2), b.c_ln_g, b.c_ln_b, WS(a.xn3), WS(a.mu3), WS(a.rs3));
        if ((rc = lin_fwd(WS(a.xn3), b.pw1, M, 2 * D, D, WS(a.ga)))) return rc;
        hipLaunchKernelGGL(k_glu_fwd, grid1(MD), dim3(256), 0, s, WS(a.ga), WS(a.g), M, D);
        const dim3 gr(ceil_div(D, 256), ceil_div(T, COCR_DW_TC), N);
        if (K == 31) hipLaunchKernelGGL((k_dw1d_rows<false, 31>), gr, dim3(256), 0, s, WS(a.g), P(b.dww), WS(a.dwo), N, T, D, K);
        else if (K <= 32) hipLaunchKernelGGL((k_dw1d_rows<false, 0>), gr, dim3(256), 0, s, WS(a.g), P(b.dww), WS(a.dwo), N, T, D, K);
        else hipLaunchKernelGGL(k_dw1d_fwd_flat, grid1(MD), dim3(256), 0, s, WS(a.g), P(b.dww), WS(a.dwo), N, T, D, K, 0);
        colsum(CS_SQ, WS(a.dwo), nullptr, M, D, WS(rd.Vec), WS(rd.Vec) + D);      // sum x | sum x^2
        hipLaunchKernelGGL(k_bn_finalize, dim3(ceil_div(D, 256)), dim3(256), 0, s, WS(rd.Vec), WS(rd.Vec) + D, M, D, WS(a.bnm), WS(a.bnr), P(b.bn_mean), P(b.bn_var), 0.1f);
        hipLaunchKernelGGL(k_bn_apply_silu, grid1(MD), dim3(256), 0, s, WS(a.dwo), WS(a.bnm), WS(a.bnr), P(b.bn_g), P(b.bn_b), WS(a.xhat), WS(a.bny), WS(a.sact), M, D);
        if ((rc = lin_fwd(WS(a.sact), b.pw2, M, D, D, WS(g.a)))) return rc;
        hipLaunchKernelGGL(k_add3_drop, grid1(MD), dim3(256), 0, s, WS(a.x3), WS(a.x2), WS(g.a), 1.0f, MD, p_cv, seed, drop_site(l, DROP_CONV_OUT));
        return COCR_OK;
    }
    // the block-final LayerNorm (encoder.py:99) writes the next block's input, or the encoder output
    void final_ln_fwd(int l) {
        ln_fwd(WS(lay[l].f1.out), w.blocks[l].f_ln_g, w.blocks[l].f_ln_b, WS(l + 1 < L ? lay[l + 1].x_in : Xout), WS(lay[l].mu5), WS(lay[l].rs5));
    }
    // decoder, then the criterion (model.py:119,136-142): summed CTC loss (read back: the stream is drained here) and d loss / d probits.
    // teacher (DEVICE (N, T, ncls) logits, or null): the distillation term joins -- Dlog becomes
    // (1 - lambda) dCTC + lambda tau (q - p) (untouched at lambda = 0), loss_out[1] the summed KD read back with the same wait.
    int decoder_criterion(const int32_t *in_lens, const int32_t *targets, const int32_t *label_lens, const float *teacher, float tau, float lambda, float *loss_out) {
        int rc;
        if ((rc = lin_fwd(WS(Xout), w.dec, M, ncls, D, WS(Logits)))) return rc;
        LAUNCH_CHECK();
        std::vector<int32_t> out_lens(N);
        for (int i = 0; i < N; ++i) out_lens[i] = cocr_out_len(in_lens[i], m->hp.subsampling_factor);
        if ((rc = cocr_ctc_loss(m, WS(Logits), N, T, ncls, out_lens.data(), targets, label_lens, WS(Nll), WS(Dlog), (void *)s))) return rc;
        if (teacher && (rc = distill_loss_on(m, WS(Logits), teacher, N, T, ncls, out_lens.data(), tau, WS(kd.Kd), lambda > 0.f ? WS(Dlog) : nullptr, 1.0f - lambda, lambda, 1,
                                             WS(kd.Frame), s)))
            return rc;
        std::vector<float> nll(N), kdv(teacher ? N : 0);
        HIP_TRY(hipMemcpyAsync(nll.data(), WS(Nll), (size_t)N * 4, hipMemcpyDeviceToHost, s));
        if (teacher) HIP_TRY(hipMemcpyAsync(kdv.data(), WS(kd.Kd), (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        double sum = 0.0;
        for (float v : nll) sum += v;
        loss_out[0] = (float)sum;
        if (teacher) {
            sum = 0.0;
            for (float v : kdv) sum += v;
            loss_out[1] = (float)sum;
        }
        return COCR_OK;
    }

    // ============================================================================================ backward (dx: see above)
    int decoder_bwd() {
        dx = WS(g.b);
        return lin_bwd(WS(Dlog), WS(Xout), w.dec, M, ncls, D, dx);
    }
    void final_ln_bwd(int l) {
        ln_bwd(dx, WS(lay[l].f1.out), WS(lay[l].mu5), WS(lay[l].rs5), w.blocks[l].f_ln_g, w.blocks[l].f_ln_b, WS(g.d), 0);
        dx = WS(g.d);
    }
    // dx holds d x_out on entry, d x_in on exit
    int ffn_bwd(int l, int which) {
        const Ffn &f = ffn_act(l, which);
        const TrainFfnW &fw = w.blocks[l].ffn[which];
        int r;
        hipLaunchKernelGGL(k_scale_drop, grid1(MD), dim3(256), 0, s, WS(g.a), dx, ffr, MD, p_ff, seed, drop_site(l, DROP_FF_OUT, which));
        if ((r = lin_bwd(WS(g.a), WS(f.a), fw.down, M, D, ff, WS(g.wide)))) return r;
        hipLaunchKernelGGL(k_silu_bwd_drop, grid1((size_t)M * ff), dim3(256), 0, s, WS(f.h), WS(g.wide), (size_t)M * ff, p_ff, seed, drop_site(l, DROP_FF_HIDDEN, which));
        if ((r = lin_bwd(WS(g.wide), WS(f.xn), fw.up, M, ff, D, WS(g.c)))) return r;
        ln_bwd(WS(g.c), WS(which == 0 ? lay[l].x_in : lay[l].x3), WS(f.mu), WS(f.rs), fw.ln_g, fw.ln_b, dx, 1);
        return COCR_OK;
    }
    int conv_bwd(int l) {
        const Lay &a = lay[l];
        const TrainBlockW &b = w.blocks[l];
        int rc;
        hipLaunchKernelGGL(k_scale_drop, grid1(MD), dim3(256), 0, s, WS(g.a), dx, 1.0f, MD, p_cv, seed, drop_site(l, DROP_CONV_OUT));
        if ((rc = lin_bwd(WS(g.a), WS(a.sact), b.pw2, M, D, D, WS(g.c)))) return rc;
        hipLaunchKernelGGL(k_silu_bwd, grid1(MD), dim3(256), 0, s, WS(a.bny), WS(g.c), MD);               // d bn_y
        float *gbeta = G(b.bn_b), *ggamma = G(b.bn_g);
        // sum dy (= d beta) | sum dy xhat (= d gamma), straight into the gradient vector; the input gradient reads them there
        colsum(CS_AB, WS(g.c), WS(a.xhat), M, D, gbeta, ggamma);
        hipLaunchKernelGGL(k_bn_bwd, grid1(MD), dim3(256), 0, s, WS(g.c), WS(a.xhat), P(b.bn_g), WS(a.bnr), gbeta, ggamma, WS(g.e), M, D);      // d dwo
        if (K <= 32) {
            const int nch = ceil_div(T, COCR_DW_WC);
            const dim3 gw(ceil_div(D, 256), nch, N), gr(ceil_div(D, 256), ceil_div(T, COCR_DW_TC), N);
            if (K == 31) hipLaunchKernelGGL(k_dw1d_bwd_w<31>, gw, dim3(256), 0, s, WS(g.e), WS(a.g), WS(rd.LinePart), N, T, D, K);
            else hipLaunchKernelGGL(k_dw1d_bwd_w<0>, gw, dim3(256), 0, s, WS(g.e), WS(a.g), WS(rd.LinePart), N, T, D, K);
            colsum_final(WS(rd.LinePart), N * nch, D * K, G(b.dww), true);
            if (K == 31) hipLaunchKernelGGL((k_dw1d_rows<true, 31>), gr, dim3(256), 0, s, WS(g.e), P(b.dww), WS(g.c), N, T, D, K);   // d g
            else hipLaunchKernelGGL((k_dw1d_rows<true, 0>), gr, dim3(256), 0, s, WS(g.e), P(b.dww), WS(g.c), N, T, D, K);
        } else {
            hipLaunchKernelGGL(k_dw1d_bwd_w_flat, dim3(ceil_div(D, 64), K, N), dim3(64), 0, s, WS(g.e), WS(a.g), WS(rd.LinePart), N, T, D, K);
            colsum_final(WS(rd.LinePart), N, D * K, G(b.dww));
            hipLaunchKernelGGL(k_dw1d_fwd_flat, grid1(MD), dim3(256), 0, s, WS(g.e), P(b.dww), WS(g.c), N, T, D, K, 1);   // d g
        }
        hipLaunchKernelGGL(k_glu_bwd, grid1(MD), dim3(256), 0, s, WS(a.ga), WS(g.c), WS(g.wide), M, D);                  // d a (M, 2D)
        if ((rc = lin_bwd(WS(g.wide), WS(a.xn3), b.pw1, M, 2 * D, D, WS(g.c)))) return rc;
        ln_bwd(WS(g.c), WS(a.x2), WS(a.mu3), WS(a.rs3), b.c_ln_g, b.c_ln_b, dx, 1);
        return COCR_OK;
    }
    // batched form.  In: d ctx in g.c.  Out: d(q + u) -> du, d(q + vb) -> dvb, dK -> g.e, dV -> g.a, per-line d(positional rows) -> rd.LinePart
    int attn_bwd_gemm(int l, float *du, float *dvb) {
        const Lay &a = lay[l];
        const TrainBlockW &b = w.blocks[l];
        const unsigned site = drop_site(l, DROP_ATTN_WEIGHTS);
        const long long zTT = (long long)Hh * sTT, zHT = (long long)Hh * sHT;
        int rc;
        hipLaunchKernelGGL(k_attn_qu_qv, grid1(MD), dim3(256), 0, s, WS(a.q), P(b.ub), P(b.vb), WS(at.Qu), WS(at.Qv), MD, D);
        // dA = dctx V^T, then ds (in place): at.Dsb
        if ((rc = bgemm(WS(g.c), D, sTD, dh, WS(a.v), D, sTD, dh, T, T, dh, WS(at.Dsb), Tk, zTT, sTT))) return rc;
        hipLaunchKernelGGL(k_attn_softmax_bwd, dim3((unsigned)((arows + 3) / 4)), dim3(256), 0, s, WS(at.Dsb), WS(a.attn), arows, T, Tk, scale, p_at, seed, site);
        // dV = drop(attn)^T dctx -> g.a
        square_T(WS(a.attn), WS(at.TT), true, p_at, site);
        head_T(WS(g.c), WS(at.HT));
        if ((rc = bgemm(WS(at.TT), Tk, zTT, sTT, WS(at.HT), Tk, zHT, sHT, T, dh, Tk, WS(g.a), D, sTD, dh))) return rc;
        // d(q + u) = ds K
        head_T(WS(a.k), WS(at.HT));
        if ((rc = bgemm(WS(at.Dsb), Tk, zTT, sTT, WS(at.HT), Tk, zHT, sHT, T, dh, Tk, du, D, sTD, dh))) return rc;
        // dK = ds^T (q + u) -> g.e
        square_T(WS(at.Dsb), WS(at.TT), false, 0.f, 0u);
        head_T(WS(at.Qu), WS(at.HT));
        if ((rc = bgemm(WS(at.TT), Tk, zTT, sTT, WS(at.HT), Tk, zHT, sHT, T, dh, Tk, WS(g.e), D, sTD, dh))) return rc;
        // dR = shift^-1(ds) -> at.Rm;  d(q + vb) = dR P_h
        hipLaunchKernelGGL(k_attn_unshift, dim3((unsigned)((arows + 3) / 4)), dim3(256), 0, s, WS(at.Dsb), WS(at.Rm), arows, T, Tk, Rk);
        hipLaunchKernelGGL(k_btranspose, dim3(ceil_div(Rk, 32), ceil_div(dh, 32), Hh), dim3(256), 0, s, WS(a.P), WS(at.PmT), R, dh, (long long)D, (long long)Rk, Rk, Hh, 0ll,
                           (long long)dh, (long long)dh * Rk, 0, 0.f, 0ull, 0u);
        if ((rc = bgemm(WS(at.Rm), Rk, (long long)Hh * sTR, sTR, WS(at.PmT), Rk, 0, (long long)dh * Rk, T, dh, Rk, dvb, D, sTD, dh))) return rc;
        // dP_h = sum over the lines of dR^T (q + vb): per line into rd.LinePart [line][R][D], summed by the caller
        hipLaunchKernelGGL(k_btranspose, dim3(ceil_div(Tk, 32), ceil_div(R, 32), Z), dim3(256), 0, s, WS(at.Rm), WS(at.DRT), T, R, (long long)Rk, (long long)Tk, Tk, 1, sTR, 0ll,
                           (long long)R * Tk, 0, 0.f, 0ull, 0u);
        head_T(WS(at.Qv), WS(at.HT));
        return bgemm(WS(at.DRT), Tk, (long long)Hh * R * Tk, (long long)R * Tk, WS(at.HT), Tk, zHT, sHT, R, dh, Tk, WS(rd.LinePart), D, (long long)R * D, dh);
    }
    int attn_bwd(int l) {
        const Lay &a = lay[l];
        const TrainBlockW &b = w.blocks[l];
        int rc;
        hipLaunchKernelGGL(k_scale_drop, grid1(MD), dim3(256), 0, s, WS(g.a), dx, 1.0f, MD, p_at, seed, drop_site(l, DROP_ATTN_OUT));
        if ((rc = lin_bwd(WS(g.a), WS(a.ctx), b.out, M, D, D, WS(g.c)))) return rc;   // d ctx
        float *du_part = WS(g.wide), *dvb_part = WS(g.wide) + MD;
        if (attn_gemm) {
            if ((rc = attn_bwd_gemm(l, du_part, dvb_part))) return rc;
        } else {
            const unsigned site = drop_site(l, DROP_ATTN_WEIGHTS);
            hipLaunchKernelGGL(k_attn_bwd_rows, dim3((unsigned)((arows + 3) / 4)), dim3(256), 4 * dh * 4, s, WS(g.c), WS(a.k), WS(a.v), WS(a.P), WS(a.attn), WS(at.Dsb),
                               du_part, dvb_part, arows, T, Hh, dh, scale, p_at, seed, site);
            hipLaunchKernelGGL(k_attn_bwd_cols, dim3((unsigned)((arows + 3) / 4)), dim3(256), 0, s, WS(g.c), WS(a.q), P(b.ub), WS(a.attn), WS(at.Dsb), WS(g.e), WS(g.a),
                               arows, T, Hh, dh, p_at, seed, site);            // d k -> g.e, d v -> g.a
            hipLaunchKernelGGL(k_attn_bwd_pos, dim3(ceil_div(R * Hh, 4), N), dim3(256), 0, s, WS(a.q), P(b.vb), WS(at.Dsb), WS(rd.LinePart), N, T, Hh, dh);
        }
        HIP_TRY(hipMemsetAsync(WS(at.DP), 0, (size_t)Rp * D * 4, s));
        colsum_final(WS(rd.LinePart), N, R * D, WS(at.DP));
        colsum(CS_ONE, du_part, nullptr, M, D, G(b.ub), nullptr, DEFER);
        colsum(CS_ONE, dvb_part, nullptr, M, D, G(b.vb), nullptr, DEFER);
        hipLaunchKernelGGL(k_axpy, grid1(MD), dim3(256), 0, s, du_part, dvb_part, 1.0f, MD);                 // d q
        // pos_proj weight: P = PE Wpos^T  ->  d Wpos = dP^T PE
        if ((rc = lin_bwd(WS(at.DP), t->pe.p, b.pos, R, D, D, nullptr))) return rc;
        float *dxn = WS(g.c);          // (not g.wide2: the LayerNorm below needs that)
        if ((rc = lin_bwd(du_part, WS(a.xn2), b.q, M, D, D, dxn))) return rc;
        if ((rc = lin_bwd(WS(g.e), WS(a.xn2), b.k, M, D, D, WS(g.wide2)))) return rc;
        hipLaunchKernelGGL(k_axpy, grid1(MD), dim3(256), 0, s, dxn, WS(g.wide2), 1.0f, MD);
        if ((rc = lin_bwd(WS(g.a), WS(a.xn2), b.v, M, D, D, WS(g.wide2)))) return rc;
        hipLaunchKernelGGL(k_axpy, grid1(MD), dim3(256), 0, s, dxn, WS(g.wide2), 1.0f, MD);
        ln_bwd(dxn, WS(a.f0.out), WS(a.mu2), WS(a.rs2), b.a_ln_g, b.a_ln_b, dx, 1);
        return COCR_OK;
    }
    // dx is d x_in of block l = d(output of block l-1's LayerNorm): out of g.d, which the next block's backward overwrites first
    int block_done() {
        const int rc = copy(WS(g.b), dx, MD);
        dx = WS(g.b);
        return rc;
    }
    int front_bwd() {
        int rc;
        dropout(dx, MD, p_in, DROP_SITE_INPUT);
        if ((rc = lin_bwd(dx, WS(Zt), w.out, M, D, C * F, WS(fg.Zg)))) return rc;
        float *dz3 = snum == 1 ? WS(fg.Z1g) : WS(fg.Za), *dz2 = WS(fg.Zb);      // (factor 2: the flattened tensor IS conv.0's output)
        tfc(WS(fg.Zg), dz3, 1);
        for (int i = snum - 2; i >= 0; --i) {
            const size_t rows = (size_t)N * Ts[i + 1] * Fs[i + 1];
            if (i == snum - 2) hipLaunchKernelGGL(k_relu_bwd, grid1(rows * C), dim3(256), 0, s, WS(stg[i].z3), dz3, rows * C);     // (later stages: masked where it was produced)
            if ((rc = lin_bwd(dz3, WS(stg[i].z2), w.stages[i].pw, (int)rows, C, C, dz2))) return rc;
            const float *zin = i == 0 ? WS(Z1) : WS(stg[i - 1].z3);
            const int chunks = ceil_div(N * Ts[i + 1], COCR_CV_ROWS);
            hipLaunchKernelGGL(k_dw3_bwd_w, dim3(chunks), dim3(256), cw_lds, s, dz2, zin, WS(rd.Part), N, Ts[i], Fs[i], Ts[i + 1], Fs[i + 1], C);
            hipLaunchKernelGGL(k_conv_w_final, dim3(ceil_div(C * 10, 64)), dim3(256), 0, s, WS(rd.Part), chunks, C, G(w.stages[i].dw_w), G(w.stages[i].dw_b));
            // d (stage input), masked by the ReLU that produced that input (conv.0's for i == 0, the previous stage's conv.3's otherwise)
            float *dzin = i == 0 ? WS(fg.Z1g) : dz3;              // (for i > 0 the previous stage's d z3 has the shape of z3[i-1] <= big_rows x C)
            hipLaunchKernelGGL(k_dw3_bwd_in, dim3(N * Ts[i]), dim3(256), 0, s, dz2, P(w.stages[i].dw_w), dzin, zin, N, Ts[i], Fs[i], Ts[i + 1], Fs[i + 1], C);
        }
        if (snum == 1) hipLaunchKernelGGL(k_relu_bwd, grid1((size_t)N * Ts[0] * Fs[0] * C), dim3(256), 0, s, WS(Z1), WS(fg.Z1g), (size_t)N * Ts[0] * Fs[0] * C);
        const int chunks = ceil_div(N * Ts[0], COCR_CV_ROWS);
        hipLaunchKernelGGL(k_conv0_bwd_w, dim3(chunks), dim3(256), cw_lds, s, WS(fg.Z1g), WS(X), WS(rd.Part), N, H, W, Ts[0], Fs[0], C);
        hipLaunchKernelGGL(k_conv_w_final, dim3(ceil_div(C * 10, 64)), dim3(256), 0, s, WS(rd.Part), chunks, C, G(w.w0), G(w.b0));
        return COCR_OK;
    }
};
