// Training behind the C ABI: the output layer alone (cocr_decoder_*), and the training step of the whole network:
//     cocr_train_begin      fp32 master copy of every parameter / buffer (reference state-dict names) on the device, zeroed AdamW state
//     cocr_train_step       RecognitionModel.training_step (model.py:129-152): train-mode forward (batch-statistics BatchNorm, dropout at the
//                           reference's six sites), CTC criterion, backward through decoder AND encoder -> the gradient of every parameter
//     cocr_train_step_distill    the same step with a teacher's logits: (1 - weight) CTC + weight KD (distill.hip.h)
//     cocr_train_adamw      torch.optim.AdamW over all parameters (model.py:283-284)
//     cocr_train_optim_step      one step of AdamW / Adam / SGD / RMSprop over all parameters (model.py:283-289); cocr_decoder_optim_step: on the output layer
//     cocr_train_adopt_decoder   the output layer a frozen-backbone phase trained (cocr_decoder_adamw / _optim_step), with its optimizer state, into this state
//     cocr_train_optim_state / _restore, cocr_decoder_optim_state / _restore   the optimizer state out of and back into the library (resuming a fit)
//     cocr_train_get        a parameter / buffer / gradient by name (checkpointing, tests)
//     cocr_train_end        the trained values back into the model's state (re-finalize to serve them)
// This file holds the entry points and the optimizer plumbing; the step's state, its per-shape plan, its primitives and its stages are
// train_step.hip.h.  fp32 master weights, activations and gradients, correctness-first (train_enc.hip.h).  Every matrix product is an MFMA GEMM
// of gemm.hip.h, in one of two precisions (cocr_train_set_matmul):
//     'highest'  exact fp32: Y = X W^T directly, dX = dY (W^T)^T and dW = dY^T (X^T)^T through explicit fp32 transposes
//     'medium'   bf16-rounded operands, fp32 accumulation: the forward keeps a bf16 copy of every Linear's input, weight and transposed weight;
//                dW = dY^T X reads dY and X K-major (gemm_tn_kernel, no transposed copies), dX = dY W takes the kept W^T
// The inference path (bf16 row chains, fused frontend) is not touched: training keeps its own activations (everything the backward needs is
// stored; nothing is recomputed except dropout masks, which are regenerated from (seed, site, index)).
#include <mutex>

#include "model.hip.h"
#include "gemm.hip.h"
#include "train.hip.h"
#include "train_enc.hip.h"
#include "train_optim.hip.h"
#include "train_step.hip.h"

// ------------------------------------------------------------------------------------ output-layer training step (train.hip.h)
extern "C" int cocr_decoder_backward(cocr_model *m, const float *grad_probits, int N, int T, float *grad_weight, float *grad_bias, float *grad_output,
                                     void *stream) {
    if (!m || !grad_probits || !grad_weight || !grad_bias) return fail(COCR_EINVAL, "null argument");
    if (!m->w->blob) return fail(COCR_ESTATE, "model not finalized");
    { const int rc = adopt_layout(m); if (rc) return rc; }
    if (N != m->ws.lastN || T != m->ws.lastT || !m->ws.xn) return fail(COCR_ESTATE, "no forward of shape (%d lines, %d frames) precedes this call (last forward: %d, %d)", N, T, m->ws.lastN, m->ws.lastT);
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const int M = N * T, C = m->ncls, D = m->D, chunks = ceil_div(M, COCR_TR_ROWS);
    const size_t per = (size_t)C * D + C, need = per * chunks;
    HIP_TRY(m->dtr.tr_part.grow(need));
    float *part_w = m->dtr.tr_part.p, *part_b = m->dtr.tr_part.p + (size_t)chunks * C * D;
    // A padded model (set_engine_dims): the kernels work on the engine's D-wide rows (the padded columns of the encoder output and of
    // the weight are zero, so are their gradients); the caller's tensors have the model's own width rD: strided copies at the boundary.
    const int rD = m->rD;
    float *gw_dst = grad_weight, *go_dst = grad_output;
    if (m->padded) {
        const size_t need_pad = (size_t)C * D + (grad_output ? (size_t)M * D : 0);
        HIP_TRY(m->dtr.tr_pad.grow(need_pad));
        gw_dst = m->dtr.tr_pad.p;
        if (grad_output) go_dst = m->dtr.tr_pad.p + (size_t)C * D;
    }
    const dim3 grid(chunks, ceil_div(C, COCR_TR_CT));
    if (m->dtype == COCR_BF16) hipLaunchKernelGGL((decoder_wgrad_kernel<bf16_t>), grid, dim3(256), 0, s, grad_probits, (const bf16_t *)m->ws.xn, M, C, D, part_w, part_b);
    else hipLaunchKernelGGL((decoder_wgrad_kernel<float>), grid, dim3(256), 0, s, grad_probits, (const float *)m->ws.xn, M, C, D, part_w, part_b);
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
    HIP_TRY(hipMalloc((void **)&m->dtr.tr_state, 3 * n * 4));
    HIP_TRY(hipMemsetAsync(m->dtr.tr_state + n, 0, 2 * n * 4, s));
    auto w = m->host.find("decoder.weight"), b = m->host.find("decoder.bias");
    if (w != m->host.end() && w->second.set && w->second.data.size() == nw_model && b != m->host.end() && b->second.set && b->second.data.size() == nb) {
        HIP_TRY(hipMemsetAsync(m->dtr.tr_state, 0, nw * 4, s));
        HIP_TRY(hipMemcpy2DAsync(m->dtr.tr_state, row_e, w->second.data.data(), row_m, row_m, m->ncls, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(m->dtr.tr_state + nw, b->second.data.data(), nb * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));                                   // pageable sources
    } else {
        blob_to_f32(m, m->w->plan.wdec, m->dtr.tr_state, nw, s);
        HIP_TRY(hipMemcpyAsync(m->dtr.tr_state + nw, m->w->blob + m->w->plan.bdec, nb * 4, hipMemcpyDeviceToDevice, s));
        LAUNCH_CHECK();
    }
    m->dtr.tr_step = 0;
    m->dtr.tr_kind = -1;
    return COCR_OK;
}

extern "C" int cocr_get_tensor(cocr_model *m, const char *name, float *host_out, int64_t max_elems, void *stream) {
    if (!m || !name || !host_out) return fail(COCR_EINVAL, "null argument");
    const bool is_w = !strcmp(name, "decoder.weight"), is_b = !strcmp(name, "decoder.bias");
    if (!is_w && !is_b) return fail(COCR_EINVAL, "only decoder.weight / decoder.bias are trained by this library (got '%s')", name);
    const size_t nw = (size_t)m->ncls * m->D, nb = (size_t)m->ncls, n = is_w ? (size_t)m->ncls * m->rD : nb;      // nw: the engine's (maybe padded) copy
    if ((int64_t)n > max_elems) return fail(COCR_EINVAL, "%s has %zu elements, buffer %lld", name, n, (long long)max_elems);
    auto it = m->host.find(name);
    if (m->dtr.tr_state) {
        HIP_TRY(hipSetDevice(m->device));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        if (is_w) HIP_TRY(hipMemcpy2D(host_out, (size_t)m->rD * 4, m->dtr.tr_state, (size_t)m->D * 4, (size_t)m->rD * 4, m->ncls, hipMemcpyDeviceToHost));
        else HIP_TRY(hipMemcpy(host_out, m->dtr.tr_state + nw, n * 4, hipMemcpyDeviceToHost));
        if (it != m->host.end() && it->second.data.size() == n) memcpy(it->second.data.data(), host_out, n * 4);      // a later cocr_finalize keeps the trained values
        return COCR_OK;
    }
    if (it == m->host.end() || !it->second.set || it->second.data.size() != n) return fail(COCR_ESTATE, "%s was never set on this model", name);
    memcpy(host_out, it->second.data.data(), n * 4);
    return COCR_OK;
}

void train_free(cocr_model *m) {
    TrainState *t = m->train;
    if (!t) return;
    for (void *p : {(void *)t->P, (void *)t->G, (void *)t->Mo, (void *)t->Vo})
        if (p) (void)hipFree(p);
    delete t;                                     // (its scratch buffers release themselves)
    m->train = nullptr;
}

static bool train_is_buffer(const std::string &n) { return n.find("running_mean") != std::string::npos || n.find("running_var") != std::string::npos; }

extern "C" int cocr_train_set_matmul(cocr_model *m, int bf16_operands) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    if (!m->train) return fail(COCR_ESTATE, "cocr_train_begin first");
    TrainState *t = m->train;
    t->matmul_bf16 = bf16_operands != 0;
    { const char *e = getenv("COCR_TRAIN_NO_TN"); t->no_tn = e && e[0] == '1'; }
    if (t->matmul_bf16) {
        HIP_TRY(hipSetDevice(m->device));
        HIP_TRY(t->Wb.grow(t->nparam * 4 + 256));
        HIP_TRY(t->WTb.grow(t->nparam * 4 + 256));
    }
    return COCR_OK;
}

extern "C" int cocr_train_begin(cocr_model *m) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    if (m->hp.subsampling_conv_channels % 4 != 0 || m->hp.subsampling_conv_channels > 1024)
        return fail(COCR_EUNSUPPORTED, "training: subsampling_conv_channels must be a multiple of 4 and at most 1024 (is %d)", m->hp.subsampling_conv_channels);
    HIP_TRY(hipSetDevice(m->device));
    train_free(m);
    TrainState *t = new TrainState();
    m->train = t;
    for (int pass = 0; pass < 2; ++pass) {        // parameters, then buffers
        for (auto &n : m->names) {
            const HostTensor &h = m->host[n];
            if (!h.set) { train_free(m); return fail(COCR_ESTATE, "missing tensor '%s'", n.c_str()); }
            if (train_is_buffer(n) != (pass == 1)) continue;
            TrainEntry e;
            e.off = t->ntotal; e.n = h.data.size(); e.param = pass == 0;
            t->ntotal += (e.n + 3) / 4 * 4;              // 16-byte aligned tensors
            t->idx[n] = e;
            t->order.push_back(n);
        }
        if (pass == 0) t->nparam = t->ntotal;
    }
    { const int rc = train_resolve(t, m->snum, m->L); if (rc) { train_free(m); return rc; } }
    std::vector<float> flat(t->ntotal, 0.f);
    for (auto &kv : t->idx) memcpy(flat.data() + kv.second.off, m->host[kv.first].data.data(), kv.second.n * 4);
    HIP_TRY(hipMalloc((void **)&t->P, t->ntotal * 4));
    HIP_TRY(hipMalloc((void **)&t->G, t->nparam * 4));
    HIP_TRY(hipMalloc((void **)&t->Mo, t->nparam * 4));
    HIP_TRY(hipMalloc((void **)&t->Vo, t->nparam * 4));
    HIP_TRY(hipMemcpy(t->P, flat.data(), t->ntotal * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(t->G, 0, t->nparam * 4));
    // both slots zeroed: SGD's / RMSprop's momentum buffer needs no first-step flag (torch sets buf = g' on a tensor's first step, and
    // mu 0 + g' is exactly that), the moments and square averages start at 0 as torch's do
    HIP_TRY(hipMemset(t->Mo, 0, t->nparam * 4));
    HIP_TRY(hipMemset(t->Vo, 0, t->nparam * 4));
    return COCR_OK;
}

// kind: 0 = value (parameter or buffer), 1 = gradient of the last cocr_train_step
extern "C" int cocr_train_get(cocr_model *m, const char *name, int kind, float *host_out, int64_t n_elems, void *stream) {
    if (!m || !name || !host_out) return fail(COCR_EINVAL, "null argument");
    TrainState *t = m->train;
    if (!t) return fail(COCR_ESTATE, "cocr_train_begin has not been called");
    auto it = t->idx.find(name);
    if (it == t->idx.end()) return fail(COCR_EINVAL, "unknown tensor '%s'", name);
    if ((size_t)n_elems != it->second.n) return fail(COCR_EINVAL, "tensor '%s' has %zu elements", name, it->second.n);
    if (kind == 1 && !it->second.param) return fail(COCR_EINVAL, "'%s' is a buffer: no gradient", name);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemcpyAsync(host_out, (kind == 1 ? t->G : t->P) + it->second.off, it->second.n * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return COCR_OK;
}

// the flat device gradient vector (all parameters, the order of cocr_train_begin): what a data-parallel job all-reduces between
// cocr_train_step and cocr_train_adamw
extern "C" int cocr_train_grad_buffer(cocr_model *m, void **device_ptr, size_t *n_floats) {
    if (!m || !device_ptr || !n_floats) return fail(COCR_EINVAL, "null argument");
    if (!m->train) return fail(COCR_ESTATE, "cocr_train_begin has not been called");
    *device_ptr = m->train->G;
    *n_floats = m->train->nparam;
    return COCR_OK;
}

// the flat device VALUE vector in the same layout: parameters [0, n_params), then buffers (BatchNorm running statistics) up to n_total.
// A caller that keeps the parameters elsewhere (torch: `net.nn.parameters()`, updated by a torch optimizer) writes them here before
// cocr_train_step and reads the running statistics back afterwards (device-to-device, stream-ordered).
extern "C" int cocr_train_param_buffer(cocr_model *m, void **device_ptr, size_t *n_total, size_t *n_params) {
    if (!m || !device_ptr || !n_total || !n_params) return fail(COCR_EINVAL, "null argument");
    if (!m->train) return fail(COCR_ESTATE, "cocr_train_begin has not been called");
    *device_ptr = m->train->P;
    *n_total = m->train->ntotal;
    *n_params = m->train->nparam;
    return COCR_OK;
}
// where a reference state-dict name lives in those vectors: float offset and element count; *is_param = 0 for a buffer (no gradient)
extern "C" int cocr_train_layout(cocr_model *m, const char *name, int64_t *offset, int64_t *n_elems, int *is_param) {
    if (!m || !name || !offset || !n_elems || !is_param) return fail(COCR_EINVAL, "null argument");
    if (!m->train) return fail(COCR_ESTATE, "cocr_train_begin has not been called");
    auto it = m->train->idx.find(name);
    if (it == m->train->idx.end()) return fail(COCR_EINVAL, "unknown tensor '%s'", name);
    *offset = (int64_t)it->second.off;
    *n_elems = (int64_t)it->second.n;
    *is_param = it->second.param ? 1 : 0;
    return COCR_OK;
}

extern "C" int cocr_train_end(cocr_model *m) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    TrainState *t = m->train;
    if (!t) return fail(COCR_ESTATE, "cocr_train_begin has not been called");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<float> flat(t->ntotal);
    HIP_TRY(hipMemcpy(flat.data(), t->P, t->ntotal * 4, hipMemcpyDeviceToHost));
    for (auto &kv : t->idx) memcpy(m->host[kv.first].data.data(), flat.data() + kv.second.off, kv.second.n * 4);
    train_free(m);
    return COCR_OK;
}

static const char *optim_name(int kind) {
    static const char *names[] = {"AdamW", "Adam", "SGD", "RMSprop"};
    return kind >= 0 && kind < 4 ? names[kind] : "none";
}

extern "C" int cocr_train_adamw(cocr_model *m, float lr, float beta1, float beta2, float eps, float weight_decay, void *stream) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    TrainState *t = m->train;
    if (!t) return fail(COCR_ESTATE, "cocr_train_begin has not been called");
    if (!(lr >= 0.f) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f) || !(weight_decay >= 0.f))
        return fail(COCR_EINVAL, "invalid AdamW hyper-parameters");
    if (t->kind >= 0 && t->kind != COCR_OPT_ADAMW) return fail(COCR_ESTATE, "the optimizer state is of kind %d, not AdamW", t->kind);
    HIP_TRY(hipSetDevice(m->device));
    t->kind = COCR_OPT_ADAMW;
    t->step += 1;
    const float bc1 = 1.0f - powf(beta1, (float)t->step), bc2 = 1.0f - powf(beta2, (float)t->step);
    if (t->dec_steps == 0) {
        hipLaunchKernelGGL(k_adamw_flat, dim3(1024), dim3(256), 0, (hipStream_t)stream, t->P, t->G, t->Mo, t->Vo, t->nparam, lr, beta1, beta2, eps, weight_decay, bc1, bc2);
    } else {
        // per-tensor step counts: the adopted output layer is dec_steps steps ahead of every other parameter
        const long k = t->step + t->dec_steps;
        AdamwRanges r = {};
        int i = 0;
        for (const char *name : {"decoder.weight", "decoder.bias"}) {
            const TrainEntry &e = t->idx.at(name);
            r.lo[i] = e.off; r.hi[i] = e.off + e.n;
            r.bc1[i] = 1.0f - powf(beta1, (float)k); r.bc2[i] = 1.0f - powf(beta2, (float)k);
            ++i;
        }
        hipLaunchKernelGGL(k_adamw_flat_ranges, dim3(1024), dim3(256), 0, (hipStream_t)stream, t->P, t->G, t->Mo, t->Vo, t->nparam, lr, beta1, beta2, eps, weight_decay, bc1, bc2, r);
    }
    LAUNCH_CHECK();
    return COCR_OK;
}

// The output layer of `src` as its decoder-only steps left it (cocr_decoder_adamw: fp32 master copy, both moments, step count k) into the
// training state of `dst`: device to device on `stream`, rows re-strided from the engine's (maybe padded) width to the model's own.
// cocr_train_adamw then continues that layer at step k + 1.  A `src` that never stepped hands over its values, zero moments and k = 0.
extern "C" int cocr_train_adopt_decoder(cocr_model *dst, cocr_model *src, void *stream) {
    if (!dst || !src) return fail(COCR_EINVAL, "null argument");
    TrainState *t = dst->train;
    if (!t) return fail(COCR_ESTATE, "cocr_train_begin has not been called on the adopting model");
    if (!src->w->blob) return fail(COCR_ESTATE, "the source model is not finalized");
    { const int rc = adopt_layout(src); if (rc) return rc; }
    if (src->device != dst->device) return fail(COCR_EINVAL, "the two models live on different devices (%d, %d)", src->device, dst->device);
    auto w = t->idx.find("decoder.weight"), b = t->idx.find("decoder.bias");
    if (w == t->idx.end() || b == t->idx.end()) return fail(COCR_ESTATE, "the training state has no output layer");
    if (src->ncls != dst->ncls || src->rD != dst->rD || w->second.n != (size_t)src->ncls * src->rD || b->second.n != (size_t)src->ncls)
        return fail(COCR_EINVAL, "output layers differ: (%d, %d) into (%d, %d)", src->ncls, src->rD, dst->ncls, dst->rD);
    if (src->dtr.tr_state && src->dtr.tr_kind >= 0 && t->kind >= 0 && src->dtr.tr_kind != t->kind)
        return fail(COCR_EINVAL, "the two states have taken steps of different optimizer kinds (%s into %s)", optim_name(src->dtr.tr_kind), optim_name(t->kind));
    HIP_TRY(hipSetDevice(dst->device));
    hipStream_t s = (hipStream_t)stream;
    if (!src->dtr.tr_state) { const int rc = decoder_master_init(src, s); if (rc) return rc; }
    const size_t nw = (size_t)src->ncls * src->D, n = nw + (size_t)src->ncls;
    const size_t row_e = (size_t)src->D * 4, row_m = (size_t)src->rD * 4;
    float *dsts[3] = {t->P, t->Mo, t->Vo};
    for (int i = 0; i < 3; ++i) {
        const float *from = src->dtr.tr_state + (size_t)i * n;
        HIP_TRY(hipMemcpy2DAsync(dsts[i] + w->second.off, row_m, from, row_e, row_m, src->ncls, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(dsts[i] + b->second.off, from + nw, (size_t)src->ncls * 4, hipMemcpyDeviceToDevice, s));
    }
    t->dec_steps = src->dtr.tr_step - t->step;        // (the layer's count is dst's own count + dec_steps: an adoption after dst has stepped keeps k exact)
    if (t->kind < 0) t->kind = src->dtr.tr_kind;      // (slots and count mean what they meant in `src`; SGD / RMSprop read no count)
    return COCR_OK;
}

// ---- one step of any optimizer kind ------------------------------------------------------------------------------------------------------------
// torch.optim's own constructor checks
static int optim_check(const cocr_optim *o) {
    if (!o) return fail(COCR_EINVAL, "null argument");
    if (o->kind < COCR_OPT_ADAMW || o->kind > COCR_OPT_RMSPROP) return fail(COCR_EINVAL, "unknown optimizer kind %d", o->kind);
    if (!(o->lr >= 0.f)) return fail(COCR_EINVAL, "invalid learning rate %g", (double)o->lr);
    if (!(o->weight_decay >= 0.f)) return fail(COCR_EINVAL, "invalid weight_decay %g", (double)o->weight_decay);
    if (o->kind == COCR_OPT_ADAMW || o->kind == COCR_OPT_ADAM) {
        if (!(o->beta1 >= 0.f && o->beta1 < 1.f) || !(o->beta2 >= 0.f && o->beta2 < 1.f)) return fail(COCR_EINVAL, "invalid beta (%g, %g)", (double)o->beta1, (double)o->beta2);
        if (!(o->eps >= 0.f)) return fail(COCR_EINVAL, "invalid epsilon %g", (double)o->eps);
    } else {
        if (!(o->momentum >= 0.f)) return fail(COCR_EINVAL, "invalid momentum %g", (double)o->momentum);
        if (o->kind == COCR_OPT_RMSPROP && (!(o->eps >= 0.f) || !(o->alpha >= 0.f))) return fail(COCR_EINVAL, "invalid epsilon / alpha (%g, %g)", (double)o->eps, (double)o->alpha);
    }
    return COCR_OK;
}

// n elements of (P, G, S0, S1); bc1 / bc2: the bias corrections of every element outside `ranges` (Adam kinds; null: no ranges)
// grad_scale: every gradient element enters the step as fl(grad_scale g) (cocr_train_optim_step_ex; 1.0f: the gradient as it is)
static int launch_optim(hipStream_t s, const cocr_optim *o, float *P, const float *G, float *S0, float *S1, size_t n, float bc1, float bc2, const AdamwRanges *ranges,
                        bf16_t *serve_b, float *serve_f, float grad_scale = 1.0f) {
    if (n == 0) return COCR_OK;
    // 16 bytes per lane where all four vectors are aligned at the same elements; otherwise (a slot that starts at an odd float offset of
    // its allocation) every element goes the scalar way
    size_t head = std::min<size_t>(n, (size_t)((16 - ((uintptr_t)P & 15)) & 15) / 4);
    for (const void *q : {(const void *)(P + head), (const void *)(G + head), (const void *)(S0 + head), (const void *)(S1 + head)})
        if ((uintptr_t)q & 15) head = n;
    const size_t nvec = (n - head) / 4;
    const OptimArgs a = {o->lr, o->weight_decay, o->beta1, o->beta2, o->eps, o->momentum, o->alpha, bc1, bc2, grad_scale};
    const AdamwRanges r = ranges ? *ranges : AdamwRanges{};
    const dim3 grid((unsigned)std::max<size_t>(1, std::min<size_t>((std::max(nvec, n - 4 * nvec) + 255) / 256, 2048))), block(256);
    const bool flag = (o->kind == COCR_OPT_ADAMW || o->kind == COCR_OPT_ADAM) ? ranges != nullptr : o->momentum > 0.f;
#define COCR_OPTIM_LAUNCH(K, F) hipLaunchKernelGGL((k_optim_flat<K, F>), grid, block, 0, s, P, G, S0, S1, n, head, nvec, a, r, serve_b, serve_f)
    switch (o->kind * 2 + (flag ? 1 : 0)) {
        case COCR_OPT_ADAMW * 2: COCR_OPTIM_LAUNCH(COCR_OPT_ADAMW, false); break;
        case COCR_OPT_ADAMW * 2 + 1: COCR_OPTIM_LAUNCH(COCR_OPT_ADAMW, true); break;
        case COCR_OPT_ADAM * 2: COCR_OPTIM_LAUNCH(COCR_OPT_ADAM, false); break;
        case COCR_OPT_ADAM * 2 + 1: COCR_OPTIM_LAUNCH(COCR_OPT_ADAM, true); break;
        case COCR_OPT_SGD * 2: COCR_OPTIM_LAUNCH(COCR_OPT_SGD, false); break;
        case COCR_OPT_SGD * 2 + 1: COCR_OPTIM_LAUNCH(COCR_OPT_SGD, true); break;
        case COCR_OPT_RMSPROP * 2: COCR_OPTIM_LAUNCH(COCR_OPT_RMSPROP, false); break;
        default: COCR_OPTIM_LAUNCH(COCR_OPT_RMSPROP, true); break;
    }
#undef COCR_OPTIM_LAUNCH
    LAUNCH_CHECK();
    return COCR_OK;
}

// cocr_train_optim_step with the gradient read from `grad` (NULL: the state's own vector) and scaled by grad_scale on its way in
extern "C" int cocr_train_optim_step_ex(cocr_model *m, const cocr_optim *o, const float *grad, float grad_scale, void *stream) {
    if (!m || !o) return fail(COCR_EINVAL, "null argument");
    TrainState *t = m->train;
    if (!t) return fail(COCR_ESTATE, "cocr_train_begin has not been called");
    { const int rc = optim_check(o); if (rc) return rc; }
    // finite and >= 0, or NaN (what torch's clip makes of a NaN norm; the Trainer never passes one)
    if (!std::isnan(grad_scale) && !(grad_scale >= 0.f && std::isfinite(grad_scale))) return fail(COCR_EINVAL, "invalid grad_scale %g", (double)grad_scale);
    if (t->kind >= 0 && t->kind != o->kind) return fail(COCR_ESTATE, "the optimizer state is %s's: a %s step cannot follow", optim_name(t->kind), optim_name(o->kind));
    HIP_TRY(hipSetDevice(m->device));
    t->kind = o->kind;
    t->step += 1;
    float bc1 = 1.f, bc2 = 1.f;
    AdamwRanges r = {};
    bool ranges = false;
    if (o->kind == COCR_OPT_ADAMW || o->kind == COCR_OPT_ADAM) {      // (the corrections of cocr_train_adamw, expression for expression)
        bc1 = 1.0f - powf(o->beta1, (float)t->step); bc2 = 1.0f - powf(o->beta2, (float)t->step);
        if (t->dec_steps != 0) {
            // per-tensor step counts: the adopted output layer is dec_steps steps ahead of every other parameter
            const long k = t->step + t->dec_steps;
            int i = 0;
            for (const char *name : {"decoder.weight", "decoder.bias"}) {
                const TrainEntry &e = t->idx.at(name);
                r.lo[i] = e.off; r.hi[i] = e.off + e.n;
                r.bc1[i] = 1.0f - powf(o->beta1, (float)k); r.bc2[i] = 1.0f - powf(o->beta2, (float)k);
                ++i;
            }
            ranges = true;
        }
    }
    return launch_optim((hipStream_t)stream, o, t->P, grad ? grad : t->G, t->Mo, t->Vo, t->nparam, bc1, bc2, ranges ? &r : nullptr, nullptr, nullptr, grad_scale);
}

// = cocr_train_optim_step_ex(m, o, NULL, 1.0f, stream): fl(1.0f g) is g for every float, so the step keeps its bits
extern "C" int cocr_train_optim_step(cocr_model *m, const cocr_optim *o, void *stream) { return cocr_train_optim_step_ex(m, o, nullptr, 1.0f, stream); }

// ---- the gradient window on raw device vectors (kernels: train_optim.hip.h) ------------------------------------------------------------------------
extern "C" int cocr_grad_accumulate(float *dst, const float *src, size_t n, float scale, int overwrite, int device, void *stream) {
    if (n == 0) return COCR_OK;
    if (!dst || !src) return fail(COCR_EINVAL, "null argument");
    if (dst == src && !overwrite) return fail(COCR_EINVAL, "dst may be src only with overwrite (the in-place scale)");
    HIP_TRY(hipSetDevice(device));
    // 16 bytes per lane where both vectors are aligned at the same elements; otherwise every element goes the scalar way
    size_t head = std::min<size_t>(n, (size_t)((16 - ((uintptr_t)dst & 15)) & 15) / 4);
    if (((uintptr_t)(dst + head) & 15) || ((uintptr_t)(src + head) & 15)) head = n;
    const size_t nvec = (n - head) / 4;
    const dim3 grid((unsigned)std::max<size_t>(1, std::min<size_t>((std::max(nvec, n - 4 * nvec) + 255) / 256, 2048))), block(256);
    hipLaunchKernelGGL(k_grad_accumulate, grid, block, 0, (hipStream_t)stream, dst, src, n, head, nvec, scale, overwrite ? 1 : 0);
    LAUNCH_CHECK();
    return COCR_OK;
}

// The norm's scratch, one per device, allocated on the first call there and kept for the life of the process: the chunk sums and the
// result on the device, the result's pinned host twin.  One call at a time per device holds it from its launches to its wait.
#define COCR_NORM_DEVICES 64
struct NormScratch { double *dev = nullptr, *host = nullptr; std::mutex mu; };
static NormScratch g_norm[COCR_NORM_DEVICES];

extern "C" int cocr_grad_norm(const float *g, size_t n, int device, double *norm_out, void *stream) {
    if (!norm_out) return fail(COCR_EINVAL, "null argument");
    if (n == 0) { *norm_out = 0.0; return COCR_OK; }
    if (!g) return fail(COCR_EINVAL, "null argument");
    if ((uintptr_t)g & 3) return fail(COCR_EINVAL, "the vector is not aligned to a float");
    if (device < 0 || device >= COCR_NORM_DEVICES) return fail(COCR_EINVAL, "device %d out of range", device);
    HIP_TRY(hipSetDevice(device));
    NormScratch &sc = g_norm[device];
    std::lock_guard<std::mutex> lock(sc.mu);
    if (!sc.dev) HIP_TRY(hipMalloc((void **)&sc.dev, (COCR_NORM_MAX_CHUNKS + 1) * sizeof(double)));
    if (!sc.host) HIP_TRY(hipHostMalloc((void **)&sc.host, sizeof(double)));
    // the chunk length depends on n only: a multiple of 4 floats, at least 4096, at most COCR_NORM_MAX_CHUNKS chunks
    const size_t len = std::max<size_t>(4096, ((n + COCR_NORM_MAX_CHUNKS - 1) / COCR_NORM_MAX_CHUNKS + 3) / 4 * 4);
    const int nchunk = (int)((n + len - 1) / len);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sumsq_chunks, dim3(nchunk), dim3(256), 0, s, g, n, len, ((uintptr_t)g & 15) == 0 ? 1 : 0, sc.dev);
    hipLaunchKernelGGL(k_sumsq_finish, dim3(1), dim3(256), 0, s, (const double *)sc.dev, nchunk, sc.dev + COCR_NORM_MAX_CHUNKS);
    LAUNCH_CHECK();
    HIP_TRY(hipMemcpyAsync(sc.host, sc.dev + COCR_NORM_MAX_CHUNKS, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *norm_out = *sc.host;
    return COCR_OK;
}

// What a step on the output layer's own state (fp32 master copy [W | b], slot 0, slot 1: created on the first call; the frozen-backbone
// phase) starts with, whichever kernel follows: the checks, the caller's gradient at the engine's row width (*grad_weight), the sticky
// kind, the step count (*k).
static int decoder_step_begin(cocr_model *m, const float **grad_weight, const float *grad_bias, const cocr_optim *o, hipStream_t s, long *k) {
    if (!m || !*grad_weight || !grad_bias || !o) return fail(COCR_EINVAL, "null argument");
    if (!m->w->blob) return fail(COCR_ESTATE, "model not finalized");
    if (!m->w->owned_by(m)) return fail(COCR_ESTATE, "this model shares another model's weights: step the owner");
    { const int rc = adopt_layout(m); if (rc) return rc; }
    { const int rc = optim_check(o); if (rc) return rc; }
    HIP_TRY(hipSetDevice(m->device));
    if (m->padded) {    // the caller's (ncls, rD) gradient embedded in the engine's zero-padded rows
        const size_t nw = (size_t)m->ncls * m->D, row_e = (size_t)m->D * 4, row_m = (size_t)m->rD * 4;
        HIP_TRY(m->dtr.tr_pad.grow(nw));
        HIP_TRY(hipMemsetAsync(m->dtr.tr_pad.p, 0, nw * 4, s));
        HIP_TRY(hipMemcpy2DAsync(m->dtr.tr_pad.p, row_e, *grad_weight, row_m, row_m, m->ncls, hipMemcpyDeviceToDevice, s));
        *grad_weight = m->dtr.tr_pad.p;
    }
    if (!m->dtr.tr_state) { const int rc = decoder_master_init(m, s); if (rc) return rc; }
    if (m->dtr.tr_kind >= 0 && m->dtr.tr_kind != o->kind)
        return fail(COCR_ESTATE, "the output layer's optimizer state is %s's: a %s step cannot follow", optim_name(m->dtr.tr_kind), optim_name(o->kind));
    m->dtr.tr_kind = o->kind;
    *k = ++m->dtr.tr_step;
    return COCR_OK;
}

// The step of cocr_train_optim_step on that state; the updated values also go where the next cocr_forward reads them (the compute
// dtype's copy of the weight, the fp32 bias).
extern "C" int cocr_decoder_optim_step(cocr_model *m, const float *grad_weight, const float *grad_bias, const cocr_optim *o, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    long k;
    { const int rc = decoder_step_begin(m, &grad_weight, grad_bias, o, s, &k); if (rc) return rc; }
    const size_t nw = (size_t)m->ncls * m->D, nb = (size_t)m->ncls, n = nw + nb;
    float bc1 = 1.f, bc2 = 1.f;
    if (o->kind == COCR_OPT_ADAMW || o->kind == COCR_OPT_ADAM) { bc1 = 1.0f - powf(o->beta1, (float)k); bc2 = 1.0f - powf(o->beta2, (float)k); }
    float *p = m->dtr.tr_state, *s0 = p + n, *s1 = s0 + n;
    const bool bf = m->dtype == COCR_BF16;
    int rc = launch_optim(s, o, p, grad_weight, s0, s1, nw, bc1, bc2, nullptr, bf ? (bf16_t *)(m->w->blob + m->w->plan.wdec) : nullptr, bf ? nullptr : (float *)(m->w->blob + m->w->plan.wdec));
    if (rc) return rc;
    return launch_optim(s, o, p + nw, grad_bias, s0 + nw, s1 + nw, nb, bc1, bc2, nullptr, nullptr, (float *)(m->w->blob + m->w->plan.bdec));
}

// torch.optim.AdamW on the same state through adamw_kernel (train.hip.h), the step every frozen-backbone AdamW fit has taken.  NOT
// cocr_decoder_optim_step with kind AdamW: see the note at the kernel.
extern "C" int cocr_decoder_adamw(cocr_model *m, const float *grad_weight, const float *grad_bias, float lr, float beta1, float beta2, float eps,
                                  float weight_decay, void *stream) {
    const cocr_optim o = {COCR_OPT_ADAMW, lr, weight_decay, beta1, beta2, eps};
    hipStream_t s = (hipStream_t)stream;
    long t;
    { const int rc = decoder_step_begin(m, &grad_weight, grad_bias, &o, s, &t); if (rc) return rc; }
    const size_t nw = (size_t)m->ncls * m->D, nb = (size_t)m->ncls, n = nw + nb;
    const float bc1 = 1.0f - (float)pow((double)beta1, (double)t), bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)t));
    float *p = m->dtr.tr_state, *m1 = p + n, *m2 = m1 + n;
    if (m->dtype == COCR_BF16)
        hipLaunchKernelGGL((adamw_kernel<bf16_t>), dim3(ceil_div((int)nw, 256)), dim3(256), 0, s, p, grad_weight, m1, m2, nw, lr, beta1, beta2, eps, weight_decay, bc1, bc2s,
                           (bf16_t *)(m->w->blob + m->w->plan.wdec), (float *)nullptr);
    else
        hipLaunchKernelGGL((adamw_kernel<float>), dim3(ceil_div((int)nw, 256)), dim3(256), 0, s, p, grad_weight, m1, m2, nw, lr, beta1, beta2, eps, weight_decay, bc1, bc2s,
                           (float *)nullptr, (float *)(m->w->blob + m->w->plan.wdec));
    hipLaunchKernelGGL((adamw_kernel<float>), dim3(ceil_div((int)nb, 256)), dim3(256), 0, s, p + nw, grad_bias, m1 + nw, m2 + nw, nb, lr, beta1, beta2, eps, weight_decay, bc1, bc2s,
                       (float *)nullptr, (float *)(m->w->blob + m->w->plan.bdec));
    LAUNCH_CHECK();
    return COCR_OK;
}

// ---- the optimizer state out of and back into the library (resuming a fit) -----------------------------------------------------------------------
extern "C" int cocr_train_optim_state(cocr_model *m, int *kind, int64_t *step, int64_t *dec_steps, void **slot0, void **slot1, size_t *n_floats) {
    if (!m || !kind || !step || !dec_steps || !slot0 || !slot1 || !n_floats) return fail(COCR_EINVAL, "null argument");
    TrainState *t = m->train;
    if (!t) return fail(COCR_ESTATE, "cocr_train_begin has not been called");
    *kind = t->kind; *step = t->step; *dec_steps = t->dec_steps;
    *slot0 = t->Mo; *slot1 = t->Vo; *n_floats = t->nparam;
    return COCR_OK;
}

extern "C" int cocr_train_optim_restore(cocr_model *m, int kind, int64_t step, int64_t dec_steps) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    TrainState *t = m->train;
    if (!t) return fail(COCR_ESTATE, "cocr_train_begin has not been called");
    if (kind < -1 || kind > COCR_OPT_RMSPROP) return fail(COCR_EINVAL, "unknown optimizer kind %d", kind);
    if (step < 0 || step + dec_steps < 0 || (kind < 0 && step != 0)) return fail(COCR_EINVAL, "invalid step counts (%lld, %lld) for kind %d", (long long)step, (long long)dec_steps, kind);
    t->kind = kind; t->step = (long)step; t->dec_steps = (long)dec_steps;
    return COCR_OK;
}

extern "C" int cocr_decoder_optim_state(cocr_model *m, int *kind, int64_t *step, void **state, size_t *n_floats) {
    if (!m || !kind || !step || !state || !n_floats) return fail(COCR_EINVAL, "null argument");
    if (!m->w->blob) return fail(COCR_ESTATE, "model not finalized");
    { const int rc = adopt_layout(m); if (rc) return rc; }
    *kind = m->dtr.tr_state ? m->dtr.tr_kind : -1;
    *step = m->dtr.tr_state ? m->dtr.tr_step : 0;
    *state = m->dtr.tr_state;
    *n_floats = 3 * ((size_t)m->ncls * m->D + (size_t)m->ncls);
    return COCR_OK;
}

extern "C" int cocr_decoder_optim_restore(cocr_model *m, int kind, int64_t step, const float *state_device, size_t n_floats, void *stream) {
    if (!m || !state_device) return fail(COCR_EINVAL, "null argument");
    if (!m->w->blob) return fail(COCR_ESTATE, "model not finalized");
    if (!m->w->owned_by(m)) return fail(COCR_ESTATE, "this model shares another model's weights: restore the owner");
    { const int rc = adopt_layout(m); if (rc) return rc; }
    const size_t nw = (size_t)m->ncls * m->D, nb = (size_t)m->ncls, n = nw + nb;
    if (n_floats != 3 * n) return fail(COCR_EINVAL, "the output layer's state has %zu floats, not %zu", 3 * n, n_floats);
    if (kind < -1 || kind > COCR_OPT_RMSPROP || step < 0 || (kind < 0 && step != 0)) return fail(COCR_EINVAL, "invalid kind %d / step %lld", kind, (long long)step);
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    if (!m->dtr.tr_state) { const int rc = decoder_master_init(m, s); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(m->dtr.tr_state, state_device, 3 * n * 4, hipMemcpyDeviceToDevice, s));
    m->dtr.tr_kind = kind; m->dtr.tr_step = (long)step;
    const bool bf = m->dtype == COCR_BF16;
    hipLaunchKernelGGL(k_serve_copy, dim3(64), dim3(256), 0, s, (const float *)m->dtr.tr_state, nw, bf ? (bf16_t *)(m->w->blob + m->w->plan.wdec) : (bf16_t *)nullptr,
                       bf ? (float *)nullptr : (float *)(m->w->blob + m->w->plan.wdec));
    hipLaunchKernelGGL(k_serve_copy, dim3(1), dim3(256), 0, s, (const float *)(m->dtr.tr_state + nw), nb, (bf16_t *)nullptr, (float *)(m->w->blob + m->w->plan.bdec));
    LAUNCH_CHECK();
    return COCR_OK;
}

// dropout_p: {input, feed_forward, attention, conv} (the reference's four probabilities, encoder.py:144-147); loss_out (host): the summed CTC loss
// The body of both entries.  teacher null: cocr_train_step (loss_out[0] alone is written); else cocr_train_step_distill
static int train_step_body(cocr_model *m, const void *lines, int line_dtype, int N, int H, int W, const int32_t *in_lens, const int32_t *targets,
                           const int32_t *label_lens, const float *dropout_p, uint64_t seed, const float *teacher, float tau, float lambda, float *loss_out,
                           void *stream) {
    if (!m || !lines || !in_lens || !label_lens || !loss_out) return fail(COCR_EINVAL, "null argument");
    TrainState *t = m->train;
    if (!t) return fail(COCR_ESTATE, "cocr_train_begin has not been called");
    if (H != m->H) return fail(COCR_EINVAL, "line height %d does not match the model's height %d", H, m->H);
    if (N < 1 || W < 1) return fail(COCR_EINVAL, "empty batch");
    if (line_dtype != COCR_F32 && line_dtype != COCR_U8) return fail(COCR_EINVAL, "line dtype must be COCR_F32 or COCR_U8");
    const float no_drop[4] = {0.f, 0.f, 0.f, 0.f}, *drop = dropout_p ? dropout_p : no_drop;
    for (int i = 0; i < 4; ++i) if (!(drop[i] >= 0.f && drop[i] < 1.f)) return fail(COCR_EINVAL, "dropout probability outside [0, 1)");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    Train c(m, train_plan(m, t, N, H, W), s, seed, drop);

    // ---- the three per-step arenas, (re)sized for this shape (a growth frees memory that work in flight may still read)
    if (c.parts_floats > t->parts.n) HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(t->parts.grow(c.parts_floats));
    HIP_TRY(grow_pair(t->jobs_dev, t->jobs_host, COCR_MAX_COLSUM_JOBS));
    t->parts_used = 0;
    t->jobs.clear();
    if (t->matmul_bf16) {
        if (c.xb_bytes > t->Xb.n) HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(t->Xb.grow(c.xb_bytes));
        t->Xb_used = 0;
        t->Xb_off.assign(t->W.nlin, TRAIN_NONE);
    }
    if (c.ws_bytes > t->ws.n) HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(t->ws.grow(c.ws_bytes));

    // ---- positional rows PE(p), p = T-1 ... -(T-1) (embedding.py:35-56,66), cached per T
    if (t->peT != c.T) {
        const int T = c.T, R = c.R, D = c.D;
        t->peT = 0;                                   // (until the new rows are in place)
        t->pe.release();
        std::vector<float> pe((size_t)R * D);
        for (int r = 0; r < R; ++r) {
            const float pos = (float)(T - 1 - r);
            for (int i = 0; i < D; i += 2) {
                const float div = expf((float)i * (float)(-(log(10000.0) / D)));
                pe[(size_t)r * D + i] = sinf(pos * div);
                if (i + 1 < D) pe[(size_t)r * D + i + 1] = cosf(pos * div);
            }
        }
        HIP_TRY(t->pe.grow(pe.size()));
        HIP_TRY(hipMemcpy(t->pe.p, pe.data(), pe.size() * 4, hipMemcpyHostToDevice));
        t->peT = T;
    }
    HIP_TRY(hipMemsetAsync(t->G, 0, t->nparam * 4, s));

    int rc;
    if ((rc = c.front_fwd(lines, line_dtype))) return rc;
    for (int l = 0; l < c.L; ++l) {
        if ((rc = c.ffn_fwd(l, 0)) || (rc = c.attn_fwd(l)) || (rc = c.conv_fwd(l)) || (rc = c.ffn_fwd(l, 1))) return rc;
        c.final_ln_fwd(l);
    }
    if ((rc = c.decoder_criterion(in_lens, targets, label_lens, teacher, tau, lambda, loss_out))) return rc;

    if ((rc = c.decoder_bwd())) return rc;
    for (int l = c.L - 1; l >= 0; --l) {
        c.final_ln_bwd(l);
        if ((rc = c.ffn_bwd(l, 1)) || (rc = c.conv_bwd(l)) || (rc = c.attn_bwd(l)) || (rc = c.ffn_bwd(l, 0)) || (rc = c.block_done())) return rc;
    }
    if ((rc = c.front_bwd()) || (rc = c.flush_finals())) return rc;
    LAUNCH_CHECK();
    return COCR_OK;
}

extern "C" int cocr_train_step(cocr_model *m, const void *lines, int line_dtype, int N, int H, int W, const int32_t *in_lens, const int32_t *targets,
                               const int32_t *label_lens, const float *dropout_p, uint64_t seed, float *loss_out, void *stream) {
    return train_step_body(m, lines, line_dtype, N, H, W, in_lens, targets, label_lens, dropout_p, seed, nullptr, 1.0f, 0.0f, loss_out, stream);
}

// cocr_train_step with the distillation term: teacher_logits DEVICE (N, T, ncls), T = the frames of a W px line;
// the criterion is (1 - weight) sum CTC + weight sum KD at temperature tau; loss_out (host) [2]: the two sums, unweighted
extern "C" int cocr_train_step_distill(cocr_model *m, const void *lines, int line_dtype, int N, int H, int W, const int32_t *in_lens, const int32_t *targets,
                                       const int32_t *label_lens, const float *dropout_p, uint64_t seed, const float *teacher_logits, float tau, float weight,
                                       float *loss_out, void *stream) {
    if (!teacher_logits) return fail(COCR_EINVAL, "null argument");
    if (!std::isfinite(tau) || !(tau > 0.f)) return fail(COCR_EINVAL, "the temperature must be finite and positive, not %g", (double)tau);
    if (!(weight >= 0.f && weight <= 1.f)) return fail(COCR_EINVAL, "the distillation weight %g is outside [0, 1]", (double)weight);
    return train_step_body(m, lines, line_dtype, N, H, W, in_lens, targets, label_lens, dropout_p, seed, teacher_logits, tau, weight, loss_out, stream);
}
