// Line images behind the C ABI (units of the host layer: model.hip.h): host-side collation, pre-processing, baseline line
// extraction from pages, training augmentation.
#include <thread>

#include "model.hip.h"
#include "preproc.hip.h"
#include "page.hip.h"
#include "augment.hip.h"

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
    if (need > m->lines.pre_buf.n) HIP_TRY(hipStreamSynchronize(s));      // an earlier call on this stream may still read the old buffer
    HIP_TRY(m->lines.pre_buf.grow(need, need + need / 4));
    PreLine *d_lines = reinterpret_cast<PreLine *>(m->lines.pre_buf.p);
    int *d_tab = reinterpret_cast<int *>(m->lines.pre_buf.p + lines_b);
    unsigned char *d_tmp = m->lines.pre_buf.p + lines_b + tab_b;
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
    if (need > m->lines.page_buf.n) HIP_TRY(hipStreamSynchronize(s));     // an earlier call on this stream may still read the old buffer
    HIP_TRY(m->lines.page_buf.grow(need, need + need / 4));
    unsigned char *b = m->lines.page_buf.p;
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
