// Baseline line extraction in front of the pre-processing: a page image in device memory plus per-line
// geometry -> one straightened grayscale strip per text line, packed the way cocr_preproc_lines reads its input (cpp = 1).
//
// The host (conformer_ocr_amd/page.py) turns a line's baseline and boundary polygon into a per-column frame: the baseline point
// B(c) and the unit normal N(c) of strip column c, int64 fixed point in 1/65536 px.  Strip pixel (r, c) samples the page at
// B(c) + (r - T) N(c), quantised to 1/256 px, by an integer bilinear blend of its four neighbours; a neighbour outside the page or
// outside the polygon counts as `fill`.  The polygon mask is exact (even-odd rule on integer vertices): per source row y the
// crossing thresholds ceil(x_cross(y)) of the edges that straddle y, sorted, are half-open spans [t0, t1) [t2, t3) ...
//
// Two kernels:
//   page_spans_kernel  one thread per (line, source row of the polygon's bounding box): thresholds of every edge, insertion-sorted
//                      into the row's slot of the span table (slot sizes are counted on the host from the edges' row ranges);
//   page_sample_kernel lanes along the strip column (coalesced stores), a thread owns a column and walks a chunk of rows (B and N
//                      are per column; each row only adds N); the neighbours are byte gathers served by L1 / L2, every one of them
//                      bounds-checked against its own page.
// Both are integer only.  Lines of one launch may come from different pages.
#pragma once
#include "common.hip.h"

struct PageLine {
    const unsigned char *page;   // first byte of the line's page (device), rows of pw * cpp bytes
    long long out_off;           // first byte of the strip in the output buffer (hs rows of ws bytes)
    long long col_off;           // first column record (Bx, By, Nx, Ny int64) in the column table
    long long row_off;           // first entry of the line's (nrows + 1) span-row offsets
    int ph, pw, cpp;             // page rows, columns, bytes per pixel (1 | 3)
    int hs, ws, t;               // strip rows, columns, the baseline's row
    int vert_off, nverts;        // first vertex (x, y int32 pairs) of the boundary polygon, vertex count
    int ymin, nrows;             // the polygon's source rows [ymin, ymin + nrows)
    int fill;                    // value of a neighbour outside the page or the polygon
};

static constexpr int PAGE_ROWS_PER_THREAD = 16;

// ceil(n / d) for d > 0, exact for either sign of n
__host__ __device__ __forceinline__ long long page_ceil_div(long long n, long long d) {
    return n >= 0 ? (n + d - 1) / d : -((-n) / d);
}

__global__ __launch_bounds__(256) void page_spans_kernel(const PageLine *__restrict__ lines, const int *__restrict__ verts,
                                                         const long long *__restrict__ row_start, int *__restrict__ thr) {
    const PageLine L = lines[blockIdx.y];
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= L.nrows) return;
    const int y = L.ymin + r;
    const long long base = row_start[L.row_off + r];
    const int *v = verts + 2 * (size_t)L.vert_off;
    int n = 0;
    for (int e = 0; e < L.nverts; ++e) {
        const int f = e + 1 == L.nverts ? 0 : e + 1;
        const int ax = v[2 * e], ay = v[2 * e + 1], bx = v[2 * f], by = v[2 * f + 1];
        if ((ay > y) == (by > y)) continue;
        long long num = (long long)(y - ay) * (bx - ax), den = by - ay;
        if (den < 0) { num = -num; den = -den; }
        const int t = ax + (int)page_ceil_div(num, den);
        int k = n++;                                         // insertion sort into the row's slot
        while (k > 0 && thr[base + k - 1] > t) { thr[base + k] = thr[base + k - 1]; --k; }
        thr[base + k] = t;
    }
}

// inside iff an odd number of the row's thresholds are > x (the thresholds are sorted: a binary search)
__device__ __forceinline__ bool page_inside(const PageLine &L, const long long *__restrict__ row_start, const int *__restrict__ thr,
                                            int x, int y) {
    const int r = y - L.ymin;
    if (r < 0 || r >= L.nrows) return false;
    long long lo = row_start[L.row_off + r], hi = row_start[L.row_off + r + 1];
    const long long end = hi;
    while (lo < hi) {                                        // first threshold > x
        const long long mid = (lo + hi) >> 1;
        if (thr[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return ((end - lo) & 1) != 0;
}

__device__ __forceinline__ int page_pixel(const PageLine &L, const long long *__restrict__ row_start, const int *__restrict__ thr,
                                          int x, int y) {
    if (x < 0 || y < 0 || x >= L.pw || y >= L.ph) return L.fill;
    if (!page_inside(L, row_start, thr, x, y)) return L.fill;
    const unsigned char *p = L.page + ((size_t)y * L.pw + x) * L.cpp;
    if (L.cpp == 1) return p[0];
    return (p[0] * 19595 + p[1] * 38470 + p[2] * 7471 + 0x8000) >> 16;     // Pillow's RGB -> L, as pre_pixel
}

__global__ __launch_bounds__(256) void page_sample_kernel(const PageLine *__restrict__ lines, const long long *__restrict__ cols,
                                                          const long long *__restrict__ row_start, const int *__restrict__ thr,
                                                          unsigned char *__restrict__ out) {
    const PageLine L = lines[blockIdx.y];
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int r0 = blockIdx.z * PAGE_ROWS_PER_THREAD;
    if (c >= L.ws || r0 >= L.hs) return;
    const long long *cr = cols + 4 * (L.col_off + c);
    const long long bx = cr[0], by = cr[1], nx = cr[2], ny = cr[3];
    const int r1 = min(r0 + PAGE_ROWS_PER_THREAD, L.hs);
    unsigned char *o = out + L.out_off + c;
    for (int r = r0; r < r1; ++r) {
        const long long X = bx + (long long)(r - L.t) * nx, Y = by + (long long)(r - L.t) * ny;
        const long long xq = (X + 128) >> 8, yq = (Y + 128) >> 8;           // floor((v + 128) / 256): 1/256 px
        const int x0 = (int)(xq >> 8), y0 = (int)(yq >> 8), fx = (int)(xq & 255), fy = (int)(yq & 255);
        const int p00 = page_pixel(L, row_start, thr, x0, y0), p10 = page_pixel(L, row_start, thr, x0 + 1, y0);
        const int p01 = page_pixel(L, row_start, thr, x0, y0 + 1), p11 = page_pixel(L, row_start, thr, x0 + 1, y0 + 1);
        const int v = ((256 - fx) * (256 - fy) * p00 + fx * (256 - fy) * p10 + (256 - fx) * fy * p01 + fx * fy * p11 + 32768) >> 16;
        o[(size_t)r * L.ws] = (unsigned char)v;
    }
}
