// Training-time augmentation of a pre-processed line batch: the (N, H, W) uint8 batch cocr_preproc_lines
// leaves on the device -> a warped, blurred and dropped-out copy in a second buffer of the same shape.
//
// Every parameter is drawn on the host (conformer_ocr_amd/augment.py) and arrives in two DEVICE tables, so a launch never waits for
// the host: a per-line record of AUG_FIELDS int64 (seq_len, stage flags, the inverse affine map in 1/65536 px, blur kind / length /
// direction, the dropout threshold and hash key) and a per-line control grid of (dx, dy, shear) int32 triples every 32 columns.
//
// One workgroup per (tile of AUG_TW columns x AUG_TH rows, line):
//   1. the warped tile plus a halo of AUG_HALO pixels goes to LDS: pixel (r, c) of the line is the integer bilinear sample (1/256 px
//      weights, +32768 >> 16, as the page sampler) of the input at the mapped position; anything outside [0, H) x [0, seq_len)
//      of the input or of the output counts as 0 (the collation's padding);
//   2. from LDS: 3x3 box, 3x3 median or a motion blur of length 3 / 5 / 7 along one of four directions, then pixel dropout by a
//      splitmix64 hash of (key, r, c); a thread owns 8 consecutive columns of a row and writes them with one 8-byte store.
// Columns >= seq_len are copied unchanged; a line with no stage on is copied.  Integer only: no floating-point contraction can make
// the device differ from tests/augment_ref.py.
#pragma once
#include "common.hip.h"

static constexpr int AUG_FIELDS = 16;
static constexpr int AUG_TW = 64, AUG_TH = 32, AUG_HALO = 3;
static constexpr int AUG_LW = AUG_TW + 2 * AUG_HALO, AUG_LH = AUG_TH + 2 * AUG_HALO;
static constexpr int AUG_GRID_STEP = 32;                                   // control columns every 32 px
enum { AUG_F_SEQ = 0, AUG_F_FLAGS = 1, AUG_F_A = 2, AUG_F_BLUR = 8, AUG_F_MLEN = 9, AUG_F_MDIR = 10, AUG_F_DROP = 11, AUG_F_KEY = 12 };
enum { AUG_GEOM = 1, AUG_ELASTIC = 2, AUG_BLUR = 4, AUG_DROPOUT = 8 };

// floor(n / d), d > 0
__device__ __forceinline__ long long aug_floor_div(long long n, long long d) { return n >= 0 ? n / d : -((-n + d - 1) / d); }

__device__ __forceinline__ unsigned long long aug_mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the counter-based hash of augment.py: splitmix64's output for state key + (x + 1) * golden
__device__ __forceinline__ unsigned long long aug_hash(unsigned long long key, unsigned long long x) {
    return aug_mix64(key + (x + 1ull) * 0x9E3779B97F4A7C15ull);
}

__device__ __forceinline__ int aug_px(const unsigned char *__restrict__ img, int W, int H, int sl, long long x, long long y) {
    return (x >= 0 && x < sl && y >= 0 && y < H) ? (int)img[(size_t)y * W + (size_t)x] : 0;
}

__device__ __forceinline__ void aug_cswap(int &a, int &b) { const int lo = min(a, b), hi = max(a, b); a = lo; b = hi; }

// 5th smallest of 9 (a fixed exchange network: no indexed arrays, nothing leaves the registers)
__device__ __forceinline__ int aug_median9(int p0, int p1, int p2, int p3, int p4, int p5, int p6, int p7, int p8) {
    aug_cswap(p1, p2); aug_cswap(p4, p5); aug_cswap(p7, p8); aug_cswap(p0, p1); aug_cswap(p3, p4); aug_cswap(p6, p7);
    aug_cswap(p1, p2); aug_cswap(p4, p5); aug_cswap(p7, p8); aug_cswap(p0, p3); aug_cswap(p5, p8); aug_cswap(p4, p7);
    aug_cswap(p3, p6); aug_cswap(p1, p4); aug_cswap(p2, p5); aug_cswap(p4, p7); aug_cswap(p4, p2); aug_cswap(p6, p4);
    aug_cswap(p4, p2);
    return p4;
}

__global__ __launch_bounds__(256) void augment_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out,
                                                      const long long *__restrict__ params, const int *__restrict__ grid, int G, int H,
                                                      int W) {
    __shared__ unsigned char tile[AUG_LH][AUG_LW + 2];
    const int n = blockIdx.z, c0 = blockIdx.x * AUG_TW, r0 = blockIdx.y * AUG_TH, tid = threadIdx.x;
    const long long *P = params + (size_t)n * AUG_FIELDS;
    const int sl = (int)min(max(P[AUG_F_SEQ], 0ll), (long long)W);
    const int flags = (int)P[AUG_F_FLAGS] & 15;
    const unsigned char *src = in + (size_t)n * H * W;
    unsigned char *dst = out + (size_t)n * H * W;
    const int rr = tid >> 3, cb = (tid & 7) * 8;                          // this thread's 8 output pixels of the tile
    const int r = r0 + rr, cs = c0 + cb;
    const bool vec = (W & 7) == 0 && cs + 8 <= W;                         // 8-byte aligned and inside the row

    if (flags == 0 || c0 >= sl) {                                         // copy
        if (r >= H || cs >= W) return;
        const size_t o = (size_t)r * W + cs;
        if (vec) *reinterpret_cast<uint2 *>(dst + o) = *reinterpret_cast<const uint2 *>(src + o);
        else for (int k = 0; k < 8 && cs + k < W; ++k) dst[o + k] = src[o + k];
        return;
    }
    const bool warp = (flags & (AUG_GEOM | AUG_ELASTIC)) != 0, blur = (flags & AUG_BLUR) != 0;
    const int kind = blur ? (int)P[AUG_F_BLUR] : 0;
    const int halo = blur ? AUG_HALO : 0;
    // ---- 1. warped values of the tile (+ halo) into LDS
    const long long a0 = P[AUG_F_A], a1 = P[AUG_F_A + 1], a2 = P[AUG_F_A + 2], a3 = P[AUG_F_A + 3], a4 = P[AUG_F_A + 4], a5 = P[AUG_F_A + 5];
    const bool geom = (flags & AUG_GEOM) != 0, elastic = (flags & AUG_ELASTIC) != 0;
    const int *g = grid + (size_t)n * G * 3;
    const int lh = AUG_TH + 2 * halo, lw = AUG_TW + 2 * halo;
    for (int i = tid; i < lh * lw; i += 256) {
        const int tr = i / lw, tc = i - tr * lw;
        const int y = r0 - halo + tr, x = c0 - halo + tc;
        int v = 0;
        if (y >= 0 && y < H && x >= 0 && x < sl) {
            if (!warp) {
                v = src[(size_t)y * W + x];
            } else {
                long long X = (long long)x << 16, Y = (long long)y << 16;
                if (geom) {
                    X = a0 * x + a1 * y + a2;
                    Y = a3 * x + a4 * y + a5;
                }
                if (elastic) {
                    const int j = x >> 5, t = x & 31;
                    const int *g0 = g + 3 * j, *g1 = g0 + 3;
                    const long long dx = ((long long)g0[0] * (32 - t) + (long long)g1[0] * t) >> 5;
                    const long long dy = ((long long)g0[1] * (32 - t) + (long long)g1[1] * t) >> 5;
                    const long long sh = ((long long)g0[2] * (32 - t) + (long long)g1[2] * t) >> 5;
                    X += dx + aug_floor_div(sh * (2 * y - H + 1), H);
                    Y += dy;
                }
                const long long Xq = (X + 128) >> 8, Yq = (Y + 128) >> 8;
                const long long x0 = Xq >> 8, y0 = Yq >> 8;
                const int fx = (int)(Xq & 255), fy = (int)(Yq & 255);
                const int p00 = aug_px(src, W, H, sl, x0, y0), p10 = aug_px(src, W, H, sl, x0 + 1, y0);
                const int p01 = aug_px(src, W, H, sl, x0, y0 + 1), p11 = aug_px(src, W, H, sl, x0 + 1, y0 + 1);
                v = ((256 - fx) * (256 - fy) * p00 + fx * (256 - fy) * p10 + (256 - fx) * fy * p01 + fx * fy * p11 + 32768) >> 16;
            }
        }
        tile[tr][tc] = (unsigned char)v;
    }
    __syncthreads();
    if (r >= H || cs >= W) return;
    // ---- 2. filter + dropout from LDS, 8 columns per thread
    const int mlen = (int)P[AUG_F_MLEN], mdir = (int)P[AUG_F_MDIR];
    const int mdx = mdir == 1 ? 0 : 1, mdy = mdir == 0 ? 0 : (mdir == 3 ? -1 : 1);
    const bool drop = (flags & AUG_DROPOUT) != 0;
    const unsigned thr = (unsigned)min(max(P[AUG_F_DROP], 0ll), 65536ll);
    const unsigned long long key = (unsigned long long)P[AUG_F_KEY];
    const size_t o = (size_t)r * W + cs;
    unsigned char px[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = cs + k;
        int v;
        if (c >= W) {
            v = 0;
        } else if (c >= sl) {
            v = src[o + k];
        } else {
            const int ty = rr + halo, tx = cb + k + halo;
            v = tile[ty][tx];
            if (kind == 1 || kind == 2) {
                const int q0 = tile[ty - 1][tx - 1], q1 = tile[ty - 1][tx], q2 = tile[ty - 1][tx + 1];
                const int q3 = tile[ty][tx - 1], q5 = tile[ty][tx + 1];
                const int q6 = tile[ty + 1][tx - 1], q7 = tile[ty + 1][tx], q8 = tile[ty + 1][tx + 1];
                v = kind == 1 ? (q0 + q1 + q2 + q3 + v + q5 + q6 + q7 + q8 + 4) / 9 : aug_median9(q0, q1, q2, q3, v, q5, q6, q7, q8);
            } else if (kind == 3 && (mlen == 3 || mlen == 5 || mlen == 7)) {
                const int h = mlen >> 1;
                int s = 0;
                for (int d = -h; d <= h; ++d) s += tile[ty + d * mdy][tx + d * mdx];
                v = (s + h) / mlen;
            }
            if (drop && (unsigned)(aug_hash(key, ((unsigned long long)r << 16) + (unsigned long long)c) >> 48) < thr) v = 0;
        }
        px[k] = (unsigned char)v;
    }
    if (vec) {
        uint2 w;
        w.x = px[0] | (px[1] << 8) | (px[2] << 16) | ((unsigned)px[3] << 24);
        w.y = px[4] | (px[5] << 8) | (px[6] << 16) | ((unsigned)px[7] << 24);
        *reinterpret_cast<uint2 *>(dst + o) = w;
    } else {
        for (int k = 0; k < 8 && cs + k < W; ++k) dst[o + k] = px[k];
    }
}
