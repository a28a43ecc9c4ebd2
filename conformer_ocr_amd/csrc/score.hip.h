// Batched edit-distance alignment for the CER / WER scoring and the confusion report: P pairs of int32 symbol
// sequences (a = ground truth, b = prediction) -> per pair (distance, insertions, deletions, substitutions) and, when asked for, the
// alignment itself.  The definition is evaluate.global_align: unit costs, cost[i][0] = i, cost[0][j] = j, and a traceback from (n, m) that
// prefers the diagonal step when cost[i][j] == cost[i-1][j-1] + (a[i-1] != b[j-1]), else the deletion when cost[i][j] == cost[i-1][j] + 1,
// else the insertion.  That choice is local to a cell, so the cell's op code (2 bits) is written while the costs are computed and the
// traceback never sees a cost: 0 equal, 1 substitution, 2 deletion (a symbol of a against a gap), 3 insertion (a gap against a symbol of b).
//
// One wave per pair.  Columns of b in blocks of 64, lane l owning column j0 + l + 1; the rows are skewed so that the cells of an
// anti-diagonal are computed together: at step s lane l computes row i = s - l + 1.  A lane keeps its own two last costs
// (cost[i-1][j] and cost[i-2][j]) packed in one register (a cost is at most 4096); its left neighbour's pair, one lane shift away, is
// (cost[i][j-1], cost[i-1][j-1]).  The symbol of a travels along the lanes the same way (lane 0 takes a[s] from a 64-symbol chunk the wave
// loads every 64 steps).  The last column of a block goes to a carry column in LDS, which lane 0 of the next block reads in chunks of 64
// rows; the writes of a block trail the next chunk's reads by 63 rows, so one column serves both.
// Op codes: a lane packs 16 consecutive rows of its column into one word, dir[(j - 1) * ceil(n / 16) + (i - 1) / 16] -- in LDS when the
// pair's table fits the launch's budget (DIR_LDS), else in the workgroup's region of a global workspace (same code).
// Traceback: every lane walks the same chain (uniform addresses: one broadcast read per step, a packed word serving a whole run of
// deletions); lane 0 writes the ops backwards from the end of the pair's slot, so the alignment ends up in forward order in the LAST
// ops_len[p] bytes of the slot.  Every loop is bounded by n, m or n + m; nothing waits on another workgroup.
#pragma once
#include "common.hip.h"

static constexpr int SCORE_MAX_LEN = 4096;                 // symbols per sequence (a cost fits 16 bits)

// dynamic LDS of one pair: the carry column (n + 1 costs, padded to 16 bytes), then the op-code table when it lives in LDS
__host__ __device__ static inline size_t score_carry_bytes(int n) { return ((size_t)(n + 1) * 4 + 15) & ~(size_t)15; }
__host__ __device__ static inline size_t score_dir_words(int n, int m) { return (size_t)m * (size_t)((n + 15) / 16); }

template <bool DIR_LDS>
__global__ __launch_bounds__(64) void edit_align_kernel(const int *__restrict__ a_all, const int *__restrict__ b_all,
                                                        const long long *__restrict__ a_offs, const long long *__restrict__ b_offs,
                                                        const int *__restrict__ order, int count, int *__restrict__ counts,
                                                        unsigned char *__restrict__ ops, int *__restrict__ ops_len,
                                                        unsigned *__restrict__ ws, size_t ws_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char score_lds[];
    const int lane = threadIdx.x;
    for (int k = blockIdx.x; k < count; k += gridDim.x) {
        const int p = order[k];
        const long long a0 = a_offs[p], b0 = b_offs[p];
        const int n = (int)(a_offs[p + 1] - a0), m = (int)(b_offs[p + 1] - b0);
        const int *a = a_all + a0, *b = b_all + b0;
        int *carry = reinterpret_cast<int *>(score_lds);
        unsigned *dir = DIR_LDS ? reinterpret_cast<unsigned *>(score_lds + score_carry_bytes(n)) : ws + (size_t)blockIdx.x * ws_stride;
        const int rw = (n + 15) >> 4;                                    // words per column of the op-code table

        // ---- costs and op codes, one block of 64 columns after the other
        for (int j0 = 0; j0 < m && n > 0; j0 += 64) {
            const int W = min(64, m - j0);                               // columns of this block
            const bool last = j0 + 64 >= m;
            const int j = j0 + lane + 1;
            const bool col = lane < W;
            const int bj = col ? b[j - 1] : 0;
            unsigned pair = (unsigned)j << 16;                           // (cost[i-1][j] << 16) | cost[i-2][j]; row 0: cost[0][j] = j
            unsigned acc = 0;                                            // op codes of up to 16 rows of column j
            int ai = 0, a_chunk = 0, c_chunk = 0;
            int diag0 = j0;                                              // lane 0: cost[i-1][j0]
            const int steps = n + W - 1;
            for (int s = 0; s < steps; ++s) {
                if ((s & 63) == 0) {                                     // the next 64 symbols of a and rows of the carry column
                    __syncthreads();                                     // (one wave: orders the carry column's writes before these reads)
                    a_chunk = s + lane < n ? a[s + lane] : 0;
                    const int r = s + 1 + lane;
                    c_chunk = r <= n ? (j0 ? carry[r] : r) : 0;
                }
                const unsigned left_pair = __shfl_up(pair, 1);
                const int a_left = __shfl_up(ai, 1);
                const int a_new = __shfl(a_chunk, s & 63), left0 = __shfl(c_chunk, s & 63);
                ai = lane == 0 ? a_new : a_left;
                const int left = lane == 0 ? left0 : (int)(left_pair >> 16);
                const int diag = lane == 0 ? diag0 : (int)(left_pair & 0xffffu);
                diag0 = left0;
                const int i = s - lane + 1;
                if (col && i >= 1 && i <= n) {
                    const int up = (int)(pair >> 16);
                    const int neq = ai != bj;
                    const int cd = diag + neq, cu = up + 1;
                    const int c = min(cd, min(cu, left + 1));
                    const unsigned code = c == cd ? (unsigned)neq : (c == cu ? 2u : 3u);
                    pair = ((unsigned)c << 16) | (unsigned)up;
                    acc |= code << (2 * ((i - 1) & 15));
                    if (((i - 1) & 15) == 15 || i == n) {
                        dir[(size_t)(j - 1) * rw + ((i - 1) >> 4)] = acc;
                        acc = 0;
                    }
                    if (!last && lane == 63) carry[i] = c;
                }
            }
        }
        __syncthreads();
        if (!DIR_LDS) __threadfence();                                   // the workspace words written above are read below

        // ---- traceback (uniform over the wave; lane 0 writes)
        int i = n, j = m, n_ins = 0, n_del = 0, n_sub = 0, pos = n + m;
        unsigned char *slot = ops ? ops + ((a0 - a_offs[0]) + (b0 - b_offs[0])) : nullptr;   // pair p's n + m bytes follow the earlier pairs'
        unsigned word = 0;
        long long have = -1;
        while (i > 0 || j > 0) {
            unsigned code;
            if (i == 0) code = 3u;
            else if (j == 0) code = 2u;
            else {
                const long long key = (long long)(j - 1) * rw + ((i - 1) >> 4);
                if (key != have) { word = dir[key]; have = key; }
                code = (word >> (2 * ((i - 1) & 15))) & 3u;
            }
            --pos;
            if (slot && lane == 0) slot[pos] = (unsigned char)code;
            if (code <= 1u) { --i; --j; n_sub += (int)code; }
            else if (code == 2u) { --i; ++n_del; }
            else { --j; ++n_ins; }
        }
        if (lane == 0) {
            *reinterpret_cast<int4 *>(counts + 4 * (size_t)p) = make_int4(n_ins + n_del + n_sub, n_ins, n_del, n_sub);
            if (ops_len) ops_len[p] = n + m - pos;
        }
        __syncthreads();                                                 // the next pair of this workgroup reuses the LDS
    }
}
