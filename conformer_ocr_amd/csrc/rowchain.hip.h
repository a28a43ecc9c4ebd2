// Row-local chains of a conformer block in ONE kernel (bf16; encoder_dim 256 or 512).
//
// Everything in a block except the attention core (needs all frames of a line) maps a row of the (M, D) activation to a row:
// projections, feed-forward modules, residual adds, LayerNorms, and -- with a +-15 frame halo -- the depthwise conv.  A workgroup
// that owns a block of rows therefore runs a whole sequence of them back to back:
//     first chain (block 0):                 frontend output linear (K = F C, + LayerNorm)  ->  FFN 1 (+ residual + LayerNorm)  ->  q/k/v projection
//     chain A (after the attention core):    out-proj + residual + LayerNorm  ->  pointwise conv 1 + GLU
//     chain B (after the GLU):               depthwise conv + BatchNorm + SiLU  ->  pointwise conv 2 + residual + LayerNorm  ->  FFN 2
//                                            (+ block-final LayerNorm + next block's LayerNorm)  ->  next block's FFN 1 (+ LayerNorm)
//                                            ->  its q/k/v projection
// Chain A is row-local throughout, and chain B needs it only for its own rows and the depthwise conv's +-15 frames around them: at 64, 48 and
// 32 rows (D = 256, conv kernel 31) chain A runs as the HEAD of chain B's launch, on the workgroup's rows plus one 16-row tile on either
// side (template parameters H0, H1 below) -- one launch less per block, the GLU output and the stream between the two never in memory.
// Reference lines: attention.py:70,103 (out_proj), convolution.py:138-143 (pointwise convs, GLU, depthwise conv, BatchNorm, SiLU),
// feed_forward.py:45-52, modules.py:32 (residual), encoder.py:62-99.
//
// Machinery:
//   * 8 waves; the workgroup owns BMC = 16 MT rows (MT = 6: 96 rows, the throughput form; fewer rows = more workgroups for small
//     batches / one batch in flight).  Every product is computed with the WEIGHTS on the MFMA row side: accumulator register q of
//     lane (r16 = lane & 15, g = lane >> 4) of tile (i, j) is out[row 16 i + r16][column 32 wave + 16 j + 4 g + q] of a 256-column
//     step, i.e. a lane holds 4 consecutive output columns of one activation row.
//   * weights stream L2 -> REGISTERS from a fragment-major copy (pack_frag_kernel: [n/32][k/32][2][64 lanes][8]): the 16 B-fragments
//     of one step (32 output columns x 256 k) are one contiguous 16 KiB run per wave, requested one step ahead through a 16-fragment
//     register ring (the compiler's vmcnt bookkeeping orders it).
//   * activations are MFMA operands read from swizzled LDS images ([k/64 panels][rows][128 B]): the D-wide operand rows and, for the
//     FFN, two 256-wide hidden-chunk images (software pipeline: bias + SiLU of chunk c folded into the k-steps of the second
//     product of chunk c-1).
//   * THE RESIDUAL STREAM LIVES IN THE ACCUMULATORS: x (fp32) is loaded once per launch in the accumulator layout and is the C operand
//     of every stage's product (x + bias as the initial accumulator; the half-step factor of the FFN is folded into the packed copy of
//     its second matrix), so the residual add costs nothing and x never round-trips through memory inside a launch.
//   * LayerNorm straight from those registers: per-lane partial sums (8 or 16 values per row) -> two lane-swap butterflies
//     (v_permlane32_swap / v_permlane16_swap) -> per-wave partials in LDS -> one barrier -> every lane sums the 8 waves' partials of
//     its rows; the normalised values go straight into the operand image as bf16.  (The first version staged the fp32 tile in LDS,
//     re-read x from global in a row-per-16-lanes layout and wrote x back after every stage: 3 round trips of the stream per launch.)
#pragma once
#include <type_traits>

#include "gemm.hip.h"
#include "rowchain_args.hip.h"

#ifndef COCR_STAMP_WG
#define COCR_STAMP_WG 7        // dev (stamps build): the workgroup whose phase boundaries are stamped
#endif

// Lane-swap butterflies (gfx950).  v_permlane32_swap a, b: a <- [a.lo32, b.lo32], b <- [a.hi32, b.hi32]; v_permlane16_swap a, b (rows of 16
// lanes r0..r3): a <- [a.r0, b.r0, a.r2, b.r2], b <- [a.r1, b.r1, a.r3, b.r3].  Inline asm: the builtin's two results come back as ONE register when
// both are consumed by a floating-point add (hipcc 7.2: `v_add_f32 v1, v1, v1`); the s_nop covers the VALU-write -> permlane-read hazard.
__device__ __forceinline__ void swap32(float &a, float &b) { asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ void swap16(float &a, float &b) { asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b)); }
// four per-lane values a, b, c, d, each to be summed over the lanes {l, l^16, l^32, l^48}: returns ONE register whose 16-lane row rho holds
// the total of {a, c, b, d}[rho]
__device__ __forceinline__ float butterfly4(float a, float b, float c, float d) {
    swap32(a, b);
    swap32(c, d);
    float ab = a + b, cd = c + d;          // ab: [sum over halves of a | of b]
    swap16(ab, cd);
    return ab + cd;                        // rows: a, c, b, d
}

// slack behind the two hidden-chunk images (the q / k / v output tiles' padded rows reach into it)
constexpr size_t ROWCHAIN_SLACK = 4096;
// channels per pass of the depthwise prologue (window + taps of that many channels in LDS at a time)
constexpr int ROWCHAIN_DW_PASS = 256;
// operand image + hidden images + slack.  HEAD (the out-proj -> GLU head in front of the depthwise prologue): the head's operand image of
// MT + 2 row tiles and, BEHIND it (the GLU epilogue writes window rows while other waves still read the image), the GLU window of the
// same rows ([row][2 D bytes]) alias that area; where they need more (48 and 32 rows) the area grows.
template <int D, int MT, bool HEAD = false> constexpr size_t rowchain_area_bytes() {
    constexpr size_t imgx = (size_t)(D / 64) * 16 * MT * 128, area = imgx + 2 * 4 * (size_t)(16 * MT) * 128 + ROWCHAIN_SLACK;
    constexpr size_t harea = (size_t)(D / 64) * 16 * (MT + 2) * 128 + (size_t)16 * (MT + 2) * 2 * D;
    return HEAD && harea > area ? harea : area;
}
template <int D, int MT, bool HEAD = false> constexpr size_t rowchain_lds_bytes() {
    return rowchain_area_bytes<D, MT, HEAD>() + 16 * (size_t)D + 12 * (size_t)(16 * MT) + 64;
}
// Where the depthwise taps of a channel pass ((DWK + 1) rows of floats) are staged in LDS: 1 = behind the window inside the hidden-image
// area, 2 = in an area of their own behind everything else, 0 = nowhere (no room: every thread loads its own taps from global memory)
template <int D, int MT, int DWK> constexpr int rowchain_taps_place() {
    if (DWK == 0 || (DWK + 1) % 8 != 0) return 0;
    constexpr size_t cw = ROWCHAIN_DW_PASS, rpi = 64 / (cw / 8);
    constexpr size_t hsb = 2 * 4 * (size_t)(16 * MT) * 128 + ROWCHAIN_SLACK, win = ((16 * MT + DWK - 1 + rpi - 1) / rpi) * 1024, taps = (size_t)(DWK + 1) * cw * 4;
    if (win + taps <= hsb) return 1;
    if (rowchain_lds_bytes<D, MT>() + taps <= 160 * 1024) return 2;
    return 0;
}

// KD / KL: zero-padded narrow models (cocr_api.hip: set_engine_dims) -- the k-steps (32 k each) of a K = D product and of the FFN's LAST
// hidden chunk that hold real columns; the k-steps beyond them multiply zeros and are skipped (their weight fragments are still streamed:
// the ring's bookkeeping stays one shape).  8 / 8 = nothing skipped.  The reference's default model (encoder_dim 144, feed-forward 576 in
// a 256 / 768-wide engine): 5 / 2.
//
// H0 / H1: the HEAD of a depthwise-prologue chain (ST_ROWLN, ST_GLU = ChainArgs::st[4], st[5]; -1 = none): what used to be the launch in front
// of it -- out-proj + residual + conv-module LayerNorm -> pointwise conv 1 + GLU -- computed by the workgroup itself for its own rows AND one
// 16-row tile on either side (MT + 2 row tiles), which is all the depthwise conv's +-15-frame halo needs (16, not 15: in the blocked stream
// layout the halo tiles are whole tiles of the neighbouring row blocks).  The GLU values go straight into the depthwise window in LDS and
// the stream of the own rows stays in the accumulators from the attention residual to the end of the launch.  Every row's values are
// computed with the arithmetic of the stand-alone launch, whichever workgroup computes them: bit-identical.  Halo rows outside [0, M)
// (clamped addresses, a clamped neighbour block) and frames of other lines hold values no tap reads (the tap range, `tpos`).
template <int D, int MT, int DWK, int K0, int K1, int K2, int K3, bool TAPS, int KD = 8, int KL = 8, int H0 = -1, int H1 = -1>
__global__ __launch_bounds__(512, 2) void rowchain_kernel(ChainArgs p) {
    typedef bf16_t T;
    constexpr bool HEAD = H0 >= 0;
    constexpr int ME = MT + 2;                 // row tiles of the head
    static_assert(!HEAD || (H0 == ST_ROWLN && H1 == ST_GLU && K0 == ST_ROWLN && DWK == 31 && D == 256 && ME <= 6), "head: out-proj -> GLU in front of the 31-tap prologue, 256 wide, at most 6 row tiles");
    static_assert(D == 256 || D == 512, "encoder_dim of the row-chain kernels");
    static_assert(MT >= 2 && MT <= 6, "16-row tiles per workgroup");
    static_assert(KD >= 1 && KD <= 8 && KL >= 1 && KL <= 8 && (D == 256 || (KD == 8 && KL == 8)), "skipped k-steps: the 256-wide engine only");
    typedef std::integral_constant<int, 8> KK8;
    typedef std::integral_constant<int, KD> KKD;           // K = D products
    typedef std::integral_constant<int, KL> KKL;           // the second product of the FFN's last hidden chunk
    // the ROWLN stage of the out-proj -> GLU chain multiplies the attention context, whose real columns sit in head slots all over the
    // padded width ([64 h, 64 h + d_head)): no k-step of it is all zeros
    typedef std::integral_constant<int, (K1 == ST_GLU) ? 8 : KD> KKR;
    constexpr int BMC = 16 * MT;
    constexpr int KS = D / 256;                // 256-deep k slices of a K = D product
    constexpr int NS = D / 256;                // 256-column steps of an N = D product
    constexpr int NJ = 2 * NS;                 // 16-column tiles of this wave per row tile of an N = D product
    constexpr int PANEL = BMC * 128;           // one [rows][128 B] panel of an operand image (64 bf16 of k per row)
    constexpr int IMGX = (D / 64) * PANEL;     // BMC x D bf16
    constexpr int IMGH = 4 * PANEL;            // BMC x 256 bf16 (hidden chunk)
    constexpr int OS = 256 * 2 + 16;           // bf16 staged row of a 256-column output tile (q / k / v)
    constexpr int OSD = D * 2 + 16;            // bf16 staged row of a D-column output tile (GLU)
    constexpr int SLICE = 16 * 512;            // elements in one step's weight run (16 fragments)
    constexpr int PROW = 80;                   // LayerNorm partials: 8 waves x (sum, sum of squares) per row, padded 64 -> 80 bytes (the 16 rows a
                                               // ds_read_b128 lane group touches then fall on 16 different bank quads)
    constexpr int HSB = 2 * IMGH + (int)ROWCHAIN_SLACK;     // hidden images + slack (output tiles, depthwise window, LayerNorm partials alias them)
    constexpr int AREA = (int)rowchain_area_bytes<D, MT, HEAD>();            // = IMGX + HSB, or what the head's image + window need
    constexpr int PANELE = 16 * ME * 128, IMGE = (D / 64) * PANELE;          // head: its operand image (ME tiles) at xa
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *xa = smem;                  // operand image
    unsigned char *hs = smem + IMGX;           // 2 hidden-chunk images
    float *lnp = reinterpret_cast<float *>(smem + AREA);                           // LayerNorm parameters of the running stage: g1, b1, g2, b2 (4 x D floats)
    long long *rowoff = reinterpret_cast<long long *>(smem + AREA + 16 * D);   // row -> offset of its (line, frame) in the q / k / v layouts
    int *tpos = reinterpret_cast<int *>(smem + AREA + 16 * D + 8 * BMC);      // frame index of each row inside its line

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4, swz = r16 & 7;
    // XCD-aware order (p.xcd_order): hardware workgroup ids go round the 8 XCDs; the row block a workgroup owns is chosen so that each XCD
    // holds a contiguous range of row blocks, i.e. of lines -- the same lines whose (line, head) workgroups the attention kernels put on that
    // XCD: what one launch writes (context rows, GLU output, stream, q / k / v) the next one reads from the same L2
    const int rblk = p.xcd_order ? xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int M = p.M, m0 = rblk * BMC, mend = min(M, m0 + BMC);
    const int lrow = lane >> 3, cpos = lane & 7;
#ifdef COCR_CHAIN_STAMPS_BUILD
    int sk = 0;
#define RSTAMP() { if (p.stamps && rblk == COCR_STAMP_WG && lane == 0) p.stamps[wave * 64 + sk] = __builtin_readcyclecounter(); ++sk; }
#else
#define RSTAMP()
#endif
    RSTAMP()                                       // 0: start
    auto lds_fence_barrier = [&]() {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };

    constexpr int DWPAD = DWK ? (DWK - 1) / 2 : 0, DWROWS = BMC + 2 * DWPAD;
    constexpr int CW = ROWCHAIN_DW_PASS;                   // channels per pass of the depthwise prologue
    constexpr int WS = CW * 2;                 // bytes per window row
    constexpr int LPR = CW / 8, RPI = 64 / LPR;            // lanes per window row (16 B each), window rows per wave-instruction
    constexpr int WINB = ((DWROWS + RPI - 1) / RPI) * 1024;
    static_assert(DWK == 0 || (size_t)WINB <= (size_t)HSB, "depthwise window (CW channels at a time) must fit the hidden-image area");
    static_assert((size_t)BMC * OSD <= (size_t)HSB && 2 * (size_t)BMC * OS <= (size_t)HSB, "output tiles alias the hidden-image area");
    // head: the GLU window of the ME tiles' rows m0 - 16 .. m0 + BMC + 15 lies behind the head's operand image; row 0 of the depthwise window
    // (m0 - PAD) is its row 1
    unsigned char *winx = smem + IMGE;
    static_assert(!HEAD || (IMGE >= IMGX && IMGE + 16 * ME * WS <= AREA && CW == D && DWPAD == 15), "head: window behind both operand images");
    const unsigned char *win = HEAD ? winx + (16 - DWPAD) * WS : hs;
    // head: the attention context of the ME tiles' rows -> operand image (addresses clamped to [0, M)); ME wave-instructions per wave
    auto head_dma = [&]() {
#pragma unroll
        for (int u = 0; u < (D / 64) * ME / 4; ++u) {
            const int id = wave + 8 * u, pnl = id / (2 * ME), rg = id - pnl * (2 * ME), row = rg * 8 + lrow;
            const T *src = p.A0 + (size_t)min(max(m0 - 16 + row, 0), M - 1) * D + pnl * 64 + ((cpos ^ (row & 7)) * 8);
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(xa + pnl * PANELE + rg * 1024), 16, 0, 0);
        }
    };
    // depthwise window of channel pass `h`: rows m0 - PAD .. m0 + BMC + PAD - 1 of the GLU output (addresses clamped; frames outside the row's
    // own line are excluded by the tap range below), [row][WS bytes] at hs: one wave-instruction = RPI rows
    auto dw_window = [&](int h) {
        for (int q2 = wave; q2 < WINB / 1024; q2 += 8) {
            const int j = RPI * q2 + lane / LPR, mrow = min(max(m0 - DWPAD + j, 0), M - 1);
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(p.dw_in + (size_t)mrow * D + h * CW + (lane % LPR) * 8), (lds_ptr_t)(hs + q2 * 1024), 16, 0, 0);
        }
    };
    // FRONT (first stage = the frontend's output linear, K = F C): its (BMC x 256)-deep operand slices go through the two hidden-image areas,
    // double buffered, MT wave-instructions per wave and slice (4 panels x BMC / 8 row groups of 8 rows x 128 B)
    constexpr bool FRONT0 = K0 == ST_FRONT;
    static_assert(!FRONT0 || DWK == 0, "the output linear starts a launch");
    static_assert(K1 != ST_FRONT && K2 != ST_FRONT && K3 != ST_FRONT, "FRONT is a first stage");
    auto front_dma = [&](int ks) {
        unsigned char *buf = hs + (ks & 1) * IMGH;
        const int Kf = p.st[0].K;
#pragma unroll
        for (int u = 0; u < MT; ++u) {
            const int id = wave + 8 * u, pnl = id / (BMC / 8), rg = id - pnl * (BMC / 8), row = rg * 8 + lrow;
            const T *src = p.A0 + (size_t)min(m0 + row, M - 1) * Kf + ks * 256 + pnl * 64 + ((cpos ^ (row & 7)) * 8);
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(buf + pnl * PANEL + rg * 1024), 16, 0, 0);
        }
    };
    static_assert(4 * (BMC / 8) == 8 * MT, "operand slice: MT wave-instructions per wave");
    if constexpr (FRONT0) {
        front_dma(0);
    } else if constexpr (DWK == 0) {
        // ---- first operand tile -> LDS image: (D / 64) panels x BMC / 8 row groups of 8 rows, one wave-instruction each
        for (int id = wave; id < (D / 64) * (BMC / 8); id += 8) {
            const int pnl = id / (BMC / 8), rg = id - pnl * (BMC / 8), row = rg * 8 + lrow;
            const T *src = p.A0 + (size_t)min(m0 + row, M - 1) * D + pnl * 64 + ((cpos ^ (row & 7)) * 8);
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(xa + pnl * PANEL + rg * 1024), 16, 0, 0);
        }
    } else if constexpr (HEAD) {
        head_dma();
    } else {
        dw_window(0);
    }
    // depthwise taps and bias of a channel half: DWK + 1 rows of 256 floats behind the window in LDS, one DMA each, requested with the window
    // and ahead of the weight ring (loads return in order: behind the ring they would wait for all of it).  Every thread then reads its
    // channel pair's taps from there.  (Each thread loading its own taps from global memory -- 32 eight-byte loads, the same 32 KB four times
    // per workgroup -- made 68 loads per wave at the kernel's start, more than the 63 a wave can have outstanding: the prologue started
    // 16 k cycles into the launch.)
    typedef float dw_f32x2 __attribute__((ext_vector_type(2)));
    dw_f32x2 dw_wt[DWK ? DWK : 1], dw_bias = {0.f, 0.f};
    constexpr int TAPLACE = rowchain_taps_place<D, MT, DWK>();
    static_assert(!HEAD || TAPLACE == 2, "head: the taps in their own area (the window is the head's to write)");
    unsigned char *tapa = TAPLACE == 1 ? hs + WINB : smem + rowchain_lds_bytes<D, MT, HEAD>();
    constexpr int TPI = 256 / CW;                  // tap rows (CW floats) per wave-instruction
    auto dw_taps = [&](int h) {
        if constexpr (DWK != 0 && TAPLACE != 0) {
#pragma unroll
            for (int r2 = wave; r2 < (DWK + 1) / TPI; r2 += 8) {           // (DWK + 1) % 8 == 0: the same number of requests in every wave
                const int r = r2 * TPI + lane / (64 / TPI);
                const float *src = (r < DWK ? p.dw_w + (size_t)r * D : p.dw_b) + h * CW + (lane % (64 / TPI)) * 4;
                __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(tapa + r2 * 1024), 16, 0, 0);
            }
        } else if constexpr (DWK != 0) {
            const int c = h * CW + 2 * (tid % (CW / 2));
#pragma unroll
            for (int tau = 0; tau < DWK; ++tau) dw_wt[tau] = *reinterpret_cast<const dw_f32x2 *>(p.dw_w + (size_t)tau * D + c);
            dw_bias = *reinterpret_cast<const dw_f32x2 *>(p.dw_b + c);
        }
    };
    auto dw_taps_read = [&]() {                    // after the barrier that publishes the window and the taps
        if constexpr (DWK != 0 && TAPLACE != 0) {
            const unsigned char *tb = tapa + (tid % (CW / 2)) * 8;
#pragma unroll
            for (int tau = 0; tau < DWK; ++tau) dw_wt[tau] = *reinterpret_cast<const dw_f32x2 *>(tb + tau * (CW * 4));
            dw_bias = *reinterpret_cast<const dw_f32x2 *>(tb + DWK * (CW * 4));
        }
    };
    RSTAMP()                                       // window / operand tile requested
    dw_taps(0);
    RSTAMP()                                       // taps requested
    // ---- weight ring: the first step's 16 fragments
    // the ring holds the current step's 16 fragments, slot f refilled with fragment f of the next step's run as soon as its k-step is done
    constexpr int RING = 16;
    bf16x8 ring[RING];
    auto fill = [&](const T *slice, int f) { ring[f] = *reinterpret_cast<const bf16x8 *>(slice + f * 512 + lane * 8); };
    const T *cur_run;                          // (written by every step, read by nothing: without it the compiler schedules the 96-row chains differently)
    {
        const T *run0 = p.st[HEAD ? 4 : 0].W + (size_t)wave * (FRONT0 ? p.st[0].K / 256 : KS) * SLICE;
#pragma unroll
        for (int f = 0; f < RING; ++f) fill(run0, f);
    }
    __builtin_amdgcn_sched_barrier(0);
    RSTAMP()                                       // ring requested
    // ---- the residual stream of this workgroup's rows, in the accumulator layout: xs[i][2 ns + j][q] = x[m0 + 16 i + r16][256 ns + 32 wave + 16 j + 4 g + q].
    // Requested AFTER the operand tile / depthwise window and the ring (loads return in order): the prologue and the first product do not
    // wait for these 16 MT D bytes per wave (a CU takes in ~10 B per cycle: 96 KiB = 4.6 us), only the first epilogue does.
    // With the depthwise prologue they are requested after it: their 8 MT NJ registers are free for the prologue (with them the ring did
    // not fit: fragments were parked in scratch memory at the kernel's start, i.e. waited for), and the first product hides them.
    f32x4 xs[MT][NJ];
    // (blocked form: see ChainArgs::x_in_blocked)
    const size_t xblk = ((size_t)rblk * 8 + wave) * (MT * NJ) * 256 + lane * 4;      // floats
    auto load_stream = [&]() {
        if (p.x_in_blocked) {
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int c = 0; c < NJ; ++c) xs[i][c] = *reinterpret_cast<const f32x4 *>(p.x + xblk + (i * NJ + c) * 256);
            return;
        }
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const float *xrow = p.x + (size_t)min(m0 + 16 * i + r16, mend - 1) * D + 32 * wave + 4 * g;
#pragma unroll
            for (int c = 0; c < NJ; ++c) xs[i][c] = *reinterpret_cast<const f32x4 *>(xrow + 256 * (c >> 1) + 16 * (c & 1));
        }
    };
    // head: the stream of the ME tiles (blocked layout: the last tile of row block rblk - 1, the own tiles, the first tile of block rblk + 1;
    // at the ends of the batch the own block stands in -- those rows are outside every line).  The own tiles become xs after the head.
    f32x4 xe[HEAD ? ME : 1][NJ];
    if constexpr (HEAD) {
        const int nblk = gridDim.x;
#pragma unroll
        for (int e = 0; e < ME; ++e) {
            const int blk = e == 0 ? max(rblk - 1, 0) : e == ME - 1 ? min(rblk + 1, nblk - 1) : rblk, tile = e == 0 ? MT - 1 : e == ME - 1 ? 0 : e - 1;
            const float *src = p.xh + (((size_t)blk * 8 + wave) * MT + tile) * (NJ * 256) + lane * 4;
#pragma unroll
            for (int c = 0; c < NJ; ++c) xe[e][c] = *reinterpret_cast<const f32x4 *>(src + c * 256);
        }
    }
    constexpr int EARLY_XS = HEAD ? ME * NJ : (DWK == 0 && !FRONT0) ? MT * NJ : 0;     // stream loads in flight at the first wait
    if constexpr (DWK == 0 && !FRONT0) load_stream();                 // (FRONT: the stream is born in this launch)
    __builtin_amdgcn_sched_barrier(0);
    if (tid < BMC) {
        const int m = min(m0 + tid, M - 1), b = m / p.T_, t = m - b * p.T_;
        rowoff[tid] = ((long long)b * p.heads * p.Tp + t) * p.dhp;
        tpos[tid] = t;
    }
    RSTAMP()                                       // 1: loads requested
    // the operand DMAs (older than the ring and stream loads) have landed.  The count is the FEWEST loads that can be in flight behind them:
    // a first step that skips k-steps never reads its last ring slots and the compiler drops those loads (with 16 here and 10 loads issued the
    // wait let the depthwise window arrive late: wrong rows in the first launch on fresh LDS, right ones by luck afterwards)
    constexpr int KK0 = HEAD ? 8 : K0 == ST_ROWLN ? KKR::value : K0 == ST_FFN ? KKD::value : 8;       // k-steps of the launch's first step
    constexpr int RING0 = 2 * KK0;
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(RING0 + EARLY_XS) : "memory");
    lds_fence_barrier();
    RSTAMP()                                       // 2: operand tile / window landed

    auto dw_prologue = [&]() { if constexpr (DWK != 0) {      // (run below, behind the head where there is one)
        // Depthwise conv (kernel DWK, zero padding at the line ends, BatchNorm folded) + SiLU on the GLU output (convolution.py:140-142),
        // for the workgroup's rows from the (BMC + DWK - 1)-row window in LDS, written straight into the operand image; 256 channels at a
        // time.  thread = one channel pair x BMC / 4 rows (groups of 8); a wave's lanes share their rows, so the boundary test is uniform.
        // Accumulation order per output: bias, then taps ascending (as the stand-alone kernel: bit-identical).
        typedef float f32x2_t __attribute__((ext_vector_type(2)));
        constexpr int CPAIRS = CW / 2, NRG = 512 / CPAIRS;    // channel pairs of a pass; row groups the threads split the block's rows into
        constexpr int RQ = BMC / NRG;                         // rows of one thread
        constexpr int G = RQ % 8 == 0 ? 8 : (RQ % 6 == 0 ? 6 : 8);      // rows walked together (a window row read serves G outputs)
        static_assert(BMC % NRG == 0 && RQ >= G, "rows per thread of the depthwise prologue");
        const int cp = tid % CPAIRS, rq = __builtin_amdgcn_readfirstlane(tid / CPAIRS);
        const int T_ = p.T_;
#pragma unroll 1
        for (int h = 0; h < D / CW; ++h) {
            if (h > 0) {                                     // next channel pass: the window area is free after the barrier that ended the previous one
                dw_window(h);
                dw_taps(h);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                lds_fence_barrier();
            }
            const int c = 2 * cp;                            // channel inside the pass
            dw_taps_read();
            const f32x2_t bias = dw_bias;
            // rows of this thread: group rq of the block, G at a time (a ragged last group re-does rows of the previous one)
#pragma unroll 1
            for (int r0 = RQ * rq; r0 < RQ * (rq + 1); r0 += G) {
                const int rb = min(r0, RQ * (rq + 1) - G);
                const int t0 = __builtin_amdgcn_readfirstlane(tpos[rb]);
                f32x2_t acc[G];
#pragma unroll
                for (int i = 0; i < G; ++i) acc[i] = bias;
                const unsigned char *wbase = win + (size_t)rb * WS + c * 2;
                if (t0 >= DWPAD && t0 + (G - 1) + DWPAD < T_) {        // all G rows inside one line, full tap range
#pragma unroll
                    for (int rin = 0; rin < G + DWK - 1; ++rin) {
                        const bf16x2 xv = *reinterpret_cast<const bf16x2 *>(wbase + rin * WS);
                        const f32x2_t xf = {(float)xv[0], (float)xv[1]};
#pragma unroll
                        for (int i = 0; i < G; ++i) {
                            const int tau = rin - i;
                            if (tau >= 0 && tau < DWK) acc[i] = __builtin_elementwise_fma(dw_wt[tau], xf, acc[i]);
                        }
                    }
                } else if (__builtin_amdgcn_readfirstlane(tpos[rb + G - 1]) == t0 + G - 1) {
                    // near a line end, the G rows inside one line: the same walk over the window with the rows outside the line read as zero
                    // (a zero tap product leaves the sum as it is: the same values as skipping the tap).  The per-tap form below costs 3 x
                    // the instructions; with one line end per three 96-row blocks it set the kernel's duration: the launch is as long as its
                    // slowest workgroup (timing experiment without the prologue's arithmetic: - 11 us of 63).
#pragma unroll
                    for (int rin = 0; rin < G + DWK - 1; ++rin) {
                        const bool ok = (unsigned)(t0 + rin - DWPAD) < (unsigned)T_;     // (uniform)
                        const bf16x2 xv = *reinterpret_cast<const bf16x2 *>(wbase + rin * WS);
                        const f32x2_t xf = {ok ? (float)xv[0] : 0.f, ok ? (float)xv[1] : 0.f};
#pragma unroll
                        for (int i = 0; i < G; ++i) {
                            const int tau = rin - i;
                            if (tau >= 0 && tau < DWK) acc[i] = __builtin_elementwise_fma(dw_wt[tau], xf, acc[i]);
                        }
                    }
                } else {                                               // rows of two lines: tap tau of row i is in range iff 0 <= t_i + tau - PAD < T
                    int ti[G];
#pragma unroll
                    for (int i = 0; i < G; ++i) ti[i] = __builtin_amdgcn_readfirstlane(tpos[rb + i]);
#pragma unroll
                    for (int rin = 0; rin < G + DWK - 1; ++rin) {      // the same walk, the window row masked per output row
                        const bf16x2 xv = *reinterpret_cast<const bf16x2 *>(wbase + rin * WS);
                        const f32x2_t xr = {(float)xv[0], (float)xv[1]};
#pragma unroll
                        for (int i = 0; i < G; ++i) {
                            const int tau = rin - i;
                            if (tau >= 0 && tau < DWK) {
                                const bool ok = (unsigned)(ti[i] + tau - DWPAD) < (unsigned)T_;
                                const f32x2_t xf = {ok ? xr[0] : 0.f, ok ? xr[1] : 0.f};
                                acc[i] = __builtin_elementwise_fma(dw_wt[tau], xf, acc[i]);
                            }
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < G; ++i) {
                    const int row = rb + i, cc = h * CW + c;
                    const bf16x2 o = {(T)silu_f(acc[i][0]), (T)silu_f(acc[i][1])};
                    *reinterpret_cast<bf16x2 *>(xa + (cc >> 6) * PANEL + row * 128 + ((((cc & 63) >> 3) ^ (row & 7)) << 4) + (cc & 7) * 2) = o;
                    if constexpr (TAPS) {
                        if (p.tap_dw && m0 + row < mend) *reinterpret_cast<bf16x2 *>(p.tap_dw + (size_t)(m0 + row) * D + cc) = o;
                    }
                }
            }
            lds_fence_barrier();                             // this pass of the operand image complete; the window is free
        }
        if constexpr (!HEAD) load_stream();        // (head: the stream is in the registers already)
        __builtin_amdgcn_sched_barrier(0);
        RSTAMP()                                   // 3: depthwise prologue done
    } };

    // One step: acc[rows][32 columns of this wave] += image[256 k] . ring ; ring <- the 16 fragments at `nxt`.  `side(kk)` is independent VALU
    // work folded into the k-step.  `fresh`: the accumulators start from zero -- the first k-step's MFMAs take the constant 0 as their C
    // operand instead of registers zeroed by v_mov (the VALU is the scarce unit of this kernel).
    // (MTC: the row tiles of the image and of `acc` -- MT, or the head's MT + 2)
    auto step_n = [&](auto MTC, const unsigned char *img, auto &acc, int c0, const T *nxt, auto &&side, auto FRESH, auto KKC) {      // acc[MTN][..]: tiles c0, c0 + 1
        constexpr int MTN = decltype(MTC)::value, PANELN = 16 * MTN * 128;
        constexpr bool fresh = decltype(FRESH)::value;
        constexpr int KK = decltype(KKC)::value;           // k-steps with real columns (the others multiply zeros: skipped)
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            // row tiles in two halves: half the operand registers live
            constexpr int HT = (MTN > 3 && MTN % 2 == 0) ? MTN / 2 : MTN;
#pragma unroll
            for (int h0 = 0; h0 < MTN; h0 += HT) {
                bf16x8 a[HT];
#pragma unroll
                for (int i = 0; i < HT; ++i) a[i] = lds_frag_swz(img + (kk >> 1) * PANELN + (16 * (h0 + i) + r16) * 128, kk & 1, g, swz, T());
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < HT; ++i)
                        acc[h0 + i][c0 + j] = mma16(ring[2 * kk + j], a[i], (fresh && kk == 0) ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[h0 + i][c0 + j]);
            }
            fill(nxt, 2 * kk);
            fill(nxt, 2 * kk + 1);
            side(kk);
            __builtin_amdgcn_sched_barrier(0);               // keep the refill (and the side work) here: the scheduler otherwise sinks all of it to the step's end
        }
        if constexpr (KK < 8) {
#pragma unroll
            for (int f = 2 * KK; f < RING; ++f) fill(nxt, f);  // the skipped k-steps' ring slots: the next step's fragments all the same
            __builtin_amdgcn_sched_barrier(0);
        }
        cur_run = nxt;
    };
    typedef std::integral_constant<int, MT> MTC0;
    typedef std::integral_constant<int, ME> MEC;
    auto step = [&](const unsigned char *img, auto &acc, int c0, const T *nxt, auto &&side, auto FRESH, auto KKC) { step_n(MTC0{}, img, acc, c0, nxt, side, FRESH, KKC); };
    auto no_side = [](int) {};
    // this wave's weight run of k slice `ks` of the 256-column step `n` of a product with K = D
    auto wslice = [&](const T *W, int n, int ks) { return W + ((size_t)(n * 8 + wave) * KS + ks) * SLICE; };
    // A K = D product from zero: acc[..][c0], acc[..][c0 + 1] = operand image . step `n` of W, over its KS slices; the ring then takes the run
    // at `nxt()` (a callable, evaluated where the last slice's step begins: where the address arithmetic sits decides the compiler's schedule)
    auto fresh_n = [&](auto MTC, auto &acc, int c0, const T *W, int n, auto &&nxt, auto KKC) {
        constexpr int PANELN = 16 * decltype(MTC)::value * 128;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const T *then = ks + 1 < KS ? wslice(W, n, ks + 1) : nxt();
            if (ks == 0) step_n(MTC, xa, acc, c0, then, no_side, std::true_type{}, KKC);
            else step_n(MTC, xa + ks * 4 * PANELN, acc, c0, then, no_side, std::false_type{}, KKC);
        }
    };
    // LayerNorm parameters of a stage -> LDS, requested at the stage's start by waves 0..3 (one array each); the epilogue's vmcnt(16) + barrier
    // publishes them (at least one step = 16 younger ring loads lies between)
    auto request_ln_params = [&](const ChainStage &st) {
        if (wave < 4) {
            const float *src = wave == 0 ? st.g1 : wave == 1 ? st.b1 : wave == 2 ? (st.g2 ? st.g2 : st.g1) : (st.b2 ? st.b2 : st.b1);
#pragma unroll
            for (int c = 0; c < D / 256; ++c)
                __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src + c * 256 + lane * 4), (lds_ptr_t)(reinterpret_cast<unsigned char *>(lnp) + wave * D * 4 + c * 1024), 16, 0, 0);
        }
    };
    // this wave's 2 x 4 bias values of a 256-column step (requested BEFORE the step: younger loads than the ring's would make their
    // consumer wait for the whole ring)
    struct Bias2 { f32x4 v[2]; };
    auto load_bias = [&](const float *bias) {
        Bias2 b;
        b.v[0] = *reinterpret_cast<const f32x4 *>(bias + 32 * wave + 4 * g);
        b.v[1] = *reinterpret_cast<const f32x4 *>(bias + 32 * wave + 16 + 4 * g);
        return b;
    };
    auto add_bias_n = [&](auto MTC, auto &xs, const float *bias, float alpha) {       // xs += alpha * bias: the stream becomes the product's initial accumulator
        constexpr int MTN = decltype(MTC)::value;
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) {
            const Bias2 b = load_bias(bias + 256 * ns);
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < MTN; ++i) xs[i][2 * ns + j] += b.v[j] * alpha;
        }
    };
    auto add_bias_to_stream = [&](const float *bias, float alpha) { add_bias_n(MTC0{}, xs, bias, alpha); };
    // fp32 stream -> global in the accumulator layout (16 bytes per lane, 64-byte row segments; once per launch and consumer)
    auto store_stream = [&](float *dst) {
        if (dst == p.x && p.x_out_blocked) {                  // (rows beyond M inside the last block carry finite values nobody uses)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int c = 0; c < NJ; ++c) *reinterpret_cast<f32x4 *>(dst + xblk + (i * NJ + c) * 256) = xs[i][c];
            return;
        }
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            if (m0 + 16 * i + r16 < mend) {
                float *xrow = dst + (size_t)(m0 + 16 * i + r16) * D + 32 * wave + 4 * g;
#pragma unroll
                for (int c = 0; c < NJ; ++c) *reinterpret_cast<f32x4 *>(xrow + 256 * (c >> 1) + 16 * (c & 1)) = xs[i][c];
            }
        }
    };
    // Row statistics of the stream registers: per-lane sums of its NJ x 4 values per row tile, butterflies over the 4 lanes of a row, per-wave
    // partials (sum, sum of squares) in LDS at `pbuf` [row][wave], one barrier, then every lane adds the 8 waves' partials of its MT rows.
    // One pass (E[x^2] - mean^2 in fp32 over D <= 512 values of magnitude ~1: the bf16 operand this feeds has 8 significant bits).
    auto row_stats_n = [&](auto MTC, auto &xs, unsigned char *pbuf, bool wait_params, auto &mean, auto &rstd) {
        constexpr int MTN = decltype(MTC)::value;
        float s[MTN], ss[MTN];
#pragma unroll
        for (int i = 0; i < MTN; ++i) {
            // (explicit fused multiply-adds here and in `normalise`: every instantiation -- rows per workgroup, debug taps -- must round a row's
            // statistics the same way, whatever the compiler's contraction choices are in that instantiation)
            f32x4 a = xs[i][0], b = xs[i][0] * xs[i][0];
#pragma unroll
            for (int c = 1; c < NJ; ++c) { a += xs[i][c]; b = __builtin_elementwise_fma(xs[i][c], xs[i][c], b); }
            s[i] = (a[0] + a[1]) + (a[2] + a[3]);
            ss[i] = (b[0] + b[1]) + (b[2] + b[3]);
        }
#pragma unroll
        for (int i0 = 0; i0 < MTN; i0 += 4) {
            const int i1 = min(i0 + 1, MTN - 1), i2 = min(i0 + 2, MTN - 1), i3 = min(i0 + 3, MTN - 1);
            const float ts = butterfly4(s[i0], s[i1], s[i2], s[i3]), tss = butterfly4(ss[i0], ss[i1], ss[i2], ss[i3]);
            const int tile = g == 0 ? i0 : g == 1 ? i2 : g == 2 ? i1 : i3;              // which tile's totals this lane's row holds
            *reinterpret_cast<f32x2 *>(pbuf + (16 * tile + r16) * PROW + wave * 8) = (f32x2){ts, tss};
        }
        if (wait_params && wave < 4) {      // this stage's LayerNorm parameters have landed (requested before the stage's first step)
            if constexpr (KD == 8 && KL == 8) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(RING) : "memory");      // ... at least one step = 16 younger ring loads lies between
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                    // (steps that skip k-steps issue fewer: the compiler drops the dead ones)
        }
        lds_fence_barrier();
        const float inv_d = p.inv_d;                       // (raw moments: zero-padded columns add nothing, the divisor is the real width)
#pragma unroll
        for (int i = 0; i < MTN; ++i) {
            const unsigned char *pr = pbuf + (16 * i + r16) * PROW;
            f32x4 v = *reinterpret_cast<const f32x4 *>(pr);
#pragma unroll
            for (int w2 = 1; w2 < 4; ++w2) v += *reinterpret_cast<const f32x4 *>(pr + 16 * w2);
            const float S = v[0] + v[2], SS = v[1] + v[3];
            mean[i] = S * inv_d;
            const float ex2 = SS * inv_d;
            rstd[i] = __builtin_amdgcn_rsqf(fmaxf(__builtin_fmaf(-mean[i], mean[i], ex2), 0.f) + 1e-5f);
        }
    };
    auto row_stats = [&](unsigned char *pbuf, bool wait_params, float (&mean)[MT], float (&rstd)[MT]) { row_stats_n(MTC0{}, xs, pbuf, wait_params, mean, rstd); };
    // (x - mean) rstd gamma + beta for this lane's columns; which: 0 = (g1, b1), 1 = (g2, b2).  IN_PLACE: the stream itself is normalised
    // (chained LayerNorms); otherwise the result goes to the operand image (and the stream stays).
    auto normalise_n = [&](auto MTC, auto &xs, int which, const auto &mean, const auto &rstd, auto IN_PLACE) {
        constexpr int MTN = decltype(MTC)::value, PANELN = 16 * MTN * 128;
        constexpr bool in_place = decltype(IN_PLACE)::value;
        const float *ga = lnp + which * 2 * D, *be = ga + D;
#pragma unroll
        for (int c = 0; c < NJ; ++c) {
            const int col = 256 * (c >> 1) + 32 * wave + 16 * (c & 1) + 4 * g;
            const f32x4 gv = *reinterpret_cast<const f32x4 *>(ga + col), bv = *reinterpret_cast<const f32x4 *>(be + col);
#pragma unroll
            for (int i = 0; i < MTN; ++i) {
                const float r = rstd[i], mr = -mean[i] * r;
                const f32x4 y = __builtin_elementwise_fma(__builtin_elementwise_fma(xs[i][c], (f32x4){r, r, r, r}, (f32x4){mr, mr, mr, mr}), gv, bv);
                if constexpr (in_place) {
                    xs[i][c] = y;
                } else {
                    const int row = 16 * i + r16;
                    const bf16x4 o = {(T)y[0], (T)y[1], (T)y[2], (T)y[3]};
                    *reinterpret_cast<bf16x4 *>(xa + (col >> 6) * PANELN + row * 128 + ((((col & 63) >> 3) ^ (row & 7)) << 4) + (col & 4) * 2) = o;
                }
            }
        }
    };
    auto normalise = [&](int which, const float (&mean)[MT], const float (&rstd)[MT], auto IN_PLACE) { normalise_n(MTC0{}, xs, which, mean, rstd, IN_PLACE); };
    // Coalesced copy of a staged [BMC][D] bf16 tile to the workgroup's rows of the (M, D) matrix `dst`; `src(row, ch)`: where the tile
    // holds the 16-byte chunk ch of its row
    auto copy_out = [&](T *dst, auto &&src) {
        for (int id = tid; id < BMC * (D / 8); id += 512) {
            const int row = id / (D / 8), ch = id - row * (D / 8);
            if (m0 + row < mend) copy16(dst + (size_t)(m0 + row) * D + ch * 8, reinterpret_cast<const T *>(src(row, ch)));
        }
    };
    // Residual + LayerNorm(s) of a stage whose product has left x_new in the stream registers.
    //   single:  x <- x_new ;            operand <- LN1(x)
    //   chained: x <- LN1(x_new) ;       operand <- LN2(x)          (block-final LayerNorm + the next block's first)
    // `pbuf`: 2 x BMC x PROW bytes of LDS nobody reads or writes during the epilogue (a hidden-chunk image that is not the last one read).
    auto rowln_epilogue = [&](const ChainStage &st, unsigned char *pbuf) {
        const bool chained = st.g2 != nullptr;
        if constexpr (TAPS) { if (st.tap_pre) store_stream(st.tap_pre); }
        float mean[MT], rstd[MT];
        if (!chained) {
            if (st.store_x) store_stream(p.x);
            row_stats(pbuf, true, mean, rstd);               // (barrier inside: every wave is also done reading the old operand image)
            normalise(0, mean, rstd, std::false_type{});
        } else {
            row_stats(pbuf, true, mean, rstd);
            normalise(0, mean, rstd, std::true_type{});
            if (st.store_x) store_stream(p.x);
            if constexpr (TAPS) { if (st.tap_post) store_stream(st.tap_post); }
            row_stats(pbuf + BMC * PROW, false, mean, rstd);
            normalise(1, mean, rstd, std::false_type{});
        }
        lds_fence_barrier();                                 // new operand image complete
        if (st.store_xn) {                                   // bf16 operand rows -> global (the decoder's input), coalesced from the image
            for (int id = tid; id < BMC * (D / 8); id += 512) {
                const int row = id / (D / 8), ch = id - row * (D / 8);
                if (m0 + row < mend)
                    copy16(p.xn + (size_t)(m0 + row) * D + ch * 8, reinterpret_cast<const T *>(xa + (ch >> 3) * PANEL + row * 128 + (((ch & 7) ^ (row & 7)) << 4)));
            }
        }
    };

    // GLU of step s2 of the pointwise conv's 2 D packed columns: wave w's pair acc[..][0], acc[..][1] = (value tile, gate tile) of channels
    // 128 s2 + 16 w .. + 15 (bb.v[0]: value bias, v[1]: gate bias) -> bf16 [row][stride bytes] at `tile`
    auto glu_n = [&](auto MTC, const auto &acc, const Bias2 &bb, unsigned char *tile, int stride, int s2) {
#pragma unroll
        for (int i = 0; i < decltype(MTC)::value; ++i) {
            const int row = 16 * i + r16;
            bf16x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = (T)((acc[i][0][q] + bb.v[0][q]) * sigmoid_f(acc[i][1][q] + bb.v[1][q]));
            *reinterpret_cast<bf16x4 *>(tile + row * stride + (s2 * 128 + 16 * wave + 4 * g) * 2) = o;
        }
    };

    auto run_stage = [&](auto KIND, auto FIRST, const ChainStage &st, const T *after) {      // `after`: this wave's first slice of the next stage
        constexpr int kind = decltype(KIND)::value;
        if constexpr (kind == ST_ROWLN) {
            // x_new = x + bias + A W^T: NS column steps x KS k-slices
            request_ln_params(st);
            if constexpr (decltype(FIRST)::value) {
                // first stage of a launch: the stream is still on its way -- the product starts from zero and the stream (+ bias) is
                // added afterwards
                f32x4 acc[MT][NJ];
#pragma unroll
                for (int ns = 0; ns < NS; ++ns) fresh_n(MTC0{}, acc, 2 * ns, st.W, ns, [&] { return ns + 1 < NS ? wslice(st.W, ns + 1, 0) : after; }, KKR{});
                add_bias_to_stream(st.bias, 1.0f);
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int c = 0; c < NJ; ++c) xs[i][c] += acc[i][c];
            } else {
                // accumulate straight onto the stream registers (x + bias = the product's initial accumulator)
                add_bias_to_stream(st.bias, 1.0f);
#pragma unroll
                for (int ns = 0; ns < NS; ++ns)
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        step(xa + ks * 4 * PANEL, xs, 2 * ns, ks + 1 < KS ? wslice(st.W, ns, ks + 1) : (ns + 1 < NS ? wslice(st.W, ns + 1, 0) : after), no_side, std::false_type{}, KKR{});
            }
            RSTAMP()                               // product done
            rowln_epilogue(st, hs);
            RSTAMP()                               // epilogue done
        } else if constexpr (kind == ST_FRONT) {
            // x = bias + Z Wout^T with K = F C (the frontend's output linear, convolution.py:224,235-236; the flatten of (f, c) is a view of the
            // channel-last frontend output, the weight's columns were permuted at load), then the first block's LayerNorm.  24 slices of 256 k at
            // F C = 6144: slice ks + 1 is in flight (LDS-DMA into the other hidden image) while slice ks is multiplied; one barrier per slice.
            // The split-K GEMM + reduction this replaces ran 300 workgroups on all 256 CUs for 50 us; this form streams every weight byte once
            // per row block, like every other stage.
            static_assert(decltype(FIRST)::value, "FRONT is a first stage");
            request_ln_params(st);
            const int nsl = st.K / 256;
            auto slice = [&](int ns, int ks) { return st.W + ((size_t)(ns * 8 + wave) * nsl + ks) * SLICE; };
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int c = 0; c < NJ; ++c) xs[i][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
            add_bias_to_stream(st.bias, 1.0f);
#pragma unroll 1
            for (int ks = 0; ks < nsl; ++ks) {
                // here: slice ks has landed and is published, every wave is done with the other image
                if (ks + 1 < nsl) front_dma(ks + 1);
                const unsigned char *img = hs + (ks & 1) * IMGH;
#pragma unroll
                for (int ns = 0; ns < NS; ++ns)
                    step(img, xs, 2 * ns, ns + 1 < NS ? slice(ns + 1, ks) : (ks + 1 < nsl ? slice(0, ks + 1) : after), no_side, std::false_type{}, KK8{});
                if (ks + 1 < nsl) {
                    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(RING) : "memory");      // the DMAs of slice ks + 1 are older than the last step's 16 ring loads
                    lds_fence_barrier();
                }
            }
            RSTAMP()                               // product done
            rowln_epilogue(st, hs + (nsl & 1) * IMGH);                     // partials in the image the last slice did not use
            RSTAMP()                               // epilogue done
        } else if constexpr (kind == ST_FFN) {
            // Software pipeline over the 256-wide hidden chunks:   P1(c): hidden(c) = xa W1(c)^T                  (KS steps)
            //                                                      P2(c-1): stream += silu(hidden(c-1)) W2(c-1)^T  (NS steps)  beside
            //                                                      S(c):  bias + SiLU of hidden(c) -> LDS          (VALU, folded into P2(c-1)'s k-steps)
            // weight stream order: W1(0), W1(1), W2(0), W1(2), W2(1), ..., W2(last).
            const int FF = st.N, nchunks = FF / 256;
            auto w1 = [&](int c) { return wslice(st.W, c, 0); };        // the first slice of W1(c)
            auto w2 = [&](int c, int ns) { return st.W2 + ((size_t)(ns * 8 + wave) * (FF / 32) + c * 8) * 1024; };
            f32x4 acc1[MT][2];
            Bias2 bb;
            auto silu_tile = [&](int tIdx, unsigned char *hb, auto PIN) {  // tile t = (row tile t / 2, column tile t % 2) of acc1 -> hb
                const int i = tIdx >> 1, j = tIdx & 1;
                // PIN: called from a k-step -- the arithmetic below is pure, and instruction selection otherwise gathers all twelve tiles'
                // worth of it in one block ahead of the product's first k-step (seen in the ISA: only the LDS stores stayed inside the
                // steps), where nothing overlaps it; an empty volatile asm on the inputs keeps each tile between its step's fences
                if constexpr (decltype(PIN)::value) asm volatile("" : "+v"(acc1[i][j]));
                const int jj = 32 * wave + 16 * j + 4 * g;               // hidden column inside the chunk
                const int ch16 = (jj & 63) >> 3, row = 16 * i + r16;
                // packed fp32 arithmetic around the two transcendentals: 5 packed + 4 transcendental + 1 convert per value pair
                typedef float f32x2_t __attribute__((ext_vector_type(2)));
                const f32x4 v4 = acc1[i][j] + bb.v[j];
                unsigned packed[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const f32x2_t v = {v4[2 * h], v4[2 * h + 1]};
                    f32x2_t e = v * (f32x2_t){-1.44269504088896340736f, -1.44269504088896340736f};
                    e = (f32x2_t){__builtin_amdgcn_exp2f(e[0]), __builtin_amdgcn_exp2f(e[1])} + (f32x2_t){1.0f, 1.0f};
                    const f32x2_t o = v * (f32x2_t){__builtin_amdgcn_rcpf(e[0]), __builtin_amdgcn_rcpf(e[1])};
                    packed[h] = __builtin_bit_cast(unsigned, __builtin_convertvector(o, bf16x2));
                }
                typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
                *reinterpret_cast<u32x2_t *>(hb + (jj >> 6) * PANEL + row * 128 + ((ch16 ^ (row & 7)) << 4) + ((jj & 7) >> 2) * 8) = (u32x2_t){packed[0], packed[1]};
            };
            auto p1 = [&](int c, const T *then) {                        // hidden(c) -> acc1; `then`: the slice that follows W1(c)
                // Waves 4..7 (the SIMD partners of 0..3) run this matrix-only product at raised priority: they finish it first and do the
                // vector-heavy second product + SiLU while their partners are still in this one, instead of both waves of a SIMD being
                // in the same kind of phase at the same time (without it the older wave always wins the matrix pipe: 3.0 k / 4.4 k cycles
                // for this product, the partners then alone in a 2.4 k tail of the next; chunk iteration 10.7 k -> 9.9 k cycles)
                if (wave >= 4) __builtin_amdgcn_s_setprio(1);
                fresh_n(MTC0{}, acc1, 0, st.W, c, [&] { return then; }, KKD{});
                if (wave >= 4) __builtin_amdgcn_s_setprio(0);
            };
            request_ln_params(st);
            bb = load_bias(st.bias);
            p1(0, nchunks > 1 ? w1(1) : w2(0, 0));                     // P1(0)
            RSTAMP()                                                      // P1(0) done
#pragma unroll
            for (int t2 = 0; t2 < 2 * MT; ++t2) silu_tile(t2, hs, std::false_type{});       // S(0)
            add_bias_to_stream(st.bias2, st.alpha);                       // stream + alpha b2 = the second product's initial accumulator (after P1(0):
                                                                          // as a launch's first stage the stream loads are still in flight before)
            RSTAMP()                                                      // S(0) done
            lds_fence_barrier();
            RSTAMP()                                                      // barrier
            for (int c = 1; c < nchunks; ++c) {
                bb = load_bias(st.bias + c * 256);
                p1(c, w2(c - 1, 0));                                      // P1(c)
                RSTAMP()                                                  // P1(c) done
                unsigned char *hb = hs + (c & 1) * IMGH;
#pragma unroll
                for (int ns = 0; ns < NS; ++ns)                           // P2(c-1) beside S(c): the 2 MT tiles spread over the NS x 8 k-steps
                    step(hs + ((c - 1) & 1) * IMGH, xs, 2 * ns, ns + 1 < NS ? w2(c - 1, ns + 1) : (c + 1 < nchunks ? w1(c + 1) : w2(c, 0)),
                         [&](int kk) {
#pragma unroll
                             for (int t2 = 0; t2 < 2 * MT; ++t2) if ((t2 * 8 * NS) / (2 * MT) == ns * 8 + kk) silu_tile(t2, hb, std::true_type{});
                         }, std::false_type{}, KK8{});
                RSTAMP()                                                  // P2(c-1) + S(c) done
                lds_fence_barrier();
                RSTAMP()                                                  // barrier
            }
#pragma unroll
            for (int ns = 0; ns < NS; ++ns)                               // P2(last)
                step(hs + ((nchunks - 1) & 1) * IMGH, xs, 2 * ns, ns + 1 < NS ? w2(nchunks - 1, ns + 1) : after, no_side, std::false_type{}, KKL{});
            RSTAMP()                                                      // P2(last) done
            rowln_epilogue(st, hs + (nchunks & 1) * IMGH);               // partials in the hidden image the last product did not read
            RSTAMP()                                                      // epilogue done
        } else if constexpr (kind == ST_GLU) {
            // 2 D packed columns in steps of 256: wave w's pair = (value tile, gate tile) of channels 128 step + 16 w .. +15
            constexpr int NSTEP = 2 * D / 256;
#pragma unroll 1
            for (int s2 = 0; s2 < NSTEP; ++s2) {
                const Bias2 bb = load_bias(st.bias + s2 * 256);
                f32x4 acc[MT][2];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {          // (not fresh_n: at D = 512 this loop compiles differently through it)
                    const T *nxt = ks + 1 < KS ? wslice(st.W, s2, ks + 1) : (s2 + 1 < NSTEP ? wslice(st.W, s2 + 1, 0) : after);
                    if (ks == 0) step(xa, acc, 0, nxt, no_side, std::true_type{}, KKD{});
                    else step(xa + ks * 4 * PANEL, acc, 0, nxt, no_side, std::false_type{}, KKD{});
                }
                glu_n(MTC0{}, acc, bb, hs, OSD, s2);
            }
            lds_fence_barrier();
            copy_out(st.out, [&](int row, int ch) { return hs + row * OSD + ch * 16; });
        } else if constexpr (kind == ST_QKV) {   // 3 D columns in steps of 256; step s3 lies inside one of q, k, v
            constexpr int NSTEP = 3 * D / 256;
#pragma unroll
            for (int s3 = 0; s3 < NSTEP; ++s3) {
                const Bias2 bb = load_bias(st.bias + s3 * 256);
                f32x4 acc[MT][2];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {          // (not fresh_n: at D = 512 this loop compiles differently through it)
                    const T *nxt = ks + 1 < KS ? wslice(st.W, s3, ks + 1) : (s3 + 1 < NSTEP ? wslice(st.W, s3 + 1, 0) : after);
                    if (ks == 0) step(xa, acc, 0, nxt, no_side, std::true_type{}, KKD{});
                    else step(xa + ks * 4 * PANEL, acc, 0, nxt, no_side, std::false_type{}, KKD{});
                }
                unsigned char *tile = hs + (s3 & 1) * (BMC * OS);
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < MT; ++i) {
                        const int row = 16 * i + r16;
                        bf16x4 o;
#pragma unroll
                        for (int q = 0; q < 4; ++q) o[q] = (T)(acc[i][j][q] + bb.v[j][q]);
                        *reinterpret_cast<bf16x4 *>(tile + row * OS + (32 * wave + 16 * j + 4 * g) * 2) = o;
                    }
                RSTAMP()                                     // product + staging of step s3 done
                lds_fence_barrier();                         // tile s3 complete (tile s3-1 was flushed before this barrier)
                {   // thread -> one 8-column chunk of BMC / 16 rows
                    const int which = s3 / NS;
                    T *base = which == 0 ? st.q : (which == 1 ? st.k : st.v);
                    const int ch = tid & 31, hd = (s3 - which * NS) * 256 + ch * 8, hh = hd / p.dh, d = hd - hh * p.dh;
                    base += (size_t)hh * p.Tp * p.dhp + d;
#pragma unroll
                    for (int i = 0; i < MT; ++i) {
                        const int row = (tid >> 5) + 16 * i;
                        if (m0 + row < mend) copy16(base + rowoff[row], reinterpret_cast<const T *>(tile + row * OS + ch * 16));
                    }
                }
            }
        }
    };
    auto first_slice = [&](int i) -> const T * { return p.st[i].W + (size_t)wave * ((i == 0 && FRONT0) ? p.st[0].K / 256 : KS) * SLICE; };
    // The head (D = 256: one column step, one k slice per product): the ROWLN and GLU stage code above at ME row tiles -- the stream xe, the
    // operand image of ME tiles at xa, the GLU values into the window.
    auto run_head = [&]() { if constexpr (HEAD) {
        const ChainStage &hr = p.st[4], &hg = p.st[5];
        request_ln_params(hr);
        {   // x_new = x + bias + ctx Wo^T, as the first stage of a launch computes it: the product from zero, then stream + bias, then their sum
            f32x4 acc[ME][NJ];
            fresh_n(MEC{}, acc, 0, hr.W, 0, [&] { return wslice(hg.W, 0, 0); }, KK8{});
            add_bias_n(MEC{}, xe, hr.bias, 1.0f);
#pragma unroll
            for (int i = 0; i < ME; ++i)
#pragma unroll
                for (int c = 0; c < NJ; ++c) xe[i][c] += acc[i][c];
        }
        RSTAMP()                                   // head: out-proj done
        if constexpr (TAPS) {
            if (hr.tap_pre) {                      // the stream after the attention residual, own rows
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    if (m0 + 16 * i + r16 < mend) {
                        float *xrow = hr.tap_pre + (size_t)(m0 + 16 * i + r16) * D + 32 * wave + 4 * g;
#pragma unroll
                        for (int c = 0; c < NJ; ++c) *reinterpret_cast<f32x4 *>(xrow + 256 * (c >> 1) + 16 * (c & 1)) = xe[i + 1][c];
                    }
                }
            }
        }
        {
            float mean[ME], rstd[ME];
            row_stats_n(MEC{}, xe, winx, true, mean, rstd);      // (partials in the window area: nothing is there yet)
            normalise_n(MEC{}, xe, 0, mean, rstd, std::false_type{});
        }
        lds_fence_barrier();                       // the conv module's operand image (ME tiles) complete
        // the own rows' stream stays in the registers to the end of the launch (a renaming: the loops are unrolled)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int c = 0; c < NJ; ++c) xs[i][c] = xe[i + 1][c];
        RSTAMP()                                   // head: LayerNorm done
        // pointwise conv 1 + GLU: wave w's pair = (value tile, gate tile) of channels 128 step + 16 w .. +15; the bf16 values the stand-alone
        // launch stores go into the window instead
#pragma unroll 1
        for (int s2 = 0; s2 < 2; ++s2) {
            const Bias2 bb = load_bias(hg.bias + s2 * 256);
            f32x4 acc[ME][2];
            fresh_n(MEC{}, acc, 0, hg.W, s2, [&] { return s2 == 0 ? wslice(hg.W, 1, 0) : first_slice(0); }, KKD{});
            glu_n(MEC{}, acc, bb, winx, WS, s2);
        }
        lds_fence_barrier();                       // window complete; every wave is done with the head's operand image
        if constexpr (TAPS) { if (hg.out) copy_out(hg.out, [&](int row, int ch) { return winx + (16 + row) * WS + ch * 16; }); }      // the GLU output, own rows
        RSTAMP()                                   // head: GLU done
    } };
    run_head();
    dw_prologue();
    run_stage(std::integral_constant<int, K0>{}, std::true_type{}, p.st[0], K1 >= 0 ? first_slice(1) : first_slice(0));
    run_stage(std::integral_constant<int, K1>{}, std::false_type{}, p.st[1], K2 >= 0 ? first_slice(2) : first_slice(0));
    run_stage(std::integral_constant<int, K2>{}, std::false_type{}, p.st[2], K3 >= 0 ? first_slice(3) : first_slice(0));
    run_stage(std::integral_constant<int, K3>{}, std::false_type{}, p.st[3], first_slice(0));
    RSTAMP()                                       // end
#undef RSTAMP
}

template <int D, int MT, int DWK, int K0, int K1, int K2, int K3, bool TAPS, int KD = 8, int KL = 8, int H0 = -1, int H1 = -1>
static inline hipError_t launch_rowchain_mt(hipStream_t s, const ChainArgs &a) {
    constexpr size_t lds = rowchain_lds_bytes<D, MT, (H0 >= 0)>() + (rowchain_taps_place<D, MT, DWK>() == 2 ? (size_t)(DWK + 1) * 1024 : 0);
    static_assert(lds <= 160 * 1024, "LDS of one workgroup");
    auto kern = rowchain_kernel<D, MT, DWK, K0, K1, K2, K3, TAPS, KD, KL, H0, H1>;
    hipError_t e = raise_lds_limit((const void *)kern, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(ceil_div(a.M, 16 * MT)), dim3(512), lds, s, a);
    return hipGetLastError();
}

// One chain shape at every instantiated number of row tiles (MTS: 2, 3, 4, 6 at D = 256; 2, 4 at D = 512; 2, 3, 4 behind the head), each in
// up to three forms.  (Ascending: the compiler instantiates the fold's last operand first, so a unit's kernels are emitted tallest first, in
// the order the code object has always had.)  HAS_TAPS: whether the debug instantiation exists for this chain shape (the shapes the default forward uses).
// H0, H1: the out-proj -> GLU head (ChainArgs::nhead = 2), or -1.
template <int... MTS> struct RowTiles {};
template <int D, int DWK, int K0, int K1, int K2, int K3, bool HAS_TAPS, int H0, int H1, int... MTS>
static inline hipError_t launch_rowchain_cfg(hipStream_t s, const ChainArgs &a, bool taps, int rows_hint, RowTiles<MTS...>) {
    const int mt = rowchain_pick_mt<D>(a.M, rows_hint);
    if (taps && !HAS_TAPS) return hipErrorInvalidValue;
    // the reference's default model in its zero-padded 256 / 768-wide form: 5 of 8 k-steps per K = D product, 2 of 8 in the FFN's last chunk
    // (no debug instantiation: taps run the full-depth kernels, which compute the same values -- the skipped products are exact zeros)
    const bool narrow = D == 256 && a.kd == 5 && a.kl == 2 && !taps;
    auto form = [&](auto MTV) {
        constexpr int MT = decltype(MTV)::value;
        if constexpr (HAS_TAPS) { if (taps) return launch_rowchain_mt<D, MT, DWK, K0, K1, K2, K3, true, 8, 8, H0, H1>(s, a); }
        if constexpr (D == 256) { if (narrow) return launch_rowchain_mt<D, MT, DWK, K0, K1, K2, K3, false, 5, 2, H0, H1>(s, a); }
        return launch_rowchain_mt<D, MT, DWK, K0, K1, K2, K3, false, 8, 8, H0, H1>(s, a);
    };
    hipError_t e = hipErrorInvalidValue;
    (void)((mt == MTS && ((e = form(std::integral_constant<int, MTS>{})), true)) || ...);
    return e;
}

// the kinds of a chain's (up to four) stages, -1 behind the last
struct ChainKinds { int k0, k1, k2, k3; };
static inline ChainKinds rowchain_kinds(const ChainArgs &a) {
    return {a.st[0].kind, a.nstages > 1 ? a.st[1].kind : -1, a.nstages > 2 ? a.st[2].kind : -1, a.nstages > 3 ? a.st[3].kind : -1};
}

// The depthwise-prologue chains behind the out-proj -> GLU head (ChainArgs::nhead = 2), 256 wide: 64, 48 and 32 rows (the 96-row form would
// hold 8 row tiles of accumulators and stream in the head: it keeps its two launches).
template <int D>      // (a template so that only the unit that calls it instantiates the kernels)
static inline hipError_t launch_rowchain_head(hipStream_t s, const ChainArgs &a, bool taps, int rows_hint) {
    static_assert(D == 256, "the head: encoder_dim 256");
    const auto [k0, k1, k2, k3] = rowchain_kinds(a);
    typedef RowTiles<2, 3, 4> Tiles;
    if (a.nhead != 2 || a.st[4].kind != ST_ROWLN || a.st[5].kind != ST_GLU || !a.dw_w || !a.A0 || !a.xh || a.xh == a.x || !a.x_in_blocked) return hipErrorInvalidValue;
    if (k0 == ST_ROWLN && k1 == ST_FFN && k2 == ST_FFN && k3 == ST_QKV) return launch_rowchain_cfg<D, 31, ST_ROWLN, ST_FFN, ST_FFN, ST_QKV, true, ST_ROWLN, ST_GLU>(s, a, taps, rows_hint, Tiles{});
    if (k0 == ST_ROWLN && k1 == ST_FFN && k2 == -1) return launch_rowchain_cfg<D, 31, ST_ROWLN, ST_FFN, -1, -1, true, ST_ROWLN, ST_GLU>(s, a, taps, rows_hint, Tiles{});
    return hipErrorInvalidValue;
}

// the chain shapes the forward uses; stage weights point at the fragment-major copies
template <int D>
static inline hipError_t launch_rowchain(hipStream_t s, const ChainArgs &a, bool taps, int rows_hint) {
    const auto [k0, k1, k2, k3] = rowchain_kinds(a);
    typedef std::conditional_t<D == 256, RowTiles<2, 3, 4, 6>, RowTiles<2, 4>> Tiles;
    if (a.nhead) return hipErrorInvalidValue;      // (launch_rowchain_head)
    if (a.dw_in) {                       // depthwise-conv prologue (kernel 31): the chains that follow the conv module's GLU
        if (k0 == ST_ROWLN && k1 == ST_FFN && k2 == ST_FFN && k3 == ST_QKV) return launch_rowchain_cfg<D, 31, ST_ROWLN, ST_FFN, ST_FFN, ST_QKV, true, -1, -1>(s, a, taps, rows_hint, Tiles{});
        if (k0 == ST_ROWLN && k1 == ST_FFN && k2 == -1) return launch_rowchain_cfg<D, 31, ST_ROWLN, ST_FFN, -1, -1, true, -1, -1>(s, a, taps, rows_hint, Tiles{});
        return hipErrorInvalidValue;
    }
    if (k0 == ST_FRONT && k1 == ST_FFN && k2 == ST_QKV && k3 == -1) return launch_rowchain_cfg<D, 0, ST_FRONT, ST_FFN, ST_QKV, -1, true, -1, -1>(s, a, taps, rows_hint, Tiles{});
    if (k0 == ST_FFN && k1 == ST_QKV && k2 == -1) return launch_rowchain_cfg<D, 0, ST_FFN, ST_QKV, -1, -1, true, -1, -1>(s, a, taps, rows_hint, Tiles{});
    // one feed-forward module alone (operand tile + stream in, LayerNorm epilogue, nothing else): the measurement probe of forward.hip
    // (COCR_FFN_PROBE=1: matrix-pipe counters of the FFN products by themselves, tools/ffn_probe.py)
    if (k0 == ST_FFN && k1 == -1) return launch_rowchain_cfg<D, 0, ST_FFN, -1, -1, -1, false, -1, -1>(s, a, false, rows_hint, Tiles{});
    if (k0 == ST_ROWLN && k1 == ST_GLU && k2 == -1) return launch_rowchain_cfg<D, 0, ST_ROWLN, ST_GLU, -1, -1, true, -1, -1>(s, a, taps, rows_hint, Tiles{});
    // (without the depthwise prologue: conv kernels other than 31 -- the stand-alone depthwise kernel runs before the launch --, COCR_NO_DW_FUSE A/B runs)
    if (k0 == ST_ROWLN && k1 == ST_FFN && k2 == ST_FFN && k3 == ST_QKV) return launch_rowchain_cfg<D, 0, ST_ROWLN, ST_FFN, ST_FFN, ST_QKV, true, -1, -1>(s, a, taps, rows_hint, Tiles{});
    if (k0 == ST_ROWLN && k1 == ST_FFN && k2 == -1) return launch_rowchain_cfg<D, 0, ST_ROWLN, ST_FFN, -1, -1, true, -1, -1>(s, a, taps, rows_hint, Tiles{});
    return hipErrorInvalidValue;
}
