// svtme_tff.hip — temporal filtering's luma prediction and weighting as a
// picture-window job (svtme_tf_filter, include/svtme.h): what
// produce_temporally_filtered_pic does with the sub-pel stage's result
// (temporal_filtering.c:3196-3390): the final inter prediction of every block,
// the 32x32 errors of the 64x64 branches, the per-16x16 filter weights, the
// accumulation over the window and the normalisation. 8-bit,
// use_zz_based_filter == 0 only. The chroma stage of svtme_tf_filter_yuv and
// svtme_tf_window_yuv (4:2:0) has a section of its own below, with its kernels
// k_tff_pred_uv, k_tff_norm_uv and k_tff_norm_uv_pic; the luma-only calls launch
// the three luma kernels alone.
//
// Three luma kernels.
//
// k_tff_pred, one 256-thread workgroup per (reference, SB), the whole window in
// one launch. Wavefront 0 turns the SB's branch and split flags into a list of
// units: the 64x64 block as four slabs of 16 rows (one block on one wavefront
// would idle three), else per 32x32 block one 32x32 unit, or per 16x16 block a
// 16x16 unit or four 8x8 units. A wavefront takes one unit at a time: it stages
// the unit's window in its own LDS slice (aligned dwords, v_alignbyte), runs
// the horizontal pass into an int16 LDS plane when both phases are non-zero,
// then the vertical pass / the x-only, y-only or copy case, and writes the
// pixels into the SB's 64x64 u8 tile in LDS. Then every wavefront reduces, for
// the four 16x16 quarters of its 32x32 block, the SSE of centre against
// prediction and (64x64 branches) sum and SSE of the rows sub_sampling_shift
// keeps (DPP). One lane per quarter derives the weight. The tile, the 16
// weights and the 4 errors go to the context's device scratch.
//
// k_tff_norm, one workgroup per SB: 1000 x centre plus the weighted tiles of
// the references, normalised, 16 pixels per thread, into a dense device plane
// of whole SBs, which the host copies out row by row.
//
// k_tff_norm_pic (svtme_tf_window), the same normalisation straight into the
// padded level 0 of a resident picture, inside the aligned picture only; the
// destination may be the centre picture's own plane.
//
// Semantics restated (reference line beside each):
//  * tf_64x64_inter_prediction (temporal_filtering.c:2255-2361): one 64x64 block
//    at mv[0]; tf_32x32_inter_prediction (:2362-2605): per 32x32 block 32x32 at
//    mv[1 + i] when split_32x32[i] is 0, else per 16x16 block 16x16 at
//    mv[5 + 4 i + j], or four 8x8 at mv[21 + 16 i + 4 j + l] where
//    split_16x16[i][j] is set. The interpolation filter is MULTITAP_SHARP at
//    every size (:2261, :2368): the AV1 specification's Subpel_Filters[2].
//  * MV clamp: clamp_mv_to_umv_border_sb with the block's own edges
//    (enc_inter_prediction.c:28-48), mb_to_*_edge from mi_rows / mi_cols of the
//    aligned picture (temporal_filtering.c:2319-2322 and alike); position and
//    phase from the clamped q4 MV (enc_inter_prediction.c:3154-3163).
//  * the four convolve cases (enc_inter_prediction.c:3113-3165, 3227-3343;
//    svt_av1_convolve_2d_sr_c round_0 3, round_1 11; _x_sr_c; _y_sr_c; copy).
//    All rows are predicted.
//  * convert_64x64_info_to_32x32_info (:2690-2757): on the 64x64 branches the
//    32x32 MVs are the 64x64 MV, no block is split, and the 32x32 error is the
//    variance of the final prediction against the centre block over the rows
//    sub_sampling_shift keeps, << shift (variance.c:300-306).
//  * svt_av1_apply_temporal_filter_planewise_medium_partial_c with is_chroma 0
//    (:1028-1142) on each 32x32 block (apply_filtering_block_plane_wise,
//    :1411-1493, BW >> 1): distance_threshold_fp16 (:1040), sqrt_fast
//    (:740-749), d_factor_fp8 (:1055, 1067), the doubled decay factor of an
//    unsplit block (:1061), block_error_fp8 (:1058, 1072), the window error
//    (:1077-1102: (((sum << 4) / 16) << 4) / 16 is the SSE itself, sum << 4 <
//    2^32), the 5 : 1 balance (:1118), avg_err_fp10, a 32-bit product (:1123),
//    scaled_diff16 (:1125) and the exp(-x / 16) table (:1128). unsigned
//    arithmetic wraps as the reference's uint32_t does; col * col + row * row
//    is computed unsigned.
//  * svt_aom_apply_filtering_central_c (:349-369): 1000 x source, count 1000;
//    svt_aom_get_final_filtered_pixels_c (:2607-2626): (accum + (count >> 1)) /
//    count.
// The two tables are computed at compile time from their defining formulas:
// floor(exp(-i / 16) * 2^16), i = 0..112, and floor(sqrt(i) * 2^16), i = 0..15.
//
// Reads stay inside the device full plane exactly as in svtme_tfsp.hip: the
// predictor has the same 8 taps (3 left / above, 4 right / below) and the same
// clamp, a unit's window is a part of its block's (b + 7) x (b + 7) window, and
// the staging reads the same aligned dwords. The centre block reads
// x in [px, px + 63], px <= W - 8, rows up to py + 63 <= H + 55.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svtme_launch.h"
#include "svtme_me_common.h"

using namespace svtme;

struct TffArgs {
    DevPlane cen;                       // full plane of the centre picture
    DevPlane ref[SVTME_MAX_BATCH_JOBS]; // full planes of the references
    const svtme_tf_subpel_sb *sub;      // [n][sbs]
    uint8_t *tile;                      // [n][sbs][64 * 64] predictions
    uint32_t *wgt;                      // [n][sbs][16] weights, 32x32 block * 4 + quarter
    uint32_t *e32;                      // [n][sbs][4] 32x32 errors
    uint8_t *plane;                     // k_tff_norm: the filtered plane, whole SBs, stride pic_w_b64 * 64
    DevPlane dst;                       // k_tff_norm_pic: level 0 of the result picture (may be cen)
    uint32_t decay, dist_th, ss;        // svtme_tf_filter_controls
    uint32_t n, sbs, pic_w_b64;
    int32_t W, H; // the 8-aligned picture
};

#define TFF_WP 19    // dwords per staged window row (18 + 1, odd)
#define TFF_WROWS 39 // 32 + 7: the tallest unit
#define TFF_UNITS 64

// AV1 specification, Subpel_Filters[2] (MULTITAP_SHARP), phases 0..15
__constant__ int16_t c_tff_sharp[16][8] = {
    {0, 0, 0, 128, 0, 0, 0, 0},          {-2, 2, -6, 126, 8, -2, 2, 0},       {-2, 6, -12, 124, 16, -6, 4, -2},
    {-2, 8, -18, 120, 26, -10, 6, -2},   {-4, 10, -22, 116, 38, -14, 6, -2},  {-4, 10, -22, 108, 48, -18, 8, -2},
    {-4, 10, -24, 100, 60, -20, 8, -2},  {-4, 10, -24, 90, 70, -22, 10, -2},  {-4, 12, -24, 80, 80, -24, 12, -4},
    {-2, 10, -22, 70, 90, -24, 10, -4},  {-2, 8, -20, 60, 100, -24, 10, -4},  {-2, 8, -18, 48, 108, -22, 10, -4},
    {-2, 6, -14, 38, 116, -22, 10, -4},  {-2, 6, -10, 26, 120, -18, 8, -2},   {-2, 4, -6, 16, 124, -12, 6, -2},
    {0, 2, -2, 8, 126, -6, 2, -2}};

// floor(exp(-i / 16) * 2^16): exp(-1 / 16) by its series, then its powers (compile time only; no value
// lies within 0.01 of an integer)
struct TffExpTab {
    int32_t v[113];
};
constexpr TffExpTab tff_make_exp() {
    TffExpTab t{};
    double r = 1.0, term = 1.0;
    for (int k = 1; k < 24; k++) {
        term *= -0.0625 / k;
        r += term;
    }
    double p = 1.0;
    for (int i = 0; i < 113; i++) {
        t.v[i] = (int32_t)(p * 65536.0);
        p *= r;
    }
    return t;
}
// floor(sqrt(i) * 2^16) = floor(sqrt(i << 32))
struct TffSqrtTab {
    uint32_t v[16];
};
constexpr TffSqrtTab tff_make_sqrt() {
    TffSqrtTab t{};
    for (uint64_t i = 0; i < 16; i++) {
        uint64_t r = 0;
        for (int bit = 19; bit >= 0; bit--)
            if ((r | (1ull << bit)) * (r | (1ull << bit)) <= (i << 32))
                r |= 1ull << bit;
        t.v[i] = (uint32_t)r;
    }
    return t;
}
__constant__ TffExpTab c_tff_exp   = tff_make_exp();
__constant__ TffSqrtTab c_tff_sqrt = tff_make_sqrt();

typedef __attribute__((address_space(1))) const uint32_t g_u32; // global, not flat, loads

__device__ __forceinline__ int tff_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// taps along a row of bytes (p at tap 0)
__device__ __forceinline__ int tff_hsum(const uint8_t *p, const int t[8]) {
    return t[0] * p[0] + t[1] * p[1] + t[2] * p[2] + t[3] * p[3] + t[4] * p[4] + t[5] * p[5] + t[6] * p[6] + t[7] * p[7];
}

// sqrt_fast (temporal_filtering.c:740-749); svt_log2f is the index of the highest set bit
__device__ __forceinline__ uint32_t tff_sqrt_fast(uint32_t x) {
    if (x > 15) {
        const int log2_half = (31 - __clz((int)x)) >> 1;
        const int base      = (int)(x >> (2 * log2_half - 2));
        return c_tff_sqrt.v[base] >> (17 - log2_half);
    }
    return c_tff_sqrt.v[x] >> 16;
}

// One unit on one wavefront: rows [oy, oy + h) of the b x b block at (px, py) of the picture, (bx, by)
// of the SB, predicted at the 1/8-pel MV into the SB's tile. `on` is wave-uniform; every wavefront
// of the workgroup calls this the same number of times (workgroup barriers inside).
__device__ void tff_predict(const TffArgs &A, const DevPlane &R, uint32_t *win, int16_t *im, uint8_t *tile, int lane,
                            bool on, int b, int px, int py, int bx, int by, int oy, int h, int mvx, int mvy) {
    int fx = 0, fy = 0;
    if (on) {
        // clamp_mv_to_umv_border_sb (enc_inter_prediction.c:28-48): q4 units, ss_x = ss_y = 0
        int qx = (int16_t)(mvx * 2), qy = (int16_t)(mvy * 2);
        const int spel = (4 + b) << 4;
        const int lo_x = -(px * 8) * 2 - spel, hi_x = (A.W - b - px) * 8 * 2 + spel - 16;
        const int lo_y = -(py * 8) * 2 - spel, hi_y = (A.H - b - py) * 8 * 2 + spel - 16;
        qx = qx < lo_x ? lo_x : qx > hi_x ? hi_x : qx;
        qy = qy < lo_y ? lo_y : qy > hi_y ? hi_y : qy;
        fx = qx & 15, fy = qy & 15;
        const int x0 = px + (qx >> 4), y0 = py + oy + (qy >> 4);
        // the window: byte c of staged row r is plane sample (x0 - 3 + c, y0 - 3 + r)
        const int wx = x0 - 3, shb = wx & 3, ndw = (b + 10) >> 2, rows = h + 7;
        const uint8_t *wp = uni_ptr(R.base + (ptrdiff_t)(y0 - 3) * R.stride + (wx - shb));
        const int rst     = UNI(R.stride);
        const uint32_t m  = magic_u32((uint32_t)ndw);
#pragma unroll 4
        for (int i = lane; i < rows * ndw; i += 64) {
            const int row = mdiv(i, m), j = i - row * ndw;
            const g_u32 *p = (const g_u32 *)(uintptr_t)(wp + (ptrdiff_t)row * rst) + j;
            win[row * TFF_WP + j] = __builtin_amdgcn_alignbyte(p[1], p[0], (uint32_t)shb);
        }
    }
    __syncthreads();
    const uint8_t *wb = (const uint8_t *)win;
    const int col = lane & (b - 1), rsub = b == 64 ? 0 : lane / b, rpi = 64 / b;
    int tx[8], ty[8];
    if (on) {
#pragma unroll
        for (int k = 0; k < 8; k++) tx[k] = UNI((int)c_tff_sharp[fx][k]), ty[k] = UNI((int)c_tff_sharp[fy][k]);
        if (fx && fy) // horizontal pass of svt_av1_convolve_2d_sr_c: bd 8, round_0 3
#pragma unroll 2
            for (int r = rsub; r < h + 7; r += rpi)
                im[r * 64 + col] = (int16_t)(((1 << 14) + tff_hsum(wb + r * (TFF_WP * 4) + col, tx) + 4) >> 3);
    }
    __syncthreads();
    if (on) {
        uint8_t *tp = tile + (by + oy) * 64 + bx + col;
#pragma unroll 2
        for (int y = rsub; y < h; y += rpi) {
            int v;
            if (fx && fy) { // vertical pass: offset_bits 19, round_1 11, bits 0
                int s = 1 << 19;
#pragma unroll
                for (int k = 0; k < 8; k++) s += ty[k] * im[(y + k) * 64 + col];
                v = tff_clip8((int16_t)(((s + 1024) >> 11) - ((1 << 8) + (1 << 7))));
            } else if (fx) { // svt_av1_convolve_x_sr_c: round_0 3, then FILTER_BITS - round_0
                const int s = (tff_hsum(wb + (y + 3) * (TFF_WP * 4) + col, tx) + 4) >> 3;
                v           = tff_clip8((s + 8) >> 4);
            } else if (fy) { // svt_av1_convolve_y_sr_c: FILTER_BITS
                const uint8_t *p = wb + y * (TFF_WP * 4) + col + 3;
                int s            = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) s += ty[k] * p[k * TFF_WP * 4];
                v = tff_clip8((s + 64) >> 7);
            } else {
                v = wb[(y + 3) * (TFF_WP * 4) + col + 3];
            }
            tp[y * 64] = (uint8_t)v;
        }
    }
}

__global__ void __launch_bounds__(256) k_tff_pred(const TffArgs A) {
    __shared__ uint32_t s_win[4][TFF_WROWS * TFF_WP];
    __shared__ int16_t s_im[4][TFF_WROWS * 64];
    __shared__ uint4 s_cen[64 * 4];  // the SB's 64 x 64 block of the centre picture
    __shared__ uint4 s_tile[64 * 4]; // its prediction
    __shared__ uint32_t s_unit[TFF_UNITS]; // level | index << 2
    __shared__ int s_units;
    __shared__ uint32_t s_sse[16], s_e32[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t u   = UNI(xcd_remap(blockIdx.x, gridDim.x));
    const uint32_t ri  = UNI(u / A.sbs), b64 = u - ri * A.sbs;
    const uint32_t sby = UNI(b64 / A.pic_w_b64), sbx = b64 - sby * A.pic_w_b64;
    DevPlane R = A.ref[0];
#pragma unroll
    for (int k = 1; k < SVTME_MAX_BATCH_JOBS; k++) // constant-index argument reads
        if (ri == (uint32_t)k)
            R = A.ref[k];
    const size_t unit   = (size_t)ri * A.sbs + b64;
    const uint32_t *sub = uni_ptr((const uint32_t *)(A.sub + unit)); // 85 MVs, 85 errors, 5 dwords of flags, branch
    const int sb_x = (int)sbx * 64, sb_y = (int)sby * 64;
    const int br   = UNI(sub[175] & 0xFF);
    const bool b32 = br == SVTME_TFSP_32;

    // the centre block: row tid / 4, 16 bytes at column 16 (tid % 4) (16-byte aligned: sb_x is a multiple of 64)
    s_cen[tid] = *(const uint4 *)(A.cen.base + (ptrdiff_t)(sb_y + (tid >> 2)) * A.cen.stride + sb_x + (tid & 3) * 16);
    if (wid == 0) {
        // lane = 8x8 block idx_32x32 * 16 + 4 * idx_16x16 + idx_8x8: the first 8x8 block of a predicted
        // block stands for it
        const int i = lane >> 4, j = (lane >> 2) & 3, l = lane & 3;
        const bool f32 = ((sub[170] >> (8 * i)) & 0xFF) != 0, f16 = ((sub[171 + i] >> (8 * j)) & 0xFF) != 0;
        bool lead;
        uint32_t code;
        if (!b32)
            lead = lane < 4, code = 0u | ((uint32_t)lane << 2); // slab `lane` of the 64x64 block
        else if (!f32)
            lead = (lane & 15) == 0, code = 1u | ((uint32_t)i << 2);
        else if (!f16)
            lead = l == 0, code = 2u | ((uint32_t)(i * 4 + j) << 2);
        else
            lead = true, code = 3u | ((uint32_t)lane << 2);
        int total;
        const int at = wave_compact(lead, &total);
        if (lead)
            s_unit[at] = code;
        if (lane == 0)
            s_units = total;
    }
    __syncthreads();

    const int units = s_units;
    for (int u0 = 0; u0 < units; u0 += 4) {
        const int un  = u0 + wid;
        const bool on = un < units;
        const uint32_t code = UNI(s_unit[on ? un : 0]);
        const int lv = (int)(code & 3), k = (int)(code >> 2);
        int b = 64, bx = 0, by = 0, oy = 0, h = 16, mi = 0;
        if (lv == 0)
            oy = k * 16;
        else {
            b = h = 64 >> lv;
            mi = (lv == 1 ? SVTME_TFSP_OFF_32 : lv == 2 ? SVTME_TFSP_OFF_16 : SVTME_TFSP_OFF_8) + k;
            for (int j = 0; j < lv; j++) { // origin of block k (Z order) of the level inside the SB
                const int pair = (k >> (2 * (lv - 1 - j))) & 3;
                bx += (pair & 1) * (32 >> j);
                by += (pair >> 1) * (32 >> j);
            }
        }
        const uint32_t mv = sub[mi];
        tff_predict(A, R, s_win[wid], s_im[wid], (uint8_t *)s_tile, lane, on, b, sb_x + bx, sb_y + by, bx, by, oy, h,
                    (int16_t)(mv & 0xFFFF), (int16_t)(mv >> 16));
    }
    __syncthreads();

    // wavefront wid: the 32x32 block wid, a 16x16 quarter at a time, lane = row * 4 + dword of the row
    {
        const int X = (wid & 1) * 32, Y = (wid >> 1) * 32, row = lane >> 2, dw = lane & 3;
        const bool kept = (row & (int)A.ss) == 0;
        uint32_t sk = 0, ssek = 0;
        for (int q = 0; q < 4; q++) {
            const int off = (Y + (q >> 1) * 16 + row) * 64 + X + (q & 1) * 16 + dw * 4;
            const uint32_t p = *(const uint32_t *)((const uint8_t *)s_tile + off);
            const uint32_t c = *(const uint32_t *)((const uint8_t *)s_cen + off);
            int sum = 0;
            uint32_t sse = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int d = (int)((p >> (8 * k)) & 0xFF) - (int)((c >> (8 * k)) & 0xFF);
                sum += d;
                sse += (uint32_t)(d * d);
            }
            sk += wave_sum_u32(kept ? (uint32_t)sum : 0u);
            ssek += wave_sum_u32(kept ? sse : 0u);
            sse = wave_sum_u32(sse);
            if (lane == 0)
                s_sse[wid * 4 + q] = sse;
        }
        if (lane == 0) {
            // 64x64 branches: svt_aom_variance32x32_c / 32x16_c on the kept rows, << shift (:2726-2734)
            const int sum = (int)sk;
            const uint32_t var = (ssek - (uint32_t)(((int64_t)sum * sum) >> (10 - A.ss))) << A.ss; // / (32 * (32 >> shift))
            s_e32[wid] = b32 ? sub[85 + SVTME_TFSP_OFF_32 + wid] : var;
        }
    }
    __syncthreads();

    // the tile, whole 16-byte vectors
    ((uint4 *)(A.tile + unit * 4096))[tid] = s_tile[tid];
    if (tid < 4)
        A.e32[unit * 4 + tid] = s_e32[tid];
    if (tid < 16) {
        // svt_av1_apply_temporal_filter_planewise_medium_partial_c (:1028-1142), quarter tid % 4 of 32x32 block tid / 4
        const int i = tid >> 2;
        const uint32_t dth = (uint32_t)max((int)(A.dist_th << 16) / 10, 1 << 16);
        const bool split   = b32 && ((sub[170] >> (8 * i)) & 0xFF) != 0;
        const uint32_t mv  = sub[split ? SVTME_TFSP_OFF_16 + tid : b32 ? SVTME_TFSP_OFF_32 + i : 0];
        const uint32_t be  = split ? sub[85 + SVTME_TFSP_OFF_16 + tid] : s_e32[i] >> 2;
        const uint32_t dec = split ? A.decay : A.decay << 1;
        const int col = (int16_t)(mv & 0xFFFF), row = (int16_t)(mv >> 16);
        const uint32_t d2   = (uint32_t)col * (uint32_t)col + (uint32_t)row * (uint32_t)row;
        const uint32_t dist = tff_sqrt_fast(d2 << 8);
        uint32_t dfac       = (dist << 12) / (dth >> 8);
        dfac                = dfac > 256u ? dfac : 256u;
        const uint32_t comb = (s_sse[tid] * 5u + be) / 6u;
        const uint32_t avg  = (comb >> 3) * (dfac >> 3);
        const uint32_t dd   = (dec >> 10) ? (dec >> 10) : 1u;
        uint32_t sd         = avg / dd;
        sd                  = sd < 112u ? sd : 112u;
        A.wgt[unit * 16 + tid] = (uint32_t)(c_tff_exp.v[sd] * 1000) >> 16;
    }
}

// The normalisation of 16 pixels of one row of SB b64: row tid / 4, columns 16 (tid % 4) .. + 15 (all in
// one 16x16 quarter), packed into four dwords. The only centre samples read are those 16.
__device__ __forceinline__ void tff_norm16(const TffArgs &A, uint32_t b64, uint32_t sbx, uint32_t sby, int tid,
                                           uint32_t o[4]) {
    const int row = tid >> 2, c16 = tid & 3;
    const int wi = ((row >> 5) * 2 + (c16 >> 1)) * 4 + ((row >> 4) & 1) * 2 + (c16 & 1);
    const uint4 cv = *(const uint4 *)(A.cen.base + (ptrdiff_t)((int)sby * 64 + row) * A.cen.stride + (int)sbx * 64 + c16 * 16);
    const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w};
    uint32_t acc[16], cnt = 1000; // svt_aom_apply_filtering_central_c (:360-368)
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = 1000u * ((cw[k >> 2] >> (8 * (k & 3))) & 0xFF);
    for (uint32_t r = 0; r < A.n; r++) {
        const size_t unit = (size_t)r * A.sbs + b64;
        const uint32_t w  = A.wgt[unit * 16 + wi];
        const uint4 pv    = ((const uint4 *)(A.tile + unit * 4096))[tid];
        const uint32_t pw[4] = {pv.x, pv.y, pv.z, pv.w};
        cnt += w; // (:1137-1138)
#pragma unroll
        for (int k = 0; k < 16; k++) acc[k] += w * ((pw[k >> 2] >> (8 * (k & 3))) & 0xFF);
    }
    // (accum + (count >> 1)) / count (:2621): count <= 17000 and accum < 2^23, so the high product
    // by 2^32 / count rounded up is the quotient or one more
    const uint32_t m = 0xFFFFFFFFu / cnt + 1u;
    o[0] = o[1] = o[2] = o[3] = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t v = acc[k] + (cnt >> 1);
        uint32_t q       = __umulhi(v, m);
        q -= q * cnt > v;
        o[k >> 2] |= q << (8 * (k & 3));
    }
}

__global__ void __launch_bounds__(256) k_tff_norm(const TffArgs A) {
    const int tid      = threadIdx.x;
    const uint32_t b64 = blockIdx.x;
    const uint32_t sby = b64 / A.pic_w_b64, sbx = b64 - sby * A.pic_w_b64;
    const int row = tid >> 2, c16 = tid & 3;
    uint32_t o[4];
    tff_norm16(A, b64, sbx, sby, tid, o);
    uint8_t *op = A.plane + ((size_t)sby * 64 + row) * ((size_t)A.pic_w_b64 * 64) + (size_t)sbx * 64 + c16 * 16;
    *(uint4 *)op = make_uint4(o[0], o[1], o[2], o[3]);
}

// The same into level 0 of a resident picture: only samples x < W, y < H of the aligned picture are
// stored (W is a multiple of 8: a thread's 16 pixels are all inside, the first 8 inside, or all
// outside), the margins are the pyramid kernels' to write afterwards. A.dst may be A.cen (the centre
// picture replaced in place): a thread reads from the centre plane its own 16 pixels alone
// (tff_norm16), before it stores them, and the samples nobody stores (x >= W or y >= H) are nobody's
// input either, so no thread reads what another writes. k_tff_pred, which reads the centre widely,
// has finished by stream order.
__global__ void __launch_bounds__(256) k_tff_norm_pic(const TffArgs A) {
    const int tid      = threadIdx.x;
    const uint32_t b64 = blockIdx.x;
    const uint32_t sby = b64 / A.pic_w_b64, sbx = b64 - sby * A.pic_w_b64;
    const int x = (int)sbx * 64 + (tid & 3) * 16, y = (int)sby * 64 + (tid >> 2);
    if (x >= A.W || y >= A.H)
        return;
    uint32_t o[4];
    tff_norm16(A, b64, sbx, sby, tid, o);
    uint8_t *op = A.dst.base + (ptrdiff_t)y * A.dst.stride + x; // 16-byte aligned, as the centre's load
    if (x + 16 <= A.W)
        *(uint4 *)op = make_uint4(o[0], o[1], o[2], o[3]);
    else
        *(uint2 *)op = make_uint2(o[0], o[1]);
}

// n references of one window: the predictions and weights in one launch, then the normalisation
static hipError_t tff_args(TffArgs &A, const DevPlane *cen, const DevPlane *ref, uint32_t n, uint32_t width,
                           uint32_t height, const svtme_tf_filter_controls *ctl, const svtme_tf_subpel_sb *d_sub,
                           uint8_t *d_tile, uint32_t *d_wgt, uint32_t *d_e32) {
    if (!n || n > SVTME_MAX_BATCH_JOBS)
        return hipErrorInvalidValue;
    A.cen = *cen;
    for (uint32_t k = 0; k < SVTME_MAX_BATCH_JOBS; k++) A.ref[k] = ref[k < n ? k : 0];
    A.sub       = d_sub;
    A.tile      = d_tile;
    A.wgt       = d_wgt;
    A.e32       = d_e32;
    A.decay     = ctl->tf_decay_factor_fp16;
    A.dist_th   = ctl->tf_mv_dist_th;
    A.ss        = ctl->sub_sampling_shift;
    A.n         = n;
    A.pic_w_b64 = (width + 63) / 64;
    A.sbs       = A.pic_w_b64 * ((height + 63) / 64);
    A.W         = (int32_t)width;
    A.H         = (int32_t)height;
    return hipSuccess;
}

extern "C" hipError_t svtme_launch_tff(const DevPlane *cen, const DevPlane *ref, uint32_t n, uint32_t width,
                                       uint32_t height, const svtme_tf_filter_controls *ctl,
                                       const svtme_tf_subpel_sb *d_sub, uint8_t *d_tile, uint32_t *d_wgt,
                                       uint32_t *d_e32, uint8_t *d_plane, hipStream_t s) {
    TffArgs A{};
    const hipError_t e = tff_args(A, cen, ref, n, width, height, ctl, d_sub, d_tile, d_wgt, d_e32);
    if (e != hipSuccess)
        return e;
    A.plane = d_plane;
    hipLaunchKernelGGL(k_tff_pred, dim3(n * A.sbs), dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_tff_norm, dim3(A.sbs), dim3(256), 0, s, A);
    return hipGetLastError();
}

// svtme_tf_window: the same two steps, the normalisation into level 0 of the result picture
// (width x height, the window's aligned size; it may be the centre picture's own plane)
extern "C" hipError_t svtme_launch_tff_pic(const DevPlane *cen, const DevPlane *ref, uint32_t n, uint32_t width,
                                           uint32_t height, const svtme_tf_filter_controls *ctl,
                                           const svtme_tf_subpel_sb *d_sub, uint8_t *d_tile, uint32_t *d_wgt,
                                           uint32_t *d_e32, const DevPlane *dst, hipStream_t s) {
    TffArgs A{};
    const hipError_t e = tff_args(A, cen, ref, n, width, height, ctl, d_sub, d_tile, d_wgt, d_e32);
    if (e != hipSuccess)
        return e;
    if (dst->width != (int32_t)width || dst->height != (int32_t)height)
        return hipErrorInvalidValue;
    A.dst = *dst;
    hipLaunchKernelGGL(k_tff_pred, dim3(n * A.sbs), dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_tff_norm_pic, dim3(A.sbs), dim3(256), 0, s, A);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------
// The chroma stage (svtme_tf_filter_yuv, svtme_tf_window_yuv): 8-bit 4:2:0,
// tf_chroma set. Three more kernels, launched after k_tff_pred on the same stream;
// the luma kernels above are launched as they are.
//
// k_tff_pred_uv, one 256-thread workgroup per (reference, SB): the SB's 32x32 Cb
// and Cr tiles from the unit list k_tff_pred builds (the same flags), a wavefront
// per (unit, plane); the per-8x8 SSE of both planes against the centre; the 16
// luma window errors, RECOMPUTED from k_tff_pred's luma tile and the centre
// block (8 KB of reads per workgroup that hit the L2; k_tff_pred stays the code it
// is, with no second instantiation); 2 x 16 weights. Tiles and weights go to
// their own sections of the context's scratch.
//
// k_tff_norm_uv, one workgroup per SB: tff_norm16's scheme on both planes, 8
// pixels per thread (one 8x8 quarter, one weight per reference), into two dense
// planes of whole SBs. k_tff_norm_uv_pic: the same into the result picture's
// chroma planes, inside W/2 x H/2 only. W/2 is a multiple of 4, not of 8: a
// thread's 8 pixels are all inside, the first 4 inside, or all outside.
//
// Semantics restated (reference line beside each):
//  * the blocks are luma's (tf_64x64_inter_prediction / tf_32x32_inter_prediction,
//    temporal_filtering.c:2255-2605, PICTURE_BUFFER_DESC_FULL_MASK): a luma block of
//    size b at (px, py) predicts a b/2 x b/2 block of Cb and of Cr at (px / 2,
//    py / 2) (svt_aom_inter_prediction, enc_inter_prediction.c:4248-4360:
//    svt_aom_enc_make_inter_predictor with ss_x = ss_y = 1).
//  * clamp and phase (enc_inter_prediction.c:28-48, 3154-3163): q4 = (int16_t)mv,
//    the luma 1/8 MV is the chroma 1/16 MV; clamped to [mb_to_left_edge -
//    ((4 + b/2) << 4), mb_to_right_edge + ((4 + b/2) << 4) - 16] with the luma
//    block's mb_to_*_edge (1/8 luma pel, unscaled at ss 1), the same vertically;
//    position p / 2 + (q4 >> 4), phase q4 & 15. Not half the luma clamp.
//  * the filter: MULTITAP_SHARP through av1_get_convolve_filter_params with the
//    chroma size (inter_prediction.h:137-153): Subpel_Filters[2] at 32, 16 and 8;
//    the 4x4 blocks (8x8 luma, split_16x16 set) take sub_pel_filters_4 (the
//    specification's Subpel_Filters[4]) in both directions. Rounding and the four
//    convolve cases are luma's (round_0 3, round_1 11).
//  * svt_av1_apply_temporal_filter_planewise_medium_partial_c with is_chroma 1
//    (:1028-1142) per 32x32 luma block on its 16x16 chroma block and 8x8 quarters:
//    d_factor_fp8, block_error_fp8, the doubled decay of an unsplit block and the
//    table are luma's, from the luma MVs and block errors; the window error of a
//    quarter is (((sse << 4) / 8) << 4) / 8 = 4 sse (sse <= 64 * 255^2), then
//    (that * 5 + the luma window error of the same quarter) / 6 in uint32_t
//    (:1104-1112) before the 5 : 1 balance; the decay factor is
//    tf_decay_factor_fp16[C_U] or [C_V] (:1166, :1179).
//  * the centre adds 1000 x src with count 1000 (:372-380); the result is (accum +
//    (count >> 1)) / count (:2627-2644).
//
// Reads stay inside the device chroma planes (svtme_device.h: 48 bytes left and at
// least 48 right of W/2, 40 rows above and below H/2): the clamp
// keeps a block's first sample in [-(4 + b), W/2 + 3], and at W/2 + 3 or -(4 + b)
// exactly only with phase 0; the staged window starts 3 before, at a dword at or
// after -40, and ends before W/2 + 44; rows -39 .. H/2 + 38. The centre block
// reads x <= W/2 + 27, y <= H/2 + 27.
// ----------------------------------------------------------------------------
#define TFFC_WP 11    // dwords per staged window row (10 + 1, odd)
#define TFFC_WROWS 39 // 32 + 7

// sub_pel_filters_4 (inter_prediction.c:239-255): the AV1 specification's Subpel_Filters[4]
__constant__ int16_t c_tffc_four[16][8] = {
    {0, 0, 0, 128, 0, 0, 0, 0},     {0, 0, -4, 126, 8, -2, 0, 0},    {0, 0, -8, 122, 18, -4, 0, 0},
    {0, 0, -10, 116, 28, -6, 0, 0}, {0, 0, -12, 110, 38, -8, 0, 0},  {0, 0, -12, 102, 48, -10, 0, 0},
    {0, 0, -14, 94, 58, -10, 0, 0}, {0, 0, -12, 84, 66, -10, 0, 0},  {0, 0, -12, 76, 76, -12, 0, 0},
    {0, 0, -10, 66, 84, -12, 0, 0}, {0, 0, -10, 58, 94, -14, 0, 0},  {0, 0, -10, 48, 102, -12, 0, 0},
    {0, 0, -8, 38, 110, -12, 0, 0}, {0, 0, -6, 28, 116, -10, 0, 0},  {0, 0, -4, 18, 122, -8, 0, 0},
    {0, 0, -2, 8, 126, -4, 0, 0}};

// One (unit, plane) on one wavefront: rows [oy, oy + h) of the b x b chroma block of the luma block at
// (px, py) of the picture, (bx, by) of the SB's 32x32 chroma tile, predicted at the luma MV from the
// reference plane `rbase`. tff_predict's scheme at half size (`on` is wave-uniform; workgroup
// barriers inside).
__device__ void tffc_predict(const TffcArgs &A, const uint8_t *rbase, uint32_t *win, int16_t *im, uint8_t *tile,
                             int lane, bool on, int b, int px, int py, int bx, int by, int oy, int h, int mvx,
                             int mvy) {
    int fx = 0, fy = 0;
    if (on) {
        // clamp_mv_to_umv_border_sb (enc_inter_prediction.c:28-48): q4 units, ss_x = ss_y = 1, bw = b
        int qx = mvx, qy = mvy;
        const int spel = (4 + b) << 4;
        const int lo_x = -(px * 8) - spel, hi_x = (A.W - 2 * b - px) * 8 + spel - 16;
        const int lo_y = -(py * 8) - spel, hi_y = (A.H - 2 * b - py) * 8 + spel - 16;
        qx = qx < lo_x ? lo_x : qx > hi_x ? hi_x : qx;
        qy = qy < lo_y ? lo_y : qy > hi_y ? hi_y : qy;
        fx = qx & 15, fy = qy & 15;
        const int x0 = (px >> 1) + (qx >> 4), y0 = (py >> 1) + oy + (qy >> 4);
        // the window: byte c of staged row r is plane sample (x0 - 3 + c, y0 - 3 + r)
        const int wx = x0 - 3, shb = wx & 3, ndw = (b + 10) >> 2, rows = h + 7;
        const int rst     = UNI(A.ref_stride);
        const uint8_t *wp = uni_ptr(rbase + (ptrdiff_t)(y0 - 3) * rst + (wx - shb));
        const uint32_t m  = magic_u32((uint32_t)ndw);
#pragma unroll 4
        for (int i = lane; i < rows * ndw; i += 64) {
            const int row = mdiv(i, m), j = i - row * ndw;
            const g_u32 *p = (const g_u32 *)(uintptr_t)(wp + (ptrdiff_t)row * rst) + j;
            win[row * TFFC_WP + j] = __builtin_amdgcn_alignbyte(p[1], p[0], (uint32_t)shb);
        }
    }
    __syncthreads();
    const uint8_t *wb = (const uint8_t *)win;
    const int col = lane & (b - 1), rsub = lane / b, rpi = 64 / b;
    int tx[8], ty[8];
    if (on) {
        const int16_t(*tab)[8] = b == 4 ? c_tffc_four : c_tff_sharp;
#pragma unroll
        for (int k = 0; k < 8; k++) tx[k] = UNI((int)tab[fx][k]), ty[k] = UNI((int)tab[fy][k]);
        if (fx && fy) // horizontal pass of svt_av1_convolve_2d_sr_c: bd 8, round_0 3
#pragma unroll 2
            for (int r = rsub; r < h + 7; r += rpi)
                im[r * 32 + col] = (int16_t)(((1 << 14) + tff_hsum(wb + r * (TFFC_WP * 4) + col, tx) + 4) >> 3);
    }
    __syncthreads();
    if (on) {
        uint8_t *tp = tile + (by + oy) * 32 + bx + col;
#pragma unroll 2
        for (int y = rsub; y < h; y += rpi) {
            int v;
            if (fx && fy) { // vertical pass: offset_bits 19, round_1 11, bits 0
                int s = 1 << 19;
#pragma unroll
                for (int k = 0; k < 8; k++) s += ty[k] * im[(y + k) * 32 + col];
                v = tff_clip8((int16_t)(((s + 1024) >> 11) - ((1 << 8) + (1 << 7))));
            } else if (fx) { // svt_av1_convolve_x_sr_c
                const int s = (tff_hsum(wb + (y + 3) * (TFFC_WP * 4) + col, tx) + 4) >> 3;
                v           = tff_clip8((s + 8) >> 4);
            } else if (fy) { // svt_av1_convolve_y_sr_c
                const uint8_t *p = wb + y * (TFFC_WP * 4) + col + 3;
                int s            = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) s += ty[k] * p[k * TFFC_WP * 4];
                v = tff_clip8((s + 64) >> 7);
            } else {
                v = wb[(y + 3) * (TFFC_WP * 4) + col + 3];
            }
            tp[y * 32] = (uint8_t)v;
        }
    }
}

__device__ __forceinline__ uint32_t tffc_sse4(uint32_t p, uint32_t c) {
    uint32_t sse = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int d = (int)((p >> (8 * k)) & 0xFF) - (int)((c >> (8 * k)) & 0xFF);
        sse += (uint32_t)(d * d);
    }
    return sse;
}

// weight index (32x32 luma block * 4 + quarter) of the 8x8 chroma block (g, row8) of the SB's 32x32 tile
__device__ __forceinline__ int tffc_wi(int g, int row8) {
    return ((row8 >> 1) * 2 + (g >> 1)) * 4 + (row8 & 1) * 2 + (g & 1);
}

__global__ void __launch_bounds__(256) k_tff_pred_uv(const TffcArgs A) {
    __shared__ uint32_t s_win[4][TFFC_WROWS * TFFC_WP];
    __shared__ int16_t s_im[4][TFFC_WROWS * 32];
    __shared__ uint4 s_cen[2 * 64];  // the SB's 32 x 32 blocks of the centre picture's Cb and Cr
    __shared__ uint4 s_tile[2 * 64]; // their predictions
    __shared__ uint32_t s_unit[TFF_UNITS]; // level | index << 2
    __shared__ int s_units;
    __shared__ uint32_t s_ssey[16], s_ssec[32];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t u   = UNI(xcd_remap(blockIdx.x, gridDim.x));
    const uint32_t ri  = UNI(u / A.sbs), b64 = u - ri * A.sbs;
    const uint32_t sby = UNI(b64 / A.pic_w_b64), sbx = b64 - sby * A.pic_w_b64;
    const uint8_t *rcb = A.ref[0][0], *rcr = A.ref[1][0];
#pragma unroll
    for (int k = 1; k < SVTME_MAX_BATCH_JOBS; k++) // constant-index argument reads
        if (ri == (uint32_t)k)
            rcb = A.ref[0][k], rcr = A.ref[1][k];
    const size_t unit   = (size_t)ri * A.sbs + b64;
    const uint32_t *sub = uni_ptr((const uint32_t *)(A.sub + unit));
    const int sb_x = (int)sbx * 64, sb_y = (int)sby * 64;
    const int br   = UNI(sub[175] & 0xFF);
    const bool b32 = br == SVTME_TFSP_32;

    // the luma window errors: the SSE of k_tff_pred's tile against the centre block per 16x16 quarter;
    // thread = row tid / 4, 16 bytes at column 16 (tid % 4), a wavefront = 16 rows
    {
        const uint4 pv = ((const uint4 *)(A.tile_y + unit * 4096))[tid];
        const uint4 cv = *(const uint4 *)(A.cen_y.base + (ptrdiff_t)(sb_y + (tid >> 2)) * A.cen_y.stride + sb_x +
                                          (tid & 3) * 16);
        uint32_t sse = tffc_sse4(pv.x, cv.x) + tffc_sse4(pv.y, cv.y) + tffc_sse4(pv.z, cv.z) + tffc_sse4(pv.w, cv.w);
#pragma unroll
        for (int m = 4; m < 64; m <<= 1) sse += (uint32_t)__shfl_xor((int)sse, m);
        if (lane < 4) {
            const int row = tid >> 2;
            s_ssey[((row >> 5) * 2 + (lane >> 1)) * 4 + ((row >> 4) & 1) * 2 + (lane & 1)] = sse;
        }
    }
    // the centre blocks: plane tid / 64, row (tid / 2) % 32, 16 bytes at column 16 (tid % 2) (16-byte aligned)
    if (tid < 128) {
        const uint8_t *cb = tid < 64 ? A.cen[0].base : A.cen[1].base;
        const int cst     = tid < 64 ? A.cen[0].stride : A.cen[1].stride;
        s_cen[tid] = *(const uint4 *)(cb + (ptrdiff_t)((sb_y >> 1) + ((tid >> 1) & 31)) * cst + (sb_x >> 1) + (tid & 1) * 16);
    }
    if (wid == 0) { // the unit list, as k_tff_pred builds it
        const int i = lane >> 4, j = (lane >> 2) & 3, l = lane & 3;
        const bool f32 = ((sub[170] >> (8 * i)) & 0xFF) != 0, f16 = ((sub[171 + i] >> (8 * j)) & 0xFF) != 0;
        bool lead;
        uint32_t code;
        if (!b32)
            lead = lane < 4, code = 0u | ((uint32_t)lane << 2); // slab `lane` of the 64x64 block
        else if (!f32)
            lead = (lane & 15) == 0, code = 1u | ((uint32_t)i << 2);
        else if (!f16)
            lead = l == 0, code = 2u | ((uint32_t)(i * 4 + j) << 2);
        else
            lead = true, code = 3u | ((uint32_t)lane << 2);
        int total;
        const int at = wave_compact(lead, &total);
        if (lead)
            s_unit[at] = code;
        if (lane == 0)
            s_units = total;
    }
    __syncthreads();

    // work item t: unit t / 2, plane t % 2
    const int items = s_units * 2;
    for (int t0 = 0; t0 < items; t0 += 4) {
        const int t   = t0 + wid;
        const bool on = t < items;
        const int pl  = t & 1;
        const uint32_t code = UNI(s_unit[on ? t >> 1 : 0]);
        const int lv = (int)(code & 3), k = (int)(code >> 2);
        int b = 32, bx = 0, by = 0, oy = 0, h = 8, mi = 0;
        if (lv == 0)
            oy = k * 8; // 16 luma rows of the 64x64 block
        else {
            b = h = 32 >> lv;
            mi = (lv == 1 ? SVTME_TFSP_OFF_32 : lv == 2 ? SVTME_TFSP_OFF_16 : SVTME_TFSP_OFF_8) + k;
            for (int j = 0; j < lv; j++) { // origin of block k (Z order) of the level inside the tile
                const int pair = (k >> (2 * (lv - 1 - j))) & 3;
                bx += (pair & 1) * (16 >> j);
                by += (pair >> 1) * (16 >> j);
            }
        }
        const uint32_t mv = sub[mi];
        tffc_predict(A, pl ? rcr : rcb, s_win[wid], s_im[wid], (uint8_t *)s_tile + pl * 1024, lane, on, b,
                     sb_x + 2 * bx, sb_y + 2 * by, bx, by, oy, h, (int16_t)(mv & 0xFFFF), (int16_t)(mv >> 16));
    }
    __syncthreads();

    // per 8x8 SSE: plane tid / 128, row (tid / 4) % 32, 8 bytes at column 8 (tid % 4); the 8 rows of an
    // 8x8 block are 32 consecutive lanes of one wavefront
    {
        const int g = tid & 3, row = (tid >> 2) & 31;
        const uint2 p = ((const uint2 *)s_tile)[tid], c = ((const uint2 *)s_cen)[tid];
        uint32_t sse  = tffc_sse4(p.x, c.x) + tffc_sse4(p.y, c.y);
#pragma unroll
        for (int m = 4; m < 32; m <<= 1) sse += (uint32_t)__shfl_xor((int)sse, m);
        if ((lane & 28) == 0)
            s_ssec[(tid >> 7) * 16 + tffc_wi(g, row >> 3)] = sse;
    }
    __syncthreads();

    // the tiles, whole 16-byte vectors
    if (tid < 128)
        ((uint4 *)(A.tile + unit * 2048))[tid] = s_tile[tid];
    if (tid < 32) {
        // svt_av1_apply_temporal_filter_planewise_medium_partial_c (:1028-1142), is_chroma 1: plane tid / 16,
        // quarter q % 4 of 32x32 luma block q / 4
        const int q = tid & 15, i = q >> 2;
        const uint32_t dth = (uint32_t)max((int)(A.dist_th << 16) / 10, 1 << 16);
        const bool split   = b32 && ((sub[170] >> (8 * i)) & 0xFF) != 0;
        const uint32_t mv  = sub[split ? SVTME_TFSP_OFF_16 + q : b32 ? SVTME_TFSP_OFF_32 + i : 0];
        const uint32_t be  = split ? sub[85 + SVTME_TFSP_OFF_16 + q] : A.e32[unit * 4 + i] >> 2;
        const uint32_t d0  = tid < 16 ? A.decay_cb : A.decay_cr;
        const uint32_t dec = split ? d0 : d0 << 1;
        const int col = (int16_t)(mv & 0xFFFF), row = (int16_t)(mv >> 16);
        const uint32_t d2   = (uint32_t)col * (uint32_t)col + (uint32_t)row * (uint32_t)row;
        const uint32_t dist = tff_sqrt_fast(d2 << 8);
        uint32_t dfac       = (dist << 12) / (dth >> 8);
        dfac                = dfac > 256u ? dfac : 256u;
        const uint32_t win  = ((s_ssec[tid] << 2) * 5u + s_ssey[q]) / 6u; // (:1104-1112)
        const uint32_t comb = (win * 5u + be) / 6u;
        const uint32_t avg  = (comb >> 3) * (dfac >> 3);
        const uint32_t dd   = (dec >> 10) ? (dec >> 10) : 1u;
        uint32_t sd         = avg / dd;
        sd                  = sd < 112u ? sd : 112u;
        A.wgt[unit * 32 + tid] = (uint32_t)(c_tff_exp.v[sd] * 1000) >> 16;
    }
}

// The normalisation of 8 pixels of one row of one plane of SB b64: plane tid / 128, row (tid / 4) % 32,
// columns 8 (tid % 4) .. + 7 (all in one 8x8 quarter), packed into two dwords. The only centre
// samples read are those 8.
__device__ __forceinline__ void tffc_norm8(const TffcArgs &A, uint32_t b64, uint32_t sbx, uint32_t sby, int tid,
                                           uint32_t o[2]) {
    const int pl = tid >> 7, t = tid & 127, row = t >> 2, g = t & 3;
    const int wi = pl * 16 + tffc_wi(g, row >> 3);
    const uint8_t *cb = pl ? A.cen[1].base : A.cen[0].base;
    const int cst     = pl ? A.cen[1].stride : A.cen[0].stride;
    const uint2 cv    = *(const uint2 *)(cb + (ptrdiff_t)((int)sby * 32 + row) * cst + (int)sbx * 32 + g * 8);
    const uint32_t cw[2] = {cv.x, cv.y};
    uint32_t acc[8], cnt = 1000; // svt_aom_apply_filtering_central_c (:372-380)
#pragma unroll
    for (int k = 0; k < 8; k++) acc[k] = 1000u * ((cw[k >> 2] >> (8 * (k & 3))) & 0xFF);
    for (uint32_t r = 0; r < A.n; r++) {
        const size_t unit = (size_t)r * A.sbs + b64;
        const uint32_t w  = A.wgt[unit * 32 + wi];
        const uint2 pv    = ((const uint2 *)(A.tile + unit * 2048))[tid];
        const uint32_t pw[2] = {pv.x, pv.y};
        cnt += w;
#pragma unroll
        for (int k = 0; k < 8; k++) acc[k] += w * ((pw[k >> 2] >> (8 * (k & 3))) & 0xFF);
    }
    // (accum + (count >> 1)) / count (:2627-2644), as tff_norm16 divides
    const uint32_t m = 0xFFFFFFFFu / cnt + 1u;
    o[0] = o[1] = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t v = acc[k] + (cnt >> 1);
        uint32_t q       = __umulhi(v, m);
        q -= q * cnt > v;
        o[k >> 2] |= q << (8 * (k & 3));
    }
}

__global__ void __launch_bounds__(256) k_tff_norm_uv(const TffcArgs A) {
    const int tid      = threadIdx.x;
    const uint32_t b64 = blockIdx.x;
    const uint32_t sby = b64 / A.pic_w_b64, sbx = b64 - sby * A.pic_w_b64;
    const int pl = tid >> 7, row = (tid >> 2) & 31, g = tid & 3;
    uint32_t o[2];
    tffc_norm8(A, b64, sbx, sby, tid, o);
    uint8_t *op = A.plane + (size_t)pl * A.sbs * 1024 + ((size_t)sby * 32 + row) * ((size_t)A.pic_w_b64 * 32) +
                  (size_t)sbx * 32 + g * 8;
    *(uint2 *)op = make_uint2(o[0], o[1]);
}

// The same into the chroma planes of a resident picture: only samples x < W/2, y < H/2 are stored, the
// rest of the plane is the padding's to write afterwards. A.dst may be A.cen (in place): a thread reads
// from the centre's plane its own 8 pixels alone (tffc_norm8), before it stores them or the first 4 of
// them; the 4 it does not store (x >= W/2) are nobody's input (no other thread's 8 pixels hold them),
// so no thread reads what another writes. k_tff_pred_uv, which reads the centre's 32x32 blocks, has
// finished by stream order.
__global__ void __launch_bounds__(256) k_tff_norm_uv_pic(const TffcArgs A) {
    const int tid      = threadIdx.x;
    const uint32_t b64 = blockIdx.x;
    const uint32_t sby = b64 / A.pic_w_b64, sbx = b64 - sby * A.pic_w_b64;
    const int pl = tid >> 7;
    const int x = (int)sbx * 32 + (tid & 3) * 8, y = (int)sby * 32 + ((tid >> 2) & 31);
    if (x >= (A.W >> 1) || y >= (A.H >> 1))
        return;
    uint32_t o[2];
    tffc_norm8(A, b64, sbx, sby, tid, o);
    uint8_t *db = pl ? A.dst[1].base : A.dst[0].base;
    const int ds = pl ? A.dst[1].stride : A.dst[0].stride;
    uint8_t *op = db + (ptrdiff_t)y * ds + x; // 8-byte aligned, as the centre's load
    if (x + 8 <= (A.W >> 1))
        *(uint2 *)op = make_uint2(o[0], o[1]);
    else
        *(uint32_t *)op = o[0];
}

// svtme_tf_filter_yuv: the chroma stage of a window whose luma stage (svtme_launch_tff) is already
// queued on `s`, into the two dense planes
extern "C" hipError_t svtme_launch_tffc(const TffcArgs *A, hipStream_t s) {
    if (!A->n || A->n > SVTME_MAX_BATCH_JOBS || !A->sbs)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tff_pred_uv, dim3(A->n * A->sbs), dim3(256), 0, s, *A);
    hipLaunchKernelGGL(k_tff_norm_uv, dim3(A->sbs), dim3(256), 0, s, *A);
    return hipGetLastError();
}

// svtme_tf_window_yuv: svtme_launch_tff_pic's two steps with the chroma stage's between and after
// them. Both predictions run before either normalisation: in place (dst is cen) k_tff_pred_uv still
// reads the centre's unfiltered luma for the luma window errors.
extern "C" hipError_t svtme_launch_tff_pic_yuv(const DevPlane *cen, const DevPlane *ref, uint32_t n, uint32_t width,
                                               uint32_t height, const svtme_tf_filter_controls *ctl,
                                               const svtme_tf_subpel_sb *d_sub, uint8_t *d_tile, uint32_t *d_wgt,
                                               uint32_t *d_e32, const DevPlane *dst, const TffcArgs *U, hipStream_t s) {
    TffArgs A{};
    const hipError_t e = tff_args(A, cen, ref, n, width, height, ctl, d_sub, d_tile, d_wgt, d_e32);
    if (e != hipSuccess)
        return e;
    if (dst->width != (int32_t)width || dst->height != (int32_t)height || U->n != n || U->sbs != A.sbs)
        return hipErrorInvalidValue;
    for (int p = 0; p < 2; p++)
        if (U->dst[p].width != (int32_t)width / 2 || U->dst[p].height != (int32_t)height / 2)
            return hipErrorInvalidValue;
    A.dst = *dst;
    hipLaunchKernelGGL(k_tff_pred, dim3(n * A.sbs), dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_tff_pred_uv, dim3(n * A.sbs), dim3(256), 0, s, *U);
    hipLaunchKernelGGL(k_tff_norm_pic, dim3(A.sbs), dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_tff_norm_uv_pic, dim3(A.sbs), dim3(256), 0, s, *U);
    return hipGetLastError();
}

extern "C" hipError_t svtme_prime_tff(void) { // (see svtme_prime_pyramid)
    hipFuncAttributes a;
    hipError_t e = hipFuncGetAttributes(&a, (const void *)k_tff_pred);
    if (e == hipSuccess)
        e = hipFuncGetAttributes(&a, (const void *)k_tff_norm);
    return e != hipSuccess ? e : hipFuncGetAttributes(&a, (const void *)k_tff_norm_pic);
}
