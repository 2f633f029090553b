// svtme_tf_common.h — what the temporal-filter kernels share (svtme_tff.hip, svtme_tfld.hip and,
// for the block origins, svtme_tfsp.hip): the interpolation and weight tables, sqrt_fast, the
// unit list of an SB and its decoder, the predictor tf_predict<T, UV>, the weight rule, and the
// packed loads, stores and normalisation. Device code only; every function is inlined into the
// kernel that calls it and the tables are per translation unit.
//
// T is the sample type (uint8_t: 8 bit, uint16_t: 10 bit in 16), UV the plane kind (0: luma,
// 1: 4:2:0 chroma, every size halved).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "svtme_device.h"
#include "svtme_me_common.h"

namespace svtme {

typedef __attribute__((address_space(1))) const uint32_t tf_g_u32; // global, not flat, loads

// AV1 specification, Subpel_Filters[2] (MULTITAP_SHARP), phases 0..15
static __constant__ int16_t c_tf_sharp[16][8] = {
    {0, 0, 0, 128, 0, 0, 0, 0},          {-2, 2, -6, 126, 8, -2, 2, 0},       {-2, 6, -12, 124, 16, -6, 4, -2},
    {-2, 8, -18, 120, 26, -10, 6, -2},   {-4, 10, -22, 116, 38, -14, 6, -2},  {-4, 10, -22, 108, 48, -18, 8, -2},
    {-4, 10, -24, 100, 60, -20, 8, -2},  {-4, 10, -24, 90, 70, -22, 10, -2},  {-4, 12, -24, 80, 80, -24, 12, -4},
    {-2, 10, -22, 70, 90, -24, 10, -4},  {-2, 8, -20, 60, 100, -24, 10, -4},  {-2, 8, -18, 48, 108, -22, 10, -4},
    {-2, 6, -14, 38, 116, -22, 10, -4},  {-2, 6, -10, 26, 120, -18, 8, -2},   {-2, 4, -6, 16, 124, -12, 6, -2},
    {0, 2, -2, 8, 126, -6, 2, -2}};

// sub_pel_filters_4 (inter_prediction.c:239-255): the AV1 specification's Subpel_Filters[4]
static __constant__ int16_t c_tf_four[16][8] = {
    {0, 0, 0, 128, 0, 0, 0, 0},     {0, 0, -4, 126, 8, -2, 0, 0},    {0, 0, -8, 122, 18, -4, 0, 0},
    {0, 0, -10, 116, 28, -6, 0, 0}, {0, 0, -12, 110, 38, -8, 0, 0},  {0, 0, -12, 102, 48, -10, 0, 0},
    {0, 0, -14, 94, 58, -10, 0, 0}, {0, 0, -12, 84, 66, -10, 0, 0},  {0, 0, -12, 76, 76, -12, 0, 0},
    {0, 0, -10, 66, 84, -12, 0, 0}, {0, 0, -10, 58, 94, -14, 0, 0},  {0, 0, -10, 48, 102, -12, 0, 0},
    {0, 0, -8, 38, 110, -12, 0, 0}, {0, 0, -6, 28, 116, -10, 0, 0},  {0, 0, -4, 18, 122, -8, 0, 0},
    {0, 0, -2, 8, 126, -4, 0, 0}};

// The two tables of the weight rule, computed at compile time from their defining formulas.
// floor(exp(-i / 16) * 2^16), i = 0..112: exp(-1 / 16) by its series, then its powers (no value lies
// within 0.01 of an integer)
struct TfExpTab {
    int32_t v[113];
};
constexpr TfExpTab tf_make_exp() {
    TfExpTab t{};
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
// floor(sqrt(i) * 2^16) = floor(sqrt(i << 32)), i = 0..15
struct TfSqrtTab {
    uint32_t v[16];
};
constexpr TfSqrtTab tf_make_sqrt() {
    TfSqrtTab t{};
    for (uint64_t i = 0; i < 16; i++) {
        uint64_t r = 0;
        for (int bit = 19; bit >= 0; bit--)
            if ((r | (1ull << bit)) * (r | (1ull << bit)) <= (i << 32))
                r |= 1ull << bit;
        t.v[i] = (uint32_t)r;
    }
    return t;
}
static __constant__ TfExpTab c_tf_exp   = tf_make_exp();
static __constant__ TfSqrtTab c_tf_sqrt = tf_make_sqrt();

// sqrt_fast (temporal_filtering.c:740-749); svt_log2f is the index of the highest set bit
__device__ __forceinline__ uint32_t tf_sqrt_fast(uint32_t x) {
    if (x > 15) {
        const int log2_half = (31 - __clz((int)x)) >> 1;
        const int base      = (int)(x >> (2 * log2_half - 2));
        return c_tf_sqrt.v[base] >> (17 - log2_half);
    }
    return c_tf_sqrt.v[x] >> 16;
}

// ---- packed samples ----
// N samples of type T at p (aligned to N * sizeof(T) bytes: 4, 8, 16 or 32), one per element of v
template <typename T, int N>
__device__ __forceinline__ void tf_load(const uint8_t *p, uint32_t v[N]) {
    constexpr int DW = N * (int)sizeof(T) / 4;
    uint32_t w[DW];
    if constexpr (DW == 1)
        w[0] = *(const uint32_t *)p;
    else if constexpr (DW == 2) {
        const uint2 a = *(const uint2 *)p;
        w[0] = a.x, w[1] = a.y;
    } else {
#pragma unroll
        for (int i = 0; i < DW / 4; i++) {
            const uint4 a = ((const uint4 *)p)[i];
            w[4 * i] = a.x, w[4 * i + 1] = a.y, w[4 * i + 2] = a.z, w[4 * i + 3] = a.w;
        }
    }
#pragma unroll
    for (int k = 0; k < N; k++)
        v[k] = sizeof(T) == 1 ? (w[k >> 2] >> (8 * (k & 3))) & 0xFFu : (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
}

// N samples of type T to p, packed, or with `half` the first N / 2 of them (N * sizeof(T) >= 8). MASK
// false: the caller knows that every value fits T
template <typename T, int N, bool MASK = true>
__device__ __forceinline__ void tf_store(uint8_t *p, const uint32_t v[N], bool half) {
    constexpr int DW = N * (int)sizeof(T) / 4;
    uint32_t w[DW];
#pragma unroll
    for (int i = 0; i < DW; i++) w[i] = 0;
#pragma unroll
    for (int k = 0; k < N; k++)
        if constexpr (sizeof(T) == 1)
            w[k >> 2] |= (MASK ? v[k] & 0xFFu : v[k]) << (8 * (k & 3));
        else
            w[k >> 1] |= (MASK ? v[k] & 0xFFFFu : v[k]) << (16 * (k & 1));
    if constexpr (DW == 1)
        *(uint32_t *)p = w[0];
    else if constexpr (DW == 2) {
        if (half)
            *(uint32_t *)p = w[0];
        else
            *(uint2 *)p = make_uint2(w[0], w[1]);
    } else if constexpr (DW == 4) {
        if (!half)
            *(uint4 *)p = make_uint4(w[0], w[1], w[2], w[3]);
        else
            *(uint2 *)p = make_uint2(w[0], w[1]);
    } else {
        ((uint4 *)p)[0] = make_uint4(w[0], w[1], w[2], w[3]);
        if (!half)
            ((uint4 *)p)[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
}

// the sum of squared differences of N samples
template <int N>
__device__ __forceinline__ uint32_t tf_sse(const uint32_t a[N], const uint32_t b[N]) {
    uint32_t sse = 0;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const int d = (int)a[k] - (int)b[k];
        sse += (uint32_t)(d * d);
    }
    return sse;
}

// svt_aom_get_final_filtered_pixels_c (temporal_filtering.c:2607-2655): (accum + (count >> 1)) / count
// for N accumulators. count <= 17000 and accum < 2^25, so the high product by 2^32 / count rounded up
// is the quotient or one more (the excess is below accum / 2^32)
template <int N>
__device__ __forceinline__ void tf_norm(uint32_t acc[N], uint32_t cnt) {
    const uint32_t m = 0xFFFFFFFFu / cnt + 1u;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const uint32_t v = acc[k] + (cnt >> 1);
        uint32_t q       = __umulhi(v, m);
        q -= q * cnt > v;
        acc[k] = q;
    }
}

// The error of a 32x32 luma block of a 64x64 prediction from the sum `sk` and the SSE `ssek` of its
// differences over the rows sub_sampling_shift keeps, << shift. 8 bit: svt_aom_variance32x32_c / 32x16_c
// (variance.c:300-306: sse - (sum * sum) / N in 32 bits). 10 bit: svt_aom_highbd_10_variance32x32_c /
// 32x16_c (svt_psnr.c:139-177: SSE rounded by 4 bits, sum by 2, the difference clamped at 0).
template <typename T>
__device__ __forceinline__ uint32_t tf_var32(int sk, uint32_t ssek, int ss) {
    if constexpr (sizeof(T) == 1)
        return (ssek - (uint32_t)(((int64_t)sk * sk) >> (10 - ss))) << ss; // / (32 * (32 >> shift))
    else {
        const uint32_t s4 = (ssek + 8u) >> 4;
        const int s2      = (sk + 2) >> 2;
        const int64_t v   = (int64_t)s4 - (((int64_t)s2 * s2) >> (10 - ss));
        return (uint32_t)(v >= 0 ? v : 0) << ss;
    }
}

// ---- the prediction units of an SB ----
// Wavefront 0 turns the SB's branch and split flags (dwords 170..175 of its svtme_tf_subpel_sb) into
// the list of units, `level | index << 2`: the 64x64 block as four slabs of 16 rows (one block on
// one wavefront would idle three), else per 32x32 block one 32x32 unit, or per 16x16 block a 16x16
// unit or four 8x8 units. Chroma predicts the same list at half size.
// lane = 8x8 block idx_32x32 * 16 + 4 * idx_16x16 + idx_8x8: the first 8x8 block of a predicted
// block stands for it.
__device__ __forceinline__ void tf_unit_list(const uint32_t *sub, bool b32, int lane, uint32_t *s_unit, int *s_units) {
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
        *s_units = total;
}
#define TF_UNITS 64 // the longest list: 64 8x8 blocks

// origin of block k (Z order) of level lv (0: the whole SB .. 3) inside an SB whose half is `half` samples
__device__ __forceinline__ void tf_unit_origin(int lv, int k, int half, int *x, int *y) {
    int bx = 0, by = 0;
    for (int j = 0; j < lv; j++) {
        const int pair = (k >> (2 * (lv - 1 - j))) & 3;
        bx += (pair & 1) * (half >> j);
        by += (pair >> 1) * (half >> j);
    }
    *x = bx, *y = by;
}

// A unit: rows [oy, oy + h) of the b x b block at (bx, by) of the SB's tile (64 >> UV samples wide), at
// MV `mi` of the SB's 85
struct TfUnit {
    int b, bx, by, oy, h, mi;
};
template <int UV>
__device__ __forceinline__ TfUnit tf_unit_decode(uint32_t code) {
    constexpr int S = 64 >> UV;
    const int lv = (int)(code & 3), k = (int)(code >> 2);
    TfUnit u = {S, 0, 0, 0, S / 4, 0};
    if (lv == 0)
        u.oy = k * (S / 4); // 16 luma rows of the 64x64 block
    else {
        u.b = u.h = S >> lv;
        u.mi = (lv == 1 ? SVTME_TFSP_OFF_32 : lv == 2 ? SVTME_TFSP_OFF_16 : SVTME_TFSP_OFF_8) + k;
        int bx, by;
        tf_unit_origin(lv, k, S / 2, &bx, &by);
        u.bx = bx, u.by = by;
    }
    return u;
}

// weight index (32x32 luma block * 4 + 16x16 quarter) of the quarter (g, r) of the SB's 4 x 4 quarters
__device__ __forceinline__ int tf_wi(int g, int r) { return ((r >> 1) * 2 + (g >> 1)) * 4 + (r & 1) * 2 + (g & 1); }

// ---- the predictor ----
// The LDS layout of a predicting wavefront, per variant as each was laid out:
//  * 8 bit: the staged window's rows are bytes at a fixed pitch of 19 (luma: 18 + 1) or 11 (chroma:
//    10 + 1) dwords, odd; the intermediate of the 2-D case int16 at a pitch of 64 / 32. The tallest unit
//    has 32 + 7 rows (the 32x32 block; chroma: rows to spare).
//  * 16 bit: rows of b + 8 samples in b / 2 + 4 dwords at a pitch of b / 2 + 5 dwords (luma 37, 21, 13, 9
//    for b = 64, 32, 16, 8; chroma 21, 13, 9, 7 for b = 32, 16, 8, 4): the pitch follows the unit instead
//    of doubling the 8-bit one, and is odd. A 32-lane half reads one row (b >= 32), two rows (b = 16, 8
//    dwords each, 13 apart), four (b = 8, 4 dwords each, 9 apart) or eight (b = 4): no two rows of a half
//    share a bank at any tap. The tallest are, luma, the 64x16 slab, 23 x 37 = 851 dwords (the 32x32 block:
//    39 x 21 = 819) and, chroma, the 32x8 slab, 15 x 21 = 315 (the 16x16 block: 23 x 13 = 299). The
//    intermediate is int16 at a pitch of b: 23 x 64 = 1472 values, chroma 15 x 32 = 480.
template <typename T, int UV>
struct TfLayout;
template <int UV>
struct TfLayout<uint8_t, UV> {
    static constexpr int WIN_DW = 39 * (UV ? 11 : 19), IM = 39 * (64 >> UV); // per wavefront
    static __device__ __forceinline__ int win_pitch(int) { return UV ? 11 : 19; }
    static __device__ __forceinline__ int im_pitch(int) { return 64 >> UV; }
};
template <int UV>
struct TfLayout<uint16_t, UV> {
    static constexpr int WIN_DW = UV ? 315 : 851, IM = UV ? 480 : 1472; // per wavefront
    static __device__ __forceinline__ int win_pitch(int b) { return (b >> 1) + 5; }
    static __device__ __forceinline__ int im_pitch(int b) { return b; }
};

// taps along a row of samples (p at tap 0)
template <typename T>
__device__ __forceinline__ int tf_hsum(const T *p, const int t[8]) {
    return t[0] * p[0] + t[1] * p[1] + t[2] * p[2] + t[3] * p[3] + t[4] * p[4] + t[5] * p[5] + t[6] * p[6] + t[7] * p[7];
}

// One unit on one wavefront: rows [oy, oy + h) of the b x b block of the plane (luma: b x b at (px, py)
// of the picture; chroma: the b x b chroma block of the 2b x 2b luma block at (px, py)), (bx, by) of the
// SB's tile, predicted at the luma 1/8-pel MV from the reference plane whose interior sample (0, 0) is
// `rbase`. W x H is the 8-aligned luma size. `on` is wave-uniform; every wavefront of the workgroup
// calls this the same number of times (workgroup barriers inside).
//  * clamp_mv_to_umv_border_sb (enc_inter_prediction.c:28-48) in q4 units with the luma block's
//    mb_to_*_edge (1/8 luma pel, unscaled at ss 1) and the plane's block size; the luma 1/8 MV is the
//    chroma 1/16 MV, so the chroma clamp is not half the luma clamp. Position and phase from the
//    clamped MV (enc_inter_prediction.c:3154-3163).
//  * the four convolve cases with round_0 3, round_1 11 at both depths (convolve.h:40-60: widened only
//    at 12 bit). 8 bit: svt_av1_convolve_2d_sr_c, _x_sr_c, _y_sr_c and the copy
//    (enc_inter_prediction.c:3113-3165, 3227-3343). 10 bit: svt_av1_highbd_convolve_2d_sr_c, _x_sr_c,
//    _y_sr_c and the copy (inter_prediction.c:670-777), clip_pixel_highbd. The horizontal pass adds
//    1 << (bd + FILTER_BITS - 1), the vertical has offset_bits bd + 2 FILTER_BITS - round_0; the
//    intermediate is below 1 << 15. All rows are predicted.
//  * MULTITAP_SHARP through av1_get_convolve_filter_params with the plane's block size
//    (inter_prediction.h:137-153): Subpel_Filters[2], but sub_pel_filters_4 in both directions for the
//    4x4 chroma blocks (8x8 luma, split_16x16 set).
template <typename T, int UV>
__device__ void tf_predict(const uint8_t *rbase, int rstride, int W, int H, uint32_t *win, int16_t *im, T *tile,
                           int lane, bool on, int b, int px, int py, int bx, int by, int oy, int h, int mvx, int mvy) {
    using L = TfLayout<T, UV>;
    constexpr int BPP = (int)sizeof(T), SPD = 4 / BPP, LOG_SPD = 3 - BPP; // bytes a sample, samples a dword
    constexpr int BD = BPP == 1 ? 8 : 10, PMAX = (1 << BD) - 1;
    constexpr int Q = 2 >> UV;  // q4 units per 1/8 luma pel
    constexpr int TP = 64 >> UV; // the tile's pitch
    // `res` of the 2-D case as the reference declares it: int16_t in svt_av1_convolve_2d_sr_c, int32_t in
    // svt_av1_highbd_convolve_2d_sr_c (the value fits either)
    using res_t = std::conditional_t<BPP == 1, int16_t, int32_t>;
    auto clip = [](int v) { return v < 0 ? 0 : v > PMAX ? PMAX : v; };
    int fx = 0, fy = 0;
    const int wp = L::win_pitch(b); // dwords per staged row
    if (on) {
        int qx = (int16_t)(mvx * Q), qy = (int16_t)(mvy * Q);
        const int spel = (4 + b) << 4;
        const int lo_x = -(px * 8) * Q - spel, hi_x = (W - (b << UV) - px) * 8 * Q + spel - 16;
        const int lo_y = -(py * 8) * Q - spel, hi_y = (H - (b << UV) - py) * 8 * Q + spel - 16;
        qx = qx < lo_x ? lo_x : qx > hi_x ? hi_x : qx;
        qy = qy < lo_y ? lo_y : qy > hi_y ? hi_y : qy;
        fx = qx & 15, fy = qy & 15;
        const int x0 = (px >> UV) + (qx >> 4), y0 = (py >> UV) + oy + (qy >> 4);
        // the window: sample c of staged row r is plane sample (x0 - 3 + c, y0 - 3 + r); a row's b + 7
        // samples from aligned dwords
        const int wx = x0 - 3, sh = wx & (SPD - 1), ndw = (b + 6 + SPD) >> LOG_SPD, rows = h + 7;
        const int rst     = UNI(rstride);
        const uint8_t *wpt = uni_ptr(rbase + (ptrdiff_t)(y0 - 3) * rst + (ptrdiff_t)(wx - sh) * BPP);
        const uint32_t m  = magic_u32((uint32_t)ndw);
#pragma unroll 4
        for (int i = lane; i < rows * ndw; i += 64) {
            const int row = mdiv(i, m), j = i - row * ndw;
            const tf_g_u32 *p = (const tf_g_u32 *)(uintptr_t)(wpt + (ptrdiff_t)row * rst) + j;
            win[row * wp + j] = __builtin_amdgcn_alignbyte(p[1], p[0], (uint32_t)(sh * BPP));
        }
    }
    __syncthreads();
    const T *ws = (const T *)win;
    const int wps = wp * SPD, ip = L::im_pitch(b); // samples per staged row, values per intermediate row
    const int col = lane & (b - 1), rsub = !UV && b == 64 ? 0 : lane / b, rpi = 64 / b;
    int tx[8], ty[8];
    if (on) {
        const int16_t(*tab)[8] = UV && b == 4 ? c_tf_four : c_tf_sharp;
#pragma unroll
        for (int k = 0; k < 8; k++) tx[k] = UNI((int)tab[fx][k]), ty[k] = UNI((int)tab[fy][k]);
        if (fx && fy) // the horizontal pass of the 2-D case: round_0 3
#pragma unroll 2
            for (int r = rsub; r < h + 7; r += rpi)
                im[r * ip + col] = (int16_t)(((1 << (BD + 6)) + tf_hsum(ws + r * wps + col, tx) + 4) >> 3);
    }
    __syncthreads();
    if (on) {
        T *tp = tile + (by + oy) * TP + bx + col;
#pragma unroll 2
        for (int y = rsub; y < h; y += rpi) {
            int v;
            if (fx && fy) { // vertical pass: offset_bits BD + 11, round_1 11, bits 0
                int s = 1 << (BD + 11);
#pragma unroll
                for (int k = 0; k < 8; k++) s += ty[k] * im[(y + k) * ip + col];
                v = clip((res_t)(((s + 1024) >> 11) - ((1 << BD) + (1 << (BD - 1)))));
            } else if (fx) { // x only: round_0 3, then FILTER_BITS - round_0
                const int s = (tf_hsum(ws + (y + 3) * wps + col, tx) + 4) >> 3;
                v           = clip((s + 8) >> 4);
            } else if (fy) { // y only: FILTER_BITS
                const T *p = ws + y * wps + col + 3;
                int s      = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) s += ty[k] * p[k * wps];
                v = clip((s + 64) >> 7);
            } else {
                v = ws[(y + 3) * wps + col + 3];
            }
            tp[y * TP] = (T)v;
        }
    }
}

// ---- the weight of a 16x16 luma quarter (chroma: its 8x8 block) ----
// svt_av1_apply_temporal_filter_planewise_medium_partial_c (temporal_filtering.c:1028-1142) and its
// _hbd_ twin (:1211-1333) on quarter q % 4 of 32x32 block q / 4 of the SB whose sub-pel result is `sub`:
// distance_threshold_fp16 (:1040), sqrt_fast, d_factor_fp8 (:1055, 1067), the doubled decay factor of an
// unsplit block (:1061, hbd :1245), block_error_fp8 (:1058, 1072), the 5 : 1 balance (:1118),
// avg_err_fp10, a 32-bit product (:1123), scaled_diff16 (:1125) and the exp(-x / 16) table (:1128).
// unsigned arithmetic wraps as the reference's uint32_t does; col * col + row * row is computed unsigned.
//  * sse: the quarter's SSE of prediction against centre, >> (bd - 8) * 2 already (:792-801). The luma
//    window error (:1077-1102) (((sum << 4) / 16) << 4) / 16 is that SSE itself (sum << 4 < 2^32); the
//    chroma one is (((sse << 4) / 8) << 4) / 8 = 4 sse (sse <= 64 * 255^2, or 64 * 1023^2 >> 4 < 2^23),
//    then (that * 5 + luma_win) / 6 in uint32_t with the luma window error of the same quarter
//    (:1104-1112, hbd :1295-1303).
//  * e32: the error of the 32x32 block; dsh is (bd - 8) * 2. The block error is the 16x16 error >> dsh of
//    a split block (hbd :1241), e32 >> 2 + dsh of an unsplit one (hbd :1256).
//  * decay: the plane's tf_decay_factor_fp16 (chroma :1166, :1179, hbd :1370, :1385).
template <bool CHROMA>
__device__ __forceinline__ uint32_t tf_weight(const uint32_t *sub, bool b32, int q, uint32_t sse, uint32_t luma_win,
                                              uint32_t e32, int dsh, uint32_t decay, uint32_t dist_th) {
    const int i = q >> 2;
    const uint32_t dth = (uint32_t)max((int)(dist_th << 16) / 10, 1 << 16);
    const bool split   = b32 && ((sub[170] >> (8 * i)) & 0xFF) != 0;
    const uint32_t mv  = sub[split ? SVTME_TFSP_OFF_16 + q : b32 ? SVTME_TFSP_OFF_32 + i : 0];
    const uint32_t be  = split ? sub[85 + SVTME_TFSP_OFF_16 + q] >> dsh : e32 >> (2 + dsh);
    const uint32_t dec = split ? decay : decay << 1;
    const int col = (int16_t)(mv & 0xFFFF), row = (int16_t)(mv >> 16);
    const uint32_t d2   = (uint32_t)col * (uint32_t)col + (uint32_t)row * (uint32_t)row;
    const uint32_t dist = tf_sqrt_fast(d2 << 8);
    uint32_t dfac       = (dist << 12) / (dth >> 8);
    dfac                = dfac > 256u ? dfac : 256u;
    const uint32_t win  = CHROMA ? ((sse << 2) * 5u + luma_win) / 6u : sse;
    const uint32_t comb = (win * 5u + be) / 6u;
    const uint32_t avg  = (comb >> 3) * (dfac >> 3);
    const uint32_t dd   = (dec >> 10) ? (dec >> 10) : 1u;
    uint32_t sd         = avg / dd;
    sd                  = sd < 112u ? sd : 112u;
    return (uint32_t)(c_tf_exp.v[sd] * 1000) >> 16;
}

} // namespace svtme
