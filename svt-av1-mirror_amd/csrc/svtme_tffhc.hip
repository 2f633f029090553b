// svtme_tffhc.hip — temporal filtering's chroma stage on 10-bit pictures
// (svtme_tf_filter_yuv_10bit, svtme_tf_window_yuv_10bit, include/svtme.h): 4:2:0,
// tf_chroma set, use_zz_based_filter == 0, use_8bit_subpel == 1. It joins the chroma
// stage's structure (svtme_tff.hip, k_tff_pred_uv and its two normalisations) with the
// 16-bit prediction of svtme_tffh.hip. Both files are left as they are: these are three
// kernels of their own with their own copies of the tables, launched after k_tffh_pred on
// the same stream; k_tffh_pred is launched as it is.
//
// k_tffh_pred_uv, one 256-thread workgroup per (reference, SB): the SB's 32x32 Cb and Cr
// tiles (u16) from the unit list k_tffh_pred builds (the same flags), a wavefront per
// (unit, plane); the per-8x8 SSE of both planes against the centre; the 16 luma window
// errors RECOMPUTED from k_tffh_pred's 16-bit luma tile and the centre's 16-bit luma block
// (16 KB of reads per workgroup that hit the L2; k_tffh_pred stays the code it is); 2 x 16
// weights. Tiles and weights go to their own sections of the context's scratch.
//
// k_tffh_norm_uv, one workgroup per SB: 1000 x centre plus the weighted tiles,
// normalised, 8 samples per thread (one 8x8 quarter, one weight per reference), into two
// dense u16 planes of whole SBs. k_tffh_norm_uv_pic: the same into the result picture's
// 16-bit chroma planes, inside W/2 x H/2 only. W/2 is a multiple of 4, not of 8: a
// thread's 8 samples are all inside, the first 4 inside, or all outside.
//
// LDS of k_tffh_pred_uv (17.4 KB), laid out for the 16-bit samples rather than by doubling
// the 8-bit chroma stage's rows:
//  * the staged window of a (unit, plane), per wavefront: rows of b + 8 samples in
//    b / 2 + 4 dwords at a pitch of b / 2 + 5 dwords (21, 13, 9, 7 for b = 32, 16, 8, 4),
//    odd, so the rows a 32-lane half reads (one at b = 32, two at 16, four at 8, eight at 4)
//    start in different banks at every tap. The tallest are the 32x8 slab, 15 x 21 = 315
//    dwords, and the 16x16 block, 23 x 13 = 299.
//  * the intermediate of the 2-D case, int16 at a pitch of b: 15 x 32 = 480 values.
//  * the two tiles (4 KB) and the centre's two 32x32 blocks (4 KB).
//
// Semantics restated (reference line beside each):
//  * the blocks are luma's; a luma block of size b at (px, py) predicts a b/2 x b/2 block
//    of Cb and of Cr at (px / 2, py / 2) (svt_aom_inter_prediction,
//    enc_inter_prediction.c:4248-4360, ss_x = ss_y = 1, is_highbd).
//  * clamp and phase (enc_inter_prediction.c:28-48, 3154-3163): q4 = (int16_t)mv, the luma
//    1/8 MV is the chroma 1/16 MV; clamped to [mb_to_left_edge - ((4 + b/2) << 4),
//    mb_to_right_edge + ((4 + b/2) << 4) - 16] with the luma block's mb_to_*_edge, the same
//    vertically; position p / 2 + (q4 >> 4), phase q4 & 15. Not half the luma clamp.
//  * svt_highbd_inter_predictor at bd 10, MULTITAP_SHARP through
//    av1_get_convolve_filter_params with the chroma size (inter_prediction.h:137-153):
//    Subpel_Filters[2] at 32, 16 and 8, sub_pel_filters_4 for the 4x4 blocks in both
//    directions; round_0 3, round_1 11, horizontal offset 1 << 16, offset_bits 21,
//    clip_pixel_highbd(.., 10) (inter_prediction.c:670-777), as k_tffh_pred.
//  * svt_av1_apply_temporal_filter_planewise_medium_hbd_partial_c, is_chroma 1
//    (temporal_filtering.c:1211-1333) per 32x32 luma block on its 16x16 chroma block and
//    8x8 quarters: the quarter's SSE >> 4 (:800), the window error
//    (((sum << 4) / 8) << 4) / 8 = 4 sum (sum <= 64 * 1023^2 >> 4 < 2^23), then (that * 5 +
//    the luma window error of the same quarter) / 6 in uint32_t (:1295-1303), the luma
//    window error itself (((sum << 4) / 16) << 4) / 16 = the 16x16 SSE >> 4; the 16x16
//    error >> 4 of a split block (:1241), the 32x32 error >> 6 of an unsplit one (:1256),
//    which doubles the decay (:1245); the plane's own decay factor (:1370, :1385);
//    d_factor and the exp table are luma's.
//  * svt_aom_apply_filtering_central_highbd_c (:386-407): 1000 x source, count 1000;
//    svt_aom_get_final_filtered_pixels_c, is_highbd (:2645-2655).
//
// Reads stay inside the 16-bit chroma planes (svtme_hbd_chroma_geometry: 48 samples left
// and at least 48 right of W/2, 40 rows above and below H/2): the clamp keeps a block's
// first sample in [-(4 + b), W/2 + 3]; the staged window starts 3 before at an even sample
// at or after -40, and its b / 2 + 5 dwords (the last one read for the alignment alone) end
// at or before sample W/2 + 41; rows -39 .. H/2 + 38. The centre blocks read x <= W/2 + 27,
// y <= H/2 + 27. The luma tile and centre reads are k_tffh_pred's own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svtme_launch.h"
#include "svtme_me_common.h"

using namespace svtme;

// k_tffh_pred and k_tffh_norm_pic (svtme_tffh.hip) are launched from here by
// svtme_launch_tffh_pic_yuv, which puts k_tffh_pred_uv between them; their argument block is
// restated, field for field, because that file is not to change.
struct TffhArgs {
    DevPlane cen;
    DevPlane ref[SVTME_MAX_BATCH_JOBS];
    const svtme_tf_subpel_sb *sub;
    uint16_t *tile;
    uint32_t *wgt;
    uint32_t *e32;
    uint16_t *plane;
    DevPlane dst;
    DevPlane dst8;
    uint32_t decay, dist_th, ss;
    uint32_t n, sbs, pic_w_b64;
    int32_t W, H;
};
__global__ void k_tffh_pred(const TffhArgs A);
__global__ void k_tffh_norm_pic(const TffhArgs A);

#define TFFHC_WIN_DW 315 // 15 rows x 21 dwords: the 32x8 slab
#define TFFHC_IM 480     // 15 rows x 32 values
#define TFFHC_UNITS 64

// AV1 specification, Subpel_Filters[2] (MULTITAP_SHARP), phases 0..15
__constant__ int16_t c_tffhc_sharp[16][8] = {
    {0, 0, 0, 128, 0, 0, 0, 0},          {-2, 2, -6, 126, 8, -2, 2, 0},       {-2, 6, -12, 124, 16, -6, 4, -2},
    {-2, 8, -18, 120, 26, -10, 6, -2},   {-4, 10, -22, 116, 38, -14, 6, -2},  {-4, 10, -22, 108, 48, -18, 8, -2},
    {-4, 10, -24, 100, 60, -20, 8, -2},  {-4, 10, -24, 90, 70, -22, 10, -2},  {-4, 12, -24, 80, 80, -24, 12, -4},
    {-2, 10, -22, 70, 90, -24, 10, -4},  {-2, 8, -20, 60, 100, -24, 10, -4},  {-2, 8, -18, 48, 108, -22, 10, -4},
    {-2, 6, -14, 38, 116, -22, 10, -4},  {-2, 6, -10, 26, 120, -18, 8, -2},   {-2, 4, -6, 16, 124, -12, 6, -2},
    {0, 2, -2, 8, 126, -6, 2, -2}};

// sub_pel_filters_4 (inter_prediction.c:239-255): the AV1 specification's Subpel_Filters[4]
__constant__ int16_t c_tffhc_four[16][8] = {
    {0, 0, 0, 128, 0, 0, 0, 0},     {0, 0, -4, 126, 8, -2, 0, 0},    {0, 0, -8, 122, 18, -4, 0, 0},
    {0, 0, -10, 116, 28, -6, 0, 0}, {0, 0, -12, 110, 38, -8, 0, 0},  {0, 0, -12, 102, 48, -10, 0, 0},
    {0, 0, -14, 94, 58, -10, 0, 0}, {0, 0, -12, 84, 66, -10, 0, 0},  {0, 0, -12, 76, 76, -12, 0, 0},
    {0, 0, -10, 66, 84, -12, 0, 0}, {0, 0, -10, 58, 94, -14, 0, 0},  {0, 0, -10, 48, 102, -12, 0, 0},
    {0, 0, -8, 38, 110, -12, 0, 0}, {0, 0, -6, 28, 116, -10, 0, 0},  {0, 0, -4, 18, 122, -8, 0, 0},
    {0, 0, -2, 8, 126, -4, 0, 0}};

// floor(exp(-i / 16) * 2^16) and floor(sqrt(i) * 2^16), computed as svtme_tff.hip computes them
struct TffhcExpTab {
    int32_t v[113];
};
constexpr TffhcExpTab tffhc_make_exp() {
    TffhcExpTab t{};
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
struct TffhcSqrtTab {
    uint32_t v[16];
};
constexpr TffhcSqrtTab tffhc_make_sqrt() {
    TffhcSqrtTab t{};
    for (uint64_t i = 0; i < 16; i++) {
        uint64_t r = 0;
        for (int bit = 19; bit >= 0; bit--)
            if ((r | (1ull << bit)) * (r | (1ull << bit)) <= (i << 32))
                r |= 1ull << bit;
        t.v[i] = (uint32_t)r;
    }
    return t;
}
__constant__ TffhcExpTab c_tffhc_exp   = tffhc_make_exp();
__constant__ TffhcSqrtTab c_tffhc_sqrt = tffhc_make_sqrt();

typedef __attribute__((address_space(1))) const uint32_t ghc_u32; // global, not flat, loads

__device__ __forceinline__ int tffhc_clip10(int v) { return v < 0 ? 0 : v > 1023 ? 1023 : v; }

// taps along a row of samples (p at tap 0)
__device__ __forceinline__ int tffhc_hsum(const uint16_t *p, const int t[8]) {
    return t[0] * p[0] + t[1] * p[1] + t[2] * p[2] + t[3] * p[3] + t[4] * p[4] + t[5] * p[5] + t[6] * p[6] + t[7] * p[7];
}

// sqrt_fast (temporal_filtering.c:740-749)
__device__ __forceinline__ uint32_t tffhc_sqrt_fast(uint32_t x) {
    if (x > 15) {
        const int log2_half = (31 - __clz((int)x)) >> 1;
        const int base      = (int)(x >> (2 * log2_half - 2));
        return c_tffhc_sqrt.v[base] >> (17 - log2_half);
    }
    return c_tffhc_sqrt.v[x] >> 16;
}

// the SSE of the two samples of a dword pair
__device__ __forceinline__ uint32_t tffhc_sse2(uint32_t p, uint32_t c) {
    const int d0 = (int)(p & 0xFFFFu) - (int)(c & 0xFFFFu), d1 = (int)(p >> 16) - (int)(c >> 16);
    return (uint32_t)(d0 * d0) + (uint32_t)(d1 * d1);
}
__device__ __forceinline__ uint32_t tffhc_sse8(const uint4 p, const uint4 c) {
    return tffhc_sse2(p.x, c.x) + tffhc_sse2(p.y, c.y) + tffhc_sse2(p.z, c.z) + tffhc_sse2(p.w, c.w);
}

// One (unit, plane) on one wavefront: rows [oy, oy + h) of the b x b chroma block of the luma block at
// (px, py) of the picture, (bx, by) of the SB's 32x32 chroma tile, predicted at the luma MV from the
// reference plane `rbase`. tffh_predict's scheme at half size with tffc_predict's clamp and tables
// (`on` is wave-uniform; workgroup barriers inside).
__device__ void tffhc_predict(const TffhcArgs &A, const uint8_t *rbase, uint32_t *win, int16_t *im, uint16_t *tile,
                              int lane, bool on, int b, int px, int py, int bx, int by, int oy, int h, int mvx,
                              int mvy) {
    int fx = 0, fy = 0;
    const int wp = (b >> 1) + 5; // dwords per staged row
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
        // the window: sample c of staged row r is plane sample (x0 - 3 + c, y0 - 3 + r)
        const int wx = x0 - 3, shs = wx & 1, ndw = (b >> 1) + 4, rows = h + 7;
        const int rst      = UNI(A.ref_stride);
        const uint8_t *wpt = uni_ptr(rbase + (ptrdiff_t)(y0 - 3) * rst + (ptrdiff_t)(wx - shs) * 2);
        const uint32_t m   = magic_u32((uint32_t)ndw);
#pragma unroll 4
        for (int i = lane; i < rows * ndw; i += 64) {
            const int row = mdiv(i, m), j = i - row * ndw;
            const ghc_u32 *p = (const ghc_u32 *)(uintptr_t)(wpt + (ptrdiff_t)row * rst) + j;
            win[row * wp + j] = __builtin_amdgcn_alignbyte(p[1], p[0], (uint32_t)(shs * 2));
        }
    }
    __syncthreads();
    const uint16_t *ws = (const uint16_t *)win;
    const int wps = wp * 2; // samples per staged row
    const int col = lane & (b - 1), rsub = lane / b, rpi = 64 / b;
    int tx[8], ty[8];
    if (on) {
        const int16_t(*tab)[8] = b == 4 ? c_tffhc_four : c_tffhc_sharp;
#pragma unroll
        for (int k = 0; k < 8; k++) tx[k] = UNI((int)tab[fx][k]), ty[k] = UNI((int)tab[fy][k]);
        if (fx && fy) // horizontal pass of svt_av1_highbd_convolve_2d_sr_c: bd 10, round_0 3
#pragma unroll 2
            for (int r = rsub; r < h + 7; r += rpi)
                im[r * b + col] = (int16_t)(((1 << 16) + tffhc_hsum(ws + r * wps + col, tx) + 4) >> 3);
    }
    __syncthreads();
    if (on) {
        uint16_t *tp = tile + (by + oy) * 32 + bx + col;
#pragma unroll 2
        for (int y = rsub; y < h; y += rpi) {
            int v;
            if (fx && fy) { // vertical pass: offset_bits 21, round_1 11, bits 0
                int s = 1 << 21;
#pragma unroll
                for (int k = 0; k < 8; k++) s += ty[k] * im[(y + k) * b + col];
                v = tffhc_clip10(((s + 1024) >> 11) - ((1 << 10) + (1 << 9)));
            } else if (fx) { // svt_av1_highbd_convolve_x_sr_c: round_0 3, then FILTER_BITS - round_0
                const int s = (tffhc_hsum(ws + (y + 3) * wps + col, tx) + 4) >> 3;
                v           = tffhc_clip10((s + 8) >> 4);
            } else if (fy) { // svt_av1_highbd_convolve_y_sr_c: FILTER_BITS
                const uint16_t *p = ws + y * wps + col + 3;
                int s             = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) s += ty[k] * p[k * wps];
                v = tffhc_clip10((s + 64) >> 7);
            } else {
                v = ws[(y + 3) * wps + col + 3];
            }
            tp[y * 32] = (uint16_t)v;
        }
    }
}

// weight index (32x32 luma block * 4 + quarter) of the 8x8 chroma block (g, row8) of the SB's 32x32 tile
__device__ __forceinline__ int tffhc_wi(int g, int row8) {
    return ((row8 >> 1) * 2 + (g >> 1)) * 4 + (row8 & 1) * 2 + (g & 1);
}

__global__ void __launch_bounds__(256) k_tffh_pred_uv(const TffhcArgs A) {
    __shared__ uint32_t s_win[4][TFFHC_WIN_DW];
    __shared__ int16_t s_im[4][TFFHC_IM];
    __shared__ uint4 s_cen[2 * 128];  // the SB's 32 x 32 u16 blocks of the centre picture's Cb and Cr
    __shared__ uint4 s_tile[2 * 128]; // their predictions
    __shared__ uint32_t s_unit[TFFHC_UNITS]; // level | index << 2
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

    // the luma window errors: the SSE of k_tffh_pred's tile against the centre block per 16x16 quarter,
    // >> 4; thread = row tid / 4, 16 samples at column 16 (tid % 4), a wavefront = 16 rows
    {
        const uint4 *tp = (const uint4 *)(A.tile_y + unit * 4096) + tid * 2;
        const uint4 *cp = (const uint4 *)(A.cen_y.base + (ptrdiff_t)(sb_y + (tid >> 2)) * A.cen_y.stride +
                                          (ptrdiff_t)(sb_x + (tid & 3) * 16) * 2);
        uint32_t sse = tffhc_sse8(tp[0], cp[0]) + tffhc_sse8(tp[1], cp[1]);
#pragma unroll
        for (int m = 4; m < 64; m <<= 1) sse += (uint32_t)__shfl_xor((int)sse, m);
        if (lane < 4) {
            const int row = tid >> 2;
            s_ssey[((row >> 5) * 2 + (lane >> 1)) * 4 + ((row >> 4) & 1) * 2 + (lane & 1)] = sse >> 4;
        }
    }
    // the centre blocks: plane tid / 128, row (tid / 4) % 32, 8 samples at column 8 (tid % 4) (16-byte aligned)
    {
        const int pl      = tid >> 7;
        const uint8_t *cb = pl ? A.cen[1].base : A.cen[0].base;
        const int cst     = pl ? A.cen[1].stride : A.cen[0].stride;
        s_cen[tid] = *(const uint4 *)(cb + (ptrdiff_t)((sb_y >> 1) + ((tid >> 2) & 31)) * cst +
                                      (ptrdiff_t)((sb_x >> 1) + (tid & 3) * 8) * 2);
    }
    if (wid == 0) { // the unit list, as k_tffh_pred builds it
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
        tffhc_predict(A, pl ? rcr : rcb, s_win[wid], s_im[wid], (uint16_t *)s_tile + pl * 1024, lane, on, b,
                      sb_x + 2 * bx, sb_y + 2 * by, bx, by, oy, h, (int16_t)(mv & 0xFFFF), (int16_t)(mv >> 16));
    }
    __syncthreads();

    // per 8x8 SSE: plane tid / 128, row (tid / 4) % 32, 8 samples at column 8 (tid % 4); the 8 rows of an
    // 8x8 block are 32 consecutive lanes of one wavefront
    {
        const int g = tid & 3, row = (tid >> 2) & 31;
        uint32_t sse = tffhc_sse8(s_tile[tid], s_cen[tid]);
#pragma unroll
        for (int m = 4; m < 32; m <<= 1) sse += (uint32_t)__shfl_xor((int)sse, m);
        if ((lane & 28) == 0)
            s_ssec[(tid >> 7) * 16 + tffhc_wi(g, row >> 3)] = sse >> 4; // (:800)
    }
    __syncthreads();

    // the tiles, whole 16-byte vectors
    ((uint4 *)(A.tile + unit * 2048))[tid] = s_tile[tid];
    if (tid < 32) {
        // svt_av1_apply_temporal_filter_planewise_medium_hbd_partial_c (:1211-1333), is_chroma 1: plane
        // tid / 16, quarter q % 4 of 32x32 luma block q / 4
        const int q = tid & 15, i = q >> 2;
        const uint32_t dth = (uint32_t)max((int)(A.dist_th << 16) / 10, 1 << 16);
        const bool split   = b32 && ((sub[170] >> (8 * i)) & 0xFF) != 0;
        const uint32_t mv  = sub[split ? SVTME_TFSP_OFF_16 + q : b32 ? SVTME_TFSP_OFF_32 + i : 0];
        const uint32_t be  = split ? sub[85 + SVTME_TFSP_OFF_16 + q] >> 4 : A.e32[unit * 4 + i] >> 6; // (:1241, :1256)
        const uint32_t d0  = tid < 16 ? A.decay_cb : A.decay_cr;
        const uint32_t dec = split ? d0 : d0 << 1;
        const int col = (int16_t)(mv & 0xFFFF), row = (int16_t)(mv >> 16);
        const uint32_t d2   = (uint32_t)col * (uint32_t)col + (uint32_t)row * (uint32_t)row;
        const uint32_t dist = tffhc_sqrt_fast(d2 << 8);
        uint32_t dfac       = (dist << 12) / (dth >> 8);
        dfac                = dfac > 256u ? dfac : 256u;
        const uint32_t win  = ((s_ssec[tid] << 2) * 5u + s_ssey[q]) / 6u; // (:1295-1303)
        const uint32_t comb = (win * 5u + be) / 6u;
        const uint32_t avg  = (comb >> 3) * (dfac >> 3);
        const uint32_t dd   = (dec >> 10) ? (dec >> 10) : 1u;
        uint32_t sd         = avg / dd;
        sd                  = sd < 112u ? sd : 112u;
        A.wgt[unit * 32 + tid] = (uint32_t)(c_tffhc_exp.v[sd] * 1000) >> 16;
    }
}

// The normalisation of 8 samples of one row of one plane of SB b64: plane tid / 128, row (tid / 4) % 32,
// columns 8 (tid % 4) .. + 7 (all in one 8x8 quarter), two samples a dword. The only centre samples
// read are those 8.
__device__ __forceinline__ void tffhc_norm8(const TffhcArgs &A, uint32_t b64, uint32_t sbx, uint32_t sby, int tid,
                                            uint32_t o[4]) {
    const int pl = tid >> 7, t = tid & 127, row = t >> 2, g = t & 3;
    const int wi = pl * 16 + tffhc_wi(g, row >> 3);
    const uint8_t *cb = pl ? A.cen[1].base : A.cen[0].base;
    const int cst     = pl ? A.cen[1].stride : A.cen[0].stride;
    const uint4 cv = *(const uint4 *)(cb + (ptrdiff_t)((int)sby * 32 + row) * cst + (ptrdiff_t)((int)sbx * 32 + g * 8) * 2);
    const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w};
    uint32_t acc[8], cnt = 1000; // svt_aom_apply_filtering_central_highbd_c (:401-407)
#pragma unroll
    for (int k = 0; k < 8; k++) acc[k] = 1000u * ((cw[k >> 1] >> (16 * (k & 1))) & 0xFFFF);
    for (uint32_t r = 0; r < A.n; r++) {
        const size_t unit = (size_t)r * A.sbs + b64;
        const uint32_t w  = A.wgt[unit * 32 + wi];
        const uint4 pv    = ((const uint4 *)(A.tile + unit * 2048))[tid];
        const uint32_t pw[4] = {pv.x, pv.y, pv.z, pv.w};
        cnt += w; // (:1328-1329)
#pragma unroll
        for (int k = 0; k < 8; k++) acc[k] += w * ((pw[k >> 1] >> (16 * (k & 1))) & 0xFFFF);
    }
    // (accum + (count >> 1)) / count (:2650): count <= 17000 and accum < 2^25, as tffh_norm16 divides
    const uint32_t m = 0xFFFFFFFFu / cnt + 1u;
    o[0] = o[1] = o[2] = o[3] = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t v = acc[k] + (cnt >> 1);
        uint32_t q       = __umulhi(v, m);
        q -= q * cnt > v;
        o[k >> 1] |= (q & 0xFFFFu) << (16 * (k & 1));
    }
}

__global__ void __launch_bounds__(256) k_tffh_norm_uv(const TffhcArgs A) {
    const int tid      = threadIdx.x;
    const uint32_t b64 = blockIdx.x;
    const uint32_t sby = b64 / A.pic_w_b64, sbx = b64 - sby * A.pic_w_b64;
    const int pl = tid >> 7, row = (tid >> 2) & 31, g = tid & 3;
    uint32_t o[4];
    tffhc_norm8(A, b64, sbx, sby, tid, o);
    uint16_t *op = A.plane + (size_t)pl * A.sbs * 1024 + ((size_t)sby * 32 + row) * ((size_t)A.pic_w_b64 * 32) +
                   (size_t)sbx * 32 + g * 8;
    *(uint4 *)op = make_uint4(o[0], o[1], o[2], o[3]);
}

// The same into the 16-bit chroma planes of a resident picture: only samples x < W/2, y < H/2 are
// stored, the rest of the plane is the padding's to write afterwards. A.dst may be A.cen (in place): a
// thread reads from the centre's plane its own 8 samples alone (tffhc_norm8), before it stores them or
// the first 4 of them; the 4 it does not store (x >= W/2) are nobody's input, so no thread reads what
// another writes. k_tffh_pred_uv, which reads the centre's 32x32 blocks, has finished by stream order.
__global__ void __launch_bounds__(256) k_tffh_norm_uv_pic(const TffhcArgs A) {
    const int tid      = threadIdx.x;
    const uint32_t b64 = blockIdx.x;
    const uint32_t sby = b64 / A.pic_w_b64, sbx = b64 - sby * A.pic_w_b64;
    const int pl = tid >> 7;
    const int x = (int)sbx * 32 + (tid & 3) * 8, y = (int)sby * 32 + ((tid >> 2) & 31);
    if (x >= (A.W >> 1) || y >= (A.H >> 1))
        return;
    uint32_t o[4];
    tffhc_norm8(A, b64, sbx, sby, tid, o);
    uint8_t *db  = pl ? A.dst[1].base : A.dst[0].base;
    const int ds = pl ? A.dst[1].stride : A.dst[0].stride;
    uint8_t *op  = db + (ptrdiff_t)y * ds + (ptrdiff_t)x * 2; // 16-byte aligned, as the centre's load
    if (x + 8 <= (A.W >> 1))
        *(uint4 *)op = make_uint4(o[0], o[1], o[2], o[3]);
    else
        *(uint2 *)op = make_uint2(o[0], o[1]);
}

static hipError_t tffhc_check(const TffhcArgs *A) {
    if (!A->n || A->n > SVTME_MAX_BATCH_JOBS || !A->sbs)
        return hipErrorInvalidValue;
    for (int p = 0; p < 2; p++)
        if (A->cen[p].width != A->W / 2 || A->cen[p].height != A->H / 2)
            return hipErrorInvalidValue;
    return hipSuccess;
}

// svtme_tf_filter_yuv_10bit: the chroma stage of a window whose luma stage (svtme_launch_tffh) is
// already queued on `s`, into the two dense planes
extern "C" hipError_t svtme_launch_tffhc(const TffhcArgs *A, hipStream_t s) {
    const hipError_t e = tffhc_check(A);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_tffh_pred_uv, dim3(A->n * A->sbs), dim3(256), 0, s, *A);
    hipLaunchKernelGGL(k_tffh_norm_uv, dim3(A->sbs), dim3(256), 0, s, *A);
    return hipGetLastError();
}

// svtme_tf_window_yuv_10bit: svtme_launch_tffh_pic's two steps with the chroma stage's between and
// after them. Both predictions run before either normalisation: in place (dst is cen) k_tffh_pred_uv
// still reads the centre's unfiltered luma for the luma window errors.
extern "C" hipError_t svtme_launch_tffh_pic_yuv(const DevPlane *cen, const DevPlane *ref, uint32_t n, uint32_t width,
                                                uint32_t height, const svtme_tf_filter_controls *ctl,
                                                const svtme_tf_subpel_sb *d_sub, uint16_t *d_tile, uint32_t *d_wgt,
                                                uint32_t *d_e32, const DevPlane *dst, const DevPlane *dst8,
                                                const TffhcArgs *U, hipStream_t s) {
    if (!n || n > SVTME_MAX_BATCH_JOBS)
        return hipErrorInvalidValue;
    const DevPlane *same[3] = {cen, dst, dst8};
    for (const DevPlane *p : same)
        if (p->width != (int32_t)width || p->height != (int32_t)height)
            return hipErrorInvalidValue;
    for (uint32_t k = 0; k < n; k++)
        if (ref[k].width != (int32_t)width || ref[k].height != (int32_t)height)
            return hipErrorInvalidValue;
    TffhArgs A{}; // as svtme_tffh.hip's tffh_args fills it
    A.cen = *cen;
    for (uint32_t k = 0; k < SVTME_MAX_BATCH_JOBS; k++) A.ref[k] = ref[k < n ? k : 0];
    A.sub       = d_sub;
    A.tile      = d_tile;
    A.wgt       = d_wgt;
    A.e32       = d_e32;
    A.dst       = *dst;
    A.dst8      = *dst8;
    A.decay     = ctl->tf_decay_factor_fp16;
    A.dist_th   = ctl->tf_mv_dist_th;
    A.ss        = ctl->sub_sampling_shift;
    A.n         = n;
    A.pic_w_b64 = (width + 63) / 64;
    A.sbs       = A.pic_w_b64 * ((height + 63) / 64);
    A.W         = (int32_t)width;
    A.H         = (int32_t)height;
    const hipError_t e = tffhc_check(U);
    if (e != hipSuccess)
        return e;
    if (U->n != n || U->sbs != A.sbs || U->W != A.W || U->H != A.H)
        return hipErrorInvalidValue;
    for (int p = 0; p < 2; p++)
        if (U->dst[p].width != (int32_t)width / 2 || U->dst[p].height != (int32_t)height / 2)
            return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tffh_pred, dim3(n * A.sbs), dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_tffh_pred_uv, dim3(n * A.sbs), dim3(256), 0, s, *U);
    hipLaunchKernelGGL(k_tffh_norm_pic, dim3(A.sbs), dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_tffh_norm_uv_pic, dim3(A.sbs), dim3(256), 0, s, *U);
    return hipGetLastError();
}

extern "C" hipError_t svtme_prime_tffhc(void) { // (see svtme_prime_pyramid)
    hipFuncAttributes a;
    hipError_t e = hipFuncGetAttributes(&a, (const void *)k_tffh_pred_uv);
    if (e == hipSuccess)
        e = hipFuncGetAttributes(&a, (const void *)k_tffh_norm_uv);
    return e != hipSuccess ? e : hipFuncGetAttributes(&a, (const void *)k_tffh_norm_uv_pic);
}
