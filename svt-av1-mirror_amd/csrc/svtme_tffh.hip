// svtme_tffh.hip — temporal filtering's luma prediction and weighting on 10-bit
// pictures (svtme_tf_filter_10bit, svtme_tf_window_10bit, include/svtme.h): what
// produce_temporally_filtered_pic does after the sub-pel refinement when is_highbd
// is set (temporal_filtering.c:3196-3390). The sub-pel results are those of the
// 8-bit search on the MSB planes (use_8bit_subpel == 1); everything here reads the
// resident 16-bit planes (svtme_picture_attach_10bit). use_zz_based_filter == 0,
// luma only. svtme_tff.hip, the 8-bit stage, is left as it is: these are kernels of
// their own with their own copies of the three tables.
//
// k_tffh_pred, one 256-thread workgroup per (reference, SB): k_tff_pred's unit list
// (the blocks, the MV clamp, position and phase do not depend on the bit depth), a
// wavefront per unit, the prediction into the SB's 64x64 u16 tile in LDS, then per
// 32x32 block the SSE of the four 16x16 quarters and, on the 64x64 branches, sum and
// SSE of the rows sub_sampling_shift keeps. One lane per quarter derives the weight.
// The tile (8 KB), the 16 weights and the 4 errors go to the context's scratch.
//
// k_tffh_norm, one workgroup per SB: 1000 x centre plus the weighted tiles,
// normalised, 16 pixels per thread, into a dense u16 plane of whole SBs.
// k_tffh_norm_pic: the same into the result picture's 16-bit plane and, >> 2, into
// its level 0 (what svt_unpack_and_2bcompress leaves as the 8-bit plane,
// temporal_filtering.c:193-211, 4261-4287), inside the aligned picture only.
//
// LDS of k_tffh_pred (33.6 KB: four workgroups a CU, as k_tff_pred):
//  * the staged window of a unit, per wavefront: rows of b + 8 samples in b / 2 + 4
//    dwords at a pitch of b / 2 + 5 dwords (37, 21, 13, 9 for b = 64, 32, 16, 8): the
//    pitch follows the unit instead of doubling the 8-bit one. A 32-lane half reads
//    one row (b >= 32), two rows (b = 16, 8 dwords each, 13 apart) or four (b = 8, 4
//    dwords each, 9 apart): no two rows of a half share a bank at any tap. The tallest
//    are the 64x16 slab, 23 x 37 = 851 dwords, and the 32x32 block, 39 x 21 = 819.
//  * the intermediate of the 2-D case, int16 at a pitch of b: 23 x 64 = 1472 values.
//  * the tile, 8 KB. The centre block (8 KB) is loaded into registers at the start and
//    stored, after the last prediction, over the intermediates, which are dead by then.
//
// Semantics restated (reference line beside each):
//  * svt_highbd_inter_predictor with get_conv_params_no_round(.., bd 10): round_0 3,
//    round_1 11 (convolve.h:40-60: widened only at 12 bit); the four cases
//    svt_av1_highbd_convolve_2d_sr_c (offset 1 << (bd + FILTER_BITS - 1) = 1 << 16 in
//    the horizontal pass, offset_bits bd + 2 FILTER_BITS - round_0 = 21 in the
//    vertical), _x_sr_c, _y_sr_c and the copy (inter_prediction.c:670-777);
//    clip_pixel_highbd(.., 10). The intermediate is below 1 << 15.
//  * svt_aom_highbd_10_variance32x32_c / 32x16_c (svt_psnr.c:139-177) on the 64x64
//    branches (convert_64x64_info_to_32x32_info, temporal_filtering.c:2736-2754): SSE
//    rounded by 4 bits, sum by 2, sse - sum^2 / N clamped at 0, << sub_sampling_shift.
//  * svt_av1_apply_temporal_filter_planewise_medium_hbd_partial_c, is_chroma 0
//    (:1211-1333): the 8-bit function with the quarter's SSE >> (bd - 8) * 2
//    (:792-801) and with the block errors scaled too: the 16x16 error >> 4 of a split
//    block (:1241), the 32x32 error >> 6 of an unsplit one (:1256; 8 bit: >> 0, >> 2).
//  * svt_aom_apply_filtering_central_highbd_c (:386-407): 1000 x source, count 1000;
//    svt_aom_get_final_filtered_pixels_c, is_highbd (:2645-2655).
//
// Reads stay inside the 16-bit plane (svtme_hbd_geometry: 80 samples left, at least
// 88 right, 72 rows above and below, the 8-bit level 0's margins in samples): the
// clamp keeps a block's first sample in [-(4 + b), W + 3], the staged window starts 3
// before at an even sample at or after -72 and its b / 2 + 5 dwords end at or before
// W + 73; rows -71 .. H + 71.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svtme_launch.h"
#include "svtme_me_common.h"

using namespace svtme;

struct TffhArgs {
    DevPlane cen;                       // the centre picture's 16-bit plane (stride in bytes)
    DevPlane ref[SVTME_MAX_BATCH_JOBS]; // the references'
    const svtme_tf_subpel_sb *sub;      // [n][sbs]
    uint16_t *tile;                     // [n][sbs][64 * 64] predictions
    uint32_t *wgt;                      // [n][sbs][16] weights, 32x32 block * 4 + quarter
    uint32_t *e32;                      // [n][sbs][4] 32x32 errors
    uint16_t *plane;                    // k_tffh_norm: the filtered plane, whole SBs, pic_w_b64 * 64 samples a row
    DevPlane dst;                       // k_tffh_norm_pic: the result picture's 16-bit plane (may be cen)
    DevPlane dst8;                      //                  and its level 0
    uint32_t decay, dist_th, ss;        // svtme_tf_filter_controls
    uint32_t n, sbs, pic_w_b64;
    int32_t W, H; // the 8-aligned picture
};

#define TFFH_WIN_DW 851 // 23 rows x 37 dwords: the 64x16 slab
#define TFFH_IM 1472    // 23 rows x 64 values
#define TFFH_UNITS 64

// AV1 specification, Subpel_Filters[2] (MULTITAP_SHARP), phases 0..15
__constant__ int16_t c_tffh_sharp[16][8] = {
    {0, 0, 0, 128, 0, 0, 0, 0},          {-2, 2, -6, 126, 8, -2, 2, 0},       {-2, 6, -12, 124, 16, -6, 4, -2},
    {-2, 8, -18, 120, 26, -10, 6, -2},   {-4, 10, -22, 116, 38, -14, 6, -2},  {-4, 10, -22, 108, 48, -18, 8, -2},
    {-4, 10, -24, 100, 60, -20, 8, -2},  {-4, 10, -24, 90, 70, -22, 10, -2},  {-4, 12, -24, 80, 80, -24, 12, -4},
    {-2, 10, -22, 70, 90, -24, 10, -4},  {-2, 8, -20, 60, 100, -24, 10, -4},  {-2, 8, -18, 48, 108, -22, 10, -4},
    {-2, 6, -14, 38, 116, -22, 10, -4},  {-2, 6, -10, 26, 120, -18, 8, -2},   {-2, 4, -6, 16, 124, -12, 6, -2},
    {0, 2, -2, 8, 126, -6, 2, -2}};

// floor(exp(-i / 16) * 2^16) and floor(sqrt(i) * 2^16), computed as svtme_tff.hip computes them
struct TffhExpTab {
    int32_t v[113];
};
constexpr TffhExpTab tffh_make_exp() {
    TffhExpTab t{};
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
struct TffhSqrtTab {
    uint32_t v[16];
};
constexpr TffhSqrtTab tffh_make_sqrt() {
    TffhSqrtTab t{};
    for (uint64_t i = 0; i < 16; i++) {
        uint64_t r = 0;
        for (int bit = 19; bit >= 0; bit--)
            if ((r | (1ull << bit)) * (r | (1ull << bit)) <= (i << 32))
                r |= 1ull << bit;
        t.v[i] = (uint32_t)r;
    }
    return t;
}
__constant__ TffhExpTab c_tffh_exp   = tffh_make_exp();
__constant__ TffhSqrtTab c_tffh_sqrt = tffh_make_sqrt();

typedef __attribute__((address_space(1))) const uint32_t gh_u32; // global, not flat, loads

__device__ __forceinline__ int tffh_clip10(int v) { return v < 0 ? 0 : v > 1023 ? 1023 : v; }

// taps along a row of samples (p at tap 0)
__device__ __forceinline__ int tffh_hsum(const uint16_t *p, const int t[8]) {
    return t[0] * p[0] + t[1] * p[1] + t[2] * p[2] + t[3] * p[3] + t[4] * p[4] + t[5] * p[5] + t[6] * p[6] + t[7] * p[7];
}

// sqrt_fast (temporal_filtering.c:740-749)
__device__ __forceinline__ uint32_t tffh_sqrt_fast(uint32_t x) {
    if (x > 15) {
        const int log2_half = (31 - __clz((int)x)) >> 1;
        const int base      = (int)(x >> (2 * log2_half - 2));
        return c_tffh_sqrt.v[base] >> (17 - log2_half);
    }
    return c_tffh_sqrt.v[x] >> 16;
}

// One unit on one wavefront: rows [oy, oy + h) of the b x b block at (px, py) of the picture, (bx, by)
// of the SB, predicted at the 1/8-pel MV into the SB's tile. `on` is wave-uniform; every wavefront
// of the workgroup calls this the same number of times (workgroup barriers inside).
__device__ void tffh_predict(const TffhArgs &A, const DevPlane &R, uint32_t *win, int16_t *im, uint16_t *tile, int lane,
                             bool on, int b, int px, int py, int bx, int by, int oy, int h, int mvx, int mvy) {
    int fx = 0, fy = 0;
    const int wp = (b >> 1) + 5; // dwords per staged row
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
        // the window: sample c of staged row r is plane sample (x0 - 3 + c, y0 - 3 + r)
        const int wx = x0 - 3, shs = wx & 1, ndw = (b >> 1) + 4, rows = h + 7;
        const uint8_t *wpt = uni_ptr(R.base + (ptrdiff_t)(y0 - 3) * R.stride + (ptrdiff_t)(wx - shs) * 2);
        const int rst      = UNI(R.stride);
        const uint32_t m   = magic_u32((uint32_t)ndw);
#pragma unroll 4
        for (int i = lane; i < rows * ndw; i += 64) {
            const int row = mdiv(i, m), j = i - row * ndw;
            const gh_u32 *p = (const gh_u32 *)(uintptr_t)(wpt + (ptrdiff_t)row * rst) + j;
            win[row * wp + j] = __builtin_amdgcn_alignbyte(p[1], p[0], (uint32_t)(shs * 2));
        }
    }
    __syncthreads();
    const uint16_t *ws = (const uint16_t *)win;
    const int wps = wp * 2; // samples per staged row
    const int col = lane & (b - 1), rsub = b == 64 ? 0 : lane / b, rpi = 64 / b;
    int tx[8], ty[8];
    if (on) {
#pragma unroll
        for (int k = 0; k < 8; k++) tx[k] = UNI((int)c_tffh_sharp[fx][k]), ty[k] = UNI((int)c_tffh_sharp[fy][k]);
        if (fx && fy) // horizontal pass of svt_av1_highbd_convolve_2d_sr_c: bd 10, round_0 3
#pragma unroll 2
            for (int r = rsub; r < h + 7; r += rpi)
                im[r * b + col] = (int16_t)(((1 << 16) + tffh_hsum(ws + r * wps + col, tx) + 4) >> 3);
    }
    __syncthreads();
    if (on) {
        uint16_t *tp = tile + (by + oy) * 64 + bx + col;
#pragma unroll 2
        for (int y = rsub; y < h; y += rpi) {
            int v;
            if (fx && fy) { // vertical pass: offset_bits 21, round_1 11, bits 0
                int s = 1 << 21;
#pragma unroll
                for (int k = 0; k < 8; k++) s += ty[k] * im[(y + k) * b + col];
                v = tffh_clip10(((s + 1024) >> 11) - ((1 << 10) + (1 << 9)));
            } else if (fx) { // svt_av1_highbd_convolve_x_sr_c: round_0 3, then FILTER_BITS - round_0
                const int s = (tffh_hsum(ws + (y + 3) * wps + col, tx) + 4) >> 3;
                v           = tffh_clip10((s + 8) >> 4);
            } else if (fy) { // svt_av1_highbd_convolve_y_sr_c: FILTER_BITS
                const uint16_t *p = ws + y * wps + col + 3;
                int s             = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) s += ty[k] * p[k * wps];
                v = tffh_clip10((s + 64) >> 7);
            } else {
                v = ws[(y + 3) * wps + col + 3];
            }
            tp[y * 64] = (uint16_t)v;
        }
    }
}

__global__ void __launch_bounds__(256) k_tffh_pred(const TffhArgs A) {
    __shared__ uint32_t s_win[4][TFFH_WIN_DW];
    __shared__ __attribute__((aligned(16))) int16_t s_im[4][TFFH_IM]; // then the centre block: 8192 of its 11776 bytes
    __shared__ uint4 s_tile[64 * 8];                                  // the SB's prediction, 64 x 64 u16
    __shared__ uint32_t s_unit[TFFH_UNITS]; // level | index << 2
    __shared__ int s_units;
    __shared__ uint32_t s_sse[16], s_e32[4];
    static_assert(sizeof(s_im) >= 64 * 64 * 2, "the centre block fits the intermediates");
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

    // the centre block: row tid / 4, 16 samples at column 16 (tid % 4) (32-byte steps from a 16-byte aligned row
    // start); kept in registers until the intermediates are dead
    const uint4 *cp = (const uint4 *)(A.cen.base + (ptrdiff_t)(sb_y + (tid >> 2)) * A.cen.stride +
                                      (ptrdiff_t)(sb_x + (tid & 3) * 16) * 2);
    const uint4 c0 = cp[0], c1 = cp[1];
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
        tffh_predict(A, R, s_win[wid], s_im[wid], (uint16_t *)s_tile, lane, on, b, sb_x + bx, sb_y + by, bx, by, oy, h,
                     (int16_t)(mv & 0xFFFF), (int16_t)(mv >> 16));
    }
    __syncthreads(); // every prediction is in the tile and no intermediate is read any more
    uint4 *s_cen = (uint4 *)&s_im[0][0];
    s_cen[tid * 2] = c0, s_cen[tid * 2 + 1] = c1;
    __syncthreads();

    // wavefront wid: the 32x32 block wid, a 16x16 quarter at a time, lane = row * 4 + the row's group of 4 samples
    {
        const int X = (wid & 1) * 32, Y = (wid >> 1) * 32, row = lane >> 2, g = lane & 3;
        const bool kept = (row & (int)A.ss) == 0;
        uint32_t sk = 0, ssek = 0;
        for (int q = 0; q < 4; q++) {
            const int off = (Y + (q >> 1) * 16 + row) * 64 + X + (q & 1) * 16 + g * 4; // samples, a multiple of 4
            const uint2 p = *(const uint2 *)((const uint16_t *)s_tile + off);
            const uint2 c = *(const uint2 *)((const uint16_t *)s_cen + off);
            const uint32_t pw[2] = {p.x, p.y}, cw[2] = {c.x, c.y};
            int sum = 0;
            uint32_t sse = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int d = (int)((pw[k >> 1] >> (16 * (k & 1))) & 0xFFFF) - (int)((cw[k >> 1] >> (16 * (k & 1))) & 0xFFFF);
                sum += d;
                sse += (uint32_t)(d * d);
            }
            sk += wave_sum_u32(kept ? (uint32_t)sum : 0u);
            ssek += wave_sum_u32(kept ? sse : 0u);
            sse = wave_sum_u32(sse);
            if (lane == 0)
                s_sse[wid * 4 + q] = sse >> 4; // calculate_squared_errors_sum_highbd: >> (bd - 8) * 2 (:800)
        }
        if (lane == 0) {
            // 64x64 branches: svt_aom_highbd_10_variance32x32_c / 32x16_c on the kept rows, << shift (:2746-2753)
            const uint32_t sse = (ssek + 8u) >> 4;
            const int sum      = ((int)sk + 2) >> 2;
            const int64_t var  = (int64_t)sse - (((int64_t)sum * sum) >> (10 - A.ss)); // / (32 * (32 >> shift))
            s_e32[wid] = b32 ? sub[85 + SVTME_TFSP_OFF_32 + wid] : (uint32_t)(var >= 0 ? var : 0) << A.ss;
        }
    }
    __syncthreads();

    // the tile, whole 16-byte vectors
    ((uint4 *)(A.tile + unit * 4096))[tid * 2]     = s_tile[tid * 2];
    ((uint4 *)(A.tile + unit * 4096))[tid * 2 + 1] = s_tile[tid * 2 + 1];
    if (tid < 4)
        A.e32[unit * 4 + tid] = s_e32[tid];
    if (tid < 16) {
        // svt_av1_apply_temporal_filter_planewise_medium_hbd_partial_c (:1211-1333), quarter tid % 4 of 32x32 block tid / 4
        const int i = tid >> 2;
        const uint32_t dth = (uint32_t)max((int)(A.dist_th << 16) / 10, 1 << 16);
        const bool split   = b32 && ((sub[170] >> (8 * i)) & 0xFF) != 0;
        const uint32_t mv  = sub[split ? SVTME_TFSP_OFF_16 + tid : b32 ? SVTME_TFSP_OFF_32 + i : 0];
        const uint32_t be  = split ? sub[85 + SVTME_TFSP_OFF_16 + tid] >> 4 : s_e32[i] >> 6; // (:1241, :1256)
        const uint32_t dec = split ? A.decay : A.decay << 1;
        const int col = (int16_t)(mv & 0xFFFF), row = (int16_t)(mv >> 16);
        const uint32_t d2   = (uint32_t)col * (uint32_t)col + (uint32_t)row * (uint32_t)row;
        const uint32_t dist = tffh_sqrt_fast(d2 << 8);
        uint32_t dfac       = (dist << 12) / (dth >> 8);
        dfac                = dfac > 256u ? dfac : 256u;
        const uint32_t comb = (s_sse[tid] * 5u + be) / 6u;
        const uint32_t avg  = (comb >> 3) * (dfac >> 3);
        const uint32_t dd   = (dec >> 10) ? (dec >> 10) : 1u;
        uint32_t sd         = avg / dd;
        sd                  = sd < 112u ? sd : 112u;
        A.wgt[unit * 16 + tid] = (uint32_t)(c_tffh_exp.v[sd] * 1000) >> 16;
    }
}

// The normalisation of 16 pixels of one row of SB b64: row tid / 4, columns 16 (tid % 4) .. + 15 (all in
// one 16x16 quarter), two samples a dword. The only centre samples read are those 16.
__device__ __forceinline__ void tffh_norm16(const TffhArgs &A, uint32_t b64, uint32_t sbx, uint32_t sby, int tid,
                                            uint32_t o[8]) {
    const int row = tid >> 2, c16 = tid & 3;
    const int wi = ((row >> 5) * 2 + (c16 >> 1)) * 4 + ((row >> 4) & 1) * 2 + (c16 & 1);
    const uint4 *cp = (const uint4 *)(A.cen.base + (ptrdiff_t)((int)sby * 64 + row) * A.cen.stride +
                                      (ptrdiff_t)((int)sbx * 64 + c16 * 16) * 2);
    const uint4 ca = cp[0], cb = cp[1];
    const uint32_t cw[8] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
    uint32_t acc[16], cnt = 1000; // svt_aom_apply_filtering_central_highbd_c (:401-407)
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = 1000u * ((cw[k >> 1] >> (16 * (k & 1))) & 0xFFFF);
    for (uint32_t r = 0; r < A.n; r++) {
        const size_t unit = (size_t)r * A.sbs + b64;
        const uint32_t w  = A.wgt[unit * 16 + wi];
        const uint4 *tp   = (const uint4 *)(A.tile + unit * 4096) + tid * 2;
        const uint4 pa = tp[0], pb = tp[1];
        const uint32_t pw[8] = {pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, pb.z, pb.w};
        cnt += w; // (:1328-1329)
#pragma unroll
        for (int k = 0; k < 16; k++) acc[k] += w * ((pw[k >> 1] >> (16 * (k & 1))) & 0xFFFF);
    }
    // (accum + (count >> 1)) / count (:2650): count <= 17000 and accum < 2^25, so the high product by
    // 2^32 / count rounded up is the quotient or one more (the excess is below accum / 2^32)
    const uint32_t m = 0xFFFFFFFFu / cnt + 1u;
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t v = acc[k] + (cnt >> 1);
        uint32_t q       = __umulhi(v, m);
        q -= q * cnt > v;
        o[k >> 1] |= (q & 0xFFFFu) << (16 * (k & 1));
    }
}

__global__ void __launch_bounds__(256) k_tffh_norm(const TffhArgs A) {
    const int tid      = threadIdx.x;
    const uint32_t b64 = blockIdx.x;
    const uint32_t sby = b64 / A.pic_w_b64, sbx = b64 - sby * A.pic_w_b64;
    const int row = tid >> 2, c16 = tid & 3;
    uint32_t o[8];
    tffh_norm16(A, b64, sbx, sby, tid, o);
    uint4 *op = (uint4 *)(A.plane + ((size_t)sby * 64 + row) * ((size_t)A.pic_w_b64 * 64) + (size_t)sbx * 64 + c16 * 16);
    op[0] = make_uint4(o[0], o[1], o[2], o[3]);
    op[1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// The same into the result picture: the 16-bit plane and, >> 2, level 0. Only samples x < W, y < H of
// the aligned picture are stored (W is a multiple of 8: a thread's 16 pixels are all inside, the first
// 8 inside, or all outside); the margins are the padding kernels' to write afterwards. A.dst may be
// A.cen (in place): a thread reads from the centre's 16-bit plane its own 16 pixels alone, before it
// stores them, and nobody reads the samples nobody stores. Nothing here reads level 0.
__global__ void __launch_bounds__(256) k_tffh_norm_pic(const TffhArgs A) {
    const int tid      = threadIdx.x;
    const uint32_t b64 = blockIdx.x;
    const uint32_t sby = b64 / A.pic_w_b64, sbx = b64 - sby * A.pic_w_b64;
    const int x = (int)sbx * 64 + (tid & 3) * 16, y = (int)sby * 64 + (tid >> 2);
    if (x >= A.W || y >= A.H)
        return;
    uint32_t o[8];
    tffh_norm16(A, b64, sbx, sby, tid, o);
    uint32_t m[4]; // the MSB plane: four samples a dword
#pragma unroll
    for (int k = 0; k < 4; k++)
        m[k] = ((o[2 * k] & 0xFFFFu) >> 2) | (((o[2 * k] >> 16) >> 2) << 8) | (((o[2 * k + 1] & 0xFFFFu) >> 2) << 16) |
               (((o[2 * k + 1] >> 16) >> 2) << 24);
    uint4 *op   = (uint4 *)(A.dst.base + (ptrdiff_t)y * A.dst.stride + (ptrdiff_t)x * 2); // 16-byte aligned
    uint8_t *o8 = A.dst8.base + (ptrdiff_t)y * A.dst8.stride + x;
    op[0] = make_uint4(o[0], o[1], o[2], o[3]);
    if (x + 16 <= A.W) {
        op[1]        = make_uint4(o[4], o[5], o[6], o[7]);
        *(uint4 *)o8 = make_uint4(m[0], m[1], m[2], m[3]);
    } else
        *(uint2 *)o8 = make_uint2(m[0], m[1]);
}

// The padded 16-bit plane from w x h true samples, two samples a thread: the replication to the
// aligned size and the margins are one clamp of the source coordinate (k_build_full's scheme). With
// pad_only the source is the plane's own interior: the dwords wholly inside it are left alone, the
// others are written from samples no thread changes.
__global__ void __launch_bounds__(256) k_build_full16(const uint16_t *src, uint32_t src_stride, int w, int h,
                                                      DevPlane dst, int left, int top, int rows, int pad_only) {
    const int dw_per_row = dst.stride >> 2;
    const int idx        = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= dw_per_row * rows)
        return;
    const int ry = idx / dw_per_row, x0 = (idx - ry * dw_per_row) * 2 - left;
    if (pad_only && x0 >= 0 && x0 + 1 < w && ry >= top && ry - top < h)
        return;
    const int y  = min(max(ry - top, 0), h - 1);
    const int xa = min(max(x0, 0), w - 1), xb = min(max(x0 + 1, 0), w - 1);
    const uint16_t *sr = src + (size_t)y * src_stride;
    uint32_t *row = (uint32_t *)(dst.base - (ptrdiff_t)top * dst.stride - (ptrdiff_t)left * 2);
    row[idx]      = (uint32_t)sr[xa] | ((uint32_t)sr[xb] << 16);
}

extern "C" hipError_t svtme_launch_build_full16(const uint16_t *src, uint32_t src_stride, int w, int h, DevPlane dst,
                                                int left, int top, int rows, hipStream_t s) {
    const int n        = (dst.stride >> 2) * rows;
    const int pad_only = (const uint8_t *)src == dst.base && src_stride * 2 == (uint32_t)dst.stride;
    hipLaunchKernelGGL(k_build_full16, dim3((n + 255) / 256), dim3(256), 0, s, src, src_stride, w, h, dst, left, top,
                       rows, pad_only);
    return hipGetLastError();
}

static hipError_t tffh_args(TffhArgs &A, const DevPlane *cen, const DevPlane *ref, uint32_t n, uint32_t width,
                            uint32_t height, const svtme_tf_filter_controls *ctl, const svtme_tf_subpel_sb *d_sub,
                            uint16_t *d_tile, uint32_t *d_wgt, uint32_t *d_e32) {
    if (!n || n > SVTME_MAX_BATCH_JOBS)
        return hipErrorInvalidValue;
    if (cen->width != (int32_t)width || cen->height != (int32_t)height)
        return hipErrorInvalidValue;
    for (uint32_t k = 0; k < n; k++)
        if (ref[k].width != (int32_t)width || ref[k].height != (int32_t)height)
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

// n references of one window: the predictions and weights in one launch, then the normalisation
extern "C" hipError_t svtme_launch_tffh(const DevPlane *cen, const DevPlane *ref, uint32_t n, uint32_t width,
                                        uint32_t height, const svtme_tf_filter_controls *ctl,
                                        const svtme_tf_subpel_sb *d_sub, uint16_t *d_tile, uint32_t *d_wgt,
                                        uint32_t *d_e32, uint16_t *d_plane, hipStream_t s) {
    TffhArgs A{};
    const hipError_t e = tffh_args(A, cen, ref, n, width, height, ctl, d_sub, d_tile, d_wgt, d_e32);
    if (e != hipSuccess)
        return e;
    A.plane = d_plane;
    hipLaunchKernelGGL(k_tffh_pred, dim3(n * A.sbs), dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_tffh_norm, dim3(A.sbs), dim3(256), 0, s, A);
    return hipGetLastError();
}

// svtme_tf_window_10bit: the same two steps, the normalisation into the result picture's 16-bit plane
// `dst` (it may be the centre's) and its level 0 `dst8`, both width x height
extern "C" hipError_t svtme_launch_tffh_pic(const DevPlane *cen, const DevPlane *ref, uint32_t n, uint32_t width,
                                            uint32_t height, const svtme_tf_filter_controls *ctl,
                                            const svtme_tf_subpel_sb *d_sub, uint16_t *d_tile, uint32_t *d_wgt,
                                            uint32_t *d_e32, const DevPlane *dst, const DevPlane *dst8, hipStream_t s) {
    TffhArgs A{};
    const hipError_t e = tffh_args(A, cen, ref, n, width, height, ctl, d_sub, d_tile, d_wgt, d_e32);
    if (e != hipSuccess)
        return e;
    if (dst->width != (int32_t)width || dst->height != (int32_t)height || dst8->width != (int32_t)width ||
        dst8->height != (int32_t)height)
        return hipErrorInvalidValue;
    A.dst = *dst, A.dst8 = *dst8;
    hipLaunchKernelGGL(k_tffh_pred, dim3(n * A.sbs), dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_tffh_norm_pic, dim3(A.sbs), dim3(256), 0, s, A);
    return hipGetLastError();
}

extern "C" hipError_t svtme_prime_tffh(void) { // (see svtme_prime_pyramid)
    hipFuncAttributes a;
    hipError_t e = hipFuncGetAttributes(&a, (const void *)k_tffh_pred);
    if (e == hipSuccess)
        e = hipFuncGetAttributes(&a, (const void *)k_tffh_norm);
    if (e == hipSuccess)
        e = hipFuncGetAttributes(&a, (const void *)k_build_full16);
    return e != hipSuccess ? e : hipFuncGetAttributes(&a, (const void *)k_tffh_norm_pic);
}
