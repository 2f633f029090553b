// svtme_tff.hip — temporal filtering's prediction and weighting as a picture-window
// job (svtme_tf_filter, svtme_tf_window and their _yuv, _10bit and _yuv_10bit forms,
// include/svtme.h): what produce_temporally_filtered_pic does with the sub-pel stage's
// result (temporal_filtering.c:3196-3390): the final inter prediction of every block,
// the 32x32 errors of the 64x64 branches, the per-16x16 filter weights, the accumulation
// over the window and the normalisation. use_zz_based_filter == 0 only. Luma, and with
// tf_chroma set 4:2:0 chroma; 8 bit on level 0 and the attached chroma planes, 10 bit
// (is_highbd; the sub-pel results are those of the 8-bit search on the MSB planes,
// use_8bit_subpel == 1) on the attached 16-bit planes. The kernels are templates over the
// sample type T (uint8_t, uint16_t); their shared parts are svtme_tf_common.h's.
//
// The luma stage.
//
// k_tff_pred<T> (a body per depth over the shared tff_pred_units and tff_pred_finish: they
// differ around the centre block, below), one 256-thread workgroup per (reference, SB), the
// whole window in one launch. Wavefront 0 turns the SB's branch and split flags into a list
// of units (tf_unit_list; the blocks, the MV clamp, position and phase do not depend on the bit
// depth). A wavefront takes one unit at a time (tf_predict): it stages the unit's window
// in its own LDS slice (aligned dwords, v_alignbyte), runs the horizontal pass into an
// int16 LDS plane when both phases are non-zero, then the vertical pass / the x-only,
// y-only or copy case, and writes the samples into the SB's 64x64 tile in LDS. Then every
// wavefront reduces, for the four 16x16 quarters of its 32x32 block, the SSE of centre
// against prediction and (64x64 branches) sum and SSE of the rows sub_sampling_shift
// keeps (DPP). One lane per quarter derives the weight (tf_weight). The tile (4 KB, 8 KB
// at 10 bit), the 16 weights and the 4 errors go to the context's device scratch.
//
// LDS of k_tff_pred (four workgroups a CU at either depth), with TfLayout's windows and
// intermediates:
//  * 8 bit, 39.4 KB: the centre block (4 KB) has LDS of its own beside the tile (4 KB).
//  * 10 bit, 33.1 KB: the tile is 8 KB. The centre block (8 KB) is loaded into registers at
//    the start and stored, after the last prediction, over the intermediates, which are
//    dead by then.
//
// k_tff_norm<T, false>, one workgroup per SB: 1000 x centre plus the weighted tiles of
// the references, normalised, 16 samples per thread, into a dense device plane of whole
// SBs, which the host copies out row by row.
//
// k_tff_norm<T, true> (the window calls), the same normalisation straight into the
// result picture, inside the aligned picture only: at 8 bit the padded level 0, at 10 bit
// the 16-bit plane and, >> 2, level 0 (what svt_unpack_and_2bcompress leaves as the 8-bit
// plane, temporal_filtering.c:193-211, 4261-4287). The destination may be the centre
// picture's own plane.
//
// The chroma stage (the _yuv calls), launched after k_tff_pred on the same stream.
//
// k_tff_pred_uv<T>, one 256-thread workgroup per (reference, SB): the SB's 32x32 Cb and Cr
// tiles from the same unit list, a wavefront per (unit, plane); the per-8x8 SSE of both
// planes against the centre; the 16 luma window errors, RECOMPUTED from k_tff_pred's luma
// tile and the centre's luma block (8 KB of reads per workgroup, 16 KB at 10 bit, that hit
// the L2); 2 x 16 weights. Tiles and weights go to their own sections of the scratch.
// LDS: 20.9 KB at 8 bit, 17.1 KB at 10 bit: TfLayout's windows and intermediates, the two
// tiles and the centre's two 32x32 blocks (2 KB each at 8 bit, 4 KB at 10).
//
// k_tff_norm_uv<T, false>, one workgroup per SB: the luma scheme (tff_norm) on both planes, 8 samples
// per thread (one 8x8 quarter, one weight per reference), into two dense planes of whole
// SBs. k_tff_norm_uv<T, true>: the same into the result picture's chroma planes, inside
// W/2 x H/2 only. W/2 is a multiple of 4, not of 8: a thread's 8 samples are all inside,
// the first 4 inside, or all outside.
//
// Semantics restated (reference line beside each; 8 bit | 10 bit where they differ):
//  * tf_64x64_inter_prediction (temporal_filtering.c:2255-2361): one 64x64 block at
//    mv[0]; tf_32x32_inter_prediction (:2362-2605): per 32x32 block 32x32 at mv[1 + i]
//    when split_32x32[i] is 0, else per 16x16 block 16x16 at mv[5 + 4 i + j], or four 8x8
//    at mv[21 + 16 i + 4 j + l] where split_16x16[i][j] is set. The interpolation filter
//    is MULTITAP_SHARP at every size (:2261, :2368). PICTURE_BUFFER_DESC_FULL_MASK: a luma
//    block of size b at (px, py) predicts a b/2 x b/2 block of Cb and of Cr at (px / 2,
//    py / 2) (svt_aom_inter_prediction, enc_inter_prediction.c:4248-4360:
//    svt_aom_enc_make_inter_predictor | svt_highbd_inter_predictor with
//    get_conv_params_no_round(.., bd 10); ss_x = ss_y = 1 for chroma).
//  * the MV clamp, the four convolve cases and the chroma filter choice: at tf_predict.
//  * convert_64x64_info_to_32x32_info (:2690-2757): on the 64x64 branches the 32x32 MVs are
//    the 64x64 MV, no block is split, and the 32x32 error is the variance of the final
//    prediction against the centre block over the rows sub_sampling_shift keeps, << shift
//    (:2726-2734 | :2736-2754; tf_var32).
//  * the weights: svt_av1_apply_temporal_filter_planewise_medium_partial_c |
//    _medium_hbd_partial_c with is_chroma 0 on each 32x32 block
//    (apply_filtering_block_plane_wise, :1411-1493, BW >> 1) and with is_chroma 1 per 32x32
//    luma block on its 16x16 chroma block and 8x8 quarters, from the luma MVs and block
//    errors: at tf_weight.
//  * svt_aom_apply_filtering_central_c (:349-380) | svt_aom_apply_filtering_central_highbd_c
//    (:386-407): 1000 x source, count 1000; count += weight (:1137-1138 | :1328-1329);
//    svt_aom_get_final_filtered_pixels_c (:2607-2644 | :2645-2655): (accum + (count >> 1)) /
//    count.
//
// Reads stay inside the planes.
//  * 8-bit luma, the device full plane exactly as in svtme_tfsp.hip: the predictor has the
//    same 8 taps (3 left / above, 4 right / below) and the same clamp, a unit's window is a
//    part of its block's (b + 7) x (b + 7) window, and the staging reads the same aligned
//    dwords. The centre block reads x in [px, px + 63], px <= W - 8, rows up
//    to py + 63 <= H + 55.
//  * 8-bit chroma (svtme_device.h: 48 bytes left and at least 48 right of W/2, 40 rows
//    above and below H/2): the clamp keeps a block's first sample in
//    [-(4 + b), W/2 + 3], and at W/2 + 3 or -(4 + b) exactly only with phase 0; the staged
//    window starts 3 before, at a dword at or after -40, and ends before W/2 + 44; rows
//    -39 .. H/2 + 38. The centre blocks read x <= W/2 + 27, y <= H/2 + 27.
//  * 16-bit luma (svtme_hbd_geometry: 80 samples left, at least 88 right, 72 rows above and
//    below, the 8-bit level 0's margins in samples): the clamp keeps a block's first sample
//    in [-(4 + b), W + 3], the staged window starts 3 before at an even sample at or after
//    -72 and its b / 2 + 5 dwords end at or before W + 73; rows -71 .. H + 71.
//  * 16-bit chroma (svtme_hbd_chroma_geometry: 48 samples left and at least 48 right of
//    W/2, 40 rows above and below H/2): the clamp keeps a block's first sample in
//    [-(4 + b), W/2 + 3]; the staged window starts 3 before at an even sample at or after
//    -40, and its b / 2 + 5 dwords (the last one read for the alignment alone) end at or
//    before sample W/2 + 41; rows -39 .. H/2 + 38. The centre blocks read x <= W/2 + 27,
//    y <= H/2 + 27.
// svtme_launch_tf_stage checks every plane's size against the window's before it launches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svtme_launch.h"
#include "svtme_tf_common.h"

using namespace svtme;

// the work of a prediction workgroup: SB b64 at (sbx, sby) of reference ri
struct TffSb {
    uint32_t ri;
    size_t unit;         // ri * sbs + b64: its place in every scratch section
    const uint32_t *sub; // its sub-pel result: 85 MVs, 85 errors, 5 dwords of flags, branch
    int x, y;            // the SB's luma origin
    bool b32;            // the 32x32 branch; else one 64x64 block
};
template <typename Args>
__device__ __forceinline__ TffSb tff_sb_of_wg(const Args &A) {
    const uint32_t u   = UNI(xcd_remap(blockIdx.x, gridDim.x));
    const uint32_t ri  = UNI(u / A.sbs), b64 = u - ri * A.sbs;
    const uint32_t sby = UNI(b64 / A.pic_w_b64), sbx = b64 - sby * A.pic_w_b64;
    const size_t unit   = (size_t)ri * A.sbs + b64;
    const uint32_t *sub = uni_ptr((const uint32_t *)(A.sub + unit));
    return {ri, unit, sub, (int)sbx * 64, (int)sby * 64, UNI(sub[175] & 0xFF) == SVTME_TFSP_32};
}

// The luma prediction kernel's two parts that do not depend on where the centre block waits.
// The predictions: a wavefront takes one unit of the list at a time into the SB's tile.
template <typename T>
__device__ __forceinline__ void tff_pred_units(const TfLumaArgs &A, const TffSb &sb, const uint32_t *s_unit, int units,
                                               uint32_t *win, int16_t *im, T *tile) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    DevPlane R = A.ref[0];
#pragma unroll
    for (int k = 1; k < SVTME_MAX_BATCH_JOBS; k++) // constant-index argument reads
        if (sb.ri == (uint32_t)k)
            R = A.ref[k];
    for (int u0 = 0; u0 < units; u0 += 4) {
        const int un  = u0 + wid;
        const bool on = un < units;
        const TfUnit t    = tf_unit_decode<0>(UNI(s_unit[on ? un : 0]));
        const uint32_t mv = sb.sub[t.mi];
        tf_predict<T, 0>(R.base, R.stride, A.W, A.H, win, im, tile, lane, on, t.b, sb.x + t.bx, sb.y + t.by, t.bx, t.by,
                         t.oy, t.h, (int16_t)(mv & 0xFFFF), (int16_t)(mv >> 16));
    }
}

// The errors, the weights and the outputs, from the tile and the centre block in LDS (both written and
// a barrier passed): wavefront wid has the 32x32 block wid, a 16x16 quarter at a time, lane = row * 4 +
// the row's group of 4 samples.
template <typename T>
__device__ __forceinline__ void tff_pred_finish(const TfLumaArgs &A, const TffSb &sb, const uint4 *s_tile,
                                                const uint4 *s_cen, uint32_t *s_sse, uint32_t *s_e32) {
    constexpr int BPP = (int)sizeof(T), DSH = (BPP - 1) * 4; // bytes a sample; (bd - 8) * 2
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t *sub = sb.sub;
    {
        const int X = (wid & 1) * 32, Y = (wid >> 1) * 32, row = lane >> 2, g = lane & 3;
        const bool kept = (row & (int)A.ss) == 0;
        uint32_t sk = 0, ssek = 0;
        for (int q = 0; q < 4; q++) {
            const int off = (Y + (q >> 1) * 16 + row) * 64 + X + (q & 1) * 16 + g * 4; // samples, a multiple of 4
            uint32_t p[4], c[4];
            tf_load<T, 4>((const uint8_t *)s_tile + off * BPP, p);
            tf_load<T, 4>((const uint8_t *)s_cen + off * BPP, c);
            int sum      = 0;
            uint32_t sse = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int d = (int)p[k] - (int)c[k];
                sum += d;
                sse += (uint32_t)(d * d);
            }
            sk += wave_sum_u32(kept ? (uint32_t)sum : 0u);
            ssek += wave_sum_u32(kept ? sse : 0u);
            sse = wave_sum_u32(sse);
            if (lane == 0)
                s_sse[wid * 4 + q] = sse >> DSH; // calculate_squared_errors_sum_highbd: >> (bd - 8) * 2 (:800)
        }
        if (lane == 0)
            s_e32[wid] = sb.b32 ? sub[85 + SVTME_TFSP_OFF_32 + wid] : tf_var32<T>((int)sk, ssek, (int)A.ss);
    }
    __syncthreads();

    // the tile, whole 16-byte vectors
#pragma unroll
    for (int i = 0; i < BPP; i++) ((uint4 *)(A.tile + sb.unit * (4096 * BPP)))[tid * BPP + i] = s_tile[tid * BPP + i];
    if (tid < 4)
        A.e32[sb.unit * 4 + tid] = s_e32[tid];
    if (tid < 16) // quarter tid % 4 of 32x32 block tid / 4
        A.wgt[sb.unit * 16 + tid] =
            tf_weight<false>(sub, sb.b32, tid, s_sse[tid], 0u, s_e32[tid >> 2], DSH, A.decay, A.dist_th);
}

// k_tff_pred has a body per depth: they are designed differently around the centre block.
template <typename T>
__global__ void k_tff_pred(const TfLumaArgs A);

// 8 bit: the centre block has LDS of its own from the start
template <>
__global__ void __launch_bounds__(256) k_tff_pred<uint8_t>(const TfLumaArgs A) {
    using L = TfLayout<uint8_t, 0>;
    __shared__ uint32_t s_win[4][L::WIN_DW];
    __shared__ int16_t s_im[4][L::IM];
    __shared__ uint4 s_cen[64 * 4];        // the SB's 64 x 64 block of the centre picture
    __shared__ uint4 s_tile[64 * 4];       // its prediction
    __shared__ uint32_t s_unit[TF_UNITS];  // level | index << 2
    __shared__ int s_units;
    __shared__ uint32_t s_sse[16], s_e32[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const TffSb sb = tff_sb_of_wg(A);
    // the centre block: row tid / 4, 16 bytes at column 16 (tid % 4) (16-byte aligned: sb.x is a multiple of 64)
    s_cen[tid] = *(const uint4 *)(A.cen.base + (ptrdiff_t)(sb.y + (tid >> 2)) * A.cen.stride + sb.x + (tid & 3) * 16);
    if (wid == 0)
        tf_unit_list(sb.sub, sb.b32, lane, s_unit, &s_units);
    __syncthreads();
    tff_pred_units<uint8_t>(A, sb, s_unit, s_units, s_win[wid], s_im[wid], (uint8_t *)s_tile);
    __syncthreads();
    tff_pred_finish<uint8_t>(A, sb, s_tile, s_cen, s_sse, s_e32);
}

// 10 bit: the centre block (8 KB) waits in registers and is stored, after the last prediction, over the
// intermediates, which are dead by then
template <>
__global__ void __launch_bounds__(256) k_tff_pred<uint16_t>(const TfLumaArgs A) {
    using L = TfLayout<uint16_t, 0>;
    __shared__ uint32_t s_win[4][L::WIN_DW];
    __shared__ __attribute__((aligned(16))) int16_t s_im[4][L::IM]; // then the centre block: 8192 of its 11776 bytes
    __shared__ uint4 s_tile[64 * 8];                                // the SB's prediction, 64 x 64 u16
    __shared__ uint32_t s_unit[TF_UNITS];                           // level | index << 2
    __shared__ int s_units;
    __shared__ uint32_t s_sse[16], s_e32[4];
    static_assert(sizeof(s_im) >= 64 * 64 * 2, "the centre block fits the intermediates");
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const TffSb sb = tff_sb_of_wg(A);
    // the centre block: row tid / 4, 16 samples at column 16 (tid % 4) (32-byte steps from a 16-byte aligned row start)
    const uint4 *cp = (const uint4 *)(A.cen.base + (ptrdiff_t)(sb.y + (tid >> 2)) * A.cen.stride +
                                      (ptrdiff_t)(sb.x + (tid & 3) * 16) * 2);
    const uint4 c0 = cp[0], c1 = cp[1];
    if (wid == 0)
        tf_unit_list(sb.sub, sb.b32, lane, s_unit, &s_units);
    __syncthreads();
    tff_pred_units<uint16_t>(A, sb, s_unit, s_units, s_win[wid], s_im[wid], (uint16_t *)s_tile);
    __syncthreads(); // every prediction is in the tile and no intermediate is read any more
    uint4 *s_cen = (uint4 *)&s_im[0][0];
    s_cen[tid * 2] = c0, s_cen[tid * 2 + 1] = c1;
    __syncthreads();
    tff_pred_finish<uint16_t>(A, sb, s_tile, s_cen, s_sse, s_e32);
}

template <typename T>
__global__ void __launch_bounds__(256) k_tff_pred_uv(const TfChromaArgs A) {
    using L = TfLayout<T, 1>;
    constexpr int BPP = (int)sizeof(T), DSH = (BPP - 1) * 4; // bytes a sample; (bd - 8) * 2
    constexpr int CVEC = 128 * BPP;                          // 16-byte vectors of two 32 x 32 blocks
    __shared__ uint32_t s_win[4][L::WIN_DW];
    __shared__ int16_t s_im[4][L::IM];
    __shared__ uint4 s_cen[CVEC];  // the SB's 32 x 32 blocks of the centre picture's Cb and Cr
    __shared__ uint4 s_tile[CVEC]; // their predictions
    __shared__ uint32_t s_unit[TF_UNITS]; // level | index << 2
    __shared__ int s_units;
    __shared__ uint32_t s_ssey[16], s_ssec[32];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const TffSb sb      = tff_sb_of_wg(A);
    const uint32_t *sub = sb.sub;
    const size_t unit   = sb.unit;
    const int sb_x = sb.x, sb_y = sb.y;
    const bool b32 = sb.b32;
    const uint8_t *rcb = A.ref[0][0], *rcr = A.ref[1][0];
#pragma unroll
    for (int k = 1; k < SVTME_MAX_BATCH_JOBS; k++) // constant-index argument reads
        if (sb.ri == (uint32_t)k)
            rcb = A.ref[0][k], rcr = A.ref[1][k];

    // the luma window errors: the SSE of k_tff_pred's tile against the centre block per 16x16 quarter,
    // >> (bd - 8) * 2; thread = row tid / 4, 16 samples at column 16 (tid % 4), a wavefront = 16 rows
    {
        uint32_t p[16], c[16];
        tf_load<T, 16>(A.tile_y + (unit * 256 + tid) * (16 * BPP), p);
        tf_load<T, 16>(A.cen_y.base + (ptrdiff_t)(sb_y + (tid >> 2)) * A.cen_y.stride + (ptrdiff_t)(sb_x + (tid & 3) * 16) * BPP,
                       c);
        uint32_t sse = tf_sse<16>(p, c);
#pragma unroll
        for (int m = 4; m < 64; m <<= 1) sse += (uint32_t)__shfl_xor((int)sse, m);
        if (lane < 4)
            s_ssey[tf_wi(lane, wid)] = sse >> DSH;
    }
    // the centre blocks, 16 bytes a thread: plane, row, and the row's 64 BPP bytes in turn (16-byte aligned)
    if (tid < CVEC) {
        const int pl = tid / (64 * BPP), row = (tid / (2 * BPP)) & 31, xb = (tid & (2 * BPP - 1)) * 16;
        const uint8_t *cb = pl ? A.cen[1].base : A.cen[0].base;
        const int cst     = pl ? A.cen[1].stride : A.cen[0].stride;
        s_cen[tid] = *(const uint4 *)(cb + (ptrdiff_t)((sb_y >> 1) + row) * cst + (ptrdiff_t)(sb_x >> 1) * BPP + xb);
    }
    if (wid == 0)
        tf_unit_list(sub, b32, lane, s_unit, &s_units);
    __syncthreads();

    // work item t: unit t / 2, plane t % 2
    const int items = s_units * 2;
    for (int t0 = 0; t0 < items; t0 += 4) {
        const int t   = t0 + wid;
        const bool on = t < items;
        const int pl  = t & 1;
        const TfUnit n    = tf_unit_decode<1>(UNI(s_unit[on ? t >> 1 : 0]));
        const uint32_t mv = sub[n.mi];
        tf_predict<T, 1>(pl ? rcr : rcb, A.ref_stride, A.W, A.H, s_win[wid], s_im[wid], (T *)s_tile + pl * 1024, lane, on,
                         n.b, sb_x + 2 * n.bx, sb_y + 2 * n.by, n.bx, n.by, n.oy, n.h, (int16_t)(mv & 0xFFFF),
                         (int16_t)(mv >> 16));
    }
    __syncthreads();

    // per 8x8 SSE: plane tid / 128, row (tid / 4) % 32, 8 samples at column 8 (tid % 4); the 8 rows of an
    // 8x8 block are 32 consecutive lanes of one wavefront
    {
        const int g = tid & 3, row = (tid >> 2) & 31;
        uint32_t p[8], c[8];
        tf_load<T, 8>((const uint8_t *)s_tile + tid * (8 * BPP), p);
        tf_load<T, 8>((const uint8_t *)s_cen + tid * (8 * BPP), c);
        uint32_t sse = tf_sse<8>(p, c);
#pragma unroll
        for (int m = 4; m < 32; m <<= 1) sse += (uint32_t)__shfl_xor((int)sse, m);
        if ((lane & 28) == 0)
            s_ssec[(tid >> 7) * 16 + tf_wi(g, row >> 3)] = sse >> DSH; // (:800)
    }
    __syncthreads();

    // the tiles, whole 16-byte vectors
    if (tid < CVEC)
        ((uint4 *)(A.tile + unit * (2048 * BPP)))[tid] = s_tile[tid];
    if (tid < 32) { // plane tid / 16, quarter q % 4 of 32x32 luma block q / 4
        const int q = tid & 15;
        A.wgt[unit * 32 + tid] = tf_weight<true>(sub, b32, q, s_ssec[tid], s_ssey[q], A.e32[unit * 4 + (q >> 2)], DSH,
                                                 tid < 16 ? A.decay_cb : A.decay_cr, A.dist_th);
    }
}

// the centre and result planes of a normalising thread's plane (constant-index argument reads)
__device__ __forceinline__ void tff_planes(const TfLumaArgs &A, int, const uint8_t **cen, int *cst, uint8_t **dst, int *dstr) {
    *cen = A.cen.base, *cst = A.cen.stride, *dst = A.dst.base, *dstr = A.dst.stride;
}
__device__ __forceinline__ void tff_planes(const TfChromaArgs &A, int pl, const uint8_t **cen, int *cst, uint8_t **dst,
                                           int *dstr) {
    *cen = pl ? A.cen[1].base : A.cen[0].base, *cst = pl ? A.cen[1].stride : A.cen[0].stride;
    *dst = pl ? A.dst[1].base : A.dst[0].base, *dstr = pl ? A.dst[1].stride : A.dst[0].stride;
}

// The normalisation, one workgroup per SB. A thread has N = 16 (chroma: 8) samples of one row of one
// plane of the SB, all in one 16x16 (8x8) quarter, so with one weight per reference: luma row tid / 4,
// columns 16 (tid % 4) .. + 15; chroma plane tid / 128, row (tid / 4) % 32, columns 8 (tid % 4) .. + 7.
// A unit's tile holds the workgroup's samples in thread order and 256 / N weights a plane. The only
// centre samples a thread reads are its own N.
// PIC: into the result picture. Only samples x < W, y < H of the aligned plane are stored (W is a
// multiple of 8, W/2 of 4: a thread's samples are all inside, the first half inside, or all outside);
// the margins and what lies beyond the true size are the padding kernels' to write afterwards. A.dst
// may be A.cen (the centre picture replaced in place): a thread reads from the centre plane its own
// samples alone, before it stores them or the first half of them, and the samples nobody stores are
// nobody's input either, so no thread reads what another writes. The prediction kernels, which read
// the centre widely (k_tff_pred_uv its luma too, hence both predictions before either normalisation),
// have finished by stream order. Nothing here reads level 0 at 10 bit.
template <typename T, int UV, bool PIC, typename Args>
__device__ __forceinline__ void tff_norm(const Args &A) {
    constexpr int BPP = (int)sizeof(T), N = 16 >> UV, S = 64 >> UV; // samples a thread, a side of the SB's tile
    constexpr bool MASK = BPP == 2; // a mean of bytes, exactly divided, is a byte: packed as it is
    const int tid      = threadIdx.x;
    const uint32_t b64 = blockIdx.x;
    const uint32_t sby = b64 / A.pic_w_b64, sbx = b64 - sby * A.pic_w_b64;
    const int pl = UV ? tid >> 7 : 0, row = (tid >> 2) & (S - 1), g = tid & 3;
    const int x = (int)sbx * S + g * N, y = (int)sby * S + row, W = A.W >> UV, H = A.H >> UV;
    if (PIC && (x >= W || y >= H))
        return;
    const uint8_t *cen;
    uint8_t *dst;
    int cst, dstr;
    tff_planes(A, pl, &cen, &cst, &dst, &dstr);
    const int wi = pl * 16 + tf_wi(g, row / N);
    uint32_t acc[N], pre[N], cnt = 1000; // svt_aom_apply_filtering_central[_highbd]_c
    tf_load<T, N>(cen + (ptrdiff_t)y * cst + (ptrdiff_t)x * BPP, acc);
#pragma unroll
    for (int k = 0; k < N; k++) acc[k] *= 1000u;
    for (uint32_t r = 0; r < A.n; r++) {
        const size_t unit = (size_t)r * A.sbs + b64;
        const uint32_t w  = A.wgt[unit * (256 / N) + wi];
        tf_load<T, N>(A.tile + (unit * 256 + tid) * (N * BPP), pre);
        cnt += w;
#pragma unroll
        for (int k = 0; k < N; k++) acc[k] += w * pre[k];
    }
    tf_norm<N>(acc, cnt);
    if constexpr (!PIC) { // plane pl of whole SBs
        uint8_t *op = A.plane + ((size_t)pl * A.sbs * (S * S) + (size_t)y * ((size_t)A.pic_w_b64 * S) + x) * BPP;
        tf_store<T, N, MASK>(op, acc, false);
    } else {
        const bool half = x + N > W;
        tf_store<T, N, MASK>(dst + (ptrdiff_t)y * dstr + (ptrdiff_t)x * BPP, acc, half); // aligned as the centre's load
        if constexpr (BPP == 2 && !UV) { // the result picture's level 0: the MSB plane
#pragma unroll
            for (int k = 0; k < N; k++) acc[k] >>= 2;
            tf_store<uint8_t, N>(A.dst8.base + (ptrdiff_t)y * A.dst8.stride + x, acc, half);
        }
    }
}

template <typename T, bool PIC>
__global__ void __launch_bounds__(256) k_tff_norm(const TfLumaArgs A) {
    tff_norm<T, 0, PIC>(A);
}
template <typename T, bool PIC>
__global__ void __launch_bounds__(256) k_tff_norm_uv(const TfChromaArgs A) {
    tff_norm<T, 1, PIC>(A);
}

// One window's stage: the predictions and weights of its n references in one launch per plane kind,
// and the normalisations, dense (PIC false: into Y.plane, U->plane) or into the result picture (Y.dst,
// Y.dst8 at 10 bit, U->dst). U NULL: luma alone. Into the result picture both predictions run before
// either normalisation: in place (dst is cen) k_tff_pred_uv still reads the centre's unfiltered luma for
// the luma window errors. The dense planes alias nothing, so there each normalisation follows its
// prediction, whose tiles it then finds in the cache.
template <typename T, bool PIC>
static void tff_launch(const TfLumaArgs &Y, const TfChromaArgs *U, hipStream_t s) {
    const dim3 units(Y.n * Y.sbs), sbs(Y.sbs), wg(256);
    hipLaunchKernelGGL(k_tff_pred<T>, units, wg, 0, s, Y);
    if (!PIC)
        hipLaunchKernelGGL((k_tff_norm<T, PIC>), sbs, wg, 0, s, Y);
    if (U)
        hipLaunchKernelGGL(k_tff_pred_uv<T>, units, wg, 0, s, *U);
    if (PIC)
        hipLaunchKernelGGL((k_tff_norm<T, PIC>), sbs, wg, 0, s, Y);
    if (U)
        hipLaunchKernelGGL((k_tff_norm_uv<T, PIC>), sbs, wg, 0, s, *U);
}

// The planes are checked here, before the launch: every size is the window's, so the kernels' reads
// and stores stay where the file's head says they do.
extern "C" hipError_t svtme_launch_tf_stage(const TfLumaArgs *Y, const TfChromaArgs *U, int hbd, int pic, hipStream_t s) {
    auto sized = [](const DevPlane &p, int32_t w, int32_t h) { return p.width == w && p.height == h; };
    const int32_t W = Y->W, H = Y->H;
    if (!Y->n || Y->n > SVTME_MAX_BATCH_JOBS || W <= 0 || H <= 0 || Y->pic_w_b64 != (uint32_t)(W + 63) / 64 ||
        Y->sbs != Y->pic_w_b64 * ((uint32_t)(H + 63) / 64))
        return hipErrorInvalidValue;
    if (!sized(Y->cen, W, H) || (pic && !sized(Y->dst, W, H)) || (pic && hbd && !sized(Y->dst8, W, H)))
        return hipErrorInvalidValue;
    for (uint32_t k = 0; k < Y->n; k++)
        if (!sized(Y->ref[k], W, H))
            return hipErrorInvalidValue;
    if (U) {
        if (U->n != Y->n || U->sbs != Y->sbs || U->pic_w_b64 != Y->pic_w_b64 || U->W != W || U->H != H || !sized(U->cen_y, W, H))
            return hipErrorInvalidValue;
        for (int p = 0; p < 2; p++)
            if (!sized(U->cen[p], W / 2, H / 2) || (pic && !sized(U->dst[p], W / 2, H / 2)))
                return hipErrorInvalidValue;
    }
    if (hbd)
        pic ? tff_launch<uint16_t, true>(*Y, U, s) : tff_launch<uint16_t, false>(*Y, U, s);
    else
        pic ? tff_launch<uint8_t, true>(*Y, U, s) : tff_launch<uint8_t, false>(*Y, U, s);
    return hipGetLastError();
}

template <typename T>
static hipError_t tff_prime() {
    const void *k[] = {(const void *)k_tff_pred<T>,
                       (const void *)k_tff_pred_uv<T>,
                       (const void *)k_tff_norm<T, false>,
                       (const void *)k_tff_norm<T, true>,
                       (const void *)k_tff_norm_uv<T, false>,
                       (const void *)k_tff_norm_uv<T, true>};
    hipFuncAttributes a;
    hipError_t e = hipSuccess;
    for (const void *f : k)
        if (e == hipSuccess)
            e = hipFuncGetAttributes(&a, f);
    return e;
}

extern "C" hipError_t svtme_prime_tff(void) { // (see svtme_prime_pyramid)
    const hipError_t e = tff_prime<uint8_t>();
    return e != hipSuccess ? e : tff_prime<uint16_t>();
}
