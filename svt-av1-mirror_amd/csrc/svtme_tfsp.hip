// svtme_tfsp.hip — temporal filtering's sub-pel refinement as a picture-window
// job (svtme_tf_subpel, include/svtme.h): the stage of temporal_filtering.c:
// 3177-3336 that follows the TF-ME call, up to but not including the first
// tf_64x64_inter_prediction / tf_32x32_inter_prediction. Per (reference, SB)
// the 64x64 block, the four 32x32, the sixteen 16x16 and optionally the
// sixty-four 8x8 blocks are refined from the full-pel winners of the TF-ME
// record: the centre position, then up to 8 half, 8 quarter and 8 eighth-pel
// positions around the running best, each an AV1 interpolation of the block
// (8-tap regular or bilinear, separable) and a variance against the centre
// picture. 8-bit path only.
//
// One 256-thread workgroup per (reference, SB), the whole window in one launch.
// The blocks of one size are searched together, stage by stage (centre, half,
// quarter, eighth): within a stage every (block, candidate position) is one
// work unit, a wavefront takes one unit at a time, and the units of a stage are
// all evaluated before a single lane per block resolves them in the
// reference's order (x offset outer, y offset inner, strict <, the best == 0
// skip, the running-best early exit, diagonals dropped when the stage's mode is
// >= 2). A unit the reference would skip changes nothing when it is ignored at
// the resolve, so evaluating it is harmless; blocks whose best already stops
// the search (0, or under the early-exit threshold: the best never grows) and
// the dropped diagonals are not evaluated at all.
//
// A unit: the wavefront stages the (b + 7) x (b + 7) window of its clamped
// position in its own LDS slice (aligned dwords, v_alignbyte), runs the
// horizontal pass into an int16 LDS plane when both phases are non-zero
// (svt_av1_convolve_2d_sr_c: round_0 = 3, round_1 = 11 and its offsets), then
// the vertical pass / the x-only, y-only or copy case on the rows
// sub_sampling_shift keeps, and reduces sum and sse of the difference to the
// centre block (the SB's 64 x 64 block, staged in LDS once per workgroup) with DPP. Multiply-adds are plain 32-bit (v_mad_i32_i24 /
// v_mad_u32_u24 by the compiler): the pixels are u8 and the taps signed, so
// the signed x signed byte dot product does not apply as it stands, and the
// 2-D pass multiplies 13-bit intermediates. The taps are wave-uniform (SGPRs).
//
// Semantics restated (reference line beside each):
//  * start MVs: the record's winners << 3; the 64x64 start is hme_sc << 3 when
//    tf_early_exit is set (temporal_filtering.c:1866-1869, 1980, 2113, 2232).
//    The record keeps the PUs in Z order, which is tab16x16 / tab8x8 of the
//    raster indices idx_32x32_to_idx_16x16 / _8x8 give: the 16x16 block
//    idx_32x32 * 4 + idx_16x16 starts from record PU 5 + that index, the 8x8
//    block idx_32x32 * 16 + 4 * idx_16x16 + idx_8x8 from PU 21 + that index.
//  * MV clamp: clamp_mv_to_umv_border_sb with mb_to_*_edge from mi_rows /
//    mi_cols of the aligned picture (enc_inter_prediction.c:28-48, 3154-3163);
//    position and phase come from the clamped q4 MV. Only even phases occur.
//  * the four convolve cases (inter_prediction.c:311-418); the taps below are
//    the AV1 specification's sub-pel filter table (regular: Subpel_Filters[0],
//    bilinear: 128 - 8 p, 8 p at taps 3 and 4).
//  * variance: sse - (uint32)((int64)sum * sum / (W * H)) over the kept rows,
//    shifted left by sub_sampling_shift (variance.c:300-306,
//    temporal_filtering.c:1605-1636). The centre position of the reference
//    predicts only the kept rows from a doubled stride; its MV is full-pel
//    (the clamp bounds are whole pixels), so that is a copy of the same rows.
//  * decisions: tf_use_64x64_pred (:2675), the 64-vs-32 test (:3265), the
//    pred_error_32x32_th bypass (:3293), derive_tf_32x32_block_split_flag
//    (:236-285).
//
// Reads stay inside the device full plane (svtme_device.h: left 80, top 72, a
// row of stride >= W + 80 + 88 bytes, 72 rows below; W x H the 8-aligned
// picture). With b the block size and (px, py) its origin, the clamp bounds the
// q4 MV to [-(px * 16) - (b + 4) * 16, (W - b - px) * 16 + (b + 4) * 16 - 16],
// so the block origin x0 = px + (q4 >> 4) lies in [-(b + 4), W + 3] (y alike
// with H). The taps reach 3 left / above and 4 right / below: window bytes lie
// in x in [-(b + 7), W + b + 6], i.e. [-71, W + 70] for b = 64 (rows
// [-71, H + 70], inside the 72 rows of padding). The staging reads aligned
// dwords from (x0 - 3) & ~3 >= -72 up to dword index ceil((b + 7) / 4): bytes
// up to x0 - 3 + 4 * 19 + 3 <= W + 79 < W + 88. The centre block reads
// x in [px, px + 63] with px <= W - 8 and rows up to py + 63 <= H + 55.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svtme_launch.h"
#include "svtme_tf_common.h"

using namespace svtme;

struct TfspArgs {
    DevPlane cen;                       // full plane of the centre picture
    DevPlane ref[SVTME_MAX_BATCH_JOBS]; // full planes of the references
    const svtme_ref_record *rec;        // [n][sbs] slot 0 of each TF-ME job
    svtme_tf_subpel_sb *out;            // [n][sbs]
    svtme_tf_subpel_controls ctl;
    uint32_t sbs, pic_w_b64;
    int32_t W, H; // the 8-aligned picture
};

#define TF_WP 19    // dwords per staged window row (18 + 1, odd)
#define TF_WROWS 71 // 64 + 7
#define TF_UNSET SVTME_TFSP_UNSET_ERROR

// AV1 specification, Subpel_Filters[0] (EIGHTTAP_REGULAR), phases 0..15
__constant__ int16_t c_tf_regular[16][8] = {
    {0, 0, 0, 128, 0, 0, 0, 0},
    {0, 2, -6, 126, 8, -2, 0, 0},     {0, 2, -10, 122, 18, -4, 0, 0},  {0, 2, -12, 116, 28, -8, 2, 0},
    {0, 2, -14, 110, 38, -10, 2, 0},  {0, 2, -14, 102, 48, -12, 2, 0}, {0, 2, -16, 94, 58, -12, 2, 0},
    {0, 2, -14, 84, 66, -12, 2, 0},   {0, 2, -14, 76, 76, -14, 2, 0},  {0, 2, -12, 66, 84, -14, 2, 0},
    {0, 2, -12, 58, 94, -16, 2, 0},   {0, 2, -12, 48, 102, -14, 2, 0}, {0, 2, -10, 38, 110, -14, 2, 0},
    {0, 2, -8, 28, 116, -12, 2, 0},   {0, 0, -4, 18, 122, -10, 2, 0},  {0, 0, -2, 8, 126, -6, 2, 0}};

typedef __attribute__((address_space(1))) const uint32_t g_u32; // global, not flat, loads

// the taps of one phase in SGPRs: t[1..6] regular, t[3..4] bilinear
__device__ __forceinline__ void tf_taps(bool bil, int phase, int t[8]) {
#pragma unroll
    for (int k = 0; k < 8; k++) t[k] = bil ? 0 : UNI((int)c_tf_regular[phase][k]);
    if (bil) {
        t[3] = 128 - 8 * phase;
        t[4] = 8 * phase;
    }
}

// taps along a row of bytes (p at tap 0)
__device__ __forceinline__ int tf_hsum(const uint8_t *p, const int t[8], bool bil) {
    if (bil)
        return t[3] * p[3] + t[4] * p[4];
    return t[1] * p[1] + t[2] * p[2] + t[3] * p[3] + t[4] * p[4] + t[5] * p[5] + t[6] * p[6];
}

__device__ __forceinline__ int tf_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// One unit on one wavefront: the variance (<< shift) of the b x b block at (px, py) of the centre
// picture against the reference block the 1/8-pel MV points to. `on` is wave-uniform; every
// wavefront of the workgroup calls this the same number of times (workgroup barriers inside).
// `cen` is the SB's 64 x 64 centre block in LDS, (px, py) = SB origin + (bx, by).
__device__ uint32_t tf_eval(const TfspArgs &A, const DevPlane &R, uint32_t *win, int16_t *im, const uint8_t *cen,
                            int lane, bool on, int b, int px, int py, int bx, int by, int mvx, int mvy, bool bil) {
    const int ss = A.ctl.sub_sampling_shift;
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
        const int x0 = px + (qx >> 4), y0 = py + (qy >> 4);
        // the window: byte c of staged row r is plane sample (x0 - 3 + c, y0 - 3 + r)
        const int wx = x0 - 3, shb = wx & 3, ndw = (b + 10) >> 2, rows = b + 7;
        const uint8_t *wp = uni_ptr(R.base + (ptrdiff_t)(y0 - 3) * R.stride + (wx - shb));
        const int rst     = UNI(R.stride);
        const uint32_t m  = magic_u32((uint32_t)ndw);
#pragma unroll 4
        for (int i = lane; i < rows * ndw; i += 64) {
            const int row = mdiv(i, m), j = i - row * ndw;
            const g_u32 *p = (const g_u32 *)(uintptr_t)(wp + (ptrdiff_t)row * rst) + j;
            win[row * TF_WP + j] = __builtin_amdgcn_alignbyte(p[1], p[0], (uint32_t)shb);
        }
    }
    __syncthreads();
    const uint8_t *wb = (const uint8_t *)win;
    const int col = lane & (b - 1), rsub = b == 64 ? 0 : lane / b, rpi = 64 / b;
    int tx[8], ty[8];
    if (on) {
        tf_taps(bil, fx, tx);
        tf_taps(bil, fy, ty);
        if (fx && fy) // horizontal pass of svt_av1_convolve_2d_sr_c: bd 8, round_0 3
#pragma unroll 4
            for (int r = rsub; r < b + 7; r += rpi)
                im[r * 64 + col] = (int16_t)(((1 << 14) + tf_hsum(wb + r * (TF_WP * 4) + col, tx, bil) + 4) >> 3);
    }
    __syncthreads();
    uint32_t dist = 0;
    if (on) {
        int sum = 0;
        uint32_t sse = 0;
        const uint8_t *cp = cen + by * 64 + bx + col;
#pragma unroll 4
        for (int yi = rsub; yi < (b >> ss); yi += rpi) {
            const int y = yi << ss;
            int v;
            if (fx && fy) { // vertical pass: offset_bits 19, round_1 11, bits 0
                int s = 1 << 19;
                if (bil)
                    s += ty[3] * im[(y + 3) * 64 + col] + ty[4] * im[(y + 4) * 64 + col];
                else
#pragma unroll
                    for (int k = 1; k < 7; k++) s += ty[k] * im[(y + k) * 64 + col];
                v = tf_clip8((int16_t)(((s + 1024) >> 11) - ((1 << 8) + (1 << 7))));
            } else if (fx) { // svt_av1_convolve_x_sr_c: round_0 3, then FILTER_BITS - round_0
                const int s = (tf_hsum(wb + (y + 3) * (TF_WP * 4) + col, tx, bil) + 4) >> 3;
                v           = tf_clip8((s + 8) >> 4);
            } else if (fy) { // svt_av1_convolve_y_sr_c: FILTER_BITS
                const uint8_t *p = wb + y * (TF_WP * 4) + col + 3;
                int s            = 0;
                if (bil)
                    s = ty[3] * p[3 * TF_WP * 4] + ty[4] * p[4 * TF_WP * 4];
                else
#pragma unroll
                    for (int k = 1; k < 7; k++) s += ty[k] * p[k * TF_WP * 4];
                v = tf_clip8((s + 64) >> 7);
            } else {
                v = wb[(y + 3) * (TF_WP * 4) + col + 3];
            }
            const int d = v - (int)cp[y * 64];
            sum += d;
            sse += (uint32_t)(d * d);
        }
        sum = (int)wave_sum_u32((uint32_t)sum);
        sse = wave_sum_u32(sse);
        // svt_aom_variance{W}x{H}_c (variance.c:300-306) on the kept rows, << shift
        dist = (sse - (uint32_t)(((int64_t)sum * sum) / (b * (b >> ss)))) << ss;
    }
    return dist;
}

__global__ void __launch_bounds__(256) k_tfsp(const TfspArgs A) {
    __shared__ uint32_t s_win[4][TF_WROWS * TF_WP];
    __shared__ int16_t s_im[4][TF_WROWS * 64];
    __shared__ uint4 s_cen[64 * 4]; // the SB's 64 x 64 block of the centre picture
    __shared__ int16_t s_mvx[85], s_mvy[85]; // running best per block, 1/8 pel
    __shared__ uint32_t s_err[85];
    __shared__ int16_t s_cx[64], s_cy[64]; // the stage's centre MV per block of the level
    __shared__ uint32_t s_cd[64 * 8];      // the stage's candidate distortions
    __shared__ uint8_t s_act[64];          // block of the level is searched / still refines in this stage
    __shared__ uint8_t s_f32[4], s_f16[16], s_skip32[4];
    __shared__ int s_branch;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t u   = UNI(xcd_remap(blockIdx.x, gridDim.x));
    const uint32_t ri  = UNI(u / A.sbs), b64 = u - ri * A.sbs;
    const uint32_t sby = UNI(b64 / A.pic_w_b64), sbx = b64 - sby * A.pic_w_b64;
    DevPlane R = A.ref[0];
#pragma unroll
    for (int k = 1; k < SVTME_MAX_BATCH_JOBS; k++) // constant-index argument reads
        if (ri == (uint32_t)k)
            R = A.ref[k];
    const svtme_ref_record *rec = uni_ptr(A.rec + (size_t)ri * A.sbs + b64);
    const int sb_x = (int)sbx * 64, sb_y = (int)sby * 64;
    const uint32_t eth = A.ctl.subpel_early_exit_th;
    // the TF-ME early exit leaves tf_use_pred_64x64_only_th at ~0 (motion_estimation.c:3111), as a control of 255 does
    const bool exit_me = UNI(rec->tf_early_exit) != 0 || A.ctl.use_pred_64x64_only_th == 255;

    // the centre block: row tid / 4, 16 bytes at column 16 (tid % 4) (16-byte aligned: sb_x is a multiple of 64)
    s_cen[tid] = *(const uint4 *)(A.cen.base + (ptrdiff_t)(sb_y + (tid >> 2)) * A.cen.stride + sb_x + (tid & 3) * 16);
    // start MVs (the winners << 3, int16 as the reference's fields) and INT_MAX errors
    if (tid < 85) {
        const uint32_t mv = rec->best_mv[tid];
        int16_t x = (int16_t)((int16_t)(mv & 0xFFFF) << 3), y = (int16_t)((int16_t)(mv >> 16) << 3);
        if (tid == 0 && exit_me)
            x = (int16_t)(rec->hme_sc_x << 3), y = (int16_t)(rec->hme_sc_y << 3);
        s_mvx[tid] = x, s_mvy[tid] = y;
        s_err[tid] = TF_UNSET;
    }
    if (tid < 16)
        s_f16[tid] = 0;
    if (tid < 4)
        s_f32[tid] = 0, s_skip32[tid] = 0;
    if (tid == 0) {
        // the branch known before any search (temporal_filtering.c:3177-3179, tf_use_64x64_pred :2675)
        int only64 = 0;
        const uint32_t th = exit_me ? 255u : A.ctl.use_pred_64x64_only_th;
        if (th) {
            if (th == 255u)
                only64 = 1;
            else {
                const uint32_t d32 = rec->best_sad[1] + rec->best_sad[2] + rec->best_sad[3] + rec->best_sad[4];
                const int64_t a = rec->best_sad[0] > 1 ? rec->best_sad[0] : 1, c = d32 > 1 ? d32 : 1;
                only64          = ((a - c) * 100) / c < (int64_t)th;
            }
        }
        s_branch = only64 ? SVTME_TFSP_64_ONLY : -1;
    }
    __syncthreads();

    for (int lv = 0; lv < 4; lv++) {
        const int b = 64 >> lv, nblk = 1 << (2 * lv);
        const int off = lv == 0 ? 0 : lv == 1 ? SVTME_TFSP_OFF_32 : lv == 2 ? SVTME_TFSP_OFF_16 : SVTME_TFSP_OFF_8;
        const bool bil = lv < 2 && A.ctl.use_2tap; // 16x16 and 8x8: always the regular filter (:2022, 2142)
        if (lv == 1 && s_branch == SVTME_TFSP_64_ONLY)
            break;
        if (lv == 2 && s_branch != SVTME_TFSP_32)
            break;
        if (lv == 3 && !A.ctl.enable_8x8_pred)
            break;
        for (int st = 0; st < 4; st++) {
            const int md = st == 1 ? A.ctl.half_pel_mode : st == 2 ? A.ctl.quarter_pel_mode : A.ctl.eight_pel_mode;
            if (st && !md)
                continue;
            const int step = 8 >> st; // 4, 2, 1 for the half, quarter and eighth-pel stages
            if (tid < nblk) {
                const uint32_t e = s_err[off + tid];
                bool act         = lv < 2 || !s_skip32[tid >> (2 * (lv - 1))];
                // every later position is skipped once the best is 0 or under the early-exit threshold
                if (st && (e == 0 || (eth && e < (uint32_t)(b * b) * eth)))
                    act = false;
                s_act[tid] = act;
                s_cx[tid] = s_mvx[off + tid], s_cy[tid] = s_mvy[off + tid];
            }
            __syncthreads();
            // units: st 0 one per block, else 8 per block in the reference's order (x outer, y inner)
            const int nc = st ? 8 : 1, units = nblk * nc;
            for (int u0 = 0; u0 < units; u0 += 4) {
                const int un = u0 + wid;
                bool on      = un < units;
                int k = 0, c = 0, xd = 0, yd = 0;
                if (on) {
                    k = st ? un >> 3 : un, c = un & 7;
                    if (st) {
                        const int cc = c < 4 ? c : c + 1; // 3 x 3 grid without its centre
                        xd = (cc / 3 - 1) * step, yd = (cc % 3 - 1) * step;
                    }
                    on = s_act[k] && !(st && md >= 2 && xd && yd);
                }
                int bx, by;
                tf_unit_origin(lv, k, 32, &bx, &by);
                const uint32_t d = tf_eval(A, R, s_win[wid], s_im[wid], (const uint8_t *)s_cen, lane, on, b, sb_x + bx,
                                           sb_y + by, bx, by, (int16_t)(s_cx[k] + xd), (int16_t)(s_cy[k] + yd), bil);
                if (on && lane == 0)
                    s_cd[st ? un : un * 8] = d;
            }
            __syncthreads();
            // svt_check_position in the reference's order (temporal_filtering.c:1560-1662)
            if (tid < nblk && s_act[tid]) {
                uint32_t best = s_err[off + tid];
                int16_t bmx = s_mvx[off + tid], bmy = s_mvy[off + tid];
                for (int c = 0; c < nc; c++) {
                    int xd = 0, yd = 0;
                    if (st) {
                        const int cc = c < 4 ? c : c + 1;
                        xd = (cc / 3 - 1) * step, yd = (cc % 3 - 1) * step;
                        if (md >= 2 && xd && yd)
                            continue;
                    }
                    if (best == 0)
                        continue;
                    if (eth && best < (uint32_t)(b * b) * eth)
                        continue;
                    const uint32_t d = s_cd[tid * 8 + c];
                    if (d < best)
                        best = d, bmx = (int16_t)(s_cx[tid] + xd), bmy = (int16_t)(s_cy[tid] + yd);
                }
                s_err[off + tid] = best, s_mvx[off + tid] = bmx, s_mvy[off + tid] = bmy;
            }
            __syncthreads();
        }
        if (lv == 1 && tid == 0) {
            // 64x64 against the four 32x32 (temporal_filtering.c:3260-3266), then the bypass (:3293)
            const uint64_t e64 = s_err[0];
            const uint64_t s32 = (uint64_t)s_err[1] + s_err[2] + s_err[3] + s_err[4];
            if (e64 * 14 < s32 * 16 && e64 < (1u << 18))
                s_branch = SVTME_TFSP_64_CHOSEN;
            else {
                s_branch = SVTME_TFSP_32;
                for (int i = 0; i < 4; i++) s_skip32[i] = (uint64_t)s_err[1 + i] < A.ctl.pred_error_32x32_th;
            }
        }
        __syncthreads();
    }

    // derive_tf_32x32_block_split_flag (temporal_filtering.c:236-285), int arithmetic
    if (tid < 4 && s_branch == SVTME_TFSP_32 && !s_skip32[tid]) {
        const int block_error = (int)s_err[SVTME_TFSP_OFF_32 + tid];
        int sum = 0;
        for (int i = 0; i < 4; i++) {
            int e = (int)s_err[SVTME_TFSP_OFF_16 + tid * 4 + i];
            if (A.ctl.enable_8x8_pred) {
                int e8 = 0;
                for (int j = 0; j < 4; j++) e8 += (int)s_err[SVTME_TFSP_OFF_8 + tid * 16 + 4 * i + j];
                if (!(e * 8 < e8 * 16)) {
                    s_f16[tid * 4 + i]                      = 1;
                    s_err[SVTME_TFSP_OFF_16 + tid * 4 + i] = (uint32_t)e8;
                    e                                       = e8;
                }
            }
            sum += e;
        }
        s_f32[tid] = !(block_error * 14 < sum * 16);
    }
    __syncthreads();

    // the result, whole dwords by vector stores; unwritten blocks keep MV 0 and INT_MAX
    uint32_t *o = (uint32_t *)(A.out + (size_t)ri * A.sbs + b64);
    const int br = s_branch;
    if (tid < 85) {
        const int lv = tid < 1 ? 0 : tid < 5 ? 1 : tid < 21 ? 2 : 3;
        uint32_t e   = s_err[tid];
        int16_t x = s_mvx[tid], y = s_mvy[tid];
        if (lv == 1 && br != SVTME_TFSP_32) // convert_64x64_info_to_32x32_info (:2696-2706)
            x = s_mvx[0], y = s_mvy[0], e = TF_UNSET;
        if (e == TF_UNSET && !(lv == 1 && br != SVTME_TFSP_32))
            x = 0, y = 0; // never searched on this branch
        o[tid]      = (uint32_t)(uint16_t)x | ((uint32_t)(uint16_t)y << 16);
        o[85 + tid] = e;
    } else if (tid < 90) {
        const int i = tid - 85; // 170 + i: flags of 32x32 block i (i < 4), then branch
        if (i == 0)
            o[170] = (uint32_t)s_f32[0] | ((uint32_t)s_f32[1] << 8) | ((uint32_t)s_f32[2] << 16) | ((uint32_t)s_f32[3] << 24);
        else
            o[170 + i] = (uint32_t)s_f16[4 * (i - 1)] | ((uint32_t)s_f16[4 * (i - 1) + 1] << 8) |
                         ((uint32_t)s_f16[4 * (i - 1) + 2] << 16) | ((uint32_t)s_f16[4 * (i - 1) + 3] << 24);
    } else if (tid == 90) {
        o[175] = (uint32_t)br;
    }
}

// n references of one window in one launch
extern "C" hipError_t svtme_launch_tfsp(const DevPlane *cen, const DevPlane *ref, uint32_t n, uint32_t width,
                                        uint32_t height, const svtme_tf_subpel_controls *ctl,
                                        const svtme_ref_record *d_rec, svtme_tf_subpel_sb *d_out, hipStream_t s) {
    if (!n || n > SVTME_MAX_BATCH_JOBS)
        return hipErrorInvalidValue;
    TfspArgs A{};
    A.cen = *cen;
    for (uint32_t k = 0; k < SVTME_MAX_BATCH_JOBS; k++) A.ref[k] = ref[k < n ? k : 0];
    A.rec       = d_rec;
    A.out       = d_out;
    A.ctl       = *ctl;
    A.pic_w_b64 = (width + 63) / 64;
    A.sbs       = A.pic_w_b64 * ((height + 63) / 64);
    A.W         = (int32_t)width;
    A.H         = (int32_t)height;
    hipLaunchKernelGGL(k_tfsp, dim3(n * A.sbs), dim3(256), 0, s, A);
    return hipGetLastError();
}

extern "C" hipError_t svtme_prime_tfsp(void) { // (see svtme_prime_pyramid)
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void *)k_tfsp);
}
