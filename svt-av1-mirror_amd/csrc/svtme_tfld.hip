// svtme_tfld.hip — low-delay temporal filtering (svtme_tf_filter_ld, svtme_tf_window_ld):
// produce_temporally_filtered_pic_ld (temporal_filtering.c:3404-3816) in one fused kernel,
// 8 and 10 bit, luma alone or with 4:2:0 chroma.
//
// The low-delay path searches nothing: the prediction of every 64x64 block is the co-located
// block of the reference picture (tf_64x64_inter_prediction at MV (0, 0): svt_aom_inter_prediction's
// copy case, read from the padded plane where the SB overhangs the picture). So all a 32x32 luma
// block needs is that block of the centre and of each reference, and no accumulator, prediction
// or weight has to live in memory.
//
// Mapping: one workgroup of four wavefronts per SB, wavefront wid = the 32x32 luma block
// col + 2 row (the index of tf_32x32_block_error and of var32). A lane holds 16 luma samples of
// one row (row lane >> 1, columns 16 (lane & 1) .. + 15) and, with chroma, 4 samples of one row
// of the block's 16x16 Cb and Cr (row lane >> 2, columns 4 (lane & 3) .. + 3). Its accumulators
// stay in registers; the counts are wave-uniform. Per reference: load, the lane's sum and sum of
// squares of the luma differences over the rows sub_sampling_shift keeps, two wave reductions
// (DPP, no LDS), the three weights as uniform values, accumulate. Each sample of each picture is
// read once. No LDS, no scratch.
//
// Semantics restated (reference line beside each):
//  * svt_aom_apply_filtering_central[_highbd]_c (:349-421): accum 1000 x centre, count 1000.
//  * the 32x32 errors (:3725-3767): svt_aom_variance32x32_c, with sub_sampling_shift 1
//    svt_aom_variance32x16_c on every second row and << 1 (variance.c:300-306:
//    sse - (sum * sum) / N in 32 bits); at 10 bit svt_aom_highbd_10_variance32x32_c / 32x16_c
//    (svt_psnr.c:139-177: SSE rounded by 4 bits, sum by 2, the difference clamped at 0).
//  * svt_av1_apply_zz_based_temporal_filter_planewise_medium[_hbd]_partial_c (:818-864,
//    :920-967) with split flags 0: e = var32 >> 2 (10 bit: >> 6), sd = min((e << 2) /
//    max(decay >> 10, 1), 112), w = (exp_tab[sd] * 1000) >> 17, for each plane with its own
//    decay factor and the LUMA variance; count += w, accum += w * pred.
//  * svt_aom_get_final_filtered_pixels_c (:2607-): (accum + (count >> 1)) / count.
//
// Reads stay inside the planes: an SB overhangs the 8-aligned picture by 56 samples at the most
// (margins: 88 right, 72 below, svtme_plane_geometry / svtme_hbd_geometry), a chroma SB by 28
// (48 right, 40 below). Interior rows start 16-byte aligned in every plane and a lane's first
// sample is a multiple of 16 (chroma: 4) samples into the row, so every load is aligned to its
// width. Stores cover x < W, y < H of the aligned picture only (W a multiple of 8: a lane's 16
// luma samples are all inside, the first 8 inside, or all outside; its 4 chroma samples all inside
// or all outside). In place (dst == cen) is safe by construction: a wavefront reads from the
// centre only the block it writes, before it writes it, and the part of an edge SB beyond W, H is
// read and never written here (the padding kernels rewrite it afterwards on the same stream).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svtme_launch.h"
#include "svtme_tf_common.h"

using namespace svtme;

template <typename T, bool CHROMA>
__global__ void __launch_bounds__(256) k_tfld(const TfldArgs A) {
    constexpr int BPP = (int)sizeof(T);
    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
    const uint32_t b64 = blockIdx.x;
    const uint32_t sby = b64 / A.pic_w_b64, sbx = b64 - sby * A.pic_w_b64;
    const int ss = (int)A.ss;
    // luma: this lane's 16 samples
    const int x = (int)sbx * 64 + (wid & 1) * 32 + (lane & 1) * 16, y = (int)sby * 64 + (wid >> 1) * 32 + (lane >> 1);
    const ptrdiff_t yo = (ptrdiff_t)y * A.y_stride + (ptrdiff_t)x * BPP;
    const bool kept    = ((lane >> 1) & ss) == 0;
    // chroma: this lane's 4 samples of Cb and of Cr
    const int cx = (int)sbx * 32 + (wid & 1) * 16 + (lane & 3) * 4, cy = (int)sby * 32 + (wid >> 1) * 16 + (lane >> 2);
    const ptrdiff_t co = (ptrdiff_t)cy * A.c_stride + (ptrdiff_t)cx * BPP;

    uint32_t cen[16], acc[16], cnt[3] = {1000u, 1000u, 1000u}; // svt_aom_apply_filtering_central[_highbd]_c
    uint32_t cacc[2][4];
    tf_load<T, 16>(A.cen_y + yo, cen);
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = 1000u * cen[k];
    if constexpr (CHROMA) {
#pragma unroll
        for (int p = 0; p < 2; p++) {
            tf_load<T, 4>(A.cen_c[p] + co, cacc[p]);
#pragma unroll
            for (int k = 0; k < 4; k++) cacc[p][k] *= 1000u;
        }
    }

    for (uint32_t r = 0; r < A.n; r++) {
        uint32_t pre[16], cpre[2][4];
        tf_load<T, 16>(A.ref_y[r] + yo, pre);
        if constexpr (CHROMA) {
            tf_load<T, 4>(A.ref_c[0][r] + co, cpre[0]);
            tf_load<T, 4>(A.ref_c[1][r] + co, cpre[1]);
        }
        int sum      = 0;
        uint32_t sse = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int d = (int)pre[k] - (int)cen[k];
            sum += d;
            sse += (uint32_t)(d * d);
        }
        const int sk        = (int)wave_sum_u32(kept ? (uint32_t)sum : 0u);
        const uint32_t ssek = wave_sum_u32(kept ? sse : 0u);
        const uint32_t var = tf_var32<T>(sk, ssek, ss);
        const uint32_t e   = var >> (BPP == 1 ? 2 : 6); // (:831, :933)
        if (A.var32 && lane == 0)
            A.var32[((size_t)r * A.sbs + b64) * 4 + wid] = var;
        uint32_t w[3];
#pragma unroll
        for (int p = 0; p < (CHROMA ? 3 : 1); p++) {
            const uint32_t dd = (A.decay[p] >> 10) ? (A.decay[p] >> 10) : 1u;
            uint32_t sd       = (e << 2) / dd;
            sd                = sd < 112u ? sd : 112u;
            w[p]              = (uint32_t)(c_tf_exp.v[sd] * 1000) >> 17;
            cnt[p] += w[p];
        }
#pragma unroll
        for (int k = 0; k < 16; k++) acc[k] += w[0] * pre[k];
        if constexpr (CHROMA) {
#pragma unroll
            for (int p = 0; p < 2; p++)
#pragma unroll
                for (int k = 0; k < 4; k++) cacc[p][k] += w[1 + p] * cpre[p][k];
        }
    }

    if (x < A.W && y < A.H) {
        tf_norm<16>(acc, cnt[0]);
        const bool half = x + 16 > A.W;
        tf_store<T, 16>(A.dst_y.base + (ptrdiff_t)y * A.dst_y.stride + (ptrdiff_t)x * BPP, acc, half);
        if constexpr (BPP == 2) {
            if (A.dst8.base) { // the result picture's level 0: the MSB plane
#pragma unroll
                for (int k = 0; k < 16; k++) acc[k] >>= 2;
                tf_store<uint8_t, 16>(A.dst8.base + (ptrdiff_t)y * A.dst8.stride + x, acc, half);
            }
        }
    }
    if constexpr (CHROMA) {
        if (cx < (A.W >> 1) && cy < (A.H >> 1)) {
#pragma unroll
            for (int p = 0; p < 2; p++)
                if (A.dst_c[p].base) {
                    tf_norm<4>(cacc[p], cnt[1 + p]);
                    tf_store<T, 4>(A.dst_c[p].base + (ptrdiff_t)cy * A.dst_c[p].stride + (ptrdiff_t)cx * BPP, cacc[p],
                                     false);
                }
        }
    }
}

// The planes of A are checked here, before the launch: every size is the window's, so the kernel's
// reads and stores stay where the file's head says they do.
extern "C" hipError_t svtme_launch_tfld(const TfldArgs *A, int hbd, int chroma, hipStream_t s) {
    if (!A->n || A->n > SVTME_MAX_BATCH_JOBS || A->W <= 0 || A->H <= 0 || (A->W & 7) || (A->H & 7) || A->ss > 1)
        return hipErrorInvalidValue;
    if (A->pic_w_b64 != (uint32_t)(A->W + 63) / 64 || A->sbs != A->pic_w_b64 * ((uint32_t)(A->H + 63) / 64))
        return hipErrorInvalidValue;
    if (!A->cen_y || !A->dst_y.base || A->dst_y.width != A->W || A->dst_y.height != A->H)
        return hipErrorInvalidValue;
    if (A->dst8.base && (!hbd || A->dst8.width != A->W || A->dst8.height != A->H))
        return hipErrorInvalidValue;
    for (uint32_t k = 0; k < A->n; k++)
        if (!A->ref_y[k] || (chroma && (!A->ref_c[0][k] || !A->ref_c[1][k])))
            return hipErrorInvalidValue;
    for (int p = 0; chroma && p < 2; p++)
        if (!A->cen_c[p] || (A->dst_c[p].base && (A->dst_c[p].width != A->W / 2 || A->dst_c[p].height != A->H / 2)))
            return hipErrorInvalidValue;
    const dim3 grid(A->sbs), block(256);
    if (hbd && chroma)
        hipLaunchKernelGGL((k_tfld<uint16_t, true>), grid, block, 0, s, *A);
    else if (hbd)
        hipLaunchKernelGGL((k_tfld<uint16_t, false>), grid, block, 0, s, *A);
    else if (chroma)
        hipLaunchKernelGGL((k_tfld<uint8_t, true>), grid, block, 0, s, *A);
    else
        hipLaunchKernelGGL((k_tfld<uint8_t, false>), grid, block, 0, s, *A);
    return hipGetLastError();
}

extern "C" hipError_t svtme_prime_tfld(void) { // (see svtme_prime_pyramid)
    hipFuncAttributes a;
    hipError_t e = hipFuncGetAttributes(&a, (const void *)k_tfld<uint8_t, false>);
    if (e == hipSuccess)
        e = hipFuncGetAttributes(&a, (const void *)k_tfld<uint8_t, true>);
    if (e == hipSuccess)
        e = hipFuncGetAttributes(&a, (const void *)k_tfld<uint16_t, false>);
    return e != hipSuccess ? e : hipFuncGetAttributes(&a, (const void *)k_tfld<uint16_t, true>);
}
