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
#include "svtme_me_common.h"

using namespace svtme;

// floor(exp(-i / 16) * 2^16), computed as svtme_tff.hip computes it
struct TfldExpTab {
    int32_t v[113];
};
constexpr TfldExpTab tfld_make_exp() {
    TfldExpTab t{};
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
__constant__ TfldExpTab c_tfld_exp = tfld_make_exp();

// N samples of type T at p (aligned to N * sizeof(T) bytes: 4, 8, 16 or 32), one per element of v
template <typename T, int N>
__device__ __forceinline__ void tfld_load(const uint8_t *p, uint32_t v[N]) {
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

// the first `count` (N or N / 2) of N samples of type T to p, packed; shift: >> 2 into bytes (level 0 of a 10-bit result)
template <typename T, int N>
__device__ __forceinline__ void tfld_store(uint8_t *p, const uint32_t v[N], bool half) {
    constexpr int DW = N * (int)sizeof(T) / 4;
    uint32_t w[DW];
#pragma unroll
    for (int i = 0; i < DW; i++) w[i] = 0;
#pragma unroll
    for (int k = 0; k < N; k++)
        if constexpr (sizeof(T) == 1)
            w[k >> 2] |= (v[k] & 0xFFu) << (8 * (k & 3));
        else
            w[k >> 1] |= (v[k] & 0xFFFFu) << (16 * (k & 1));
    if constexpr (DW == 1)
        *(uint32_t *)p = w[0];
    else if constexpr (DW == 2)
        *(uint2 *)p = make_uint2(w[0], w[1]);
    else if constexpr (DW == 4) {
        if (half)
            *(uint2 *)p = make_uint2(w[0], w[1]);
        else
            *(uint4 *)p = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        ((uint4 *)p)[0] = make_uint4(w[0], w[1], w[2], w[3]);
        if (!half)
            ((uint4 *)p)[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
}

// (accum + (count >> 1)) / count for N accumulators: count <= 9000 and accum < 2^25, so the high
// product by 2^32 / count rounded up is the quotient or one more (svtme_tffh.hip's tffh_norm16)
template <int N>
__device__ __forceinline__ void tfld_norm(uint32_t acc[N], uint32_t cnt) {
    const uint32_t m = 0xFFFFFFFFu / cnt + 1u;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const uint32_t v = acc[k] + (cnt >> 1);
        uint32_t q       = __umulhi(v, m);
        q -= q * cnt > v;
        acc[k] = q;
    }
}

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
    tfld_load<T, 16>(A.cen_y + yo, cen);
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = 1000u * cen[k];
    if constexpr (CHROMA) {
#pragma unroll
        for (int p = 0; p < 2; p++) {
            tfld_load<T, 4>(A.cen_c[p] + co, cacc[p]);
#pragma unroll
            for (int k = 0; k < 4; k++) cacc[p][k] *= 1000u;
        }
    }

    for (uint32_t r = 0; r < A.n; r++) {
        uint32_t pre[16], cpre[2][4];
        tfld_load<T, 16>(A.ref_y[r] + yo, pre);
        if constexpr (CHROMA) {
            tfld_load<T, 4>(A.ref_c[0][r] + co, cpre[0]);
            tfld_load<T, 4>(A.ref_c[1][r] + co, cpre[1]);
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
        uint32_t var, e;
        if constexpr (BPP == 1) {
            var = (ssek - (uint32_t)(((int64_t)sk * sk) >> (10 - ss))) << ss; // / (32 * (32 >> shift))
            e   = var >> 2;                                                  // (:831)
        } else {
            const uint32_t s4 = (ssek + 8u) >> 4;
            const int s2      = (sk + 2) >> 2;
            const int64_t v   = (int64_t)s4 - (((int64_t)s2 * s2) >> (10 - ss));
            var               = (uint32_t)(v >= 0 ? v : 0) << ss;
            e                 = var >> 6; // (:933)
        }
        if (A.var32 && lane == 0)
            A.var32[((size_t)r * A.sbs + b64) * 4 + wid] = var;
        uint32_t w[3];
#pragma unroll
        for (int p = 0; p < (CHROMA ? 3 : 1); p++) {
            const uint32_t dd = (A.decay[p] >> 10) ? (A.decay[p] >> 10) : 1u;
            uint32_t sd       = (e << 2) / dd;
            sd                = sd < 112u ? sd : 112u;
            w[p]              = (uint32_t)(c_tfld_exp.v[sd] * 1000) >> 17;
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
        tfld_norm<16>(acc, cnt[0]);
        const bool half = x + 16 > A.W;
        tfld_store<T, 16>(A.dst_y.base + (ptrdiff_t)y * A.dst_y.stride + (ptrdiff_t)x * BPP, acc, half);
        if constexpr (BPP == 2) {
            if (A.dst8.base) { // the result picture's level 0: the MSB plane
#pragma unroll
                for (int k = 0; k < 16; k++) acc[k] >>= 2;
                tfld_store<uint8_t, 16>(A.dst8.base + (ptrdiff_t)y * A.dst8.stride + x, acc, half);
            }
        }
    }
    if constexpr (CHROMA) {
        if (cx < (A.W >> 1) && cy < (A.H >> 1)) {
#pragma unroll
            for (int p = 0; p < 2; p++)
                if (A.dst_c[p].base) {
                    tfld_norm<4>(cacc[p], cnt[1 + p]);
                    tfld_store<T, 4>(A.dst_c[p].base + (ptrdiff_t)cy * A.dst_c[p].stride + (ptrdiff_t)cx * BPP, cacc[p],
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
