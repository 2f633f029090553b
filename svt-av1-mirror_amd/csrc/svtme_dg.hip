// svtme_dg.hip — the dynamic-GOP detector's early HME search as a picture-pair
// job (svtme_dg_detect, include/svtme.h): TASK_DG_DETECTOR_HME of the
// reference's ME threads (me_process.c:327-333, dg_detector_hme_level0 and
// early_hme_b64, pd_process.c:393-590). Per 64x64 SB one exhaustive full-SAD
// search of the 16x16 block of the current picture's sixteenth plane over up
// to 128 x 128 positions of the reference picture's sixteenth plane, then the
// frame metrics of the pair.
//
// One 256-thread workgroup per (pair, SB). The clamped reference window
// (sa_w + 15 columns x sa_h + 15 rows, at most 143 x 143 bytes) is staged in
// LDS once, shifted so that position 0 starts a dword; the 16 x 16 source block
// sits in 64 SGPRs. A lane owns aligned position quads (v_qsad_pk_u16_u8: the
// 4 SADs of one source dword against the 4 byte shifts of a dword pair) of 8
// consecutive position rows, so that one LDS row read (5 dwords) feeds up to
// 8 x 4 qsads. The largest SAD is 16 * 16 * 255 = 65 280: the u16 accumulators
// hold the whole block. The argmin is an integer min of
// sad << 14 | y * 128 + x (30 bits): the reference's loop visits positions
// y-major then x with a strict <, so the first position in raster order wins
// a tie, which is the smallest key.
//
// Reads stay inside the device sixteenth plane: with w16 = W / 4 the clamp
// gives x0 = org_x + sa_origin_x >= -15 and x0 + sa_w <= w16, so window bytes
// lie in x in [-15, w16 + 14] (y alike). The staging reads whole aligned
// dwords of at most nq + 5 dwords from (x0 & ~3), nq = ceil(sa_w / 4): bytes
// from >= -16 to <= x0 + 4 (nq + 3) + 7 <= w16 + 22. A plane row holds
// x in [-16, stride - 16) with stride >= w16 + 16 + 24 (svtme_plane_geometry),
// rows y in [-16, h16 + 16). The source block reads x in [org_x, org_x + 15]
// with org_x <= w16 - 1, the same range.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svtme_launch.h"
#include "svtme_me_common.h"

using namespace svtme;

struct DgArgs {
    DevPlane cur[SVTME_DG_MAX_PAIRS]; // sixteenth planes of the pairs
    DevPlane ref[SVTME_DG_MAX_PAIRS];
    svtme_dg_metrics *acc; // [n], zeroed: the four accumulated fields
    svtme_dg_sb *sb;       // [n][sbs]
    uint32_t sbs, pic_w_b64, pic_h_b64;
    int16_t sa_w, sa_h;
};

#define DG_PITCH 37 // dwords per staged row (32 quads + 4, odd: row blocks on different banks)
#define DG_ROWS 143 // 128 + 15
#define DG_PR 8     // position rows per lane and task

typedef uint32_t dg_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(4))) const dg_u32x4 c_u32x4; // constant address space: scalar loads
typedef __attribute__((address_space(1))) const uint32_t g_u32;   // global, not flat, loads

// one axis of early_hme_b64's window clamp (pd_process.c:409-449), int16 arithmetic; pad = 16 - 1
__device__ __forceinline__ void dg_clamp(int16_t org, int16_t dim, int16_t *origin, int16_t *sa, bool mult8) {
    int16_t o = i16(-(*sa >> 1)), s = *sa;
    const int16_t pad = 15;
    if (org + o < -pad) {
        o = i16(-pad - org);
        s = i16(s - (-pad - (org + o))); // zero once the origin has moved: the area is not reduced
    }
    if (org + o > dim - 1)
        o = i16(o - ((org + o) - (dim - 1)));
    if (org + o + s > dim) {
        const int16_t t = i16(s - ((org + o + s) - dim));
        s               = t > 1 ? t : 1;
    }
    if (mult8)
        s = s < 8 ? s : i16(s & ~7);
    *origin = o;
    *sa     = s;
}

__global__ void __launch_bounds__(256) k_dg(const DgArgs A) {
    __shared__ uint32_t win[DG_ROWS * DG_PITCH];
    __shared__ uint32_t wmin[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t u    = UNI(xcd_remap(blockIdx.x, gridDim.x));
    const uint32_t pair = UNI(u / A.sbs), b64 = u - pair * A.sbs;
    const uint32_t by = UNI(b64 / A.pic_w_b64), bx = b64 - by * A.pic_w_b64;
    DevPlane C = A.cur[0], R = A.ref[0];
#pragma unroll
    for (int k = 1; k < SVTME_DG_MAX_PAIRS; k++) // constant-index argument reads
        if (pair == (uint32_t)k) {
            C = A.cur[k];
            R = A.ref[k];
        }
    const int16_t org_x = i16(((int16_t)(bx * 64)) >> 2), org_y = i16(((int16_t)(by * 64)) >> 2);
    int16_t ox, oy, sw = i16((A.sa_w + 7) & ~7), sh = A.sa_h;
    dg_clamp(org_x, i16(R.width), &ox, &sw, true);
    dg_clamp(org_y, i16(R.height), &oy, &sh, false);
    const int x0 = org_x + ox, y0 = org_y + oy;
    const int nq = (sw + 3) >> 2, ndw = nq + 4, nrow = sh + 15;

    // the source block: 16 rows of 4 dwords, scalar loads (16-byte aligned: org_x is a multiple of 16)
    uint32_t src[16][4];
    {
        const uint8_t *sp = uni_ptr(C.base + (ptrdiff_t)org_y * C.stride + org_x);
        const int sst     = UNI(C.stride);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const dg_u32x4 v = *(c_u32x4 *)(uintptr_t)(sp + (ptrdiff_t)r * sst);
            src[r][0] = v.x, src[r][1] = v.y, src[r][2] = v.z, src[r][3] = v.w;
        }
    }
    // the window: staged dword j of row i holds bytes x0 + 4 j .. + 3 of plane row y0 + i
    {
        const int shb       = x0 & 3;
        const uint8_t *wp   = uni_ptr(R.base + (ptrdiff_t)y0 * R.stride + (x0 - shb));
        const int rst       = UNI(R.stride);
        const uint32_t m    = magic_u32((uint32_t)ndw);
        const int total     = nrow * ndw;
        for (int i = tid; i < total; i += 256) {
            const int row = mdiv(i, m), j = i - row * ndw;
            const g_u32 *p = (const g_u32 *)(uintptr_t)(wp + (ptrdiff_t)row * rst) + j;
            win[row * DG_PITCH + j] = __builtin_amdgcn_alignbyte(p[1], p[0], (uint32_t)shb);
        }
    }
    __syncthreads();

    uint32_t best = U32MAX;
    const int nrb = (sh + DG_PR - 1) / DG_PR, ntask = nq * nrb;
    const uint32_t mq = magic_u32((uint32_t)nq);
    for (int t = tid; t < ntask; t += 256) {
        const int rb = mdiv(t, mq), q = t - rb * nq;
        const uint32_t *L = win + rb * DG_PR * DG_PITCH + q;
        unsigned long long a[DG_PR] = {};
        // window row DG_PR rb + i is block row i - j of position row DG_PR rb + j
#pragma unroll
        for (int i = 0; i < DG_PR + 15; i++) {
            uint32_t d[5];
#pragma unroll
            for (int k = 0; k < 5; k++) d[k] = L[i * DG_PITCH + k];
#pragma unroll
            for (int j = 0; j < DG_PR; j++) {
                const int r = i - j;
                if (r < 0 || r > 15)
                    continue;
#pragma unroll
                for (int k = 0; k < 4; k++) a[j] = qsad(d[k], d[k + 1], src[r][k], a[j]);
            }
        }
        const int xb = 4 * q, yb = DG_PR * rb;
        const bool whole = xb + 3 < sw && yb + DG_PR - 1 < sh;
#pragma unroll
        for (int j = 0; j < DG_PR; j++) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const uint32_t sad = (uint32_t)(a[j] >> (16 * e)) & 0xFFFFu;
                const uint32_t key = (sad << 14) + (uint32_t)(((yb + j) << 7) + xb + e);
                if (whole || (xb + e < sw && yb + j < sh))
                    best = min_u32(best, key);
            }
        }
    }
    best = wave_min_u32(best);
    if (lane == 0)
        wmin[wid] = best;
    __syncthreads();
    if (tid == 0) {
        best = min_u32(min_u32(wmin[0], wmin[1]), min_u32(wmin[2], wmin[3]));
        const uint32_t sad = best >> 14;
        const int16_t mvx = i16(i16((int)(best & 127u) + ox) * 4);
        const int16_t mvy = i16(i16((int)((best >> 7) & 127u) + oy) * 4);
        // one 8-byte vector store of {sad, mv_x, mv_y}
        *(uint2 *)(A.sb + (size_t)pair * A.sbs + b64) =
            make_uint2(sad, (uint32_t)(uint16_t)mvx | ((uint32_t)(uint16_t)mvy << 16));
        // frame metrics (pd_process.c:543-580): the middle row / column counts nothing
        svtme_dg_metrics *M = A.acc + pair;
        atomicAdd((unsigned long long *)&M->tot_dist, (unsigned long long)sad);
        if (sad > 16 * 16 * 30)
            atomicAdd(&M->tot_cplx, 1u);
        if (mvx != 0 || mvy != 0)
            atomicAdd(&M->tot_active, 1u);
        const int sy = mvy > 0 ? 1 : mvy < 0 ? -1 : 0, sx = mvx > 0 ? 1 : mvx < 0 ? -1 : 0;
        const uint32_t hy = A.pic_h_b64 / 2, hx = A.pic_w_b64 / 2;
        const int in = (by < hy ? -sy : by > hy ? sy : 0) + (bx < hx ? -sx : bx > hx ? sx : 0);
        if (in)
            atomicAdd(&M->sum_in_vectors, in);
    }
}

// n pairs of one size in one launch; acc zeroed by the caller on the same stream
extern "C" hipError_t svtme_launch_dg(const DevPlane *cur, const DevPlane *ref, uint32_t n, uint32_t width,
                                      uint32_t height, uint16_t sa_w, uint16_t sa_h, svtme_dg_metrics *d_acc,
                                      svtme_dg_sb *d_sb, hipStream_t s) {
    if (!n || n > SVTME_DG_MAX_PAIRS)
        return hipErrorInvalidValue;
    DgArgs A{};
    for (uint32_t k = 0; k < SVTME_DG_MAX_PAIRS; k++) {
        A.cur[k] = cur[k < n ? k : 0];
        A.ref[k] = ref[k < n ? k : 0];
    }
    A.acc       = d_acc;
    A.sb        = d_sb;
    A.pic_w_b64 = (width + 63) / 64;
    A.pic_h_b64 = (height + 63) / 64;
    A.sbs       = A.pic_w_b64 * A.pic_h_b64;
    A.sa_w      = (int16_t)sa_w;
    A.sa_h      = (int16_t)sa_h;
    hipLaunchKernelGGL(k_dg, dim3(n * A.sbs), dim3(256), 0, s, A);
    return hipGetLastError();
}

extern "C" hipError_t svtme_prime_dg(void) { // (see svtme_prime_pyramid)
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void *)k_dg);
}
