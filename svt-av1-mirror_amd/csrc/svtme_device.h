// svtme_device.h — device-side layouts shared by the HIP kernels and the host
// code (svtme_ctx.h and its files). gfx950 (MI355X) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svtme.h"

// Device plane margins. The LOGICAL padding the search clamps use is the
// reference's (72 / 32 / 16, reference_object.c:243-305); the device margins
// are at least as wide and keep each interior row start 16-byte aligned and
// 8 bytes of slack on the right for aligned dword loads. Margins hold the same
// edge-replicated samples as the reference's padding.
#define SVTME_DEV_FULL_LEFT 80
#define SVTME_DEV_FULL_TOP 72
#define SVTME_DEV_Q_LEFT 32
#define SVTME_DEV_Q_TOP 32
#define SVTME_DEV_S_LEFT 16
#define SVTME_DEV_S_TOP 16

struct DevPlane {
    uint8_t *base;   // interior sample (0, 0); negative offsets reach the padding
    int32_t stride;  // bytes per row (multiple of 64)
    int32_t width;   // interior width
    int32_t height;  // interior height
    int32_t pad;     // logical padding (org_x == org_y of the reference plane)
};

// Chroma planes (svtme_picture_upload_chroma; 8-bit 4:2:0). The LOGICAL padding is
// SVTME_PAD_CHROMA (40): the chroma predictor of temporal filtering reaches 39
// samples beyond each edge. The device margins are 48 on the left
// and at least 48 on the right (16-byte aligned interior row starts, 8 bytes of
// slack beyond the padding for aligned dword loads), 40 rows above and below.
#define SVTME_DEV_C_LEFT 48
#define SVTME_DEV_C_TOP 40

struct DevPyramid {
    DevPlane lv[3];  // 0 = full, 1 = quarter, 2 = sixteenth
};

// Stage-A result of one search (svtme_stages.hip). Index layout per SB:
// [0, 8) zz SAD by slot (sad = raw sub-sampled n x m sum), [8, 24) pre-HME
// slot * 2 + region, [24, 56) HME level 0 slot * 4 + quadrant (sx * 2 + sy).
struct ARes {
    uint32_t sad;
    int16_t x, y; // final (scaled, absolute) search-centre MV
};
#define SVTME_A_ZZ 0
#define SVTME_A_PH 8
#define SVTME_A_L0 24
#define SVTME_A_N 56

// Per-SB state between the stages (svtme_stages.hip). Stage D writes each
// slot's zz SAD and do_ref after the zz / pre-HME pruning and the level-0
// centres after the worst-quadrant replacement; stage B writes the level-1/2
// refinement of every (slot, quadrant); stage C selects the search centre
// from the highest enabled level (set_final_seach_centre_sb).
struct BState {
    uint64_t lsad[8][4]; // level 0, [slot][q = sx * 2 + sy]
    uint64_t hsad[8][4]; // highest enabled level above 0
    int16_t lx[8][4], ly[8][4];
    int16_t hx[8][4], hy[8][4];
    uint32_t zz[8];
    uint8_t do_ref[8];
    // real-time tune on the split path (k_stage_d<true>): the HME-L0 area of
    // every slot from slot 0's centre, and the slots whose HME-L0 runs (bit s)
    int16_t rt_sa[8][2];
    uint8_t rt_need;
};

// Per (SB, reference record) state the wide full-pel stage (k_stage_c1)
// leaves for the per-SB decode (k_stage_e), svtme_stages.hip.
struct CSlot {
    uint64_t hme_sad;
    uint32_t zz;
    int16_t sc_x, sc_y;        // HME search centre (record fields)
    int16_t xo, yo, w, xc, yc; // full-pel window origin and width, probe centre
    uint8_t searched, do_ref, probe, tf_exit;
};

// Parameters of one picture job as the kernel sees them.
struct DevJob {
    svtme_job job;                 // controls + picture description (host copy)
    DevPyramid cur;
    DevPyramid ref[2][4];
    svtme_ref_record *out_records; // [sb_count][R]
    svtme_sb_result *out_sb;       // [sb_count] or nullptr
    uint32_t R;
    uint32_t pic_w_b64;
    ARes *ares;                    // [sb_count][SVTME_A_N] stage-A results
    BState *bst;                   // [sb_count] stage-B state
    uint32_t ta_count;             // stage-A searches per SB
    uint8_t ta_list[SVTME_A_N];    // their ARes indices
    uint32_t ta1_count;            // real-time tune, split path: the second stage-A round
    uint8_t ta1_list[8];           // (TA_L0RT << 3 | slot)
    uint32_t tb_count;             // stage-B refinements per SB
    uint8_t tb_list[32];           // their (slot << 2 | quadrant)
    unsigned long long *keys;      // [sb_count][R][85] full-pel argmin keys (sad << 32 | order)
    CSlot *cslot;                  // [sb_count][R]
    uint32_t parts;                // search-row bands per (SB, reference) in k_stage_c1; 0 = per-SB k_stage_c
    // per-slot search parameters independent of the SB (svtme_hme_prepare, host)
    uint16_t sdist[8];             // |picture distance| of slot s (ref_dist_const)
    int16_t l0_sa[8][2];           // HME-L0 area (get_hme_l0_search_area)
    int16_t ph_sa[8][2][2];        // pre-HME region areas (prehme_core)
    uint32_t paths;                // SVTME_PATH_* of the submitting context (host dispatch only)
};

// A launch over a batch of picture jobs (svtme_submit_batch_device). The jobs
// live in device memory; start[k] is the first work unit (wave or workgroup,
// per stage) of job k in this launch, start[n..] = UINT32_MAX. Unit u belongs
// to the job with the largest start[k] <= u (constant-index compares: the
// kernel argument is never indexed dynamically).
#define SVTME_MAX_BATCH 16
struct DevBatch {
    const DevJob *jobs;
    uint32_t n;
    uint32_t total; // units of this launch
    uint32_t start[SVTME_MAX_BATCH];
};

// Stage-A search kinds (DevJob.ta_list / ta1_list entries are kind << 3 | slot): written by the
// host's stage lists (svtme_dispatch.cpp), read by k_stage_a and k_l0_full.
#define TA_HME 0   // zz SAD + the four HME-L0 quadrants of one slot
#define TA_PH 1    // the two pre-HME regions of one slot
#define TA_ZZ 2    // zz SAD only (real-time tune, slots 1-7: their HME-L0 waits for slot 0's)
#define TA_L0RT 3  // the four HME-L0 quadrants with the area k_stage_d<true> left in BState

// LDS row geometry of k_fp_wide that the host's svtme_fp_wide_lds tests an area against.
#define FPW_BOFF 40  // fw_b within the row: one base address serves both copies
#define FPW_TQ 4 // position quads per set (2 quad pairs, 16 positions; 6 wastes a third of the
                 // last set at 64 positions, 8 measures the same as 4)
// svtme_fp_wide_lds admits 14 + nsets * FPW_TQ + 3 <= FPW_BOFF; k_fp_wide codes a record's set
// in 8 bits (rc & 0xFF), so that bound must keep nsets below 256
static_assert((FPW_BOFF - 14 - 3) / FPW_TQ < 256, "k_fp_wide's 8-bit set code holds every nsets svtme_fp_wide_lds admits");

// Search parameters the host's dispatch and the kernels derive alike (pure).
#define SVTME_HD __host__ __device__ __forceinline__
namespace svtme {
SVTME_HD int16_t i16(int v) { return (int16_t)v; }
SVTME_HD int absi(int v) { return v < 0 ? -v : v; }
SVTME_HD int imin(int a, int b) { return a < b ? a : b; }
SVTME_HD uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }
SVTME_HD uint64_t min_u64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// motion_estimation.c:1239-1243
SVTME_HD uint16_t scaled_dist(uint16_t dist) {
    uint8_t round_up = ((dist % 8) == 0) ? 0 : 1;
    return (uint16_t)(((dist * 5) / 8) + round_up);
}
SVTME_HD uint16_t ref_dist_const(const svtme_job &j, int l, int r) {
    int64_t d = (int64_t)j.picture_number - (int64_t)j.ref_picture_number[l][r];
    return (uint16_t)(int16_t)(d < 0 ? -d : d);
}

// get_hme_l0_search_area (motion_estimation.c:1800-1867); the per-ref
// mutate/restore of hme_l0_sa makes it a function of (list, ref, dist)
SVTME_HD void hme_l0_area(const svtme_controls &c, int l, int r, uint16_t dist, int16_t l00x, int16_t l00y,
                          int16_t *sa_w, int16_t *sa_h) {
    uint32_t mnw = c.hme_l0_sa.sa_min.width, mnh = c.hme_l0_sa.sa_min.height;
    uint32_t mxw = c.hme_l0_sa.sa_max.width, mxh = c.hme_l0_sa.sa_max.height;
    if (c.enable_me_sr_adjustment && c.distance_based_hme_resizing) {
        uint8_t is_hor = 1, is_ver = 1, is_still = 0;
        if (c.reduce_hme_l0_sr_th_min && c.reduce_hme_l0_sr_th_max && (l || r)) {
            const int mvx = l00x, mvy = l00y;
            is_ver   = (absi(mvx) < c.reduce_hme_l0_sr_th_min) && (absi(mvy) > c.reduce_hme_l0_sr_th_max);
            is_hor   = (absi(mvx) > c.reduce_hme_l0_sr_th_max) && (absi(mvy) < c.reduce_hme_l0_sr_th_min);
            is_still = (absi(mvx) < (c.reduce_hme_l0_sr_th_min * 3)) && (absi(mvy) < (c.reduce_hme_l0_sr_th_min * 3));
        }
        uint8_t xo = 1, yo = 1;
        if (!is_ver)
            yo = 2;
        if (!is_hor)
            xo = 2;
        if (c.enable_me_sr_adjustment == 2 && is_still)
            xo = yo = 4;
        mnw = (uint16_t)(mnw / (xo + r));
        mnh = (uint16_t)(mnh / (yo + r));
        mxw = (uint16_t)(mxw / (xo + r));
        mxh = (uint16_t)(mxh / (yo + r));
    }
    const int32_t f = scaled_dist(dist);
    int16_t w       = i16(mnw / c.num_hme_sa_w);
    w               = i16(imin((((w * f) + 15) & ~0x0F), (int)(((mxw / c.num_hme_sa_w) + 15) & ~0x0F)));
    int16_t h       = i16(mnh / c.num_hme_sa_h);
    h               = i16(imin((h * f), (int)(mxh / c.num_hme_sa_h)));
    *sa_w = w, *sa_h = h;
}
} // namespace svtme

static inline uint32_t svtme_round_up(uint32_t v, uint32_t a) { return (v + a - 1) / a * a; }
static inline uint32_t svtme_align8_u(uint32_t v) { return (v + 7u) & ~7u; }

// plane geometry for an aligned W x H picture
static inline void svtme_plane_geometry(int level, uint32_t W, uint32_t H, uint32_t *w, uint32_t *h, uint32_t *left,
                                        uint32_t *top, uint32_t *stride, uint32_t *rows, uint32_t *pad) {
    if (level == 0) {
        *w = W, *h = H, *left = SVTME_DEV_FULL_LEFT, *top = SVTME_DEV_FULL_TOP, *pad = SVTME_PAD_FULL;
        *stride = svtme_round_up(W + SVTME_DEV_FULL_LEFT + 88, 64);
    } else if (level == 1) {
        *w = W / 2, *h = H / 2, *left = SVTME_DEV_Q_LEFT, *top = SVTME_DEV_Q_TOP, *pad = SVTME_PAD_QUARTER;
        *stride = svtme_round_up(W / 2 + SVTME_DEV_Q_LEFT + 40, 64);
    } else {
        *w = W / 4, *h = H / 4, *left = SVTME_DEV_S_LEFT, *top = SVTME_DEV_S_TOP, *pad = SVTME_PAD_SIXTEENTH;
        *stride = svtme_round_up(W / 4 + SVTME_DEV_S_LEFT + 24, 64);
    }
    *rows = *h + 2 * *top;
}

// chroma plane geometry (Cb and Cr alike) for an aligned W x H picture, 4:2:0
static inline void svtme_chroma_geometry(uint32_t W, uint32_t H, uint32_t *w, uint32_t *h, uint32_t *left,
                                         uint32_t *top, uint32_t *stride, uint32_t *rows) {
    *w = W / 2, *h = H / 2, *left = SVTME_DEV_C_LEFT, *top = SVTME_DEV_C_TOP;
    *stride = svtme_round_up(W / 2 + SVTME_DEV_C_LEFT + 48, 64);
    *rows   = *h + 2 * *top;
}

// geometry of the attached 16-bit luma plane (svtme_picture_attach_10bit) of an aligned W x H picture:
// level 0's in samples (80 left, at least 88 right, 72 rows above and below, the logical padding
// SVTME_PAD_FULL), two bytes a sample; `stride` is in bytes. A DevPlane describes it with `base` at
// sample (0, 0), the stride in bytes and width, height and pad in samples.
static inline void svtme_hbd_geometry(uint32_t W, uint32_t H, uint32_t *left, uint32_t *top, uint32_t *stride,
                                      uint32_t *rows) {
    *left = SVTME_DEV_FULL_LEFT, *top = SVTME_DEV_FULL_TOP;
    *stride = svtme_round_up((W + SVTME_DEV_FULL_LEFT + 88) * 2, 64);
    *rows   = H + 2 * *top;
}

// geometry of the attached 16-bit chroma planes (svtme_picture_attach_chroma_10bit; Cb and Cr alike) of
// an aligned W x H picture, 4:2:0: the 8-bit chroma planes' in samples (48 left, at least 48 right, 40
// rows above and below, the logical padding SVTME_PAD_CHROMA), two bytes a sample; `stride` is in bytes
// (a multiple of 64; an interior row starts 96 bytes into its row, 16-byte aligned). A DevPlane
// describes a plane as svtme_hbd_geometry's: stride in bytes, width, height and pad in samples.
static inline void svtme_hbd_chroma_geometry(uint32_t W, uint32_t H, uint32_t *w, uint32_t *h, uint32_t *left,
                                             uint32_t *top, uint32_t *stride, uint32_t *rows) {
    *w = W / 2, *h = H / 2, *left = SVTME_DEV_C_LEFT, *top = SVTME_DEV_C_TOP;
    *stride = svtme_round_up((W / 2 + SVTME_DEV_C_LEFT + 48) * 2, 64);
    *rows   = *h + 2 * *top;
}

// Arguments of temporal filtering's two stages (svtme_tff.hip), filled by the host
// (svtme_windows.cpp) and checked by svtme_launch_tf_stage. As in TfldArgs the planes are addressed
// in bytes at either depth and the launcher's `hbd` chooses the sample type: at 8 bit the luma planes
// are level 0 and the chroma planes the attached 8-bit ones, at 10 bit the attached 16-bit planes.
// Strides are in bytes; a DevPlane's width and height are in samples.
// The luma stage: k_tff_pred, k_tff_norm.
struct TfLumaArgs {
    DevPlane cen;                       // the centre picture's plane
    DevPlane ref[SVTME_MAX_BATCH_JOBS]; // the references'
    const svtme_tf_subpel_sb *sub;      // [n][sbs]
    uint8_t *tile;                      // [n][sbs][64 * 64] predictions
    uint32_t *wgt;                      // [n][sbs][16] weights, 32x32 block * 4 + quarter
    uint32_t *e32;                      // [n][sbs][4] 32x32 errors
    uint8_t *plane;                     // dense: the filtered plane, whole SBs, pic_w_b64 * 64 samples a row
    DevPlane dst;                       // into the result picture: its plane (may be cen)
    DevPlane dst8;                      //   10 bit: and its level 0, the MSB plane; unused at 8 bit
    uint32_t decay, dist_th, ss;        // svtme_tf_filter_controls
    uint32_t n, sbs, pic_w_b64;
    int32_t W, H; // the 8-aligned picture
};

// The chroma stage: k_tff_pred_uv, k_tff_norm_uv. Plane 0 is Cb, 1 is Cr; every picture of a
// window has the same chroma geometry, so the references are base pointers with one stride.
struct TfChromaArgs {
    DevPlane cen_y;                                // the centre picture's luma plane
    DevPlane cen[2];                               // its chroma planes
    const uint8_t *ref[2][SVTME_MAX_BATCH_JOBS];   // interior sample (0, 0) of the references' chroma planes
    int32_t ref_stride;
    const svtme_tf_subpel_sb *sub;                 // [n][sbs]
    const uint8_t *tile_y;                         // [n][sbs][64 * 64] luma predictions (k_tff_pred)
    const uint32_t *e32;                           // [n][sbs][4] 32x32 errors (k_tff_pred)
    uint8_t *tile;                                 // [n][sbs][2][32 * 32] chroma predictions
    uint32_t *wgt;                                 // [n][sbs][2][16] chroma weights
    uint8_t *plane;                                // dense: [2] planes of whole SBs, pic_w_b64 * 32 samples a row
    DevPlane dst[2];                               // into the result picture: its chroma planes (may be cen)
    uint32_t decay_cb, decay_cr, dist_th;
    uint32_t n, sbs, pic_w_b64;
    int32_t W, H;                                  // the 8-aligned luma size
};

// Arguments of the low-delay filter (svtme_tfld.hip: k_tfld), filled by the host. Every picture of a
// window has the same geometry, so the sources are pointers to interior sample (0, 0) with one stride
// per kind of plane. At 8 bit the luma planes are level 0 and the chroma planes the attached 8-bit
// ones; at 10 bit the attached 16-bit planes. Strides are in bytes.
struct TfldArgs {
    const uint8_t *cen_y, *cen_c[2];                 // the centre picture (cen_c: with chroma)
    const uint8_t *ref_y[SVTME_MAX_BATCH_JOBS];      // the references
    const uint8_t *ref_c[2][SVTME_MAX_BATCH_JOBS];
    int32_t y_stride, c_stride;
    DevPlane dst_y, dst_c[2]; // a dense plane or the result picture's (may be the centre's); dst_c[p].base may be NULL
    DevPlane dst8;            // 10 bit, the window call: the result picture's level 0; base NULL: none
    uint32_t *var32;          // NULL or [n][sbs][4]
    uint32_t decay[3], ss;    // svtme_tf_ld_controls
    uint32_t n, sbs, pic_w_b64;
    int32_t W, H; // the 8-aligned luma size
};

// Bytes per unit (one reference's SB) of the temporal filter's scratch sections at 8 bit, as
// svtme_tff.hip indexes them; the host lays the sections out by these (TfScratch, svtme_windows.cpp).
// At 10 bit the sections of samples (tiles, dense planes) hold two bytes a sample: these times two.
#define SVTME_TFF_TILE_BYTES 4096   // luma prediction: 64 x 64 samples (the dense luma plane holds as much per SB)
#define SVTME_TFF_WGT_BYTES 64      // luma weights: `A.wgt[unit * 16 + ...]`, 16 dwords
#define SVTME_TFF_E32_BYTES 16      // 32x32 errors: `A.e32[unit * 4 + ...]`, 4 dwords
#define SVTME_TFFC_TILE_BYTES 2048  // Cb and Cr predictions: 2 x 32 x 32 samples
#define SVTME_TFFC_WGT_BYTES 128    // chroma weights: `A.wgt[unit * 32 + ...]`, 32 dwords
#define SVTME_TFFC_PLANE_SB_BYTES 1024 // one SB of one dense chroma plane: 32 x 32 samples
