/*
 * svtme.h — C ABI of the MI355X-native open-loop motion-estimation (ME) stage.
 *
 * Two surfaces, both plain C (pointers + sizes, no torch types):
 *
 *  1. Per-kernel rtcd variants (`*_hip`). Byte-identical signatures to the
 *     reference's run-time-dispatch pointers so an encoder can register them
 *     as a new variant after `svt_aom_setup_rtcd_internal`.
 *     They take caller-owned HOST memory, run synchronously on the GPU and
 *     return through the same out-params. They exist for drop-in registration
 *     and per-kernel parity; one call is far below a GPU launch in size.
 *
 *  2. The picture-level job API (`svtme_*`). This is the performance boundary:
 *     it replaces the per-SB loop of the ME thread
 *     (reference Source/Lib/Codec/me_process.c:174-290) with one GPU job that
 *     covers every 64x64 superblock (SB) x every reference of one picture.
 *     Pictures are uploaded once; their padded full / quarter / sixteenth
 *     pyramids stay resident in HBM, keyed by picture_number, until released.
 *
 * No entry point falls back to a CPU path. A HIP failure is reported through
 * the returned status (job API) or svtme_last_error() (rtcd variants), and a
 * message on stderr.
 */
#ifndef SVTME_H
#define SVTME_H

#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * Constants (reference values cited)
 * ------------------------------------------------------------------------- */
#define SVTME_PU_COUNT 85           /* SQUARE_PU_COUNT, me_sb_results.h:24 */
#define SVTME_MAX_LISTS 2           /* MAX_NUM_OF_REF_PIC_LIST, definitions.h:2337 */
#define SVTME_MAX_REFS 4            /* REF_LIST_MAX_DEPTH, EbSvtAv1Enc.h:36 */
#define SVTME_MAX_PA_ME_CAND 23     /* MAX_PA_ME_CAND, me_sb_results.h:22 */
#define SVTME_MAX_PA_ME_MV 7        /* MAX_PA_ME_MV, me_sb_results.h:21 */
#define SVTME_MAX_SAD_VALUE (128u * 128u * 255u) /* motion_estimation.h:85 */
#define SVTME_SUB_SAD_SEARCH 0      /* definitions.h:2071 */
#define SVTME_FULL_SAD_SEARCH 1     /* definitions.h:2072 */
/* svtme_job.me_type: the EbMeType values of me_context.h:44-51 */
#define SVTME_ME_MCTF 1             /* temporal-filtering ME (temporal_filtering.c:3169) */
#define SVTME_ME_OPEN_LOOP 3        /* pre-analysis open-loop ME (me_process.c:266) */
#define SVTME_PAD_FULL 72           /* PA full-res padding (enc_handle.c:4057-4069) */
#define SVTME_PAD_QUARTER 32        /* b64_size >> 1, reference_object.c:272 */
#define SVTME_PAD_SIXTEENTH 16      /* b64_size >> 2, reference_object.c:287 */

/* Status codes: the values of EbErrorType (API/EbSvtAv1.h:121-130). */
typedef int32_t svtme_status;
#define SVTME_OK 0
#define SVTME_ERR_INSUFFICIENT_RESOURCES ((int32_t)0x80001000)
#define SVTME_ERR_UNDEFINED ((int32_t)0x80001001)
#define SVTME_ERR_BAD_PARAMETER ((int32_t)0x80001005)

/* ---------------------------------------------------------------------------
 * Picture-level ME controls: a POD snapshot of the MeContext control fields
 * (me_context.h:280-364, 366-509) as set per picture by svt_aom_sig_deriv_me
 * (enc_mode_config.c:671-808). The GPU takes them as parameters; it never
 * re-derives them from the preset.
 * ------------------------------------------------------------------------- */
typedef struct svtme_area {
    uint16_t width;
    uint16_t height;
} svtme_area;

typedef struct svtme_area_minmax {
    svtme_area sa_min;
    svtme_area sa_max;
} svtme_area_minmax;

typedef struct svtme_controls {
    /* search methods: SVTME_SUB_SAD_SEARCH / SVTME_FULL_SAD_SEARCH */
    uint8_t hme_search_method;
    uint8_t me_search_method;
    /* HME enables (me_context.h:409-412) */
    uint8_t enable_hme_flag;
    uint8_t enable_hme_level0_flag;
    uint8_t enable_hme_level1_flag;
    uint8_t enable_hme_level2_flag;
    /* number of HME-L0 search regions; only 2x2 is supported (motion_estimation.c:1875) */
    uint8_t num_hme_sa_w;
    uint8_t num_hme_sa_h;
    /* search areas (MeHmeSearchAreaCtrls, me_context.h:342-347 / 421-429); a job is refused when
     * hme_l2_sa.width exceeds 8192 with HME level 2 on, or when the widest full-pel area (me_sa max x
     * the mv multiplier x 3/2 variance growth) exceeds 1016 positions with enable_me_sr_adjustment 2 */
    svtme_area_minmax hme_l0_sa;
    svtme_area hme_l1_sa;
    svtme_area hme_l2_sa;
    svtme_area_minmax me_sa;
    /* MeHmeRefPruneCtrls (me_context.h:280-290) */
    uint8_t enable_me_hme_ref_pruning;
    uint8_t pad0;
    uint16_t prune_ref_if_hme_sad_dev_bigger_than_th;
    uint16_t prune_ref_if_me_sad_dev_bigger_than_th;
    uint16_t zz_sad_pct;
    uint32_t zz_sad_th;
    uint32_t phme_sad_th;
    uint16_t phme_sad_pct;
    /* MeSrCtrls (me_context.h:292-305); with enable_me_sr_adjustment and HME on, an open-loop job
     * whose stationary_me_sr_divisor or me_sr_divisor_for_low_hme_sad is 0 is refused */
    uint8_t enable_me_sr_adjustment;
    uint8_t distance_based_hme_resizing;
    uint16_t reduce_me_sr_based_on_mv_length_th;
    uint16_t stationary_hme_sad_abs_th;
    uint16_t stationary_me_sr_divisor;
    uint16_t reduce_me_sr_based_on_hme_sad_abs_th;
    uint16_t me_sr_divisor_for_low_hme_sad;
    /* MvBasedSearchAdj (me_context.h:356-364) */
    uint8_t mv_sa_adj_enabled;
    uint8_t mv_sa_adj_nearest_ref_only;
    uint16_t mv_sa_adj_mv_size_th;
    uint16_t mv_sa_adj_sa_multiplier;
    /* Me8x8VarCtrls (me_context.h:310-319) */
    uint8_t me_8x8_var_enabled;
    uint8_t pad1;
    uint32_t me_sr_div4_th;
    uint32_t me_sr_div2_th;
    uint32_t me_sr_mult2_th;
    /* PreHmeCtrls (me_context.h:336-341) */
    uint8_t prehme_enable;
    uint8_t prehme_skip_search_line;
    uint8_t prehme_l1_early_exit;
    uint8_t pad2;
    svtme_area_minmax prehme_sa_cfg[2];
    /* misc (me_context.h:490-508) */
    int32_t prune_me_candidates_th;
    uint8_t use_best_unipred_cand_only;
    uint8_t reduce_hme_l0_sr_th_min;
    uint8_t reduce_hme_l0_sr_th_max;
    uint8_t pad3;
    uint32_t me_early_exit_th;
    uint32_t me_safe_limit_zz_th;
    uint32_t prev_me_stage_based_exit_th;
} svtme_controls;

/* ---------------------------------------------------------------------------
 * One picture's ME job (the fields the reference reads from
 * PictureParentControlSet / SequenceControlSet / MeContext per picture).
 * ------------------------------------------------------------------------- */
typedef struct svtme_job {
    uint64_t picture_number;
    uint32_t width;   /* luma width of the PA picture, multiple of 8 (aligned_width) */
    uint32_t height;  /* luma height, multiple of 8 (aligned_height) */
    uint64_t ref_picture_number[SVTME_MAX_LISTS][SVTME_MAX_REFS];
    uint8_t num_lists;                 /* 1 = P slice, 2 = B slice (me_process.c:219-221) */
    uint8_t num_refs[SVTME_MAX_LISTS]; /* ref_list{0,1}_count_try (me_process.c:223-225) */
    uint8_t temporal_layer_index;
    uint8_t is_ref;
    uint8_t hierarchical_levels;
    uint8_t similar_brightness_refs;
    /* candidate construction (motion_estimation.c:2532-2835) */
    uint8_t enable_me_8x8;
    uint8_t enable_me_16x16;
    uint8_t max_cand;   /* pa_me_data->max_cand (pcs.c:91-96) */
    uint8_t max_refs;   /* pa_me_data->max_refs */
    uint8_t max_l0;     /* pa_me_data->max_l0 */
    uint8_t only_l_bwd; /* scs->mrp_ctrls.only_l_bwd */
    uint8_t input_resolution; /* EbInputResolution: 0=240p .. 6=8K (definitions.h:2079-2085) */
    uint8_t gm_enabled;       /* pcs->gm_ctrls.enabled */
    uint8_t gm_use_distance_based_active_th;
    /* SVTME_ME_OPEN_LOOP (0 is accepted as the same) or SVTME_ME_MCTF. MCTF jobs
     * (one list, one reference) skip the HME/ME reference pruning, search the
     * full-pel area unscaled by distance (motion_estimation.c:1300-1302), stop
     * after HME when the list-0 ref-0 HME SAD is below tf_me_exit_th (:3109-3113)
     * and build no candidate arrays (:3126) */
    uint8_t me_type;
    uint8_t pad;
    uint16_t tf_me_exit_th; /* MeContext.tf_me_exit_th (me_context.h:495) */
    /* SB range [sb_begin, sb_begin + sb_count) in raster b64 order; sb_count 0 = all */
    uint32_t sb_begin;
    uint32_t sb_count;
    svtme_controls ctrl;
} svtme_job;

/* ---------------------------------------------------------------------------
 * Outputs.
 * ------------------------------------------------------------------------- */
/* Per SB x per searched (list, ref) slot; slots ordered list 0 refs then list 1
 * refs, R = num_refs[0] + (num_lists == 2 ? num_refs[1] : 0) slots per SB. */
typedef struct svtme_ref_record {
    uint32_t best_sad[SVTME_PU_COUNT]; /* p_sb_best_sad[l][r][] Z-order PUs; 0xFFFFFFFF if !searched */
    uint32_t best_mv[SVTME_PU_COUNT];  /* p_sb_best_mv[l][r][]: (uint32)(y<<16)|(uint16)x, full-pel */
    uint64_t hme_sad;    /* final search_results[l][r].hme_sad (HME SAD, or me_prune_ref's 8x8 sum) */
    int16_t hme_sc_x;    /* HME search centre (full-pel), search_results[l][r].hme_sc_{x,y} */
    int16_t hme_sc_y;
    uint32_t zz_sad;     /* zz_sad[l][r] (0xFFFFFFFF if not computed) */
    uint8_t searched;    /* do_ref when the integer search ran */
    uint8_t do_ref;      /* final do_ref */
    uint8_t tf_early_exit; /* MCTF only: HME-only exit taken (tf_use_pred_64x64_only_th = ~0, :3111) */
    uint8_t pad[5];        /* pad bytes are zero: every kernel path writes whole 704-byte records */
} svtme_ref_record; /* 704 bytes */

/* Per SB candidate list + distortions (MeSbResults, me_sb_results.h:44, and the
 * per-SB pcs arrays written by compute_distortion, motion_estimation.c:2964). */
typedef struct svtme_sb_result {
    uint8_t total_me_candidate_index[SVTME_PU_COUNT];
    uint8_t pad0[3];
    /* MeCandidate bit-field byte: direction | ref_idx_l0<<2 | ref_idx_l1<<4 |
     * ref0_list<<6 | ref1_list<<7 ; indexed [pu_index][cand] */
    uint8_t me_candidate_array[SVTME_PU_COUNT][SVTME_MAX_PA_ME_CAND];
    uint8_t pad1[1];
    uint32_t me_mv_array[SVTME_PU_COUNT][SVTME_MAX_PA_ME_MV]; /* [pu_index][max_refs slot] */
    uint32_t me_distortion[SVTME_PU_COUNT];
    uint32_t me_8x8_cost_variance;
    uint32_t rc_me_distortion;
    uint32_t me_64x64_distortion;
    uint32_t me_32x32_distortion;
    uint32_t me_16x16_distortion;
    uint32_t me_8x8_distortion;
    uint8_t stationary_block_present;
    uint8_t rc_me_allow_gm;
    uint8_t pad2[6];
} svtme_sb_result;

/* The last 24 bytes of svtme_ref_record: the per-reference state an encoder
 * keeps after the SB (search_results[l][r], zz_sad[l][r], me_context.h:459). */
typedef struct svtme_record_tail {
    uint64_t hme_sad;
    int16_t hme_sc_x;
    int16_t hme_sc_y;
    uint32_t zz_sad;
    uint8_t searched;
    uint8_t do_ref;
    uint8_t tf_early_exit;
    uint8_t pad[5]; /* zero, as in svtme_ref_record */
} svtme_record_tail;

/* Packed host output of svtme_submit_picture_packed_async: per SB, only what the
 * encoder's consumer reads, sized by its MeSbResults allocation (pcs.c:91-117),
 * so the device-to-host copy carries no unused candidate slots. SB k of the job
 * starts at byte k * svtme_packed_sb_bytes(layout, R):
 *   R records: svtme_ref_record (full_records = 1) or svtme_record_tail (0)
 *   when sb_results = 1:
 *     uint32 me_8x8_cost_variance, rc_me_distortion, me_64x64_distortion,
 *            me_32x32_distortion, me_16x16_distortion, me_8x8_distortion
 *     uint32 me_distortion[85]
 *     uint32 me_mv_array[n_pus][max_refs]
 *     uint8  stationary_block_present, rc_me_allow_gm, 0, 0
 *     uint8  total_me_candidate_index[n_pus]
 *     uint8  me_candidate_array[n_pus][max_cand]
 *   zero bytes up to the next multiple of 16.
 * The block is a function of the job's outputs alone: the pad bytes of the records and tails
 * are zero, best_sad is 0xFFFFFFFF on a slot that was not searched, and nothing of the job that
 * used the ticket's buffers before shows (tests/test_pack.py asserts each against the oracle). */
typedef struct svtme_pack_layout {
    uint16_t n_pus;       /* PUs with candidates: 85, 21 (no 8x8) or 5 (no 16x16) */
    uint8_t max_cand;     /* pa_me_data->max_cand, 1 .. SVTME_MAX_PA_ME_CAND */
    uint8_t max_refs;     /* pa_me_data->max_refs, 1 .. SVTME_MAX_PA_ME_MV */
    uint8_t full_records; /* 1: whole records (TF-ME reads the 85-PU winners), 0: tails */
    uint8_t sb_results;   /* 1: the SB-result fields (PA-ME) */
    uint8_t pad[2];
} svtme_pack_layout;

static inline uint32_t svtme_packed_sb_bytes(const svtme_pack_layout *L, uint32_t R) {
    uint32_t b = R * (L->full_records ? (uint32_t)sizeof(svtme_ref_record) : (uint32_t)sizeof(svtme_record_tail));
    if (L->sb_results)
        b += 4u * (6u + SVTME_PU_COUNT) + 4u * L->n_pus * L->max_refs + 4u + L->n_pus * (1u + L->max_cand);
    return (b + 15u) & ~15u;
}

/* ---------------------------------------------------------------------------
 * Picture-level job API (the performance boundary)
 * ------------------------------------------------------------------------- */
typedef struct svtme_ctx svtme_ctx;

/* Create a context on HIP device `device`. Sizes the plane cache lazily. */
svtme_status svtme_ctx_create(int device, svtme_ctx **out);
void svtme_ctx_destroy(svtme_ctx *ctx);

/* Upload one 8-bit luma picture (host memory, `stride` bytes per row,
 * width x height visible samples; width/height need not be multiples of 8:
 * the right/bottom are replicated to the next multiple of 8 as
 * svt_aom_pad_picture_to_multiple_of_min_blk_size_dimensions does). Builds the
 * padded full (pad 72), quarter (pad 32) and sixteenth (pad 16) planes on the
 * GPU (svt_aom_downsample_filtering_input_picture, pic_analysis_process.c:1945). */
svtme_status svtme_picture_upload(svtme_ctx *ctx, uint64_t picture_number, const uint8_t *y,
                                  uint32_t stride, uint32_t width, uint32_t height);
/* Same, for a 10-bit picture in uint16 samples (stride in samples): the
 * searched plane is the 8-bit MSB plane p >> 2 (enc_handle.c:4964-4972). */
svtme_status svtme_picture_upload_10bit(svtme_ctx *ctx, uint64_t picture_number, const uint16_t *y,
                                        uint32_t stride, uint32_t width, uint32_t height);
/* Asynchronous form of svtme_picture_upload: the pyramid is built on the
 * context's upload stream, overlapping with jobs already running. From
 * page-locked host memory (svtme_host_alloc, svtme_host_register, hipHostMalloc)
 * the build reads the plane itself over PCIe; from pageable memory the rows are
 * first copied by DMA into a device staging plane (SVTME_UPLOAD_ZERO_COPY=0:
 * always the DMA). The call returns once the work is queued (pageable memory:
 * once the driver has staged it). The first job that reads the picture waits
 * for the upload on the GPU. With pinned host memory the caller keeps `y`
 * unchanged until svtme_sync() or a job reading the picture has completed.
 * Jobs queued earlier that read an older version of the picture finish before
 * it is overwritten. */
svtme_status svtme_picture_upload_async(svtme_ctx *ctx, uint64_t picture_number, const uint8_t *y, uint32_t stride,
                                        uint32_t width, uint32_t height);
/* Asynchronous upload from PAGEABLE memory the library never page-locks (an
 * encoder's own picture buffers): the calling thread copies the w x h samples
 * into a page-locked staging buffer the library owns (a ring of
 * SVTME_UPLOAD_SLOTS, each reused once its DMA has run), outside the context
 * lock, then the DMA and the pyramid build are queued as in
 * svtme_picture_upload_async; `y` may change as soon as the call returns.
 * With more than SVTME_UPLOAD_SLOTS callers at once, a caller waits for a slot
 * (released as soon as its rows are staged and its DMA queued).
 * Page-locking the caller's memory instead (svtme_host_register) makes it a
 * driver user-pointer mapping, which the kernel may invalidate at any time
 * (NUMA balancing, page migration, compaction); every invalidation evicts the
 * process's GPU queues until the mapping is rebuilt -- a stall of the work in
 * flight. */
#define SVTME_UPLOAD_SLOTS 4
svtme_status svtme_picture_upload_copy_async(svtme_ctx *ctx, uint64_t picture_number, const uint8_t *y,
                                             uint32_t stride, uint32_t width, uint32_t height);
/* Same, from a DEVICE pointer already in HBM (no PCIe). */
svtme_status svtme_picture_upload_device(svtme_ctx *ctx, uint64_t picture_number, const uint8_t *d_y,
                                         uint32_t stride, uint32_t width, uint32_t height);
/* Asynchronous form of svtme_picture_upload_device (the input distribution of a
 * picture split over GPUs, SURVEY.md 8(e): the plane arrives in HBM by an RCCL
 * broadcast): the pyramid is built from d_y on the context's upload stream
 * (svtme_upload_stream) and the first job reading the picture waits for it on
 * the GPU. The caller makes the upload stream wait for d_y's producer before the
 * call and keeps d_y unchanged until the work queued on that stream has run. */
svtme_status svtme_picture_upload_device_async(svtme_ctx *ctx, uint64_t picture_number, const uint8_t *d_y,
                                               uint32_t stride, uint32_t width, uint32_t height);
/* The hipStream_t of the asynchronous uploads (created on first use). */
void *svtme_upload_stream(svtme_ctx *ctx);
svtme_status svtme_picture_release(svtme_ctx *ctx, uint64_t picture_number);
/* The resident picture's source planes were replaced (temporal filtering
 * re-decimates the filtered picture, temporal_filtering.c:3895-3931
 * pad_and_decimate_filtered_pic): rebuild its pyramid from the new 8-bit
 * plane. Ordered after every job already submitted on the context (those read
 * the old planes), before every later one. Fails if the picture is not
 * resident (a stale pyramid is never silently kept). */
svtme_status svtme_picture_invalidate(svtme_ctx *ctx, uint64_t picture_number, const uint8_t *y, uint32_t stride,
                                      uint32_t width, uint32_t height);
/* Copy a resident pyramid level back to host (level 0 = full, 1 = quarter,
 * 2 = sixteenth), padding included: dst gets (h + 2 pad) rows of `stride` bytes. */
svtme_status svtme_picture_download(svtme_ctx *ctx, uint64_t picture_number, int level, uint8_t *dst,
                                    uint32_t *stride, uint32_t *width, uint32_t *height, uint32_t *pad);

/* Resident chroma (8-bit, 4:2:0), for the chroma stage of temporal filtering
 * (svtme_tf_filter_yuv, svtme_tf_window_yuv). Attach the Cb and Cr planes of a
 * picture that is already resident: width x height is the LUMA source size the
 * picture was uploaded with, the planes hold (width + 1) >> 1 x (height + 1) >> 1
 * samples, rows `stride` bytes apart. They are padded by replication to W/2 x H/2
 * of the 8-aligned picture (svt_aom_pad_picture_to_multiple_of_min_blk_size_dimensions
 * on buffer_cb / buffer_cr, pic_analysis_process.c:1695-1711), then the margins
 * are replicated (svt_aom_generate_padding, temporal_filtering.c:3916-3927) to a
 * logical padding of SVTME_PAD_CHROMA.
 *
 * The padding is 40 where the reference's own is org_x >> 1 = 36: the chroma
 * predictor of temporal filtering reaches 39 samples beyond an edge
 * (clamp_mv_to_umv_border_sb with ss 1 and bw 32 lets a block start at -(4 + 32)
 * with a non-zero phase, and the 8 taps read 3 further). For an MV that points 36
 * or more chroma samples beyond an edge with a fractional phase the reference
 * reads up to 3 bytes of the neighbouring row; this library defines those reads
 * as replicated edge samples. TF-ME's search areas keep real MVs far from this.
 *
 * Synchronous, under the context lock; ordered after every job queued earlier on
 * any lane that reads the picture and before every later one. The chroma is
 * released with the picture; any later luma upload, svtme_picture_invalidate or
 * svtme_tf_window result under the same number drops it (a stale plane is never
 * silently kept). The luma calls never read it. Returns
 * SVTME_ERR_BAD_PARAMETER before any GPU work for a NULL ctx / cb / cr, a zero
 * size, a stride under the chroma width, a picture that is not resident or
 * whose aligned size is not that of width x height. */
#define SVTME_PAD_CHROMA 40
svtme_status svtme_picture_upload_chroma(svtme_ctx *ctx, uint64_t picture_number, const uint8_t *cb,
                                         const uint8_t *cr, uint32_t stride, uint32_t width, uint32_t height);
/* Copy a resident chroma plane (1 = Cb, 2 = Cr) back to host, padding included, in
 * the shape of svtme_picture_download: width x height are W/2 x H/2 of the aligned
 * picture, pad is SVTME_PAD_CHROMA, dst (NULL: sizes only) gets (height + 2 pad)
 * rows of stride = width + 2 pad bytes. Fails for a picture without chroma. */
svtme_status svtme_picture_download_chroma(svtme_ctx *ctx, uint64_t picture_number, int plane, uint8_t *dst,
                                           uint32_t *stride, uint32_t *width, uint32_t *height, uint32_t *pad);

/* Run ME for one picture. `ref_records` receives sb_count x R records and
 * `sb_results` (may be NULL) sb_count results, in host memory. Synchronous. */
svtme_status svtme_submit_picture(svtme_ctx *ctx, const svtme_job *job, svtme_ref_record *ref_records,
                                  svtme_sb_result *sb_results);

/* Asynchronous variant for pipelining / benchmarking: records stay in device
 * memory owned by ctx; svtme_sync waits, svtme_fetch copies them out. */
svtme_status svtme_submit_picture_async(svtme_ctx *ctx, const svtme_job *job);
svtme_status svtme_sync(svtme_ctx *ctx);
svtme_status svtme_fetch(svtme_ctx *ctx, svtme_ref_record *ref_records, svtme_sb_result *sb_results);
/* Asynchronous variant writing into caller-provided DEVICE buffers (e.g. the
 * slice of an all-gather tensor): sb_count x R records, and sb_count results
 * when d_sb_results is not NULL. */
svtme_status svtme_submit_picture_device(svtme_ctx *ctx, const svtme_job *job, svtme_ref_record *d_ref_records,
                                         svtme_sb_result *d_sb_results);
/* Run ME for a batch of n <= SVTME_MAX_BATCH_JOBS pictures (the ready
 * pictures of a mini-GOP, or this rank's SB band of n pictures) with ONE launch
 * of each stage kernel (jobs needing different kernel variants are launched
 * as separate groups). Job k writes its sb_count x R records to
 * d_ref_records[k] and, when d_sb_results is not NULL and d_sb_results[k] is
 * not NULL, its sb_count results to d_sb_results[k] (DEVICE buffers).
 * Asynchronous on the context's stream; the reference runs these pictures on
 * its ME threads concurrently (me_process.c:97-104). */
#define SVTME_MAX_BATCH_JOBS 16
svtme_status svtme_submit_batch_device(svtme_ctx *ctx, const svtme_job *jobs, uint32_t n,
                                       svtme_ref_record *const *d_ref_records, svtme_sb_result *const *d_sb_results);
/* The same on submission lane `lane` (0 .. SVTME_LANES-1): each lane has its own
 * stream (svtme_lane_stream; lane 0's is svtme_stream) and inter-stage
 * scratch, so batches on different lanes overlap on the GPU (the next batch's
 * workgroups fill the CUs while the previous one drains) the way the
 * reference's ME threads process pictures concurrently. Pictures are shared:
 * a lane waits for asynchronous uploads, and a re-upload or rebuild waits for
 * every lane's queued readers. Completion is signalled on the lane's stream. */
#define SVTME_LANES 2
svtme_status svtme_submit_batch_device_lane(svtme_ctx *ctx, uint32_t lane, const svtme_job *jobs, uint32_t n,
                                            svtme_ref_record *const *d_ref_records,
                                            svtme_sb_result *const *d_sb_results);
/* The hipStream_t of a lane (created on first use), NULL on a bad lane. */
void *svtme_lane_stream(svtme_ctx *ctx, uint32_t lane);

/* Asynchronous job with packed HOST output, for an encoder's ME threads (the
 * reference runs several pictures' ME at once, me_process.c:97-104). The job
 * runs on lane `lane` into device buffers the context keeps per ticket, is
 * packed on the device (svtme_pack_layout) and copied into host_out
 * (sb_count x svtme_packed_sb_bytes(layout, R) bytes) on the context's download
 * stream, overlapping later jobs. Returns at once with *ticket. host_out should
 * be page-locked (svtme_host_alloc): a pageable destination makes the copy
 * synchronous. At most SVTME_MAX_TICKETS tickets are outstanding (the
 * reference runs up to 25 ME threads and the TF threads beside them, one job in
 * flight each, enc_handle.c:744-773). A submission that finds every slot taken
 * waits for svtme_ticket_wait (another thread's) to retire one; it is refused
 * (SVTME_ERR_INSUFFICIENT_RESOURCES) only when no ticket is retired within
 * 100 ms while none is being waited on -- the caller holds them itself. */
#define SVTME_MAX_TICKETS 64
svtme_status svtme_submit_picture_packed_async(svtme_ctx *ctx, uint32_t lane, const svtme_job *job,
                                               const svtme_pack_layout *layout, void *host_out, uint64_t *ticket);
/* The same for n jobs (1 .. SVTME_MAX_BATCH_JOBS) in ONE batched launch: the
 * temporal filter's (central picture, reference) pairs of one window, all
 * known at its first ME call (temporal_filtering.c:3029-3030, 3096). Job k's
 * output goes to host_outs[k] under tickets[k]; each ticket is waited for and
 * retired on its own. */
svtme_status svtme_submit_pictures_packed_async(svtme_ctx *ctx, uint32_t lane, uint32_t n, const svtme_job *jobs,
                                                const svtme_pack_layout *layouts, void *const *host_outs,
                                                uint64_t *tickets);
/* Block until ticket's packed output is in host memory, then retire the ticket.
 * Safe to call from any thread, without holding anything the submitter holds. */
svtme_status svtme_ticket_wait(svtme_ctx *ctx, uint64_t ticket);
/* The same, and the job's GPU-side times (HIP events): from its turn on its
 * lane to its packed output on the device (waits for its pictures' uploads,
 * the search, the pack), and from there to the output in host memory (the
 * download stream's copy). Either pointer may be NULL. */
svtme_status svtme_ticket_wait_timed(svtme_ctx *ctx, uint64_t ticket, float *gpu_ms, float *copy_ms);
/* Page-locked host memory for packed outputs (NULL on failure), and its release. */
void *svtme_host_alloc(uint64_t bytes);
void svtme_host_free(void *p);
/* Page-lock an existing host range (e.g. an encoder's picture buffer) so that
 * svtme_picture_upload_async reads it from the GPU without staging it through
 * the CPU; svtme_host_unregister undoes it once the uploads reading it have run. */
svtme_status svtme_host_register(void *p, uint64_t bytes);
svtme_status svtme_host_unregister(void *p);
/* Size the device memory of later jobs ahead of them: every submission lane's
 * inter-stage scratch and the device buffers of the first `tickets` packed-job
 * slots, for jobs over pictures up to width x height with up to max_refs
 * reference slots and any pack layout, and for batches of up to
 * SVTME_MAX_BATCH_JOBS such pictures of one reference slot each (a TF window).
 * Submissions within those bounds then allocate nothing (a job beyond them
 * still grows the buffers it needs, after its lane's queued work has run). */
svtme_status svtme_reserve(svtme_ctx *ctx, uint32_t width, uint32_t height, uint32_t max_refs, uint32_t tickets);
/* Keep `count` picture buffers of a width x height picture (its three padded
 * planes) in the context's free pool, so that the uploads of up to that many
 * pictures beyond the resident ones allocate no device memory. Released
 * pictures' buffers return to the pool once the work reading them has run
 * (never hipFree on the steady path: it serialises the device). */
svtme_status svtme_reserve_pictures(svtme_ctx *ctx, uint32_t width, uint32_t height, uint32_t count);
/* Kernel timing with HIP events on the context's stream, recorded around every
 * stage launch of every submission while enabled (enable = 1). svtme_timing_read
 * waits for the recorded launch groups and returns the milliseconds of stage 0
 * (k_stage_a: zz / pre-HME / HME-L0, or the fused k_hme), 1 (k_stage_d: their
 * decisions), 2 (k_stage_b: HME-L1/L2), 3 (k_stage_c1, or the per-SB
 * k_stage_c) and 4 (k_stage_e) in stage_ms[0..4], each averaged over the
 * launch groups that ran that stage; returns the number of launch groups read
 * and clears them. At most 256 groups are kept between reads; later ones are
 * not recorded and the read sets svtme_last_error(). */
svtme_status svtme_set_timing(svtme_ctx *ctx, int enable);
uint32_t svtme_timing_read(svtme_ctx *ctx, float stage_ms[5]);
/* Kernel-path selection of a context, for diagnostics and A/B runs: each bit
 * forces a general path where a specialised kernel would apply (results are
 * identical). 0, the default, takes every specialised kernel that applies. A
 * context starts with the bits of the environment variables named below (read
 * once, at svtme_ctx_create); svtme_set_paths replaces them for the jobs
 * submitted after it. */
#define SVTME_PATH_NO_FUSED_HME 1u /* SVTME_NO_FUSED_HME: k_stage_a -> k_stage_d -> k_stage_b, not k_hme */
#define SVTME_PATH_NO_L1_FULL 2u   /* SVTME_NO_L1_FULL: full-SAD HME-L1 on k_stage_b, not k_l1_full */
#define SVTME_PATH_NO_L0_FULL 4u   /* SVTME_NO_L0_FULL: full-SAD stage A on k_stage_a, not k_l0_full */
#define SVTME_PATH_NO_FP_WIDE 8u   /* SVTME_NO_FP_WIDE: wide full-pel areas on k_stage_c1, not k_fp_wide */
#define SVTME_PATH_SPLIT_PASS 16u  /* SVTME_SPLIT_PASS: k_hme -> k_stage_c1 -> k_stage_e, not one k_hme */
#define SVTME_PATH_NO_A1_GATE 32u  /* SVTME_NO_A1_GATE: list-1 pre-HME searched with list 0 (no second A1 round) */
#define SVTME_PATH_HME_4WAVES 64u  /* SVTME_HME_4WAVES: k_hme workgroups of 4 wavefronts where svtme_hme_waves gives 3 */
svtme_status svtme_set_paths(svtme_ctx *ctx, uint32_t paths);
/* Device pointer of the last job's record buffer (for RCCL all-gather). */
void *svtme_device_records(svtme_ctx *ctx, uint64_t *bytes);
/* The HIP stream (hipStream_t) the context launches on, for event timing. */
void *svtme_stream(svtme_ctx *ctx);

/* ---------------------------------------------------------------------------
 * Dynamic-GOP detector: the early HME search of picture decision
 * (TASK_DG_DETECTOR_HME, me_process.c:327-333; dg_detector_hme_level0 and
 * early_hme, pd_process.c:393-634) as one job per picture pair. Per 64x64 SB
 * the 16x16 block of the current picture's sixteenth plane is searched
 * exhaustively (full SAD) over the search area on the reference picture's
 * sixteenth plane; the per-SB results give the frame metrics the detector
 * compares. Both pictures are resident (svtme_picture_upload*).
 * ------------------------------------------------------------------------- */
#define SVTME_DG_MAX_PAIRS 8
#define SVTME_DG_MAX_SA 128

typedef struct svtme_dg_pair {
    uint64_t cur_picture_number; /* the "src" picture of early_hme (pd_process.c:592-598) */
    uint64_t ref_picture_number;
} svtme_dg_pair;

typedef struct svtme_dg_sb { /* 8 bytes, one per SB in raster b64 order */
    uint32_t sad;            /* hme_level0_sad */
    int16_t mv_x, mv_y;      /* sr_center.col / .row, already x4 (pd_process.c:484-487) */
} svtme_dg_sb;

typedef struct svtme_dg_metrics { /* 32 bytes */
    uint64_t tot_dist;            /* DGDetectorMetrics, pcs.h:732-735 */
    uint32_t tot_cplx, tot_active;
    int32_t sum_in_vectors;
    int16_t mv_in_out_count;      /* PictureDecisionContext fields, pd_process.h:122-125, */
    uint8_t perc_cplx, perc_active;
    uint64_t norm_dist;           /* derived exactly as pd_process.c:630-633 */
} svtme_dg_metrics;

/* The reference's search area for an EbInputResolution: <= 360p 16x16,
 * <= 480p 64x64, else 128x128 (pd_process.c:497-498). */
void svtme_dg_search_area(int input_resolution, uint16_t *sa_width, uint16_t *sa_height);

/* Host only, no GPU: the frame metrics of a width x height picture from its
 * svtme_sb_total(width, height) per-SB results (pd_process.c:543-580, 630-633). */
void svtme_dg_reduce(uint32_t width, uint32_t height, const svtme_dg_sb *sb, svtme_dg_metrics *out);

/* The search of n pairs (1 .. SVTME_DG_MAX_PAIRS, all of one picture size: the
 * three pairs of one decision, pd_process.c:672-718) in one launch on lane 0's
 * stream. metrics receives n entries; sb_out is NULL or receives
 * n x svtme_sb_total(width, height) per-SB results (host memory). sa_width is
 * rounded up to a multiple of 8 as the reference does and, so rounded, is at
 * most SVTME_DG_MAX_SA, as is sa_height. The call waits for a pending
 * asynchronous upload of either picture on the GPU and is synchronous: it
 * returns when the outputs are written. */
svtme_status svtme_dg_detect(svtme_ctx *ctx, const svtme_dg_pair *pairs, uint32_t n, uint16_t sa_width,
                             uint16_t sa_height, svtme_dg_metrics *metrics, svtme_dg_sb *sb_out);

/* ---------------------------------------------------------------------------
 * Temporal filtering: the sub-pel refinement that follows the TF-ME call
 * (temporal_filtering.c:3177-3336, up to but not including the first
 * tf_64x64_inter_prediction / tf_32x32_inter_prediction) as one job per picture
 * window. Per (reference picture, 64x64 SB) the 64x64, 32x32, 16x16 and
 * optionally 8x8 blocks are refined from the full-pel winners of the TF-ME job
 * (SVTME_ME_MCTF, full records) by half, quarter and eighth-pel steps: AV1
 * interpolation of the reference block, variance against the centre picture.
 * 8-bit path only (8-bit input, or 10-bit input with tf_ctrls.use_8bit_subpel,
 * on the MSB plane the library holds).
 * ------------------------------------------------------------------------- */
/* The tf_ctrls / MeContext fields the stage reads (definitions.h:167-209,
 * me_context.h:496-497). The caller passes them; nothing is derived from a preset. */
typedef struct svtme_tf_subpel_controls {
    uint8_t half_pel_mode;          /* 0 off, 1 all 8 neighbours, 2 / 3 no diagonals (0..3) */
    uint8_t quarter_pel_mode;       /* the same (0..3) */
    uint8_t eight_pel_mode;         /* 0 off, 1 all 8 neighbours (0..1) */
    uint8_t use_2tap;               /* 64x64 and 32x32 blocks: 1 bilinear, 0 8-tap regular (0..1) */
    uint8_t sub_sampling_shift;     /* variance over every (1 << shift)-th row (0..1) */
    uint8_t enable_8x8_pred;        /* search the 8x8 blocks (0..1) */
    uint8_t use_pred_64x64_only_th; /* tf_use_64x64_pred threshold, 0 = off */
    uint8_t subpel_early_exit_th;   /* running-best early exit per pixel, 0 = off */
    uint64_t pred_error_32x32_th;   /* 32x32 error under which its 16x16 search is bypassed */
} svtme_tf_subpel_controls; /* 16 bytes */

/* svtme_tf_subpel_sb.branch */
#define SVTME_TFSP_64_ONLY 0   /* 64x64 only: use_pred_64x64_only_th (tf_use_64x64_pred) or the TF-ME early exit */
#define SVTME_TFSP_64_CHOSEN 1 /* 64x64 chosen after the 32x32 search (temporal_filtering.c:3265) */
#define SVTME_TFSP_32 2        /* the 32x32 path: 16x16 (8x8) searches and the split flags */

#define SVTME_TFSP_BLOCKS 85   /* 1 + 4 + 16 + 64 */
#define SVTME_TFSP_OFF_32 1    /* block index: idx_32x32 */
#define SVTME_TFSP_OFF_16 5    /* idx_32x32 * 4 + idx_16x16 */
#define SVTME_TFSP_OFF_8 21    /* idx_32x32 * 16 + 4 * idx_16x16 + idx_8x8 */
#define SVTME_TFSP_UNSET_ERROR 0x7FFFFFFFu /* INT_MAX: the reference's initial block error */

/* Per (reference, SB) result, the reference's own index orders (me_context.h:472-486).
 * Blocks the reference leaves unwritten on the branch taken hold MV 0 and error
 * INT_MAX. On the two 64x64 branches the 32x32 MVs are the 64x64 MV and the flags 0
 * (convert_64x64_info_to_32x32_info), the 32x32 errors INT_MAX (they belong to the
 * final prediction). Where 8x8 replaces 16x16 the 16x16 error is the 8x8 sum
 * (derive_tf_32x32_block_split_flag). */
typedef struct svtme_tf_subpel_sb {
    struct {
        int16_t x, y; /* 1/8 pel */
    } mv[SVTME_TFSP_BLOCKS];
    uint32_t error[SVTME_TFSP_BLOCKS];
    uint8_t split_32x32[4];    /* tf_32x32_block_split_flag */
    uint8_t split_16x16[4][4]; /* tf_16x16_block_split_flag */
    uint8_t branch;            /* SVTME_TFSP_* */
    uint8_t pad[3];
} svtme_tf_subpel_sb; /* 704 bytes */
#ifdef __cplusplus
static_assert(sizeof(svtme_tf_subpel_sb) == 704 && sizeof(svtme_tf_subpel_controls) == 16, "svtme_tf_subpel layout");
#else
_Static_assert(sizeof(svtme_tf_subpel_sb) == 704 && sizeof(svtme_tf_subpel_controls) == 16, "svtme_tf_subpel layout");
#endif

/* The refinement of n references (1 .. SVTME_MAX_BATCH_JOBS) of one window against
 * the centre picture, in one launch on lane 0's stream. All pictures are resident
 * and width x height (the aligned size of the TF-ME jobs). `records` holds
 * n x svtme_sb_total(width, height) records in host memory: slot 0 of each TF-ME
 * job in the order of ref_picture_numbers; `out` receives as many results.
 * Synchronous; returns SVTME_ERR_BAD_PARAMETER before any GPU work for a NULL
 * ctx / ref_picture_numbers / controls / records / out, n out of range, a control
 * above its range, a picture that is not resident or has another size. */
svtme_status svtme_tf_subpel(svtme_ctx *ctx, uint64_t centre_picture_number, const uint64_t *ref_picture_numbers,
                             uint32_t n, uint32_t width, uint32_t height, const svtme_tf_subpel_controls *controls,
                             const svtme_ref_record *records, svtme_tf_subpel_sb *out);

/* ---------------------------------------------------------------------------
 * Temporal filtering: the step after the sub-pel refinement
 * (temporal_filtering.c:3196-3390): the final inter prediction of every block
 * (MULTITAP_SHARP), the 32x32 errors of the 64x64 branches, the per-16x16
 * filter weights (svt_av1_apply_temporal_filter_planewise_medium_c, luma), the
 * accumulation over the window and the normalisation
 * (svt_aom_get_final_filtered_pixels_c). Luma, 8-bit,
 * tf_ctrls.use_zz_based_filter == 0.
 * ------------------------------------------------------------------------- */
typedef struct svtme_tf_filter_controls {
    uint32_t tf_decay_factor_fp16; /* MeContext.tf_decay_factor_fp16[C_Y], any value */
    uint16_t tf_mv_dist_th;        /* MeContext.tf_mv_dist_th, 0..32767 (the reference sets 64..450) */
    uint8_t sub_sampling_shift;    /* tf_ctrls.sub_sampling_shift, 0..1 */
    uint8_t pad;
} svtme_tf_filter_controls; /* 8 bytes */
#ifdef __cplusplus
static_assert(sizeof(svtme_tf_filter_controls) == 8, "svtme_tf_filter layout");
#else
_Static_assert(sizeof(svtme_tf_filter_controls) == 8, "svtme_tf_filter layout");
#endif

/* The filtered luma of the centre picture from n references (1 ..
 * SVTME_MAX_BATCH_JOBS, the references the caller kept) of one window, on lane 0's
 * stream. All pictures are resident and width x height (the aligned size the other
 * TF calls take). `subpel` holds n x svtme_sb_total(width, height) results of
 * svtme_tf_subpel in host memory, in the order of ref_picture_numbers. `out`
 * receives every pixel x < width, y < height of what
 * svt_aom_get_final_filtered_pixels_c leaves in the centre picture, rows out_stride
 * bytes apart; bytes at x >= width are not written. `err32_out` is NULL or receives
 * n x SBs x 4 values: the 32x32 block error the reference holds when it filters
 * that quadrant (64x64 branches: convert_64x64_info_to_32x32_info's variance of the
 * final prediction; SVTME_TFSP_32: the sub-pel stage's error). The resident centre
 * picture is not modified. Synchronous; returns SVTME_ERR_BAD_PARAMETER before any
 * GPU work for a NULL ctx / ref_picture_numbers / controls / subpel / out, n out of
 * range, out_stride < width, a control above its range, a subpel[..].branch above
 * 2, a picture that is not resident or has another size. */
svtme_status svtme_tf_filter(svtme_ctx *ctx, uint64_t centre_picture_number, const uint64_t *ref_picture_numbers,
                             uint32_t n, uint32_t width, uint32_t height, const svtme_tf_filter_controls *controls,
                             const svtme_tf_subpel_sb *subpel, uint8_t *out, uint32_t out_stride,
                             uint32_t *err32_out);

/* ---------------------------------------------------------------------------
 * Temporal filtering: one window in one call, resident to resident. The
 * window's TF-ME jobs, svtme_tf_subpel and svtme_tf_filter chained on lane 0's
 * stream through device memory, and the filtered luma left as a resident
 * picture (what pad_and_decimate_filtered_pic leaves in the encoder,
 * temporal_filtering.c:3895-3934). Nothing crosses to the host unless asked for.
 * ------------------------------------------------------------------------- */
/* Host copies of the window's results; every pointer may be NULL. */
typedef struct svtme_tf_window_out {
    uint8_t *plane;            /* filtered luma, x < src_width, y < src_height, after the re-pad */
    uint32_t plane_stride;     /* bytes between its rows, >= src_width; bytes at x >= src_width are not written */
    uint32_t pad;
    svtme_ref_record *records; /* n x SBs: slot 0 of each TF-ME job (what svtme_tf_subpel takes) */
    svtme_tf_subpel_sb *subpel; /* n x SBs: what svtme_tf_subpel returns */
    uint32_t *err32;           /* n x SBs x 4: what svtme_tf_filter returns */
} svtme_tf_window_out;         /* 40 bytes */
#ifdef __cplusplus
static_assert(sizeof(svtme_tf_window_out) == 40, "svtme_tf_window layout");
#else
_Static_assert(sizeof(svtme_tf_window_out) == 40, "svtme_tf_window layout");
#endif

/* `jobs` are the window's n TF-ME jobs (1 .. SVTME_MAX_BATCH_JOBS) as
 * svtme_submit_pictures_packed_async takes them: me_type SVTME_ME_MCTF, one list
 * with one reference (job k's is ref_picture_number[0][0]), all with the same
 * picture_number (the centre) and the same width x height, each over the whole
 * picture (sb_begin 0, sb_count 0 or every SB). src_width x src_height is the size
 * the centre picture was uploaded with; aligned to 8 it is the jobs' size.
 *
 * The jobs run as one batch and write their records where the sub-pel stage reads
 * them; its results stay where the filter reads them; the normalisation writes
 * level 0 of the picture out_picture_number (the window's aligned size). There the
 * samples at x >= src_width or y >= src_height are re-padded from the last true
 * column and row, the margins written and levels 1 and 2 decimated, as an upload of
 * the src_width x src_height filtered plane would leave them. out_picture_number
 * may be the centre's number: the picture is replaced in place, after work queued
 * earlier on any lane that reads it. It may not be one of the references. Any other
 * number leaves the centre picture as it was. Later jobs on any lane that read the
 * result picture are ordered after the window on the GPU.
 *
 * With `out` NULL or every pointer of it NULL the call returns once the work is
 * queued (svtme_sync, or any later synchronous call on the context, covers it);
 * otherwise it returns when the requested copies are written.
 *
 * Returns SVTME_ERR_BAD_PARAMETER before any GPU work for a NULL ctx / jobs /
 * controls, n out of range, a job that is not SVTME_ME_MCTF, has more than one
 * reference, another centre, another size or covers part of the picture, src_* that
 * do not align to the jobs' size, plane set with plane_stride < src_width, a control
 * above the ranges of svtme_tf_subpel / svtme_tf_filter, a picture that is not
 * resident or has another size, out_picture_number among the references. */
svtme_status svtme_tf_window(svtme_ctx *ctx, const svtme_job *jobs, uint32_t n, uint32_t src_width,
                             uint32_t src_height, const svtme_tf_subpel_controls *subpel_controls,
                             const svtme_tf_filter_controls *filter_controls, uint64_t out_picture_number,
                             const svtme_tf_window_out *out);

/* ---------------------------------------------------------------------------
 * Temporal filtering with chroma (tf_chroma set: TF levels 1..5, presets M0..M7;
 * enc_handle.c tf_controls). 8-bit, 4:2:0, use_zz_based_filter == 0. Every
 * picture of the window carries resident chroma (svtme_picture_upload_chroma).
 * The chroma stage predicts, for every luma block of size b at (px, py) with MV
 * mv, a b/2 x b/2 block of Cb and of Cr at (px / 2, py / 2) at the same MV read
 * as 1/16 chroma pel (svt_aom_inter_prediction's chroma part,
 * enc_inter_prediction.c:4248-4360; the 4x4 blocks with the 4-tap
 * sub_pel_filters_4), and weights them per 8x8 quarter of each 16x16 chroma
 * block (svt_av1_apply_temporal_filter_planewise_medium_partial_c, is_chroma 1:
 * the luma MVs and block errors, (5 x chroma window error + luma window error) /
 * 6, the plane's own decay factor). Reads beyond a chroma plane see replicated
 * edge samples (see svtme_picture_upload_chroma: a deviation from the reference
 * for MVs 36 or more chroma samples beyond an edge).
 * ------------------------------------------------------------------------- */
typedef struct svtme_tf_filter_yuv_controls {
    svtme_tf_filter_controls luma;    /* as svtme_tf_filter takes them */
    uint32_t tf_decay_factor_cb_fp16; /* MeContext.tf_decay_factor_fp16[C_U], any value */
    uint32_t tf_decay_factor_cr_fp16; /* MeContext.tf_decay_factor_fp16[C_V], any value */
} svtme_tf_filter_yuv_controls;       /* 16 bytes */

typedef struct svtme_tf_filter_yuv_out {
    uint8_t *y;         /* filtered luma, x < width, y < height (required) */
    uint8_t *cb;        /* filtered Cb, x < (width + 1) >> 1, y < (height + 1) >> 1; may be NULL */
    uint8_t *cr;        /* filtered Cr, likewise; may be NULL */
    uint32_t y_stride;  /* bytes between rows, >= width; bytes beyond the plane's width are not written */
    uint32_t cb_stride; /* >= (width + 1) >> 1 when cb is set */
    uint32_t cr_stride; /* >= (width + 1) >> 1 when cr is set */
    uint32_t pad;
    uint32_t *err32;    /* NULL or n x SBs x 4, as svtme_tf_filter's err32_out */
} svtme_tf_filter_yuv_out; /* 48 bytes */

/* Host copies of a window's filtered chroma; every pointer may be NULL. */
typedef struct svtme_tf_window_yuv_out {
    uint8_t *cb;        /* x < (src_width + 1) >> 1, y < (src_height + 1) >> 1 */
    uint8_t *cr;
    uint32_t cb_stride; /* >= (src_width + 1) >> 1 when cb is set */
    uint32_t cr_stride;
} svtme_tf_window_yuv_out; /* 24 bytes */
#ifdef __cplusplus
static_assert(sizeof(svtme_tf_filter_yuv_controls) == 16 && sizeof(svtme_tf_filter_yuv_out) == 48 &&
                  sizeof(svtme_tf_window_yuv_out) == 24, "svtme_tf_*_yuv layout");
#else
_Static_assert(sizeof(svtme_tf_filter_yuv_controls) == 16 && sizeof(svtme_tf_filter_yuv_out) == 48 &&
                   sizeof(svtme_tf_window_yuv_out) == 24, "svtme_tf_*_yuv layout");
#endif

/* svtme_tf_filter with the chroma stage: the same arguments, the controls with
 * the two chroma decay factors and the outputs in a struct. out->y and
 * out->err32 receive byte for byte what svtme_tf_filter writes; out->cb and
 * out->cr what svt_aom_get_final_filtered_pixels_c leaves in the centre
 * picture's chroma. No resident picture is modified. Synchronous. Errors: those
 * of svtme_tf_filter (out, out->y in the place of its out), and before any GPU
 * work too a chroma stride under the chroma width and a picture of the window
 * without chroma. */
svtme_status svtme_tf_filter_yuv(svtme_ctx *ctx, uint64_t centre_picture_number, const uint64_t *ref_picture_numbers,
                                 uint32_t n, uint32_t width, uint32_t height,
                                 const svtme_tf_filter_yuv_controls *controls, const svtme_tf_subpel_sb *subpel,
                                 const svtme_tf_filter_yuv_out *out);

/* svtme_tf_window with the chroma stage chained on lane 0's stream after the luma
 * prediction. The result picture also gets chroma planes: the filtered samples
 * inside the true chroma size, re-padded beyond it with the margins, as
 * svtme_picture_upload_chroma of the filtered planes would leave them. In place
 * (out_picture_number the centre's) the centre's chroma is replaced too. `out` is
 * svtme_tf_window's, `out_uv` (NULL or every pointer NULL: nothing copied) asks
 * for the chroma host copies. The luma side, the ordering guarantees and the
 * refusals are svtme_tf_window's; refused too, before any GPU work, are a chroma
 * stride under the chroma width and a picture of the window without chroma. */
svtme_status svtme_tf_window_yuv(svtme_ctx *ctx, const svtme_job *jobs, uint32_t n, uint32_t src_width,
                                 uint32_t src_height, const svtme_tf_subpel_controls *subpel_controls,
                                 const svtme_tf_filter_yuv_controls *filter_controls, uint64_t out_picture_number,
                                 const svtme_tf_window_out *out, const svtme_tf_window_yuv_out *out_uv);

/* ---------------------------------------------------------------------------
 * Temporal filtering of 10-bit luma (is_highbd in temporal_filtering.c). The
 * TF-ME search and the sub-pel refinement of a 10-bit picture run on its MSB plane
 * (svtme_picture_upload_10bit; every level of tf_controls sets use_8bit_subpel), so
 * svtme_tf_subpel serves them as it is. What follows reads the full-precision
 * pictures: the final MULTITAP_SHARP prediction (svt_highbd_inter_predictor, bd
 * 10), the 32x32 errors of the 64x64 branches (svt_aom_highbd_10_variance32x32_c /
 * 32x16_c), the weights (svt_av1_apply_temporal_filter_planewise_medium_hbd_c: the
 * 8-bit function with the window SSE >> 4, the 16x16 block error >> 4 and the
 * 32x32 block error >> 6 instead of >> 2), the accumulation and the normalisation
 * into 16-bit samples. Luma, 10 bit, use_zz_based_filter == 0, use_8bit_subpel ==
 * 1; chroma beside it in the section after this one. Not served: the
 * high-bit-depth sub-pel search (use_8bit_subpel == 0), the zz filter, 12 bit.
 * ------------------------------------------------------------------------- */
/* Attach the full-precision luma (16-bit samples, values 0..1023, rows `stride`
 * SAMPLES apart) to a picture that is already resident, normally one uploaded with
 * svtme_picture_upload_10bit from the same samples: keeping the MSB plane p >> 2
 * consistent with it is the caller's duty. width x height is the size the luma was
 * uploaded with. The plane is a buffer of its own, replicated to the 8-aligned size
 * and by SVTME_PAD_FULL on every side, which is what svt_aom_pack_highbd_pic makes
 * of the reference's padded 8-bit and 2-bit planes. Synchronous, ordered after
 * queued readers of the picture; released with the picture; any later luma upload,
 * svtme_picture_invalidate, svtme_tf_window or svtme_tf_window_yuv result under the
 * same number drops it. The 8-bit calls and the 8-bit yuv calls never read it. Samples
 * above 1023 are the caller's error: the results of the 10-bit calls are then
 * unspecified, but no read or write leaves the buffers. Returns
 * SVTME_ERR_BAD_PARAMETER before any GPU work for a NULL ctx / y, a zero size,
 * stride < width, a picture that is not resident or of another aligned size. */
svtme_status svtme_picture_attach_10bit(svtme_ctx *ctx, uint64_t picture_number, const uint16_t *y, uint32_t stride,
                                        uint32_t width, uint32_t height);
/* Copy the padded 16-bit plane back in the shape of svtme_picture_download for
 * level 0: (height + 2 pad) rows of (width + 2 pad) samples, *stride in samples;
 * dst NULL asks for the sizes alone. SVTME_ERR_BAD_PARAMETER for a NULL ctx, a
 * picture that is not resident or has no 10-bit plane. */
svtme_status svtme_picture_download_10bit(svtme_ctx *ctx, uint64_t picture_number, uint16_t *dst, uint32_t *stride,
                                          uint32_t *width, uint32_t *height, uint32_t *pad);

/* svtme_tf_filter on the attached 16-bit planes: the same arguments, `subpel` what
 * svtme_tf_subpel returned on the MSB planes, `out` 16-bit samples with out_stride
 * in samples, err32_out NULL or the 32x32 errors (64x64 branches: the 10-bit
 * variance). No resident picture is modified. Synchronous. Refusals: those of
 * svtme_tf_filter, and a picture of the window without an attached 10-bit plane. */
svtme_status svtme_tf_filter_10bit(svtme_ctx *ctx, uint64_t centre_picture_number, const uint64_t *ref_picture_numbers,
                                   uint32_t n, uint32_t width, uint32_t height,
                                   const svtme_tf_filter_controls *controls, const svtme_tf_subpel_sb *subpel,
                                   uint16_t *out, uint32_t out_stride, uint32_t *err32_out);

/* svtme_tf_window for 10-bit pictures: the TF-ME batch and the sub-pel refinement on
 * the MSB planes, then the 10-bit prediction, weighting and normalisation, chained on
 * lane 0's stream through device memory. The result picture gets both planes: the
 * filtered 16-bit plane inside the aligned size, re-padded beyond src_width x
 * src_height with the margins written, as svtme_picture_attach_10bit of the filtered
 * plane would leave it; and level 0 = filtered >> 2 (what svt_unpack_and_2bcompress
 * writes as the 8-bit plane) with its re-pad, margins and levels 1 and 2 made as
 * svtme_tf_window makes them: the picture is what svtme_picture_upload_10bit plus
 * svtme_picture_attach_10bit of the filtered plane leave. Chroma attached to the
 * result's number, 8-bit or 16-bit, is dropped. out->plane receives the MSB plane; plane16 (NULL or
 * rows plane16_stride SAMPLES apart, >= src_width) the 16-bit plane. In place, a
 * fresh number, the ordering guarantees, the asynchronous return when no host copy
 * is asked for and the refusals are svtme_tf_window's; refused too, before any GPU
 * work, are plane16 set with plane16_stride < src_width and a picture of the window
 * without an attached 10-bit plane. */
svtme_status svtme_tf_window_10bit(svtme_ctx *ctx, const svtme_job *jobs, uint32_t n, uint32_t src_width,
                                   uint32_t src_height, const svtme_tf_subpel_controls *subpel_controls,
                                   const svtme_tf_filter_controls *filter_controls, uint64_t out_picture_number,
                                   const svtme_tf_window_out *out, uint16_t *plane16, uint32_t plane16_stride);

/* ---------------------------------------------------------------------------
 * Temporal filtering of 10-bit pictures with chroma (is_highbd and tf_chroma: every
 * level of tf_controls from 1 to 7 sets chroma_lvl 1 for at least one picture type,
 * so presets M0 to M7 filter Cb and Cr beside luma on the packed 16-bit pictures).
 * 10 bit, 4:2:0, use_zz_based_filter == 0, use_8bit_subpel == 1. The chroma stage is
 * svtme_tf_filter_yuv's on 16-bit samples: the luma blocks and MVs, the chroma clamp,
 * svt_highbd_inter_predictor at bd 10 with MULTITAP_SHARP at the chroma size
 * (sub_pel_filters_4 for the 4x4 blocks), and the weights of
 * svt_av1_apply_temporal_filter_planewise_medium_hbd_partial_c with is_chroma 1: the
 * 8x8 quarter's SSE >> 4, times 4, blended 5 : 1 with the luma window error (the 16x16
 * SSE >> 4) of the same quarter, the luma block errors >> 4 (split) or >> 6, the
 * plane's own decay factor. With the 8-bit calls, the yuv calls and the 10-bit luma
 * calls this completes {8, 10 bit} x {luma, yuv}. Not served: use_8bit_subpel == 0,
 * the zz filter, 12 bit.
 * ------------------------------------------------------------------------- */
/* Attach the full-precision Cb and Cr (16-bit samples, values 0..1023, rows `stride`
 * SAMPLES apart in both planes) to a resident picture. width x height is the LUMA size
 * the picture was uploaded with; each plane holds (width + 1) >> 1 by (height + 1) >> 1
 * samples. They are kept in a buffer of their own, replicated to W/2 x H/2 of the
 * 8-aligned picture and by SVTME_PAD_CHROMA (40) on every side: the padding, and the
 * deviation from the reference's 36, of svtme_picture_upload_chroma. Inside those 36
 * the planes are what svt_aom_pack_highbd_pic makes of the reference's padded 8-bit
 * and 2-bit chroma planes: pad_2b_compressed_input_picture and
 * svt_aom_generate_padding_compressed_10bit repeat the edge sample's two bits where
 * pad_input_picture and svt_aom_generate_padding repeat its eight. Synchronous,
 * ordered after queued readers of the picture; released with the picture; dropped by
 * whatever drops the 16-bit luma plane (a later luma upload, svtme_picture_invalidate,
 * a svtme_tf_window or svtme_tf_window_yuv result under the number) and by a
 * svtme_tf_window_10bit result under the number. svtme_picture_attach_10bit and this
 * call may come in either order after the luma upload. Only the two calls below read
 * the planes. Returns SVTME_ERR_BAD_PARAMETER before any GPU work for a NULL ctx / cb /
 * cr, a zero size, a stride under the chroma width, a picture that is not resident or
 * of another aligned size. */
svtme_status svtme_picture_attach_chroma_10bit(svtme_ctx *ctx, uint64_t picture_number, const uint16_t *cb,
                                               const uint16_t *cr, uint32_t stride, uint32_t width, uint32_t height);
/* Copy a resident 16-bit chroma plane (1 = Cb, 2 = Cr) back in the shape of
 * svtme_picture_download_chroma, in 16-bit samples: width x height are W/2 x H/2, pad
 * SVTME_PAD_CHROMA, *stride = width + 2 pad in samples; dst NULL asks for the sizes
 * alone. Fails for a picture without 16-bit chroma. */
svtme_status svtme_picture_download_chroma_10bit(svtme_ctx *ctx, uint64_t picture_number, int plane, uint16_t *dst,
                                                 uint32_t *stride, uint32_t *width, uint32_t *height, uint32_t *pad);

/* The 16-bit form of svtme_tf_filter_yuv_out: strides in SAMPLES. */
typedef struct svtme_tf_filter_yuv16_out {
    uint16_t *y;        /* [height] rows of y_stride samples */
    uint16_t *cb;       /* NULL, or [(height + 1) >> 1] rows of cb_stride samples, (width + 1) >> 1 written */
    uint16_t *cr;       /* likewise */
    uint32_t y_stride;  /* >= width */
    uint32_t cb_stride; /* >= (width + 1) >> 1 where cb is set */
    uint32_t cr_stride;
    uint32_t pad;
    uint32_t *err32;    /* NULL, or [n][SBs][4] as svtme_tf_filter_10bit's err32_out */
} svtme_tf_filter_yuv16_out; /* 48 bytes */

/* Host copies of a 10-bit window's filtered chroma; every pointer may be NULL. Strides in SAMPLES. */
typedef struct svtme_tf_window_yuv16_out {
    uint16_t *cb; /* [(src_height + 1) >> 1] rows of cb_stride samples */
    uint16_t *cr;
    uint32_t cb_stride;
    uint32_t cr_stride;
} svtme_tf_window_yuv16_out; /* 24 bytes */
#ifdef __cplusplus
static_assert(sizeof(svtme_tf_filter_yuv16_out) == 48 && sizeof(svtme_tf_window_yuv16_out) == 24,
              "svtme_tf_*_yuv16 layout");
#else
_Static_assert(sizeof(svtme_tf_filter_yuv16_out) == 48 && sizeof(svtme_tf_window_yuv16_out) == 24,
               "svtme_tf_*_yuv16 layout");
#endif

/* svtme_tf_filter_10bit with the chroma stage: the same arguments, the controls of
 * svtme_tf_filter_yuv (the luma controls and the two chroma decay factors) and the
 * outputs in a struct. out->y and out->err32 are byte for byte what
 * svtme_tf_filter_10bit writes; out->cb and out->cr (either may be NULL) receive the
 * filtered chroma at the true chroma size. Every picture of the window carries the
 * 16-bit luma plane and the 16-bit chroma planes. No resident picture is modified.
 * Synchronous. Refusals: those of svtme_tf_filter_10bit, and before any GPU work a
 * chroma stride under the chroma width and a picture of the window without 16-bit
 * chroma. */
svtme_status svtme_tf_filter_yuv_10bit(svtme_ctx *ctx, uint64_t centre_picture_number,
                                       const uint64_t *ref_picture_numbers, uint32_t n, uint32_t width,
                                       uint32_t height, const svtme_tf_filter_yuv_controls *controls,
                                       const svtme_tf_subpel_sb *subpel, const svtme_tf_filter_yuv16_out *out);

/* svtme_tf_window_10bit with the chroma stage chained on lane 0's stream after the
 * luma prediction. The result picture is what svtme_picture_upload_10bit +
 * svtme_picture_attach_10bit + svtme_picture_attach_chroma_10bit of the filtered
 * planes would leave: the chroma re-padded beyond the true chroma size and its margins
 * too. In place (out_picture_number the centre's) all planes of the centre are
 * replaced. 8-bit chroma under the result's number is dropped. `out`, plane16 and
 * plane16_stride are svtme_tf_window_10bit's; out_uv may be NULL. The ordering
 * guarantees, the asynchronous return when no host copy is asked for and the refusals
 * are svtme_tf_window_10bit's; refused too, before any GPU work, are a chroma stride
 * under the chroma width and a picture of the window without the 16-bit luma plane or
 * without the 16-bit chroma planes. */
svtme_status svtme_tf_window_yuv_10bit(svtme_ctx *ctx, const svtme_job *jobs, uint32_t n, uint32_t src_width,
                                       uint32_t src_height, const svtme_tf_subpel_controls *subpel_controls,
                                       const svtme_tf_filter_yuv_controls *filter_controls, uint64_t out_picture_number,
                                       const svtme_tf_window_out *out, uint16_t *plane16, uint32_t plane16_stride,
                                       const svtme_tf_window_yuv16_out *out_uv);

/* ---------------------------------------------------------------------------
 * Low-delay temporal filtering: produce_temporally_filtered_pic_ld
 * (temporal_filtering.c:3404-3816), what svt_av1_init_temporal_filtering runs with
 * SVT_AV1_PRED_LOW_DELAY_B. No TF-ME and no sub-pel search: the prediction of every
 * 64x64 block is the co-located block of the reference picture (MV (0, 0)), its
 * 32x32 luma errors are VARIANCES (svt_aom_variance32x32_c / 32x16_c, at 10 bit
 * svt_aom_highbd_10_variance*), and the weights are those of
 * svt_av1_apply_zz_based_temporal_filter_planewise_medium[_hbd]_c: per 32x32 luma
 * block and plane, (exp_tab[min(((var32 >> 2 (10 bit: >> 6)) << 2) /
 * max(decay_fp16 >> 10, 1), 112)] * 1000) >> 17, 500 at the most, the chroma planes
 * with the luma variance and their own decay factor. One fused kernel
 * (svtme_tfld.hip) serves 8 and 10 bit, with and without 4:2:0 chroma.
 * ------------------------------------------------------------------------- */
typedef struct svtme_tf_ld_controls {
    uint32_t tf_decay_factor_fp16[3]; /* MeContext.tf_decay_factor_fp16[C_Y / C_U / C_V], any value; [1], [2] ignored without chroma */
    uint8_t sub_sampling_shift;       /* 0..1 */
    uint8_t bit_depth;                /* 8 or 10 */
    uint8_t chroma;                   /* 0: luma only; 1: tf_chroma, 4:2:0 */
    uint8_t pad;                      /* 0 */
} svtme_tf_ld_controls;               /* 16 bytes */

typedef struct svtme_tf_ld_out {
    void *y, *cb, *cr;                       /* uint8_t samples at 8 bit, uint16_t at 10 */
    uint32_t y_stride, cb_stride, cr_stride; /* in samples */
    uint32_t pad;
    uint32_t *var32; /* NULL or n x SBs x 4: the 32x32 variances, SB raster order, quadrant = col + 2 * row */
} svtme_tf_ld_out;   /* 48 bytes */
#ifdef __cplusplus
static_assert(sizeof(svtme_tf_ld_controls) == 16 && sizeof(svtme_tf_ld_out) == 48, "svtme_tf_ld layout");
#else
_Static_assert(sizeof(svtme_tf_ld_controls) == 16 && sizeof(svtme_tf_ld_out) == 48, "svtme_tf_ld layout");
#endif

/* The low-delay filter of one window of resident pictures into host memory: the
 * counterpart of svtme_tf_filter / _yuv / _10bit / _yuv_10bit by controls->bit_depth
 * and controls->chroma. width x height is the 8-aligned size the other TF calls
 * take. At 8 bit the call reads level 0 of each picture and, with chroma, its
 * attached 8-bit chroma; at 10 bit the attached 16-bit plane and, with chroma, the
 * attached 16-bit chroma. out->y (required) receives x < width, y < height; out->cb
 * and out->cr (optional, honoured only with chroma) the (width + 1) >> 1 by
 * (height + 1) >> 1 chroma planes; out->var32 (optional) the variances. Synchronous;
 * no resident picture is modified. Returns SVTME_ERR_BAD_PARAMETER before any GPU
 * work for a NULL ctx / refs / controls / out / out->y, n outside
 * 1..SVTME_MAX_BATCH_JOBS, a size that is not a non-zero multiple of 8 up to 16384,
 * bit_depth not 8 or 10, chroma or sub_sampling_shift above 1, pad not 0, a stride
 * under its plane's width, the centre among the references, and a picture that is
 * not resident, has another size or lacks a plane the mode reads. */
svtme_status svtme_tf_filter_ld(svtme_ctx *ctx, uint64_t centre_picture_number, const uint64_t *ref_picture_numbers,
                                uint32_t n, uint32_t width, uint32_t height, const svtme_tf_ld_controls *controls,
                                const svtme_tf_ld_out *out);

/* The same window resident to resident: the counterpart of svtme_tf_window / _yuv /
 * _10bit / _yuv_10bit, with no jobs (nothing is searched). src_width x src_height is
 * the true size; the call aligns it to 8. The result picture out_picture_number is
 * what the matching window call leaves by bit_depth and chroma: the filtered planes
 * re-padded beyond the true size with their margins, levels 1 and 2 rebuilt, at 10
 * bit level 0 = the 16-bit plane >> 2, and the attached planes of an older picture
 * under that number kept or dropped as that call does. out_picture_number may be the
 * centre's (in place) and may not be a reference's. `out` may be NULL; with no host
 * copy asked for (NULL, or y, cb, cr and var32 all NULL) the call returns once the
 * work is queued, and later readers of the result are ordered behind it on every
 * lane. The host copies have the true size (chroma (src_width + 1) >> 1). Refusals:
 * those of svtme_tf_filter_ld with a zero or oversized source size in place of the
 * size rule, and the result number among the references; a refused call changes no
 * picture. */
svtme_status svtme_tf_window_ld(svtme_ctx *ctx, uint64_t centre_picture_number, const uint64_t *ref_picture_numbers,
                                uint32_t n, uint32_t src_width, uint32_t src_height,
                                const svtme_tf_ld_controls *controls, uint64_t out_picture_number,
                                const svtme_tf_ld_out *out);

/* Number of 64x64 SBs of a width x height picture, and R for a job. */
uint32_t svtme_sb_total(uint32_t width, uint32_t height);
uint32_t svtme_job_ref_slots(const svtme_job *job);

/* Last error message of this thread (empty string if none). */
const char *svtme_last_error(void);

/* Fill `ctrl` as svt_aom_sig_deriv_me does for the non-RTC, non-screen-content
 * path (enc_mode_config.c:671-808) for preset `enc_mode`, qp and resolution. */
void svtme_derive_controls(int enc_mode, int qp, int input_resolution, int temporal_layer_index,
                           int hierarchical_levels, int frame_rate_q16, svtme_controls *ctrl);

/* Fill `ctrl` as the reference does for one temporal-filtering ME job
 * (me_type SVTME_ME_MCTF): svt_aom_sig_deriv_me_tf (enc_mode_config.c:814-854)
 * for tf_ctrls.hme_me_level 0..4 and tf_ctrls.qp_opt, the tf HME enables
 * (:1620-1645) and set_hme_search_params_mctf(ctx, 0) (temporal_filtering.c:2759). */
void svtme_derive_controls_tf(int hme_me_level, int qp_opt, int qp, int input_resolution, svtme_controls *ctrl);

/* ---------------------------------------------------------------------------
 * Per-kernel rtcd variants. Signatures identical to the pointers declared in
 * the reference's Source/Lib/Codec/aom_dsp_rtcd.h (line cited per entry).
 * ------------------------------------------------------------------------- */
/* The variants are reentrant (per-thread HIP stream and scratch). They never
 * return an error: on a HIP failure they leave their outputs untouched, set
 * svtme_last_error() and raise the calling thread's failure flag, which
 * svtme_rtcd_failed() returns (1) and clears, so the caller can re-run the call
 * on the variant it replaced (integration/svtme_svt_glue.c). */
int svtme_rtcd_failed(void);

/* aom_dsp_rtcd.h:779 svt_sad_loop_kernel */
void svt_sad_loop_kernel_hip(uint8_t *src, uint32_t src_stride, uint8_t *ref, uint32_t ref_stride,
                             uint32_t block_height, uint32_t block_width, uint64_t *best_sad,
                             int16_t *x_search_center, int16_t *y_search_center, uint32_t src_stride_raw,
                             uint8_t skip_search_line, int16_t search_area_width, int16_t search_area_height);
/* aom_dsp_rtcd.h:856 svt_nxm_sad_kernel */
uint32_t svt_nxm_sad_kernel_hip(const uint8_t *src, uint32_t src_stride, const uint8_t *ref, uint32_t ref_stride,
                                uint32_t height, uint32_t width);
/* aom_dsp_rtcd.h:842 svt_ext_sad_calculation_8x8_16x16 */
void svt_ext_sad_calculation_8x8_16x16_hip(uint8_t *src, uint32_t src_stride, uint8_t *ref, uint32_t ref_stride,
                                           uint32_t *p_best_sad_8x8, uint32_t *p_best_sad_16x16,
                                           uint32_t *p_best_mv8x8, uint32_t *p_best_mv16x16, uint32_t mv,
                                           uint32_t *p_sad16x16, uint32_t *p_sad8x8, bool sub_sad);
/* aom_dsp_rtcd.h:848 svt_ext_sad_calculation_32x32_64x64 */
void svt_ext_sad_calculation_32x32_64x64_hip(uint32_t *p_sad16x16, uint32_t *p_best_sad_32x32,
                                             uint32_t *p_best_sad_64x64, uint32_t *p_best_mv32x32,
                                             uint32_t *p_best_mv64x64, uint32_t mv, uint32_t *p_sad32x32);
/* aom_dsp_rtcd.h:853 svt_ext_all_sad_calculation_8x8_16x16 */
void svt_ext_all_sad_calculation_8x8_16x16_hip(uint8_t *src, uint32_t src_stride, uint8_t *ref, uint32_t ref_stride,
                                               uint32_t mv, uint32_t *p_best_sad_8x8, uint32_t *p_best_sad_16x16,
                                               uint32_t *p_best_mv8x8, uint32_t *p_best_mv16x16,
                                               uint32_t p_eight_sad16x16[16][8], uint32_t p_eight_sad8x8[64][8],
                                               bool sub_sad);
/* aom_dsp_rtcd.h:854 svt_ext_eight_sad_calculation_32x32_64x64 */
void svt_ext_eight_sad_calculation_32x32_64x64_hip(uint32_t p_sad16x16[16][8], uint32_t *p_best_sad_32x32,
                                                   uint32_t *p_best_sad_64x64, uint32_t *p_best_mv32x32,
                                                   uint32_t *p_best_mv64x64, uint32_t mv, uint32_t p_sad32x32[4][8]);
/* aom_dsp_rtcd.h:855 svt_initialize_buffer_32bits */
void svt_initialize_buffer_32bits_hip(uint32_t *pointer, uint32_t count128, uint32_t count32, uint32_t value);
/* aom_dsp_rtcd.h:841 downsample_2d */
void svt_aom_downsample_2d_hip(uint8_t *input_samples, uint32_t input_stride, uint32_t input_area_width,
                               uint32_t input_area_height, uint8_t *decim_samples, uint32_t decim_stride,
                               uint32_t decim_step);
/* aom_dsp_rtcd.h:863 sad_16b_kernel (mode-decision consumer; not on the ME path) */
uint32_t svt_aom_sad_16b_kernel_hip(uint16_t *src, uint32_t src_stride, uint16_t *ref, uint32_t ref_stride,
                                    uint32_t height, uint32_t width);

/* aom_dsp_rtcd.h:868 svt_pme_sad_loop_kernel (mode decision's full-pel MV
 * refinement, C at product_coding_loop.c:1811): SAD + MV rate of every visited
 * position of a (search_step-strided) area, strict-< update of *best_cost /
 * *best_mvx / *best_mvy (1/8-pel units). mv_cost_params is the reference's
 * MV_COST_PARAMS (mcomp.h:37); this library reads it through the layout below,
 * which integration/svtme_svt_glue.c checks against the reference header. */
struct svt_mv_cost_param;
#define SVTME_MVCOST_OFF_REF_MV 0         /* const MV *ref_mv (int16 row, col) */
#define SVTME_MVCOST_OFF_TYPE 12          /* MV_COST_TYPE (uint8): 0 entropy .. 5 none */
#define SVTME_MVCOST_OFF_MVJCOST 16       /* const int *mvjcost (4 joints) */
#define SVTME_MVCOST_OFF_MVCOST 24        /* const int *mvcost[2] (row, col; centred) */
#define SVTME_MVCOST_OFF_ERROR_PER_BIT 40 /* int error_per_bit */
void svt_pme_sad_loop_kernel_hip(const struct svt_mv_cost_param *mv_cost_params, uint8_t *src, uint32_t src_stride,
                                 uint8_t *ref, uint32_t ref_stride, uint32_t block_height, uint32_t block_width,
                                 uint32_t *best_cost, int16_t *best_mvx, int16_t *best_mvy,
                                 int16_t search_position_start_x, int16_t search_position_start_y,
                                 int16_t search_area_width, int16_t search_area_height, int16_t search_step,
                                 int16_t mvx, int16_t mvy);

#ifdef __cplusplus
}
#endif
#endif /* SVTME_H */
