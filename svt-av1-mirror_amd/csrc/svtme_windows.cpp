// svtme_windows.cpp — the calls over a window of resident pictures, all on lane 0: the dynamic-GOP
// detector (svtme_dg.hip) and temporal filtering's stages (svtme_tfsp.hip, svtme_tff.hip), alone and as
// one window resident to resident, and the low-delay filter (svtme_tfld.hip). Each holds the context
// lock from its first launch to its last copy, as svtme_submit_picture does: the device outputs are the
// context's, and a release / invalidate of a picture from another thread waits for the lock.
#include <cstring>

#include "svtme_ctx.h"

using namespace svtme_host;

// ---- dynamic-GOP detector (dg_detector_hme_level0 / early_hme, pd_process.c:492-634) ----
extern "C" svtme_status svtme_dg_detect(svtme_ctx *c, const svtme_dg_pair *pairs, uint32_t n, uint16_t sa_width,
                                        uint16_t sa_height, svtme_dg_metrics *metrics, svtme_dg_sb *sb_out) {
    if (!c || !pairs || !metrics)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_dg_detect: null ctx, pairs or metrics");
    if (n < 1 || n > SVTME_DG_MAX_PAIRS)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_dg_detect: %u pairs (1..%d)", n, SVTME_DG_MAX_PAIRS);
    if (!sa_width || !sa_height || ((sa_width + 7u) & ~7u) > SVTME_DG_MAX_SA || sa_height > SVTME_DG_MAX_SA)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_dg_detect: search area %ux%u (1..%d, the width rounded up to 8)",
                    sa_width, sa_height, SVTME_DG_MAX_SA);
    std::lock_guard<std::mutex> lk(c->mu);
    PicBuf *pb[2 * SVTME_DG_MAX_PAIRS]; // pair k: the current picture at 2k, the reference at 2k + 1
    for (uint32_t k = 0; k < n; k++) {
        const uint64_t pn[2] = {pairs[k].cur_picture_number, pairs[k].ref_picture_number};
        PicBuf **pk          = pb + 2 * k;
        for (int i = 0; i < 2; i++)
            if (!(pk[i] = find_pic(c, pn[i])))
                return fail(SVTME_ERR_BAD_PARAMETER, "svtme_dg_detect: picture %llu is not resident",
                            (unsigned long long)pn[i]);
        if (pk[0]->W != pk[1]->W || pk[0]->H != pk[1]->H)
            return fail(SVTME_ERR_BAD_PARAMETER, "svtme_dg_detect: pair %u: picture %llu is %ux%u, picture %llu %ux%u", k,
                        (unsigned long long)pn[0], pk[0]->W, pk[0]->H, (unsigned long long)pn[1], pk[1]->W, pk[1]->H);
        if (pk[0]->W != pb[0]->W || pk[0]->H != pb[0]->H)
            return fail(SVTME_ERR_BAD_PARAMETER, "svtme_dg_detect: pair %u is %ux%u, pair 0 %ux%u: one size per call", k,
                        pk[0]->W, pk[0]->H, pb[0]->W, pb[0]->H);
    }
    const uint32_t W = pb[0]->W, H = pb[0]->H, sbs = svtme_sb_total(W, H);
    HIP_TRY(hipSetDevice(c->device));
    const size_t acc_bytes = sizeof(svtme_dg_metrics) * SVTME_DG_MAX_PAIRS;
    svtme_status st        = ensure_buf(&c->d_dg, &c->dg_cap, acc_bytes + sizeof(svtme_dg_sb) * (size_t)n * sbs);
    if (st)
        return st;
    DevPlane cur[SVTME_DG_MAX_PAIRS], ref[SVTME_DG_MAX_PAIRS];
    for (uint32_t k = 0; k < 2 * n; k++) {
        if ((st = join_upload(c, *pb[k], 0)))
            return st;
        (k & 1 ? ref : cur)[k / 2] = pb[k]->pyr.lv[2];
    }
    Lane &L               = c->lanes[0];
    svtme_dg_metrics *d_m = (svtme_dg_metrics *)c->d_dg;
    svtme_dg_sb *d_sb     = (svtme_dg_sb *)((uint8_t *)c->d_dg + acc_bytes);
    HIP_TRY(hipMemsetAsync(d_m, 0, sizeof(svtme_dg_metrics) * n, L.s));
    HIP_TRY(svtme_launch_dg(cur, ref, n, W, H, sa_width, sa_height, d_m, d_sb, L.s));
    hipEvent_t done;
    if ((st = submission_done(L, &done)))
        return st;
    mark_read(pb, 2 * n, 0, done);
    HIP_TRY(hipMemcpyAsync(metrics, d_m, sizeof(svtme_dg_metrics) * n, hipMemcpyDeviceToHost, L.s));
    if (sb_out)
        HIP_TRY(hipMemcpyAsync(sb_out, d_sb, sizeof(svtme_dg_sb) * (size_t)n * sbs, hipMemcpyDeviceToHost, L.s));
    HIP_TRY(hipStreamSynchronize(L.s));
    for (uint32_t k = 0; k < n; k++) svtme_dg_finish(W, H, &metrics[k]);
    return SVTME_OK;
}

// ---- what the temporal-filter calls share ----
// The resident pictures pn[0..count) of a window, each W x H (8-aligned) and, where the call
// filters chroma, with chroma attached, where it filters 10-bit luma, with the 16-bit plane
// attached, where it filters 10-bit chroma, with the 16-bit chroma planes attached. The first picture
// that fails decides the message.
static svtme_status resident_pics(svtme_ctx *c, const char *fn, const uint64_t *pn, uint32_t count, uint32_t W,
                                  uint32_t H, bool chroma, PicBuf **pb, bool hbd = false, bool hbd_chroma = false) {
    for (uint32_t k = 0; k < count; k++) {
        if (!(pb[k] = find_pic(c, pn[k])))
            return fail(SVTME_ERR_BAD_PARAMETER, "%s: picture %llu is not resident", fn, (unsigned long long)pn[k]);
        if (pb[k]->W != W || pb[k]->H != H)
            return fail(SVTME_ERR_BAD_PARAMETER, "%s: picture %llu is %ux%u, the window %ux%u", fn,
                        (unsigned long long)pn[k], pb[k]->W, pb[k]->H, W, H);
        if (chroma && !pb[k]->cmem)
            return fail(SVTME_ERR_BAD_PARAMETER, "%s: picture %llu has no chroma", fn, (unsigned long long)pn[k]);
        if (hbd && !pb[k]->hmem)
            return fail(SVTME_ERR_BAD_PARAMETER, "%s: picture %llu has no 10-bit plane", fn, (unsigned long long)pn[k]);
        if (hbd_chroma && !pb[k]->hcmem)
            return fail(SVTME_ERR_BAD_PARAMETER, "%s: picture %llu has no 10-bit chroma", fn, (unsigned long long)pn[k]);
    }
    return SVTME_OK;
}

// lane 0 waits for the uploads of the centre pb[0] and the n references behind it; ref[k]: level 0 of reference k
static svtme_status join_window(svtme_ctx *c, PicBuf *const *pb, uint32_t n, DevPlane *ref) {
    for (uint32_t k = 0; k <= n; k++) {
        svtme_status st = join_upload(c, *pb[k], 0);
        if (st)
            return st;
        if (k)
            ref[k - 1] = pb[k]->pyr.lv[0];
    }
    return SVTME_OK;
}

// the ranges of the two stages' controls; `what` names them in the message ("controls" where the
// call has one set, "sub-pel controls" / "filter controls" in the window call)
static svtme_status tfsp_controls_check(const char *fn, const char *what, const svtme_tf_subpel_controls *ctl) {
    if (ctl->half_pel_mode <= 3 && ctl->quarter_pel_mode <= 3 && ctl->eight_pel_mode <= 1 && ctl->use_2tap <= 1 &&
        ctl->sub_sampling_shift <= 1 && ctl->enable_8x8_pred <= 1)
        return SVTME_OK;
    return fail(SVTME_ERR_BAD_PARAMETER,
                "%s: %s out of range: half %u quarter %u (0..3), eighth %u, use_2tap %u, "
                "sub_sampling_shift %u, enable_8x8_pred %u (0..1)", fn, what,
                ctl->half_pel_mode, ctl->quarter_pel_mode, ctl->eight_pel_mode, ctl->use_2tap,
                ctl->sub_sampling_shift, ctl->enable_8x8_pred);
}
static svtme_status tff_controls_check(const char *fn, const char *what, const svtme_tf_filter_controls *ctl) {
    if (ctl->tf_mv_dist_th <= 32767 && ctl->sub_sampling_shift <= 1)
        return SVTME_OK;
    return fail(SVTME_ERR_BAD_PARAMETER, "%s: %s out of range: tf_mv_dist_th %u (0..32767), sub_sampling_shift %u (0..1)",
                fn, what, ctl->tf_mv_dist_th, ctl->sub_sampling_shift);
}

// The filter's scratch in c->d_tff, n references over sbs SBs (units = n x sbs):
//   results of the sub-pel stage | luma tiles | weights | errors | (dense) the luma plane, whole SBs |
//   (chroma) Cb and Cr tiles | weights | (chroma, dense) the two planes, whole SBs
// (704 bytes a result, multiples of 16 per unit or SB elsewhere: the sections stay 16-byte aligned).
// The 10-bit calls (hbd) hold 16-bit luma tiles and a 16-bit dense plane in the same places, and with
// chroma 16-bit chroma tiles and dense planes.
// The stage calls copy dense planes out; the window call writes the result picture and has none.
struct TfScratch {
    svtme_tf_subpel_sb *sub;
    uint8_t *tile, *plane;   // plane: dense only
    uint32_t *wgt, *e32;
    uint8_t *ctile, *cplane; // chroma only, as cwgt; cplane: Cb then Cr, cplane_bytes each, dense only
    uint32_t *cwgt;
    size_t sub_bytes, e32_bytes, cplane_bytes;
};
static svtme_status tf_scratch(svtme_ctx *c, uint32_t n, uint32_t sbs, bool dense, bool chroma, TfScratch *S,
                               bool hbd = false) {
    const size_t units = (size_t)n * sbs;
    S->sub_bytes    = sizeof(svtme_tf_subpel_sb) * units;
    S->e32_bytes    = SVTME_TFF_E32_BYTES * units;
    const size_t bpp = hbd ? 2 : 1;
    S->cplane_bytes = SVTME_TFFC_PLANE_SB_BYTES * bpp * sbs;
    size_t end = 0;
    auto take  = [&end](bool present, size_t bytes) { // the section's offset; absent sections are empty
        const size_t at = end;
        end += present ? bytes : 0;
        return at;
    };
    const size_t tile_bytes = SVTME_TFF_TILE_BYTES * bpp, ctile_bytes = SVTME_TFFC_TILE_BYTES * bpp;
    const size_t o_sub = take(true, S->sub_bytes), o_tile = take(true, tile_bytes * units),
                 o_wgt = take(true, SVTME_TFF_WGT_BYTES * units), o_e32 = take(true, S->e32_bytes),
                 o_plane = take(dense, tile_bytes * sbs),
                 o_ctile = take(chroma, ctile_bytes * units),
                 o_cwgt = take(chroma, SVTME_TFFC_WGT_BYTES * units),
                 o_cplane = take(chroma && dense, 2 * S->cplane_bytes);
    svtme_status st = ensure_buf(&c->d_tff, &c->tff_cap, end);
    if (st)
        return st;
    uint8_t *base = (uint8_t *)c->d_tff;
    S->sub = (svtme_tf_subpel_sb *)(base + o_sub), S->tile = base + o_tile, S->plane = base + o_plane;
    S->wgt = (uint32_t *)(base + o_wgt), S->e32 = (uint32_t *)(base + o_e32);
    S->ctile = base + o_ctile, S->cplane = base + o_cplane, S->cwgt = (uint32_t *)(base + o_cwgt);
    return SVTME_OK;
}

// the chroma side of the yuv calls: the decay factors and the host copies. In the 10-bit yuv calls (a
// TfHbd beside it) `out` holds uint16_t planes and the strides are in samples.
struct TfChroma {
    uint32_t decay[2];
    uint8_t *out[2]; // Cb, Cr; either may be NULL
    uint32_t stride[2];
};

// the 10-bit side of svtme_tf_filter_10bit / svtme_tf_window_10bit: the host copy of the 16-bit plane
struct TfHbd {
    uint16_t *out; // the filter call: required; the window call: may be NULL
    uint32_t stride; // samples
};

// checked before any GPU work: a stride under the chroma width
static svtme_status chroma_strides_ok(const char *fn, const TfChroma *uv, uint32_t width) {
    for (int p = 0; p < 2; p++)
        if (uv->out[p] && uv->stride[p] < (width + 1) >> 1)
            return fail(SVTME_ERR_BAD_PARAMETER, "%s: %s stride %u under the chroma width %u", fn, p ? "cr" : "cb",
                        uv->stride[p], (width + 1) >> 1);
    return SVTME_OK;
}

// the planes the filters read and write of a picture: level 0 and the attached 8-bit chroma, or (hbd) the
// attached 16-bit planes
static const DevPlane &tf_luma(const PicBuf *p, bool hbd) { return hbd ? p->hbd : p->pyr.lv[0]; }
static const DevPlane &tf_chroma(const PicBuf *p, int pl, bool hbd) { return hbd ? p->hchroma[pl] : p->chroma[pl]; }

// The two stages' arguments (svtme_launch_tf_stage) over the scratch of a call: the centre pb[0] and the n
// references behind it. U is filled where the call has chroma (uv). The result picture's planes (Y.dst,
// Y.dst8, U.dst) are the window call's to set; a dense call leaves them zero and the kernels it launches
// do not read them.
static void tf_stage_fill(TfLumaArgs &Y, TfChromaArgs &U, PicBuf *const *pb, uint32_t n, uint32_t W, uint32_t H,
                          const svtme_tf_filter_controls *ctl, const TfChroma *uv, bool hbd, const TfScratch &S) {
    Y.cen = tf_luma(pb[0], hbd);
    for (uint32_t k = 0; k < SVTME_MAX_BATCH_JOBS; k++) Y.ref[k] = tf_luma(pb[k < n ? k + 1 : 1], hbd);
    Y.sub       = S.sub;
    Y.tile      = S.tile;
    Y.wgt       = S.wgt;
    Y.e32       = S.e32;
    Y.plane     = S.plane;
    Y.decay     = ctl->tf_decay_factor_fp16;
    Y.dist_th   = ctl->tf_mv_dist_th;
    Y.ss        = ctl->sub_sampling_shift;
    Y.n         = n;
    Y.pic_w_b64 = (W + 63) / 64;
    Y.sbs       = svtme_sb_total(W, H);
    Y.W         = (int32_t)W;
    Y.H         = (int32_t)H;
    if (!uv)
        return;
    U.cen_y = Y.cen;
    for (int p = 0; p < 2; p++) {
        U.cen[p] = tf_chroma(pb[0], p, hbd);
        for (uint32_t k = 0; k < SVTME_MAX_BATCH_JOBS; k++) U.ref[p][k] = tf_chroma(pb[k < n ? k + 1 : 1], p, hbd).base;
    }
    U.ref_stride = tf_chroma(pb[1], 0, hbd).stride;
    U.sub        = S.sub;
    U.tile_y     = S.tile;
    U.e32        = S.e32;
    U.tile       = S.ctile;
    U.wgt        = S.cwgt;
    U.plane      = S.cplane;
    U.decay_cb   = uv->decay[0];
    U.decay_cr   = uv->decay[1];
    U.dist_th    = ctl->tf_mv_dist_th;
    U.n          = n;
    U.pic_w_b64  = Y.pic_w_b64;
    U.sbs        = Y.sbs;
    U.W          = Y.W;
    U.H          = Y.H;
}

// ---- Temporal filtering's sub-pel refinement (svtme_tfsp.hip) ----
extern "C" svtme_status svtme_tf_subpel(svtme_ctx *c, uint64_t centre_picture_number,
                                        const uint64_t *ref_picture_numbers, uint32_t n, uint32_t width,
                                        uint32_t height, const svtme_tf_subpel_controls *ctl,
                                        const svtme_ref_record *records, svtme_tf_subpel_sb *out) {
    const char *fn = "svtme_tf_subpel";
    if (!c || !ref_picture_numbers || !ctl || !records || !out)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: null ctx, ref_picture_numbers, controls, records or out", fn);
    if (n < 1 || n > SVTME_MAX_BATCH_JOBS)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: %u references (1..%d)", fn, n, SVTME_MAX_BATCH_JOBS);
    svtme_status st;
    if ((st = tfsp_controls_check(fn, "controls", ctl)))
        return st;
    if (!width || !height)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: %ux%u picture", fn, width, height);
    const uint32_t W = svtme_align8_u(width), H = svtme_align8_u(height);
    uint64_t pn[SVTME_MAX_BATCH_JOBS + 1] = {centre_picture_number};
    memcpy(pn + 1, ref_picture_numbers, n * sizeof(uint64_t));
    std::lock_guard<std::mutex> lk(c->mu);
    PicBuf *pb[SVTME_MAX_BATCH_JOBS + 1];
    if ((st = resident_pics(c, fn, pn, n + 1, W, H, false, pb)))
        return st;
    const uint32_t sbs = svtme_sb_total(W, H);
    HIP_TRY(hipSetDevice(c->device));
    const size_t rec_bytes = sizeof(svtme_ref_record) * (size_t)n * sbs;
    const size_t out_bytes = sizeof(svtme_tf_subpel_sb) * (size_t)n * sbs;
    DevPlane ref[SVTME_MAX_BATCH_JOBS];
    if ((st = ensure_buf(&c->d_tfsp, &c->tfsp_cap, rec_bytes + out_bytes)) || (st = join_window(c, pb, n, ref)))
        return st;
    Lane &L                   = c->lanes[0];
    svtme_ref_record *d_rec   = (svtme_ref_record *)c->d_tfsp;
    svtme_tf_subpel_sb *d_out = (svtme_tf_subpel_sb *)((uint8_t *)c->d_tfsp + rec_bytes);
    HIP_TRY(hipMemcpyAsync(d_rec, records, rec_bytes, hipMemcpyHostToDevice, L.s));
    HIP_TRY(svtme_launch_tfsp(&pb[0]->pyr.lv[0], ref, n, W, H, ctl, d_rec, d_out, L.s));
    hipEvent_t done;
    if ((st = submission_done(L, &done)))
        return st;
    mark_read(pb, n + 1, 0, done);
    HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, L.s));
    HIP_TRY(hipStreamSynchronize(L.s));
    return SVTME_OK;
}

// ---- Temporal filtering's prediction and weighting (svtme_tff.hip) ----
// svtme_tf_filter (uv and hb NULL), svtme_tf_filter_yuv (uv), svtme_tf_filter_10bit (hb: `out` and
// `out_stride` are hb's, the stride in samples) and svtme_tf_filter_yuv_10bit (both)
static svtme_status tf_filter_impl(const char *fn, const TfChroma *uv, const TfHbd *hb, svtme_ctx *c,
                                   uint64_t centre_picture_number,
                                   const uint64_t *ref_picture_numbers, uint32_t n, uint32_t width, uint32_t height,
                                   const svtme_tf_filter_controls *ctl, const svtme_tf_subpel_sb *subpel, uint8_t *out,
                                   uint32_t out_stride, uint32_t *err32_out) {
    if (!c || !ref_picture_numbers || !ctl || !subpel || !out)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: null ctx, ref_picture_numbers, controls, subpel or out", fn);
    if (n < 1 || n > SVTME_MAX_BATCH_JOBS)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: %u references (1..%d)", fn, n, SVTME_MAX_BATCH_JOBS);
    svtme_status st;
    if ((st = tff_controls_check(fn, "controls", ctl)))
        return st;
    if (!width || !height)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: %ux%u picture", fn, width, height);
    if (out_stride < width)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: out_stride %u under the width %u", fn, out_stride, width);
    if (uv && (st = chroma_strides_ok(fn, uv, width)))
        return st;
    const uint32_t W = svtme_align8_u(width), H = svtme_align8_u(height);
    const uint32_t sbs = svtme_sb_total(W, H);
    for (size_t k = 0; k < (size_t)n * sbs; k++)
        if (subpel[k].branch > SVTME_TFSP_32)
            return fail(SVTME_ERR_BAD_PARAMETER, "%s: subpel[%zu].branch is %u (0..2)", fn, k, subpel[k].branch);
    uint64_t pn[SVTME_MAX_BATCH_JOBS + 1] = {centre_picture_number};
    memcpy(pn + 1, ref_picture_numbers, n * sizeof(uint64_t));
    std::lock_guard<std::mutex> lk(c->mu);
    PicBuf *pb[SVTME_MAX_BATCH_JOBS + 1];
    const bool hbd = hb != nullptr;
    if ((st = resident_pics(c, fn, pn, n + 1, W, H, uv && !hbd, pb, hbd, uv && hbd)))
        return st;
    HIP_TRY(hipSetDevice(c->device));
    TfScratch S;
    DevPlane ref[SVTME_MAX_BATCH_JOBS];
    if ((st = tf_scratch(c, n, sbs, true, uv != nullptr, &S, hbd)) || (st = join_window(c, pb, n, ref)))
        return st;
    Lane &L              = c->lanes[0];
    const size_t pstride = (size_t)((W + 63) / 64) * 64; // of the dense luma plane; the chroma planes' is half
    HIP_TRY(hipMemcpyAsync(S.sub, subpel, S.sub_bytes, hipMemcpyHostToDevice, L.s));
    TfLumaArgs Y{};
    TfChromaArgs U{};
    tf_stage_fill(Y, U, pb, n, W, H, ctl, uv, hbd, S);
    HIP_TRY(svtme_launch_tf_stage(&Y, uv ? &U : nullptr, hbd, 0, L.s));
    hipEvent_t done;
    if ((st = submission_done(L, &done)))
        return st;
    mark_read(pb, n + 1, 0, done);
    const size_t bpp = hbd ? 2 : 1;
    HIP_TRY(hipMemcpy2DAsync(out, out_stride * bpp, S.plane, pstride * bpp, width * bpp, height, hipMemcpyDeviceToHost,
                             L.s));
    if (err32_out)
        HIP_TRY(hipMemcpyAsync(err32_out, S.e32, S.e32_bytes, hipMemcpyDeviceToHost, L.s));
    for (int p = 0; uv && p < 2; p++)
        if (uv->out[p])
            HIP_TRY(hipMemcpy2DAsync(uv->out[p], uv->stride[p] * bpp, S.cplane + p * S.cplane_bytes, pstride / 2 * bpp,
                                     ((width + 1) >> 1) * bpp, (height + 1) >> 1, hipMemcpyDeviceToHost, L.s));
    HIP_TRY(hipStreamSynchronize(L.s));
    return SVTME_OK;
}

extern "C" svtme_status svtme_tf_filter(svtme_ctx *c, uint64_t centre_picture_number,
                                        const uint64_t *ref_picture_numbers, uint32_t n, uint32_t width,
                                        uint32_t height, const svtme_tf_filter_controls *ctl,
                                        const svtme_tf_subpel_sb *subpel, uint8_t *out, uint32_t out_stride,
                                        uint32_t *err32_out) {
    return tf_filter_impl("svtme_tf_filter", nullptr, nullptr, c, centre_picture_number, ref_picture_numbers, n, width, height,
                          ctl, subpel, out, out_stride, err32_out);
}

extern "C" svtme_status svtme_tf_filter_yuv(svtme_ctx *c, uint64_t centre_picture_number,
                                            const uint64_t *ref_picture_numbers, uint32_t n, uint32_t width,
                                            uint32_t height, const svtme_tf_filter_yuv_controls *ctl,
                                            const svtme_tf_subpel_sb *subpel, const svtme_tf_filter_yuv_out *out) {
    if (!ctl || !out)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_tf_filter_yuv: null controls or out");
    const TfChroma uv = {{ctl->tf_decay_factor_cb_fp16, ctl->tf_decay_factor_cr_fp16},
                         {out->cb, out->cr},
                         {out->cb_stride, out->cr_stride}};
    return tf_filter_impl("svtme_tf_filter_yuv", &uv, nullptr, c, centre_picture_number, ref_picture_numbers, n, width, height,
                          &ctl->luma, subpel, out->y, out->y_stride, out->err32);
}

extern "C" svtme_status svtme_tf_filter_10bit(svtme_ctx *c, uint64_t centre_picture_number,
                                              const uint64_t *ref_picture_numbers, uint32_t n, uint32_t width,
                                              uint32_t height, const svtme_tf_filter_controls *ctl,
                                              const svtme_tf_subpel_sb *subpel, uint16_t *out, uint32_t out_stride,
                                              uint32_t *err32_out) {
    const TfHbd hb = {out, out_stride};
    return tf_filter_impl("svtme_tf_filter_10bit", nullptr, &hb, c, centre_picture_number, ref_picture_numbers, n, width,
                          height, ctl, subpel, (uint8_t *)out, out_stride, err32_out);
}

// ----------------------------------------------------------------------------
// One temporal-filtering window, resident to resident: the TF-ME batch, k_tfsp,
// k_tff_pred and the normalisation into the result picture, chained by lane 0's
// stream through the two stages' scratch.
// ----------------------------------------------------------------------------
// svtme_tf_window (uv and hb NULL), svtme_tf_window_yuv (uv), svtme_tf_window_10bit (hb: the TF-ME
// batch and k_tfsp on the MSB planes as ever, then svtme_tff.hip on the 16-bit planes) and
// svtme_tf_window_yuv_10bit (both)
static svtme_status tf_window_impl(const char *fn, const TfChroma *uv, const TfHbd *hb, svtme_ctx *c,
                                   const svtme_job *jobs, uint32_t n,
                                   uint32_t src_width, uint32_t src_height, const svtme_tf_subpel_controls *sp_ctl,
                                   const svtme_tf_filter_controls *f_ctl, uint64_t out_pn,
                                   const svtme_tf_window_out *out) {
    if (!c || !jobs || !sp_ctl || !f_ctl)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: null ctx, jobs, subpel_controls or filter_controls", fn);
    if (n < 1 || n > SVTME_MAX_BATCH_JOBS)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: %u jobs (1..%d)", fn, n, SVTME_MAX_BATCH_JOBS);
    const uint32_t W = jobs[0].width, H = jobs[0].height;
    if (!W || !H || (W & 7) || (H & 7) || W > 16384 || H > 16384)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: job size %ux%u must be a non-zero multiple of 8, "
                                             "16384 at the most", fn, W, H);
    const uint32_t sbs = svtme_sb_total(W, H);
    for (uint32_t k = 0; k < n; k++) {
        const svtme_job &j = jobs[k];
        if (j.me_type != SVTME_ME_MCTF || j.num_lists != 1 || j.num_refs[0] != 1)
            return fail(SVTME_ERR_BAD_PARAMETER,
                        "%s: job %u: me_type %u, %u lists, %u references (SVTME_ME_MCTF, one list, one "
                        "reference)", fn, k, j.me_type, j.num_lists, j.num_refs[0]);
        if (j.picture_number != jobs[0].picture_number)
            return fail(SVTME_ERR_BAD_PARAMETER, "%s: job %u's centre is picture %llu, job 0's %llu", fn, k,
                        (unsigned long long)j.picture_number, (unsigned long long)jobs[0].picture_number);
        if (j.width != W || j.height != H)
            return fail(SVTME_ERR_BAD_PARAMETER, "%s: job %u is %ux%u, job 0 %ux%u", fn, k, j.width, j.height,
                        W, H);
        if (j.sb_begin != 0 || (j.sb_count != 0 && j.sb_count != sbs))
            return fail(SVTME_ERR_BAD_PARAMETER, "%s: job %u covers SBs [%u, %u) of %u: the whole picture "
                                                 "only", fn, k, j.sb_begin, j.sb_begin + j.sb_count, sbs);
    }
    if (!src_width || !src_height || svtme_align8_u(src_width) != W || svtme_align8_u(src_height) != H)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: source size %ux%u does not align to the jobs' %ux%u", fn,
                    src_width, src_height, W, H);
    if (out && out->plane && out->plane_stride < src_width)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: plane_stride %u under the width %u", fn, out->plane_stride,
                    src_width);
    if (hb && hb->out && hb->stride < src_width)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: plane16_stride %u under the width %u", fn, hb->stride, src_width);
    svtme_status st;
    if ((uv && (st = chroma_strides_ok(fn, uv, src_width))) || (st = tfsp_controls_check(fn, "sub-pel controls", sp_ctl)) ||
        (st = tff_controls_check(fn, "filter controls", f_ctl)))
        return st;
    uint64_t pn[SVTME_MAX_BATCH_JOBS + 1] = {jobs[0].picture_number};
    for (uint32_t k = 0; k < n; k++) {
        pn[k + 1] = jobs[k].ref_picture_number[0][0];
        if (pn[k + 1] == out_pn)
            return fail(SVTME_ERR_BAD_PARAMETER, "%s: the result picture %llu is job %u's reference", fn,
                        (unsigned long long)out_pn, k);
    }
    std::lock_guard<std::mutex> lk(c->mu);
    // The batch checks the same; here before the result picture is made. The pointers hold across
    // the batch and the result picture's allocation: std::map keeps its other nodes where they
    // are, and the result picture, where it is the centre, has the centre's size and stays too.
    PicBuf *pb[SVTME_MAX_BATCH_JOBS + 1];
    const bool hbd = hb != nullptr, uv8 = uv && !hbd, uv16 = uv && hbd;
    if ((st = resident_pics(c, fn, pn, n + 1, W, H, uv8, pb, hbd, uv16)))
        return st;
    HIP_TRY(hipSetDevice(c->device));
    // the sub-pel scratch holds the records (its results go to the filter's scratch)
    const size_t rec_bytes = sizeof(svtme_ref_record) * (size_t)n * sbs;
    TfScratch S;
    if ((st = ensure_buf(&c->d_tfsp, &c->tfsp_cap, rec_bytes)) || (st = tf_scratch(c, n, sbs, false, uv != nullptr, &S, hbd)))
        return st;
    svtme_ref_record *d_rec = (svtme_ref_record *)c->d_tfsp;
    // the TF-ME jobs: one batch, job k's records (R = 1) at d_rec + k x SBs, the array k_tfsp reads
    svtme_ref_record *recs_of[SVTME_MAX_BATCH_JOBS];
    for (uint32_t k = 0; k < n; k++) recs_of[k] = d_rec + (size_t)k * sbs;
    if ((st = submit_batch_locked(c, jobs, n, recs_of, nullptr, false, 0)))
        return st;
    // the result picture (a new number: a buffer of the pool)
    PicBuf *po;
    if ((st = alloc_pic(c, out_pn, W, H, &po, uv8, hbd, uv16)) || (uv8 && (st = alloc_chroma(c, *po))) ||
        (hbd && (st = alloc_hbd(c, *po))) || (uv16 && (st = alloc_hbd_chroma(c, *po))))
        return st;
    Lane &L = c->lanes[0];
    DevPlane ref[SVTME_MAX_BATCH_JOBS];
    for (uint32_t k = 0; k < n; k++) ref[k] = pb[k + 1]->pyr.lv[0]; // (joined to lane 0 by the batch)
    // its old planes, if it had any: an upload still running, readers queued on the other lanes
    if ((st = join_upload(c, *po, 0)) || (st = after_readers(c, *po, L.s)))
        return st;
    HIP_TRY(svtme_launch_tfsp(&pb[0]->pyr.lv[0], ref, n, W, H, sp_ctl, d_rec, S.sub, L.s));
    TfLumaArgs Y{};
    TfChromaArgs U{};
    tf_stage_fill(Y, U, pb, n, W, H, f_ctl, uv, hbd, S);
    Y.dst = tf_luma(po, hbd);
    if (hbd)
        Y.dst8 = po->pyr.lv[0];
    for (int p = 0; uv && p < 2; p++) U.dst[p] = tf_chroma(po, p, hbd);
    HIP_TRY(svtme_launch_tf_stage(&Y, uv ? &U : nullptr, hbd, 1, L.s));
    // the 16-bit planes beyond their true sizes and their margins, from their own interiors
    if (hbd && (st = build_hbd(po, (const uint16_t *)po->hbd.base, (uint32_t)po->hbd.stride / 2, src_width, src_height, L.s)))
        return st;
    for (int p = 0; uv16 && p < 2; p++)
        if ((st = build_hbd_chroma(po, p, (const uint16_t *)po->hchroma[p].base, (uint32_t)po->hchroma[p].stride / 2,
                                   (src_width + 1) >> 1, (src_height + 1) >> 1, L.s)))
            return st;
    // the sub-8 re-pad and the margins from the plane's own interior, then levels 1 and 2
    if ((st = build_pyramid(c, po, po->pyr.lv[0].base, (uint32_t)po->pyr.lv[0].stride, src_width, src_height, 0, L.s)))
        return st;
    // the chroma planes likewise: beyond the true chroma size and the margins, from their own interior
    for (int p = 0; uv8 && p < 2; p++)
        if ((st = build_chroma(po, p, po->chroma[p].base, (uint32_t)po->chroma[p].stride, (src_width + 1) >> 1,
                               (src_height + 1) >> 1, L.s)))
            return st;
    hipEvent_t done;
    if ((st = submission_done(L, &done)))
        return st;
    mark_read(pb, n + 1, 0, done);
    po->used[0] = done; // a later upload under its number waits for the window
    // the other lanes' later readers wait for the window as they do for an asynchronous upload
    if (!po->ready)
        HIP_TRY(hipEventCreateWithFlags(&po->ready, hipEventDisableTiming));
    if ((st = upload_publish(*po, L.s, kAllLanes & ~1u)))
        return st;
    const bool want_uv = uv && (uv->out[0] || uv->out[1]);
    const bool want_16 = hb && hb->out;
    if (!want_uv && !want_16 && (!out || (!out->plane && !out->records && !out->subpel && !out->err32)))
        return SVTME_OK;
    if (out && out->records)
        HIP_TRY(hipMemcpyAsync(out->records, d_rec, rec_bytes, hipMemcpyDeviceToHost, L.s));
    if (out && out->subpel)
        HIP_TRY(hipMemcpyAsync(out->subpel, S.sub, S.sub_bytes, hipMemcpyDeviceToHost, L.s));
    if (out && out->err32)
        HIP_TRY(hipMemcpyAsync(out->err32, S.e32, S.e32_bytes, hipMemcpyDeviceToHost, L.s));
    if (out && out->plane)
        HIP_TRY(hipMemcpy2DAsync(out->plane, out->plane_stride, po->pyr.lv[0].base, (size_t)po->pyr.lv[0].stride,
                                 src_width, src_height, hipMemcpyDeviceToHost, L.s));
    if (want_16)
        HIP_TRY(hipMemcpy2DAsync(hb->out, (size_t)hb->stride * 2, po->hbd.base, (size_t)po->hbd.stride,
                                 (size_t)src_width * 2, src_height, hipMemcpyDeviceToHost, L.s));
    for (int p = 0; want_uv && p < 2; p++) {
        const DevPlane &cp = uv16 ? po->hchroma[p] : po->chroma[p];
        const size_t bpp   = uv16 ? 2 : 1;
        if (uv->out[p])
            HIP_TRY(hipMemcpy2DAsync(uv->out[p], uv->stride[p] * bpp, cp.base, (size_t)cp.stride,
                                     ((src_width + 1) >> 1) * bpp, (src_height + 1) >> 1, hipMemcpyDeviceToHost, L.s));
    }
    HIP_TRY(hipStreamSynchronize(L.s));
    return SVTME_OK;
}

extern "C" svtme_status svtme_tf_window(svtme_ctx *c, const svtme_job *jobs, uint32_t n, uint32_t src_width,
                                        uint32_t src_height, const svtme_tf_subpel_controls *sp_ctl,
                                        const svtme_tf_filter_controls *f_ctl, uint64_t out_pn,
                                        const svtme_tf_window_out *out) {
    return tf_window_impl("svtme_tf_window", nullptr, nullptr, c, jobs, n, src_width, src_height, sp_ctl, f_ctl, out_pn, out);
}

extern "C" svtme_status svtme_tf_window_yuv(svtme_ctx *c, const svtme_job *jobs, uint32_t n, uint32_t src_width,
                                            uint32_t src_height, const svtme_tf_subpel_controls *sp_ctl,
                                            const svtme_tf_filter_yuv_controls *f_ctl, uint64_t out_pn,
                                            const svtme_tf_window_out *out, const svtme_tf_window_yuv_out *out_uv) {
    if (!f_ctl)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_tf_window_yuv: null filter_controls");
    const TfChroma uv = {{f_ctl->tf_decay_factor_cb_fp16, f_ctl->tf_decay_factor_cr_fp16},
                         {out_uv ? out_uv->cb : nullptr, out_uv ? out_uv->cr : nullptr},
                         {out_uv ? out_uv->cb_stride : 0, out_uv ? out_uv->cr_stride : 0}};
    return tf_window_impl("svtme_tf_window_yuv", &uv, nullptr, c, jobs, n, src_width, src_height, sp_ctl, &f_ctl->luma, out_pn,
                          out);
}

extern "C" svtme_status svtme_tf_window_10bit(svtme_ctx *c, const svtme_job *jobs, uint32_t n, uint32_t src_width,
                                              uint32_t src_height, const svtme_tf_subpel_controls *sp_ctl,
                                              const svtme_tf_filter_controls *f_ctl, uint64_t out_pn,
                                              const svtme_tf_window_out *out, uint16_t *plane16, uint32_t plane16_stride) {
    const TfHbd hb = {plane16, plane16_stride};
    return tf_window_impl("svtme_tf_window_10bit", nullptr, &hb, c, jobs, n, src_width, src_height, sp_ctl, f_ctl, out_pn,
                          out);
}

extern "C" svtme_status svtme_tf_filter_yuv_10bit(svtme_ctx *c, uint64_t centre_picture_number,
                                                  const uint64_t *ref_picture_numbers, uint32_t n, uint32_t width,
                                                  uint32_t height, const svtme_tf_filter_yuv_controls *ctl,
                                                  const svtme_tf_subpel_sb *subpel, const svtme_tf_filter_yuv16_out *out) {
    if (!ctl || !out)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_tf_filter_yuv_10bit: null controls or out");
    const TfChroma uv = {{ctl->tf_decay_factor_cb_fp16, ctl->tf_decay_factor_cr_fp16},
                         {(uint8_t *)out->cb, (uint8_t *)out->cr},
                         {out->cb_stride, out->cr_stride}};
    const TfHbd hb    = {out->y, out->y_stride};
    return tf_filter_impl("svtme_tf_filter_yuv_10bit", &uv, &hb, c, centre_picture_number, ref_picture_numbers, n, width,
                          height, &ctl->luma, subpel, (uint8_t *)out->y, out->y_stride, out->err32);
}

extern "C" svtme_status svtme_tf_window_yuv_10bit(svtme_ctx *c, const svtme_job *jobs, uint32_t n, uint32_t src_width,
                                                  uint32_t src_height, const svtme_tf_subpel_controls *sp_ctl,
                                                  const svtme_tf_filter_yuv_controls *f_ctl, uint64_t out_pn,
                                                  const svtme_tf_window_out *out, uint16_t *plane16,
                                                  uint32_t plane16_stride, const svtme_tf_window_yuv16_out *out_uv) {
    if (!f_ctl)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_tf_window_yuv_10bit: null filter_controls");
    const TfChroma uv = {{f_ctl->tf_decay_factor_cb_fp16, f_ctl->tf_decay_factor_cr_fp16},
                         {out_uv ? (uint8_t *)out_uv->cb : nullptr, out_uv ? (uint8_t *)out_uv->cr : nullptr},
                         {out_uv ? out_uv->cb_stride : 0, out_uv ? out_uv->cr_stride : 0}};
    const TfHbd hb    = {plane16, plane16_stride};
    return tf_window_impl("svtme_tf_window_yuv_10bit", &uv, &hb, c, jobs, n, src_width, src_height, sp_ctl, &f_ctl->luma,
                          out_pn, out);
}

// ----------------------------------------------------------------------------
// Low-delay temporal filtering (svtme_tfld.hip): one fused kernel over the co-located blocks,
// into dense planes for the host (svtme_tf_filter_ld) or into the result picture
// (svtme_tf_window_ld), which is then re-padded and published as tf_window_impl's is.
// ----------------------------------------------------------------------------
// the checks of both calls that need no context; W x H: the 8-aligned size
static svtme_status tf_ld_check(const char *fn, const svtme_ctx *c, uint64_t centre, const uint64_t *refs, uint32_t n,
                                uint32_t W, uint32_t H, uint32_t out_w, const svtme_tf_ld_controls *ctl,
                                const svtme_tf_ld_out *out) {
    if (!c || !refs || !ctl)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: null ctx, ref_picture_numbers or controls", fn);
    if (n < 1 || n > SVTME_MAX_BATCH_JOBS)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: %u references (1..%d)", fn, n, SVTME_MAX_BATCH_JOBS);
    if (!W || !H || (W & 7) || (H & 7) || W > 16384 || H > 16384)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: size %ux%u must be a non-zero multiple of 8, 16384 at the most", fn,
                    W, H);
    if ((ctl->bit_depth != 8 && ctl->bit_depth != 10) || ctl->chroma > 1 || ctl->sub_sampling_shift > 1 || ctl->pad)
        return fail(SVTME_ERR_BAD_PARAMETER,
                    "%s: controls out of range: bit_depth %u (8 or 10), chroma %u, sub_sampling_shift %u (0..1), "
                    "pad %u (0)", fn, ctl->bit_depth, ctl->chroma, ctl->sub_sampling_shift, ctl->pad);
    if (out && out->y && out->y_stride < out_w)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: y_stride %u under the width %u", fn, out->y_stride, out_w);
    if (out && ctl->chroma) {
        const TfChroma uv = {{0, 0}, {(uint8_t *)out->cb, (uint8_t *)out->cr}, {out->cb_stride, out->cr_stride}};
        const svtme_status st = chroma_strides_ok(fn, &uv, out_w);
        if (st)
            return st;
    }
    for (uint32_t k = 0; k < n; k++)
        if (refs[k] == centre)
            return fail(SVTME_ERR_BAD_PARAMETER, "%s: the centre picture %llu is reference %u", fn,
                        (unsigned long long)centre, k);
    return SVTME_OK;
}

// the kernel's sources: the planes the mode reads of the centre pb[0] and the n references behind it
static void tfld_sources(TfldArgs &A, PicBuf *const *pb, uint32_t n, uint32_t W, uint32_t H,
                         const svtme_tf_ld_controls *ctl) {
    const bool hbd = ctl->bit_depth == 10;
    A.cen_y        = tf_luma(pb[0], hbd).base;
    A.y_stride     = tf_luma(pb[0], hbd).stride;
    for (uint32_t k = 0; k < SVTME_MAX_BATCH_JOBS; k++) A.ref_y[k] = tf_luma(pb[k < n ? k + 1 : 1], hbd).base;
    for (int p = 0; ctl->chroma && p < 2; p++) {
        A.cen_c[p] = tf_chroma(pb[0], p, hbd).base;
        A.c_stride = tf_chroma(pb[0], p, hbd).stride;
        for (uint32_t k = 0; k < SVTME_MAX_BATCH_JOBS; k++) A.ref_c[p][k] = tf_chroma(pb[k < n ? k + 1 : 1], p, hbd).base;
    }
    for (int p = 0; p < 3; p++) A.decay[p] = ctl->tf_decay_factor_fp16[p];
    A.ss        = ctl->sub_sampling_shift;
    A.n         = n;
    A.pic_w_b64 = (W + 63) / 64;
    A.sbs       = svtme_sb_total(W, H);
    A.W         = (int32_t)W;
    A.H         = (int32_t)H;
}

extern "C" svtme_status svtme_tf_filter_ld(svtme_ctx *c, uint64_t centre_picture_number,
                                           const uint64_t *ref_picture_numbers, uint32_t n, uint32_t width,
                                           uint32_t height, const svtme_tf_ld_controls *ctl, const svtme_tf_ld_out *out) {
    const char *fn = "svtme_tf_filter_ld";
    if (!out || !out->y)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: null out or out->y", fn);
    svtme_status st;
    if ((st = tf_ld_check(fn, c, centre_picture_number, ref_picture_numbers, n, width, height, width, ctl, out)))
        return st;
    const uint32_t W = width, H = height, sbs = svtme_sb_total(W, H);
    const bool hbd = ctl->bit_depth == 10, uv = ctl->chroma != 0;
    uint64_t pn[SVTME_MAX_BATCH_JOBS + 1] = {centre_picture_number};
    memcpy(pn + 1, ref_picture_numbers, n * sizeof(uint64_t));
    std::lock_guard<std::mutex> lk(c->mu);
    PicBuf *pb[SVTME_MAX_BATCH_JOBS + 1];
    if ((st = resident_pics(c, fn, pn, n + 1, W, H, uv && !hbd, pb, hbd, uv && hbd)))
        return st;
    HIP_TRY(hipSetDevice(c->device));
    // the scratch: the variances | the dense luma plane | Cb | Cr, rows of whole SBs (16-byte aligned sections)
    const size_t bpp = hbd ? 2 : 1, pstride = (size_t)((W + 63) / 64) * 64;
    const size_t var_bytes = sizeof(uint32_t) * 4 * (size_t)n * sbs, y_bytes = pstride * bpp * H;
    const size_t c_bytes   = pstride / 2 * bpp * (H / 2);
    if ((st = ensure_buf(&c->d_tff, &c->tff_cap, var_bytes + y_bytes + (uv ? 2 * c_bytes : 0))))
        return st;
    DevPlane ref[SVTME_MAX_BATCH_JOBS];
    if ((st = join_window(c, pb, n, ref)))
        return st;
    uint8_t *base = (uint8_t *)c->d_tff;
    TfldArgs A{};
    tfld_sources(A, pb, n, W, H, ctl);
    A.var32 = (uint32_t *)base;
    A.dst_y = DevPlane{base + var_bytes, (int32_t)(pstride * bpp), (int32_t)W, (int32_t)H, 0};
    void *const host_c[2]      = {out->cb, out->cr};
    const uint32_t c_stride[2] = {out->cb_stride, out->cr_stride};
    for (int p = 0; uv && p < 2; p++)
        if (host_c[p])
            A.dst_c[p] = DevPlane{base + var_bytes + y_bytes + p * c_bytes, (int32_t)(pstride / 2 * bpp), (int32_t)W / 2,
                                  (int32_t)H / 2, 0};
    Lane &L = c->lanes[0];
    HIP_TRY(svtme_launch_tfld(&A, hbd, uv, L.s));
    hipEvent_t done;
    if ((st = submission_done(L, &done)))
        return st;
    mark_read(pb, n + 1, 0, done);
    HIP_TRY(hipMemcpy2DAsync(out->y, out->y_stride * bpp, A.dst_y.base, pstride * bpp, W * bpp, H, hipMemcpyDeviceToHost,
                             L.s));
    for (int p = 0; uv && p < 2; p++)
        if (host_c[p])
            HIP_TRY(hipMemcpy2DAsync(host_c[p], c_stride[p] * bpp, A.dst_c[p].base, pstride / 2 * bpp, W / 2 * bpp, H / 2,
                                     hipMemcpyDeviceToHost, L.s));
    if (out->var32)
        HIP_TRY(hipMemcpyAsync(out->var32, A.var32, var_bytes, hipMemcpyDeviceToHost, L.s));
    HIP_TRY(hipStreamSynchronize(L.s));
    return SVTME_OK;
}

extern "C" svtme_status svtme_tf_window_ld(svtme_ctx *c, uint64_t centre_picture_number,
                                           const uint64_t *ref_picture_numbers, uint32_t n, uint32_t src_width,
                                           uint32_t src_height, const svtme_tf_ld_controls *ctl, uint64_t out_pn,
                                           const svtme_tf_ld_out *out) {
    const char *fn = "svtme_tf_window_ld";
    if (!src_width || !src_height || src_width > 16384 || src_height > 16384)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: source size %ux%u (1..16384)", fn, src_width, src_height);
    const uint32_t W = svtme_align8_u(src_width), H = svtme_align8_u(src_height), sbs = svtme_sb_total(W, H);
    svtme_status st;
    if ((st = tf_ld_check(fn, c, centre_picture_number, ref_picture_numbers, n, W, H, src_width, ctl, out)))
        return st;
    for (uint32_t k = 0; k < n; k++)
        if (ref_picture_numbers[k] == out_pn)
            return fail(SVTME_ERR_BAD_PARAMETER, "%s: the result picture %llu is reference %u", fn,
                        (unsigned long long)out_pn, k);
    const bool hbd = ctl->bit_depth == 10, uv = ctl->chroma != 0, uv8 = uv && !hbd, uv16 = uv && hbd;
    uint64_t pn[SVTME_MAX_BATCH_JOBS + 1] = {centre_picture_number};
    memcpy(pn + 1, ref_picture_numbers, n * sizeof(uint64_t));
    std::lock_guard<std::mutex> lk(c->mu);
    // (the pointers hold across the result picture's allocation, as in tf_window_impl)
    PicBuf *pb[SVTME_MAX_BATCH_JOBS + 1];
    if ((st = resident_pics(c, fn, pn, n + 1, W, H, uv8, pb, hbd, uv16)))
        return st;
    HIP_TRY(hipSetDevice(c->device));
    const bool want_var = out && out->var32;
    const size_t var_bytes = sizeof(uint32_t) * 4 * (size_t)n * sbs;
    if (want_var && (st = ensure_buf(&c->d_tff, &c->tff_cap, var_bytes)))
        return st;
    DevPlane ref[SVTME_MAX_BATCH_JOBS];
    if ((st = join_window(c, pb, n, ref)))
        return st;
    PicBuf *po;
    if ((st = alloc_pic(c, out_pn, W, H, &po, uv8, hbd, uv16)) || (uv8 && (st = alloc_chroma(c, *po))) ||
        (hbd && (st = alloc_hbd(c, *po))) || (uv16 && (st = alloc_hbd_chroma(c, *po))))
        return st;
    Lane &L = c->lanes[0];
    // its old planes, if it had any: an upload still running, readers queued on the other lanes
    if ((st = join_upload(c, *po, 0)) || (st = after_readers(c, *po, L.s)))
        return st;
    TfldArgs A{};
    tfld_sources(A, pb, n, W, H, ctl);
    A.var32 = want_var ? (uint32_t *)c->d_tff : nullptr;
    A.dst_y = hbd ? po->hbd : po->pyr.lv[0];
    if (hbd)
        A.dst8 = po->pyr.lv[0];
    for (int p = 0; uv && p < 2; p++) A.dst_c[p] = hbd ? po->hchroma[p] : po->chroma[p];
    HIP_TRY(svtme_launch_tfld(&A, hbd, uv, L.s));
    // beyond the true sizes and the margins, each plane from its own interior; then levels 1 and 2
    if (hbd && (st = build_hbd(po, (const uint16_t *)po->hbd.base, (uint32_t)po->hbd.stride / 2, src_width, src_height, L.s)))
        return st;
    for (int p = 0; uv16 && p < 2; p++)
        if ((st = build_hbd_chroma(po, p, (const uint16_t *)po->hchroma[p].base, (uint32_t)po->hchroma[p].stride / 2,
                                   (src_width + 1) >> 1, (src_height + 1) >> 1, L.s)))
            return st;
    if ((st = build_pyramid(c, po, po->pyr.lv[0].base, (uint32_t)po->pyr.lv[0].stride, src_width, src_height, 0, L.s)))
        return st;
    for (int p = 0; uv8 && p < 2; p++)
        if ((st = build_chroma(po, p, po->chroma[p].base, (uint32_t)po->chroma[p].stride, (src_width + 1) >> 1,
                               (src_height + 1) >> 1, L.s)))
            return st;
    hipEvent_t done;
    if ((st = submission_done(L, &done)))
        return st;
    mark_read(pb, n + 1, 0, done);
    po->used[0] = done; // a later upload under its number waits for the window
    if (!po->ready)
        HIP_TRY(hipEventCreateWithFlags(&po->ready, hipEventDisableTiming));
    if ((st = upload_publish(*po, L.s, kAllLanes & ~1u)))
        return st;
    if (!out || (!out->y && !(uv && (out->cb || out->cr)) && !out->var32))
        return SVTME_OK;
    const size_t bpp = hbd ? 2 : 1;
    if (out->y)
        HIP_TRY(hipMemcpy2DAsync(out->y, out->y_stride * bpp, A.dst_y.base, (size_t)A.dst_y.stride, src_width * bpp,
                                 src_height, hipMemcpyDeviceToHost, L.s));
    void *const host_c[2]      = {out->cb, out->cr};
    const uint32_t c_stride[2] = {out->cb_stride, out->cr_stride};
    for (int p = 0; uv && p < 2; p++)
        if (host_c[p])
            HIP_TRY(hipMemcpy2DAsync(host_c[p], c_stride[p] * bpp, A.dst_c[p].base, (size_t)A.dst_c[p].stride,
                                     ((src_width + 1) >> 1) * bpp, (src_height + 1) >> 1, hipMemcpyDeviceToHost, L.s));
    if (want_var)
        HIP_TRY(hipMemcpyAsync(out->var32, A.var32, var_bytes, hipMemcpyDeviceToHost, L.s));
    HIP_TRY(hipStreamSynchronize(L.s));
    return SVTME_OK;
}
