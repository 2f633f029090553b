// svtme_submit.cpp — the picture job: validation against the resident pictures, the job-table
// ring, the batch submission every entry point ends in (submit_batch_locked), the lanes' scratch,
// packed host output with its tickets, and the fetch of the context-owned outputs.
#include <algorithm>
#include <chrono>
#include <cstring>

#include "svtme_ctx.h"

using namespace svtme_host;

// The job's pictures, resident and of its size, joined to the lane: their pyramids go into `dj`,
// the pictures themselves are appended to read[*n_read..) for the submission's done event
static svtme_status validate_job(svtme_ctx *c, const svtme_job *job, DevJob *dj, uint32_t *count, int lane,
                                 PicBuf **read, uint32_t *n_read) {
    if (!job)
        return fail(SVTME_ERR_BAD_PARAMETER, "null job");
    if ((job->width & 7) || (job->height & 7) || job->width == 0 || job->height == 0)
        return fail(SVTME_ERR_BAD_PARAMETER, "job size %ux%u must be a non-zero multiple of 8", job->width,
                    job->height);
    if (job->num_lists < 1 || job->num_lists > 2 || job->num_refs[0] > 4 || job->num_refs[1] > 4)
        return fail(SVTME_ERR_BAD_PARAMETER, "bad reference counts");
    if (job->ctrl.num_hme_sa_w != 2 || job->ctrl.num_hme_sa_h != 2)
        return fail(SVTME_ERR_BAD_PARAMETER, "only 2x2 HME-L0 search regions are supported "
                                             "(motion_estimation.c:1875)");
    if (job->me_type != 0 && job->me_type != SVTME_ME_OPEN_LOOP && job->me_type != SVTME_ME_MCTF)
        return fail(SVTME_ERR_BAD_PARAMETER, "me_type %u is neither SVTME_ME_OPEN_LOOP nor SVTME_ME_MCTF",
                    job->me_type);
    if (job->width > 16384 || job->height > 16384)
        return fail(SVTME_ERR_BAD_PARAMETER, "picture too large for int16 search arithmetic");
    // narrow fields of the kernels (svtme_stages.hip): the 13-bit column of k_hme's HME-L2 tile keys
    // (hme_tile64), the 8-bit quad count of k_stage_c's full-pel windows (FpRef::nq, the per-SB kernel
    // of enable_me_sr_adjustment == 2); and the divisors hme_prune_ref_and_adjust_sr divides by
    const svtme_controls &ctl = job->ctrl;
    if (ctl.enable_hme_flag && ctl.enable_hme_level2_flag && ctl.hme_l2_sa.width > 8192)
        return fail(SVTME_ERR_BAD_PARAMETER, "hme_l2_sa.width %u exceeds the limit of 8192 positions",
                    ctl.hme_l2_sa.width);
    if (ctl.enable_me_sr_adjustment == 2) {
        uint32_t bw, bh;
        svtme_fp_area_bound(&ctl, &bw, &bh);
        if (bw > 1016)
            return fail(SVTME_ERR_BAD_PARAMETER, "full-pel search areas up to %u positions wide exceed the limit of "
                                                 "1016 with enable_me_sr_adjustment 2", bw);
    }
    if (ctl.enable_me_sr_adjustment && ctl.enable_hme_flag && job->me_type != SVTME_ME_MCTF &&
        (ctl.stationary_me_sr_divisor == 0 || ctl.me_sr_divisor_for_low_hme_sad == 0))
        return fail(SVTME_ERR_BAD_PARAMETER, "stationary_me_sr_divisor and me_sr_divisor_for_low_hme_sad must be "
                                             "non-zero with enable_me_sr_adjustment (a search-range divisor of 0)");
    const uint32_t total = svtme_sb_total(job->width, job->height);
    const uint32_t n     = job->sb_count ? job->sb_count : total - job->sb_begin;
    if (job->sb_begin >= total || job->sb_begin + n > total)
        return fail(SVTME_ERR_BAD_PARAMETER, "SB range [%u, %u) outside the picture's %u SBs", job->sb_begin,
                    job->sb_begin + n, total);
    auto find = [&](uint64_t pn, DevPyramid *out) -> svtme_status {
        PicBuf *pb = find_pic(c, pn);
        if (!pb)
            return fail(SVTME_ERR_BAD_PARAMETER, "picture %llu is not resident (svtme_picture_upload it first)",
                        (unsigned long long)pn);
        if (pb->W != job->width || pb->H != job->height)
            return fail(SVTME_ERR_BAD_PARAMETER, "picture %llu is %ux%u, job is %ux%u", (unsigned long long)pn,
                        pb->W, pb->H, job->width, job->height);
        svtme_status js = join_upload(c, *pb, lane);
        if (js)
            return js;
        *out              = pb->pyr;
        read[(*n_read)++] = pb;
        return SVTME_OK;
    };
    memset(dj, 0, sizeof(*dj));
    dj->job   = *job;
    dj->paths = c->paths;
    svtme_status st;
    if ((st = find(job->picture_number, &dj->cur)))
        return st;
    for (int l = 0; l < job->num_lists; l++)
        for (int r = 0; r < job->num_refs[l]; r++)
            if ((st = find(job->ref_picture_number[l][r], &dj->ref[l][r])))
                return st;
    dj->R         = svtme_job_ref_slots(job);
    dj->pic_w_b64 = (job->width + 63) / 64;
    *count        = n;
    dj->job.sb_count = n;
    if (dj->R == 0)
        return fail(SVTME_ERR_BAD_PARAMETER, "job has no references");
    return SVTME_OK;
}

svtme_status svtme_host::ensure_ring(svtme_ctx *c) {
    if (c->d_table)
        return SVTME_OK;
    const size_t bytes = sizeof(DevJob) * SVTME_MAX_BATCH * svtme_ctx::kRing;
    HIP_TRY(hipMalloc((void **)&c->d_table, bytes));
    HIP_TRY(hipHostMalloc((void **)&c->h_table, bytes, hipHostMallocMapped));
    HIP_TRY(hipHostGetDevicePointer((void **)&c->h_table_dev, c->h_table, 0)); // read by k_copy_words
    for (int k = 0; k < svtme_ctx::kRing; k++)
        HIP_TRY(hipEventCreateWithFlags(&c->ring_copied[k], hipEventDisableTiming));
    return SVTME_OK;
}

// The lane's inter-stage scratch for submissions of `sbs` SBs and `slots` (SB, reference) slots;
// `wide`: with the keys and slots of the wide full-pel stage (k_stage_c1 + k_stage_e). It grows
// only between the lane's submissions (its queued work reads the old buffers), and new keys are
// not ~0 yet.
static svtme_status ensure_lane_scratch(Lane &L, size_t sbs, size_t slots, bool wide) {
    const size_t ab = sbs * SVTME_A_N * sizeof(ARes), bb = sbs * sizeof(BState);
    const size_t kb = wide ? slots * SVTME_PU_COUNT * sizeof(unsigned long long) : 0;
    const size_t cb = wide ? slots * sizeof(CSlot) : 0;
    if (L.ares_cap < ab || L.bst_cap < bb || L.keys_cap < kb || L.cslot_cap < cb)
        HIP_TRY(hipStreamSynchronize(L.s));
    svtme_status st;
    if ((st = ensure_buf((void **)&L.d_ares, &L.ares_cap, ab)) || (st = ensure_buf((void **)&L.d_bst, &L.bst_cap, bb)))
        return st;
    if (L.keys_cap < kb) {
        if ((st = ensure_buf((void **)&L.d_keys, &L.keys_cap, kb)))
            return st;
        L.keys_rest = false;
    }
    return ensure_buf((void **)&L.d_cslot, &L.cslot_cap, cb);
}

// Validate, lay out and launch n jobs. out[k] / out_sb[k]: device outputs of
// job k; null out => the context's own record buffer (single job only).
svtme_status svtme_host::submit_batch_locked(svtme_ctx *c, const svtme_job *jobs, uint32_t n,
                                             svtme_ref_record *const *out, svtme_sb_result *const *out_sb,
                                             bool with_sb, uint32_t lane) {
    HIP_TRY(hipSetDevice(c->device));
    svtme_status st;
    if ((st = ensure_lane(c, lane)))
        return st;
    Lane &L = c->lanes[lane];
    if (!out && lane != 0)
        return fail(SVTME_ERR_BAD_PARAMETER, "context-owned outputs are lane 0's");
    if (n == 0 || n > SVTME_MAX_BATCH)
        return fail(SVTME_ERR_BAD_PARAMETER, "batch of %u jobs (1..%d)", n, SVTME_MAX_BATCH);
    DevJob hj[SVTME_MAX_BATCH];
    uint32_t count[SVTME_MAX_BATCH];
    PicBuf *read[SVTME_MAX_BATCH * 9]; // the current picture and up to 4 + 4 references of every job
    uint32_t n_read = 0;
    size_t sbs = 0, slots = 0;
    for (uint32_t k = 0; k < n; k++) {
        if ((st = validate_job(c, &jobs[k], &hj[k], &count[k], (int)lane, read, &n_read)))
            return st;
        sbs += count[k];
        slots += (size_t)count[k] * hj[k].R;
    }
    if (!out && n != 1)
        return fail(SVTME_ERR_BAD_PARAMETER, "context-owned outputs hold one job");
    if (out) {
        for (uint32_t k = 0; k < n; k++) {
            if (!out[k])
                return fail(SVTME_ERR_BAD_PARAMETER, "null record buffer for job %u", k);
            hj[k].out_records = out[k];
            hj[k].out_sb      = out_sb ? out_sb[k] : nullptr;
        }
    } else {
        if ((st = ensure_buf((void **)&c->d_records, &c->records_cap, slots * sizeof(svtme_ref_record))))
            return st;
        hj[0].out_records = c->d_records;
        if (with_sb) {
            if ((st = ensure_buf((void **)&c->d_sb, &c->sb_cap, sbs * sizeof(svtme_sb_result))))
                return st;
            hj[0].out_sb = c->d_sb;
        }
    }
    bool any_banded = false, any_single = false, any_wide = false;
    for (uint32_t k = 0; k < n; k++) {
        svtme_plan_job(&hj[k]);
        any_wide |= hj[k].parts != 0;
        any_banded |= hj[k].parts > 1;
        any_single |= hj[k].parts == 1;
    }
    // inter-stage scratch of the whole batch, per-job offsets
    if ((st = ensure_lane_scratch(L, sbs, slots, any_wide)))
        return st;
    if (any_wide) {
        // banded jobs merge with atomic min into keys that must all be ~0; k_stage_e
        // resets what it consumed, plain-store (single band) jobs leave keys behind
        if (any_banded && !L.keys_rest)
            HIP_TRY(hipMemsetAsync(L.d_keys, 0xFF, L.keys_cap, L.s));
        L.keys_rest = !any_single;
    }
    size_t sb_off = 0, slot_off = 0;
    for (uint32_t k = 0; k < n; k++) {
        hj[k].ares  = L.d_ares + sb_off * SVTME_A_N;
        hj[k].bst   = L.d_bst + sb_off;
        hj[k].keys  = hj[k].parts ? L.d_keys + slot_off * SVTME_PU_COUNT : nullptr;
        hj[k].cslot = hj[k].parts ? L.d_cslot + slot_off : nullptr;
        sb_off += count[k];
        slot_off += (size_t)count[k] * hj[k].R;
    }
    // group by kernel variant (stable), publish the table, launch each group
    DevJob ordered[SVTME_MAX_BATCH];
    uint32_t keys[SVTME_MAX_BATCH], m = 0;
    for (uint32_t k = 0; k < n; k++) keys[k] = svtme_launch_key(&hj[k]);
    bool taken[SVTME_MAX_BATCH] = {};
    uint32_t group_start[SVTME_MAX_BATCH + 1], groups = 0;
    for (uint32_t k = 0; k < n; k++) {
        if (taken[k])
            continue;
        group_start[groups++] = m;
        for (uint32_t q = k; q < n; q++)
            if (!taken[q] && keys[q] == keys[k]) {
                ordered[m++] = hj[q];
                taken[q]     = true;
            }
    }
    group_start[groups] = m;
    if ((st = ensure_ring(c)))
        return st;
    int slot = -1;
    for (int k = 0; k < svtme_ctx::kRing && slot < 0; k++)
        if (c->ring_used[k] && c->ring_n[k] == n &&
            memcmp(c->h_table + (size_t)k * SVTME_MAX_BATCH, ordered, sizeof(DevJob) * n) == 0)
            slot = k; // already resident (device copy of this exact table)
    if (slot < 0) {
        slot         = c->ring_next;
        c->ring_next = (slot + 1) % svtme_ctx::kRing;
        DevJob *h    = c->h_table + (size_t)slot * SVTME_MAX_BATCH;
        if (c->ring_used[slot]) { // its pinned copy and the launches that read it (any lane) are done
            HIP_TRY(hipEventSynchronize(c->ring_copied[slot]));
            if (c->ring_read[slot])
                HIP_TRY(hipEventSynchronize(c->ring_read[slot]));
        }
        memcpy(h, ordered, sizeof(DevJob) * n);
        static_assert(sizeof(DevJob) % 4 == 0, "DevJob copied in dwords");
        HIP_TRY(svtme_launch_copy_words(c->h_table_dev + (size_t)slot * SVTME_MAX_BATCH,
                                        c->d_table + (size_t)slot * SVTME_MAX_BATCH,
                                        (uint32_t)(sizeof(DevJob) * n / 4), L.s));
        HIP_TRY(hipEventRecord(c->ring_copied[slot], L.s));
        c->ring_used[slot] = true;
        c->ring_n[slot]    = n;
    }
    DevJob *d = c->d_table + (size_t)slot * SVTME_MAX_BATCH;
    for (uint32_t g = 0; g < groups; g++) {
        hipEvent_t *ev = nullptr;
        uint32_t *mask = nullptr;
        if (c->timing && c->t_pending < svtme_ctx::kTimeSets) {
            ev   = c->tev[c->t_pending];
            mask = &c->tmask[c->t_pending++];
        } else if (c->timing) {
            c->t_dropped++;
        }
        HIP_TRY(svtme_launch_stages(d + group_start[g], ordered + group_start[g], group_start[g + 1] - group_start[g],
                                    L.s, ev, mask));
    }
    // one event per submission: the table slot and the pictures it read point at it
    hipEvent_t done;
    if ((st = submission_done(L, &done)))
        return st;
    c->ring_read[slot] = done;
    mark_read(read, n_read, lane, done);
    // svtme_fetch / svtme_device_records describe the context-owned buffers only:
    // a submission into caller buffers leaves them as they were
    if (!out) {
        c->last_count  = (uint32_t)sbs;
        c->last_R      = hj[0].R;
        c->last_has_sb = with_sb;
    }
    return SVTME_OK;
}

extern "C" svtme_status svtme_submit_picture_device(svtme_ctx *c, const svtme_job *job, svtme_ref_record *d_recs,
                                                    svtme_sb_result *d_sb) {
    if (!c || !d_recs)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_submit_picture_device: null ctx or output");
    std::lock_guard<std::mutex> lk(c->mu);
    return submit_batch_locked(c, job, 1, &d_recs, &d_sb, d_sb != nullptr);
}

extern "C" svtme_status svtme_submit_batch_device(svtme_ctx *c, const svtme_job *jobs, uint32_t n,
                                                  svtme_ref_record *const *d_recs, svtme_sb_result *const *d_sb) {
    if (!c || !jobs || !d_recs)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_submit_batch_device: null ctx, jobs or outputs");
    std::lock_guard<std::mutex> lk(c->mu);
    return submit_batch_locked(c, jobs, n, d_recs, d_sb, d_sb != nullptr);
}

extern "C" svtme_status svtme_submit_batch_device_lane(svtme_ctx *c, uint32_t lane, const svtme_job *jobs,
                                                       uint32_t n, svtme_ref_record *const *d_recs,
                                                       svtme_sb_result *const *d_sb) {
    if (!c || !jobs || !d_recs)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_submit_batch_device_lane: null ctx, jobs or outputs");
    std::lock_guard<std::mutex> lk(c->mu);
    return submit_batch_locked(c, jobs, n, d_recs, d_sb, d_sb != nullptr, lane);
}

// ---- packed host output, asynchronous (tickets) ----
// The device buffer of one packed job over sbs SBs with R slots: records | SB results | packed
// bytes, the sections 256-byte aligned
struct PackedLayout {
    size_t o_sb, o_pk, total;
};
static PackedLayout packed_layout(size_t sbs, uint32_t R, const svtme_pack_layout *L) {
    const size_t rb  = sbs * R * sizeof(svtme_ref_record);
    const size_t sbb = L->sb_results ? sbs * sizeof(svtme_sb_result) : 0;
    PackedLayout p;
    p.o_sb  = align256(rb);
    p.o_pk  = align256(p.o_sb + sbb);
    p.total = p.o_pk + sbs * svtme_packed_sb_bytes(L, R);
    return p;
}

extern "C" svtme_status svtme_reserve(svtme_ctx *c, uint32_t width, uint32_t height, uint32_t max_refs,
                                      uint32_t tickets) {
    if (!c || width == 0 || height == 0 || max_refs == 0 || max_refs > 8 || tickets > SVTME_MAX_TICKETS)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_reserve: bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    // one picture with max_refs slots, or a batch of SVTME_MAX_BATCH_JOBS pictures of one
    // slot each (a TF window): the per-SB scratch covers the batch's SBs
    const size_t pic_sbs = svtme_sb_total(width, height);
    const size_t sbs     = pic_sbs * SVTME_MAX_BATCH_JOBS;
    const size_t slots   = pic_sbs * std::max<size_t>(max_refs, SVTME_MAX_BATCH_JOBS);
    svtme_status st;
    for (uint32_t l = 0; l < SVTME_LANES; l++)
        if ((st = ensure_lane(c, l)) || (st = ensure_lane_scratch(c->lanes[l], sbs, slots, true)))
            return st;
    const svtme_pack_layout pa = {SVTME_PU_COUNT, SVTME_MAX_PA_ME_CAND, SVTME_MAX_PA_ME_MV, 0, 1, {0, 0}};
    const svtme_pack_layout tf = {0, 0, 0, 1, 0, {0, 0}};
    const size_t need = std::max(packed_layout(pic_sbs, max_refs, &pa).total, packed_layout(pic_sbs, max_refs, &tf).total);
    uint32_t k = 0;
    for (auto &t : c->tickets) {
        if (k == tickets)
            break;
        if (t.id) // outstanding: its buffer is in use
            continue;
        if ((st = ensure_buf(&t.d_mem, &t.d_cap, need)))
            return st;
        k++;
    }
    return SVTME_OK;
}

extern "C" svtme_status svtme_submit_pictures_packed_async(svtme_ctx *c, uint32_t lane, uint32_t n,
                                                           const svtme_job *jobs, const svtme_pack_layout *layouts,
                                                           void *const *host_outs, uint64_t *tickets) {
    if (!c || !jobs || !layouts || !host_outs || !tickets)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_submit_pictures_packed_async: null argument");
    if (n == 0 || n > SVTME_MAX_BATCH_JOBS)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_submit_pictures_packed_async: %u jobs (1..%d)", n,
                    SVTME_MAX_BATCH_JOBS);
    for (uint32_t k = 0; k < n; k++) {
        const svtme_pack_layout *L = &layouts[k];
        if (!host_outs[k])
            return fail(SVTME_ERR_BAD_PARAMETER, "svtme_submit_pictures_packed_async: null host_out %u", k);
        if (L->sb_results && (L->n_pus == 0 || L->n_pus > SVTME_PU_COUNT || L->max_cand == 0 ||
                              L->max_cand > SVTME_MAX_PA_ME_CAND || L->max_refs == 0 ||
                              L->max_refs > SVTME_MAX_PA_ME_MV))
            return fail(SVTME_ERR_BAD_PARAMETER, "pack layout: %u PUs, %u candidates, %u MVs", L->n_pus,
                        L->max_cand, L->max_refs);
    }
    std::unique_lock<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    // n free ticket slots; with too few free, wait for other threads' svtme_ticket_wait
    // to retire some (up to 100 ms while nobody waits on a ticket: then the caller
    // holds them itself and is refused)
    Ticket *t[SVTME_MAX_BATCH_JOBS];
    auto free_slots = [&]() {
        uint32_t k = 0;
        for (auto &x : c->tickets)
            if (!x.id && k < n)
                t[k++] = &x;
        return k == n;
    };
    auto someone_waits = [&]() {
        for (auto &x : c->tickets)
            if (x.waiting)
                return true;
        return false;
    };
    const auto grace = std::chrono::steady_clock::now() + std::chrono::milliseconds(100);
    while (!free_slots()) {
        if (!someone_waits() && std::chrono::steady_clock::now() >= grace)
            return fail(SVTME_ERR_INSUFFICIENT_RESOURCES,
                        "%d packed jobs outstanding and none being waited on (svtme_ticket_wait retires them)",
                        SVTME_MAX_TICKETS);
        c->retired.wait_for(lk, std::chrono::milliseconds(5));
    }
    if (!c->dstream)
        HIP_TRY(hipStreamCreateWithFlags(&c->dstream, hipStreamNonBlocking));
    svtme_ref_record *d_recs[SVTME_MAX_BATCH_JOBS];
    svtme_sb_result *d_sb[SVTME_MAX_BATCH_JOBS];
    void *d_pack[SVTME_MAX_BATCH_JOBS];
    size_t pbytes[SVTME_MAX_BATCH_JOBS];
    uint32_t counts[SVTME_MAX_BATCH_JOBS], Rs[SVTME_MAX_BATCH_JOBS];
    bool any_sb = false;
    svtme_status st;
    for (uint32_t k = 0; k < n; k++) {
        const svtme_job *job       = &jobs[k];
        const svtme_pack_layout *L = &layouts[k];
        const uint32_t total = svtme_sb_total(job->width, job->height);
        counts[k] = job->sb_count ? job->sb_count : (job->sb_begin < total ? total - job->sb_begin : 0);
        Rs[k]     = svtme_job_ref_slots(job);
        const PackedLayout p = packed_layout(counts[k], Rs[k], L);
        pbytes[k]            = p.total - p.o_pk;
        if ((st = ensure_buf(&t[k]->d_mem, &t[k]->d_cap, p.total))) // free slot: nothing reads it
            return st;
        d_recs[k] = (svtme_ref_record *)t[k]->d_mem;
        d_sb[k]   = L->sb_results ? (svtme_sb_result *)((uint8_t *)t[k]->d_mem + p.o_sb) : nullptr;
        d_pack[k] = (uint8_t *)t[k]->d_mem + p.o_pk;
        any_sb |= d_sb[k] != nullptr;
    }
    if ((st = ensure_lane(c, lane)))
        return st;
    for (uint32_t k = 0; k < n; k++)
        HIP_TRY(hipEventRecord(t[k]->queued, c->lanes[lane].s));
    // one launch over every job (the stage kernels take up to SVTME_MAX_BATCH jobs)
    if ((st = submit_batch_locked(c, jobs, n, d_recs, d_sb, any_sb, lane)))
        return st;
    hipStream_t ls = c->lanes[lane].s;
    for (uint32_t k = 0; k < n; k++) {
        HIP_TRY(svtme_launch_pack(d_recs[k], d_sb[k], counts[k], Rs[k], &layouts[k], d_pack[k], ls));
        HIP_TRY(hipEventRecord(t[k]->launched, ls));
        HIP_TRY(hipStreamWaitEvent(c->dstream, t[k]->launched, 0));
        HIP_TRY(hipMemcpyAsync(host_outs[k], d_pack[k], pbytes[k], hipMemcpyDeviceToHost, c->dstream));
        HIP_TRY(hipEventRecord(t[k]->done, c->dstream));
        t[k]->id   = ++c->ticket_seq;
        tickets[k] = t[k]->id;
    }
    return SVTME_OK;
}

extern "C" svtme_status svtme_submit_picture_packed_async(svtme_ctx *c, uint32_t lane, const svtme_job *job,
                                                          const svtme_pack_layout *L, void *host_out,
                                                          uint64_t *ticket) {
    if (!c || !job || !L || !host_out || !ticket)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_submit_picture_packed_async: null argument");
    return svtme_submit_pictures_packed_async(c, lane, 1, job, L, &host_out, ticket);
}

extern "C" svtme_status svtme_ticket_wait_timed(svtme_ctx *c, uint64_t ticket, float *gpu_ms, float *copy_ms) {
    if (!c || !ticket)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_ticket_wait: null ctx or ticket");
    hipEvent_t done = nullptr;
    Ticket *t       = nullptr;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        for (auto &x : c->tickets)
            if (x.id == ticket && !x.waiting) {
                t = &x;
                break;
            }
        if (!t)
            return fail(SVTME_ERR_BAD_PARAMETER, "svtme_ticket_wait: ticket %llu is not outstanding",
                        (unsigned long long)ticket);
        t->waiting = true;
        done       = t->done;
    }
    HIP_TRY(hipSetDevice(c->device));
    hipError_t e = hipEventSynchronize(done); // without the context lock: other threads submit meanwhile
    // GPU-side times: the job's turn on its lane -> its packed output ready; -> in host memory
    if (e == hipSuccess && gpu_ms)
        e = hipEventElapsedTime(gpu_ms, t->queued, t->launched);
    if (e == hipSuccess && copy_ms)
        e = hipEventElapsedTime(copy_ms, t->launched, t->done);
    std::lock_guard<std::mutex> lk(c->mu);
    t->waiting = false;
    t->id      = 0;
    c->retired.notify_all();
    if (e != hipSuccess)
        return fail(SVTME_ERR_UNDEFINED, "svtme_ticket_wait: %s", hipGetErrorString(e));
    return SVTME_OK;
}

extern "C" svtme_status svtme_ticket_wait(svtme_ctx *c, uint64_t ticket) {
    return svtme_ticket_wait_timed(c, ticket, nullptr, nullptr);
}

// ---- the context-owned outputs ----
extern "C" svtme_status svtme_submit_picture_async(svtme_ctx *c, const svtme_job *job) {
    if (!c)
        return fail(SVTME_ERR_BAD_PARAMETER, "null ctx");
    std::lock_guard<std::mutex> lk(c->mu);
    return submit_batch_locked(c, job, 1, nullptr, nullptr, true);
}

extern "C" svtme_status svtme_sync(svtme_ctx *c) {
    if (!c)
        return fail(SVTME_ERR_BAD_PARAMETER, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    return quiesce(c);
}

static svtme_status fetch_locked(svtme_ctx *c, svtme_ref_record *recs, svtme_sb_result *sb) {
    HIP_TRY(hipSetDevice(c->device));
    if (recs)
        HIP_TRY(hipMemcpyAsync(recs, c->d_records, (size_t)c->last_count * c->last_R * sizeof(svtme_ref_record),
                               hipMemcpyDeviceToHost, c->stream));
    if (sb) {
        if (!c->last_has_sb)
            return fail(SVTME_ERR_BAD_PARAMETER, "last job produced no SB results");
        HIP_TRY(hipMemcpyAsync(sb, c->d_sb, (size_t)c->last_count * sizeof(svtme_sb_result), hipMemcpyDeviceToHost,
                               c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SVTME_OK;
}

extern "C" svtme_status svtme_fetch(svtme_ctx *c, svtme_ref_record *recs, svtme_sb_result *sb) {
    if (!c)
        return fail(SVTME_ERR_BAD_PARAMETER, "null ctx");
    std::lock_guard<std::mutex> lk(c->mu);
    return fetch_locked(c, recs, sb);
}

// Submit and fetch under one hold of the context lock: the encoder's ME threads
// call this concurrently, and another thread's submission must not replace the
// context-owned records between this job's launch and its copy-out.
extern "C" svtme_status svtme_submit_picture(svtme_ctx *c, const svtme_job *job, svtme_ref_record *recs,
                                             svtme_sb_result *sb) {
    if (!c)
        return fail(SVTME_ERR_BAD_PARAMETER, "null ctx");
    std::lock_guard<std::mutex> lk(c->mu);
    svtme_status st = submit_batch_locked(c, job, 1, nullptr, nullptr, sb != nullptr);
    if (st)
        return st;
    return fetch_locked(c, recs, sb);
}

extern "C" void *svtme_device_records(svtme_ctx *c, uint64_t *bytes) {
    if (!c)
        return nullptr;
    if (bytes)
        *bytes = (uint64_t)c->last_count * c->last_R * sizeof(svtme_ref_record);
    return c->d_records;
}
