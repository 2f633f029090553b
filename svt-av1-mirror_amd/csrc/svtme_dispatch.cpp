// svtme_dispatch.cpp — host dispatch of the picture job: what a job's kernels are told to do
// (the stage lists, the per-slot search parameters, the full-pel bands: svtme_plan_job) and
// which kernels of svtme_stages.hip run it (svtme_launch_plan, the one place where the
// predicates below and the context's path bits meet). Pure host code: no kernel, no HIP call.
// The predicates are exported for the tests and the benchmark, which report a job's path.
#include "svtme_launch.h"

// Stage-A search list of a job: every independent search the reference may
// perform for a valid slot (see k_stage_a). Host-side, pure.
extern "C" void svtme_stage_a_list(const svtme_job *job, uint8_t *list, uint32_t *count) {
    const svtme_controls &c = job->ctrl;
    uint32_t n = 0;
    for (int s = 0; s < 8; s++) {
        const int l = s >> 2, r = s & 3;
        if (l >= job->num_lists || r >= job->num_refs[l])
            continue;
        if (!(job->temporal_layer_index > 0 || l == 0))
            continue;
        const bool zz = c.me_early_exit_th || c.me_safe_limit_zz_th;
        const bool l0 = c.enable_hme_flag && c.enable_hme_level0_flag;
        if (svtme_hme_rt(&c) && s > 0) { // HME-L0 in the second round (svtme_stage_a1_list)
            if (zz)
                list[n++] = (uint8_t)((TA_ZZ << 3) | s);
        } else if (zz || l0)
            list[n++] = (uint8_t)((TA_HME << 3) | s);
        if (c.prehme_enable)
            list[n++] = (uint8_t)((TA_PH << 3) | s);
    }
    *count = n;
}

// Real-time tune on the split path: the second stage-A round, the HME-L0
// quadrants of slots 1-7 (areas from slot 0's centre, k_stage_d<true>).
extern "C" void svtme_stage_a1_list(const svtme_job *job, uint8_t *list, uint32_t *count) {
    const svtme_controls &c = job->ctrl;
    uint32_t n = 0;
    if (svtme_hme_rt(&c) && c.enable_hme_flag && c.enable_hme_level0_flag)
        for (int s = 1; s < 8; s++) {
            const int l = s >> 2, r = s & 3;
            if (l >= job->num_lists || r >= job->num_refs[l])
                continue;
            if (!(job->temporal_layer_index > 0 || l == 0))
                continue;
            list[n++] = (uint8_t)((TA_L0RT << 3) | s);
        }
    *count = n;
}

// Stage-B refinement list of a job: every (slot, quadrant) HME level 1/2
// refines (hme_level1_b64 / hme_level2_b64 loop over valid slots with
// temporal_layer_index > 0 || list 0). Host-side, pure.
extern "C" void svtme_stage_b_list(const svtme_job *job, uint8_t *list, uint32_t *count) {
    const svtme_controls &c = job->ctrl;
    uint32_t n = 0;
    if (c.enable_hme_flag && (c.enable_hme_level1_flag || c.enable_hme_level2_flag))
        for (int s = 0; s < 8; s++) {
            const int l = s >> 2, r = s & 3;
            if (l >= job->num_lists || r >= job->num_refs[l])
                continue;
            if (!(job->temporal_layer_index > 0 || l == 0))
                continue;
            for (int q = 0; q < 4; q++) list[n++] = (uint8_t)((s << 2) | q);
        }
    *count = n;
}

// Wide full-pel stage geometry, host-side and pure. The largest search area
// integer_search_b64 can reach (me_sa max, x mv multiplier, x 3/2 variance
// growth, rounded up to 8 columns) decides 32-bit argmin keys, and the number
// of search-row bands per (SB, reference).
static void fp_area_bound(const svtme_controls *c, uint32_t *w, uint32_t *h) {
    // min(sa_min x distance, sa_max) (:1303-1304), x mv multiplier (:1305-1310),
    // rounded up to 8 (:1318), then x 3/2 and rounded again by the variance
    // growth (:1424-1427) when its threshold can be passed
    uint32_t mw = c->me_sa.sa_max.width, mh = c->me_sa.sa_max.height;
    if (c->mv_sa_adj_enabled) {
        mw *= c->mv_sa_adj_sa_multiplier;
        mh *= c->mv_sa_adj_sa_multiplier;
    }
    mw = (mw + 7) & ~7u;
    mh = mh < 3 ? 3 : mh;
    if (c->me_8x8_var_enabled && c->me_sr_mult2_th != 0xFFFFFFFFu) {
        mw = ((mw * 3 / 2) + 7) & ~7u;
        mh = mh * 3 / 2;
    }
    *w = mw;
    *h = mh;
}
// the same bound for job validation (svtme_submit.cpp)
extern "C" void svtme_fp_area_bound(const svtme_controls *c, uint32_t *w, uint32_t *h) { fp_area_bound(c, w, h); }

// Per-slot search parameters of k_hme that do not depend on the SB: the
// distance, get_hme_l0_search_area (motion_estimation.c:1800-1867, here with
// l00 = (0, 0); with the real-time reduction, svtme_hme_rt, k_hme recomputes
// slots 1-7 per SB) and the pre-HME areas (prehme_core :1580-1587).
extern "C" void svtme_hme_prepare(DevJob *dj) {
    const svtme_job &job    = dj->job;
    const svtme_controls &c = job.ctrl;
    for (int s = 0; s < 8; s++) {
        const int l = s >> 2, r = s & 3;
        const bool valid = l < job.num_lists && r < job.num_refs[l];
        const uint16_t dist = valid ? svtme::ref_dist_const(job, l, r) : 1;
        dj->sdist[s] = dist;
        int16_t w = 0, h = 0;
        if (valid)
            svtme::hme_l0_area(c, l, r, dist, 0, 0, &w, &h);
        dj->l0_sa[s][0] = w;
        dj->l0_sa[s][1] = h;
        const uint32_t f = svtme::scaled_dist(dist);
        for (int k = 0; k < 2; k++) {
            const uint32_t mw = (uint32_t)c.prehme_sa_cfg[k].sa_min.width * f, xw = c.prehme_sa_cfg[k].sa_max.width;
            const uint32_t mh = (uint32_t)c.prehme_sa_cfg[k].sa_min.height * f, xh = c.prehme_sa_cfg[k].sa_max.height;
            dj->ph_sa[s][k][0] = (int16_t)(uint16_t)(mw < xw ? mw : xw);
            dj->ph_sa[s][k][1] = (int16_t)(uint16_t)(mh < xh ? mh : xh);
        }
    }
}

// k_hme applies: every SB 64 wide, sub-sampled HME rows
extern "C" bool svtme_hme_fused(const svtme_job *job) {
    const svtme_controls &c = job->ctrl;
    return (job->width % 64) == 0 && c.hme_search_method != SVTME_FULL_SAD_SEARCH;
}

// Wavefronts per workgroup of the whole-pass k_hme (one SB each): 3 where ten 3-wave
// workgroups per CU measured faster than eight 4-wave ones, else 4. A pure function
// of the job; SVTME_PATH_HME_4WAVES forces 4. Left at 4, not measured at 3: full-SAD
// full-pel rows, the real-time tune's HME-L0 reduction, more than 4 records.
extern "C" uint32_t svtme_hme_waves(const svtme_job *job) {
    const svtme_controls &c = job->ctrl;
    uint32_t R = 0;
    for (int l = 0; l < job->num_lists && l < 2; l++) R += job->num_refs[l];
    return c.me_search_method != SVTME_FULL_SAD_SEARCH && !svtme_hme_rt(&c) && R <= 4 ? 3u : 4u;
}
// the same under path selection `paths`
extern "C" uint32_t svtme_hme_waves_paths(const svtme_job *job, uint32_t paths) {
    return (paths & SVTME_PATH_HME_4WAVES) ? 4u : svtme_hme_waves(job);
}

// the real-time tune's HME-L0 reduction is on (get_hme_l0_search_area,
// motion_estimation.c:1811-1819): k_hme<..., RT = true> only
extern "C" bool svtme_hme_rt(const svtme_controls *c) {
    return c->enable_me_sr_adjustment && c->distance_based_hme_resizing && c->reduce_hme_l0_sr_th_min &&
           c->reduce_hme_l0_sr_th_max;
}

// k_l1_full applies: full-SAD HME rows, HME-L1 without L2, an L1 area of at most
// 16 x 16 positions (TF-ME levels 0-2)
extern "C" bool svtme_l1_full(const svtme_controls *c) {
    return c->hme_search_method == SVTME_FULL_SAD_SEARCH && c->enable_hme_flag && c->enable_hme_level1_flag &&
           !c->enable_hme_level2_flag && c->hme_l1_sa.width <= 16 && c->hme_l1_sa.height <= 16;
}

// k_l0_full applies: full-SAD HME rows, HME-L0 on, no pre-HME, HME-L0 quadrants of
// at most 16 x 8 positions for every slot, whole source dwords on partial SBs
extern "C" bool svtme_l0_full(const DevJob *dj) {
    const svtme_controls &c = dj->job.ctrl;
    if (c.hme_search_method != SVTME_FULL_SAD_SEARCH || c.prehme_enable || !c.enable_hme_flag ||
        !c.enable_hme_level0_flag || svtme_hme_rt(&c) || (dj->job.width % 64) % 16 != 0 ||
        (dj->paths & SVTME_PATH_NO_L0_FULL))
        return false;
    for (int s = 0; s < 8; s++)
        if (dj->l0_sa[s][0] > 16 || dj->l0_sa[s][1] > 16)
            return false;
    return true;
}

// the same test on a job (bench / diagnostics: which kernel runs stage A)
extern "C" bool svtme_l0_full_job(const svtme_job *job) {
    DevJob dj{};
    dj.job = *job;
    svtme_hme_prepare(&dj);
    return svtme_l0_full(&dj);
}

// position rows per lane of k_l0_full: 2 when every quadrant has at most 8 rows
static bool l0_full_short(const DevJob *dj) {
    for (int s = 0; s < 8; s++)
        if (dj->l0_sa[s][1] > 8)
            return false;
    return true;
}

extern "C" bool svtme_fp_k32(const svtme_controls *c) {
    uint32_t w, h;
    fp_area_bound(c, &w, &h);
    return (c->me_8x8_var_enabled ? 1u : 0u) + w * h <= 4096u; // order 0 is the variance probe
}

// the full-pel area's minimum width reaches 24 positions: 6-quad load sets pay
extern "C" bool svtme_fp_wide(const svtme_controls *c) {
    return c->me_sa.sa_min.width >= 24 && c->me_sa.sa_max.width >= 24;
}

// k_fp_wide applies: sub-sampled rows, 32-bit keys, a wide area of more than one
// band, and the window of 4 bands in its LDS rows (FPW_PITCH dwords, bands of
// at most 8 rows with up to 16 parts)
extern "C" bool svtme_fp_wide_lds(const svtme_controls *c) {
    if (c->me_search_method == SVTME_FULL_SAD_SEARCH || c->enable_me_sr_adjustment == 2 || !svtme_fp_k32(c) ||
        !svtme_fp_wide(c))
        return false;
    uint32_t w, h;
    fp_area_bound(c, &w, &h);
    const uint32_t nsets = ((w + 3) / 4 + FPW_TQ - 1) / FPW_TQ;
    return (w * h) / 512 >= 2 && 14 + nsets * FPW_TQ + 2 + 1 <= FPW_BOFF && h <= 8 * 16;
}

static bool fp_wide_lds(const svtme_controls *c, uint32_t paths) {
    return svtme_fp_wide_lds(c) && !(paths & SVTME_PATH_NO_FP_WIDE);
}

// search-row bands per (SB, reference) of the wide full-pel stage under path selection `paths`
extern "C" uint32_t svtme_fp_parts_paths(const svtme_controls *c, uint32_t paths) {
    if (c->enable_me_sr_adjustment == 2)
        return 0; // slot 0's 64x64 SAD feeds the other slots' areas: per-SB k_stage_c
    uint32_t w, h;
    fp_area_bound(c, &w, &h);
    uint32_t parts = (w * h) / 512;
    if (fp_wide_lds(c, paths)) { // workgroups of 4 bands of <= 8 rows
        parts = parts > (h + 7) / 8 ? parts : (h + 7) / 8;
        parts = (parts + 3) & ~3u;
    }
    return parts < 1 ? 1 : (parts > 16 ? 16 : parts);
}
extern "C" uint32_t svtme_fp_parts(const svtme_controls *c) { return svtme_fp_parts_paths(c, 0); }

// Everything of a DevJob that is derived from its job and path bits alone (dj->job and dj->paths
// are the caller's): the full-pel bands, the stage lists and the per-slot search parameters.
extern "C" void svtme_plan_job(DevJob *dj) {
    dj->parts = svtme_fp_parts_paths(&dj->job.ctrl, dj->paths);
    svtme_stage_a_list(&dj->job, dj->ta_list, &dj->ta_count);
    svtme_stage_a1_list(&dj->job, dj->ta1_list, &dj->ta1_count);
    svtme_stage_b_list(&dj->job, dj->tb_list, &dj->tb_count);
    svtme_hme_prepare(dj);
}

// The kernels of a planned job (svtme_plan_job), by timing slot.
extern "C" void svtme_launch_plan(const DevJob *dj, LaunchPlan *p) {
    const svtme_controls &c = dj->job.ctrl;
    const uint32_t paths    = dj->paths;
    const bool full = c.me_search_method == SVTME_FULL_SAD_SEARCH, k32 = svtme_fp_k32(&c), wide = svtme_fp_wide(&c);
    const bool rt       = svtme_hme_rt(&c); // the real-time tune's HME-L0 reduction
    const bool fused    = svtme_hme_fused(&dj->job) && !(paths & SVTME_PATH_NO_FUSED_HME);
    const bool wide_lds = fp_wide_lds(&c, paths);
    *p                  = LaunchPlan{};
    p->cls = (full ? SVTME_CLS_FULL_ME : 0) | (k32 ? SVTME_CLS_K32 : 0) | (c.enable_hme_level2_flag ? SVTME_CLS_L2 : 0) |
             (dj->parts == 1 ? SVTME_CLS_ONE_PART : 0) | (wide ? SVTME_CLS_FP_WIDE : 0);
    // the whole pass in one launch; SVTME_PATH_SPLIT_PASS keeps k_hme -> k_stage_c1 -> k_stage_e (diagnostics)
    if (fused && dj->parts == 1 && !(paths & SVTME_PATH_SPLIT_PASS)) {
        if (svtme_hme_waves_paths(&dj->job, paths) == 3) // (svtme_hme_waves: sub-sampled rows, no real-time reduction)
            p->kernel[SLOT_A] = k32 ? K_HME_SUB_K32_W3 : K_HME_SUB_K64_W3;
        else
            p->kernel[SLOT_A] = full ? (k32 ? (rt ? K_HME_FULL_K32_RT : K_HME_FULL_K32) : (rt ? K_HME_FULL_K64_RT : K_HME_FULL_K64))
                                     : (k32 ? (rt ? K_HME_SUB_K32_RT : K_HME_SUB_K32) : (rt ? K_HME_SUB_K64_RT : K_HME_SUB_K64));
        return;
    }
    if (fused) {
        p->kernel[SLOT_A] = rt ? K_HME_ONLY_RT : K_HME_ONLY;
    } else {
        p->kernel[SLOT_A] = svtme_l0_full(dj) ? K_L0_FULL_4 : K_STAGE_A;
        p->l0_short       = l0_full_short(dj);
        p->rt_round       = rt;
        p->kernel[SLOT_D] = K_STAGE_D;
        p->kernel[SLOT_B] = svtme_l1_full(&c) && !(paths & SVTME_PATH_NO_L1_FULL) ? K_L1_FULL
                            : c.enable_hme_level2_flag                          ? K_STAGE_B_L2
                                                                                : K_STAGE_B;
    }
    if (dj->parts) { // wide full-pel stage + per-SB decode
        p->kernel[SLOT_C] = wide_lds ? K_FP_WIDE
                            : full   ? (!k32 ? K_STAGE_C1_FULL_K64 : wide ? K_STAGE_C1_FULL_K32_WIDE : K_STAGE_C1_FULL_K32)
                                     : (!k32 ? K_STAGE_C1_SUB_K64 : wide ? K_STAGE_C1_SUB_K32_WIDE : K_STAGE_C1_SUB_K32);
        p->kernel[SLOT_E] = K_STAGE_E;
        p->direct         = dj->job.me_type == SVTME_ME_MCTF && dj->parts == 1 && !dj->out_sb && !wide_lds;
    } else
        p->kernel[SLOT_C] = full ? K_STAGE_C_FULL : K_STAGE_C_SUB;
}

// The plan of a launch over n jobs sharing svtme_launch_key: that of the first, with the two
// reducible facts taken over all jobs and applied to the slots they decide.
extern "C" void svtme_launch_plan_group(const DevJob *h_jobs, uint32_t n, LaunchPlan *p) {
    svtme_launch_plan(&h_jobs[0], p);
    for (uint32_t k = 1; k < n; k++) {
        LaunchPlan q;
        svtme_launch_plan(&h_jobs[k], &q);
        p->l0_short &= q.l0_short;
        p->direct &= q.direct;
    }
    if (p->kernel[SLOT_A] == K_L0_FULL_4 && p->l0_short)
        p->kernel[SLOT_A] = K_L0_FULL_2;
    if (p->direct)
        p->kernel[SLOT_E] = K_NONE;
}

// Batch launch key: jobs launched together must agree on it (svtme_submit.cpp splits a batch into
// groups by it). The plan without the two reducible facts: 5 bits per slot, rt_round, cls.
extern "C" uint32_t svtme_launch_key(const DevJob *dj) {
    static_assert(K_COUNT <= 32, "a kernel id in 5 bits of the launch key");
    LaunchPlan p;
    svtme_launch_plan(dj, &p);
    uint32_t key = (uint32_t)p.cls << 1 | p.rt_round;
    for (int k = 0; k < SLOT_COUNT; k++) key = key << 5 | p.kernel[k];
    return key;
}

static const struct {
    const char *name;
    uint8_t units;
} kKernels[K_COUNT] = {
    {"none", UNITS_SB},
#define SVTME_X(id, nt, units, per_wg, ...) {#__VA_ARGS__, UNITS_##units},
    SVTME_STAGE_KERNELS(SVTME_X)
#undef SVTME_X
};

// the kernel as the table of svtme_launch.h spells it, e.g. "k_hme<true, true, true, false, 3>"
extern "C" const char *svtme_kernel_name(uint32_t id) { return id < K_COUNT ? kKernels[id].name : nullptr; }

// work units of kernel `id` for one job (the launcher sums them over a launch)
extern "C" uint32_t svtme_kernel_units(uint32_t id, const DevJob *dj) {
    const uint32_t sb = dj->job.sb_count;
    switch (kKernels[id].units) {
    case UNITS_SB_TA: return sb * dj->ta_count;
    case UNITS_SB_TA1: return sb * dj->ta1_count;
    case UNITS_SB_TB: return sb * dj->tb_count;
    case UNITS_SB_TB_PAIRS: return sb * (dj->tb_count / 2);
    case UNITS_SB_R_PARTS: return sb * dj->R * dj->parts;
    default: return sb;
    }
}

// Tests and diagnostics: the kernels a job launches when submitted alone under `paths`, with SB
// results (with_sb) or records only, in launch order: ids and their timing slots (both hold
// SVTME_MAX_JOB_KERNELS), and the job's launch key. Returns how many kernels were written.
extern "C" uint32_t svtme_job_kernels(const svtme_job *job, uint32_t paths, int with_sb, uint8_t *ids, uint8_t *slots,
                                      uint32_t *key) {
    svtme_sb_result sb; // never read: out_sb only says whether SB results are wanted
    DevJob dj{};
    dj.job          = *job;
    dj.job.sb_count = 1; // unit counts matter only as zero or not
    dj.R            = 1;
    dj.paths        = paths;
    dj.out_sb       = with_sb ? &sb : nullptr;
    svtme_plan_job(&dj);
    *key = svtme_launch_key(&dj);
    LaunchPlan p;
    svtme_launch_plan_group(&dj, 1, &p);
    uint32_t n = 0;
    auto add   = [&](uint8_t id, int slot) {
        if (svtme_kernel_units(id, &dj)) {
            ids[n]     = id;
            slots[n++] = (uint8_t)slot;
        }
    };
    for (int k = 0; k < SLOT_COUNT; k++) {
        if (p.kernel[k])
            add(p.kernel[k], k);
        if (k == SLOT_A && p.rt_round) {
            add(K_STAGE_D_RT0, SLOT_A);
            add(K_STAGE_A_R1, SLOT_A);
        }
    }
    return n;
}
