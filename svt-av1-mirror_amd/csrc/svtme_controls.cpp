// svtme_controls.cpp — the pure host functions of include/svtme.h: the reference's control
// derivation restated (svtme_derive_controls, svtme_derive_controls_tf), the dynamic-GOP
// detector's search area and host reduction, and the two counting helpers. No HIP here: the file
// compiles with a plain C++17 compiler, so it can be checked stand-alone under the sanitizers.
#include <algorithm>
#include <cstring>

#include "svtme_controls.h"

extern "C" uint32_t svtme_sb_total(uint32_t width, uint32_t height) {
    return ((width + 63) / 64) * ((height + 63) / 64);
}

extern "C" uint32_t svtme_job_ref_slots(const svtme_job *job) {
    return job->num_refs[0] + (job->num_lists == 2 ? job->num_refs[1] : 0);
}

// ---- dynamic-GOP detector (dg_detector_hme_level0 / early_hme, pd_process.c:492-634) ----
extern "C" void svtme_dg_search_area(int input_resolution, uint16_t *sa_width, uint16_t *sa_height) {
    // INPUT_SIZE_360p_RANGE = 1, INPUT_SIZE_480p_RANGE = 2 (definitions.h:2079-2085)
    const uint16_t sa = input_resolution <= 1 ? 16 : input_resolution <= 2 ? 64 : 128;
    if (sa_width)
        *sa_width = sa;
    if (sa_height)
        *sa_height = sa;
}

extern "C" void svtme_dg_reduce(uint32_t width, uint32_t height, const svtme_dg_sb *sb, svtme_dg_metrics *out) {
    if (!sb || !out || !width || !height)
        return;
    const uint32_t wb = (width + 63) / 64, hb = (height + 63) / 64;
    svtme_dg_metrics m{};
    for (uint32_t y = 0; y < hb; y++)
        for (uint32_t x = 0; x < wb; x++) {
            const svtme_dg_sb &s = sb[y * wb + x];
            m.tot_dist += s.sad;
            m.tot_cplx += s.sad > 16 * 16 * 30;
            m.tot_active += s.mv_x != 0 || s.mv_y != 0;
            // does the vector point inwards or outwards? (the middle row / column counts nothing)
            const int sy = s.mv_y > 0 ? 1 : s.mv_y < 0 ? -1 : 0, sx = s.mv_x > 0 ? 1 : s.mv_x < 0 ? -1 : 0;
            m.sum_in_vectors += y < hb / 2 ? -sy : y > hb / 2 ? sy : 0;
            m.sum_in_vectors += x < wb / 2 ? -sx : x > wb / 2 ? sx : 0;
        }
    svtme_dg_finish(width, height, &m);
    *out = m;
}

// ----------------------------------------------------------------------------
// svt_aom_sig_deriv_me restatement, non-RTC, non-screen-content
// (enc_mode_config.c:136-212 set_hme_search_params, :213-340 set_me_search_params,
//  :341-529 prune / sr / 8x8-var / mv-adj controls, :532-589 pre-HME, :671-808)
// ----------------------------------------------------------------------------
static inline int clip3(int lo, int hi, int v) { return v < lo ? lo : (v > hi ? hi : v); }

static void set_area(svtme_area_minmax &a, int w0, int h0, int w1, int h1) {
    a.sa_min = {(uint16_t)w0, (uint16_t)h0};
    a.sa_max = {(uint16_t)w1, (uint16_t)h1};
}

// an area's four sides scaled by qw / 1000, each side held at its floor
static void scale_area(svtme_area_minmax &a, int qw, int min_w, int min_h, int max_w, int max_h) {
    a.sa_min.width  = (uint16_t)std::max(min_w, (a.sa_min.width * qw) / 1000);
    a.sa_min.height = (uint16_t)std::max(min_h, (a.sa_min.height * qw) / 1000);
    a.sa_max.width  = (uint16_t)std::max(max_w, (a.sa_max.width * qw) / 1000);
    a.sa_max.height = (uint16_t)std::max(max_h, (a.sa_max.height * qw) / 1000);
}

extern "C" void svtme_derive_controls(int enc_mode, int qp, int res, int tl, int hierarchical_levels,
                                      int frame_rate_q16, svtme_controls *c) {
    memset(c, 0, sizeof(*c));
    const bool is_base = tl == 0;
    // set_me_search_params (enc_mode_config.c:213-340), rtc_tune = 0, sc_class1 = 0
    int q_mult = 0;
    if (enc_mode <= 1)
        set_area(c->me_sa, 64, 64, 256, 256);
    else if (enc_mode <= 2)
        set_area(c->me_sa, 32, 32, 128, 128);
    else if (enc_mode <= 4)
        set_area(c->me_sa, 24, 24, 104, 104);
    else if (enc_mode <= 6) {
        set_area(c->me_sa, 16, 16, 64, 32);
        q_mult = 7;
    } else if (enc_mode <= 9) {
        if (hierarchical_levels <= 3) {
            if (res < 5)
                set_area(c->me_sa, 8, 5, 16, 9);
            else
                set_area(c->me_sa, 8, 1, 8, 1);
        } else if (res < 4)
            set_area(c->me_sa, 16, 16, 32, 16);
        else
            set_area(c->me_sa, 16, 6, 16, 9);
        q_mult = 7;
    } else {
        set_area(c->me_sa, 16, 6, 16, 6);
        q_mult = 6;
    }
    if (q_mult)
        scale_area(c->me_sa, clip3(500, 1000, (int)(q_mult * ((31 * qp) - 700)) >> 3), 8, 3, 8, 3);
    if (frame_rate_q16 >> 16) { // low_frame_rate_flag (enc_mode_config.c:334-339)
        c->me_sa.sa_min.width  = (uint16_t)((c->me_sa.sa_min.width * 3) >> 1);
        c->me_sa.sa_min.height = (uint16_t)((c->me_sa.sa_min.height * 3) >> 1);
    }
    // set_hme_search_params (enc_mode_config.c:136-212)
    c->num_hme_sa_w = 2;
    c->num_hme_sa_h = 2;
    q_mult          = 0;
    if (enc_mode <= 1) {
        if (res < 5)
            set_area(c->hme_l0_sa, 32, 32, 192, 192);
        else
            set_area(c->hme_l0_sa, 240, 240, 480, 480);
    } else if (enc_mode <= 3)
        set_area(c->hme_l0_sa, 32, 32, 192, 192);
    else if (enc_mode <= 6) {
        set_area(c->hme_l0_sa, 32, 32, 192, 192);
        q_mult = 3;
    } else if (enc_mode <= 7) {
        if (res >= 5)
            set_area(c->hme_l0_sa, 32, 32, 192, 192);
        else
            set_area(c->hme_l0_sa, 16, 16, 192, 192);
        q_mult = 3;
    } else if (enc_mode <= 9) {
        set_area(c->hme_l0_sa, 16, 16, 192, 192);
        q_mult = 3;
    } else {
        if (res < 5)
            set_area(c->hme_l0_sa, 8, 8, 96, 96);
        else
            set_area(c->hme_l0_sa, 16, 16, 96, 96);
        q_mult = 3;
    }
    if (q_mult)
        scale_area(c->hme_l0_sa, clip3(500, 1000, (int)(q_mult * ((8 * qp) - 125))), 8, 8, 96, 96);
    if (enc_mode <= -1) {
        c->hme_l1_sa = {16, 16};
        c->hme_l2_sa = {16, 16};
    } else {
        c->hme_l1_sa = {8, 3};
        c->hme_l2_sa = {8, 3};
    }
    // HME level flags (enc_mode_config.c:1608-1619) and methods (:687-689)
    c->enable_hme_flag        = 1;
    c->enable_hme_level0_flag = 1;
    c->enable_hme_level1_flag = 1;
    c->enable_hme_level2_flag = enc_mode <= 6 ? 1 : 0;
    c->hme_search_method      = SVTME_SUB_SAD_SEARCH;
    c->me_search_method       = SVTME_SUB_SAD_SEARCH;
    c->reduce_hme_l0_sr_th_min = 0;
    c->reduce_hme_l0_sr_th_max = 0;
    // pre-HME level (enc_mode_config.c:707-722, :532-589)
    const int prehme_level = enc_mode <= 7 ? 2 : 4;
    c->prehme_enable = 1;
    if (prehme_level == 2) {
        set_area(c->prehme_sa_cfg[0], 8, 100, 8, 400);
        set_area(c->prehme_sa_cfg[1], 96, 3, 384, 3);
        c->prehme_skip_search_line = 0;
        c->prehme_l1_early_exit    = 0;
    } else {
        set_area(c->prehme_sa_cfg[0], 8, 100, 8, 350);
        set_area(c->prehme_sa_cfg[1], 32, 7, 128, 7);
        c->prehme_skip_search_line = 1;
        c->prehme_l1_early_exit    = 1;
    }
    // hme/me reference pruning (enc_mode_config.c:729-744, :341-410)
    int prune_level;
    if (enc_mode <= 0)
        prune_level = is_base ? 1 : 2;
    else if (enc_mode <= 1)
        prune_level = is_base ? 1 : 4;
    else if (enc_mode <= 3)
        prune_level = is_base ? 1 : 5;
    else if (enc_mode <= 9)
        prune_level = is_base ? 1 : 6;
    else
        prune_level = 6;
    static const uint16_t hme_th[7] = {0xFFFF, 80, 50, 30, 15, 5, 5};
    static const uint16_t me_th[7]  = {0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 60, 60, 60};
    c->enable_me_hme_ref_pruning               = prune_level ? 1 : 0;
    c->prune_ref_if_hme_sad_dev_bigger_than_th = hme_th[prune_level];
    c->prune_ref_if_me_sad_dev_bigger_than_th  = me_th[prune_level];
    if (prune_level == 6) {
        c->zz_sad_th    = 20 * 64 * 64;
        c->zz_sad_pct   = 5;
        c->phme_sad_th  = 10 * 64 * 64;
        c->phme_sad_pct = 5;
    }
    // hme-based ME search-area adjustment (enc_mode_config.c:747-757, :446-509)
    const int sr_level = enc_mode <= -1 ? 0 : (enc_mode <= 0 ? 1 : 3);
    if (sr_level) {
        c->enable_me_sr_adjustment              = 1;
        c->reduce_me_sr_based_on_mv_length_th   = 4;
        c->stationary_hme_sad_abs_th            = 12000;
        c->stationary_me_sr_divisor             = 8;
        c->reduce_me_sr_based_on_hme_sad_abs_th = sr_level == 3 ? 12000 : 6000;
        c->me_sr_divisor_for_low_hme_sad        = 8;
        c->distance_based_hme_resizing          = sr_level == 3 ? 1 : 0;
        if (!c->enable_hme_level2_flag) { // :500-508
            c->stationary_hme_sad_abs_th            = (uint16_t)(c->stationary_hme_sad_abs_th / 4);
            c->reduce_me_sr_based_on_hme_sad_abs_th = (uint16_t)(c->reduce_me_sr_based_on_hme_sad_abs_th / 4);
        }
    }
    // mv-based search-area adjustment (enc_mode_config.c:759-764, :411-431)
    if (enc_mode <= 3) {
        c->mv_sa_adj_enabled          = 1;
        c->mv_sa_adj_nearest_ref_only = 1;
        c->mv_sa_adj_mv_size_th       = 25;
        c->mv_sa_adj_sa_multiplier    = 2;
    }
    // 8x8-variance search-area adjustment, level 2 (enc_mode_config.c:766-767, :511-529)
    c->me_8x8_var_enabled = 1;
    c->me_sr_div4_th      = 80000;
    c->me_sr_div2_th      = 150000;
    c->me_sr_mult2_th     = 0xFFFFFFFFu;
    c->prune_me_candidates_th     = enc_mode <= 6 ? 0 : 65;
    c->use_best_unipred_cand_only = enc_mode <= 3 ? 0 : 1; // enc_mode_config.c:1802-1805
    c->me_early_exit_th           = enc_mode <= 4 ? 0 : 64 * 64 * 8;
    c->me_safe_limit_zz_th        = 0; // safe_limit_nref == 2 at mrp levels 9-10 (enc_handle.c:3542-3543)
    c->prev_me_stage_based_exit_th = 0;
}

// ----------------------------------------------------------------------------
// TF-ME (ME_MCTF) controls: the tf HME enables by tf_ctrls.hme_me_level
// (enc_mode_config.c:1620-1645), svt_aom_sig_deriv_me_tf (:814-854) with
// tf_set_me_hme_params_oq (:588-665), and set_hme_search_params_mctf(ctx, 0)
// (temporal_filtering.c:2759-2767)
// ----------------------------------------------------------------------------
extern "C" void svtme_derive_controls_tf(int hme_me_level, int qp_opt, int qp, int res, svtme_controls *c) {
    memset(c, 0, sizeof(*c));
    c->num_hme_sa_w = 2;
    c->num_hme_sa_h = 2;
    switch (hme_me_level) {
    case 0:
        set_area(c->hme_l0_sa, 30, 30, 60, 60);
        c->hme_l1_sa = {16, 16};
        c->hme_l2_sa = {16, 16};
        set_area(c->me_sa, 60, 60, 120, 120);
        break;
    case 1:
        set_area(c->hme_l0_sa, 16, 16, 32, 32);
        c->hme_l1_sa = {16, 16};
        c->hme_l2_sa = {16, 16};
        set_area(c->me_sa, 16, 16, 32, 32);
        break;
    case 2:
        if (res <= 1) { // INPUT_SIZE_360p_RANGE
            set_area(c->hme_l0_sa, 8, 8, 8, 8);
            c->hme_l1_sa = {8, 8};
        } else if (res <= 2) { // INPUT_SIZE_480p_RANGE
            set_area(c->hme_l0_sa, 8, 8, 16, 16);
            c->hme_l1_sa = {8, 8};
        } else {
            set_area(c->hme_l0_sa, 16, 16, 32, 32);
            c->hme_l1_sa = {16, 16};
        }
        c->hme_l2_sa = {16, 16};
        set_area(c->me_sa, 8, 8, 8, 8);
        break;
    case 3:
        set_area(c->hme_l0_sa, 8, 8, 8, 8);
        c->hme_l1_sa = {8, 8};
        c->hme_l2_sa = {8, 8};
        set_area(c->me_sa, 8, 8, 8, 8);
        break;
    default: // 4
        set_area(c->hme_l0_sa, 4, 4, 4, 4);
        c->hme_l1_sa = {8, 8};
        c->hme_l2_sa = {8, 8};
        set_area(c->me_sa, 8, 8, 8, 8);
        break;
    }
    if (qp_opt)
        scale_area(c->me_sa, clip3(250, 1000, (int)((8 * qp) - 125)), 8, 8, 8, 8);
    c->enable_hme_flag        = 1;
    c->enable_hme_level0_flag = 1;
    c->enable_hme_level1_flag = hme_me_level <= 2 ? 1 : 0;
    c->enable_hme_level2_flag = hme_me_level == 0 ? 1 : 0;
    c->hme_search_method = c->me_search_method = hme_me_level <= 2 ? SVTME_FULL_SAD_SEARCH : SVTME_SUB_SAD_SEARCH;
    // pre-HME, reference pruning, sr adjustment, mv-based area and 8x8 variance: level 0 (off)
    c->prune_ref_if_hme_sad_dev_bigger_than_th = 0xFFFF;
    c->prune_ref_if_me_sad_dev_bigger_than_th  = 0xFFFF;
    c->me_early_exit_th            = hme_me_level <= 1 ? 0 : 64 * 64 * 4;
    c->prev_me_stage_based_exit_th = hme_me_level <= 1 ? 0 : 64 * 64 * 4;
}
