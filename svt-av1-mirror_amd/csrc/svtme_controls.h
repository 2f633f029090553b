// svtme_controls.h — what svtme_controls.cpp (pure host code) shares with the files that call
// HIP. Internal and free of HIP itself.
#pragma once
#include "../../include/svtme.h"

// the four derived fields of the dynamic-GOP metrics from the accumulated ones (early_hme,
// pd_process.c:627-633): C integer division (toward zero for a negative sum_in_vectors) and the
// narrowing of the context's fields. svtme_dg_reduce and svtme_dg_detect both end with it.
static inline void svtme_dg_finish(uint32_t width, uint32_t height, svtme_dg_metrics *m) {
    const uint32_t sbs = svtme_sb_total(width, height);
    m->mv_in_out_count = (int16_t)(m->sum_in_vectors * 100 / (int)sbs);
    m->norm_dist       = m->tot_dist / sbs;
    m->perc_cplx       = (uint8_t)((m->tot_cplx * 100) / sbs);
    m->perc_active     = (uint8_t)((m->tot_active * 100) / sbs);
}
