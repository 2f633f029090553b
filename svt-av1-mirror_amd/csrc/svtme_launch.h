// svtme_launch.h — the launch boundary inside libsvtme.so: every launcher and primer the .hip
// files define for the host files (svtme_ctx.h), and the host dispatch of the picture job
// (svtme_dispatch.cpp). Included by the callers and by every file that defines one of these
// functions, so a declaration that drifts from its definition does not compile. Internal: none
// of this is part of include/svtme.h.
#pragma once
#include <hip/hip_runtime.h>

#include "svtme_device.h"

// ----------------------------------------------------------------------------
// The kernels of a picture job (svtme_stages.hip), one row per instantiation the launcher can
// choose: X(id, workgroup size, work units of a job, units per workgroup, kernel). Units per
// workgroup is 4 where four units (wavefronts) share a workgroup. svtme_stages.hip builds its
// launch table from these rows and svtme_prime_stages walks it; ids start at 1, 0 is "none".
// The rows keep the order in which the kernels were first instantiated: it decides their order
// in the code object, and a new row belongs at the end.
// ----------------------------------------------------------------------------
#define SVTME_STAGE_KERNELS(X)                                                                                      \
    X(K_HME_SUB_K32, 256, SB, 1, k_hme<true, true, true, false>)                                                    \
    X(K_HME_SUB_K32_RT, 256, SB, 1, k_hme<true, true, true, true>)                                                  \
    X(K_HME_ONLY, 256, SB, 1, k_hme<false, true, true, false>)                                                      \
    X(K_HME_SUB_K64, 256, SB, 1, k_hme<true, true, false, false>)                                                   \
    X(K_HME_SUB_K32_W3, 192, SB, 1, k_hme<true, true, true, false, 3>)                                              \
    X(K_HME_SUB_K64_W3, 192, SB, 1, k_hme<true, true, false, false, 3>)                                             \
    X(K_STAGE_A, 256, SB_TA, 4, k_stage_a<false>)                                                                   \
    X(K_STAGE_A_R1, 256, SB_TA1, 4, k_stage_a<true>)                                                                \
    X(K_STAGE_D, 256, SB, 4, k_stage_d<false>)                                                                      \
    X(K_STAGE_D_RT0, 256, SB, 4, k_stage_d<true>)                                                                   \
    X(K_STAGE_B, 256, SB_TB, 4, k_stage_b<false>)                                                                   \
    X(K_STAGE_B_L2, 256, SB_TB, 4, k_stage_b<true>)                                                                 \
    X(K_STAGE_C_FULL, 256, SB, 1, k_stage_c<false>)                                                                 \
    X(K_STAGE_C_SUB, 256, SB, 1, k_stage_c<true>)                                                                   \
    X(K_STAGE_C1_SUB_K32_WIDE, 256, SB_R_PARTS, 4, k_stage_c1<true, true, true>)                                    \
    X(K_STAGE_C1_SUB_K32, 256, SB_R_PARTS, 4, k_stage_c1<true, true>)                                               \
    X(K_STAGE_C1_SUB_K64, 256, SB_R_PARTS, 4, k_stage_c1<true, false>)                                              \
    X(K_STAGE_C1_FULL_K32_WIDE, 256, SB_R_PARTS, 4, k_stage_c1<false, true, true>)                                  \
    X(K_STAGE_C1_FULL_K32, 256, SB_R_PARTS, 4, k_stage_c1<false, true>)                                             \
    X(K_STAGE_C1_FULL_K64, 256, SB_R_PARTS, 4, k_stage_c1<false, false>)                                            \
    X(K_L0_FULL_2, 256, SB_TA, 4, k_l0_full<2>)                                                                     \
    X(K_L0_FULL_4, 256, SB_TA, 4, k_l0_full<4>)                                                                     \
    X(K_L1_FULL, 256, SB_TB_PAIRS, 4, k_l1_full)                                                                    \
    X(K_FP_WIDE, 256, SB_R_PARTS, 4, k_fp_wide)                                                                     \
    X(K_STAGE_E, 256, SB, 1, k_stage_e)                                                                             \
    X(K_HME_FULL_K32_RT, 256, SB, 1, k_hme<true, false, true, true>)                                                \
    X(K_HME_FULL_K32, 256, SB, 1, k_hme<true, false, true, false>)                                                  \
    X(K_HME_FULL_K64_RT, 256, SB, 1, k_hme<true, false, false, true>)                                               \
    X(K_HME_FULL_K64, 256, SB, 1, k_hme<true, false, false, false>)                                                 \
    X(K_HME_SUB_K64_RT, 256, SB, 1, k_hme<true, true, false, true>)                                                 \
    X(K_HME_ONLY_RT, 256, SB, 1, k_hme<false, true, true, true>)

enum KernelId : uint8_t {
    K_NONE = 0,
#define SVTME_X(id, nt, units, per_wg, ...) id,
    SVTME_STAGE_KERNELS(SVTME_X)
#undef SVTME_X
    K_COUNT
};

// how a kernel's work units are counted per job (svtme_kernel_units)
enum KernelUnits : uint8_t {
    UNITS_SB,          // sb_count
    UNITS_SB_TA,       // sb_count * ta_count
    UNITS_SB_TA1,      // sb_count * ta1_count
    UNITS_SB_TB,       // sb_count * tb_count
    UNITS_SB_TB_PAIRS, // sb_count * (tb_count / 2): two quadrants per wavefront
    UNITS_SB_R_PARTS,  // sb_count * R * parts
};

// The timing slots of a launch (svtme_timing_read): stage k's events are ev[2k], ev[2k + 1].
enum { SLOT_A, SLOT_D, SLOT_B, SLOT_C, SLOT_E, SLOT_COUNT };

// Job facts that choose no kernel beyond what the slots say, but by which the launch key has
// always kept jobs apart: a batch groups exactly as it did when the key was these facts.
#define SVTME_CLS_FULL_ME 1u    // me_search_method == SVTME_FULL_SAD_SEARCH
#define SVTME_CLS_K32 2u        // svtme_fp_k32
#define SVTME_CLS_L2 4u         // enable_hme_level2_flag
#define SVTME_CLS_ONE_PART 8u   // parts == 1
#define SVTME_CLS_FP_WIDE 16u   // svtme_fp_wide

// Which kernels one job runs (svtme_launch_plan). A slot's kernel is launched when the jobs of
// the launch have work units for it (a job without stage-A searches has none for slot A).
struct LaunchPlan {
    uint8_t kernel[SLOT_COUNT]; // KernelId per timing slot, or K_NONE
    uint8_t rt_round; // the real-time tune's second round, k_stage_d<true> then k_stage_a<true>, inside slot A
    uint8_t cls;      // SVTME_CLS_*
    // The two facts a launch reduces over its jobs (AND); they are not part of the launch key.
    uint8_t l0_short; // HME-L0 quadrants of at most 8 rows: K_L0_FULL_4 in slot A becomes K_L0_FULL_2
    uint8_t direct;   // every record made by k_stage_c1 (direct_records): no K_STAGE_E
};
#define SVTME_MAX_JOB_KERNELS (SLOT_COUNT + 2)

extern "C" {
// ---- host dispatch of the picture job (svtme_dispatch.cpp): pure host functions ----
void svtme_stage_a_list(const svtme_job *job, uint8_t *list, uint32_t *count);
void svtme_stage_a1_list(const svtme_job *job, uint8_t *list, uint32_t *count);
void svtme_stage_b_list(const svtme_job *job, uint8_t *list, uint32_t *count);
void svtme_fp_area_bound(const svtme_controls *c, uint32_t *w, uint32_t *h);
void svtme_hme_prepare(DevJob *dj);
bool svtme_hme_fused(const svtme_job *job);
uint32_t svtme_hme_waves(const svtme_job *job);
uint32_t svtme_hme_waves_paths(const svtme_job *job, uint32_t paths);
bool svtme_hme_rt(const svtme_controls *c);
bool svtme_l1_full(const svtme_controls *c);
bool svtme_l0_full(const DevJob *dj);
bool svtme_l0_full_job(const svtme_job *job);
bool svtme_fp_k32(const svtme_controls *c);
bool svtme_fp_wide(const svtme_controls *c);
bool svtme_fp_wide_lds(const svtme_controls *c);
uint32_t svtme_fp_parts_paths(const svtme_controls *c, uint32_t paths);
uint32_t svtme_fp_parts(const svtme_controls *c);
void svtme_plan_job(DevJob *dj);
void svtme_launch_plan(const DevJob *dj, LaunchPlan *p);
void svtme_launch_plan_group(const DevJob *h_jobs, uint32_t n, LaunchPlan *p);
uint32_t svtme_launch_key(const DevJob *dj);
uint32_t svtme_kernel_units(uint32_t id, const DevJob *dj);
uint32_t svtme_job_kernels(const svtme_job *job, uint32_t paths, int with_sb, uint8_t *ids, uint8_t *slots,
                           uint32_t *key);
const char *svtme_kernel_name(uint32_t id);

// ---- launchers and primers (the .hip files) ----
hipError_t svtme_prime_stages(void);
hipError_t svtme_launch_stages(const DevJob *d_jobs, const DevJob *h_jobs, uint32_t n, hipStream_t s, hipEvent_t *ev,
                               uint32_t *mask);
hipError_t svtme_prime_pyramid(void);
hipError_t svtme_launch_host_rows(const uint8_t *src, uint32_t src_stride, int w, int h, uint8_t *dst,
                                  uint32_t dst_stride, hipStream_t s);
hipError_t svtme_launch_build_full(const void *src, uint32_t src_stride, int w, int h, int ten_bit, DevPlane dst,
                                   int left, int top, int rows, hipStream_t s);
// an attached 16-bit plane (svtme_hbd_geometry, svtme_hbd_chroma_geometry); src_stride in samples
hipError_t svtme_launch_build_full16(const uint16_t *src, uint32_t src_stride, int w, int h, DevPlane dst, int left,
                                     int top, int rows, hipStream_t s);
hipError_t svtme_launch_build_down(DevPlane prev, DevPlane dst, int left, int top, int rows, hipStream_t s);
hipError_t svtme_launch_copy_words(const void *src, void *dst, uint32_t nwords, hipStream_t s);
hipError_t svtme_prime_pack(void);
hipError_t svtme_launch_pack(const svtme_ref_record *d_recs, const svtme_sb_result *d_sb, uint32_t n_sb, uint32_t R,
                             const svtme_pack_layout *L, void *d_out, hipStream_t s);
hipError_t svtme_prime_dg(void);
hipError_t svtme_launch_dg(const DevPlane *cur, const DevPlane *ref, uint32_t n, uint32_t width, uint32_t height,
                           uint16_t sa_w, uint16_t sa_h, svtme_dg_metrics *d_acc, svtme_dg_sb *d_sb, hipStream_t s);
hipError_t svtme_prime_tfsp(void);
hipError_t svtme_launch_tfsp(const DevPlane *cen, const DevPlane *ref, uint32_t n, uint32_t width, uint32_t height,
                             const svtme_tf_subpel_controls *ctl, const svtme_ref_record *d_rec,
                             svtme_tf_subpel_sb *d_out, hipStream_t s);
// svtme_tff.hip: temporal filtering's luma stage and, with U, its chroma stage; hbd: the 16-bit planes;
// pic: the normalisation into the result picture (Y->dst, U->dst), else into the dense planes
hipError_t svtme_prime_tff(void);
hipError_t svtme_launch_tf_stage(const TfLumaArgs *Y, const TfChromaArgs *U, int hbd, int pic, hipStream_t s);
// svtme_tfld.hip: the low-delay filter, one fused kernel; hbd: 16-bit planes, chroma: Cb and Cr too
hipError_t svtme_prime_tfld(void);
hipError_t svtme_launch_tfld(const TfldArgs *A, int hbd, int chroma, hipStream_t s);
}
