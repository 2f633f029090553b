// svtme_ctx.h — the context behind include/svtme.h and what its host files share. Internal: none
// of this is part of include/svtme.h.
//
//   svtme_ctx.cpp       error state, context create / destroy, lanes and streams, timing, host memory
//   svtme_pictures.cpp  the picture pool, pyramid builds, every upload, release, download, chroma, 10-bit luma and chroma
//   svtme_submit.cpp    job validation, the job-table ring, batch and packed submission, tickets, fetch
//   svtme_windows.cpp   the picture-window calls: svtme_dg_detect and the temporal-filter stages
//   svtme_controls.cpp  pure host code (no HIP): control derivation, the detector's reduction
//
// The helpers that take a context run with its lock held and its device current, and report
// failure as the entry points do: a status, and the message in svtme_last_error().
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <condition_variable>
#include <map>
#include <mutex>
#include <vector>

#include "svtme_controls.h"
#include "svtme_launch.h"

struct PicBuf {
    uint8_t *mem = nullptr;
    size_t bytes = 0;
    uint32_t W = 0, H = 0;
    DevPyramid pyr{};
    // attached chroma (svtme_picture_upload_chroma, svtme_tf_window_yuv): a buffer of its own, so the
    // luma geometry and svtme_reserve_pictures know nothing of it; nullptr: the picture has none
    uint8_t *cmem = nullptr;
    size_t cbytes = 0;
    DevPlane chroma[2]{}; // Cb, Cr
    // attached full-precision luma of a 10-bit picture (svtme_picture_attach_10bit, svtme_tf_window_10bit):
    // a buffer of its own as the chroma's is, 16-bit samples (svtme_hbd_geometry); nullptr: none
    uint8_t *hmem = nullptr;
    size_t hbytes = 0;
    DevPlane hbd{};
    // attached full-precision chroma of a 10-bit picture (svtme_picture_attach_chroma_10bit,
    // svtme_tf_window_yuv_10bit): a third buffer of its own, 16-bit samples (svtme_hbd_chroma_geometry)
    uint8_t *hcmem = nullptr;
    size_t hcbytes = 0;
    DevPlane hchroma[2]{}; // Cb, Cr
    hipEvent_t ready = nullptr;          // end of an asynchronous upload on the upload stream
    uint32_t pending = 0;                 // lanes whose stream has not waited on `ready` yet
    hipEvent_t used[SVTME_LANES] = {};    // end of the last submission of each lane that reads the
                                          // picture (a lane's submission event, not owned)
};

// A submission lane: a stream and the inter-stage scratch of the jobs running
// on it. Submissions on different lanes overlap on the GPU (the next one's
// workgroups fill the CUs while the previous one drains); lane 0's stream is
// the context's stream.
struct Lane {
    hipStream_t s = nullptr;
    static constexpr int kEv = 64;  // submission events, recorded round-robin: one per submission
    hipEvent_t ev[kEv] = {};
    int ev_next        = 0;
    ARes *d_ares    = nullptr; // stage-A results [count][SVTME_A_N]
    size_t ares_cap = 0;
    BState *d_bst   = nullptr; // stage-B state [count]
    size_t bst_cap  = 0;
    unsigned long long *d_keys = nullptr; // wide full-pel argmin keys [count][R][85]
    size_t keys_cap            = 0;
    bool keys_rest             = false; // every key is ~0 (banded jobs accumulate with atomic min)
    CSlot *d_cslot             = nullptr; // [count][R]
    size_t cslot_cap           = 0;
};

// An outstanding packed host-output job (svtme_submit_picture_packed_async):
// its device outputs stay allocated with the ticket slot and are reused by the
// next job that takes the slot after svtme_ticket_wait retired it.
struct Ticket {
    uint64_t id = 0;               // 0: the slot is free
    bool waiting = false;          // a thread is blocked on `done`
    hipEvent_t queued = nullptr;   // the job's turn on its lane (timing: svtme_ticket_wait_timed)
    hipEvent_t launched = nullptr; // end of the job's launches on its lane
    hipEvent_t done = nullptr;     // end of the copy into host memory (download stream)
    void *d_mem = nullptr;         // records | SB results | packed bytes
    size_t d_cap = 0;
};

struct svtme_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t ustream = nullptr; // asynchronous uploads (copy + pyramid build), created on first use
    void *ustaging = nullptr;      // their device staging plane (reused in upload-stream order)
    size_t ustaging_cap = 0;
    std::map<uint64_t, PicBuf> pics;
    // released pictures whose memory queued work may still read: freed (or reused by
    // a picture of the same size) once their upload and last readers have completed
    std::vector<PicBuf> graves;
    // idle picture buffers (released pictures whose readers have run, and those
    // svtme_reserve_pictures made), reused for pictures of the same size: no
    // hipMalloc / hipFree on the steady path
    std::vector<std::pair<size_t, uint8_t *>> freebufs;
    static constexpr size_t kMaxFree = 256;
    // page-locked staging of svtme_picture_upload_copy_async, reused in rotation
    struct UpSlot {
        void *h = nullptr;
        size_t cap = 0;
        hipEvent_t done = nullptr; // the slot's last DMA has run
        bool busy = false;         // a thread is filling it
        bool queued = false;       // `done` marks a DMA
    };
    UpSlot up[SVTME_UPLOAD_SLOTS];
    uint32_t up_next = 0;
    void *staging      = nullptr;
    size_t staging_cap = 0;
    svtme_ref_record *d_records = nullptr;
    size_t records_cap          = 0;
    svtme_sb_result *d_sb       = nullptr;
    size_t sb_cap               = 0;
    void *d_dg    = nullptr; // svtme_dg_detect: n metrics slots | n x SBs per-SB results
    size_t dg_cap = 0;
    void *d_tfsp    = nullptr; // svtme_tf_subpel: n x SBs records | n x SBs results
    size_t tfsp_cap = 0;
    void *d_tff     = nullptr; // the temporal filter's scratch (TfScratch, svtme_windows.cpp)
    size_t tff_cap  = 0;
    uint32_t last_count = 0, last_R = 0;
    bool last_has_sb    = false;
    // job tables: a ring of device slots of SVTME_MAX_BATCH DevJobs, copied from
    // pinned host memory on the job stream (in order: a slot is only rewritten
    // after every kernel queued before has read it); a table identical to the
    // last one published is reused without a copy
    static constexpr int kRing = 16;
    DevJob *d_table = nullptr, *h_table = nullptr, *h_table_dev = nullptr;
    hipEvent_t ring_copied[kRing] = {}; // the copy out of the pinned slot has run
    hipEvent_t ring_read[kRing] = {};   // end of the last submission that read the slot (not owned)
    bool ring_used[kRing] = {};
    uint32_t ring_n[kRing] = {};
    int ring_next = 0;
    // timing: start/stop events of every stage launch of every launch group
    // while enabled (attached to the dispatch packets: hipExtLaunchKernelGGL)
    static constexpr int kTimeSets = 256;
    bool timing = false;
    // uploads from page-locked host memory build the pyramid from the host plane itself
    // over PCIe (no DMA into a staging plane); SVTME_UPLOAD_ZERO_COPY=0: DMA + build
    bool zero_copy = true;
    hipEvent_t tev[kTimeSets][10] = {};
    uint32_t tmask[kTimeSets] = {};
    int t_pending = 0;
    uint32_t t_dropped = 0;
    Lane lanes[SVTME_LANES]; // lanes[0].s == stream
    uint32_t paths = 0;      // SVTME_PATH_* (svtme_set_paths; the environment at creation)
    Ticket tickets[SVTME_MAX_TICKETS];
    uint64_t ticket_seq = 0;
    hipStream_t dstream = nullptr; // packed outputs to host memory, created on first use
    std::mutex mu;
    std::condition_variable retired; // a ticket was retired (svtme_ticket_wait)
    std::condition_variable up_free; // a staging slot of svtme_picture_upload_copy_async was released
};

#define HIP_TRY(expr)                                                                                               \
    do {                                                                                                            \
        hipError_t _e = (expr);                                                                                     \
        if (_e != hipSuccess)                                                                                       \
            return svtme_host::fail(SVTME_ERR_UNDEFINED, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),    \
                                    __FILE__, __LINE__);                                                            \
    } while (0)

// The helpers the host files share. Hidden: they add nothing to the library's dynamic symbols.
namespace svtme_host __attribute__((visibility("hidden"))) {

// ---- svtme_ctx.cpp ----
svtme_status fail(svtme_status st, const char *fmt, ...);    // sets svtme_last_error(), prints it, returns `st`
svtme_status ensure_buf(void **p, size_t *cap, size_t need); // a device buffer of at least `need` bytes
svtme_status ensure_lane(svtme_ctx *c, uint32_t lane);
svtme_status ensure_ustream(svtme_ctx *c);
svtme_status quiesce(svtme_ctx *c); // no stream still uses any picture's memory
// A submission's done event: the lane's next event, recorded behind what the call queued on its
// stream. mark_read points the pictures the call read at it: a later upload, rebuild or release
// of one of them waits for these launches only.
inline svtme_status submission_done(Lane &L, hipEvent_t *done) {
    *done     = L.ev[L.ev_next];
    L.ev_next = (L.ev_next + 1) % Lane::kEv;
    HIP_TRY(hipEventRecord(*done, L.s));
    return SVTME_OK;
}
inline void mark_read(PicBuf *const *pb, uint32_t n, uint32_t lane, hipEvent_t done) {
    for (uint32_t k = 0; k < n; k++) pb[k]->used[lane] = done;
}

// ---- svtme_pictures.cpp ----
constexpr uint32_t kAllLanes = (1u << SVTME_LANES) - 1u;
// lane `lane`'s stream waits for a picture's asynchronous upload (once per upload)
inline svtme_status join_upload(svtme_ctx *c, PicBuf &pb, int lane) {
    if ((pb.pending >> lane) & 1u) {
        HIP_TRY(hipStreamWaitEvent(c->lanes[lane].s, pb.ready, 0));
        pb.pending &= ~(1u << lane);
    }
    return SVTME_OK;
}
svtme_status after_readers(svtme_ctx *c, PicBuf &pb, hipStream_t s); // `s` waits for the other lanes' readers
// `pb`, written on `s` (its `ready` exists): the lanes of `lanes` wait for that before they read it
svtme_status upload_publish(PicBuf &pb, hipStream_t s, uint32_t lanes);
svtme_status alloc_pic(svtme_ctx *c, uint64_t pn, uint32_t W, uint32_t H, PicBuf **out, bool keep_chroma = false,
                       bool keep_hbd = false, bool keep_hbd_chroma = false);
svtme_status alloc_chroma(svtme_ctx *c, PicBuf &pb);
svtme_status alloc_hbd(svtme_ctx *c, PicBuf &pb);
svtme_status alloc_hbd_chroma(svtme_ctx *c, PicBuf &pb);
// one padded 16-bit chroma plane from cw x ch true samples on the device (dsrc may be the plane's own interior)
svtme_status build_hbd_chroma(const PicBuf *pb, int plane, const uint16_t *dsrc, uint32_t src_stride, uint32_t cw,
                              uint32_t ch, hipStream_t st);
// the padded 16-bit plane from w x h true samples on the device (dsrc may be the plane's own interior)
svtme_status build_hbd(const PicBuf *pb, const uint16_t *dsrc, uint32_t src_stride, uint32_t w, uint32_t h,
                       hipStream_t st);
svtme_status build_pyramid(svtme_ctx *c, PicBuf *pb, const void *dsrc, uint32_t src_stride, uint32_t w, uint32_t h,
                           int ten_bit, hipStream_t st = nullptr);
svtme_status build_chroma(const PicBuf *pb, int plane, const void *dsrc, uint32_t src_stride, uint32_t cw,
                          uint32_t ch, hipStream_t st);

// ---- svtme_submit.cpp ----
svtme_status ensure_ring(svtme_ctx *c);
svtme_status submit_batch_locked(svtme_ctx *c, const svtme_job *jobs, uint32_t n, svtme_ref_record *const *out,
                                 svtme_sb_result *const *out_sb, bool with_sb, uint32_t lane = 0);

inline PicBuf *find_pic(svtme_ctx *c, uint64_t pn) {
    auto it = c->pics.find(pn);
    return it == c->pics.end() ? nullptr : &it->second;
}
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

} // namespace svtme_host
