// svtme_ctx.cpp — the context of the C ABI of include/svtme.h on HIP (gfx950 / MI355X): the
// per-thread error state, context creation and destruction, the submission lanes with their
// streams and done events, stage timing and page-locked host memory. No CPU fallback anywhere:
// a HIP failure returns an error status and sets svtme_last_error().
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "svtme_ctx.h"

using namespace svtme_host;

// ---- errors ----
static thread_local std::string g_last_error;

extern "C" const char *svtme_last_error(void) { return g_last_error.c_str(); }

// used by the rtcd variants (svtme_rtcd.hip), which return void
extern "C" void svtme_set_error_internal(const char *msg) {
    g_last_error = msg;
    fprintf(stderr, "[svtme] %s\n", msg);
}

svtme_status svtme_host::fail(svtme_status st, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    svtme_set_error_internal(buf);
    return st;
}

// ---- lanes and streams ----
svtme_status svtme_host::ensure_lane(svtme_ctx *c, uint32_t lane) {
    if (lane >= SVTME_LANES)
        return fail(SVTME_ERR_BAD_PARAMETER, "lane %u (0..%d)", lane, SVTME_LANES - 1);
    Lane &L = c->lanes[lane];
    if (!L.s)
        HIP_TRY(hipStreamCreateWithFlags(&L.s, hipStreamNonBlocking));
    if (!L.ev[0])
        for (auto &e : L.ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return SVTME_OK;
}

svtme_status svtme_host::ensure_ustream(svtme_ctx *c) {
    if (!c->ustream) { // high priority: its small pyramid kernels go ahead of queued search workgroups
        int lo = 0, hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIP_TRY(hipStreamCreateWithPriority(&c->ustream, hipStreamNonBlocking, hi));
    }
    return SVTME_OK;
}

svtme_status svtme_host::quiesce(svtme_ctx *c) {
    for (auto &L : c->lanes)
        if (L.s)
            HIP_TRY(hipStreamSynchronize(L.s));
    if (c->ustream)
        HIP_TRY(hipStreamSynchronize(c->ustream));
    return SVTME_OK;
}

svtme_status svtme_host::ensure_buf(void **p, size_t *cap, size_t need) {
    if (*cap >= need)
        return SVTME_OK;
    if (*p)
        HIP_TRY(hipFree(*p));
    *p   = nullptr;
    *cap = 0;
    HIP_TRY(hipMalloc(p, need));
    *cap = need;
    return SVTME_OK;
}

extern "C" void *svtme_stream(svtme_ctx *c) { return c ? (void *)c->stream : nullptr; }

extern "C" void *svtme_lane_stream(svtme_ctx *c, uint32_t lane) {
    if (!c)
        return nullptr;
    std::lock_guard<std::mutex> lk(c->mu);
    if (hipSetDevice(c->device) != hipSuccess || ensure_lane(c, lane))
        return nullptr;
    return (void *)c->lanes[lane].s;
}

extern "C" void *svtme_upload_stream(svtme_ctx *c) {
    if (!c)
        return nullptr;
    std::lock_guard<std::mutex> lk(c->mu);
    if (hipSetDevice(c->device) != hipSuccess || ensure_ustream(c))
        return nullptr;
    return (void *)c->ustream;
}

// ---- context ----
// The streams, events and job-table ring of a context, made at creation so
// that no job's latency carries them
static svtme_status prepare(svtme_ctx *c) {
    svtme_status st;
    for (uint32_t l = 0; l < SVTME_LANES; l++)
        if ((st = ensure_lane(c, l)))
            return st;
    if ((st = ensure_ustream(c)) || (st = ensure_ring(c)))
        return st;
    HIP_TRY(hipStreamCreateWithFlags(&c->dstream, hipStreamNonBlocking));
    for (auto &t : c->tickets) { // timing events: svtme_ticket_wait_timed
        HIP_TRY(hipEventCreate(&t.queued));
        HIP_TRY(hipEventCreate(&t.launched));
        HIP_TRY(hipEventCreate(&t.done));
    }
    // The first work on a stream and the first large copy in each direction cost
    // milliseconds of one-time runtime setup (the first packed job's D2H copy call
    // took 6.8 ms in a HIP API trace, later ones 10 us; small copies take another
    // path and do not set it up): a fill on every stream and a 4 MB copy each way
    // on the upload and download streams happen here, at context creation.
    void *d = nullptr, *h = nullptr;
    const size_t wb = (size_t)4 << 20;
    HIP_TRY(hipMalloc(&d, wb));
    HIP_TRY(hipHostMalloc(&h, wb, hipHostMallocDefault));
    for (uint32_t l = 0; l < SVTME_LANES; l++) HIP_TRY(hipMemsetAsync(d, 0, 256, c->lanes[l].s));
    HIP_TRY(hipMemsetAsync(d, 0, 256, c->ustream));
    HIP_TRY(hipMemcpyAsync(d, h, wb, hipMemcpyHostToDevice, c->ustream));
    HIP_TRY(hipStreamSynchronize(c->ustream));
    HIP_TRY(hipMemcpyAsync(h, d, wb, hipMemcpyDeviceToHost, c->dstream));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipFree(d));
    HIP_TRY(hipHostFree(h));
    return SVTME_OK;
}

extern "C" svtme_status svtme_ctx_create(int device, svtme_ctx **out) {
    if (!out)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_ctx_create: null out");
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_ctx_create: device %d of %d", device, n);
    HIP_TRY(hipSetDevice(device));
    svtme_ctx *c = new svtme_ctx();
    c->device    = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(SVTME_ERR_INSUFFICIENT_RESOURCES, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    c->lanes[0].s = c->stream;
    // the code objects of the kernels, loaded now rather than at a first job's launches
    if ((e = svtme_prime_pyramid()) != hipSuccess || (e = svtme_prime_pack()) != hipSuccess ||
        (e = svtme_prime_stages()) != hipSuccess || (e = svtme_prime_dg()) != hipSuccess ||
        (e = svtme_prime_tfsp()) != hipSuccess || (e = svtme_prime_tff()) != hipSuccess ||
        (e = svtme_prime_tfld()) != hipSuccess) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return fail(SVTME_ERR_UNDEFINED, "svtme_ctx_create: loading the kernels: %s", hipGetErrorString(e));
    }
    // kernel-path selection from the environment, read once (diagnostic A/B runs)
    static const struct {
        const char *var;
        uint32_t bit;
    } env_paths[] = {{"SVTME_NO_FUSED_HME", SVTME_PATH_NO_FUSED_HME}, {"SVTME_NO_L1_FULL", SVTME_PATH_NO_L1_FULL},
                     {"SVTME_NO_L0_FULL", SVTME_PATH_NO_L0_FULL},       {"SVTME_NO_FP_WIDE", SVTME_PATH_NO_FP_WIDE},
                     {"SVTME_SPLIT_PASS", SVTME_PATH_SPLIT_PASS},     {"SVTME_NO_A1_GATE", SVTME_PATH_NO_A1_GATE},
                     {"SVTME_HME_4WAVES", SVTME_PATH_HME_4WAVES}};
    for (const auto &e : env_paths)
        if (const char *v = getenv(e.var))
            if (*v && strcmp(v, "0") != 0)
                c->paths |= e.bit;
    if (const char *v = getenv("SVTME_UPLOAD_ZERO_COPY"))
        c->zero_copy = !(*v && strcmp(v, "0") == 0);
    const svtme_status ps = prepare(c);
    if (ps) {
        svtme_ctx_destroy(c);
        return ps;
    }
    *out = c;
    return SVTME_OK;
}

extern "C" svtme_status svtme_set_paths(svtme_ctx *c, uint32_t paths) {
    if (!c || (paths & ~127u))
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_set_paths: null ctx or unknown path bits 0x%x", paths);
    std::lock_guard<std::mutex> lk(c->mu);
    c->paths = paths;
    return SVTME_OK;
}

static void free_pic(PicBuf &pb) {
    (void)hipFree(pb.mem);
    if (pb.cmem)
        (void)hipFree(pb.cmem);
    if (pb.hmem)
        (void)hipFree(pb.hmem);
    if (pb.hcmem)
        (void)hipFree(pb.hcmem);
    if (pb.ready)
        (void)hipEventDestroy(pb.ready);
}

extern "C" void svtme_ctx_destroy(svtme_ctx *c) {
    if (!c)
        return;
    (void)hipSetDevice(c->device);
    for (auto &L : c->lanes)
        if (L.s)
            (void)hipStreamSynchronize(L.s);
    if (c->ustream)
        (void)hipStreamSynchronize(c->ustream);
    for (auto &kv : c->pics) free_pic(kv.second);
    for (auto &g : c->graves) free_pic(g);
    for (auto &f : c->freebufs)
        (void)hipFree(f.second);
    for (auto &u : c->up) {
        if (u.h)
            (void)hipHostFree(u.h);
        if (u.done)
            (void)hipEventDestroy(u.done);
    }
    // (hipFree of a null pointer does nothing)
    for (void *p : {c->staging, c->ustaging, (void *)c->d_records, (void *)c->d_sb, c->d_dg, c->d_tfsp, c->d_tff})
        (void)hipFree(p);
    for (auto &set : c->tev)
        for (auto &e : set)
            if (e)
                (void)hipEventDestroy(e);
    for (int k = 0; k < svtme_ctx::kRing; k++)
        if (c->ring_copied[k])
            (void)hipEventDestroy(c->ring_copied[k]);
    if (c->dstream)
        (void)hipStreamSynchronize(c->dstream);
    for (auto &t : c->tickets) {
        (void)hipFree(t.d_mem);
        for (hipEvent_t e : {t.launched, t.queued, t.done})
            if (e)
                (void)hipEventDestroy(e);
    }
    if (c->dstream)
        (void)hipStreamDestroy(c->dstream);
    (void)hipFree(c->d_table);
    if (c->h_table)
        (void)hipHostFree(c->h_table);
    for (int l = 0; l < SVTME_LANES; l++) {
        Lane &L = c->lanes[l];
        for (void *p : {(void *)L.d_ares, (void *)L.d_bst, (void *)L.d_keys, (void *)L.d_cslot})
            (void)hipFree(p);
        for (auto &e : L.ev)
            if (e)
                (void)hipEventDestroy(e);
        if (l > 0 && L.s)
            (void)hipStreamDestroy(L.s);
    }
    (void)hipStreamDestroy(c->stream);
    if (c->ustream)
        (void)hipStreamDestroy(c->ustream);
    delete c;
}

// ---- stage timing ----
extern "C" svtme_status svtme_set_timing(svtme_ctx *c, int enable) {
    if (!c)
        return fail(SVTME_ERR_BAD_PARAMETER, "null ctx");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (enable && !c->tev[0][0])
        for (auto &set : c->tev)
            for (auto &e : set) HIP_TRY(hipEventCreate(&e));
    c->timing = enable != 0;
    return SVTME_OK;
}

extern "C" uint32_t svtme_timing_read(svtme_ctx *c, float stage_ms[5]) {
    if (!c || !stage_ms)
        return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    double sum[5] = {0, 0, 0, 0, 0};
    uint32_t launches[5] = {0, 0, 0, 0, 0};
    const int n = c->t_pending;
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 5; k++) {
            if (!((c->tmask[i] >> k) & 1u))
                continue;
            float ms = 0.0f;
            if (hipEventSynchronize(c->tev[i][2 * k + 1]) != hipSuccess ||
                hipEventElapsedTime(&ms, c->tev[i][2 * k], c->tev[i][2 * k + 1]) != hipSuccess)
                return 0;
            sum[k] += ms;
            launches[k]++;
        }
    // each stage is averaged over the launch groups that ran it
    for (int k = 0; k < 5; k++) stage_ms[k] = launches[k] ? (float)(sum[k] / launches[k]) : 0.0f;
    if (c->t_dropped)
        svtme_set_error_internal("svtme_timing_read: launch groups beyond the timing capacity were not recorded");
    c->t_pending = 0;
    c->t_dropped = 0;
    return (uint32_t)n;
}

// ---- page-locked host memory ----
extern "C" void *svtme_host_alloc(uint64_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? (size_t)bytes : 1, hipHostMallocDefault) != hipSuccess) {
        svtme_set_error_internal("svtme_host_alloc: hipHostMalloc failed");
        return nullptr;
    }
    return p;
}

extern "C" void svtme_host_free(void *p) {
    if (p)
        (void)hipHostFree(p);
}

extern "C" svtme_status svtme_host_register(void *p, uint64_t bytes) {
    if (!p || !bytes)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_host_register: bad arguments");
    HIP_TRY(hipHostRegister(p, (size_t)bytes, hipHostRegisterDefault));
    return SVTME_OK;
}

extern "C" svtme_status svtme_host_unregister(void *p) {
    if (!p)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_host_unregister: null pointer");
    HIP_TRY(hipHostUnregister(p));
    return SVTME_OK;
}
