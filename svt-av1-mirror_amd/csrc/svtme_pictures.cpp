// svtme_pictures.cpp — the resident pictures of a context: their pool, the pyramid builds, every
// upload, invalidate, release, download, and the attached chroma planes. A picture is written on
// one stream and read on others: a writer waits for the readers queued on the other lanes
// (after_readers), a lane waits once for an asynchronous write before it reads (upload_publish,
// join_upload), and memory that queued work may still read rests in the graves meanwhile.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "svtme_ctx.h"

using namespace svtme_host;

// `s` waits for every launch of the other lanes already queued that reads the picture
svtme_status svtme_host::after_readers(svtme_ctx *c, PicBuf &pb, hipStream_t s) {
    for (int l = 0; l < SVTME_LANES; l++)
        if (pb.used[l] && c->lanes[l].s != s)
            HIP_TRY(hipStreamWaitEvent(s, pb.used[l], 0));
    return SVTME_OK;
}

svtme_status svtme_host::upload_publish(PicBuf &pb, hipStream_t s, uint32_t lanes) {
    HIP_TRY(hipEventRecord(pb.ready, s));
    pb.pending = lanes;
    return SVTME_OK;
}

// ---- the pool ----
// a released picture's memory is idle: its upload and its lanes' last readers have run
// (a lane's event may since mark a later submission: later, never early)
static bool grave_idle(const PicBuf &g) {
    if (g.ready && hipEventQuery(g.ready) != hipSuccess)
        return false;
    for (int l = 0; l < SVTME_LANES; l++)
        if (g.used[l] && hipEventQuery(g.used[l]) != hipSuccess)
            return false;
    return true;
}
// an idle buffer of exactly `bytes` from the free pool, or nullptr
static uint8_t *take_free(svtme_ctx *c, size_t bytes) {
    for (size_t i = 0; i < c->freebufs.size(); i++)
        if (c->freebufs[i].first == bytes) {
            uint8_t *m     = c->freebufs[i].second;
            c->freebufs[i] = c->freebufs.back();
            c->freebufs.pop_back();
            return m;
        }
    return nullptr;
}
// an idle buffer goes to the free pool; beyond kMaxFree buffers it goes back to HIP
static void give_free(svtme_ctx *c, size_t bytes, uint8_t *m) {
    if (c->freebufs.size() < svtme_ctx::kMaxFree)
        c->freebufs.emplace_back(bytes, m);
    else
        (void)hipFree(m);
}
// move the idle released pictures' memory to the free pool; with want > 0, return one idle
// buffer of exactly `want` bytes instead
static uint8_t *sweep_graves(svtme_ctx *c, size_t want) {
    uint8_t *keep = nullptr;
    for (size_t i = 0; i < c->graves.size();) {
        PicBuf &g = c->graves[i];
        if (!grave_idle(g)) {
            i++;
            continue;
        }
        if (g.ready)
            (void)hipEventDestroy(g.ready);
        if (!keep && want && g.bytes == want)
            keep = g.mem;
        else
            give_free(c, g.bytes, g.mem);
        if (g.cmem) // the chroma attached to a released picture goes with it
            give_free(c, g.cbytes, g.cmem);
        if (g.hmem) // the 16-bit plane likewise
            give_free(c, g.hbytes, g.hmem);
        if (g.hcmem) // and the 16-bit chroma
            give_free(c, g.hcbytes, g.hcmem);
        c->graves[i] = c->graves.back();
        c->graves.pop_back();
    }
    return keep;
}

// bytes of a W x H picture's three padded planes in one buffer, and their offsets
static size_t pic_bytes(uint32_t W, uint32_t H, size_t offs[3] = nullptr) {
    size_t total = 0;
    for (int lv = 0; lv < 3; lv++) {
        uint32_t w, h, left, top, stride, rows, pad;
        svtme_plane_geometry(lv, W, H, &w, &h, &left, &top, &stride, &rows, &pad);
        if (offs)
            offs[lv] = total;
        total = align256(total + (size_t)stride * rows);
    }
    return total + 1024; // slack: search-window loads may read a few dwords past the last row
}

// device memory for a picture: the free pool, an idle released picture, or HIP;
// when HIP is out of memory, wait for the released pictures' readers, give every
// idle buffer back and try once more
static svtme_status pic_mem(svtme_ctx *c, size_t total, uint8_t **out) {
    if ((*out = take_free(c, total)) || (*out = sweep_graves(c, total)))
        return SVTME_OK;
    if (hipMalloc((void **)out, total) == hipSuccess)
        return SVTME_OK;
    (void)hipGetLastError();
    for (auto &g : c->graves) {
        if (g.ready)
            HIP_TRY(hipEventSynchronize(g.ready));
        for (int l = 0; l < SVTME_LANES; l++)
            if (g.used[l])
                HIP_TRY(hipEventSynchronize(g.used[l]));
    }
    (void)sweep_graves(c, 0);
    for (auto &f : c->freebufs)
        HIP_TRY(hipFree(f.second));
    c->freebufs.clear();
    HIP_TRY(hipMalloc((void **)out, total));
    return SVTME_OK;
}

// bytes of the two padded chroma planes of a W x H picture in one buffer, and the second's offset
static size_t chroma_bytes(uint32_t W, uint32_t H, size_t *second = nullptr) {
    uint32_t w, h, left, top, stride, rows;
    svtme_chroma_geometry(W, H, &w, &h, &left, &top, &stride, &rows);
    const size_t one = align256((size_t)stride * rows);
    if (second)
        *second = one;
    return 2 * one + 256;
}

// The picture's luma is about to be replaced: its chroma no longer belongs to it. The buffer goes to
// the graves with the picture's reader events (work queued earlier may still read it).
static void drop_chroma(svtme_ctx *c, PicBuf &pb) {
    if (!pb.cmem)
        return;
    PicBuf g;
    g.mem = pb.cmem, g.bytes = pb.cbytes;
    for (int l = 0; l < SVTME_LANES; l++) g.used[l] = pb.used[l];
    c->graves.push_back(g);
    pb.cmem = nullptr, pb.cbytes = 0;
    pb.chroma[0] = pb.chroma[1] = DevPlane{};
}

// chroma planes for a resident picture that has none (contents undefined until written)
svtme_status svtme_host::alloc_chroma(svtme_ctx *c, PicBuf &pb) {
    if (pb.cmem)
        return SVTME_OK;
    size_t second;
    const size_t total = chroma_bytes(pb.W, pb.H, &second);
    svtme_status st    = pic_mem(c, total, &pb.cmem);
    if (st)
        return st;
    pb.cbytes = total;
    uint32_t w, h, left, top, stride, rows;
    svtme_chroma_geometry(pb.W, pb.H, &w, &h, &left, &top, &stride, &rows);
    for (int p = 0; p < 2; p++)
        pb.chroma[p] = DevPlane{pb.cmem + p * second + (size_t)top * stride + left, (int32_t)stride, (int32_t)w,
                                (int32_t)h, SVTME_PAD_CHROMA};
    return SVTME_OK;
}

// bytes of the padded 16-bit plane of a W x H picture
static size_t hbd_bytes(uint32_t W, uint32_t H) {
    uint32_t left, top, stride, rows;
    svtme_hbd_geometry(W, H, &left, &top, &stride, &rows);
    return align256((size_t)stride * rows) + 256; // slack: the staging's aligned dword pairs end inside the row
}

// The picture's luma is about to be replaced: its 16-bit plane no longer belongs to it (drop_chroma's way)
static void drop_hbd(svtme_ctx *c, PicBuf &pb) {
    if (!pb.hmem)
        return;
    PicBuf g;
    g.mem = pb.hmem, g.bytes = pb.hbytes;
    for (int l = 0; l < SVTME_LANES; l++) g.used[l] = pb.used[l];
    c->graves.push_back(g);
    pb.hmem = nullptr, pb.hbytes = 0;
    pb.hbd = DevPlane{};
}

// a 16-bit plane for a resident picture that has none (contents undefined until written)
svtme_status svtme_host::alloc_hbd(svtme_ctx *c, PicBuf &pb) {
    if (pb.hmem)
        return SVTME_OK;
    const size_t total = hbd_bytes(pb.W, pb.H);
    svtme_status st    = pic_mem(c, total, &pb.hmem);
    if (st)
        return st;
    pb.hbytes = total;
    uint32_t left, top, stride, rows;
    svtme_hbd_geometry(pb.W, pb.H, &left, &top, &stride, &rows);
    pb.hbd = DevPlane{pb.hmem + (size_t)top * stride + (size_t)left * 2, (int32_t)stride, (int32_t)pb.W, (int32_t)pb.H,
                      SVTME_PAD_FULL};
    return SVTME_OK;
}

// bytes of the two padded 16-bit chroma planes of a W x H picture in one buffer, and the second's offset
static size_t hbd_chroma_bytes(uint32_t W, uint32_t H, size_t *second = nullptr) {
    uint32_t w, h, left, top, stride, rows;
    svtme_hbd_chroma_geometry(W, H, &w, &h, &left, &top, &stride, &rows);
    const size_t one = align256((size_t)stride * rows);
    if (second)
        *second = one;
    return 2 * one + 256; // slack: the staging's aligned dword pairs end inside the row
}

// The picture's luma is about to be replaced: its 16-bit chroma no longer belongs to it (drop_chroma's way)
static void drop_hbd_chroma(svtme_ctx *c, PicBuf &pb) {
    if (!pb.hcmem)
        return;
    PicBuf g;
    g.mem = pb.hcmem, g.bytes = pb.hcbytes;
    for (int l = 0; l < SVTME_LANES; l++) g.used[l] = pb.used[l];
    c->graves.push_back(g);
    pb.hcmem = nullptr, pb.hcbytes = 0;
    pb.hchroma[0] = pb.hchroma[1] = DevPlane{};
}

// 16-bit chroma planes for a resident picture that has none (contents undefined until written)
svtme_status svtme_host::alloc_hbd_chroma(svtme_ctx *c, PicBuf &pb) {
    if (pb.hcmem)
        return SVTME_OK;
    size_t second;
    const size_t total = hbd_chroma_bytes(pb.W, pb.H, &second);
    svtme_status st    = pic_mem(c, total, &pb.hcmem);
    if (st)
        return st;
    pb.hcbytes = total;
    uint32_t w, h, left, top, stride, rows;
    svtme_hbd_chroma_geometry(pb.W, pb.H, &w, &h, &left, &top, &stride, &rows);
    for (int p = 0; p < 2; p++)
        pb.hchroma[p] = DevPlane{pb.hcmem + p * second + (size_t)top * stride + (size_t)left * 2, (int32_t)stride,
                                 (int32_t)w, (int32_t)h, SVTME_PAD_CHROMA};
    return SVTME_OK;
}

// allocate the three planes of a W x H picture in one buffer; chroma, the 16-bit plane and the 16-bit
// chroma attached to an earlier picture of the number are dropped unless the caller writes them too
// (svtme_tf_window_yuv, svtme_tf_window_10bit, svtme_tf_window_yuv_10bit)
svtme_status svtme_host::alloc_pic(svtme_ctx *c, uint64_t pn, uint32_t W, uint32_t H, PicBuf **out,
                                   bool keep_chroma, bool keep_hbd, bool keep_hbd_chroma) {
    auto it = c->pics.find(pn);
    if (it != c->pics.end() && it->second.W == W && it->second.H == H && !keep_chroma)
        drop_chroma(c, it->second);
    if (it != c->pics.end() && it->second.W == W && it->second.H == H && !keep_hbd)
        drop_hbd(c, it->second);
    if (it != c->pics.end() && it->second.W == W && it->second.H == H && !keep_hbd_chroma)
        drop_hbd_chroma(c, it->second);
    if (it != c->pics.end() && (it->second.W != W || it->second.H != H)) {
        // a new size: the old buffer goes to the graves (freed for reuse once its readers ran)
        c->graves.push_back(it->second);
        c->pics.erase(it);
        it = c->pics.end();
    }
    size_t offs[3];
    const size_t total = pic_bytes(W, H, offs);
    if (it == c->pics.end()) {
        PicBuf pb;
        svtme_status ms = pic_mem(c, total, &pb.mem);
        if (ms)
            return ms;
        pb.bytes = total;
        pb.W = W, pb.H = H;
        it = c->pics.emplace(pn, pb).first;
    }
    PicBuf &pb = it->second;
    for (int lv = 0; lv < 3; lv++) {
        uint32_t w, h, left, top, stride, rows, pad;
        svtme_plane_geometry(lv, W, H, &w, &h, &left, &top, &stride, &rows, &pad);
        pb.pyr.lv[lv] = DevPlane{pb.mem + offs[lv] + (size_t)top * stride + left, (int32_t)stride, (int32_t)w,
                                 (int32_t)h, (int32_t)pad};
    }
    *out = &pb;
    return SVTME_OK;
}

extern "C" svtme_status svtme_reserve_pictures(svtme_ctx *c, uint32_t width, uint32_t height, uint32_t count) {
    if (!c || width == 0 || height == 0 || count > 4096)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_reserve_pictures: bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = pic_bytes(svtme_align8_u(width), svtme_align8_u(height));
    uint32_t have      = 0;
    for (auto &f : c->freebufs)
        have += f.first == bytes;
    for (; have < count && c->freebufs.size() < svtme_ctx::kMaxFree; have++) {
        uint8_t *m = nullptr;
        HIP_TRY(hipMalloc((void **)&m, bytes));
        c->freebufs.emplace_back(bytes, m);
    }
    return SVTME_OK;
}

// ---- pyramid builds ----
svtme_status svtme_host::build_pyramid(svtme_ctx *c, PicBuf *pb, const void *dsrc, uint32_t src_stride, uint32_t w,
                                       uint32_t h, int ten_bit, hipStream_t st) {
    if (!st)
        st = c->stream;
    uint32_t pw, ph, left, top, stride, rows, pad;
    svtme_plane_geometry(0, pb->W, pb->H, &pw, &ph, &left, &top, &stride, &rows, &pad);
    HIP_TRY(svtme_launch_build_full(dsrc, src_stride, (int)w, (int)h, ten_bit, pb->pyr.lv[0], (int)left, (int)top,
                                    (int)rows, st));
    for (int lv = 1; lv < 3; lv++) {
        svtme_plane_geometry(lv, pb->W, pb->H, &pw, &ph, &left, &top, &stride, &rows, &pad);
        HIP_TRY(svtme_launch_build_down(pb->pyr.lv[lv - 1], pb->pyr.lv[lv], (int)left, (int)top, (int)rows, st));
    }
    return SVTME_OK;
}

// The device address of a page-locked host range (hipHostMalloc / hipHostRegister),
// or null for pageable memory (then a DMA through a staging plane is needed)
static const uint8_t *device_view(const svtme_ctx *c, const void *y) {
    if (!c->zero_copy)
        return nullptr;
    hipPointerAttribute_t pa;
    if (hipPointerGetAttributes(&pa, y) != hipSuccess) {
        (void)hipGetLastError(); // (pageable memory reads as an error)
        return nullptr;
    }
    if (pa.type != hipMemoryTypeHost || !pa.devicePointer)
        return nullptr;
    return (const uint8_t *)pa.devicePointer + (pa.hostPointer ? ((const uint8_t *)y - (const uint8_t *)pa.hostPointer) : 0);
}

// the pyramid of an 8-bit plane the device reads in page-locked host memory: the
// interior of level 0 streamed over PCIe by a few workgroups (svtme_launch_host_rows),
// then the padding and the lower levels from it, on device
static svtme_status build_pyramid_host(svtme_ctx *c, PicBuf *pb, const uint8_t *dv, uint32_t stride, uint32_t w,
                                       uint32_t h, hipStream_t st) {
    const DevPlane &p0 = pb->pyr.lv[0];
    HIP_TRY(svtme_launch_host_rows(dv, stride, (int)w, (int)h, p0.base, (uint32_t)p0.stride, st));
    return build_pyramid(c, pb, p0.base, (uint32_t)p0.stride, w, h, 0, st);
}
// zero-copy needs dword-aligned rows (the stream kernel's loads and stores)
static bool zero_copy_ok(const void *y, uint32_t stride, const PicBuf *pb) {
    return (((uintptr_t)y | stride | (uintptr_t)pb->pyr.lv[0].base | (uint32_t)pb->pyr.lv[0].stride) & 3) == 0;
}

// ---- synchronous uploads: on the context's stream, drained before the call returns ----
// `y`: a host plane (8-bit, or 10-bit in 16-bit samples), or with `on_device` an 8-bit device plane
static svtme_status upload_sync(const char *fn, svtme_ctx *c, uint64_t pn, const void *y, uint32_t stride, uint32_t w,
                                uint32_t h, int ten_bit, bool on_device) {
    if (!c || !y || w == 0 || h == 0 || stride < w)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: bad arguments", fn);
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t bpp = ten_bit ? 2 : 1;
    const uint8_t *dv  = ten_bit || on_device ? nullptr : device_view(c, y); // page-locked: read in place
    svtme_status st;
    PicBuf *pb;
    if ((st = alloc_pic(c, pn, svtme_align8_u(w), svtme_align8_u(h), &pb)))
        return st;
    if (dv && !zero_copy_ok(y, stride, pb))
        dv = nullptr;
    if (!dv && !on_device) {
        if ((st = ensure_buf(&c->staging, &c->staging_cap, (size_t)w * h * bpp)))
            return st;
        HIP_TRY(hipMemcpy2DAsync(c->staging, (size_t)w * bpp, y, (size_t)stride * bpp, (size_t)w * bpp, h,
                                 hipMemcpyHostToDevice, c->stream));
        y = c->staging, stride = w;
    }
    if ((st = join_upload(c, *pb, 0)) || (st = after_readers(c, *pb, c->stream)))
        return st;
    if ((st = dv ? build_pyramid_host(c, pb, dv, stride, w, h, c->stream) : build_pyramid(c, pb, y, stride, w, h, ten_bit)))
        return st;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SVTME_OK;
}

extern "C" svtme_status svtme_picture_upload(svtme_ctx *c, uint64_t pn, const uint8_t *y, uint32_t stride, uint32_t w,
                                             uint32_t h) {
    return upload_sync("svtme_picture_upload", c, pn, y, stride, w, h, 0, false);
}

extern "C" svtme_status svtme_picture_upload_10bit(svtme_ctx *c, uint64_t pn, const uint16_t *y, uint32_t stride,
                                                   uint32_t w, uint32_t h) {
    return upload_sync("svtme_picture_upload_10bit", c, pn, y, stride, w, h, 1, false);
}

extern "C" svtme_status svtme_picture_upload_device(svtme_ctx *c, uint64_t pn, const uint8_t *d_y, uint32_t stride,
                                                    uint32_t w, uint32_t h) {
    return upload_sync("svtme_picture_upload_device", c, pn, d_y, stride, w, h, 0, true);
}

extern "C" svtme_status svtme_picture_invalidate(svtme_ctx *c, uint64_t pn, const uint8_t *y, uint32_t stride,
                                                 uint32_t w, uint32_t h) {
    if (!c)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_invalidate: null ctx");
    {
        std::lock_guard<std::mutex> lk(c->mu);
        const PicBuf *pb = find_pic(c, pn);
        if (!pb)
            return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_invalidate: picture %llu not resident",
                        (unsigned long long)pn);
        if (pb->W != svtme_align8_u(w) || pb->H != svtme_align8_u(h))
            return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_invalidate: picture %llu is %ux%u, new planes %ux%u",
                        (unsigned long long)pn, pb->W, pb->H, w, h);
    }
    // same stream as the jobs: the rebuild runs after every job already queued
    return upload_sync("svtme_picture_invalidate", c, pn, y, stride, w, h, 0, false);
}

// ---- asynchronous 8-bit uploads ----
// On the upload stream: the pyramid is built there from a device plane (the caller's, or a staging
// plane one linear DMA filled: a pitched copy straight into the padded plane runs as a slow blit),
// and the first job of each lane that reads the picture waits for it on the lane's stream. Jobs
// already queued that read an earlier version of the picture finish before its planes are rewritten.
struct UploadTrace { // what svtme_picture_upload_async's SVTME_SLOW_UPLOAD_MS log wants of upload_begin
    bool resident;
    std::chrono::steady_clock::time_point allocated;
};

// the upload stream, the picture's buffer ordered behind its queued readers there, and its `ready` event
static svtme_status upload_begin(svtme_ctx *c, uint64_t pn, uint32_t w, uint32_t h, PicBuf **pb,
                                 UploadTrace *trace = nullptr) {
    svtme_status st;
    if ((st = ensure_ustream(c)))
        return st;
    const bool resident = c->pics.count(pn) != 0;
    if ((st = alloc_pic(c, pn, svtme_align8_u(w), svtme_align8_u(h), pb)))
        return st;
    if (trace)
        *trace = {resident, std::chrono::steady_clock::now()};
    if (resident && (st = after_readers(c, **pb, c->ustream))) // queued jobs may still read the old planes
        return st;
    if (!(*pb)->ready)
        HIP_TRY(hipEventCreateWithFlags(&(*pb)->ready, hipEventDisableTiming));
    return SVTME_OK;
}

// the uploads' device staging plane holds `need` bytes
static svtme_status ensure_ustaging(svtme_ctx *c, size_t need) {
    if (c->ustaging_cap >= need)
        return SVTME_OK;
    HIP_TRY(hipStreamSynchronize(c->ustream)); // only between uploads: nothing queued reads the old buffer
    return ensure_buf(&c->ustaging, &c->ustaging_cap, need);
}

// Device-resident form of svtme_picture_upload_async: the pyramid is built from
// d_y on the upload stream (the caller orders d_y's producer before it, e.g. an
// RCCL broadcast of the plane, and keeps d_y until the build has run).
extern "C" svtme_status svtme_picture_upload_device_async(svtme_ctx *c, uint64_t pn, const uint8_t *d_y,
                                                          uint32_t stride, uint32_t w, uint32_t h) {
    if (!c || !d_y || w == 0 || h == 0 || stride < w)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_upload_device_async: bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    svtme_status st;
    PicBuf *pb;
    if ((st = upload_begin(c, pn, w, h, &pb)) || (st = build_pyramid(c, pb, d_y, stride, w, h, 0, c->ustream)))
        return st;
    return upload_publish(*pb, c->ustream, kAllLanes);
}

extern "C" svtme_status svtme_picture_upload_async(svtme_ctx *c, uint64_t pn, const uint8_t *y, uint32_t stride,
                                                   uint32_t w, uint32_t h) {
    if (!c || !y || w == 0 || h == 0 || stride < w)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_upload_async: bad arguments");
    // SVTME_SLOW_UPLOAD_MS=t: a call over t ms prints where its time went (stderr)
    static const double slow_ms = getenv("SVTME_SLOW_UPLOAD_MS") ? atof(getenv("SVTME_SLOW_UPLOAD_MS")) : 0.0;
    using clk     = std::chrono::steady_clock;
    const auto t0 = clk::now();
    std::lock_guard<std::mutex> lk(c->mu);
    const auto t1 = clk::now();
    HIP_TRY(hipSetDevice(c->device));
    svtme_status st;
    PicBuf *pb;
    UploadTrace tr;
    const size_t nfree = c->freebufs.size();
    if ((st = upload_begin(c, pn, w, h, &pb, &tr)))
        return st;
    struct SlowLog {
        double lim;
        std::chrono::steady_clock::time_point t0, t1, t2;
        uint64_t pn;
        size_t nfree;
        bool resident;
        ~SlowLog() {
            if (lim <= 0.0)
                return;
            const auto t3 = std::chrono::steady_clock::now();
            auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            if (ms(t0, t3) > lim)
                fprintf(stderr, "[svtme] slow upload pn %llu: %.3f ms (lock %.3f, alloc %.3f, rest %.3f; free bufs %zu, %s)\n",
                        (unsigned long long)pn, ms(t0, t3), ms(t0, t1), ms(t1, t2), ms(t2, t3), nfree,
                        resident ? "resident" : "new");
        }
    } slow_log{slow_ms, t0, t1, tr.allocated, pn, nfree, tr.resident};
    // a page-locked plane the device can read: the pyramid build reads it over PCIe
    // itself (no DMA into a staging plane, no second pass over it)
    const uint8_t *dy = device_view(c, y);
    if (dy && zero_copy_ok(y, stride, pb))
        st = build_pyramid_host(c, pb, dy, stride, w, h, c->ustream);
    else {
        // one linear copy of the span from the first to the last sample (rows keep their
        // stride; a padded encoder plane's margins ride along): a 2D copy out of
        // pageable memory goes row by row
        const size_t need = (size_t)(h - 1) * stride + w;
        if ((st = ensure_ustaging(c, need)))
            return st;
        HIP_TRY(hipMemcpyAsync(c->ustaging, y, need, hipMemcpyHostToDevice, c->ustream));
        st = build_pyramid(c, pb, c->ustaging, stride, w, h, 0, c->ustream);
    }
    return st ? st : upload_publish(*pb, c->ustream, kAllLanes);
}

// Upload from pageable memory through the context's page-locked staging ring:
// take a slot (wait for its last DMA), copy the rows into it with no lock held,
// then queue the DMA and the pyramid build like svtme_picture_upload_async.
extern "C" svtme_status svtme_picture_upload_copy_async(svtme_ctx *c, uint64_t pn, const uint8_t *y, uint32_t stride,
                                                        uint32_t w, uint32_t h) {
    if (!c || !y || w == 0 || h == 0 || stride < w)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_upload_copy_async: bad arguments");
    svtme_ctx::UpSlot *u = nullptr;
    {
        std::unique_lock<std::mutex> lk(c->mu);
        HIP_TRY(hipSetDevice(c->device));
        const svtme_status us = ensure_ustream(c);
        if (us)
            return us;
        // every slot being filled by other threads: wait for one (each is released
        // once its rows are staged and its DMA queued, a bounded time)
        c->up_free.wait(lk, [&] {
            for (int k = 0; k < SVTME_UPLOAD_SLOTS && !u; k++) {
                svtme_ctx::UpSlot &x = c->up[(c->up_next + k) % SVTME_UPLOAD_SLOTS];
                if (!x.busy)
                    u = &x;
            }
            return u != nullptr;
        });
        if (!u->done) // before the slot is taken: a failure here leaves it free
            HIP_TRY(hipEventCreateWithFlags(&u->done, hipEventDisableTiming));
        c->up_next = (uint32_t)(u - c->up + 1) % SVTME_UPLOAD_SLOTS;
        u->busy    = true;
    }
    // outside the context lock: other threads submit jobs meanwhile
    const size_t need = (size_t)w * h;
    hipError_t e      = hipSetDevice(c->device);
    if (e == hipSuccess && u->queued)
        e = hipEventSynchronize(u->done); // the slot's previous DMA has read it
    if (e == hipSuccess && u->cap < need) {
        if (u->h)
            e = hipHostFree(u->h);
        u->h   = nullptr;
        u->cap = 0;
        if (e == hipSuccess && (e = hipHostMalloc(&u->h, need, hipHostMallocDefault)) == hipSuccess)
            u->cap = need;
    }
    if (e != hipSuccess) {
        std::lock_guard<std::mutex> lk(c->mu);
        u->busy = false;
        c->up_free.notify_all();
        return fail(SVTME_ERR_INSUFFICIENT_RESOURCES, "svtme_picture_upload_copy_async: staging: %s",
                    hipGetErrorString(e));
    }
    for (uint32_t r = 0; r < h; r++)
        memcpy((uint8_t *)u->h + (size_t)r * w, y + (size_t)r * stride, w);
    std::lock_guard<std::mutex> lk(c->mu);
    struct Release { // the slot is free again however this returns (c->mu held)
        svtme_ctx *c;
        svtme_ctx::UpSlot *u;
        ~Release() {
            u->busy = false;
            c->up_free.notify_all();
        }
    } rel{c, u};
    PicBuf *pb;
    svtme_status st;
    if ((st = upload_begin(c, pn, w, h, &pb)) || (st = ensure_ustaging(c, need)))
        return st;
    HIP_TRY(hipMemcpyAsync(c->ustaging, u->h, need, hipMemcpyHostToDevice, c->ustream));
    HIP_TRY(hipEventRecord(u->done, c->ustream));
    u->queued = true;
    if ((st = build_pyramid(c, pb, c->ustaging, w, w, h, 0, c->ustream)))
        return st;
    return upload_publish(*pb, c->ustream, kAllLanes);
}

// ---- release and download ----
extern "C" svtme_status svtme_picture_release(svtme_ctx *c, uint64_t pn) {
    if (!c)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_release: null ctx");
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->pics.find(pn);
    if (it == c->pics.end())
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_release: picture %llu not resident",
                    (unsigned long long)pn);
    HIP_TRY(hipSetDevice(c->device));
    // no device-wide wait: the memory goes to the graves until the work queued
    // before the release (its upload, the lanes' readers) has run
    c->graves.push_back(it->second);
    c->pics.erase(it);
    (void)sweep_graves(c, 0);
    return SVTME_OK;
}

// Copy a padded plane back in the reference's geometry, (h + 2 pad) rows of (w + 2 pad) bytes,
// once every stream has run; a null dst asks for the geometry alone
static svtme_status download_plane(svtme_ctx *c, const DevPlane &p, void *dst, uint32_t *stride, uint32_t *width,
                                   uint32_t *height, uint32_t *pad, uint32_t bpp = 1) {
    const uint32_t S = (uint32_t)(p.width + 2 * p.pad); // samples, bpp bytes each
    if (stride)
        *stride = S;
    if (width)
        *width = (uint32_t)p.width;
    if (height)
        *height = (uint32_t)p.height;
    if (pad)
        *pad = (uint32_t)p.pad;
    if (!dst)
        return SVTME_OK;
    HIP_TRY(hipSetDevice(c->device));
    svtme_status qs = quiesce(c);
    if (qs)
        return qs;
    HIP_TRY(hipMemcpy2D(dst, (size_t)S * bpp, p.base - (ptrdiff_t)p.pad * p.stride - (ptrdiff_t)p.pad * bpp,
                        (size_t)p.stride, (size_t)S * bpp, (size_t)(p.height + 2 * p.pad), hipMemcpyDeviceToHost));
    return SVTME_OK;
}

extern "C" svtme_status svtme_picture_download(svtme_ctx *c, uint64_t pn, int level, uint8_t *dst, uint32_t *stride,
                                               uint32_t *width, uint32_t *height, uint32_t *pad) {
    if (!c || level < 0 || level > 2)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_download: bad arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    const PicBuf *pb = find_pic(c, pn);
    if (!pb)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_download: picture %llu not resident",
                    (unsigned long long)pn);
    return download_plane(c, pb->pyr.lv[level], dst, stride, width, height, pad);
}

// ---- chroma ----
// The padded chroma plane from cw x ch true samples (src may be the plane's own interior): the
// replication to W/2 x H/2 and the margins are one clamp of the source coordinate, k_build_full's
svtme_status svtme_host::build_chroma(const PicBuf *pb, int plane, const void *dsrc, uint32_t src_stride, uint32_t cw,
                                      uint32_t ch, hipStream_t st) {
    uint32_t w, h, left, top, stride, rows;
    svtme_chroma_geometry(pb->W, pb->H, &w, &h, &left, &top, &stride, &rows);
    HIP_TRY(svtme_launch_build_full(dsrc, src_stride, (int)cw, (int)ch, 0, pb->chroma[plane], (int)left, (int)top,
                                    (int)rows, st));
    return SVTME_OK;
}

extern "C" svtme_status svtme_picture_upload_chroma(svtme_ctx *c, uint64_t pn, const uint8_t *cb, const uint8_t *cr,
                                                    uint32_t stride, uint32_t w, uint32_t h) {
    if (!c || !cb || !cr || w == 0 || h == 0)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_upload_chroma: null ctx, cb or cr, or a %ux%u picture", w, h);
    const uint32_t cw = (w + 1) >> 1, ch = (h + 1) >> 1;
    if (stride < cw)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_upload_chroma: stride %u under the chroma width %u", stride,
                    cw);
    std::lock_guard<std::mutex> lk(c->mu);
    PicBuf *pbp = find_pic(c, pn);
    if (!pbp)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_upload_chroma: picture %llu is not resident",
                    (unsigned long long)pn);
    PicBuf &pb = *pbp;
    if (pb.W != svtme_align8_u(w) || pb.H != svtme_align8_u(h))
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_upload_chroma: picture %llu is %ux%u, the chroma's %ux%u",
                    (unsigned long long)pn, pb.W, pb.H, w, h);
    HIP_TRY(hipSetDevice(c->device));
    svtme_status st;
    const size_t one = (size_t)cw * ch;
    if ((st = alloc_chroma(c, pb)) || (st = ensure_buf(&c->staging, &c->staging_cap, 2 * one)))
        return st;
    uint8_t *stg = (uint8_t *)c->staging; // (reused in stream order, as upload_sync does)
    HIP_TRY(hipMemcpy2DAsync(stg, cw, cb, stride, cw, ch, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpy2DAsync(stg + one, cw, cr, stride, cw, ch, hipMemcpyHostToDevice, c->stream));
    // queued jobs of the other lanes may still read the old planes (lane 0's run before by stream order)
    if ((st = after_readers(c, pb, c->stream)) || (st = build_chroma(&pb, 0, stg, cw, cw, ch, c->stream)) ||
        (st = build_chroma(&pb, 1, stg + one, cw, cw, ch, c->stream)))
        return st;
    // later jobs of the other lanes wait for the planes: the stream is drained before the call returns
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SVTME_OK;
}

// Copy one chroma plane back in the shape of svtme_picture_download
extern "C" svtme_status svtme_picture_download_chroma(svtme_ctx *c, uint64_t pn, int plane, uint8_t *dst,
                                                      uint32_t *stride, uint32_t *width, uint32_t *height,
                                                      uint32_t *pad) {
    if (!c || plane < 1 || plane > 2)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_download_chroma: null ctx or plane %d (1 = Cb, 2 = Cr)", plane);
    std::lock_guard<std::mutex> lk(c->mu);
    const PicBuf *pb = find_pic(c, pn);
    if (!pb || !pb->cmem)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_download_chroma: picture %llu %s", (unsigned long long)pn,
                    !pb ? "is not resident" : "has no chroma");
    return download_plane(c, pb->chroma[plane - 1], dst, stride, width, height, pad);
}

// ---- the full-precision luma of a 10-bit picture ----
svtme_status svtme_host::build_hbd(const PicBuf *pb, const uint16_t *dsrc, uint32_t src_stride, uint32_t w, uint32_t h,
                                   hipStream_t st) {
    uint32_t left, top, stride, rows;
    svtme_hbd_geometry(pb->W, pb->H, &left, &top, &stride, &rows);
    HIP_TRY(svtme_launch_build_full16(dsrc, src_stride, (int)w, (int)h, pb->hbd, (int)left, (int)top, (int)rows, st));
    return SVTME_OK;
}

extern "C" svtme_status svtme_picture_attach_10bit(svtme_ctx *c, uint64_t pn, const uint16_t *y, uint32_t stride,
                                                   uint32_t w, uint32_t h) {
    if (!c || !y || w == 0 || h == 0)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_attach_10bit: null ctx or y, or a %ux%u picture", w, h);
    if (stride < w)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_attach_10bit: stride %u under the width %u", stride, w);
    std::lock_guard<std::mutex> lk(c->mu);
    PicBuf *pbp = find_pic(c, pn);
    if (!pbp)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_attach_10bit: picture %llu is not resident",
                    (unsigned long long)pn);
    PicBuf &pb = *pbp;
    if (pb.W != svtme_align8_u(w) || pb.H != svtme_align8_u(h))
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_attach_10bit: picture %llu is %ux%u, the plane %ux%u",
                    (unsigned long long)pn, pb.W, pb.H, w, h);
    HIP_TRY(hipSetDevice(c->device));
    svtme_status st;
    if ((st = alloc_hbd(c, pb)) || (st = ensure_buf(&c->staging, &c->staging_cap, (size_t)w * h * 2)))
        return st;
    // (the staging plane is reused in stream order, as upload_sync does)
    HIP_TRY(hipMemcpy2DAsync(c->staging, (size_t)w * 2, y, (size_t)stride * 2, (size_t)w * 2, h, hipMemcpyHostToDevice,
                             c->stream));
    // queued jobs of the other lanes may still read the old plane (lane 0's run before by stream order)
    if ((st = after_readers(c, pb, c->stream)) || (st = build_hbd(&pb, (const uint16_t *)c->staging, w, w, h, c->stream)))
        return st;
    // later jobs of the other lanes wait for the plane: the stream is drained before the call returns
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SVTME_OK;
}

// Copy the 16-bit plane back in the shape of svtme_picture_download; the stride is in samples
extern "C" svtme_status svtme_picture_download_10bit(svtme_ctx *c, uint64_t pn, uint16_t *dst, uint32_t *stride,
                                                     uint32_t *width, uint32_t *height, uint32_t *pad) {
    if (!c)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_download_10bit: null ctx");
    std::lock_guard<std::mutex> lk(c->mu);
    const PicBuf *pb = find_pic(c, pn);
    if (!pb || !pb->hmem)
        return fail(SVTME_ERR_BAD_PARAMETER, "svtme_picture_download_10bit: picture %llu %s", (unsigned long long)pn,
                    !pb ? "is not resident" : "has no 10-bit plane");
    return download_plane(c, pb->hbd, dst, stride, width, height, pad, 2);
}

// ---- the full-precision chroma of a 10-bit picture ----
// k_build_full16 takes its geometry as parameters: the chroma margins serve it as the luma's do
svtme_status svtme_host::build_hbd_chroma(const PicBuf *pb, int plane, const uint16_t *dsrc, uint32_t src_stride,
                                          uint32_t cw, uint32_t ch, hipStream_t st) {
    uint32_t w, h, left, top, stride, rows;
    svtme_hbd_chroma_geometry(pb->W, pb->H, &w, &h, &left, &top, &stride, &rows);
    HIP_TRY(svtme_launch_build_full16(dsrc, src_stride, (int)cw, (int)ch, pb->hchroma[plane], (int)left, (int)top,
                                      (int)rows, st));
    return SVTME_OK;
}

extern "C" svtme_status svtme_picture_attach_chroma_10bit(svtme_ctx *c, uint64_t pn, const uint16_t *cb,
                                                          const uint16_t *cr, uint32_t stride, uint32_t w, uint32_t h) {
    const char *fn = "svtme_picture_attach_chroma_10bit";
    if (!c || !cb || !cr || w == 0 || h == 0)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: null ctx, cb or cr, or a %ux%u picture", fn, w, h);
    const uint32_t cw = (w + 1) >> 1, ch = (h + 1) >> 1;
    if (stride < cw)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: stride %u under the chroma width %u", fn, stride, cw);
    std::lock_guard<std::mutex> lk(c->mu);
    PicBuf *pbp = find_pic(c, pn);
    if (!pbp)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: picture %llu is not resident", fn, (unsigned long long)pn);
    PicBuf &pb = *pbp;
    if (pb.W != svtme_align8_u(w) || pb.H != svtme_align8_u(h))
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: picture %llu is %ux%u, the chroma's %ux%u", fn, (unsigned long long)pn,
                    pb.W, pb.H, w, h);
    HIP_TRY(hipSetDevice(c->device));
    svtme_status st;
    const size_t one = (size_t)cw * ch; // samples
    if ((st = alloc_hbd_chroma(c, pb)) || (st = ensure_buf(&c->staging, &c->staging_cap, 4 * one)))
        return st;
    uint16_t *stg = (uint16_t *)c->staging; // (reused in stream order, as upload_sync does)
    HIP_TRY(hipMemcpy2DAsync(stg, (size_t)cw * 2, cb, (size_t)stride * 2, (size_t)cw * 2, ch, hipMemcpyHostToDevice,
                             c->stream));
    HIP_TRY(hipMemcpy2DAsync(stg + one, (size_t)cw * 2, cr, (size_t)stride * 2, (size_t)cw * 2, ch,
                             hipMemcpyHostToDevice, c->stream));
    // queued jobs of the other lanes may still read the old planes (lane 0's run before by stream order)
    if ((st = after_readers(c, pb, c->stream)) || (st = build_hbd_chroma(&pb, 0, stg, cw, cw, ch, c->stream)) ||
        (st = build_hbd_chroma(&pb, 1, stg + one, cw, cw, ch, c->stream)))
        return st;
    // later jobs of the other lanes wait for the planes: the stream is drained before the call returns
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SVTME_OK;
}

// Copy one 16-bit chroma plane back in the shape of svtme_picture_download_10bit; the stride is in samples
extern "C" svtme_status svtme_picture_download_chroma_10bit(svtme_ctx *c, uint64_t pn, int plane, uint16_t *dst,
                                                            uint32_t *stride, uint32_t *width, uint32_t *height,
                                                            uint32_t *pad) {
    const char *fn = "svtme_picture_download_chroma_10bit";
    if (!c || plane < 1 || plane > 2)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: null ctx or plane %d (1 = Cb, 2 = Cr)", fn, plane);
    std::lock_guard<std::mutex> lk(c->mu);
    const PicBuf *pb = find_pic(c, pn);
    if (!pb || !pb->hcmem)
        return fail(SVTME_ERR_BAD_PARAMETER, "%s: picture %llu %s", fn, (unsigned long long)pn,
                    !pb ? "is not resident" : "has no 10-bit chroma");
    return download_plane(c, pb->hchroma[plane - 1], dst, stride, width, height, pad, 2);
}
