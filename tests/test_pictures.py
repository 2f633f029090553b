"""The resident luma pyramid (svtme_pyramid.hip: k_build_full, k_build_down, k_host_rows) and the
host code around it (svtme_pictures.cpp: the luma upload entry points, the pool, the graves).

Expected planes come from tests/pyramid_model.py, a numpy model that the CPU tests pin to the
reference's pyramid hashes of tests/golden/me_cases.json and compare with the CPU oracle at every
size of the sweep. The GPU tests read back, through svtme_picture_download, what every upload path
leaves at small awkward sizes and source layouts, what a recycled buffer holds, and what a refused
call leaves behind. Every comparison is exact.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import pyramid_model as PM

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAD_PARAMETER = 0x80001005
BASE = 19000  # picture numbers of this file's uploads
LEVELS = ("full", "quarter", "sixteenth")

# true w x h. 17x10 and 6x7 supply the residues 2 and 7 of h mod 8.
SIZES = [(1, 1), (3, 5), (5, 3), (8, 8), (11, 4), (13, 8), (9, 17), (20, 12), (24, 16), (31, 33), (46, 22), (63, 65),
         (72, 40), (121, 67), (130, 70), (200, 136), (17, 10), (6, 7)]

# how a plane reaches the library; (function, memory of the source)
ENTRY_POINTS = {
    "sync_pageable": ("svtme_picture_upload", "pageable"),
    "sync_pinned_aligned": ("svtme_picture_upload", "pinned"),  # zero copy: k_host_rows, margins-only k_build_full
    "sync_pinned_odd": ("svtme_picture_upload", "pinned"),      # not dword aligned: falls back to the DMA
    "upload_10bit": ("svtme_picture_upload_10bit", "pageable"),
    "async_pageable": ("svtme_picture_upload_async", "pageable"),
    "async_pinned": ("svtme_picture_upload_async", "pinned"),
    "copy_async": ("svtme_picture_upload_copy_async", "pageable"),
    "device": ("svtme_picture_upload_device", "device"),
    "device_async": ("svtme_picture_upload_device_async", "device"),
    "invalidate": ("svtme_picture_invalidate", "pageable"),
}
STRIDE_CLASSES = ("w", "w+1", "w+13", "r64")
UPLOAD_FUNCTIONS = sorted({fn for fn, _ in ENTRY_POINTS.values()})
FILL8, FILL16 = 0xA5, 0xFFFF  # between the rows of a source buffer; in no picture


def stride_of(w: int, cls: str) -> int:
    return {"w": w, "w+1": w + 1, "w+13": w + 13, "r64": (w + 63) // 64 * 64}[cls]


def offsets_of(ep: str):
    """Start offsets from a 4-byte aligned base: bytes, or samples for 10 bit."""
    return (0,) if ep == "sync_pinned_aligned" else (0, 1) if ep == "upload_10bit" else (0, 1, 2, 3)


def layout_allowed(ep: str, w: int, cls: str, off: int) -> bool:
    dword = ((stride_of(w, cls) | off) & 3) == 0
    return dword if ep == "sync_pinned_aligned" else not dword if ep == "sync_pinned_odd" else True


def draw_layouts(seed: int = 20240607) -> dict:
    """{(entry point, (w, h)): (stride class, offset)}: one seeded draw per pair, from the layouts the
    entry point allows at that width, preferring the classes and offsets it has met least."""
    rng = np.random.default_rng(seed)
    out, seen = {}, {}
    for ep in ENTRY_POINTS:
        for size in [SIZES[i] for i in rng.permutation(len(SIZES))]:
            options = [(c, o) for c in STRIDE_CLASSES for o in offsets_of(ep) if layout_allowed(ep, size[0], c, o)]
            if not options:
                continue
            score = [seen.get((ep, "s", c), 0) + seen.get((ep, "o", o), 0) for c, o in options]
            best = [op for op, s in zip(options, score) if s == min(score)]
            c, o = best[rng.integers(len(best))]
            out[ep, size] = (c, o)
            seen[ep, "s", c] = seen.get((ep, "s", c), 0) + 1
            seen[ep, "o", o] = seen.get((ep, "o", o), 0) + 1
    return out


LAYOUTS = draw_layouts()


def picture(w: int, h: int, ten_bit: bool = False, salt: int = 0) -> np.ndarray:
    """Seeded i.i.d. noise (a replicated or shifted column shows); the fill value appears nowhere."""
    rng = np.random.default_rng([w, h, int(ten_bit), salt])
    if ten_bit:
        return rng.integers(0, 1024, (h, w), dtype=np.uint16)
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    y[y == FILL8] ^= 1
    return y


# ----------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------
def test_size_list_reaches_the_edges():
    ws, hs = [w for w, _ in SIZES], [h for _, h in SIZES]
    assert {w % 8 for w in ws} == set(range(8)) and {h % 8 for h in hs} == set(range(8))
    assert any(w < 4 for w in ws) and any(4 <= w < 8 for w in ws) and any(8 <= w < 16 for w in ws)
    assert 1 in hs
    assert any(PM.align8(w) // 4 == 2 for w in ws)  # the sixteenth plane narrower than one thread's dword
    assert any(w > 16 and 1 <= w % 16 <= 3 for w in ws)  # k_host_rows: whole chunks and a bytewise tail
    assert any(w > 64 and h > 64 for w, h in SIZES)
    assert len(set(SIZES)) == len(SIZES)


def test_layouts_cover_strides_and_offsets():
    assert LAYOUTS == draw_layouts()  # seeded: the same draw every time
    for ep in ENTRY_POINTS:
        drawn = [LAYOUTS[ep, s] for s in SIZES if (ep, s) in LAYOUTS]
        for (w, h) in SIZES:
            if (ep, (w, h)) in LAYOUTS:
                assert layout_allowed(ep, w, *LAYOUTS[ep, (w, h)])
        for c in STRIDE_CLASSES:
            assert sum(d[0] == c for d in drawn) >= 2, (ep, c)
        for o in offsets_of(ep):
            assert sum(d[1] == o for d in drawn) >= 2, (ep, o)
    for size in SIZES:  # the aligned zero-copy path meets every size (r64 is always dword aligned)
        assert ("sync_pinned_aligned", size) in LAYOUTS
    assert all((ep, s) in LAYOUTS for ep in ENTRY_POINTS for s in SIZES)


def test_model_reproduces_reference_pyramid_hashes(svtme):
    cases = [c for c in json.load(open(os.path.join(GOLD, "me_cases.json"))) if "pyramid_sha256" in c]
    assert len(cases) >= 4
    for case in cases:
        f = svtme.test_frames(case["content"], case["w"], case["h"], [8])[8]
        planes = dict(zip(LEVELS, PM.pyramid(f)))
        assert set(case["pyramid_sha256"]) == set(LEVELS)
        for k, d in case["pyramid_sha256"].items():
            assert hashlib.sha256(np.ascontiguousarray(planes[k]).tobytes()).hexdigest() == d, (case["name"], k)


@pytest.mark.parametrize("ten_bit", (False, True), ids=("8bit", "10bit"))
def test_oracle_pyramid_equals_model(svtme, ten_bit):
    assert (svtme.PAD_FULL, svtme.PAD_QUARTER, svtme.PAD_SIXTEENTH) == PM.PADS
    for (w, h) in SIZES:
        f = picture(w, h, ten_bit)
        p = svtme.build_host_pyramid(f, "oracle")
        for name, want in zip(LEVELS, PM.pyramid(f)):
            got = getattr(p, name)
            assert got.shape == want.shape and np.array_equal(got, want), (w, h, name)


def test_model_geometry():
    for (w, h) in SIZES:
        W, H = PM.align8(w), PM.align8(h)
        for lv, (p, pad) in enumerate(zip(PM.pyramid(picture(w, h)), PM.PADS)):
            assert p.shape == ((H >> lv) + 2 * pad, (W >> lv) + 2 * pad) and p.dtype == np.uint8


# ----------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------
def source(mem: str, pic: np.ndarray, stride: int, off: int):
    """The picture inside a larger buffer of FILL: -> (what keeps the memory alive, pointer to sample (0, 0)).
    The buffer's base is at least 64-byte aligned; `off` is in samples."""
    import torch

    h, w = pic.shape
    fill = FILL16 if pic.dtype == np.uint16 else FILL8
    n = off + stride * h + 8
    if mem == "pinned":
        keep = torch.empty(n, dtype=torch.uint8).pin_memory()
        buf = keep.numpy()
        assert pic.dtype == np.uint8
    else:
        keep = np.empty(n * pic.itemsize + 64, np.uint8)
        a = (-keep.ctypes.data) % 64
        buf = keep[a:a + n * pic.itemsize].view(pic.dtype)
    assert buf.ctypes.data % 64 == 0
    buf[:] = fill
    buf[off:off + stride * h].reshape(h, stride)[:, :w] = pic
    if mem == "device":
        keep = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        assert keep.data_ptr() % 64 == 0
        return keep, keep.data_ptr() + off
    return (keep, buf), buf.ctypes.data + off * pic.itemsize


def download_checked(gpu, pn: int, w: int, h: int):
    """The three planes; the geometry the download reports is that of the 8-aligned size."""
    W, H = PM.align8(w), PM.align8(h)
    planes = []
    for lv, pad in enumerate(PM.PADS):
        g = [C.c_uint32() for _ in range(4)]
        st = gpu.lib.svtme_picture_download(gpu.ctx, pn, lv, None, *[C.byref(v) for v in g])
        assert st == 0, gpu.lib.svtme_last_error()
        assert [v.value for v in g] == [(W >> lv) + 2 * pad, W >> lv, H >> lv, pad], (w, h, lv)
        out = np.full(((H >> lv) + 2 * pad, (W >> lv) + 2 * pad), 0x3C, np.uint8)
        st = gpu.lib.svtme_picture_download(gpu.ctx, pn, lv, out.ctypes.data, *[C.byref(v) for v in g])
        assert st == 0, gpu.lib.svtme_last_error()
        planes.append(out)
    return planes


def assert_planes(got, want, what):
    for name, g, e in zip(LEVELS, got, want):
        bad = np.argwhere(g != e)
        assert bad.size == 0, (what, name, "first at (row, col)", bad[0].tolist(), int(g[tuple(bad[0])]),
                               int(e[tuple(bad[0])]), len(bad))


def upload_through(gpu, ep: str, pn: int, pic: np.ndarray, cls: str, off: int):
    """-> what keeps the source alive (until the upload has run)."""
    fn, mem = ENTRY_POINTS[ep]
    h, w = pic.shape
    stride = stride_of(w, cls)
    keep, ptr = source(mem, pic, stride, off)
    if ep == "sync_pinned_aligned":
        assert ptr % 4 == 0 and stride % 4 == 0
    if ep == "sync_pinned_odd":
        assert ptr % 4 or stride % 4
    if ep == "invalidate":
        gpu.upload(pn, picture(w, h, salt=1))  # a resident picture of that size, other content
    st = getattr(gpu.lib, fn)(gpu.ctx, pn, ptr, stride, w, h)
    assert st == 0, (fn, gpu.lib.svtme_last_error())
    return keep


@pytest.mark.gpu
@pytest.mark.parametrize("ep", list(ENTRY_POINTS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_upload_path_equals_model(svtme, gpu, size, ep):
    w, h = size
    cls, off = LAYOUTS[ep, size]
    pic = picture(w, h, ten_bit=ep == "upload_10bit")
    pn = BASE + 1
    keep = upload_through(gpu, ep, pn, pic, cls, off)
    try:
        gpu.sync()
        assert_planes(download_checked(gpu, pn, w, h), PM.pyramid(pic), (ep, size, cls, off))
    finally:
        gpu.release(pn)
        del keep


RECYCLE_SIZES = [(8, 8), (72, 40), (121, 67)]
RECYCLE_PATHS = ("sync_pageable", "async_pageable", "copy_async", "device")


def assert_recycled_buffer_rewritten(gpu, w, h, ep, reserve=False):
    ones, zeros = np.full((h, w), 0xFF, np.uint8), np.zeros((h, w), np.uint8)
    if reserve:
        gpu.reserve_pictures(w, h, 1)
    gpu.upload(BASE + 10, ones)
    for p in download_checked(gpu, BASE + 10, w, h):
        assert (p == 0xFF).all()
    gpu.release(BASE + 10)
    gpu.sync()
    if reserve:
        gpu.reserve_pictures(w, h, 1)  # the released buffer is the reserved one: nothing new
    # another number, the same byte count: the pool hands the freed buffer out again
    keep = upload_through(gpu, ep, BASE + 11, zeros, "w", 0)
    try:
        gpu.sync()
        for name, p in zip(LEVELS, download_checked(gpu, BASE + 11, w, h)):
            assert not p.any(), (w, h, ep, name, "stale bytes", int(np.count_nonzero(p)))
    finally:
        gpu.release(BASE + 11)
        gpu.sync()
        del keep


@pytest.mark.gpu
@pytest.mark.parametrize("ep", RECYCLE_PATHS)
@pytest.mark.parametrize("size", RECYCLE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_recycled_buffer_is_rewritten(svtme, gpu, size, ep):
    assert_recycled_buffer_rewritten(gpu, *size, ep)


@pytest.mark.gpu
def test_reserved_buffer_is_rewritten(svtme, gpu):
    assert_recycled_buffer_rewritten(gpu, 121, 67, "sync_pageable", reserve=True)


def refused(gpu, fn, *args):
    st = getattr(gpu.lib, fn)(*args)
    return st & 0xFFFFFFFF, gpu.lib.svtme_last_error().decode(errors="replace")


@pytest.mark.gpu
def test_size_change_drops_attached_planes(svtme, gpu):
    """The same number at another size: alloc_pic's size-change path. The planes are the new size's and
    what was attached to the old picture is gone; the old size uploaded once more is right again."""
    pn = BASE + 20
    (w0, h0), (w1, h1) = (72, 40), (121, 67)
    a, b = picture(w0, h0), picture(w1, h1)
    a10 = picture(w0, h0, ten_bit=True)
    cw, ch = (w0 + 1) >> 1, (h0 + 1) >> 1
    gpu.upload(pn, a)
    try:
        gpu.upload_chroma(pn, picture(cw, ch, salt=2), picture(cw, ch, salt=3), w0, h0)
        gpu.attach_10bit(pn, a10)
        gpu.attach_chroma_10bit(pn, picture(cw, ch, True, 4), picture(cw, ch, True, 5), w0, h0)
        assert gpu.download_chroma(pn, 1).size and gpu.download_10bit(pn).size and gpu.download_chroma_10bit(pn, 2).size
        gpu.upload(pn, b)
        assert_planes(download_checked(gpu, pn, w1, h1), PM.pyramid(b), "new size")
        g = [C.byref(C.c_uint32()) for _ in range(4)]
        for fn, args in (("svtme_picture_download_chroma", (1, None)), ("svtme_picture_download_10bit", (None,)),
                         ("svtme_picture_download_chroma_10bit", (1, None))):
            st, msg = refused(gpu, fn, gpu.ctx, pn, *args, *g)
            assert st == BAD_PARAMETER and msg.startswith(fn + ":"), (fn, hex(st), msg)
        gpu.upload(pn, a)
        assert_planes(download_checked(gpu, pn, w0, h0), PM.pyramid(a), "old size again")
        for fn, args in (("svtme_picture_download_chroma", (1, None)), ("svtme_picture_download_10bit", (None,)),
                         ("svtme_picture_download_chroma_10bit", (1, None))):
            assert refused(gpu, fn, gpu.ctx, pn, *args, *g)[0] == BAD_PARAMETER, fn
    finally:
        gpu.release(pn)


@pytest.mark.gpu
@pytest.mark.parametrize("fn", UPLOAD_FUNCTIONS)
def test_upload_refusals(svtme, gpu, fn):
    """Bad arguments are refused with BAD_PARAMETER under the called function's own name, and leave no
    picture of a new number and every byte of a resident one."""
    w, h = 24, 16
    ep = next(e for e, (f, _) in ENTRY_POINTS.items() if f == fn)
    pic = picture(w, h, ten_bit=fn == "svtme_picture_upload_10bit", salt=7)
    keep, ptr = source(ENTRY_POINTS[ep][1], pic, w, 0)
    resident, fresh = BASE + 30, BASE + 31
    gpu.upload(resident, picture(w, h, salt=8))
    try:
        before = download_checked(gpu, resident, w, h)
        bad = {"null ctx": (None, ptr, w, w, h), "null plane": (gpu.ctx, None, w, w, h), "w = 0": (gpu.ctx, ptr, w, 0, h),
               "h = 0": (gpu.ctx, ptr, w, w, 0), "stride < w": (gpu.ctx, ptr, w - 1, w, h)}
        for pn in (resident, fresh):
            for what, (ctx, p, stride, ww, hh) in bad.items():
                st, msg = refused(gpu, fn, ctx, pn, p, stride, ww, hh)
                assert st == BAD_PARAMETER, (fn, what, pn, hex(st))
                assert msg.startswith(fn + ":"), (fn, what, pn, msg)
        if fn == "svtme_picture_invalidate":
            for what, args in {"not resident": (fresh, ptr, w, w, h), "another size": (resident, ptr, w, w - 8, h),
                               "another height": (resident, ptr, w, w, h + 8)}.items():
                st, msg = refused(gpu, fn, gpu.ctx, *args)
                assert st == BAD_PARAMETER and msg.startswith(fn + ":"), (what, hex(st), msg)
        gpu.sync()
        st, msg = refused(gpu, "svtme_picture_download", gpu.ctx, fresh, 0, None, None, None, None, None)
        assert st == BAD_PARAMETER, "a refused upload left a picture"
        assert_planes(download_checked(gpu, resident, w, h), before, (fn, "resident picture changed"))
        # and the valid form of the same call succeeds
        pn = resident if fn == "svtme_picture_invalidate" else fresh
        assert getattr(gpu.lib, fn)(gpu.ctx, pn, ptr, w, w, h) == 0
        gpu.sync()
        assert_planes(download_checked(gpu, pn, w, h), PM.pyramid(pic), (fn, "valid call"))
        if pn == fresh:
            gpu.release(fresh)
    finally:
        gpu.release(resident)
        del keep
