"""Temporal filtering of 10-bit chroma: the resident 16-bit Cb/Cr planes
(svtme_picture_attach_chroma_10bit, svtme_picture_download_chroma_10bit) and the 10-bit yuv calls
(svtme_tf_filter_yuv_10bit, svtme_tf_window_yuv_10bit), include/svtme.h.

Expected values are the fixtures tests/golden/tffhc_cases.{json,npz}: the reference's
svt_highbd_inter_predictor on 16-bit chroma planes and its high-bit-depth filter functions with
tf_chroma set, under the glue of tests/golden/make_golden_tffc.py (make_golden_tffhc.py). Beside them
stands a model in numpy and Python integers (tests/tffhc_model.py). CPU tests pin the ABI, the
argument checks that need no context, the fixtures and the model to the fixtures; GPU tests compare
the calls with the fixtures, the model, each other and the calls that were there before. Every
comparison is exact.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ref_available

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
for p in (GOLD, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_golden_tff as GF  # noqa: E402
import make_golden_tffc as GC  # noqa: E402
import make_golden_tffh as GH  # noqa: E402
import make_golden_tffhc as GHC  # noqa: E402
import test_tf_window as TW  # noqa: E402  (its window helpers; its tests are collected from its own file)
import tffhc_model as MHC  # noqa: E402

DOC = json.load(open(os.path.join(GOLD, "tffhc_cases.json")))
CASES = DOC["cases"]
BAD_PARAMETER = 0x80001005
BASE = 15000  # picture numbers of this file's uploads
OUT = 900     # + BASE: the result picture of a window into a fresh number
SYMBOLS = ("svtme_picture_attach_chroma_10bit", "svtme_picture_download_chroma_10bit", "svtme_tf_filter_yuv_10bit",
           "svtme_tf_window_yuv_10bit")
PAD = 40


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLD, "tffhc_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def case_by_id(name):
    return next(c for c in CASES if c["id"] == name)


# ----------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------
def test_tffhc_symbols_exported(svtme):
    lib = svtme.load_product()
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []


_STRUCTS = {"svtme_tf_filter_yuv16_out": ("TfFilterYuv16Out", 48), "svtme_tf_window_yuv16_out": ("TfWindowYuv16Out", 24)}

# each new function assigned to a pointer of the type the Python prototypes assume: a header that
# differs does not compile
_PROTO_PROGRAM = r"""
svtme_status (*p_attach)(svtme_ctx *, uint64_t, const uint16_t *, const uint16_t *, uint32_t, uint32_t, uint32_t) =
    svtme_picture_attach_chroma_10bit;
svtme_status (*p_download)(svtme_ctx *, uint64_t, int, uint16_t *, uint32_t *, uint32_t *, uint32_t *, uint32_t *) =
    svtme_picture_download_chroma_10bit;
svtme_status (*p_filter)(svtme_ctx *, uint64_t, const uint64_t *, uint32_t, uint32_t, uint32_t,
                         const svtme_tf_filter_yuv_controls *, const svtme_tf_subpel_sb *,
                         const svtme_tf_filter_yuv16_out *) = svtme_tf_filter_yuv_10bit;
svtme_status (*p_window)(svtme_ctx *, const svtme_job *, uint32_t, uint32_t, uint32_t, const svtme_tf_subpel_controls *,
                         const svtme_tf_filter_yuv_controls *, uint64_t, const svtme_tf_window_out *, uint16_t *,
                         uint32_t, const svtme_tf_window_yuv16_out *) = svtme_tf_window_yuv_10bit;
"""


def test_tffhc_struct_sizes_offsets_and_prototypes_equal_the_header(svtme, tmp_path):
    lines = []
    for cname, (pyname, _) in _STRUCTS.items():
        lines.append(f'printf("sizeof {cname} %zu\\n", sizeof({cname}));')
        for field, _ in getattr(svtme, pyname)._fields_:
            lines.append(f'printf("{cname}.{field} %zu\\n", offsetof({cname}, {field}));')
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svtme.h"\n' + _PROTO_PROGRAM +
                   "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "abi.o")], check=True)  # the prototypes; the functions themselves are not linked
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svtme.h"\nint main(void) {\n' + "\n".join(lines) +
                   "\nreturn 0;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        key, val = line.rsplit(" ", 1)
        got[key] = int(val)
    for cname, (pyname, size) in _STRUCTS.items():
        st = getattr(svtme, pyname)
        assert got["sizeof " + cname] == C.sizeof(st) == size, cname
        for field, _ in st._fields_:
            assert got[f"{cname}.{field}"] == getattr(st, field).offset, (cname, field)
    lib, vp, u32, u64 = svtme.load_product(), C.c_void_p, C.c_uint32, C.c_uint64
    pu32 = C.POINTER(u32)
    want = {"svtme_picture_attach_chroma_10bit": [vp, u64, vp, vp, u32, u32, u32],
            "svtme_picture_download_chroma_10bit": [vp, u64, C.c_int, vp, pu32, pu32, pu32, pu32],
            "svtme_tf_filter_yuv_10bit": [vp, u64, C.POINTER(u64), u32, u32, u32, C.POINTER(svtme.TfFilterYuvControls), vp,
                                          C.POINTER(svtme.TfFilterYuv16Out)],
            "svtme_tf_window_yuv_10bit": [vp, C.POINTER(svtme.Job), u32, u32, u32, C.POINTER(svtme.TfSubpelControls),
                                          C.POINTER(svtme.TfFilterYuvControls), u64, C.POINTER(svtme.TfWindowOut), vp, u32,
                                          C.POINTER(svtme.TfWindowYuv16Out)]}
    for name, argtypes in want.items():
        assert list(getattr(lib, name).argtypes) == argtypes, name
        assert getattr(lib, name).restype is C.c_int32, name


def _controls(svtme, **over):
    return svtme.TfFilterYuvControls.from_dict(dict({"tf_decay_factor_fp16": 2_000_000, "tf_mv_dist_th": 64,
                                                     "sub_sampling_shift": 1, "tf_decay_factor_cb_fp16": 2_000_000,
                                                     "tf_decay_factor_cr_fp16": 1_000_000}, **over))


def _filter_call(svtme, lib, ctx, refs, n=None, ctl=None, null=None, w=128, h=128, centre=BASE + 8, strides=None,
                 branch=0, with_err32=True):
    """-> the status of svtme_tf_filter_yuv_10bit; on an error no output may be touched."""
    ctl = ctl if ctl is not None else _controls(svtme)
    sbs = svtme.sb_total(svtme.align8(w), svtme.align8(h))
    slots = max(len(refs), svtme.MAX_BATCH_JOBS + 1)
    arr = (C.c_uint64 * slots)(*refs)
    sub = np.zeros((slots, sbs), svtme.TF_SUBPEL_SB_DTYPE)
    sub["branch"][min(len(refs), slots) - 1, sbs - 1] = branch  # the last struct the call reads
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    sy, scb, scr = strides or (w, cw, cw)
    bufs = [np.full(h * max(sy, w), 0x5A5A, np.uint16), np.full(ch * max(scb, cw), 0x5A5A, np.uint16),
            np.full(ch * max(scr, cw), 0x5A5A, np.uint16)]
    e32 = np.full(slots * sbs * 4, 0x5A5A5A5A, np.uint32)
    out = svtme.TfFilterYuv16Out(y=None if null == "y" else bufs[0].ctypes.data, cb=bufs[1].ctypes.data,
                                 cr=bufs[2].ctypes.data, y_stride=sy, cb_stride=scb, cr_stride=scr,
                                 err32=e32.ctypes.data if with_err32 else None)
    st = lib.svtme_tf_filter_yuv_10bit(None if null == "ctx" else ctx, centre, None if null == "refs" else arr,
                                       len(refs) if n is None else n, w, h, None if null == "controls" else C.byref(ctl),
                                       None if null == "subpel" else sub.ctypes.data,
                                       None if null == "out" else C.byref(out))
    if st:
        assert all((b == 0x5A5A).all() for b in bufs) and (e32 == 0x5A5A5A5A).all()
        assert lib.svtme_last_error().decode() != ""
    return st & 0xFFFFFFFF


def _bad_filter_calls(svtme):
    ok = [BASE + 7]
    for null in ("ctx", "refs", "controls", "subpel", "out", "y"):
        yield "null " + null, dict(refs=ok, null=null)
    yield "n 0", dict(refs=ok, n=0)
    yield "n 17", dict(refs=ok * (svtme.MAX_BATCH_JOBS + 1))
    yield "y_stride under the width", dict(refs=ok, strides=(127, 64, 64))
    yield "cb_stride under the chroma width", dict(refs=ok, strides=(128, 63, 64))
    yield "cr_stride under the chroma width", dict(refs=ok, strides=(128, 64, 63))
    yield "tf_mv_dist_th 32768", dict(refs=ok, ctl=_controls(svtme, tf_mv_dist_th=32768))
    yield "sub_sampling_shift 2", dict(refs=ok, ctl=_controls(svtme, sub_sampling_shift=2))
    yield "branch 3", dict(refs=ok, branch=3)


def _attach_call(lib, ctx, null=None, w=121, h=67, stride=None, pn=BASE + 8):
    cw, ch = max((w + 1) >> 1, 1), max((h + 1) >> 1, 1)
    cb, cr = np.zeros((ch, cw), np.uint16), np.zeros((ch, cw), np.uint16)
    st = lib.svtme_picture_attach_chroma_10bit(None if null == "ctx" else ctx, pn, None if null == "cb" else cb.ctypes.data,
                                               None if null == "cr" else cr.ctypes.data, cw if stride is None else stride,
                                               w, h)
    return st & 0xFFFFFFFF


def _window_call(svtme, lib, ctx, null=None, n=1, stride=128, uv_strides=(64, 64), w=128, h=128):
    win = yuv_window_10(w, h, (7,))
    jobs = (svtme.Job * (svtme.MAX_BATCH_JOBS + 1))(TW.tf_job(svtme, win, BASE + 8, BASE + 7))
    sp, fc = svtme.TfSubpelControls.from_dict(win["subpel"]), svtme.TfFilterYuvControls.from_dict(win["filter"])
    p16 = np.full(h * w, 0x5A5A, np.uint16)
    cb, cr = np.full(h * w, 0x5A5A, np.uint16), np.full(h * w, 0x5A5A, np.uint16)
    out_uv = svtme.TfWindowYuv16Out(cb=cb.ctypes.data, cr=cr.ctypes.data, cb_stride=uv_strides[0], cr_stride=uv_strides[1])
    st = lib.svtme_tf_window_yuv_10bit(None if null == "ctx" else ctx, None if null == "jobs" else jobs, n, w, h,
                                       None if null == "subpel_controls" else C.byref(sp),
                                       None if null == "filter_controls" else C.byref(fc), BASE + OUT, None,
                                       p16.ctypes.data, stride, C.byref(out_uv))
    if st:
        assert (p16 == 0x5A5A).all() and (cb == 0x5A5A).all() and (cr == 0x5A5A).all()
    return st & 0xFFFFFFFF


def _context_free_errors(svtme, lib, ctx):
    for what, kw in _bad_filter_calls(svtme):
        assert _filter_call(svtme, lib, ctx, **kw) == BAD_PARAMETER, what
    for null in ("ctx", "cb", "cr"):
        assert _attach_call(lib, ctx, null=null) == BAD_PARAMETER, null
    assert _attach_call(lib, ctx, w=0) == BAD_PARAMETER
    assert _attach_call(lib, ctx, h=0) == BAD_PARAMETER
    assert _attach_call(lib, ctx, stride=60) == BAD_PARAMETER  # the chroma width of 121 is 61
    u32 = C.c_uint32()
    sizes = (C.byref(u32),) * 4
    assert lib.svtme_picture_download_chroma_10bit(None, BASE + 8, 1, None, *sizes) & 0xFFFFFFFF == BAD_PARAMETER
    for plane in (0, 3):
        assert lib.svtme_picture_download_chroma_10bit(ctx, BASE + 8, plane, None, *sizes) & 0xFFFFFFFF == BAD_PARAMETER
    for null in ("ctx", "jobs", "subpel_controls", "filter_controls"):
        assert _window_call(svtme, lib, ctx, null=null) == BAD_PARAMETER, null
    assert _window_call(svtme, lib, ctx, n=0) == BAD_PARAMETER
    assert _window_call(svtme, lib, ctx, n=svtme.MAX_BATCH_JOBS + 1) == BAD_PARAMETER
    assert _window_call(svtme, lib, ctx, stride=127) == BAD_PARAMETER
    assert _window_call(svtme, lib, ctx, uv_strides=(63, 64)) == BAD_PARAMETER
    assert _window_call(svtme, lib, ctx, uv_strides=(64, 63)) == BAD_PARAMETER


def test_tffhc_bad_parameters_without_a_device(svtme):
    """The checks that need no context run before the context is touched: a block of zero bytes
    stands in for it."""
    lib = svtme.load_product()
    fake = C.create_string_buffer(64)
    _context_free_errors(svtme, lib, C.cast(fake, C.c_void_p))
    assert fake.raw == bytes(64)


def test_tffhc_case_list_matches_generator():
    assert CASES == GHC.case_dicts()
    assert CASES[:5] == GC.case_dicts()  # the five 8-bit chroma cases: sizes, seeds, random_subpel, controls
    assert [(c["id"], c["kind"], c["w"], c["h"]) for c in CASES[5:]] == [("c64_clip", "clip", 64, 64)]
    shapes = {(c["w"], c["h"], len(c["refs"])) for c in CASES}
    assert shapes >= {(64, 64, 2), (72, 40, 1), (128, 128, 3), (8, 8, 1)}


def test_tffhc_coverage_counts_are_all_non_zero():
    assert set(DOC["coverage"]) == set(GHC.COVERAGE_KEYS) == set(GC.COVERAGE_KEYS) | {"clip_low_uv", "clip_high_uv"}
    assert [k for k, v in DOC["coverage"].items() if not v > 0] == []
    assert set(DOC["coverage_per_case"]) == {c["id"] for c in CASES}
    for k in GHC.COVERAGE_KEYS:
        assert sum(c.get(k, 0) for c in DOC["coverage_per_case"].values()) == DOC["coverage"][k], k
    assert DOC["weights_sse_max"] == [256 * 1023 * 1023, 64 * 1023 * 1023]


def test_tffhc_fixture_shapes(svtme, gold):
    names = [c["id"] + "." + s for c in CASES for s in GHC.FIXTURE_KEYS]
    assert sorted(gold) == sorted(names + ["weights.in", "weights.out"])
    for case in CASES:
        W, H = svtme.align8(case["w"]), svtme.align8(case["h"])
        n, sbs, name = len(case["refs"]), svtme.sb_total(W, H), case["id"]
        assert gold[name + ".y"].shape == (H, W)
        for plane in ("y", "cb", "cr"):
            assert gold[f"{name}.{plane}"].dtype == np.uint16 and gold[f"{name}.{plane}"].max() <= 1023
        assert gold[name + ".cb"].shape == gold[name + ".cr"].shape == (H // 2, W // 2)
        assert gold[name + ".err32"].shape == (n, sbs, 4) and gold[name + ".weights_uv"].shape == (n, sbs, 2, 16)
        assert gold[name + ".subpel"].tobytes() == GF.random_subpel(case).tobytes()
    assert gold["weights.in"].shape == (320, GHC.WEIGHT_COLS) and gold["weights.out"].shape == (320, 4)
    size = os.path.getsize(os.path.join(GOLD, "tffhc_cases.npz"))
    assert os.path.getsize(os.path.join(GOLD, "tffc_cases.npz")) < size < os.path.getsize(os.path.join(GOLD, "tffh_cases.npz"))


def test_tffhc_inputs_keep_the_8bit_pictures_and_reach_both_clips():
    """The MSB planes of every 10-bit frame are the 8-bit frames (so the 8-bit chroma cases' geometry, MVs
    and sub-pel results carry over); the clip case's chroma holds 0 and 1023 next to mid-grey."""
    for case in CASES:
        c8, c10 = GHC.chroma_frames8(case), GHC.chroma_frames10(case)
        if case["kind"] != "clip":
            assert all(np.array_equal(a, b) for t in c8 for a, b in zip(c8[t], GC.chroma_frames(case)[t]))
        for t in c8:
            for p8, p10 in zip(c8[t], c10[t]):
                assert p10.dtype == np.uint16 and np.array_equal(p10 >> 2, p8) and p10.max() <= 1023
                assert p10.shape == ((case["h"] + 1) >> 1, (case["w"] + 1) >> 1)
            assert not np.array_equal(c10[t][0], c10[t][1])
        if case["kind"] == "clip":
            assert all((f == 0).any() and (f == 1023).any() and ((f >= 512) & (f < 516)).any()
                       for pair in c10.values() for f in pair)
            per = DOC["coverage_per_case"][case["id"]]
            assert per["clip_low_uv"] > 0 and per["clip_high_uv"] > 0


def test_tffhc_padding_is_replication():
    c = np.arange(3 * 2, dtype=np.uint16).reshape(2, 3) * 150
    p = GHC.pad_chroma16(c, 8, 8)
    assert p.dtype == np.uint16 and p.shape == (4 + 2 * PAD, 4 + 2 * PAD) and np.array_equal(p[PAD:PAD + 2, PAD:PAD + 3], c)
    assert (p[:PAD, :PAD] == c[0, 0]).all() and (p[PAD + 2:, PAD + 3:] == c[1, 2]).all() and (p[PAD, PAD + 3:] == c[0, 2]).all()


_model_results = {}


def model_case(case):
    if case["id"] not in _model_results:
        _model_results[case["id"]] = MHC.run_case(case)
    return _model_results[case["id"]]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_tffhc_model_equals_fixture(gold, case):
    res, cover = model_case(case)
    for name in GHC.FIXTURE_KEYS:
        assert np.array_equal(res[name], gold[case["id"] + "." + name]), name
    assert {k: v for k, v in cover.items() if v} == DOC["coverage_per_case"][case["id"]]


def test_tffhc_model_equals_fixture_weights(gold):
    tuples = gold["weights.in"]
    assert np.array_equal(tuples, GHC.weight_tuples())
    assert tuples[:, 6:GF.WEIGHT_COLS:4].max() == 256 * 1023 * 1023 and tuples[:, GF.WEIGHT_COLS + 1:].max() == 64 * 1023 * 1023
    assert set(tuples[:, 0]) == {0, 1}  # the split and the unsplit path
    got = MHC.model_weights(tuples)
    assert np.array_equal(got, gold["weights.out"])
    import tff_model as M
    assert got[:113, 0].tolist() == [(e * 1000) >> 16 for e in M.EXP_TAB]  # the first 113 tuples walk the exp table


def test_tffhc_chroma_window_error_is_scaled_as_the_reference_scales_it():
    """Landmarks of the chroma weights: a chroma SSE below 16 is 0; the chroma window error is 4 x (SSE >> 4)
    and counts 5 : 1 against the luma window error (16x16 SSE >> 4); the block errors drop 4 or 6 bits."""
    args = dict(mvx=0, mvy=0, decay=32 << 10, dist_th=64)
    w = MHC.chroma_weight_hbd
    assert w(15, 15, 0, split=True, **args) == w(0, 0, 0, split=True, **args) == 1000
    assert w(16 * 12, 0, 0, split=True, **args) < 1000  # window 48 -> (48 * 5 / 6) * 5 / 6 = 33 -> index 4
    assert w(0, 16 * 5 * 12, 0, split=True, **args) == w(16 * 3, 0, 0, split=True, **args)  # 60 luma = 12 chroma window
    assert w(0, 0, 15, split=True, **args) == 1000 and w(0, 0, 16 * 48, split=True, **args) < 1000
    assert w(0, 0, 64 * 48 - 1, split=False, **args) == w(0, 0, 63 * 48, split=False, **args)


@pytest.mark.skipif(not (ref_available() and GF.reference_headers()),
                    reason="oracle/_ref not built or the reference's headers absent (the offsetof probe needs them)")
def test_tffhc_fixture_regenerates(gold):
    ar = GHC.RefArithUVH()
    for name in ("c72_rand", "c8_rand", "c64_clip"):
        case = case_by_id(name)
        res = GHC.run_case(case, ar, {k: 0 for k in GHC.COUNTED_KEYS})
        for key in GHC.FIXTURE_KEYS:
            assert res[key].tobytes() == gold[name + "." + key].tobytes(), (name, key)
    tuples = gold["weights.in"]
    assert GHC.reference_weights(tuples[::7]).tobytes() == np.ascontiguousarray(gold["weights.out"][::7]).tobytes()


# ----------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------
def upload_yuv10(gpu, case, base=BASE, luma16=True, chroma16=True, chroma8=False):
    """The 10-bit pictures of a case or window: the MSB pyramid and, attached, the 16-bit luma plane, the
    16-bit chroma planes and (chroma8) the 8-bit chroma planes. -> ({picture: y}, {picture: (cb, cr)})."""
    frames, uv = GH.frames10(case), GHC.chroma_frames10(case)
    for t, f in frames.items():
        gpu.upload(base + t, f)
        if chroma16:  # before the luma: the two attaches may come in either order
            gpu.attach_chroma_10bit(base + t, uv[t][0], uv[t][1], case["w"], case["h"])
        if luma16:
            gpu.attach_10bit(base + t, f)
        if chroma8:
            gpu.upload_chroma(base + t, (uv[t][0] >> 2).astype(np.uint8), (uv[t][1] >> 2).astype(np.uint8), case["w"],
                              case["h"])
    return frames, uv


def release(gpu, numbers, base=BASE):
    for t in numbers:
        try:
            gpu.release(base + t)
        except RuntimeError:  # not resident: the test failed before it made the picture
            pass


def assert_planes_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        y, x = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}: {int((got != want).sum())} pixels differ, first at x {x} y {y}: "
                             f"{got[y, x]} for {want[y, x]}")


def run_filter_yuv10(svtme, gpu, case, subpel, refs=None, controls=None, **kw):
    refs = case["refs"] if refs is None else refs
    ctl = svtme.TfFilterYuvControls.from_dict(case["controls"] if controls is None else controls)
    return gpu.tf_filter_yuv_10bit(BASE + case["centre"], [BASE + r for r in refs], case["w"], case["h"], ctl, subpel, **kw)


def state_of(gpu, numbers, base=BASE):
    """Every resident plane of the pictures by name: three luma levels and, where attached, the 16-bit luma
    plane, the 16-bit chroma planes and the 8-bit chroma planes, margins included."""
    out = {}
    for t in numbers:
        st = {f"l{lv}": gpu.download(base + t, lv) for lv in range(3)}
        for name, fn in (("y16", lambda: gpu.download_10bit(base + t)),
                         ("cb16", lambda: gpu.download_chroma_10bit(base + t, 1)),
                         ("cr16", lambda: gpu.download_chroma_10bit(base + t, 2)),
                         ("cb8", lambda: gpu.download_chroma(base + t, 1)),
                         ("cr8", lambda: gpu.download_chroma(base + t, 2))):
            try:
                st[name] = fn()
            except RuntimeError:
                pass
        out[t] = st
    return out


def assert_state(got, want, what):
    assert sorted(got) == sorted(want), what
    for t in want:
        assert sorted(got[t]) == sorted(want[t]), (what, t, sorted(got[t]), sorted(want[t]))
        for k in want[t]:
            a, b = got[t][k], want[t][k]
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (what, t, k)


ALL16 = ["cb16", "cr16", "l0", "l1", "l2", "y16"]


def assert_fixture(gold, case, y, cb, cr, err32, what=""):
    name, w, h = case["id"], case["w"], case["h"]
    assert np.array_equal(err32, gold[name + ".err32"]), (name, what)
    assert_planes_equal(y, gold[name + ".y"][:h, :w], f"{name} y {what}")
    assert_planes_equal(cb, gold[name + ".cb"][:(h + 1) >> 1, :(w + 1) >> 1], f"{name} cb {what}")
    assert_planes_equal(cr, gold[name + ".cr"][:(h + 1) >> 1, :(w + 1) >> 1], f"{name} cr {what}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_tffhc_vs_reference_golden(svtme, gpu, gold, case):
    """y, cb, cr and err32 of svtme_tf_filter_yuv_10bit equal the fixture, and y and err32 equal
    svtme_tf_filter_10bit's on the same window byte for byte."""
    sub = gold[case["id"] + ".subpel"]
    frames, _ = upload_yuv10(gpu, case)
    try:
        y, cb, cr, err32 = run_filter_yuv10(svtme, gpu, case, sub)
        y1, e1 = gpu.tf_filter_10bit(BASE + case["centre"], [BASE + r for r in case["refs"]], case["w"], case["h"],
                                     svtme.TfFilterControls.from_dict(GC.luma_controls(case["controls"])), sub)
    finally:
        release(gpu, frames)
    assert_fixture(gold, case, y, cb, cr, err32)
    assert y.tobytes() == np.ascontiguousarray(y1).tobytes() and err32.tobytes() == e1.tobytes()


SWEEP = [(64, 64, "frac", (7, 9), 51), (64, 64, "clip", (9,), 52), (72, 40, "frac", (7, 9, 6), 53),
         (72, 40, "clip", (7,), 54)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,kind,refs,seed", SWEEP, ids=[f"{w}x{h}_{k}_{s}" for w, h, k, _, s in SWEEP])
def test_tffhc_random_sweep_vs_model(svtme, gpu, w, h, kind, refs, seed):
    """Seeded random sub-pel results (every branch, splits, MVs far beyond each edge) and seeded controls
    against the model."""
    rng = np.random.default_rng(seed)
    pick = lambda: int(rng.choice(GF.DECAYS + (1024, 500_000, 8_000_000, 0xFFFFFFFF)))  # noqa: E731
    case = {"id": f"sweep{seed}", "kind": kind, "w": w, "h": h, "centre": 8, "refs": list(refs), "seed": seed,
            "controls": {"tf_decay_factor_fp16": pick(), "tf_mv_dist_th": int(rng.choice(GF.DIST_THS + (1, 10, 100, 200))),
                         "sub_sampling_shift": int(rng.integers(0, 2)), "tf_decay_factor_cb_fp16": pick(),
                         "tf_decay_factor_cr_fp16": pick()}}
    sub = GF.random_subpel(case)
    frames, _ = upload_yuv10(gpu, case)
    try:
        y, cb, cr, err32 = run_filter_yuv10(svtme, gpu, case, sub)
    finally:
        release(gpu, frames)
    pics, uv, _ = GHC.case_inputs(case)
    want, _ = MHC.filter_window_yuv(pics[8], [pics[r] for r in refs], uv[8], [uv[r] for r in refs], case["controls"], sub)
    assert np.array_equal(err32, want["err32"]), case
    assert_planes_equal(y, want["y"][:h, :w], f"{case} y")
    assert_planes_equal(cb, want["cb"][:(h + 1) >> 1, :(w + 1) >> 1], f"{case} cb")
    assert_planes_equal(cr, want["cr"][:(h + 1) >> 1, :(w + 1) >> 1], f"{case} cr")


@pytest.mark.gpu
def test_tffhc_window_of_three_in_three_orders(svtme, gpu, gold):
    case = case_by_id("c128_rand")
    sub = gold[case["id"] + ".subpel"]
    frames, _ = upload_yuv10(gpu, case)
    try:
        for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
            y, cb, cr, err32 = run_filter_yuv10(svtme, gpu, case, sub[list(order)], refs=[case["refs"][k] for k in order])
            assert np.array_equal(err32, gold[case["id"] + ".err32"][list(order)])
            assert_fixture(gold, case, y, cb, cr, gold[case["id"] + ".err32"], f"order {order}")
    finally:
        release(gpu, frames)


@pytest.mark.gpu
def test_tffhc_strides_null_outputs_and_the_pictures_stay(svtme, gpu, gold):
    case = case_by_id("c72_rand")
    w, h = case["w"], case["h"]
    cw = (w + 1) >> 1
    numbers = [case["centre"]] + case["refs"]
    sub = gold[case["id"] + ".subpel"]
    frames, _ = upload_yuv10(gpu, case)
    try:
        before = state_of(gpu, numbers)
        assert all(sorted(v) == ALL16 for v in before.values())
        y, cb, cr, err32 = run_filter_yuv10(svtme, gpu, case, sub)
        assert_fixture(gold, case, y, cb, cr, err32)
        y1, cb1, cr1, e1 = run_filter_yuv10(svtme, gpu, case, sub, with_err32=False, want=("cr",))
        assert e1 is None and cb1 is None
        assert_planes_equal(y1, y, "NULL err32 and cb: y")
        assert_planes_equal(cr1, cr, "NULL err32 and cb: cr")
        y2, cb2, cr2, _ = run_filter_yuv10(svtme, gpu, case, sub, want=("cb",))
        assert cr2 is None
        assert_planes_equal(cb2, cb, "NULL cr: cb")
        y3, cb3, cr3, e3 = run_filter_yuv10(svtme, gpu, case, sub, strides=(w + 13, cw + 3, cw + 9))
        for got, want, width, what in ((y3, y, w, "y"), (cb3, cb, cw, "cb"), (cr3, cr, cw, "cr")):
            assert_planes_equal(np.ascontiguousarray(got), want, "strides above the widths: " + what)
            assert (got.base[:, width:] == 0).all(), what  # the samples beyond the plane stay as they were
        assert np.array_equal(e3, err32)
        assert_state(state_of(gpu, numbers), before, "no resident picture is modified")
    finally:
        release(gpu, frames)


def numpy_repad(plane, W, H):
    return np.pad(plane, ((PAD, PAD + H // 2 - plane.shape[0]), (PAD, PAD + W // 2 - plane.shape[1])), mode="edge")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(121, 67), (124, 66)])
def test_tffhc_attach_download_equals_numpy_repad(svtme, gpu, w, h):
    """Odd true chroma sizes (61 x 34, 62 x 33) against a numpy edge pad; a second attach replaces the
    planes; no other plane of the picture is touched; either order of the two attaches."""
    rng = np.random.default_rng(w * 1000 + h)
    W, H = svtme.align8(w), svtme.align8(h)
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    y = rng.integers(0, 1024, (h, w), dtype=np.uint16)
    cb, cr, cb2, cr2 = (rng.integers(0, 1024, (ch, cw), dtype=np.uint16) for _ in range(4))
    gpu.upload(BASE + 1, y)
    try:
        gpu.attach_10bit(BASE + 1, y)
        before = state_of(gpu, [1])[1]
        gpu.attach_chroma_10bit(BASE + 1, cb, cr, w, h)
        for plane, src in ((1, cb), (2, cr)):
            got = gpu.download_chroma_10bit(BASE + 1, plane)
            assert got.shape == (H // 2 + 2 * PAD, W // 2 + 2 * PAD)
            assert_planes_equal(got, numpy_repad(src, W, H), f"{w}x{h} plane {plane}")
        # rows `stride` samples apart, and a second attach replaces the planes
        wide = np.full((2, ch, cw + 7), 0x3FF, np.uint16)
        wide[0, :, :cw], wide[1, :, :cw] = cb2, cr2
        assert gpu.lib.svtme_picture_attach_chroma_10bit(gpu.ctx, BASE + 1, wide[0].ctypes.data, wide[1].ctypes.data,
                                                         cw + 7, w, h) == 0
        assert_planes_equal(gpu.download_chroma_10bit(BASE + 1, 1), numpy_repad(cb2, W, H), "second attach cb")
        assert_planes_equal(gpu.download_chroma_10bit(BASE + 1, 2), numpy_repad(cr2, W, H), "second attach cr")
        after = state_of(gpu, [1])[1]
        assert sorted(after) == ALL16
        assert_state({1: {k: after[k] for k in before}}, {1: before}, "the other planes stay")
        # chroma first, luma second
        gpu.upload(BASE + 2, y)
        gpu.attach_chroma_10bit(BASE + 2, cb2, cr2, w, h)
        gpu.attach_10bit(BASE + 2, y)
        assert_state({1: state_of(gpu, [2])[2]}, {1: after}, "either order")
    finally:
        release(gpu, [1, 2])


def yuv_window_10(w, h, refs, kind="frac"):
    win = TW.own_window(w, h, refs, "l8", kind)
    win["filter"] = dict(win["filter"], tf_decay_factor_cb_fp16=3_000_000, tf_decay_factor_cr_fp16=1_000_000)
    return win


def window_controls(svtme, win):
    return svtme.TfSubpelControls.from_dict(win["subpel"]), svtme.TfFilterYuvControls.from_dict(win["filter"])


def luma_controls(svtme, win):
    return svtme.TfSubpelControls.from_dict(win["subpel"]), svtme.TfFilterControls.from_dict(GC.luma_controls(win["filter"]))


def run_window_yuv10(svtme, gpu, win, out_pn, centre_pn=None, refs_pn=None, want=None):
    centre_pn = BASE + win["centre"] if centre_pn is None else centre_pn
    refs_pn = [BASE + r for r in win["refs"]] if refs_pn is None else refs_pn
    jobs = [TW.tf_job(svtme, win, centre_pn, r) for r in refs_pn]
    sp, fc = window_controls(svtme, win)
    kw = {} if want is None else {"want": want}
    return gpu.tf_window_yuv_10bit(jobs, win["w"], win["h"], sp, fc, out_pn, **kw)


def me_and_subpel(svtme, gpu, win, centre_pn, refs):
    layout = svtme.PackLayout(n_pus=85, max_cand=1, max_refs=1, full_records=1, sb_results=0)
    me = np.stack([np.frombuffer(gpu.submit_packed(TW.tf_job(svtme, win, centre_pn, r), layout), svtme.REF_RECORD_DTYPE)
                   for r in refs])
    return me, gpu.tf_subpel(centre_pn, refs, win["w"], win["h"], svtme.TfSubpelControls.from_dict(win["subpel"]), me)


def separate_calls(svtme, gpu, win, centre_pn=None, refs_pn=None) -> dict:
    """The window as the three calls through host memory, named as tf_window_yuv_10bit's result."""
    centre_pn = BASE + win["centre"] if centre_pn is None else centre_pn
    refs = [BASE + r for r in win["refs"]] if refs_pn is None else refs_pn
    me, sub = me_and_subpel(svtme, gpu, win, centre_pn, refs)
    y, cb, cr, err32 = gpu.tf_filter_yuv_10bit(centre_pn, refs, win["w"], win["h"], window_controls(svtme, win)[1], sub)
    return {"plane": (y >> 2).astype(np.uint8), "records": me, "subpel": sub, "err32": err32, "plane16": y, "cb": cb,
            "cr": cr}


def assert_same_yuv10(svtme, got, want, what):
    keys16 = ("plane16", "cb", "cr")
    TW.assert_same(svtme, {k: v for k, v in got.items() if k not in keys16},
                   {k: v for k, v in want.items() if k not in keys16}, what)
    for k in keys16:
        assert_planes_equal(got[k], want[k], f"{what} {k}")


def attach_result(gpu, number, res, w, h):
    """What the window's result picture must equal: upload + both attaches of the filtered planes."""
    gpu.upload(BASE + number, res["plane16"])
    gpu.attach_10bit(BASE + number, res["plane16"])
    gpu.attach_chroma_10bit(BASE + number, res["cb"], res["cr"], w, h)


WINDOWS = [(72, 40, (7,)), (121, 67, (7, 9)), (128, 128, (7, 9, 6))]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,refs", WINDOWS, ids=[f"{w}x{h}" for w, h, _ in WINDOWS])
def test_tffhc_window_equals_the_separate_calls_fresh_and_in_place(svtme, gpu, w, h, refs):
    """svtme_tf_window_yuv_10bit against submit_packed -> tf_subpel -> tf_filter_yuv_10bit, array for array;
    the resident result (every download, chroma margins included) is what svtme_picture_upload_10bit,
    svtme_picture_attach_10bit and svtme_picture_attach_chroma_10bit of the filtered planes leave; in
    place it is the same as into a fresh number."""
    win = yuv_window_10(w, h, refs)
    what = f"{w}x{h}, references {refs}"
    numbers = [win["centre"]] + list(refs)
    upload_yuv10(gpu, win)
    try:
        before = state_of(gpu, numbers)
        want = separate_calls(svtme, gpu, win)
        assert all(len(np.unique(want[k] & 3)) == 4 for k in ("plane16", "cb", "cr"))  # the result is 10-bit deep
        got = run_window_yuv10(svtme, gpu, win, BASE + OUT)
        assert_same_yuv10(svtme, got, want, what)
        assert_state(state_of(gpu, numbers), before, what + ": the window's pictures stay")
        fresh = state_of(gpu, [OUT])
        assert sorted(fresh[OUT]) == ALL16
        attach_result(gpu, OUT + 1, got, w, h)
        assert_state({OUT: state_of(gpu, [OUT + 1])[OUT + 1]}, fresh, what + ": the resident result")
        # in place: only some outputs asked for
        place = run_window_yuv10(svtme, gpu, win, BASE + win["centre"], want=("plane16", "cb", "cr"))
        assert sorted(place) == ["cb", "cr", "plane16"]
        for k in place:
            assert_planes_equal(place[k], got[k], f"{what} in place {k}")
        after = state_of(gpu, numbers)
        assert_state({OUT: after[win["centre"]]}, fresh, what + ": in place")
        assert_state({t: after[t] for t in refs}, {t: before[t] for t in refs}, what + ": the references stay")
    finally:
        release(gpu, numbers + [OUT, OUT + 1])


@pytest.mark.gpu
def test_tffhc_second_window_reads_the_filtered_picture(svtme, gpu):
    """The result of one window is a reference of the next with nothing waited for in between: the second
    window equals the one whose reference was uploaded and attached from the first's host copies."""
    w, h = 121, 67
    first, second = yuv_window_10(w, h, (7, 9)), yuv_window_10(w, h, (7,))
    frames, _ = upload_yuv10(gpu, first)
    try:
        res = run_window_yuv10(svtme, gpu, first, BASE + OUT)
        attach_result(gpu, OUT + 1, res, w, h)
        want = run_window_yuv10(svtme, gpu, second, BASE + OUT + 2, centre_pn=BASE + 9, refs_pn=[BASE + OUT + 1])
        run_window_yuv10(svtme, gpu, first, BASE + OUT, want=())  # queued; returns at once
        got = run_window_yuv10(svtme, gpu, second, BASE + OUT + 3, centre_pn=BASE + 9, refs_pn=[BASE + OUT])
        assert_same_yuv10(svtme, got, want, "second window")
        assert_state({0: state_of(gpu, [OUT + 3])[OUT + 3]}, {0: state_of(gpu, [OUT + 2])[OUT + 2]}, "second result")
    finally:
        release(gpu, list(frames) + [OUT, OUT + 1, OUT + 2, OUT + 3])


@pytest.mark.gpu
def test_tffhc_refused_calls_leave_every_picture(svtme, gpu):
    win = yuv_window_10(128, 128, (7, 9))
    numbers = [8, 7, 9]
    frames, uv = upload_yuv10(gpu, win)
    lib, ctx = gpu.lib, gpu.ctx
    try:
        gpu.upload(BASE + 6, frames[7])  # a picture with the 16-bit luma plane and no 16-bit chroma
        gpu.attach_10bit(BASE + 6, frames[7])
        gpu.upload(BASE + 5, frames[7])  # a picture with 16-bit chroma and no 16-bit luma plane
        gpu.attach_chroma_10bit(BASE + 5, uv[7][0], uv[7][1], 128, 128)
        before = state_of(gpu, numbers + [6, 5])
        _context_free_errors(svtme, lib, ctx)
        for refs, centre, message in (([BASE + 7, BASE + 6], BASE + 8, "no 10-bit chroma"),
                                      ([BASE + 7], BASE + 6, "no 10-bit chroma"),
                                      ([BASE + 7, BASE + 5], BASE + 8, "no 10-bit plane"),
                                      ([BASE + 999], BASE + 8, "not resident")):
            assert _filter_call(svtme, lib, ctx, refs, centre=centre) == BAD_PARAMETER
            assert message in lib.svtme_last_error().decode(), (refs, centre)
        assert _filter_call(svtme, lib, ctx, [BASE + 7], w=64, h=64) == BAD_PARAMETER  # another size
        for refs_pn, out_pn in (([BASE + 7, BASE + 6], BASE + OUT), ([BASE + 7, BASE + 6], BASE + 8),
                                ([BASE + 7, BASE + 5], BASE + OUT), ([BASE + 7, BASE + 999], BASE + OUT),
                                ([BASE + 7, BASE + 9], BASE + 9)):
            with pytest.raises(RuntimeError, match="0x80001005"):
                run_window_yuv10(svtme, gpu, win, out_pn, refs_pn=refs_pn)
        with pytest.raises(RuntimeError):  # no result picture was made
            gpu.download(BASE + OUT, 0)
        assert_state(state_of(gpu, numbers + [6, 5]), before, "refused calls")
        # and the valid forms succeed
        assert _filter_call(svtme, lib, ctx, [BASE + 7, BASE + 9]) == 0
        assert _filter_call(svtme, lib, ctx, [BASE + 7], strides=(200, 70, 90), with_err32=False) == 0
    finally:
        release(gpu, numbers + [6, 5, OUT])


DROPS = ("luma upload", "invalidate", "svtme_tf_window result", "svtme_tf_window_yuv result", "svtme_tf_window_10bit result")


@pytest.mark.gpu
@pytest.mark.parametrize("event", DROPS, ids=[d.replace(" ", "_") for d in DROPS])
def test_tffhc_events_that_drop_the_chroma(svtme, gpu, event):
    """Each event that replaces a picture's luma drops its 16-bit chroma: the download fails, and with the
    16-bit luma plane attached again a yuv 10-bit call that reads the picture is refused for the chroma
    alone, until the chroma is attached again."""
    win = yuv_window_10(64, 64, (7,))
    frames, uv = upload_yuv10(gpu, win, chroma8=True)
    lib, ctx = gpu.lib, gpu.ctx
    x = 6  # the picture the event falls on: a second reference of the filter call
    jobs = [TW.tf_job(svtme, win, BASE + 8, BASE + 7)]
    try:
        gpu.upload(BASE + x, frames[7])
        gpu.attach_10bit(BASE + x, frames[7])
        gpu.attach_chroma_10bit(BASE + x, uv[7][0], uv[7][1], 64, 64)
        refs = [BASE + 7, BASE + x]
        assert _filter_call(svtme, lib, ctx, refs, w=64, h=64) == 0
        if event == "luma upload":
            gpu.upload(BASE + x, frames[7])
        elif event == "invalidate":
            gpu.invalidate(BASE + x, (frames[7] >> 2).astype(np.uint8))
        elif event == "svtme_tf_window result":
            gpu.tf_window(jobs, 64, 64, *luma_controls(svtme, win), BASE + x)
        elif event == "svtme_tf_window_yuv result":
            gpu.tf_window_yuv(jobs, 64, 64, *window_controls(svtme, win), BASE + x)
        else:
            gpu.tf_window_10bit(jobs, 64, 64, *luma_controls(svtme, win), BASE + x)
        with pytest.raises(RuntimeError, match="no 10-bit chroma"):
            gpu.download_chroma_10bit(BASE + x, 1)
        assert _filter_call(svtme, lib, ctx, refs, w=64, h=64) == BAD_PARAMETER
        if event == "svtme_tf_window_10bit result":  # its result carries the new 16-bit luma plane
            assert "no 10-bit chroma" in lib.svtme_last_error().decode()
        else:
            assert "no 10-bit plane" in lib.svtme_last_error().decode()
            gpu.attach_10bit(BASE + x, frames[7])
            assert _filter_call(svtme, lib, ctx, refs, w=64, h=64) == BAD_PARAMETER
            assert "no 10-bit chroma" in lib.svtme_last_error().decode()
        with pytest.raises(RuntimeError, match="0x80001005"):
            run_window_yuv10(svtme, gpu, win, BASE + OUT, refs_pn=[BASE + x])
        gpu.attach_chroma_10bit(BASE + x, uv[7][0], uv[7][1], 64, 64)
        assert _filter_call(svtme, lib, ctx, refs, w=64, h=64) == 0
        # planes for a picture of another size, or one that is not resident
        assert _attach_call(lib, ctx) == BAD_PARAMETER  # BASE + 8 is 64 x 64, not 121 x 67
        assert _attach_call(lib, ctx, w=64, h=64, pn=BASE + 999) == BAD_PARAMETER
    finally:
        release(gpu, list(frames) + [x, OUT])


@pytest.mark.gpu
def test_tffhc_result_drops_8bit_chroma(svtme, gpu):
    """A svtme_tf_window_yuv_10bit result under a number drops the 8-bit chroma under it."""
    win = yuv_window_10(64, 64, (7,))
    frames, uv = upload_yuv10(gpu, win)
    try:
        gpu.upload_chroma(BASE + 8, (uv[8][0] >> 2).astype(np.uint8), (uv[8][1] >> 2).astype(np.uint8), 64, 64)
        assert "cb8" in state_of(gpu, [8])[8]
        run_window_yuv10(svtme, gpu, win, BASE + 8, want=())
        assert sorted(state_of(gpu, [8])[8]) == ALL16
    finally:
        release(gpu, list(frames))


@pytest.mark.gpu
def test_tffhc_existing_calls_do_not_see_the_chroma(svtme, gpu):
    """svtme_tf_filter_10bit, svtme_tf_window_10bit, svtme_tf_filter_yuv and svtme_tf_filter on pictures with
    16-bit chroma attached give byte for byte what they give without it."""
    win = yuv_window_10(121, 67, (7, 9))
    numbers = [8, 7, 9]
    res = []
    try:
        for chroma16 in (False, True):
            upload_yuv10(gpu, win, chroma16=chroma16, chroma8=True)
            refs = [BASE + r for r in win["refs"]]
            sp, fc = luma_controls(svtme, win)
            _, sub = me_and_subpel(svtme, gpu, win, BASE + 8, refs)
            p16, e16 = gpu.tf_filter_10bit(BASE + 8, refs, 121, 67, fc, sub)
            y8, cb8, cr8, e8 = gpu.tf_filter_yuv(BASE + 8, refs, 121, 67, window_controls(svtme, win)[1], sub)
            p8, e = gpu.tf_filter(BASE + 8, refs, 121, 67, fc, sub)
            out = gpu.tf_window_10bit([TW.tf_job(svtme, win, BASE + 8, r) for r in refs], 121, 67, sp, fc, BASE + OUT)
            res.append(([p16, e16, y8, cb8, cr8, e8, p8, e], out, state_of(gpu, [OUT])[OUT]))
            release(gpu, numbers + [OUT])
    finally:
        release(gpu, numbers + [OUT])
    (a0, o0, s0), (a1, o1, s1) = res
    assert all(np.array_equal(x, y) for x, y in zip(a0, a1))
    TW.assert_same(svtme, {k: v for k, v in o1.items() if k != "plane16"}, {k: v for k, v in o0.items() if k != "plane16"},
                   "tf_window_10bit with 16-bit chroma attached")
    assert np.array_equal(o0["plane16"], o1["plane16"])
    assert_state({0: s1}, {0: s0}, "tf_window_10bit's result")
    assert sorted(s1) == ["l0", "l1", "l2", "y16"]
