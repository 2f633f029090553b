"""Temporal filtering of 10-bit luma: the resident 16-bit plane (svtme_picture_attach_10bit,
svtme_picture_download_10bit) and the 10-bit calls (svtme_tf_filter_10bit,
svtme_tf_window_10bit), include/svtme.h.

Expected values are the fixtures tests/golden/tffh_cases.{json,npz}: the reference's
svt_highbd_inter_predictor, its 10-bit variance and its high-bit-depth filter functions
under the glue of tests/golden/make_golden_tff.py (make_golden_tffh.py). Beside them
stands a model in numpy and Python integers (tests/tffh_model.py). CPU tests pin the ABI,
the argument checks that need no context, the fixtures and the model to the fixtures; GPU
tests compare the calls with the fixtures, the model, each other and the 8-bit calls.
Every comparison is exact.
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
import make_golden_tffh as GH  # noqa: E402
import test_tf_window as TW  # noqa: E402  (its window helpers; its tests are collected from its own file)
import tffh_model as MH  # noqa: E402

DOC = json.load(open(os.path.join(GOLD, "tffh_cases.json")))
CASES = DOC["cases"]
BAD_PARAMETER = 0x80001005
BASE = 14000  # picture numbers of this file's uploads
OUT = 900     # + BASE: the result picture of a window into a fresh number
SYMBOLS = ("svtme_picture_attach_10bit", "svtme_picture_download_10bit", "svtme_tf_filter_10bit", "svtme_tf_window_10bit")


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLD, "tffh_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def case_by_id(name):
    return next(c for c in CASES if c["id"] == name)


def subpel_of(gold, case):
    return gold[case["id"] + ".subpel"] if case["subpel"] == "random" else GH.case_inputs(case)[1]


# ----------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------
def test_tffh_symbols_exported(svtme):
    lib = svtme.load_product()
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []


# each new function assigned to a pointer of the type the Python prototypes assume: a header that
# differs does not compile
_PROTO_PROGRAM = r"""
#include "svtme.h"
svtme_status (*p_attach)(svtme_ctx *, uint64_t, const uint16_t *, uint32_t, uint32_t, uint32_t) = svtme_picture_attach_10bit;
svtme_status (*p_download)(svtme_ctx *, uint64_t, uint16_t *, uint32_t *, uint32_t *, uint32_t *, uint32_t *) =
    svtme_picture_download_10bit;
svtme_status (*p_filter)(svtme_ctx *, uint64_t, const uint64_t *, uint32_t, uint32_t, uint32_t,
                         const svtme_tf_filter_controls *, const svtme_tf_subpel_sb *, uint16_t *, uint32_t,
                         uint32_t *) = svtme_tf_filter_10bit;
svtme_status (*p_window)(svtme_ctx *, const svtme_job *, uint32_t, uint32_t, uint32_t, const svtme_tf_subpel_controls *,
                         const svtme_tf_filter_controls *, uint64_t, const svtme_tf_window_out *, uint16_t *,
                         uint32_t) = svtme_tf_window_10bit;
"""


def test_tffh_prototypes_equal_the_header(svtme, tmp_path):
    src = tmp_path / "proto.c"
    src.write_text(_PROTO_PROGRAM)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "proto.o")], check=True)
    lib, vp, u32, u64 = svtme.load_product(), C.c_void_p, C.c_uint32, C.c_uint64
    pu32 = C.POINTER(u32)
    want = {"svtme_picture_attach_10bit": [vp, u64, vp, u32, u32, u32],
            "svtme_picture_download_10bit": [vp, u64, vp, pu32, pu32, pu32, pu32],
            "svtme_tf_filter_10bit": [vp, u64, C.POINTER(u64), u32, u32, u32, C.POINTER(svtme.TfFilterControls), vp, vp,
                                      u32, vp],
            "svtme_tf_window_10bit": [vp, C.POINTER(svtme.Job), u32, u32, u32, C.POINTER(svtme.TfSubpelControls),
                                      C.POINTER(svtme.TfFilterControls), u64, C.POINTER(svtme.TfWindowOut), vp, u32]}
    for name, argtypes in want.items():
        assert list(getattr(lib, name).argtypes) == argtypes, name
        assert getattr(lib, name).restype is C.c_int32, name


def _controls(svtme, **over):
    return svtme.TfFilterControls.from_dict(dict({"tf_decay_factor_fp16": 2_000_000, "tf_mv_dist_th": 64,
                                                  "sub_sampling_shift": 1}, **over))


def _filter_call(svtme, lib, ctx, refs, n=None, ctl=None, null=None, w=128, h=128, centre=BASE + 8, stride=None,
                 branch=0, with_err32=True):
    """-> the status of svtme_tf_filter_10bit; on an error no output may be touched."""
    ctl = ctl if ctl is not None else _controls(svtme)
    sbs = svtme.sb_total(svtme.align8(w), svtme.align8(h))
    slots = max(len(refs), svtme.MAX_BATCH_JOBS + 1)
    arr = (C.c_uint64 * slots)(*refs)
    sub = np.zeros((slots, sbs), svtme.TF_SUBPEL_SB_DTYPE)
    sub["branch"][min(len(refs), slots) - 1, sbs - 1] = branch  # the last struct the call reads
    stride = w if stride is None else stride
    buf = np.full(h * max(stride, w), 0x5A5A, np.uint16)
    e32 = np.full(slots * sbs * 4, 0x5A5A5A5A, np.uint32)
    st = lib.svtme_tf_filter_10bit(None if null == "ctx" else ctx, centre, None if null == "refs" else arr,
                                   len(refs) if n is None else n, w, h, None if null == "controls" else C.byref(ctl),
                                   None if null == "subpel" else sub.ctypes.data,
                                   None if null == "out" else buf.ctypes.data, stride,
                                   e32.ctypes.data if with_err32 else None)
    if st:
        assert (buf == 0x5A5A).all() and (e32 == 0x5A5A5A5A).all()
        assert lib.svtme_last_error().decode() != ""
    return st & 0xFFFFFFFF


def _bad_filter_calls(svtme):
    ok = [BASE + 7]
    for null in ("ctx", "refs", "controls", "subpel", "out"):
        yield "null " + null, dict(refs=ok, null=null)
    yield "n 0", dict(refs=ok, n=0)
    yield "n 17", dict(refs=ok * (svtme.MAX_BATCH_JOBS + 1))
    yield "out_stride under the width", dict(refs=ok, stride=127)
    yield "tf_mv_dist_th 32768", dict(refs=ok, ctl=_controls(svtme, tf_mv_dist_th=32768))
    yield "sub_sampling_shift 2", dict(refs=ok, ctl=_controls(svtme, sub_sampling_shift=2))
    yield "branch 3", dict(refs=ok, branch=3)


def _attach_call(lib, ctx, null=None, w=121, h=67, stride=None, pn=BASE + 8):
    y = np.zeros((max(h, 1), max(w, 1)), np.uint16)
    st = lib.svtme_picture_attach_10bit(None if null == "ctx" else ctx, pn, None if null == "y" else y.ctypes.data,
                                        w if stride is None else stride, w, h)
    return st & 0xFFFFFFFF


def _window_call(svtme, lib, ctx, null=None, n=1, stride=128, w=128, h=128):
    win = TW.own_window(w, h, (7,), "l8")
    jobs = (svtme.Job * (svtme.MAX_BATCH_JOBS + 1))(TW.tf_job(svtme, win, BASE + 8, BASE + 7))
    sp, fc = TW.controls_of(svtme, win)
    p16 = np.full(h * w, 0x5A5A, np.uint16)
    st = lib.svtme_tf_window_10bit(None if null == "ctx" else ctx, None if null == "jobs" else jobs, n, w, h,
                                   None if null == "subpel_controls" else C.byref(sp),
                                   None if null == "filter_controls" else C.byref(fc), BASE + OUT, None, p16.ctypes.data,
                                   stride)
    if st:
        assert (p16 == 0x5A5A).all()
    return st & 0xFFFFFFFF


def _context_free_errors(svtme, lib, ctx):
    for what, kw in _bad_filter_calls(svtme):
        assert _filter_call(svtme, lib, ctx, **kw) == BAD_PARAMETER, what
    for null in ("ctx", "y"):
        assert _attach_call(lib, ctx, null=null) == BAD_PARAMETER, null
    assert _attach_call(lib, ctx, w=0) == BAD_PARAMETER
    assert _attach_call(lib, ctx, h=0) == BAD_PARAMETER
    assert _attach_call(lib, ctx, stride=120) == BAD_PARAMETER
    u32 = C.c_uint32()
    assert lib.svtme_picture_download_10bit(None, BASE + 8, None, C.byref(u32), C.byref(u32), C.byref(u32),
                                            C.byref(u32)) & 0xFFFFFFFF == BAD_PARAMETER
    for null in ("ctx", "jobs", "subpel_controls", "filter_controls"):
        assert _window_call(svtme, lib, ctx, null=null) == BAD_PARAMETER, null
    assert _window_call(svtme, lib, ctx, n=0) == BAD_PARAMETER
    assert _window_call(svtme, lib, ctx, n=svtme.MAX_BATCH_JOBS + 1) == BAD_PARAMETER
    assert _window_call(svtme, lib, ctx, stride=127) == BAD_PARAMETER


def test_tffh_bad_parameters_without_a_device(svtme):
    """The checks that need no context run before the context is touched: a block of zero bytes
    stands in for it."""
    lib = svtme.load_product()
    fake = C.create_string_buffer(64)
    _context_free_errors(svtme, lib, C.cast(fake, C.c_void_p))
    assert fake.raw == bytes(64)


def test_tffh_case_list_matches_generator():
    assert CASES == GH.case_dicts()
    shapes = {(c["w"], c["h"], len(c["refs"])) for c in CASES}
    assert shapes >= {(64, 64, 2), (72, 40, 1), (124, 66, 1), (200, 72, 1), (128, 128, 3)}
    assert all(c["w"] <= 200 and c["h"] <= 128 for c in CASES)
    by_id = {c["id"]: c for c in GF.case_dicts()}
    for c in CASES:  # the cases taken over keep their controls and their sub-pel results
        if c["kind"] != "clip":
            assert c == by_id[c["id"]]
    assert [c["id"] for c in CASES if c["kind"] == "clip"] == ["clip64_rand", "clip72_rand"]
    assert {c["controls"]["sub_sampling_shift"] for c in CASES} == {0, 1}


def test_tffh_coverage_counts_are_all_non_zero():
    assert set(DOC["coverage"]) == set(GH.COVERAGE_KEYS) >= set(GF.COVERAGE_KEYS) | {"clip_low", "clip_high"}
    assert [k for k, v in DOC["coverage"].items() if not v > 0] == []
    assert set(DOC["coverage_per_case"]) == {c["id"] for c in CASES}
    for k in GH.COUNTED_KEYS:
        total = DOC["var_clamped_to_0"] if k == "var_clamped_to_0" else DOC["coverage"][k]
        assert sum(c.get(k, 0) for c in DOC["coverage_per_case"].values()) == total, k
    assert DOC["weights_sse_max"] == 256 * 1023 * 1023


def test_tffh_fixture_shapes(svtme, gold):
    names = [c["id"] + s for c in CASES for s in (".plane", ".err32", ".weights") + ((".subpel",) if c["subpel"] == "random" else ())]
    assert sorted(gold) == sorted(names + ["weights.in", "weights.out"])
    for case in CASES:
        W, H = svtme.align8(case["w"]), svtme.align8(case["h"])
        n, sbs, name = len(case["refs"]), svtme.sb_total(W, H), case["id"]
        assert gold[name + ".plane"].shape == (H, W) and gold[name + ".plane"].dtype == np.uint16
        assert gold[name + ".plane"].max() <= 1023
        assert gold[name + ".err32"].shape == (n, sbs, 4) and gold[name + ".weights"].shape == (n, sbs, 16)
        if case["subpel"] == "random":
            assert gold[name + ".subpel"].tobytes() == GF.random_subpel(case).tobytes()
    assert gold["weights.in"].shape[1] == GF.WEIGHT_COLS and len(gold["weights.in"]) == len(gold["weights.out"]) == 400
    assert os.path.getsize(os.path.join(GOLD, "tffh_cases.npz")) < 1.25 * os.path.getsize(os.path.join(GOLD, "tff_cases.npz"))


def test_tffh_inputs_keep_the_8bit_pictures_and_reach_both_clips():
    """The MSB plane of every 10-bit frame is the 8-bit case's frame (so its sub-pel results are valid); the
    clip cases hold 0 and 1023 next to mid-grey."""
    for case in CASES:
        f8, f10 = GH.frames8(case), GH.frames10(case)
        for t in f8:
            assert f10[t].dtype == np.uint16 and np.array_equal(f10[t] >> 2, f8[t]) and f10[t].max() <= 1023
        if case["kind"] == "clip":
            assert all((f == 0).any() and (f == 1023).any() and ((f >= 512) & (f < 516)).any() for f in f10.values())
            per = DOC["coverage_per_case"][case["id"]]
            assert per["clip_low"] > 0 and per["clip_high"] > 0


def test_tffh_padding_is_replication():
    y = np.arange(5 * 3, dtype=np.uint16).reshape(3, 5) * 60
    p = GH.pad_hbd(y, 8, 8)
    assert p.shape == (8 + 144, 8 + 144) and np.array_equal(p[72:75, 72:77], y)
    assert (p[:72, :72] == y[0, 0]).all() and (p[75:, 77:] == y[2, 4]).all() and (p[73, 77:] == y[1, 4]).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_tffh_model_equals_fixture(gold, case):
    res, cover = MH.run_case(case)
    for name in ("plane", "err32", "weights"):
        assert np.array_equal(res[name], gold[case["id"] + "." + name]), name
    assert {k: v for k, v in cover.items() if v} == DOC["coverage_per_case"][case["id"]]


def test_tffh_model_equals_fixture_weights(gold):
    tuples = gold["weights.in"]
    assert np.array_equal(tuples, GH.weight_tuples())
    assert tuples[:, 6::4].max() == 256 * 1023 * 1023
    got = MH.model_weights(tuples)
    assert np.array_equal(got, gold["weights.out"])
    import tff_model as M
    assert got[:113, 0].tolist() == [(e * 1000) >> 16 for e in M.EXP_TAB]  # the first 113 tuples walk the exp table


def test_tffh_block_errors_are_scaled_as_the_reference_scales_them():
    """Landmarks of the high-bit-depth weights: an SSE below 16 is 0, and a block error is dropped by 4 bits
    when the block is split, by 6 when it is not (8 bit: 0 and 2)."""
    args = dict(mvx=0, mvy=0, decay=32 << 10, dist_th=64)
    assert MH.weight_hbd(15, 0, split=True, **args) == MH.weight_hbd(0, 0, split=True, **args) == 1000
    assert MH.weight_hbd(16 * 48, 0, split=True, **args) < 1000
    assert MH.weight_hbd(0, 15, split=True, **args) == 1000 and MH.weight_hbd(0, 16 * 48, split=True, **args) < 1000
    assert MH.weight_hbd(0, 64 * 48 - 1, split=False, **args) == MH.weight_hbd(0, 63 * 48, split=False, **args)
    assert MH.weight_hbd(0, 64 * 480, split=False, **args) < MH.weight_hbd(0, 63 * 48, split=False, **args)


@pytest.mark.skipif(not (ref_available() and GF.reference_headers()),
                    reason="oracle/_ref not built or the reference's headers absent (the offsetof probe needs them)")
def test_tffh_fixture_regenerates(gold):
    ar = GH.RefArithH()
    for name in ("own72_rand", "clip64_rand", "frac72_h0q2_wrap"):
        case = case_by_id(name)
        res = GH.run_case(case, ar, {k: 0 for k in GH.COUNTED_KEYS})
        for key, val in res.items():
            assert val.tobytes() == gold[name + "." + key].tobytes(), (name, key)
    tuples = gold["weights.in"]
    assert GH.reference_weights(tuples[::7]).tobytes() == np.ascontiguousarray(gold["weights.out"][::7]).tobytes()


# ----------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------
def upload_10(gpu, case, base=BASE, attach=True):
    """The 10-bit pictures of a case or window: the MSB pyramid (svtme_picture_upload_10bit) and, attached,
    the 16-bit plane. -> {picture: [h][w] u16}."""
    frames = GH.frames10(case)
    for t, f in frames.items():
        gpu.upload(base + t, f)
        if attach:
            gpu.attach_10bit(base + t, f)
    return frames


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


def run_filter(svtme, gpu, case, subpel, refs=None, controls=None, **kw):
    refs = case["refs"] if refs is None else refs
    ctl = svtme.TfFilterControls.from_dict(case["controls"] if controls is None else controls)
    return gpu.tf_filter_10bit(BASE + case["centre"], [BASE + r for r in refs], case["w"], case["h"], ctl, subpel, **kw)


def state_of(gpu, numbers, base=BASE):
    """Every resident plane of the pictures: three luma levels and, where attached, the 16-bit plane."""
    out = {}
    for t in numbers:
        out[t] = [gpu.download(base + t, lv) for lv in range(3)]
        try:
            out[t].append(gpu.download_10bit(base + t))
        except RuntimeError:
            pass
    return out


def assert_state(got, want, what):
    assert sorted(got) == sorted(want), what
    for t in want:
        assert len(got[t]) == len(want[t]), (what, t)
        for k, (a, b) in enumerate(zip(got[t], want[t])):
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (what, t, k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_tffh_vs_reference_golden(svtme, gpu, gold, case):
    name = case["id"]
    frames = upload_10(gpu, case)
    try:
        plane, err32 = run_filter(svtme, gpu, case, subpel_of(gold, case))
    finally:
        release(gpu, frames)
    assert np.array_equal(err32, gold[name + ".err32"]), name
    assert_planes_equal(plane, gold[name + ".plane"][:case["h"], :case["w"]], name)


SWEEP = [(64, 64, "frac", (7, 9), 41), (64, 64, "clip", (9,), 42), (72, 40, "noise", (7, 9, 6), 43),
         (72, 40, "clip", (7,), 44)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,kind,refs,seed", SWEEP, ids=[f"{w}x{h}_{k}_{s}" for w, h, k, _, s in SWEEP])
def test_tffh_random_sweep_vs_model(svtme, gpu, w, h, kind, refs, seed):
    """Seeded random sub-pel results (every branch, splits, MVs far beyond each edge) and seeded controls
    against the model."""
    rng = np.random.default_rng(seed)
    case = {"id": f"sweep{seed}", "kind": kind, "w": w, "h": h, "centre": 8, "refs": list(refs), "seed": seed,
            "controls": {"tf_decay_factor_fp16": int(rng.choice(GF.DECAYS + (1024, 500_000, 8_000_000, 0xFFFFFFFF))),
                         "tf_mv_dist_th": int(rng.choice(GF.DIST_THS + (1, 10, 100, 200))),
                         "sub_sampling_shift": int(rng.integers(0, 2))}}
    sub = GF.random_subpel(case)
    frames = upload_10(gpu, case)
    try:
        plane, err32 = run_filter(svtme, gpu, case, sub)
    finally:
        release(gpu, frames)
    pics = {t: GH.host_picture(f) for t, f in frames.items()}
    want, want_e32, _, _ = MH.filter_window(pics[8], [pics[r] for r in refs], case["controls"], sub)
    assert np.array_equal(err32, want_e32), case
    assert_planes_equal(plane, want[:h, :w], str(case))


@pytest.mark.gpu
def test_tffh_window_of_three_in_three_orders(svtme, gpu, gold):
    case = case_by_id("own128_rand")
    sub = gold[case["id"] + ".subpel"]
    frames = upload_10(gpu, case)
    try:
        for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
            plane, err32 = run_filter(svtme, gpu, case, sub[list(order)], refs=[case["refs"][k] for k in order])
            assert_planes_equal(plane, gold[case["id"] + ".plane"], f"order {order}")
            assert np.array_equal(err32, gold[case["id"] + ".err32"][list(order)])
    finally:
        release(gpu, frames)


@pytest.mark.gpu
def test_tffh_strides_null_err32_and_the_pictures_stay(svtme, gpu, gold):
    case = case_by_id("noise124_h0q2_wrap")  # 124 x 66: neither a multiple of 8
    name, w, h = case["id"], case["w"], case["h"]
    numbers = [case["centre"]] + case["refs"]
    sub = subpel_of(gold, case)
    # the input rows 124 + 5 samples apart
    frames = GH.frames10(case)
    try:
        for t, f in frames.items():
            gpu.upload(BASE + t, f)
            wide = np.full((h, w + 5), 0x3FF, np.uint16)
            wide[:, :w] = f
            assert gpu.lib.svtme_picture_attach_10bit(gpu.ctx, BASE + t, wide.ctypes.data, w + 5, w, h) == 0
        before = state_of(gpu, numbers)
        assert all(len(v) == 4 for v in before.values())
        plane, err32 = run_filter(svtme, gpu, case, sub)
        p1, e1 = run_filter(svtme, gpu, case, sub, with_err32=False)
        assert e1 is None
        assert_planes_equal(p1, plane, "NULL err32_out")
        p2, _ = run_filter(svtme, gpu, case, sub, out_stride=w + 13)
        assert_planes_equal(np.ascontiguousarray(p2), plane, "out_stride above the width")
        assert (p2.base[:, w:] == 0).all()  # the slack samples stay as they were
        assert_state(state_of(gpu, numbers), before, "no resident picture is modified")
    finally:
        release(gpu, frames)
    assert_planes_equal(plane, gold[name + ".plane"][:h, :w], name)
    assert np.array_equal(err32, gold[name + ".err32"])


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(121, 67), (124, 66)])
def test_tffh_attach_download_equals_numpy_repad(svtme, gpu, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    W, H = svtme.align8(w), svtme.align8(h)
    y, y2 = rng.integers(0, 1024, (h, w), dtype=np.uint16), rng.integers(0, 1024, (h, w), dtype=np.uint16)
    gpu.upload(BASE + 1, y)
    try:
        levels = [gpu.download(BASE + 1, lv) for lv in range(3)]
        gpu.attach_10bit(BASE + 1, y)
        got = gpu.download_10bit(BASE + 1)
        assert got.shape == (H + 144, W + 144)
        assert_planes_equal(got, GH.pad_hbd(y, W, H), f"{w}x{h}")
        assert np.array_equal(got >> 2, levels[0])  # consistent with the MSB plane's own padding
        gpu.attach_10bit(BASE + 1, y2)  # a second attach replaces the plane
        assert_planes_equal(gpu.download_10bit(BASE + 1), GH.pad_hbd(y2, W, H), "second attach")
        for lv in range(3):  # the luma planes are not touched
            assert np.array_equal(gpu.download(BASE + 1, lv), levels[lv])
    finally:
        release(gpu, [1])


@pytest.mark.gpu
def test_tffh_luma_reupload_drops_the_plane(svtme, gpu):
    case = case_by_id("own64_rand")
    frames = upload_10(gpu, case)
    lib, ctx = gpu.lib, gpu.ctx
    refs = [BASE + r for r in case["refs"]]
    r1 = case["refs"][1]
    try:
        assert _filter_call(svtme, lib, ctx, refs, w=64, h=64) == 0
        gpu.upload(BASE + r1, frames[r1])  # the same luma again
        with pytest.raises(RuntimeError, match="no 10-bit plane"):
            gpu.download_10bit(BASE + r1)
        assert _filter_call(svtme, lib, ctx, refs, w=64, h=64) == BAD_PARAMETER
        assert "no 10-bit plane" in lib.svtme_last_error().decode()
        with pytest.raises(RuntimeError, match="0x80001005"):
            gpu.tf_window_10bit([TW.tf_job(svtme, TW.own_window(64, 64, (7,), "l8"), BASE + 8, BASE + r1)], 64, 64,
                                *TW.controls_of(svtme, TW.own_window(64, 64, (7,), "l8")), BASE + OUT)
        gpu.attach_10bit(BASE + r1, frames[r1])
        assert _filter_call(svtme, lib, ctx, refs, w=64, h=64) == 0
        gpu.invalidate(BASE + case["centre"], (frames[case["centre"]] >> 2).astype(np.uint8))
        assert _filter_call(svtme, lib, ctx, refs, w=64, h=64) == BAD_PARAMETER
        # a plane for a picture of another size, or one that is not resident
        assert _attach_call(lib, ctx) == BAD_PARAMETER  # BASE + 8 is 64 x 64, not 121 x 67
        gpu.release(BASE + case["centre"])
        assert _attach_call(lib, ctx, w=64, h=64) == BAD_PARAMETER
    finally:
        release(gpu, list(frames) + [OUT])


def window_10(w, h, refs, kind="frac"):
    return TW.own_window(w, h, refs, "l8", kind)


def run_window_10(svtme, gpu, win, out_pn, centre_pn=None, refs_pn=None, want=None):
    centre_pn = BASE + win["centre"] if centre_pn is None else centre_pn
    refs_pn = [BASE + r for r in win["refs"]] if refs_pn is None else refs_pn
    jobs = [TW.tf_job(svtme, win, centre_pn, r) for r in refs_pn]
    sp, fc = TW.controls_of(svtme, win)
    kw = {} if want is None else {"want": want}
    return gpu.tf_window_10bit(jobs, win["w"], win["h"], sp, fc, out_pn, **kw)


def separate_calls(svtme, gpu, win, centre_pn=None, refs_pn=None) -> dict:
    """The window as the three calls through host memory, named as tf_window_10bit's result."""
    centre_pn = BASE + win["centre"] if centre_pn is None else centre_pn
    refs = [BASE + r for r in win["refs"]] if refs_pn is None else refs_pn
    sp, fc = TW.controls_of(svtme, win)
    layout = svtme.PackLayout(n_pus=85, max_cand=1, max_refs=1, full_records=1, sb_results=0)
    me = np.stack([np.frombuffer(gpu.submit_packed(TW.tf_job(svtme, win, centre_pn, r), layout), svtme.REF_RECORD_DTYPE)
                   for r in refs])
    sub = gpu.tf_subpel(centre_pn, refs, win["w"], win["h"], sp, me)
    p16, err32 = gpu.tf_filter_10bit(centre_pn, refs, win["w"], win["h"], fc, sub)
    return {"plane": (p16 >> 2).astype(np.uint8), "records": me, "subpel": sub, "err32": err32, "plane16": p16}


def assert_same_10(svtme, got, want, what):
    TW.assert_same(svtme, {k: v for k, v in got.items() if k != "plane16"},
                   {k: v for k, v in want.items() if k != "plane16"}, what)
    assert_planes_equal(got["plane16"], want["plane16"], what + " plane16")


WINDOWS = [(72, 40, (7,)), (121, 67, (7, 9)), (128, 128, (7, 9, 6))]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,refs", WINDOWS, ids=[f"{w}x{h}" for w, h, _ in WINDOWS])
def test_tffh_window_equals_the_separate_calls_fresh_and_in_place(svtme, gpu, w, h, refs):
    """svtme_tf_window_10bit against submit_packed -> tf_subpel -> tf_filter_10bit, array for array; the
    resident result (three levels of the MSB plane, the 16-bit plane with every margin) is what
    svtme_picture_upload_10bit and svtme_picture_attach_10bit of the filtered plane leave; in place it is
    the same as into a fresh number."""
    win = window_10(w, h, refs)
    what = f"{w}x{h}, references {refs}"
    numbers = [win["centre"]] + list(refs)
    upload_10(gpu, win)
    try:
        before = state_of(gpu, numbers)
        want = separate_calls(svtme, gpu, win)
        assert len(np.unique(want["plane16"] & 3)) == 4  # the result is 10-bit deep
        got = run_window_10(svtme, gpu, win, BASE + OUT)
        assert_same_10(svtme, got, want, what)
        assert_state(state_of(gpu, numbers), before, what + ": the window's pictures stay")
        fresh = state_of(gpu, [OUT])
        assert len(fresh[OUT]) == 4
        gpu.upload(BASE + OUT + 1, got["plane16"])
        gpu.attach_10bit(BASE + OUT + 1, got["plane16"])
        assert_state({OUT: state_of(gpu, [OUT + 1])[OUT + 1]}, fresh, what + ": the resident result")
        # in place: only some outputs asked for
        place = run_window_10(svtme, gpu, win, BASE + win["centre"], want=("plane16", "err32"))
        assert sorted(place) == ["err32", "plane16"]
        assert_planes_equal(place["plane16"], got["plane16"], what + " in place")
        after = state_of(gpu, numbers)
        assert_state({OUT: after[win["centre"]]}, fresh, what + ": in place")
        assert_state({t: after[t] for t in refs}, {t: before[t] for t in refs}, what + ": the references stay")
    finally:
        release(gpu, numbers + [OUT, OUT + 1])


@pytest.mark.gpu
def test_tffh_second_window_reads_the_filtered_picture(svtme, gpu):
    """The result of one window is a reference of the next with nothing waited for in between: the second
    window equals the one whose reference was uploaded and attached from the first's host copy."""
    w, h = 121, 67
    first, second = window_10(w, h, (7, 9)), window_10(w, h, (7,))
    frames = upload_10(gpu, first)
    try:
        res = run_window_10(svtme, gpu, first, BASE + OUT)
        gpu.upload(BASE + OUT + 1, res["plane16"])
        gpu.attach_10bit(BASE + OUT + 1, res["plane16"])
        want = run_window_10(svtme, gpu, second, BASE + OUT + 2, centre_pn=BASE + 9, refs_pn=[BASE + OUT + 1])
        run_window_10(svtme, gpu, first, BASE + OUT, want=())  # queued; returns at once
        got = run_window_10(svtme, gpu, second, BASE + OUT + 3, centre_pn=BASE + 9, refs_pn=[BASE + OUT])
        assert_same_10(svtme, got, want, "second window")
        assert_state({0: state_of(gpu, [OUT + 3])[OUT + 3]}, {0: state_of(gpu, [OUT + 2])[OUT + 2]}, "second result")
    finally:
        release(gpu, list(frames) + [OUT, OUT + 1, OUT + 2, OUT + 3])


@pytest.mark.gpu
def test_tffh_refused_calls_leave_every_picture(svtme, gpu):
    win = window_10(128, 128, (7, 9))
    numbers = [8, 7, 9]
    frames = upload_10(gpu, win)
    lib, ctx = gpu.lib, gpu.ctx
    try:
        gpu.upload(BASE + 6, frames[7])  # a picture without a 16-bit plane
        before = state_of(gpu, numbers + [6])
        _context_free_errors(svtme, lib, ctx)
        assert _filter_call(svtme, lib, ctx, [BASE + 7, BASE + 6]) == BAD_PARAMETER  # a reference without
        assert _filter_call(svtme, lib, ctx, [BASE + 7], centre=BASE + 6) == BAD_PARAMETER  # the centre without
        assert _filter_call(svtme, lib, ctx, [BASE + 999]) == BAD_PARAMETER  # not resident
        assert _filter_call(svtme, lib, ctx, [BASE + 7], w=64, h=64) == BAD_PARAMETER  # another size
        for refs_pn, out_pn in (([BASE + 7, BASE + 6], BASE + OUT), ([BASE + 7, BASE + 6], BASE + 8),
                                ([BASE + 7, BASE + 999], BASE + OUT), ([BASE + 7, BASE + 9], BASE + 9)):
            with pytest.raises(RuntimeError, match="0x80001005"):
                run_window_10(svtme, gpu, win, out_pn, refs_pn=refs_pn)
        with pytest.raises(RuntimeError):  # no result picture was made
            gpu.download(BASE + OUT, 0)
        assert_state(state_of(gpu, numbers + [6]), before, "refused calls")
        # and the valid forms succeed
        assert _filter_call(svtme, lib, ctx, [BASE + 7, BASE + 9]) == 0
        assert _filter_call(svtme, lib, ctx, [BASE + 7], stride=200, with_err32=False) == 0
    finally:
        release(gpu, numbers + [6, OUT])


@pytest.mark.gpu
def test_tffh_8bit_calls_do_not_see_the_plane(svtme, gpu):
    """svtme_tf_filter and svtme_tf_window on pictures with a 16-bit plane attached give byte for byte what
    they give without it, and svtme_tf_window's result carries none."""
    win = window_10(121, 67, (7, 9))
    numbers = [8, 7, 9]
    res = []
    try:
        for attach in (False, True):
            upload_10(gpu, win, attach=attach)
            refs = [BASE + r for r in win["refs"]]
            sp, fc = TW.controls_of(svtme, win)
            layout = svtme.PackLayout(n_pus=85, max_cand=1, max_refs=1, full_records=1, sb_results=0)
            me = np.stack([np.frombuffer(gpu.submit_packed(TW.tf_job(svtme, win, BASE + 8, r), layout),
                                         svtme.REF_RECORD_DTYPE) for r in refs])
            sub = gpu.tf_subpel(BASE + 8, refs, 121, 67, sp, me)
            plane, err32 = gpu.tf_filter(BASE + 8, refs, 121, 67, fc, sub)
            out = gpu.tf_window([TW.tf_job(svtme, win, BASE + 8, r) for r in refs], 121, 67, sp, fc, BASE + OUT)
            in_place = gpu.tf_window([TW.tf_job(svtme, win, BASE + 8, r) for r in refs], 121, 67, sp, fc, BASE + 8,
                                     want=("plane",))
            res.append((plane, err32, out, state_of(gpu, [OUT])[OUT], in_place["plane"], state_of(gpu, [8])[8]))
            release(gpu, numbers + [OUT])
    finally:
        release(gpu, numbers + [OUT])
    (p0, e0, o0, s0, i0, c0), (p1, e1, o1, s1, i1, c1) = res
    assert np.array_equal(p0, p1) and np.array_equal(e0, e1) and np.array_equal(i0, i1)
    TW.assert_same(svtme, o1, o0, "tf_window with a 16-bit plane attached")
    assert len(s0) == len(s1) == 3 and all(np.array_equal(a, b) for a, b in zip(s0, s1))
    assert len(c0) == len(c1) == 3  # in place svtme_tf_window drops the centre's 16-bit plane
    assert all(np.array_equal(a, b) for a, b in zip(c0, c1))
