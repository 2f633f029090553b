"""Temporal filtering of chroma: resident Cb / Cr planes (svtme_picture_upload_chroma,
svtme_picture_download_chroma) and the yuv calls (svtme_tf_filter_yuv,
svtme_tf_window_yuv), include/svtme.h.

Expected values are the fixtures tests/golden/tffc_cases.{json,npz}: the reference's
svt_inter_predictor on chroma planes and its filter functions with tf_chroma set, under
the glue restated in tests/golden/make_golden_tffc.py. Beside them stands a model of
the stage in numpy and Python integers (tests/tffc_model.py). CPU tests pin the ABI, the
argument checks that need no context, the fixtures and the model to the fixtures; GPU
tests compare the calls bit for bit with the fixtures, the model, each other and the
luma-only calls.
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
import make_golden_tfsp as G  # noqa: E402
import test_tf_window as TW  # noqa: E402  (its window helpers; its tests are collected from its own file)
import tff_model as M  # noqa: E402
import tffc_model as MC  # noqa: E402

DOC = json.load(open(os.path.join(GOLD, "tffc_cases.json")))
CASES = DOC["cases"]
BAD_PARAMETER = 0x80001005
BASE = 13000  # picture numbers of this file's uploads
OUT = 900     # + BASE: the result picture of a window into a fresh number
SYMBOLS = ("svtme_picture_upload_chroma", "svtme_picture_download_chroma", "svtme_tf_filter_yuv", "svtme_tf_window_yuv")


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLD, "tffc_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def case_by_id(name):
    return next(c for c in CASES if c["id"] == name)


# ----------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------
def test_tffc_symbols_exported(svtme):
    lib = svtme.load_product()
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []


_STRUCTS = {"svtme_tf_filter_yuv_controls": ("TfFilterYuvControls", 16), "svtme_tf_filter_yuv_out": ("TfFilterYuvOut", 48),
            "svtme_tf_window_yuv_out": ("TfWindowYuvOut", 24)}


def test_tffc_struct_sizes_and_offsets_equal_the_headers(svtme, tmp_path):
    lines = []
    for cname, (pyname, _) in _STRUCTS.items():
        lines.append(f'printf("sizeof {cname} %zu\\n", sizeof({cname}));')
        for field, _ in getattr(svtme, pyname)._fields_:
            lines.append(f'printf("{cname}.{field} %zu\\n", offsetof({cname}, {field}));')
    lines.append('printf("SVTME_PAD_CHROMA %d\\n", SVTME_PAD_CHROMA);')
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
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
    assert got["SVTME_PAD_CHROMA"] == svtme.PAD_CHROMA == 40
    assert [f for f, _ in svtme.TfFilterYuvControls._fields_][0] == "luma"  # the 8-byte luma controls first
    assert svtme.TfFilterYuvControls.tf_decay_factor_cb_fp16.offset == 8


def _controls(svtme, **over):
    return svtme.TfFilterYuvControls.from_dict(dict({"tf_decay_factor_fp16": 2_000_000, "tf_mv_dist_th": 64,
                                                     "sub_sampling_shift": 1, "tf_decay_factor_cb_fp16": 2_000_000,
                                                     "tf_decay_factor_cr_fp16": 2_000_000}, **over))


def _filter_call(svtme, lib, ctx, refs, n=None, ctl=None, null=None, w=128, h=128, centre=BASE + 8, strides=None,
                 branch=0, want=("cb", "cr")):
    """-> the status of svtme_tf_filter_yuv; on an error no output may be touched."""
    ctl = ctl if ctl is not None else _controls(svtme)
    sbs = svtme.sb_total(svtme.align8(w), svtme.align8(h))
    slots = max(len(refs), svtme.MAX_BATCH_JOBS + 1)
    arr = (C.c_uint64 * slots)(*refs)
    sub = np.zeros((slots, sbs), svtme.TF_SUBPEL_SB_DTYPE)
    sub["branch"][min(len(refs), slots) - 1, sbs - 1] = branch  # the last struct the call reads
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    sy, scb, scr = strides or (w, cw, cw)
    bufs = [np.full(h * max(sy, w), 0x5A, np.uint8), np.full(ch * max(scb, cw), 0x5A, np.uint8),
            np.full(ch * max(scr, cw), 0x5A, np.uint8)]
    e32 = np.full(slots * sbs * 4, 0x5A5A5A5A, np.uint32)
    out = svtme.TfFilterYuvOut(y=None if null == "y" else bufs[0].ctypes.data,
                               cb=bufs[1].ctypes.data if "cb" in want else None,
                               cr=bufs[2].ctypes.data if "cr" in want else None, y_stride=sy, cb_stride=scb,
                               cr_stride=scr, err32=e32.ctypes.data)
    st = lib.svtme_tf_filter_yuv(None if null == "ctx" else ctx, centre, None if null == "refs" else arr,
                                 len(refs) if n is None else n, w, h, None if null == "controls" else C.byref(ctl),
                                 None if null == "subpel" else sub.ctypes.data, None if null == "out" else C.byref(out))
    if st:
        assert all((b == 0x5A).all() for b in bufs) and (e32 == 0x5A5A5A5A).all()
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
    yield "cb_stride of an odd width", dict(refs=ok, w=121, h=67, strides=(121, 60, 61))
    yield "tf_mv_dist_th 32768", dict(refs=ok, ctl=_controls(svtme, tf_mv_dist_th=32768))
    yield "sub_sampling_shift 2", dict(refs=ok, ctl=_controls(svtme, sub_sampling_shift=2))
    yield "branch 3", dict(refs=ok, branch=3)


def _chroma_call(lib, ctx, null=None, w=121, h=67, stride=None):
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    cb, cr = np.zeros((max(ch, 1), max(cw, 1)), np.uint8), np.zeros((max(ch, 1), max(cw, 1)), np.uint8)
    st = lib.svtme_picture_upload_chroma(None if null == "ctx" else ctx, BASE + 8,
                                         None if null == "cb" else cb.ctypes.data,
                                         None if null == "cr" else cr.ctypes.data, cw if stride is None else stride, w, h)
    return st & 0xFFFFFFFF


def _window_call(svtme, lib, ctx, null=None, n=1, strides=(64, 64), w=128, h=128):
    win = TW.own_window(w, h, (7,), "l8")
    jobs = (svtme.Job * (svtme.MAX_BATCH_JOBS + 1))(TW.tf_job(svtme, win, BASE + 8, BASE + 7))
    sp, _ = TW.controls_of(svtme, win)
    fc = _controls(svtme)
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    cb, cr = np.full(ch * cw, 0x5A, np.uint8), np.full(ch * cw, 0x5A, np.uint8)
    uv = svtme.TfWindowYuvOut(cb=cb.ctypes.data, cr=cr.ctypes.data, cb_stride=strides[0], cr_stride=strides[1])
    st = lib.svtme_tf_window_yuv(None if null == "ctx" else ctx, None if null == "jobs" else jobs, n, w, h,
                                 None if null == "subpel_controls" else C.byref(sp),
                                 None if null == "filter_controls" else C.byref(fc), BASE + OUT, None, C.byref(uv))
    if st:
        assert (cb == 0x5A).all() and (cr == 0x5A).all()
    return st & 0xFFFFFFFF


def _context_free_errors(svtme, lib, ctx):
    for what, kw in _bad_filter_calls(svtme):
        assert _filter_call(svtme, lib, ctx, **kw) == BAD_PARAMETER, what
    for null in ("ctx", "cb", "cr"):
        assert _chroma_call(lib, ctx, null=null) == BAD_PARAMETER, null
    assert _chroma_call(lib, ctx, w=0) == BAD_PARAMETER
    assert _chroma_call(lib, ctx, h=0) == BAD_PARAMETER
    assert _chroma_call(lib, ctx, stride=60) == BAD_PARAMETER  # the chroma width of 121 is 61
    u32 = C.c_uint32()
    for ctx_, plane in ((None, 1), (ctx, 0), (ctx, 3)):
        assert lib.svtme_picture_download_chroma(ctx_, BASE + 8, plane, None, C.byref(u32), C.byref(u32), C.byref(u32),
                                                 C.byref(u32)) & 0xFFFFFFFF == BAD_PARAMETER
    for null in ("ctx", "jobs", "subpel_controls", "filter_controls"):
        assert _window_call(svtme, lib, ctx, null=null) == BAD_PARAMETER, null
    assert _window_call(svtme, lib, ctx, n=0) == BAD_PARAMETER
    assert _window_call(svtme, lib, ctx, n=svtme.MAX_BATCH_JOBS + 1) == BAD_PARAMETER
    assert _window_call(svtme, lib, ctx, strides=(63, 64)) == BAD_PARAMETER
    assert _window_call(svtme, lib, ctx, strides=(64, 63)) == BAD_PARAMETER


def test_tffc_bad_parameters_without_a_device(svtme):
    """The checks that need no context run before the context is touched: a block of zero bytes
    stands in for it."""
    lib = svtme.load_product()
    fake = C.create_string_buffer(64)
    _context_free_errors(svtme, lib, C.cast(fake, C.c_void_p))
    assert fake.raw == bytes(64)


def test_tffc_case_list_matches_generator():
    assert CASES == GC.case_dicts()
    assert [(c["w"], c["h"], len(c["refs"])) for c in CASES] == [(64, 64, 2), (72, 40, 1), (128, 128, 3), (8, 8, 1),
                                                                 (64, 64, 2)]
    assert CASES[-1]["kind"] == "same"
    ctl = [c["controls"] for c in CASES]
    for key in ("tf_decay_factor_cb_fp16", "tf_decay_factor_cr_fp16"):
        assert {c[key] for c in ctl} >= {1023, 2_000_000, 0x7FFFFFFF}
    assert {c[k] for c in ctl for k in ("tf_decay_factor_cb_fp16", "tf_decay_factor_cr_fp16")} == {0, 1023, 2_000_000,
                                                                                                0x7FFFFFFF}
    assert all(c["tf_decay_factor_cb_fp16"] != c["tf_decay_factor_cr_fp16"] for c in ctl)
    assert {c["sub_sampling_shift"] for c in ctl} == {0, 1}


def test_tffc_coverage_counts_are_all_non_zero():
    assert set(DOC["coverage"]) == set(GC.COVERAGE_KEYS)
    assert [k for k, v in DOC["coverage"].items() if not v > 0] == []
    assert set(DOC["coverage_per_case"]) == {c["id"] for c in CASES}
    for k in GC.COVERAGE_KEYS:
        assert sum(c.get(k, 0) for c in DOC["coverage_per_case"].values()) == DOC["coverage"][k], k


def test_tffc_fixture_shapes(svtme, gold):
    assert sorted(gold) == sorted(c["id"] + s for c in CASES for s in (".cb", ".cr", ".weights_uv", ".subpel"))
    for case in CASES:
        W, H = svtme.align8(case["w"]), svtme.align8(case["h"])
        n, sbs, name = len(case["refs"]), svtme.sb_total(W, H), case["id"]
        for p in (".cb", ".cr"):
            assert gold[name + p].shape == (H // 2, W // 2) and gold[name + p].dtype == np.uint8
        assert gold[name + ".weights_uv"].shape == (n, sbs, 2, 16) and gold[name + ".weights_uv"].max() <= 1000
        assert gold[name + ".subpel"].tobytes() == GF.random_subpel(case).tobytes()
    assert os.path.getsize(os.path.join(GOLD, "tffc_cases.npz")) < os.path.getsize(os.path.join(GOLD, "tff_cases.npz"))


def test_tffc_four_tap_table_and_clamp():
    """Landmarks: Subpel_Filters[4] is mirrored and has two zero taps each side; the chroma clamp is not
    half the luma clamp (a luma MV of 32767 wraps to -2 in q4 luma units and stays unclamped there)."""
    assert (MC.SPEC_FOUR[:, :2] == 0).all() and (MC.SPEC_FOUR[:, 6:] == 0).all()
    assert MC.SPEC_FOUR[8].tolist() == [0, 0, -12, 76, 76, -12, 0, 0] and MC.SPEC_FOUR[15].tolist() == [0, 0, -2, 8, 126, -4, 0, 0]
    assert G.clamp(32767, 0, 64, 64)[0] == -2
    assert GC.clamp_uv(32767, 0, 64, 64) == ((4 + 32) * 16 - 16, False, True)
    assert GC.clamp_uv(-32767, 32, 8, 64) == (-(32 * 8) - (4 + 4) * 16, True, False)


_inputs = {}


def host_inputs(svtme, case):
    """(pyramids on the CPU oracle's planes, padded chroma) of a case, built once per process."""
    if case["id"] not in _inputs:
        W, H = svtme.align8(case["w"]), svtme.align8(case["h"])
        pyr = {t: svtme.build_host_pyramid(f, "oracle") for t, f in G.case_frames(case).items()}
        uv = {t: tuple(GC.pad_chroma(p, W, H) for p in planes) for t, planes in GC.chroma_frames(case).items()}
        _inputs[case["id"]] = (pyr, uv)
    return _inputs[case["id"]]


def model_window(svtme, case, controls, subpel, refs=None):
    refs = case["refs"] if refs is None else refs
    pyr, uv = host_inputs(svtme, case)
    return MC.filter_window_yuv(pyr[case["centre"]], [pyr[r] for r in refs], uv[case["centre"]], [uv[r] for r in refs],
                                controls, subpel)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_tffc_model_equals_fixture(svtme, gold, case):
    res, cover = model_window(svtme, case, case["controls"], gold[case["id"] + ".subpel"])
    for name in ("cb", "cr", "weights_uv"):
        assert np.array_equal(res[name], gold[case["id"] + "." + name]), name
    assert {k: v for k, v in cover.items() if v} == DOC["coverage_per_case"][case["id"]]
    # and the luma beside it is the luma-only model's
    pyr, _ = host_inputs(svtme, case)
    plane, err32, weights, _ = M.filter_window(pyr[case["centre"]], [pyr[r] for r in case["refs"]],
                                               GC.luma_controls(case["controls"]), gold[case["id"] + ".subpel"])
    assert np.array_equal(plane, res["y"]) and np.array_equal(err32, res["err32"])
    assert np.array_equal(weights, res["weights"])


@pytest.mark.skipif(not (ref_available() and GF.reference_headers()),
                    reason="oracle/_ref not built or the reference's headers absent (the offsetof probe needs them)")
def test_tffc_fixture_regenerates(gold):
    for name in ("c72_rand", "c8_rand"):
        case = case_by_id(name)
        res = GC.run_case(case, GC.RefArithUV(), {k: 0 for k in GC.COVERAGE_KEYS})
        for key in ("cb", "cr", "weights_uv", "subpel"):
            assert res[key].tobytes() == gold[name + "." + key].tobytes(), (name, key)


# ----------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------
def upload_yuv(gpu, case, base=BASE, chroma=True):
    frames, uv = G.case_frames(case), GC.chroma_frames(case)
    for t, f in frames.items():
        gpu.upload(base + t, f)
        if chroma:
            gpu.upload_chroma(base + t, uv[t][0], uv[t][1], case["w"], case["h"])
    return frames


def release(gpu, numbers, base=BASE):
    for t in numbers:
        try:
            gpu.release(base + t)
        except RuntimeError:  # not resident: the test failed before it made the picture
            pass


def assert_planes_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        y, x = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}: {int((got != want).sum())} pixels differ, first at x {x} y {y}: "
                             f"{got[y, x]} for {want[y, x]}")


def run_filter_yuv(svtme, gpu, case, subpel, refs=None, controls=None, **kw):
    refs = case["refs"] if refs is None else refs
    ctl = svtme.TfFilterYuvControls.from_dict(case["controls"] if controls is None else controls)
    return gpu.tf_filter_yuv(BASE + case["centre"], [BASE + r for r in refs], case["w"], case["h"], ctl, subpel, **kw)


def state_of(gpu, numbers, base=BASE):
    """Every resident plane of the pictures: three luma levels and, where attached, Cb and Cr."""
    out = {}
    for t in numbers:
        out[t] = [gpu.download(base + t, lv) for lv in range(3)]
        try:
            out[t] += [gpu.download_chroma(base + t, p) for p in (1, 2)]
        except RuntimeError:
            pass
    return out


def assert_state(got, want, what):
    assert sorted(got) == sorted(want), what
    for t in want:
        assert len(got[t]) == len(want[t]), (what, t)
        for k, (a, b) in enumerate(zip(got[t], want[t])):
            assert a.shape == b.shape and np.array_equal(a, b), (what, t, k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_tffc_vs_reference_golden(svtme, gpu, gold, case):
    """Cb and Cr bit-exact against the reference's; luma and err32 byte for byte svtme_tf_filter's."""
    name = case["id"]
    frames = upload_yuv(gpu, case)
    try:
        y, cb, cr, err32 = run_filter_yuv(svtme, gpu, case, gold[name + ".subpel"])
        y0, err0 = gpu.tf_filter(BASE + case["centre"], [BASE + r for r in case["refs"]], case["w"], case["h"],
                                 svtme.TfFilterControls.from_dict(GC.luma_controls(case["controls"])),
                                 gold[name + ".subpel"])
    finally:
        release(gpu, frames)
    assert_planes_equal(cb, gold[name + ".cb"], name + " cb")
    assert_planes_equal(cr, gold[name + ".cr"], name + " cr")
    assert_planes_equal(y, y0, name + " y")
    assert np.array_equal(err32, err0)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", MC.SWEEP_SEEDS, ids=[f"seed{s}" for s in MC.SWEEP_SEEDS])
def test_tffc_random_sweep_vs_model(svtme, gpu, seed):
    """Random shapes (8x8 to 200x72, odd sizes among them), contents, windows of 1 to 16 and controls:
    the GPU's own TF-ME jobs and sub-pel refinement feed svtme_tf_filter_yuv, as they are and
    perturbed; all three planes and err32 against the model."""
    case = MC.sweep_case(seed)
    what = f"seed {seed}: {case['w']}x{case['h']} {case['kind']}, references {case['refs']}, filter {case['filter']}"
    refs = [BASE + r for r in case["refs"]]
    frames = upload_yuv(gpu, case)
    try:
        layout = svtme.PackLayout(n_pus=85, max_cand=1, max_refs=1, full_records=1, sb_results=0)
        me = np.stack([np.frombuffer(gpu.submit_packed(G.me_job(case, case["controls"], r, BASE), layout),
                                     svtme.REF_RECORD_DTYPE) for r in case["refs"]])
        sub = gpu.tf_subpel(BASE + case["centre"], refs, case["w"], case["h"],
                            svtme.TfSubpelControls.from_dict(case["subpel"]), me)
        inputs = [("chain", sub), ("perturbed", M.perturb_subpel(sub, 7000 + seed))]
        got = [run_filter_yuv(svtme, gpu, case, s, controls=case["filter"]) for _, s in inputs]
    finally:
        release(gpu, frames)
    w, h = case["w"], case["h"]
    for (label, s), (y, cb, cr, err32) in zip(inputs, got):
        want, _ = model_window(svtme, dict(case, id=f"sweep{seed}"), case["filter"], s)
        assert np.array_equal(err32, want["err32"]), (what, label)
        assert_planes_equal(y, want["y"][:h, :w], f"{what} ({label}) y")
        assert_planes_equal(cb, want["cb"][:(h + 1) >> 1, :(w + 1) >> 1], f"{what} ({label}) cb")
        assert_planes_equal(cr, want["cr"][:(h + 1) >> 1, :(w + 1) >> 1], f"{what} ({label}) cr")


@pytest.mark.gpu
def test_tffc_window_of_three_in_three_orders(svtme, gpu, gold):
    case = case_by_id("c128_rand")
    sub = gold[case["id"] + ".subpel"]
    w = gold[case["id"] + ".weights_uv"]
    assert len(np.unique(w[:, :, 0])) > 4  # the weights matter here
    frames = upload_yuv(gpu, case)
    try:
        for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
            _, cb, cr, _ = run_filter_yuv(svtme, gpu, case, sub[list(order)], refs=[case["refs"][k] for k in order])
            assert_planes_equal(cb, gold[case["id"] + ".cb"], f"order {order} cb")
            assert_planes_equal(cr, gold[case["id"] + ".cr"], f"order {order} cr")
    finally:
        release(gpu, frames)


@pytest.mark.gpu
def test_tffc_strides_null_outputs_and_the_pictures_stay(svtme, gpu, gold):
    case = case_by_id("c72_rand")  # 72 x 40: the second SB column holds 4 chroma samples
    name, w, h = case["id"], case["w"], case["h"]
    cw, ch = w // 2, h // 2
    numbers = [case["centre"]] + case["refs"]
    frames = upload_yuv(gpu, case)
    try:
        before = state_of(gpu, numbers)
        y, cb, cr, err32 = run_filter_yuv(svtme, gpu, case, gold[name + ".subpel"])
        y1, cb1, cr1, e1 = run_filter_yuv(svtme, gpu, case, gold[name + ".subpel"], want=(), with_err32=False)
        assert cb1 is None and cr1 is None and e1 is None
        assert_planes_equal(y1, y, "NULL chroma outputs")
        _, cb2, cr2, _ = run_filter_yuv(svtme, gpu, case, gold[name + ".subpel"], want=("cr",))
        assert cb2 is None
        assert_planes_equal(cr2, gold[name + ".cr"], "cr alone")
        # strides above the widths: the slack bytes stay as they were
        sy, scb, scr = w + 13, cw + 5, cw + 9
        bufs = [np.full((h, sy), 0xA5, np.uint8), np.full((ch, scb), 0xA5, np.uint8), np.full((ch, scr), 0xA5, np.uint8)]
        arr = (C.c_uint64 * len(case["refs"]))(*[BASE + r for r in case["refs"]])
        sub = np.ascontiguousarray(gold[name + ".subpel"])
        ctl = svtme.TfFilterYuvControls.from_dict(case["controls"])
        out = svtme.TfFilterYuvOut(y=bufs[0].ctypes.data, cb=bufs[1].ctypes.data, cr=bufs[2].ctypes.data, y_stride=sy,
                                   cb_stride=scb, cr_stride=scr, err32=None)
        assert gpu.lib.svtme_tf_filter_yuv(gpu.ctx, BASE + case["centre"], arr, len(case["refs"]), w, h, C.byref(ctl),
                                           sub.ctypes.data, C.byref(out)) == 0
        for buf, want, width in ((bufs[0], y, w), (bufs[1], gold[name + ".cb"], cw), (bufs[2], gold[name + ".cr"], cw)):
            assert_planes_equal(buf[:, :width], want, "strides above the widths")
            assert (buf[:, width:] == 0xA5).all()
        assert_state(state_of(gpu, numbers), before, "no resident picture is modified")
    finally:
        release(gpu, frames)
    assert_planes_equal(cb, gold[name + ".cb"], name)
    assert_planes_equal(cr, gold[name + ".cr"], name)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(121, 67), (124, 66)])
def test_tffc_upload_download_equals_numpy_repad(svtme, gpu, w, h):
    """The true (w + 1) / 2 x (h + 1) / 2 planes, replicated to W/2 x H/2 and by 40 more on every side."""
    rng = np.random.default_rng(w * 1000 + h)
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    W, H = svtme.align8(w), svtme.align8(h)
    cb, cr = rng.integers(0, 256, (ch, cw), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8)
    luma = rng.integers(0, 256, (h, w), dtype=np.uint8)
    gpu.upload(BASE + 1, luma)
    try:
        levels = [gpu.download(BASE + 1, lv) for lv in range(3)]
        gpu.upload_chroma(BASE + 1, cb, cr, w, h)
        got = [gpu.download_chroma(BASE + 1, p) for p in (1, 2)]
        for g, plane in zip(got, (cb, cr)):
            assert g.shape == (H // 2 + 80, W // 2 + 80)
            assert_planes_equal(g, GC.pad_chroma(plane, W, H), f"{w}x{h}")
        # a second upload replaces the planes; a stride above the width
        wide = np.full((ch, cw + 7), 0x11, np.uint8)
        wide[:, :cw] = cr
        assert gpu.lib.svtme_picture_upload_chroma(gpu.ctx, BASE + 1, wide.ctypes.data, wide.ctypes.data, cw + 7, w, h) == 0
        assert_planes_equal(gpu.download_chroma(BASE + 1, 1), GC.pad_chroma(cr, W, H), "second upload")
        for lv in range(3):  # the luma planes are not touched
            assert np.array_equal(gpu.download(BASE + 1, lv), levels[lv])
    finally:
        release(gpu, [1])


@pytest.mark.gpu
def test_tffc_luma_reupload_drops_the_chroma(svtme, gpu):
    case = case_by_id("c64_rand")
    frames = upload_yuv(gpu, case)
    lib, ctx = gpu.lib, gpu.ctx
    refs = [BASE + r for r in case["refs"]]
    try:
        assert _filter_call(svtme, lib, ctx, refs, w=64, h=64) == 0
        gpu.upload(BASE + case["refs"][1], frames[case["refs"][1]])  # the same luma again
        with pytest.raises(RuntimeError, match="no chroma"):
            gpu.download_chroma(BASE + case["refs"][1], 1)
        assert _filter_call(svtme, lib, ctx, refs, w=64, h=64) == BAD_PARAMETER
        assert "no chroma" in lib.svtme_last_error().decode()
        uv = GC.chroma_frames(case)[case["refs"][1]]
        gpu.upload_chroma(BASE + case["refs"][1], uv[0], uv[1], 64, 64)
        assert _filter_call(svtme, lib, ctx, refs, w=64, h=64) == 0
        gpu.invalidate(BASE + case["centre"], frames[case["centre"]])
        assert _filter_call(svtme, lib, ctx, refs, w=64, h=64) == BAD_PARAMETER
        # chroma for a picture that is not resident, or of another size
        assert _chroma_call(lib, ctx) == BAD_PARAMETER  # BASE + 8 is 64 x 64, not 121 x 67
        gpu.release(BASE + case["centre"])
        assert _chroma_call(lib, ctx, w=64, h=64) == BAD_PARAMETER
    finally:
        release(gpu, frames)


def yuv_window(w, h, refs, kind="frac"):
    win = TW.own_window(w, h, refs, "l8", kind)
    win["filter"] = dict(win["filter"], tf_decay_factor_cb_fp16=3_000_000, tf_decay_factor_cr_fp16=1_000_000)
    return win


def run_window_yuv(svtme, gpu, win, out_pn, centre_pn=None, refs_pn=None, want=None):
    centre_pn = BASE + win["centre"] if centre_pn is None else centre_pn
    refs_pn = [BASE + r for r in win["refs"]] if refs_pn is None else refs_pn
    jobs = [TW.tf_job(svtme, win, centre_pn, r) for r in refs_pn]
    sp = svtme.TfSubpelControls.from_dict(win["subpel"])
    fc = svtme.TfFilterYuvControls.from_dict(win["filter"])
    kw = {} if want is None else {"want": want}
    return gpu.tf_window_yuv(jobs, win["w"], win["h"], sp, fc, out_pn, **kw)


def separate_calls(svtme, gpu, win, centre_pn=None, refs_pn=None) -> dict:
    """The window as the three calls through host memory, named as tf_window_yuv's result."""
    centre_pn = BASE + win["centre"] if centre_pn is None else centre_pn
    refs = [BASE + r for r in win["refs"]] if refs_pn is None else refs_pn
    layout = svtme.PackLayout(n_pus=85, max_cand=1, max_refs=1, full_records=1, sb_results=0)
    me = np.stack([np.frombuffer(gpu.submit_packed(TW.tf_job(svtme, win, centre_pn, r), layout), svtme.REF_RECORD_DTYPE)
                   for r in refs])
    sub = gpu.tf_subpel(centre_pn, refs, win["w"], win["h"], svtme.TfSubpelControls.from_dict(win["subpel"]), me)
    y, cb, cr, err32 = gpu.tf_filter_yuv(centre_pn, refs, win["w"], win["h"],
                                         svtme.TfFilterYuvControls.from_dict(win["filter"]), sub)
    return {"plane": y, "records": me, "subpel": sub, "err32": err32, "cb": cb, "cr": cr}


def assert_same_yuv(svtme, got, want, what):
    TW.assert_same(svtme, {k: v for k, v in got.items() if k not in ("cb", "cr")},
                   {k: v for k, v in want.items() if k not in ("cb", "cr")}, what)
    assert_planes_equal(got["cb"], want["cb"], what + " cb")
    assert_planes_equal(got["cr"], want["cr"], what + " cr")


WINDOWS = [(72, 40, (7,)), (121, 67, (7, 9)), (128, 128, (7, 9, 6))]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,refs", WINDOWS, ids=[f"{w}x{h}" for w, h, _ in WINDOWS])
def test_tffc_window_equals_the_separate_calls_fresh_and_in_place(svtme, gpu, w, h, refs):
    """svtme_tf_window_yuv against submit_packed -> tf_subpel -> tf_filter_yuv, array for array; the
    resident result (three luma levels, Cb, Cr with every margin) is what uploads of the returned
    planes leave; in place it is the same as into a fresh number, and the luma side is
    svtme_tf_window's."""
    win = yuv_window(w, h, refs)
    what = f"{w}x{h}, references {refs}"
    numbers = [win["centre"]] + list(refs)
    frames = upload_yuv(gpu, win)
    try:
        before = state_of(gpu, numbers)
        want = separate_calls(svtme, gpu, win)
        got = run_window_yuv(svtme, gpu, win, BASE + OUT)
        assert_same_yuv(svtme, got, want, what)
        assert_state(state_of(gpu, numbers), before, what + ": the window's pictures stay")
        fresh = state_of(gpu, [OUT])
        assert len(fresh[OUT]) == 5
        # the resident result against uploads of the returned planes
        gpu.upload(BASE + OUT + 1, got["plane"])
        gpu.upload_chroma(BASE + OUT + 1, got["cb"], got["cr"], w, h)
        assert_state({OUT: state_of(gpu, [OUT + 1])[OUT + 1]}, fresh, what + ": the resident result")
        # the luma-only window gives the same luma side and leaves no chroma
        luma = gpu.tf_window([TW.tf_job(svtme, win, BASE + win["centre"], BASE + r) for r in refs], w, h,
                             svtme.TfSubpelControls.from_dict(win["subpel"]),
                             svtme.TfFilterControls.from_dict(GC.luma_controls(win["filter"])), BASE + OUT + 2)
        TW.assert_same(svtme, luma, {k: v for k, v in got.items() if k not in ("cb", "cr")}, what + ": luma-only")
        assert len(state_of(gpu, [OUT + 2])[OUT + 2]) == 3
        # in place: only some outputs asked for
        place = run_window_yuv(svtme, gpu, win, BASE + win["centre"], want=("plane", "cb"))
        assert sorted(place) == ["cb", "plane"]
        assert_planes_equal(place["plane"], got["plane"], what + " in place")
        assert_planes_equal(place["cb"], got["cb"], what + " in place cb")
        after = state_of(gpu, numbers)
        assert_state({OUT: after[win["centre"]]}, fresh, what + ": in place")
        assert_state({t: after[t] for t in refs}, {t: before[t] for t in refs}, what + ": the references stay")
    finally:
        release(gpu, numbers + [OUT, OUT + 1, OUT + 2])


@pytest.mark.gpu
def test_tffc_second_window_reads_the_filtered_picture(svtme, gpu):
    """The result of one window is a reference of the next, with nothing waited for in between: the
    second window equals the one whose reference was uploaded from the first's host copies."""
    w, h = 121, 67
    first, second = yuv_window(w, h, (7, 9)), yuv_window(w, h, (7,))
    frames = upload_yuv(gpu, first)
    try:
        res = run_window_yuv(svtme, gpu, first, BASE + OUT)
        gpu.upload(BASE + OUT + 1, res["plane"])
        gpu.upload_chroma(BASE + OUT + 1, res["cb"], res["cr"], w, h)
        want = run_window_yuv(svtme, gpu, second, BASE + OUT + 2, centre_pn=BASE + 9, refs_pn=[BASE + OUT + 1])
        # again, queued behind a first window that returns at once
        run_window_yuv(svtme, gpu, first, BASE + OUT, want=())
        got = run_window_yuv(svtme, gpu, second, BASE + OUT + 3, centre_pn=BASE + 9, refs_pn=[BASE + OUT])
        assert_same_yuv(svtme, got, want, "second window")
        assert_state({0: state_of(gpu, [OUT + 3])[OUT + 3]}, {0: state_of(gpu, [OUT + 2])[OUT + 2]}, "second result")
    finally:
        release(gpu, list(frames) + [OUT, OUT + 1, OUT + 2, OUT + 3])


@pytest.mark.gpu
def test_tffc_refused_calls_leave_every_picture(svtme, gpu):
    win = yuv_window(128, 128, (7, 9))
    numbers = [8, 7, 9]
    frames = upload_yuv(gpu, win)
    lib, ctx = gpu.lib, gpu.ctx
    try:
        gpu.upload(BASE + 6, frames[7])  # a picture without chroma
        before = state_of(gpu, numbers + [6])
        _context_free_errors(svtme, lib, ctx)
        assert _filter_call(svtme, lib, ctx, [BASE + 7, BASE + 6]) == BAD_PARAMETER  # a reference without chroma
        assert _filter_call(svtme, lib, ctx, [BASE + 7], centre=BASE + 6) == BAD_PARAMETER  # the centre without
        assert _filter_call(svtme, lib, ctx, [BASE + 999]) == BAD_PARAMETER  # not resident
        assert _filter_call(svtme, lib, ctx, [BASE + 7], w=64, h=64) == BAD_PARAMETER  # another size
        for refs_pn, out_pn in (([BASE + 7, BASE + 6], BASE + OUT), ([BASE + 7, BASE + 6], BASE + 8),
                                ([BASE + 7, BASE + 999], BASE + OUT), ([BASE + 7, BASE + 9], BASE + 9)):
            with pytest.raises(RuntimeError, match="0x80001005"):
                run_window_yuv(svtme, gpu, win, out_pn, refs_pn=refs_pn)
        with pytest.raises(RuntimeError):  # no result picture was made
            gpu.download(BASE + OUT, 0)
        assert_state(state_of(gpu, numbers + [6]), before, "refused calls")
        # and the valid forms succeed
        assert _filter_call(svtme, lib, ctx, [BASE + 7, BASE + 9]) == 0
        assert _filter_call(svtme, lib, ctx, [BASE + 7], strides=(200, 70, 64), want=("cb",)) == 0
        assert _filter_call(svtme, lib, ctx, [BASE + 7], strides=(128, 1, 1), want=()) == 0  # strides of NULL planes
    finally:
        release(gpu, numbers + [6, OUT])


@pytest.mark.gpu
def test_tffc_luma_calls_do_not_see_the_chroma(svtme, gpu):
    """svtme_tf_filter and svtme_tf_window on pictures with chroma attached give what they give
    without."""
    win = TW.own_window(121, 67, (7, 9), "l8")
    numbers = [8, 7, 9]
    res = []
    try:
        for chroma in (False, True):
            upload_yuv(gpu, win, chroma=chroma)
            refs = [BASE + r for r in win["refs"]]
            sp, fc = TW.controls_of(svtme, win)
            plane, err32 = gpu.tf_filter(BASE + 8, refs, 121, 67, fc, _subpel_of(svtme, gpu, win))
            out = gpu.tf_window([TW.tf_job(svtme, win, BASE + 8, r) for r in refs], 121, 67, sp, fc, BASE + OUT)
            res.append((plane, err32, out, state_of(gpu, [OUT])[OUT]))
            release(gpu, numbers + [OUT])
    finally:
        release(gpu, numbers + [OUT])
    (p0, e0, o0, s0), (p1, e1, o1, s1) = res
    assert np.array_equal(p0, p1) and np.array_equal(e0, e1)
    TW.assert_same(svtme, o1, o0, "tf_window with chroma attached")
    assert len(s0) == len(s1) == 3 and all(np.array_equal(a, b) for a, b in zip(s0, s1))


def _subpel_of(svtme, gpu, win):
    refs = [BASE + r for r in win["refs"]]
    layout = svtme.PackLayout(n_pus=85, max_cand=1, max_refs=1, full_records=1, sb_results=0)
    me = np.stack([np.frombuffer(gpu.submit_packed(TW.tf_job(svtme, win, BASE + 8, r), layout), svtme.REF_RECORD_DTYPE)
                   for r in refs])
    return gpu.tf_subpel(BASE + 8, refs, win["w"], win["h"], svtme.TfSubpelControls.from_dict(win["subpel"]), me)
