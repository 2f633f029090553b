"""One temporal-filtering window in one resident-to-resident call (svtme_tf_window, include/svtme.h).

Expected values are what the project already pins to the reference: the fixtures
tests/golden/tfsp_cases.npz (the reference's TF-ME records and sub-pel results) and
tff_cases.npz (its filtered planes and 32x32 errors), the oracle's pyramid builder for
the resident result, and the three calls the window chains (the TF-ME jobs,
svtme_tf_subpel, svtme_tf_filter), each of which has its own tests against the
reference. CPU tests pin the ABI and the argument checks that need no context; GPU tests
compare the window bit for bit with all of the above.

Records are compared with svtme.compare_records, as every other test of the GPU's ME
records is: the fields the reference defines (best_sad of a reference that was not
searched is not among them). Everything else is compared byte for byte.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
for p in (GOLD, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_golden_tfsp as G  # noqa: E402
import tff_model as M  # noqa: E402

TFF_CASES = {c["id"]: c for c in json.load(open(os.path.join(GOLD, "tff_cases.json")))["cases"]}
ME_CASES = [c for c in G.case_dicts() if c["records"] == "me"]
BAD_PARAMETER = 0x80001005
BASE = 12000  # picture numbers of this file's uploads
OUT = 900     # + BASE: the result picture of a window into a fresh number
LEVELS = ("full", "quarter", "sixteenth")


@pytest.fixture(scope="module")
def gold():
    out = {}
    with np.load(os.path.join(GOLD, "tfsp_cases.npz")) as z:
        for case in ME_CASES:
            out[case["id"] + ".rec"], out[case["id"] + ".out"] = z[case["id"] + ".rec"], z[case["id"] + ".out"]
    with np.load(os.path.join(GOLD, "tff_cases.npz")) as z:
        for case in ME_CASES:
            out[case["id"] + ".plane"], out[case["id"] + ".err32"] = z[case["id"] + ".plane"], z[case["id"] + ".err32"]
    return out


def window_of(case: dict, filt: dict = None) -> dict:
    """A window from a case dict of the fixtures (controls: the name of a control set; the filter
    controls are the same case's in tff_cases.json) or of the sweeps (controls, subpel, filter:
    dicts)."""
    named = isinstance(case["controls"], str)
    cs = G.CONTROL_SETS[case["controls"]] if named else case["controls"]
    return {"id": case["id"], "w": case["w"], "h": case["h"], "kind": case["kind"], "centre": case["centre"],
            "refs": list(case["refs"]), "me": {k: cs[k] for k in ("hme_me_level", "me_exit_th")},
            "subpel": {f: cs[f] for f in G.SUBPEL_FIELDS},
            "filter": filt if filt is not None else TFF_CASES[case["id"]]["controls"] if named else case["filter"]}


def own_window(w: int, h: int, refs, set_name: str, kind: str = "frac") -> dict:
    return window_of({"id": f"{kind}{w}x{h}_{set_name}", "w": w, "h": h, "kind": kind, "centre": 8, "refs": list(refs),
                      "controls": set_name},
                     {"tf_decay_factor_fp16": 2_000_000, "tf_mv_dist_th": 64,
                      "sub_sampling_shift": G.CONTROL_SETS[set_name]["sub_sampling_shift"]})


def tf_job(svtme, win: dict, centre_pn: int, ref_pn: int):
    """The TF-ME job of one reference (make_golden_tfsp.me_job with the picture numbers given)."""
    w, h = win["w"], win["h"]
    ctrl = svtme.derive_controls_tf(win["me"]["hme_me_level"], 0, 35, svtme.input_resolution_of(w, h))
    return svtme.case_job(ctrl, w, h, centre_pn, (ref_pn,), (), 0, me_type=svtme.ME_MCTF,
                          tf_me_exit_th=win["me"]["me_exit_th"])


def controls_of(svtme, win: dict):
    return svtme.TfSubpelControls.from_dict(win["subpel"]), svtme.TfFilterControls.from_dict(win["filter"])


# ----------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------
def test_tfw_symbol_exported(svtme):
    assert hasattr(svtme.load_product(), "svtme_tf_window")


_ABI_PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "svtme.h"
#define O(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
    printf("sizeof svtme_tf_window_out %zu\n", sizeof(svtme_tf_window_out));
    O(svtme_tf_window_out, plane); O(svtme_tf_window_out, plane_stride); O(svtme_tf_window_out, pad);
    O(svtme_tf_window_out, records); O(svtme_tf_window_out, subpel); O(svtme_tf_window_out, err32);
    return 0;
}
"""


def test_tfw_struct_sizes_and_offsets_equal_the_headers(svtme, tmp_path):
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text(_ABI_PROGRAM)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        key, val = line.rsplit(" ", 1)
        got[key] = int(val)
    out = svtme.TfWindowOut
    assert got["sizeof svtme_tf_window_out"] == C.sizeof(out) == 40
    for name, _ in out._fields_:
        assert got["svtme_tf_window_out." + name] == getattr(out, name).offset, name
    assert len(out._fields_) == 6


def _call(svtme, lib, ctx, refs=(7,), n=None, null=None, w=128, h=128, src=None, centre=8, out_pn=OUT, stride=None,
          sp=None, fc=None, edit=None, want_plane=True):
    """-> the status of svtme_tf_window for a window of `refs` around `centre` (picture numbers
    + BASE); edit(jobs) changes the job array first. On an error no output may be touched."""
    win = own_window(w, h, refs, "l8")
    slots = max(len(refs), svtme.MAX_BATCH_JOBS + 1)
    jobs = (svtme.Job * slots)(*[tf_job(svtme, win, BASE + centre, BASE + r) for r in refs])
    if edit:
        edit(jobs)
    sw, sh = (w, h) if src is None else src
    sbs = svtme.sb_total(svtme.align8(w), svtme.align8(h))
    stride = sw if stride is None else stride
    plane = np.full(max(sh, 1) * max(stride, sw, 1), 0x5A, np.uint8)
    recs = np.full(slots * sbs * svtme.REF_RECORD_DTYPE.itemsize, 0x5A, np.uint8)
    sub = np.full(slots * sbs * svtme.TF_SUBPEL_SB_DTYPE.itemsize, 0x5A, np.uint8)
    e32 = np.full(slots * sbs * 4, 0x5A5A5A5A, np.uint32)
    out = svtme.TfWindowOut(plane=plane.ctypes.data if want_plane else None, plane_stride=stride,
                            records=recs.ctypes.data, subpel=sub.ctypes.data, err32=e32.ctypes.data)
    dsp, dfc = controls_of(svtme, win)
    sp, fc = sp if sp is not None else dsp, fc if fc is not None else dfc
    st = lib.svtme_tf_window(None if null == "ctx" else ctx, None if null == "jobs" else jobs,
                             len(refs) if n is None else n, sw, sh, None if null == "subpel_controls" else C.byref(sp),
                             None if null == "filter_controls" else C.byref(fc), BASE + out_pn,
                             None if null == "out" else C.byref(out))
    if st:
        assert (plane == 0x5A).all() and (recs == 0x5A).all() and (sub == 0x5A).all() and (e32 == 0x5A5A5A5A).all()
        assert lib.svtme_last_error().decode() != ""
    return st & 0xFFFFFFFF


def _set(k, **fields):
    def edit(jobs):
        for name, v in fields.items():
            if name == "num_refs0":
                jobs[k].num_refs[0] = v
            else:
                setattr(jobs[k], name, v)
    return edit


def _bad_calls(svtme):
    """(what, keyword arguments of _call) of the argument errors that need no resident picture."""
    for null in ("ctx", "jobs", "subpel_controls", "filter_controls"):
        yield "null " + null, dict(null=null)
    yield "n 0", dict(n=0)
    yield "n 17", dict(refs=(7,) * (svtme.MAX_BATCH_JOBS + 1))
    yield "an open-loop job", dict(edit=_set(0, me_type=svtme.ME_OPEN_LOOP))
    yield "the second job is open-loop", dict(refs=(7, 9), edit=_set(1, me_type=svtme.ME_OPEN_LOOP))
    yield "two references", dict(edit=_set(0, num_refs0=2))
    yield "no reference", dict(edit=_set(0, num_refs0=0))
    yield "two lists", dict(edit=_set(0, num_lists=2))
    yield "another centre", dict(refs=(7, 9), edit=_set(1, picture_number=BASE + 6))
    yield "another size", dict(refs=(7, 9), edit=_set(1, width=64, height=64))
    yield "a size that is no multiple of 8", dict(edit=_set(0, width=124), src=(124, 128))
    yield "sb_begin 1", dict(edit=_set(0, sb_begin=1))
    yield "sb_count 1 of 4", dict(edit=_set(0, sb_count=1))
    yield "sb_count 1 of 4 in the last of 16", dict(refs=(7,) * svtme.MAX_BATCH_JOBS,
                                                    edit=_set(svtme.MAX_BATCH_JOBS - 1, sb_count=1))
    yield "src_width 120 under 128", dict(src=(120, 128))
    yield "src_height 129 over 128", dict(src=(128, 129))
    yield "src_width 0", dict(src=(0, 128))
    yield "plane_stride under src_width", dict(src=(124, 128), stride=123)
    for field, v in (("half_pel_mode", 4), ("quarter_pel_mode", 4), ("eight_pel_mode", 2), ("use_2tap", 2),
                     ("sub_sampling_shift", 2), ("enable_8x8_pred", 2)):
        yield f"sub-pel {field} {v}", dict(sp=_subpel(svtme, **{field: v}))
    yield "tf_mv_dist_th 32768", dict(fc=_filter(svtme, tf_mv_dist_th=32768))
    yield "filter sub_sampling_shift 2", dict(fc=_filter(svtme, sub_sampling_shift=2))
    yield "the result picture is the reference", dict(out_pn=7)
    yield "the result picture is the last reference of 16", dict(refs=(7,) * (svtme.MAX_BATCH_JOBS - 1) + (9,), out_pn=9)


def _subpel(svtme, **over):
    return svtme.TfSubpelControls.from_dict(dict({f: G.CONTROL_SETS["l8"][f] for f in G.SUBPEL_FIELDS}, **over))


def _filter(svtme, **over):
    return svtme.TfFilterControls.from_dict(dict({"tf_decay_factor_fp16": 2_000_000, "tf_mv_dist_th": 64,
                                                  "sub_sampling_shift": 1}, **over))


def test_tfw_bad_parameters_without_a_device(svtme):
    """The checks that need no context run before the context is touched: a block of zero bytes
    stands in for it (no device, no context can be created here)."""
    lib = svtme.load_product()
    fake = C.create_string_buffer(64)
    ctx = C.cast(fake, C.c_void_p)
    calls = list(_bad_calls(svtme))
    assert len(calls) == 31
    for what, kw in calls:
        assert _call(svtme, lib, ctx, **kw) == BAD_PARAMETER, what
    assert fake.raw == bytes(64)


def test_tfw_sweep_cases_hold_what_the_tests_need():
    assert len(ME_CASES) == 11
    assert {(c["w"], c["h"]) for c in ME_CASES} == {(128, 128), (192, 136), (124, 66)}
    assert max(len(c["refs"]) for c in ME_CASES) == 3
    assert any((c["w"], c["h"], len(c["refs"])) == (72, 40, 16) for c in CHAIN_CASES)
    assert {len(c["refs"]) for c in CHAIN_CASES} >= {1, 16}


# ----------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------
def upload(gpu, win: dict) -> dict:
    frames = G.case_frames(win)
    for t, f in frames.items():
        gpu.upload(BASE + t, f)
    return frames


def release(gpu, numbers):
    for t in numbers:
        try:
            gpu.release(BASE + t)
        except RuntimeError:  # not resident: the test failed before it made the picture
            pass


def run_window(svtme, gpu, win, out_pn, centre_pn=None, want=("plane", "records", "subpel", "err32")):
    centre_pn = BASE + win["centre"] if centre_pn is None else centre_pn
    jobs = [tf_job(svtme, win, centre_pn, BASE + r) for r in win["refs"]]
    sp, fc = controls_of(svtme, win)
    return gpu.tf_window(jobs, win["w"], win["h"], sp, fc, out_pn, want=want)


def three_calls(svtme, gpu, win, centre_pn=None) -> dict:
    """The window as the three calls through host memory, cropped and named as tf_window's result."""
    centre_pn = BASE + win["centre"] if centre_pn is None else centre_pn
    refs = [BASE + r for r in win["refs"]]
    sp, fc = controls_of(svtme, win)
    layout = svtme.PackLayout(n_pus=85, max_cand=1, max_refs=1, full_records=1, sb_results=0)
    me = np.stack([np.frombuffer(gpu.submit_packed(tf_job(svtme, win, centre_pn, r), layout), svtme.REF_RECORD_DTYPE)
                   for r in refs])
    sub = gpu.tf_subpel(centre_pn, refs, win["w"], win["h"], sp, me)
    plane, err32 = gpu.tf_filter(centre_pn, refs, svtme.align8(win["w"]), svtme.align8(win["h"]), fc, sub)
    return {"plane": plane[:win["h"], :win["w"]], "records": me, "subpel": sub, "err32": err32}


def assert_same(svtme, got: dict, want: dict, what: str):
    assert sorted(got) == sorted(want), what
    assert got["records"].shape == want["records"].shape, what
    assert svtme.compare_records(want["records"].reshape(-1, 1), got["records"].reshape(-1, 1)) == [], what
    assert got["subpel"].shape == want["subpel"].shape and got["subpel"].tobytes() == want["subpel"].tobytes(), \
        (what, "subpel", np.argwhere(got["subpel"].view(np.uint8) != want["subpel"].view(np.uint8))[:3])
    assert np.array_equal(got["err32"], want["err32"]), (what, "err32")
    if not np.array_equal(got["plane"], want["plane"]):
        y, x = np.argwhere(got["plane"] != want["plane"])[0]
        raise AssertionError(f"{what}: {int((got['plane'] != want['plane']).sum())} pixels differ, first at x {x} "
                             f"y {y}: {got['plane'][y, x]} for {want['plane'][y, x]}")


def levels(gpu, pn) -> list:
    return [gpu.download(pn, lv) for lv in range(3)]


def assert_levels(got: list, want, what):
    want = [getattr(want, name) for name in LEVELS] if not isinstance(want, list) else want
    for lv in range(3):
        assert got[lv].shape == want[lv].shape and np.array_equal(got[lv], want[lv]), (what, LEVELS[lv])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ME_CASES, ids=lambda c: c["id"])
def test_tfw_vs_reference_golden(svtme, gpu, gold, case):
    """The reference's own records, sub-pel results, 32x32 errors and filtered plane of every
    fixture case that starts from the TF-ME job: 128x128, 192x136 (a partial bottom SB row),
    124x66 (not multiples of 8) and the window of 3."""
    name, win = case["id"], window_of(case)
    frames = upload(gpu, win)
    try:
        got = run_window(svtme, gpu, win, BASE + OUT)
    finally:
        release(gpu, list(frames) + [OUT])
    # the fixture's plane is the aligned picture's: the columns and rows beyond the true size are
    # re-padded by the call and belong to test_tfw_resident_result
    want = {"plane": gold[name + ".plane"][:win["h"], :win["w"]], "records": gold[name + ".rec"],
            "subpel": gold[name + ".out"], "err32": gold[name + ".err32"]}
    assert_same(svtme, got, want, name)


def _chain_cases():
    cases = [M.sweep_case(s) for s in M.SWEEP_SEEDS[:8]]
    if not any((c["w"], c["h"], len(c["refs"])) == (72, 40, 16) for c in cases):
        import tfsp_model

        extra = dict(cases[1], id="n16_72x40", w=72, h=40)
        extra["refs"] = tfsp_model.sweep_case(1, G.S.MAX_BATCH_JOBS)["refs"]
        cases.append(extra)
    return cases


CHAIN_CASES = _chain_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CHAIN_CASES, ids=lambda c: c["id"])
def test_tfw_equals_the_three_calls(svtme, gpu, case):
    """Random shapes (8x8 to 200x72), contents, controls and windows of 1 to 16 references: every
    output of the window is that of submit_packed -> tf_subpel -> tf_filter on the same pictures."""
    win = window_of(case)
    what = f"{case['id']}: {win['w']}x{win['h']} {win['kind']}, references {win['refs']}"
    frames = upload(gpu, win)
    try:
        want = three_calls(svtme, gpu, win)
        got = run_window(svtme, gpu, win, BASE + OUT)
        only = run_window(svtme, gpu, win, BASE + OUT, want=("err32",))  # a subset of the outputs
    finally:
        release(gpu, list(frames) + [OUT])
    assert_same(svtme, got, want, what)
    assert sorted(only) == ["err32"] and np.array_equal(only["err32"], want["err32"]), what


RESIDENT = [own_window(64, 64, (7, 9), "l2"), own_window(72, 40, (9,), "l8"),
            own_window(124, 66, (7, 6), "l2"), own_window(200, 72, (9, 7), "l5")]


@pytest.mark.gpu
@pytest.mark.parametrize("win", RESIDENT, ids=lambda w: w["id"])
def test_tfw_resident_result(svtme, gpu, win):
    """The result picture under a fresh number is what an upload of the returned plane would be:
    levels 0, 1 and 2, margins and the re-pad to 8 included. The centre stays bit for bit."""
    frames = upload(gpu, win)
    try:
        before = levels(gpu, BASE + win["centre"])
        got = run_window(svtme, gpu, win, BASE + OUT)
        result = levels(gpu, BASE + OUT)
        after = levels(gpu, BASE + win["centre"])
    finally:
        release(gpu, list(frames) + [OUT])
    assert got["plane"].shape == (win["h"], win["w"])
    assert not np.array_equal(got["plane"], frames[win["centre"]])  # the filter changed the picture
    assert_levels(result, svtme.build_host_pyramid(got["plane"], "oracle"), win["id"])
    assert_levels(after, before, win["id"] + ": the centre")
    assert_levels(before, svtme.build_host_pyramid(frames[win["centre"]], "oracle"), win["id"] + ": the upload")


@pytest.mark.gpu
@pytest.mark.parametrize("win", [RESIDENT[2], RESIDENT[1]], ids=lambda w: w["id"])
def test_tfw_in_place(svtme, gpu, win):
    """out_picture_number == the centre: the centre becomes what the fresh number held, and a
    second window reads the filtered centre as the three calls read an upload of that plane (under
    the centre's own number: the TF-ME search depends on the distance between picture numbers)."""
    centre = BASE + win["centre"]
    frames = upload(gpu, win)
    try:
        fresh = run_window(svtme, gpu, win, BASE + OUT)
        want_levels = levels(gpu, BASE + OUT)
        first = run_window(svtme, gpu, win, centre)
        got_levels = levels(gpu, centre)
        second = run_window(svtme, gpu, win, centre)
        second_levels = levels(gpu, centre)
        gpu.upload(centre, fresh["plane"])  # a plain upload of the filtered plane
        want_second = three_calls(svtme, gpu, win)
    finally:
        release(gpu, list(frames) + [OUT])
    assert_same(svtme, first, fresh, win["id"] + ": in place")
    assert_levels(got_levels, want_levels, win["id"] + ": in place")
    assert_same(svtme, second, want_second, win["id"] + ": the second window")
    assert_levels(second_levels, svtme.build_host_pyramid(second["plane"], "oracle"), win["id"] + ": the second window")
    assert not np.array_equal(first["plane"], frames[win["centre"]])  # the filter changed the picture
    assert not np.array_equal(second["plane"], first["plane"])  # and the second window read the changed one


@pytest.mark.gpu
def test_tfw_orders_later_jobs_without_a_host_wait(svtme, gpu):
    """A window with no outputs returns once queued; an open-loop job queued at once on lane 0,
    and again on lane 1, with the result picture as its reference, sees the filtered picture: its
    records are those of the same job against a plain upload of the filtered plane under another
    number (one as far from the job's picture, since the search depends on that distance)."""
    win = own_window(200, 72, (9, 7), "l2")
    w, h = win["w"], win["h"]
    cur, centre = BASE + 9, BASE + win["centre"]
    other = {BASE + OUT: 2 * cur - (BASE + OUT), centre: 2 * cur - centre}  # result picture -> the plain upload
    frames = upload(gpu, win)
    stale = svtme.test_frames("noise", w, h, [0])[0]
    layout = svtme.PackLayout(n_pus=85, max_cand=1, max_refs=1, full_records=1, sb_results=0)
    ctrl = svtme.derive_controls(8, 35, svtme.input_resolution_of(w, h), 1)

    def records(ref_pn, lane):
        job = svtme.make_job(w, h, ctrl, cur, (ref_pn,), (), temporal_layer_index=1, ref_count_used=(1, 0))
        return np.frombuffer(gpu.submit_packed(job, layout, lane=lane), svtme.REF_RECORD_DTYPE).reshape(-1, 1)

    try:
        plane = run_window(svtme, gpu, win, BASE + OUT, want=("plane",))["plane"]
        want = {}
        for result, pn in other.items():
            assert pn not in (BASE + t for t in frames) and pn != BASE + OUT
            gpu.upload(pn, stale)
            unfiltered = records(pn, 0)
            gpu.upload(pn, plane)
            want[result] = records(pn, 0)
            assert svtme.compare_records(want[result], unfiltered) != []  # the reference matters
        for lane in (0, 1):
            gpu.upload(BASE + OUT, stale)  # the result picture holds something else before the window
            assert run_window(svtme, gpu, win, BASE + OUT, want=()) == {}
            assert svtme.compare_records(want[BASE + OUT], records(BASE + OUT, lane)) == [], f"lane {lane}"
        # in place, the job on lane 1: the centre as its reference
        assert run_window(svtme, gpu, win, centre, want=()) == {}
        assert svtme.compare_records(want[centre], records(centre, 1)) == [], "in place, lane 1"
        gpu.sync()
    finally:
        for pn in other.values():
            gpu.release(pn)
        release(gpu, list(frames) + [OUT])


@pytest.mark.gpu
def test_tfw_bad_parameters_with_a_context(svtme, gpu):
    small = G.tfsp_content.fractional_frames(128, 128, (7, 8, 9))
    big = G.tfsp_content.fractional_frames(192, 136, (7,))
    for t in (7, 8, 9):
        gpu.upload(BASE + t, small[t])
    gpu.upload(BASE + 107, big[7])
    lib, ctx = gpu.lib, gpu.ctx
    try:
        before = {t: levels(gpu, BASE + t) for t in (7, 8, 9, 107)}
        for what, kw in _bad_calls(svtme):
            assert _call(svtme, lib, ctx, **kw) == BAD_PARAMETER, what
        assert _call(svtme, lib, ctx, refs=(7, 9), out_pn=9) == BAD_PARAMETER  # the result among the references
        assert _call(svtme, lib, ctx, refs=(7, 999)) == BAD_PARAMETER  # a reference that is not resident
        assert _call(svtme, lib, ctx, centre=999) == BAD_PARAMETER  # the centre is not
        assert _call(svtme, lib, ctx, refs=(7, 107)) == BAD_PARAMETER  # a reference of another size
        assert _call(svtme, lib, ctx, w=192, h=136) == BAD_PARAMETER  # the window's size is not the pictures'
        for t in (7, 8, 9, 107):
            assert_levels(levels(gpu, BASE + t), before[t], f"picture {t} after the refused calls")
        with pytest.raises(RuntimeError):
            gpu.download(BASE + OUT, 0)  # no refused call made the result picture
        # and the valid forms of the same calls succeed
        assert _call(svtme, lib, ctx) == 0
        assert _call(svtme, lib, ctx, refs=(7, 9), src=(124, 122), stride=200) == 0
        assert _call(svtme, lib, ctx, want_plane=False, stride=0) == 0
        assert _call(svtme, lib, ctx, null="out") == 0
        assert _call(svtme, lib, ctx, refs=(7,) * svtme.MAX_BATCH_JOBS, out_pn=8) == 0  # in place, 16 jobs
        gpu.sync()
    finally:
        release(gpu, (7, 8, 9, 107, OUT))
