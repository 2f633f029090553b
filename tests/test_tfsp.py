"""Temporal filtering's sub-pel refinement (svtme_tf_subpel, include/svtme.h).

Expected values are the fixtures tests/golden/tfsp_cases.{json,npz}: the
reference's own planes, ME records, svt_inter_predictor and variance kernels
under the control flow restated in tests/golden/make_golden_tfsp.py. CPU tests
pin the ABI, the parameter checks that need no context and the fixtures
themselves; GPU tests compare svtme_tf_subpel bit-exactly, as whole structs,
against the fixtures.
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

import make_golden_tfsp as G  # noqa: E402

DOC = json.load(open(os.path.join(GOLD, "tfsp_cases.json")))
TFSP_CASES = DOC["cases"]
BAD_PARAMETER = 0x80001005
BASE = 9000  # picture numbers of this file's uploads


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLD, "tfsp_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def case_by_id(name):
    return next(c for c in TFSP_CASES if c["id"] == name)


# ----------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------
def test_tfsp_symbol_exported(svtme):
    assert hasattr(svtme.load_product(), "svtme_tf_subpel")


def test_tfsp_case_list_matches_generator():
    assert TFSP_CASES == G.case_dicts()
    assert set(DOC["controls"]) == set(G.CONTROL_SETS)
    for name, cs in G.CONTROL_SETS.items():
        want = {k: (v if v != G.U64_MAX else "UINT64_MAX") for k, v in cs.items()}
        assert DOC["controls"][name] == want, name


def test_tfsp_control_sets_cover_the_modes():
    sets = [G.CONTROL_SETS[c["controls"]] for c in TFSP_CASES]
    assert {s["half_pel_mode"] for s in sets} >= {1, 2}
    for field in ("use_2tap", "sub_sampling_shift", "enable_8x8_pred"):
        assert {s[field] for s in sets} == {0, 1}, field
    for field in ("subpel_early_exit_th", "pred_error_32x32_th", "use_pred_64x64_only_th"):
        assert any(s[field] for s in sets), field
    assert "l8" in {c["controls"] for c in TFSP_CASES}  # the level preset 8 uses
    assert {(c["w"], c["h"]) for c in TFSP_CASES} == {(128, 128), (192, 136)}
    assert {len(c["refs"]) for c in TFSP_CASES} >= {1, 3}
    assert {c["records"] for c in TFSP_CASES} == {"me", "edges"}


def test_tfsp_coverage_counts_are_all_non_zero():
    assert set(DOC["coverage"]) == set(G.COVERAGE_KEYS)
    zero = [k for k, v in DOC["coverage"].items() if not v > 0]
    assert zero == []


def test_tfsp_fixture_shapes(svtme, gold):
    assert sorted(gold) == sorted(c["id"] + s for c in TFSP_CASES for s in (".rec", ".out"))
    for case in TFSP_CASES:
        shape = (len(case["refs"]), svtme.sb_total(svtme.align8(case["w"]), svtme.align8(case["h"])))
        rec, out = gold[case["id"] + ".rec"], gold[case["id"] + ".out"]
        assert rec.dtype == svtme.REF_RECORD_DTYPE and out.dtype == svtme.TF_SUBPEL_SB_DTYPE
        assert rec.shape == shape and out.shape == shape, case["id"]
        assert set(np.unique(out["branch"])) <= {svtme.TFSP_64_ONLY, svtme.TFSP_64_CHOSEN, svtme.TFSP_32}
        # the fixed convention of the unwritten blocks: MV 0 and error INT_MAX (32x32 blocks on a 64x64
        # branch carry the 64x64 MV)
        unset = out["error"] == svtme.TFSP_UNSET_ERROR
        unset[..., 1:5] = False
        assert not out["mv"]["x"][unset].any() and not out["mv"]["y"][unset].any()
        on64 = out["branch"] != svtme.TFSP_32
        for i in range(1, 5):
            assert (out["error"][..., i][on64] == svtme.TFSP_UNSET_ERROR).all()
            assert (out["mv"][..., i][on64] == out["mv"][..., 0][on64]).all()


_ABI_PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "svtme.h"
#define S(T) printf("sizeof " #T " %zu\n", sizeof(T))
#define O(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
    S(svtme_tf_subpel_controls); S(svtme_tf_subpel_sb);
    O(svtme_tf_subpel_controls, half_pel_mode); O(svtme_tf_subpel_controls, quarter_pel_mode);
    O(svtme_tf_subpel_controls, eight_pel_mode); O(svtme_tf_subpel_controls, use_2tap);
    O(svtme_tf_subpel_controls, sub_sampling_shift); O(svtme_tf_subpel_controls, enable_8x8_pred);
    O(svtme_tf_subpel_controls, use_pred_64x64_only_th); O(svtme_tf_subpel_controls, subpel_early_exit_th);
    O(svtme_tf_subpel_controls, pred_error_32x32_th);
    O(svtme_tf_subpel_sb, mv); O(svtme_tf_subpel_sb, error); O(svtme_tf_subpel_sb, split_32x32);
    O(svtme_tf_subpel_sb, split_16x16); O(svtme_tf_subpel_sb, branch); O(svtme_tf_subpel_sb, pad);
    printf("SVTME_TFSP_64_ONLY %d\nSVTME_TFSP_64_CHOSEN %d\nSVTME_TFSP_32 %d\n", SVTME_TFSP_64_ONLY,
           SVTME_TFSP_64_CHOSEN, SVTME_TFSP_32);
    printf("SVTME_TFSP_BLOCKS %d\nSVTME_TFSP_OFF_32 %d\nSVTME_TFSP_OFF_16 %d\nSVTME_TFSP_OFF_8 %d\n",
           SVTME_TFSP_BLOCKS, SVTME_TFSP_OFF_32, SVTME_TFSP_OFF_16, SVTME_TFSP_OFF_8);
    printf("SVTME_TFSP_UNSET_ERROR %u\nSVTME_MAX_BATCH_JOBS %d\n", SVTME_TFSP_UNSET_ERROR, SVTME_MAX_BATCH_JOBS);
    return 0;
}
"""


def test_tfsp_struct_sizes_and_offsets_equal_the_headers(svtme, tmp_path):
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text(_ABI_PROGRAM)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        key, val = line.rsplit(" ", 1)
        got[key] = int(val)
    ctl, sb = svtme.TfSubpelControls, svtme.TF_SUBPEL_SB_DTYPE
    assert got["sizeof svtme_tf_subpel_controls"] == C.sizeof(ctl) == 16
    assert got["sizeof svtme_tf_subpel_sb"] == sb.itemsize == 704
    for name, _ in ctl._fields_:
        assert got["svtme_tf_subpel_controls." + name] == getattr(ctl, name).offset, name
    assert len(ctl._fields_) == 9
    for name in sb.names:
        assert got["svtme_tf_subpel_sb." + name] == sb.fields[name][1], name
    assert sb["mv"].subdtype[0].itemsize == 4 and sb["mv"].subdtype[0].fields["y"][1] == 2
    assert (got["SVTME_TFSP_64_ONLY"], got["SVTME_TFSP_64_CHOSEN"], got["SVTME_TFSP_32"]) == \
        (svtme.TFSP_64_ONLY, svtme.TFSP_64_CHOSEN, svtme.TFSP_32)
    assert (got["SVTME_TFSP_BLOCKS"], got["SVTME_TFSP_OFF_32"], got["SVTME_TFSP_OFF_16"], got["SVTME_TFSP_OFF_8"]) == \
        (svtme.TFSP_BLOCKS, svtme.TFSP_OFF_32, svtme.TFSP_OFF_16, svtme.TFSP_OFF_8)
    assert got["SVTME_TFSP_UNSET_ERROR"] == svtme.TFSP_UNSET_ERROR == 2 ** 31 - 1
    assert got["SVTME_MAX_BATCH_JOBS"] == svtme.MAX_BATCH_JOBS


def _call(svtme, lib, ctx, refs, n=None, ctl=None, null=None, w=128, h=128, centre=BASE + 8):
    """-> the status of svtme_tf_subpel; on an error `out` must stay untouched."""
    ctl = ctl if ctl is not None else G.subpel_controls("l2")
    sbs = svtme.sb_total(svtme.align8(w), svtme.align8(h))
    slots = max(len(refs), svtme.MAX_BATCH_JOBS + 1)
    arr = (C.c_uint64 * slots)(*refs)
    recs = np.zeros((slots, sbs), svtme.REF_RECORD_DTYPE)
    out = np.full(slots * sbs * svtme.TF_SUBPEL_SB_DTYPE.itemsize, 0x5A, np.uint8)
    st = lib.svtme_tf_subpel(None if null == "ctx" else ctx, centre, None if null == "refs" else arr,
                             len(refs) if n is None else n, w, h, None if null == "controls" else C.byref(ctl),
                             None if null == "records" else recs.ctypes.data,
                             None if null == "out" else out.ctypes.data)
    if st:
        assert (out == 0x5A).all()
        assert lib.svtme_last_error().decode() != ""
    return st & 0xFFFFFFFF


def _bad_controls():
    for field, value in (("half_pel_mode", 4), ("quarter_pel_mode", 4), ("eight_pel_mode", 2), ("use_2tap", 2),
                         ("sub_sampling_shift", 2), ("enable_8x8_pred", 2)):
        ctl = G.subpel_controls("l2")
        setattr(ctl, field, value)
        yield field, ctl


def test_tfsp_bad_parameters_without_a_device(svtme):
    """The checks that need no context run before the context is touched: a block of zero bytes
    stands in for it (no device, no context can be created here)."""
    lib = svtme.load_product()
    fake = C.create_string_buffer(64)
    ctx = C.cast(fake, C.c_void_p)
    ok = [BASE + 7]
    for null in ("ctx", "refs", "controls", "records", "out"):
        assert _call(svtme, lib, ctx, ok, null=null) == BAD_PARAMETER, null
    assert _call(svtme, lib, ctx, ok, n=0) == BAD_PARAMETER
    assert _call(svtme, lib, ctx, ok * (svtme.MAX_BATCH_JOBS + 1)) == BAD_PARAMETER
    for field, ctl in _bad_controls():
        assert _call(svtme, lib, ctx, ok, ctl=ctl) == BAD_PARAMETER, field
    assert fake.raw == bytes(64)


# AV1 specification, Subpel_Filters[0] (EIGHTTAP_REGULAR), phases 0..8; phase 16 - p is phase p
# mirrored, and every phase sums to 128. The bilinear filter is 128 - 8 p, 8 p.
_SPEC_HALF = [[0, 0, 0, 128, 0, 0, 0, 0], [0, 2, -6, 126, 8, -2, 0, 0], [0, 2, -10, 122, 18, -4, 0, 0],
              [0, 2, -12, 116, 28, -8, 2, 0], [0, 2, -14, 110, 38, -10, 2, 0], [0, 2, -14, 102, 48, -12, 2, 0],
              [0, 2, -16, 94, 58, -12, 2, 0], [0, 2, -14, 84, 66, -12, 2, 0], [0, 2, -14, 76, 76, -14, 2, 0]]
SPEC_REGULAR = np.array(_SPEC_HALF + [_SPEC_HALF[16 - p][::-1] for p in range(9, 16)], np.int64)
assert (SPEC_REGULAR.sum(axis=1) == 128).all()


def numpy_distortion(cen, ref, pad, W, H, b, px, py, mvx, mvy, bil, ss):
    """The distortion of one position by the AV1 specification's filters and the rounding of the
    single-reference convolve (round_0 3, round_1 11), independent of the reference's code."""
    qx, _, _ = G.clamp(mvx, px, b, W)
    qy, _, _ = G.clamp(mvy, py, b, H)
    fx, fy, x0, y0 = qx & 15, qy & 15, px + (qx >> 4), py + (qy >> 4)
    taps = (lambda p: np.array([0, 0, 0, 128 - 8 * p, 8 * p, 0, 0, 0], np.int64)) if bil else (lambda p: SPEC_REGULAR[p])
    win = ref[pad + y0 - 3:pad + y0 + b + 4, pad + x0 - 3:pad + x0 + b + 4].astype(np.int64)
    if fx and fy:
        im = ((1 << 14) + sum(taps(fx)[k] * win[:, k:k + b] for k in range(8)) + 4) >> 3
        s = (1 << 19) + sum(taps(fy)[k] * im[k:k + b] for k in range(8))
        pred = ((s + 1024) >> 11) - 384
    elif fx:
        pred = (((sum(taps(fx)[k] * win[3:3 + b, k:k + b] for k in range(8)) + 4) >> 3) + 8) >> 4
    elif fy:
        pred = (sum(taps(fy)[k] * win[k:k + b, 3:3 + b] for k in range(8)) + 64) >> 7
    else:
        pred = win[3:3 + b, 3:3 + b]
    pred = np.clip(pred, 0, 255)[::1 << ss]
    d = pred - cen[pad + py:pad + py + b:1 << ss, pad + px:pad + px + b].astype(np.int64)
    total, sse = int(d.sum()), int((d * d).sum())
    q = abs(total * total) // (b * (b >> ss))
    return ((sse - q) & 0xFFFFFFFF) << ss


@pytest.mark.parametrize("name", ["frac128_l2", "frac128_l8_w3", "edges192_l8"])
def test_tfsp_fixture_errors_vs_specification_filters(svtme, gold, name):
    """Every block error of a fixture at its winning MV, recomputed with the filter taps of the AV1
    specification in numpy on the oracle's planes (pinned to the reference's)."""
    case = case_by_id(name)
    cs = G.CONTROL_SETS[case["controls"]]
    pyr = {t: svtme.build_host_pyramid(f, "oracle") for t, f in G.case_frames(case).items()}
    W, H = svtme.align8(case["w"]), svtme.align8(case["h"])
    wb, pad, checked = (W + 63) // 64, svtme.PAD_FULL, 0
    out = gold[name + ".out"]
    for r, ref in enumerate(case["refs"]):
        for k in range(out.shape[1]):
            o = out[r, k]
            for idx in range(svtme.TFSP_BLOCKS):
                level = 0 if idx < 1 else 1 if idx < 5 else 2 if idx < 21 else 3
                if o["error"][idx] == svtme.TFSP_UNSET_ERROR:
                    continue
                if level == 2 and o["split_16x16"][(idx - 5) // 4][(idx - 5) % 4]:
                    continue  # the 8x8 sum replaced it
                bx, by = G.block_xy(level, idx - (0, 1, 5, 21)[level])
                d = numpy_distortion(pyr[case["centre"]].full, pyr[ref].full, pad, W, H, 64 >> level,
                                     64 * (k % wb) + bx, 64 * (k // wb) + by, int(o["mv"]["x"][idx]),
                                     int(o["mv"]["y"][idx]), bool(cs["use_2tap"]) and level < 2,
                                     cs["sub_sampling_shift"])
                assert d == int(o["error"][idx]), (name, r, k, idx)
                checked += 1
    assert checked >= out.shape[0] * out.shape[1]


@pytest.mark.skipif(not ref_available(), reason="oracle/_ref not built (needs the reference's sources)")
def test_tfsp_fixture_regenerates(gold):
    case = case_by_id("frac128_l2")
    rec, out = G.generate_case(case)
    assert rec.tobytes() == gold[case["id"] + ".rec"].tobytes()
    assert out.tobytes() == gold[case["id"] + ".out"].tobytes()


# ----------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------
def upload_case(gpu, case):
    frames = G.case_frames(case)
    for t, f in frames.items():
        gpu.upload(BASE + t, f)
    return frames


def release_case(gpu, frames):
    for t in frames:
        gpu.release(BASE + t)


def run_case(gpu, case, records, refs=None):
    refs = case["refs"] if refs is None else refs
    return gpu.tf_subpel(BASE + case["centre"], [BASE + r for r in refs], case["w"], case["h"],
                         G.subpel_controls(case["controls"]), records)


def assert_structs_equal(got, want, what):
    """Whole structs, bit-exact; the first differing (reference, SB) is named by field."""
    if got.tobytes() == want.tobytes():
        return
    assert got.shape == want.shape, what
    for idx in np.ndindex(got.shape):
        if got[idx].tobytes() != want[idx].tobytes():
            diff = {f: (got[idx][f].tolist(), want[idx][f].tolist()) for f in got.dtype.names
                    if got[idx][f].tobytes() != want[idx][f].tobytes()}
            raise AssertionError(f"{what}: (reference, SB) {idx} differs (got, want): {diff}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", TFSP_CASES, ids=lambda c: c["id"])
def test_tfsp_vs_reference_golden(svtme, gpu, gold, case):
    frames = upload_case(gpu, case)
    try:
        out = run_case(gpu, case, gold[case["id"] + ".rec"])
        assert_structs_equal(out, gold[case["id"] + ".out"], case["id"])
    finally:
        release_case(gpu, frames)


@pytest.mark.gpu
def test_tfsp_window_equals_singles(svtme, gpu, gold):
    case = case_by_id("frac128_l8_w3")
    frames = upload_case(gpu, case)
    try:
        rec, want = gold[case["id"] + ".rec"], gold[case["id"] + ".out"]
        out = run_case(gpu, case, rec)
        assert_structs_equal(out, want, "window of 3")
        for k, r in enumerate(case["refs"]):
            one = run_case(gpu, case, rec[k:k + 1], refs=[r])
            assert one.tobytes() == out[k:k + 1].tobytes(), k
        # the same reference in every slot of a full window
        full = run_case(gpu, case, np.repeat(rec[1:2], svtme.MAX_BATCH_JOBS, axis=0),
                        refs=[case["refs"][1]] * svtme.MAX_BATCH_JOBS)
        for k in range(svtme.MAX_BATCH_JOBS):
            assert full[k].tobytes() == out[1].tobytes(), k
    finally:
        release_case(gpu, frames)


@pytest.mark.gpu
def test_tfsp_sees_a_reuploaded_reference(svtme, gpu, gold):
    case = case_by_id("frac128_l5")
    frames = G.case_frames(case)
    ref = case["refs"][0]
    other = G.tfsp_content.fractional_frames(case["w"], case["h"], [ref - 2])[ref - 2]
    rec, want = gold[case["id"] + ".rec"], gold[case["id"] + ".out"]
    gpu.upload(BASE + case["centre"], frames[case["centre"]])
    gpu.upload(BASE + ref, other)  # another picture under the reference's number first
    try:
        stale = run_case(gpu, case, rec)
        assert stale.tobytes() != want.tobytes()
        gpu.upload(BASE + ref, frames[ref])
        assert_structs_equal(run_case(gpu, case, rec), want, "after the re-upload")
        gpu.invalidate(BASE + ref, other)
        assert run_case(gpu, case, rec).tobytes() == stale.tobytes()
    finally:
        release_case(gpu, frames)


@pytest.mark.gpu
def test_tfsp_after_me_jobs_on_either_lane(svtme, gpu, gold):
    """The TF-ME job of the window on lane 0, then on lane 1, each followed by the refinement of
    the records that job returned: the GPU's own records are the reference's, and the result
    does not depend on the lane that ran before."""
    case = case_by_id("frac192_l2")
    cs = G.CONTROL_SETS[case["controls"]]
    w, h, ref = case["w"], case["h"], case["refs"][0]
    frames = upload_case(gpu, case)
    try:
        ctrl = svtme.derive_controls_tf(cs["hme_me_level"], 0, 35, svtme.input_resolution_of(w, h))
        job = svtme.case_job(ctrl, w, h, BASE + case["centre"], (BASE + ref,), (), 0, me_type=svtme.ME_MCTF,
                             tf_me_exit_th=cs["me_exit_th"])
        layout = svtme.PackLayout(n_pus=85, max_cand=1, max_refs=1, full_records=1, sb_results=0)
        want_rec, want = gold[case["id"] + ".rec"], gold[case["id"] + ".out"]
        for lane in (0, 1, 0):
            packed = gpu.submit_packed(job, layout, lane=lane)
            rec = np.frombuffer(packed, svtme.REF_RECORD_DTYPE).reshape(1, -1)
            assert svtme.compare_records(want_rec.reshape(-1, 1), rec.reshape(-1, 1)) == []
            assert_structs_equal(run_case(gpu, case, rec), want, f"after lane {lane}")
    finally:
        release_case(gpu, frames)


@pytest.mark.gpu
def test_tfsp_bad_parameters_with_a_context(svtme, gpu):
    small = G.tfsp_content.fractional_frames(128, 128, (7, 8))
    big = G.tfsp_content.fractional_frames(192, 136, (7,))
    gpu.upload(BASE + 7, small[7])
    gpu.upload(BASE + 8, small[8])
    gpu.upload(BASE + 107, big[7])
    lib, ctx = gpu.lib, gpu.ctx
    ok = [BASE + 7]
    try:
        for null in ("ctx", "refs", "controls", "records", "out"):
            assert _call(svtme, lib, ctx, ok, null=null) == BAD_PARAMETER, null
        assert _call(svtme, lib, ctx, ok, n=0) == BAD_PARAMETER
        assert _call(svtme, lib, ctx, ok * (svtme.MAX_BATCH_JOBS + 1)) == BAD_PARAMETER
        for field, ctl in _bad_controls():
            assert _call(svtme, lib, ctx, ok, ctl=ctl) == BAD_PARAMETER, field
        assert _call(svtme, lib, ctx, [BASE + 999]) == BAD_PARAMETER  # a reference that is not resident
        assert _call(svtme, lib, ctx, ok, centre=BASE + 999) == BAD_PARAMETER  # the centre is not
        assert _call(svtme, lib, ctx, [BASE + 7, BASE + 107]) == BAD_PARAMETER  # a reference of another size
        assert _call(svtme, lib, ctx, ok, w=192, h=136) == BAD_PARAMETER  # the window's size is not the pictures'
        # and the valid forms of the same calls succeed
        assert _call(svtme, lib, ctx, ok) == 0
        assert _call(svtme, lib, ctx, ok * svtme.MAX_BATCH_JOBS) == 0
    finally:
        for t in (7, 8, 107):
            gpu.release(BASE + t)
