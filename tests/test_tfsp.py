"""Temporal filtering's sub-pel refinement (svtme_tf_subpel, include/svtme.h).

Expected values are the fixtures tests/golden/tfsp_cases.{json,npz}: the
reference's own planes, ME records, svt_inter_predictor and variance kernels
under the control flow restated in tests/golden/make_golden_tfsp.py. Beside them
stands a model of the whole refinement in numpy (tests/tfsp_model.py: the same
control flow around the AV1 specification's filters), which needs nothing from
the reference. CPU tests pin the ABI, the parameter checks that need no context,
the fixtures themselves, the model to the fixtures and, where the reference is
built, the model to the reference on the random sweep's inputs; GPU tests
compare svtme_tf_subpel bit-exactly, as whole structs, against the fixtures and,
on the sweep's inputs, against the model.
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
import tfsp_model as M  # noqa: E402
from tfsp_model import SPEC_REGULAR, numpy_distortion  # noqa: E402,F401

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
    assert {c["controls"] for c in TFSP_CASES} == set(G.CONTROL_SETS)  # every set is used
    sets = [G.CONTROL_SETS[c["controls"]] for c in TFSP_CASES]
    # every value the host accepts (svtme_tf_subpel's range checks)
    assert {s["half_pel_mode"] for s in sets} == {0, 1, 2, 3}
    assert {s["quarter_pel_mode"] for s in sets} == {0, 1, 2, 3}
    for field in ("eight_pel_mode", "use_2tap", "sub_sampling_shift", "enable_8x8_pred"):
        assert {s[field] for s in sets} == {0, 1}, field
    assert {s["use_pred_64x64_only_th"] for s in sets} == {0, 10, 35, 200}
    assert {s["subpel_early_exit_th"] for s in sets} == {0, 1, 2, 4, 8}
    assert {s["pred_error_32x32_th"] for s in sets} == {0, 8 * 32 * 32, 20 * 32 * 32, G.U64_MAX}
    # combinations: no half-pel stage before a quarter-pel stage; bilinear at 64/32 beside the regular
    # filter at 16/8; 8x8 blocks on 4 kept rows
    assert any(s["half_pel_mode"] == 0 and s["quarter_pel_mode"] for s in sets)
    assert any(s["use_2tap"] and s["enable_8x8_pred"] for s in sets)
    assert any(s["sub_sampling_shift"] and s["enable_8x8_pred"] for s in sets)
    assert "l8" in {c["controls"] for c in TFSP_CASES}  # the level preset 8 uses
    assert {(c["w"], c["h"]) for c in TFSP_CASES} == {(128, 128), (192, 136), (72, 40), (200, 72), (124, 66)}
    assert {len(c["refs"]) for c in TFSP_CASES} == {1, 3, 5}
    assert all(len(set(c["refs"] + [c["centre"]])) == len(c["refs"]) + 1 for c in TFSP_CASES)  # distinct pictures
    assert {c["records"] for c in TFSP_CASES} == {"me", "edges", "wrap"}
    assert all((c["seed"] is not None) == (c["records"] == "wrap") for c in TFSP_CASES)
    assert {c["kind"] for c in TFSP_CASES} == {"frac", "glide", "same", "flat", "noise"}


def test_tfsp_coverage_counts_are_all_non_zero():
    assert set(DOC["coverage"]) == set(G.COVERAGE_KEYS)
    zero = [k for k, v in DOC["coverage"].items() if not v > 0]
    assert zero == []
    assert set(DOC["coverage_per_case"]) == {c["id"] for c in TFSP_CASES}
    for k in G.COVERAGE_KEYS:
        assert sum(c.get(k, 0) for c in DOC["coverage_per_case"].values()) == DOC["coverage"][k], k


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


def case_controls(case):
    return {f: G.CONTROL_SETS[case["controls"]][f] for f in G.SUBPEL_FIELDS}


@pytest.mark.parametrize("case", TFSP_CASES, ids=lambda c: c["id"])
def test_tfsp_model_equals_fixture(svtme, gold, case):
    """The numpy model (tests/tfsp_model.py) on the oracle's planes gives every fixture as whole
    structs, and counts what the reference-side run of the generator counted."""
    pyr = {t: svtme.build_host_pyramid(f, "oracle") for t, f in G.case_frames(case).items()}
    out, cover = M.refine_window(pyr[case["centre"]], [pyr[r] for r in case["refs"]], case_controls(case),
                                 gold[case["id"] + ".rec"])
    assert_structs_equal(out, gold[case["id"] + ".out"], case["id"])
    assert {k: v for k, v in cover.items() if v} == DOC["coverage_per_case"][case["id"]]


# The random sweep (tests/tfsp_model.py: sweep_case): (seed, references or None for the seed's own draw).
# Seeds 9 and 12 draw full windows of 16 distinct references; 32 and 54 are there for the SBs that
# choose the 64x64 block after the 32x32 search, which the perturbed records seldom leave.
SWEEP = [(seed, None) for seed in list(range(24)) + [32, 54]]
_sweep_cache = {}


def sweep_expected(seed, n):
    """-> (case, the oracle's ME records, the sweep's records, the model's results, its coverage),
    computed once per process."""
    if (seed, n) not in _sweep_cache:
        case = M.sweep_case(seed, n)
        _sweep_cache[(seed, n)] = (case,) + M.sweep_model(case)
    return _sweep_cache[(seed, n)]


def test_tfsp_sweep_covers_every_branch(svtme):
    """The sweep's cases, by the model alone: together they reach every coverage count, old and
    new, every shape, content and value of the controls, and a full window."""
    cases = [sweep_expected(seed, n)[0] for seed, n in SWEEP]
    total = {k: sum(sweep_expected(seed, n)[4][k] for seed, n in SWEEP) for k in G.COVERAGE_KEYS}
    print("sweep coverage:", total)
    assert [k for k, v in total.items() if not v > 0] == []
    assert {(c["w"], c["h"]) for c in cases} == set(M.SWEEP_SHAPES)
    assert {c["kind"] for c in cases} == set(M.SWEEP_KINDS)
    assert {len(c["refs"]) for c in cases} >= {1, svtme.MAX_BATCH_JOBS}
    assert all(len(set(c["refs"] + [c["centre"]])) == len(c["refs"]) + 1 for c in cases)
    for field, values in (("half_pel_mode", range(4)), ("quarter_pel_mode", range(4)), ("eight_pel_mode", range(2)),
                          ("use_2tap", range(2)), ("sub_sampling_shift", range(2)), ("enable_8x8_pred", range(2)),
                          ("subpel_early_exit_th", M.SWEEP_EXIT_TH), ("use_pred_64x64_only_th", M.SWEEP_64_ONLY_TH),
                          ("pred_error_32x32_th", M.SWEEP_ERR_32_TH)):
        assert {c["subpel"][field] for c in cases} == set(values), field


@pytest.mark.skipif(not ref_available(), reason="oracle/_ref not built (needs the reference's sources)")
@pytest.mark.parametrize("seed,n", SWEEP, ids=[f"seed{s}" for s, _ in SWEEP])
def test_tfsp_model_equals_reference_on_sweep(svtme, seed, n):
    """The reference-backed evaluation (the reference's planes, svt_inter_predictor and variance
    kernels) on the sweep's inputs, which are no fixtures: the same structs and counts as the model."""
    case, _, recs, want, want_cover = sweep_expected(seed, n)
    pyr = {t: svtme.build_host_pyramid(f, "ref") for t, f in M.sweep_frames(case).items()}
    cover = {k: 0 for k in G.COVERAGE_KEYS}
    out = G.refine_window(pyr[case["centre"]], [pyr[r] for r in case["refs"]], case["subpel"], recs, cover)
    assert_structs_equal(want, out, f"seed {seed} controls {case['subpel']}")
    assert cover == want_cover


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
@pytest.mark.parametrize("seed,n", SWEEP, ids=[f"seed{s}" for s, _ in SWEEP])
def test_tfsp_random_sweep_vs_model(svtme, gpu, seed, n):
    """Random shapes, contents, windows and controls: the records of the GPU's own TF-ME jobs (the
    oracle's, checked here), perturbed, then svtme_tf_subpel against the numpy model as whole structs."""
    case, want_me, recs, want, _ = sweep_expected(seed, n)
    what = f"seed {seed}: {case['w']}x{case['h']} {case['kind']}, references {case['refs']}, controls {case['subpel']}"
    frames = M.sweep_frames(case)
    for t, f in frames.items():
        gpu.upload(BASE + t, f)
    try:
        layout = svtme.PackLayout(n_pus=85, max_cand=1, max_refs=1, full_records=1, sb_results=0)
        me = []
        for r in case["refs"]:
            packed = gpu.submit_packed(G.me_job(case, case["controls"], r, BASE), layout)
            me.append(np.frombuffer(packed, svtme.REF_RECORD_DTYPE))
        me = np.stack(me)
        assert svtme.compare_records(want_me.reshape(-1, 1), me.reshape(-1, 1)) == [], what
        out = gpu.tf_subpel(BASE + case["centre"], [BASE + r for r in case["refs"]], case["w"], case["h"],
                            svtme.TfSubpelControls.from_dict(case["subpel"]), M.sweep_records(case, me))
        assert_structs_equal(out, want, what)
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
