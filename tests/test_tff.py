"""Temporal filtering's luma prediction and weighting (svtme_tf_filter, include/svtme.h).

Expected values are the fixtures tests/golden/tff_cases.{json,npz}: the reference's
own planes, svt_inter_predictor, variance kernels and filter functions under the
glue restated in tests/golden/make_golden_tff.py. Beside them stands a model of the
whole stage in numpy and Python integers (tests/tff_model.py), which needs nothing
from the reference. CPU tests pin the ABI, the parameter checks that need no context,
the fixtures themselves and the model to the fixtures; GPU tests compare
svtme_tf_filter bit-exactly against the fixtures and, on a sweep whose inputs are the
GPU's own TF-ME and sub-pel results, against the model.
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
import make_golden_tfsp as G  # noqa: E402
import tff_model as M  # noqa: E402

DOC = json.load(open(os.path.join(GOLD, "tff_cases.json")))
TFF_CASES = DOC["cases"]
BAD_PARAMETER = 0x80001005
BASE = 11000  # picture numbers of this file's uploads


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLD, "tff_cases.npz")) as z:
        out = {k: z[k] for k in z.files}
    with np.load(os.path.join(GOLD, "tfsp_cases.npz")) as z:
        for case in TFF_CASES:
            if case["subpel"] == "tfsp":
                out[case["id"] + ".subpel"] = z[case["id"] + ".out"]
    return out


def case_by_id(name):
    return next(c for c in TFF_CASES if c["id"] == name)


_pyramids = {}


def oracle_pyramids(svtme, case):
    """{picture: HostPyramid} of a case on the CPU oracle's planes, built once per process."""
    if case["id"] not in _pyramids:
        _pyramids[case["id"]] = {t: svtme.build_host_pyramid(f, "oracle") for t, f in G.case_frames(case).items()}
    return _pyramids[case["id"]]


# ----------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------
def test_tff_symbol_exported(svtme):
    assert hasattr(svtme.load_product(), "svtme_tf_filter")


_ABI_PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "svtme.h"
#define O(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
    printf("sizeof svtme_tf_filter_controls %zu\n", sizeof(svtme_tf_filter_controls));
    O(svtme_tf_filter_controls, tf_decay_factor_fp16); O(svtme_tf_filter_controls, tf_mv_dist_th);
    O(svtme_tf_filter_controls, sub_sampling_shift); O(svtme_tf_filter_controls, pad);
    return 0;
}
"""


def test_tff_struct_sizes_and_offsets_equal_the_headers(svtme, tmp_path):
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text(_ABI_PROGRAM)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        key, val = line.rsplit(" ", 1)
        got[key] = int(val)
    ctl = svtme.TfFilterControls
    assert got["sizeof svtme_tf_filter_controls"] == C.sizeof(ctl) == 8
    for name, _ in ctl._fields_:
        assert got["svtme_tf_filter_controls." + name] == getattr(ctl, name).offset, name
    assert len(ctl._fields_) == 4


def _controls(svtme, **over):
    return svtme.TfFilterControls.from_dict(dict({"tf_decay_factor_fp16": 2_000_000, "tf_mv_dist_th": 64,
                                                  "sub_sampling_shift": 1}, **over))


def _call(svtme, lib, ctx, refs, n=None, ctl=None, null=None, w=128, h=128, centre=BASE + 8, stride=None, branch=0,
          err32=True):
    """-> the status of svtme_tf_filter; on an error `out` and `err32_out` must stay untouched."""
    ctl = ctl if ctl is not None else _controls(svtme)
    sbs = svtme.sb_total(svtme.align8(w), svtme.align8(h))
    slots = max(len(refs), svtme.MAX_BATCH_JOBS + 1)
    arr = (C.c_uint64 * slots)(*refs)
    sub = np.zeros((slots, sbs), svtme.TF_SUBPEL_SB_DTYPE)
    sub["branch"][min(len(refs), slots) - 1, sbs - 1] = branch  # the last struct the call reads
    stride = w if stride is None else stride
    out = np.full(h * max(stride, w), 0x5A, np.uint8)
    e32 = np.full(slots * sbs * 4, 0x5A5A5A5A, np.uint32)
    st = lib.svtme_tf_filter(None if null == "ctx" else ctx, centre, None if null == "refs" else arr,
                             len(refs) if n is None else n, w, h, None if null == "controls" else C.byref(ctl),
                             None if null == "subpel" else sub.ctypes.data, None if null == "out" else out.ctypes.data,
                             stride, e32.ctypes.data if err32 else None)
    if st:
        assert (out == 0x5A).all() and (e32 == 0x5A5A5A5A).all()
        assert lib.svtme_last_error().decode() != ""
    return st & 0xFFFFFFFF


def _bad_calls(svtme):
    """(what, keyword arguments of _call) of the argument errors that need no resident picture."""
    ok = [BASE + 7]
    for null in ("ctx", "refs", "controls", "subpel", "out"):
        yield "null " + null, dict(refs=ok, null=null)
    yield "n 0", dict(refs=ok, n=0)
    yield "n 17", dict(refs=ok * (svtme.MAX_BATCH_JOBS + 1))
    yield "out_stride under the width", dict(refs=ok, stride=127)
    yield "tf_mv_dist_th 32768", dict(refs=ok, ctl=_controls(svtme, tf_mv_dist_th=32768))
    yield "sub_sampling_shift 2", dict(refs=ok, ctl=_controls(svtme, sub_sampling_shift=2))
    yield "branch 3", dict(refs=ok, branch=3)
    yield "branch 3 in the last of 16", dict(refs=ok * svtme.MAX_BATCH_JOBS, branch=3)


def test_tff_bad_parameters_without_a_device(svtme):
    """The checks that need no context run before the context is touched: a block of zero bytes
    stands in for it (no device, no context can be created here)."""
    lib = svtme.load_product()
    fake = C.create_string_buffer(64)
    ctx = C.cast(fake, C.c_void_p)
    for what, kw in _bad_calls(svtme):
        assert _call(svtme, lib, ctx, **kw) == BAD_PARAMETER, what
    assert fake.raw == bytes(64)


def test_tff_case_list_matches_generator():
    assert TFF_CASES == GF.case_dicts()
    tfsp = [c["id"] for c in TFF_CASES if c["subpel"] == "tfsp"]
    assert tfsp == [c["id"] for c in G.case_dicts()]  # every TFSP case
    own = [c for c in TFF_CASES if c["subpel"] == "random"]
    assert {(c["w"], c["h"]) for c in own} == {(64, 64), (72, 40), (128, 128)}
    ctl = [c["controls"] for c in TFF_CASES]
    assert {c["tf_decay_factor_fp16"] for c in ctl} >= {0, 1023, 2_000_000, 0x7FFFFFFF}
    assert {c["tf_mv_dist_th"] for c in ctl} == {0, 64, 450, 32767}
    assert {c["sub_sampling_shift"] for c in ctl} == {0, 1}


def test_tff_coverage_counts_are_all_non_zero():
    assert set(DOC["coverage"]) == set(GF.COVERAGE_KEYS)
    assert [k for k, v in DOC["coverage"].items() if not v > 0] == []
    assert set(DOC["coverage_per_case"]) == {c["id"] for c in TFF_CASES}
    for k in GF.COVERAGE_KEYS:
        assert sum(c.get(k, 0) for c in DOC["coverage_per_case"].values()) == DOC["coverage"][k], k
    wc = DOC["weights_coverage"]
    assert len(wc["exp_index"]) == 113 and len(wc["sqrt_log2_half_4_15"]) == 12 and len(wc["sqrt_base_4_15"]) == 12
    assert all(v > 0 for counts in wc.values() for v in counts)  # every index 0..112, every sqrt_fast branch


def test_tff_fixture_shapes(svtme, gold):
    want = [c["id"] + s for c in TFF_CASES for s in (".plane", ".err32", ".weights", ".subpel")]
    assert sorted(gold) == sorted(want + ["weights.in", "weights.out"])
    for case in TFF_CASES:
        W, H = svtme.align8(case["w"]), svtme.align8(case["h"])
        n, sbs = len(case["refs"]), svtme.sb_total(W, H)
        name = case["id"]
        assert gold[name + ".plane"].shape == (H, W) and gold[name + ".plane"].dtype == np.uint8
        assert gold[name + ".err32"].shape == (n, sbs, 4) and gold[name + ".err32"].dtype == np.uint32
        assert gold[name + ".weights"].shape == (n, sbs, 16) and gold[name + ".weights"].max() <= 1000
        assert gold[name + ".subpel"].shape == (n, sbs) and gold[name + ".subpel"].dtype == svtme.TF_SUBPEL_SB_DTYPE
        if case["subpel"] == "random":
            assert gold[name + ".subpel"].tobytes() == GF.random_subpel(case).tobytes()
    assert gold["weights.in"].shape == (400, GF.WEIGHT_COLS) and gold["weights.out"].shape == (400, 4)
    assert np.array_equal(gold["weights.in"], GF.weight_tuples())
    assert DOC["weights_coverage"] == M.weights_coverage(gold["weights.in"])


def test_tff_tables_from_their_formulas():
    """Landmarks of the two tables the model computes: exp(-x / 16) and sqrt in 16 fractional bits."""
    assert M.EXP_TAB[0] == 65536 and M.EXP_TAB[16] == 24109 and M.EXP_TAB[112] == 59  # 65536 / e, 65536 / e^7
    assert len(M.EXP_TAB) == 113 and all(a > b for a, b in zip(M.EXP_TAB, M.EXP_TAB[1:]))
    assert M.SQRT_TAB[:5] == [0, 65536, 92681, 113511, 131072] and M.SQRT_TAB[9] == 3 << 16


def test_tff_model_equals_weights_fixture(gold):
    """Every tuple of the fixture "weights": the model's weight is the reference's, which proves each
    entry of both tables (the coverage counts say that each is reached)."""
    got = M.model_weights(gold["weights.in"])
    bad = np.argwhere(got != gold["weights.out"])
    assert bad.size == 0, (bad[0], gold["weights.in"][bad[0][0]], got[bad[0][0]], gold["weights.out"][bad[0][0]])


@pytest.mark.parametrize("case", TFF_CASES, ids=lambda c: c["id"])
def test_tff_model_equals_fixture(svtme, gold, case):
    """The model on the oracle's planes gives every fixture: plane, err32 and weights, and counts
    what the reference-side run of the generator counted."""
    pyr = oracle_pyramids(svtme, case)
    plane, err32, weights, cover = M.filter_window(pyr[case["centre"]], [pyr[r] for r in case["refs"]],
                                                   case["controls"], gold[case["id"] + ".subpel"])
    assert np.array_equal(err32, gold[case["id"] + ".err32"])
    assert np.array_equal(weights, gold[case["id"] + ".weights"])
    assert np.array_equal(plane, gold[case["id"] + ".plane"])
    assert {k: v for k, v in cover.items() if v} == DOC["coverage_per_case"][case["id"]]


@pytest.mark.skipif(not (ref_available() and GF.reference_headers()),
                    reason="oracle/_ref not built or the reference's headers absent (the offsetof probe needs them)")
def test_tff_fixture_regenerates(gold):
    case = case_by_id("own64_rand")
    pyr, sub = GF.case_inputs(case)
    cover = {k: 0 for k in GF.COVERAGE_KEYS}
    plane, err32, weights = GF.filter_window(pyr[case["centre"]], [pyr[r] for r in case["refs"]], case["controls"],
                                             sub, GF.RefArith(), cover)
    assert plane.tobytes() == gold[case["id"] + ".plane"].tobytes()
    assert err32.tobytes() == gold[case["id"] + ".err32"].tobytes()
    assert weights.tobytes() == gold[case["id"] + ".weights"].tobytes()
    assert np.array_equal(GF.reference_weights(gold["weights.in"][:120]), gold["weights.out"][:120])


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


def run_case(svtme, gpu, case, subpel, refs=None, controls=None, **kw):
    refs = case["refs"] if refs is None else refs
    W, H = svtme.align8(case["w"]), svtme.align8(case["h"])
    ctl = svtme.TfFilterControls.from_dict(case["controls"] if controls is None else controls)
    return gpu.tf_filter(BASE + case["centre"], [BASE + r for r in refs], W, H, ctl, subpel, **kw)


def assert_planes_equal(got, want, what):
    if not np.array_equal(got, want):
        y, x = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}: {int((got != want).sum())} pixels differ, first at x {x} y {y}: "
                             f"{got[y, x]} for {want[y, x]}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", TFF_CASES, ids=lambda c: c["id"])
def test_tff_vs_reference_golden(svtme, gpu, gold, case):
    """Plane and err32 bit-exact; the fixture's weights through the plane they give with the model's
    predictions, which must be the GPU's plane too."""
    name = case["id"]
    frames = upload_case(gpu, case)
    try:
        plane, err32 = run_case(svtme, gpu, case, gold[name + ".subpel"])
    finally:
        release_case(gpu, frames)
    assert np.array_equal(err32, gold[name + ".err32"]), name
    assert_planes_equal(plane, gold[name + ".plane"], name)
    pyr = oracle_pyramids(svtme, case)
    tiles = M.window_tiles(pyr[case["centre"]], [pyr[r] for r in case["refs"]], gold[name + ".subpel"])
    assert_planes_equal(plane, M.plane_from_weights(pyr[case["centre"]], tiles, gold[name + ".weights"]),
                        name + " from the fixture's weights")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", M.SWEEP_SEEDS, ids=[f"seed{s}" for s in M.SWEEP_SEEDS])
def test_tff_random_sweep_vs_model(svtme, gpu, seed):
    """Random shapes, contents, windows and controls: the GPU's own TF-ME jobs and sub-pel refinement
    feed svtme_tf_filter, as they are and perturbed; both against the model."""
    case = M.sweep_case(seed)
    what = f"seed {seed}: {case['w']}x{case['h']} {case['kind']}, references {case['refs']}, filter {case['filter']}"
    frames = G.case_frames(case)
    refs = [BASE + r for r in case["refs"]]
    W, H = svtme.align8(case["w"]), svtme.align8(case["h"])
    for t, f in frames.items():
        gpu.upload(BASE + t, f)
    try:
        layout = svtme.PackLayout(n_pus=85, max_cand=1, max_refs=1, full_records=1, sb_results=0)
        me = np.stack([np.frombuffer(gpu.submit_packed(G.me_job(case, case["controls"], r, BASE), layout),
                                     svtme.REF_RECORD_DTYPE) for r in case["refs"]])
        sub = gpu.tf_subpel(BASE + case["centre"], refs, case["w"], case["h"],
                            svtme.TfSubpelControls.from_dict(case["subpel"]), me)
        inputs = [("chain", sub), ("perturbed", M.perturb_subpel(sub, 7000 + seed))]
        got = [gpu.tf_filter(BASE + case["centre"], refs, W, H, svtme.TfFilterControls.from_dict(case["filter"]), s)
               for _, s in inputs]
    finally:
        release_case(gpu, frames)
    pyr = {t: svtme.build_host_pyramid(f, "oracle") for t, f in frames.items()}
    for (label, s), (plane, err32) in zip(inputs, got):
        want_plane, want_err32, _, _ = M.filter_window(pyr[case["centre"]], [pyr[r] for r in case["refs"]],
                                                       case["filter"], s)
        assert np.array_equal(err32, want_err32), (what, label)
        assert_planes_equal(plane, want_plane, f"{what} ({label})")


@pytest.mark.gpu
def test_tff_window_equals_accumulated_singles(svtme, gpu, gold):
    """A window of 3: each reference alone gives the model's single-reference plane, and the window
    gives the accumulation of those three calls' weights and predictions, in any order of the references."""
    case = case_by_id("own128_rand")
    controls = dict(case["controls"], tf_decay_factor_fp16=2_000_000)
    sub = gold[case["id"] + ".subpel"]
    pyr = oracle_pyramids(svtme, case)
    cen, refs = pyr[case["centre"]], [pyr[r] for r in case["refs"]]
    tiles = M.window_tiles(cen, refs, sub)
    frames = upload_case(gpu, case)
    try:
        weights = []
        for k, r in enumerate(case["refs"]):
            one, _ = run_case(svtme, gpu, case, sub[k:k + 1], refs=[r], controls=controls)
            want, _, w, _ = M.filter_window(cen, refs[k:k + 1], controls, sub[k:k + 1])
            assert_planes_equal(one, want, f"reference {k} alone")
            weights.append(w[0])
        weights = np.stack(weights)
        assert 0 < np.count_nonzero(weights) and len(np.unique(weights)) > 4  # the weights matter here
        want = M.plane_from_weights(cen, tiles, weights)
        for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
            got, _ = run_case(svtme, gpu, case, sub[list(order)], refs=[case["refs"][k] for k in order],
                              controls=controls)
            assert_planes_equal(got, want, f"order {order}")
    finally:
        release_case(gpu, frames)


@pytest.mark.gpu
def test_tff_stride_null_err32_and_the_centre_stays(svtme, gpu, gold):
    case = case_by_id("frac72_h0q2_wrap")  # 72 x 40: the second SB column holds 8 pixels
    name = case["id"]
    frames = upload_case(gpu, case)
    W, H = svtme.align8(case["w"]), svtme.align8(case["h"])
    try:
        before = gpu.download(BASE + case["centre"], 0)
        plane, err32 = run_case(svtme, gpu, case, gold[name + ".subpel"], with_err32=False)
        assert err32 is None
        assert_planes_equal(plane, gold[name + ".plane"], "err32_out NULL")
        # out_stride > width: the slack bytes stay as they were
        lib, n, sbs = gpu.lib, len(case["refs"]), svtme.sb_total(W, H)
        stride = W + 13
        buf = np.full((H, stride), 0xA5, np.uint8)
        arr = (C.c_uint64 * n)(*[BASE + r for r in case["refs"]])
        sub = np.ascontiguousarray(gold[name + ".subpel"])
        ctl = svtme.TfFilterControls.from_dict(case["controls"])
        assert lib.svtme_tf_filter(gpu.ctx, BASE + case["centre"], arr, n, W, H, C.byref(ctl), sub.ctypes.data,
                                   buf.ctypes.data, stride, None) == 0
        assert_planes_equal(buf[:, :W], gold[name + ".plane"], "out_stride > width")
        assert (buf[:, W:] == 0xA5).all()
        assert sbs == 2
        after = gpu.download(BASE + case["centre"], 0)
        assert np.array_equal(before, after)  # the resident centre picture is not modified
    finally:
        release_case(gpu, frames)


@pytest.mark.gpu
def test_tff_bad_parameters_with_a_context(svtme, gpu):
    small = G.tfsp_content.fractional_frames(128, 128, (7, 8))
    big = G.tfsp_content.fractional_frames(192, 136, (7,))
    gpu.upload(BASE + 7, small[7])
    gpu.upload(BASE + 8, small[8])
    gpu.upload(BASE + 107, big[7])
    lib, ctx = gpu.lib, gpu.ctx
    ok = [BASE + 7]
    try:
        for what, kw in _bad_calls(svtme):
            assert _call(svtme, lib, ctx, **kw) == BAD_PARAMETER, what
        assert _call(svtme, lib, ctx, [BASE + 999]) == BAD_PARAMETER  # a reference that is not resident
        assert _call(svtme, lib, ctx, ok, centre=BASE + 999) == BAD_PARAMETER  # the centre is not
        assert _call(svtme, lib, ctx, [BASE + 7, BASE + 107]) == BAD_PARAMETER  # a reference of another size
        assert _call(svtme, lib, ctx, ok, w=192, h=136) == BAD_PARAMETER  # the window's size is not the pictures'
        # and the valid forms of the same calls succeed
        assert _call(svtme, lib, ctx, ok) == 0
        assert _call(svtme, lib, ctx, ok, stride=200, err32=False) == 0
        assert _call(svtme, lib, ctx, ok * svtme.MAX_BATCH_JOBS, branch=2) == 0
        assert _call(svtme, lib, ctx, ok, ctl=_controls(svtme, tf_mv_dist_th=32767, tf_decay_factor_fp16=0xFFFFFFFF)) == 0
    finally:
        for t in (7, 8, 107):
            gpu.release(BASE + t)
