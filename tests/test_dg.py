"""The dynamic-GOP detector's early HME search (svtme_dg_detect, include/svtme.h).

Expected values are the fixtures tests/golden/dg_cases.{json,npz}: the
reference's own planes and sad_loop kernel on the windows of
tests/golden/make_golden_dg.py (a restatement of pd_process.c:409-457).
CPU tests pin the host-side pieces and the fixtures themselves (a numpy
brute-force search, regeneration where the reference harness is built); GPU
tests compare svtme_dg_detect bit-exactly against the fixtures.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from conftest import ref_available

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLD not in sys.path:
    sys.path.insert(0, GOLD)

import make_golden_dg as G  # noqa: E402

DG_CASES = json.load(open(os.path.join(GOLD, "dg_cases.json")))
BAD_PARAMETER = 0x80001005
BASE = 7000  # picture numbers of this file's uploads


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLD, "dg_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def case_by_id(name):
    return next(c for c in DG_CASES if c["id"] == name)


def metrics_rows(mets):
    return [[m.as_dict()[f] for f in G.METRIC_FIELDS] for m in mets]


# ----------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------
def test_dg_case_list_matches_generator():
    assert DG_CASES == G.case_dicts()


def test_dg_search_area_rule(svtme):
    # <= 360p 16x16, <= 480p 64x64, else 128x128 (pd_process.c:497-498)
    want = {svtme.RES_240P: 16, svtme.RES_360P: 16, svtme.RES_480P: 64, svtme.RES_720P: 128, svtme.RES_1080P: 128,
            svtme.RES_4K: 128, svtme.RES_8K: 128}
    assert len(want) == 7
    for res, sa in want.items():
        assert svtme.dg_search_area(res) == (sa, sa), res


def test_dg_struct_sizes(svtme):
    assert svtme.DG_SB_DTYPE.itemsize == 8
    assert C.sizeof(svtme.DgMetrics) == 32
    assert C.sizeof(svtme.DgPair) == 16
    assert svtme.DgMetrics.norm_dist.offset == 24 and svtme.DgMetrics.mv_in_out_count.offset == 20


@pytest.mark.parametrize("case", DG_CASES, ids=lambda c: c["id"])
def test_dg_reduce_reproduces_fixture_metrics(svtme, gold, case):
    sb, met = gold[case["id"] + ".sb"], gold[case["id"] + ".metrics"]
    assert sb.shape == (len(case["pairs"]), svtme.sb_total(case["w"], case["h"]))
    for k in range(len(case["pairs"])):
        got = metrics_rows([svtme.dg_reduce(case["w"], case["h"], sb[k])])[0]
        assert got == met[k].tolist(), (case["id"], k)


def test_dg_fixtures_cover_negative_truncation(gold):
    # a negative sum_in_vectors whose quotient is not whole: C division, not floor
    hit = False
    for case in DG_CASES:
        n = gold[case["id"] + ".sb"].shape[1]
        for m in gold[case["id"] + ".metrics"]:
            vec, in_out = int(m[3]), int(m[4])
            if vec < 0 and (vec * 100) % n:
                assert in_out == -((-vec * 100) // n)
                hit = True
    assert hit


@pytest.mark.skipif(not ref_available(), reason="oracle/_ref not built (needs the reference's sources)")
def test_dg_fixture_regenerates(gold):
    case = case_by_id("pan320_sa128")
    sb, met = G.generate_case(case)
    assert sb.tobytes() == gold[case["id"] + ".sb"].tobytes()
    assert np.array_equal(met, gold[case["id"] + ".metrics"])


def test_dg_fixture_vs_numpy_brute_force(svtme, gold):
    """An independent search over the same windows: every position's 16x16 SAD by numpy,
    first minimum in raster order, on the oracle's planes (pinned to the reference's)."""
    case = case_by_id("pan328x200_sa64")
    frames = G.case_frames(case)
    pyr = {t: svtme.build_host_pyramid(f, "oracle") for t, f in frames.items()}
    cur, ref = case["pairs"][0]
    six_c = pyr[cur].sixteenth.astype(np.int32)
    six_r = pyr[ref].sixteenth.astype(np.int32)
    pad = svtme.PAD_SIXTEENTH
    want = gold[case["id"] + ".sb"][0]
    wins = G.sb_windows(case["w"], case["h"], *case["sa"])
    assert len(wins) == len(want)
    for k, (org_x, org_y, ox, oy, sw, sh) in enumerate(wins):
        src = six_c[pad + org_y:pad + org_y + 16, pad + org_x:pad + org_x + 16]
        y0, x0 = pad + org_y + oy, pad + org_x + ox
        view = np.lib.stride_tricks.sliding_window_view(six_r[y0:y0 + sh + 15, x0:x0 + sw + 15], (16, 16))
        sad = np.abs(view - src).sum(axis=(2, 3))
        assert sad.shape == (sh, sw)
        y, x = np.unravel_index(np.argmin(sad), sad.shape)  # the first minimum in raster order
        assert (int(want["sad"][k]), int(want["mv_x"][k]), int(want["mv_y"][k])) == \
            (int(sad[y, x]), (x + ox) * 4, (y + oy) * 4), k


# ----------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------
def upload_case(gpu, case, asynchronous=False):
    frames = G.case_frames(case)
    for t, f in frames.items():
        (gpu.upload_async if asynchronous else gpu.upload)(BASE + t, f)
    return frames


def release_case(gpu, frames):
    for t in frames:
        gpu.release(BASE + t)


def assert_equal_to_fixture(case, gold, mets, sb, pairs=None):
    ks = range(len(case["pairs"])) if pairs is None else pairs
    want_sb, want_m = gold[case["id"] + ".sb"], gold[case["id"] + ".metrics"]
    for i, k in enumerate(ks):
        if sb is not None:
            for f in ("sad", "mv_x", "mv_y"):
                bad = np.flatnonzero(sb[i][f] != want_sb[k][f])
                assert bad.size == 0, (case["id"], k, f, int(bad[0]), sb[i][bad[0]], want_sb[k][bad[0]])
        assert metrics_rows([mets[i]])[0] == want_m[k].tolist(), (case["id"], k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", DG_CASES, ids=lambda c: c["id"])
def test_dg_vs_reference_golden(svtme, gpu, gold, case):
    frames = upload_case(gpu, case)
    try:
        pairs = [(BASE + c, BASE + r) for c, r in case["pairs"]]
        mets, sb = gpu.dg_detect(pairs, *case["sa"])
        assert sb.shape == (len(pairs), svtme.sb_total(case["w"], case["h"]))
        assert_equal_to_fixture(case, gold, mets, sb)
        mets2, none = gpu.dg_detect(pairs, *case["sa"], with_sb=False)
        assert none is None
        assert metrics_rows(mets2) == metrics_rows(mets)
    finally:
        release_case(gpu, frames)


@pytest.mark.gpu
def test_dg_batch_equals_singles(svtme, gpu, gold):
    case = case_by_id("triple832")
    frames = upload_case(gpu, case)
    try:
        pairs = [(BASE + c, BASE + r) for c, r in case["pairs"]]
        mets, sb = gpu.dg_detect(pairs, *case["sa"])
        for k, p in enumerate(pairs):
            m1, sb1 = gpu.dg_detect([p], *case["sa"])
            assert sb1.tobytes() == sb[k:k + 1].tobytes()
            assert metrics_rows(m1) == metrics_rows(mets[k:k + 1])
            assert_equal_to_fixture(case, gold, m1, sb1, pairs=[k])
    finally:
        release_case(gpu, frames)


@pytest.mark.gpu
def test_dg_after_async_upload(svtme, gpu, gold):
    case = case_by_id("pan328x200_sa64")
    frames = upload_case(gpu, case, asynchronous=True)  # no sync: the call waits for both uploads on the GPU
    pairs = [(BASE + c, BASE + r) for c, r in case["pairs"]]
    mets, sb = gpu.dg_detect(pairs, *case["sa"])
    for t in frames:
        assert gpu.lib.svtme_picture_release(gpu.ctx, BASE + t) == 0
    gpu.sync()
    assert_equal_to_fixture(case, gold, mets, sb)


@pytest.mark.gpu
def test_dg_leaves_me_jobs_unchanged(svtme, gpu):
    w, h = 320, 192
    syn = svtme.Synth(w, h)
    frames = {t: syn.frame(t) for t in (6, 7, 8, 9)}
    for t, f in frames.items():
        gpu.upload(BASE + t, f)
    try:
        ctrl = svtme.derive_controls(8, 35, svtme.input_resolution_of(w, h), 1)
        job = svtme.make_job(w, h, ctrl, BASE + 8, (BASE + 7, BASE + 6), (BASE + 9,), temporal_layer_index=1,
                             ref_count_used=(2, 1))
        recs0, sbr0 = gpu.submit(job)
        mets, sb = gpu.dg_detect([(BASE + 8, BASE + 6)], 128, 128)
        recs1, sbr1 = gpu.submit(job)
        assert svtme.compare_records(recs0, recs1, sbr0, sbr1) == []
        assert svtme.records_checksum(recs0, sbr0) == svtme.records_checksum(recs1, sbr1)
        mets2, sb2 = gpu.dg_detect([(BASE + 8, BASE + 6)], 128, 128)
        assert sb2.tobytes() == sb.tobytes() and metrics_rows(mets2) == metrics_rows(mets)
    finally:
        for t in frames:
            gpu.release(BASE + t)


@pytest.mark.gpu
def test_dg_bad_arguments(svtme, gpu):
    small = svtme.test_frames("pan", 320, 192, (6, 8))
    big = svtme.test_frames("pan", 384, 192, (6, 8))
    gpu.upload(BASE + 6, small[6])
    gpu.upload(BASE + 8, small[8])
    gpu.upload(BASE + 106, big[6])
    gpu.upload(BASE + 108, big[8])
    lib, ctx = gpu.lib, gpu.ctx
    sbs = svtme.sb_total(384, 192)
    sentinel = 0x5A

    def call(pairs, sa_w=64, sa_h=64, null=None, n=None):
        """-> the status; the outputs must stay untouched (nothing launched, nothing copied)."""
        arr = (svtme.DgPair * max(len(pairs), 1))(*[svtme.DgPair(c, r) for c, r in pairs])
        met = (svtme.DgMetrics * (svtme.DG_MAX_PAIRS * 2))()
        C.memset(met, sentinel, C.sizeof(met))
        sb = np.full(svtme.DG_MAX_PAIRS * 2 * sbs * 8, sentinel, np.uint8)
        st = lib.svtme_dg_detect(None if null == "ctx" else ctx, None if null == "pairs" else arr,
                                 len(pairs) if n is None else n, sa_w, sa_h, None if null == "metrics" else met,
                                 sb.ctypes.data)
        assert bytes(met) == bytes([sentinel]) * C.sizeof(met)
        assert (sb == sentinel).all()
        if st:
            assert lib.svtme_last_error().decode() != ""
        return st & 0xFFFFFFFF

    ok = [(BASE + 8, BASE + 6)]
    try:
        for null in ("ctx", "pairs", "metrics"):
            assert call(ok, null=null) == BAD_PARAMETER, null
        assert call(ok, n=0) == BAD_PARAMETER
        assert call(ok * (svtme.DG_MAX_PAIRS + 1)) == BAD_PARAMETER
        for sa in ((0, 64), (64, 0), (129, 64), (64, 129)):  # 129 rounds up to 136; 121 (below) to 128
            assert call(ok, *sa) == BAD_PARAMETER, sa
        assert call([(BASE + 8, BASE + 999)]) == BAD_PARAMETER  # not resident
        assert call([(BASE + 999, BASE + 6)]) == BAD_PARAMETER
        assert call([(BASE + 8, BASE + 106)]) == BAD_PARAMETER  # sizes differ within a pair
        assert call(ok + [(BASE + 108, BASE + 106)]) == BAD_PARAMETER  # pairs of different sizes
        # and the valid forms of the same calls succeed
        mets, sb = gpu.dg_detect(ok, 121, 64)
        mets8, sb8 = gpu.dg_detect(ok, 128, 64)
        assert sb.tobytes() == sb8.tobytes() and metrics_rows(mets) == metrics_rows(mets8)
        gpu.dg_detect(ok * svtme.DG_MAX_PAIRS, 64, 64, with_sb=False)
    finally:
        for t in (6, 8, 106, 108):
            gpu.release(BASE + t)
