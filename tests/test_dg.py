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


# ============================================================================
# The kernel against an independent model (tests/dg_model.py) away from the fixture shapes
# ============================================================================
import functools  # noqa: E402
import itertools  # noqa: E402

import dg_model as DM  # noqa: E402
import pyramid_model as PM  # noqa: E402

MODEL = DM.DgModel()
SWEEP_SIZES = [(8, 8), (64, 64), (136, 72), (121, 67), (200, 136)]
BIG = (576, 520)  # the smallest picture class in which an interior SB gets the whole 128 x 128 window
SWEEP_AREAS = [(8, 8), (16, 16), (20, 12), (64, 64), (128, 128), (128, 1), (8, 121), (40, 7)]
CONTENTS = ("ramp++", "ramp+-", "ramp-+", "ramp--", "noise", "same", "sat", "flat", "tile", "tile_skew", "thr")
SWEEP_SEED, SWEEP_DRAWS = 4242, 118  # the coverage test passes from 19 draws on; 120 detector calls


def content(kind: str, w: int, h: int, seed: int = 0):
    """-> (cur, ref), (h, w) uint8 each. Values are constant over 4x4 blocks where the sixteenth plane is
    to hold chosen values exactly (the 2x2 means of equal samples are the samples)."""
    rng = np.random.default_rng([w, h, seed, CONTENTS.index(kind)])
    X, Y = np.meshgrid(np.arange(w) // 4, np.arange(h) // 4)
    if kind.startswith("ramp"):
        # flat zero against a ramp of 3 per sixteenth sample: the SAD is least in one corner of every window
        gx = X if kind[4] == "+" else X.max() - X
        gy = Y if kind[5] == "+" else Y.max() - Y
        ref = 3 * (gx + gy)
        assert ref.max() <= 255
        return np.zeros((h, w), np.uint8), ref.astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "same":
        cur = rng.integers(0, 256, (h, w), dtype=np.uint8)
        return cur, cur.copy()
    if kind == "sat":
        return np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    if kind == "flat":
        return np.full((h, w), 128, np.uint8), np.full((h, w), 128, np.uint8)
    if kind in ("tile", "tile_skew"):
        # a sixteenth-resolution tile repeated: equal minima a chosen number of rows and columns apart;
        # skewed, row y of the tile is row 0 rotated by 5 y, so the minima of later rows lie in earlier columns
        if kind == "tile":
            T = rng.integers(0, 256, (9, 12), dtype=np.uint8)
        else:
            row = rng.integers(0, 256, 16, dtype=np.uint8)
            T = np.stack([np.roll(row, -5 * y) for y in range(16)])
        six = np.tile(T, (h // 4 // T.shape[0] + 2, w // 4 // T.shape[1] + 2))
        pic = np.kron(six, np.ones((4, 4), np.uint8))[:h, :w]
        return pic, pic.copy()
    if kind == "thr":
        # SADs of exactly 16 * 16 * 30 and, in the SB whose block holds the one sample at 31, one more
        cur = np.full((h, w), 30, np.uint8)
        cur[20:24, 20:24] = 31
        return cur, np.zeros((h, w), np.uint8)
    raise ValueError(kind)


def sweep_list(draws: int):
    """(size, area, content kind): two calls at BIG, then the first `draws` of a seeded shuffle of
    SWEEP_SIZES x SWEEP_AREAS x CONTENTS."""
    rng = np.random.default_rng(SWEEP_SEED)
    every = list(itertools.product(SWEEP_SIZES, SWEEP_AREAS, CONTENTS))
    return [(BIG, (128, 128), "noise"), (BIG, (128, 128), "tile_skew")] + \
        [every[i] for i in rng.permutation(len(every))[:draws]]


@functools.lru_cache(maxsize=None)
def expected(size, area, kind):
    """The model's (per-SB results, metrics, per-SB events) of one sweep entry; computed once."""
    cur, ref = content(kind, *size)
    events = []
    sb, met = MODEL.detect(cur, ref, *area, events=events)
    sb.setflags(write=False)
    return sb, tuple(met), tuple(events)


def coverage_items(entries) -> dict:
    """{item: reached}: conditions on the inputs, from the model alone."""
    ev = [e for entry in entries for e in expected(*entry)[2]]
    mets = [expected(*entry)[1] for entry in entries]

    def some(f):
        return any(f(e) for e in ev)

    got = {
        "winner at (0, 0)": some(lambda e: e["win_x"] == 0 and e["win_y"] == 0 and e["n_pos"] > 1),
        "winner in the last column": some(lambda e: e["win_x"] == e["sw"] - 1 and e["sw"] > 1),
        "winner in the last row": some(lambda e: e["win_y"] == e["sh"] - 1 and e["sh"] > 1),
        "winner at (sw - 1, sh - 1)": some(lambda e: e["win_x"] == e["sw"] - 1 and e["win_y"] == e["sh"] - 1 and
                                           e["sw"] > 1 and e["sh"] > 1),
        "minima 8 or more rows apart": some(lambda e: 2 <= e["n_min"] < e["n_pos"] and e["min_row_span"] >= 8),
        "minima 4 or more columns apart, the earlier row in the later column":
            some(lambda e: e["n_min"] < e["n_pos"] and e["min_skew"]),
        "every position ties": some(lambda e: e["n_min"] == e["n_pos"] and e["n_pos"] > 1),
        "sw of 8 that is no multiple of 16": some(lambda e: e["sw"] % 8 == 0 and e["sw"] % 16 != 0),
        "sh of 1": some(lambda e: e["sh"] == 1),
        "sh no multiple of 8": some(lambda e: e["sh"] % 8 != 0 and e["sh"] > 8),
        "sh of 128": some(lambda e: e["sh"] == 128),
        "x0 & 3 of 0": some(lambda e: e["x0_and_3"] == 0),
        "x0 & 3 of 1": some(lambda e: e["x0_and_3"] == 1),
        "clamped at both sides": some(lambda e: e["clamped"][0] and e["clamped"][1]),
        "clamped above and below": some(lambda e: e["clamped"][2] and e["clamped"][3]),
        "negative sum_in_vectors": any(m[3] < 0 for m in mets),
    }
    for sw in (6, 8, 16, 24, 128):
        got[f"sw of {sw}"] = some(lambda e: e["sw"] == sw)
    for k, side in enumerate(("left", "right", "top", "bottom")):
        got[f"clamped at the {side}"] = some(lambda e: e["clamped"][k])
    for sad in (0, 65280, DM.CPLX_TH, DM.CPLX_TH + 1):
        got[f"SAD of {sad}"] = some(lambda e: e["min_sad"] == sad)
    for axis in ("mv_x", "mv_y"):
        got[f"negative {axis}"] = some(lambda e: e[axis] < 0)
        got[f"zero {axis}"] = some(lambda e: e[axis] == 0)
        got[f"positive {axis}"] = some(lambda e: e[axis] > 0)
    return got


SWEEP = sweep_list(SWEEP_DRAWS)


def entry_id(entry):
    (w, h), (sa_w, sa_h), kind = entry
    return f"{w}x{h}-sa{sa_w}x{sa_h}-{kind}"


# ----------------------------------------------------------------------------
# CPU: the model against the fixtures, the generator and svtme_dg_reduce; what the sweep reaches
# ----------------------------------------------------------------------------
def test_dg_model_is_a_second_restatement():
    src = open(DM.__file__).read()
    assert "import make_golden_dg" not in src and "import svtme" not in src and DM.METRIC_FIELDS == G.METRIC_FIELDS
    assert DM.SB_DTYPE == G.S.DG_SB_DTYPE


@pytest.mark.parametrize("case", DG_CASES, ids=lambda c: c["id"])
def test_dg_model_equals_fixture(gold, case):
    frames = G.case_frames(case)
    for k, (cur, ref) in enumerate(case["pairs"]):
        sb, met = MODEL.detect(frames[cur], frames[ref], *case["sa"])
        want = gold[case["id"] + ".sb"][k]
        for f in ("sad", "mv_x", "mv_y"):
            bad = np.flatnonzero(sb[f] != want[f])
            assert bad.size == 0, (case["id"], k, f, int(bad[0]), sb[bad[0]], want[bad[0]])
        assert met == gold[case["id"] + ".metrics"][k].tolist(), (case["id"], k)


def test_dg_model_windows_equal_generator():
    for (w, h) in SWEEP_SIZES + [BIG]:
        for sa in SWEEP_AREAS:
            assert [win[:6] for win in MODEL.sb_windows(w, h, *sa)] == G.sb_windows(w, h, *sa), (w, h, sa)


def test_dg_reduce_equals_model_on_random_arrays(svtme):
    """svtme_dg_reduce (product host code) against the model's metrics. perc_active and perc_cplx are
    count * 100 / n with count <= n, at most 100: the uint8_t narrowing never changes them, so no input
    can need the & 0xFF; the arrays reach 100 instead."""
    rng = np.random.default_rng(99)
    hit = set()
    for wb, hb in ((1, 1), (1, 2), (2, 1), (3, 2), (4, 4), (9, 9)):
        n = wb * hb
        for rep in range(12):
            w, h = 64 * wb - int(rng.integers(0, 56)), 64 * hb - int(rng.integers(0, 56))
            sb = np.zeros(n, svtme.DG_SB_DTYPE)
            sb["sad"] = rng.choice([0, DM.CPLX_TH, DM.CPLX_TH + 1, 65280, int(rng.integers(0, 65281))], n)
            sb["mv_x"] = rng.integers(-128, 128, n) * 4 * rng.integers(0, 2, n)
            sb["mv_y"] = rng.integers(-128, 128, n) * 4 * rng.integers(0, 2, n)
            if rep == 0:  # every vector points inwards
                bx, by = np.arange(n) % wb, np.arange(n) // wb
                sb["mv_x"] = np.where(bx < wb // 2, 4, -4)
                sb["mv_y"] = np.where(by < hb // 2, 8, -8)
            if rep == 1:  # one inward vector
                sb["mv_x"], sb["mv_y"] = 0, 0
                sb["mv_x"][0] = 4
            want = MODEL.metrics(w, h, sb)
            assert metrics_rows([svtme.dg_reduce(w, h, sb)])[0] == want, (wb, hb, rep, sb)
            hit |= {("sad", int(s)) for s in sb["sad"] if s in (DM.CPLX_TH, DM.CPLX_TH + 1)}
            if want[3] < 0 and (want[3] * 100) % n:
                hit.add("negative, not whole")
                assert want[4] == -((-want[3] * 100) // n) != (want[3] * 100) // n
            if want[6] == 100:
                hit.add("all active")
    assert hit == {("sad", DM.CPLX_TH), ("sad", DM.CPLX_TH + 1), "negative, not whole", "all active"}


def test_dg_sweep_coverage():
    assert len(SWEEP) == len(set(SWEEP)) <= 150 and sum(e[0] == BIG for e in SWEEP) <= 2
    assert {e[0] for e in SWEEP} == set(SWEEP_SIZES + [BIG]) and {e[1] for e in SWEEP} == set(SWEEP_AREAS)
    assert {e[2] for e in SWEEP} == set(CONTENTS)
    missing = [k for k, v in coverage_items(SWEEP).items() if not v]
    assert not missing, missing


PYRAMID_VARIANTS = {"round with +1": dict(rnd=1), "round with +0": dict(rnd=0), "zero margins": dict(margin="constant"),
                    "pad to 8 by zeros": dict(pad8="constant"), "quarter from the padded plane, shifted": dict(quarter_shift=1)}
DG_VARIANTS = {"the last minimum wins": dict(first_wins=False), "x-major order": dict(y_major=False),
               "no & ~7 on the width": dict(width_mult8=False),
               "area reduced when the left clamp moves the origin": dict(reduce_on_left_clamp=True),
               "padding 16": dict(pad=16), ">= at the complexity threshold": dict(cplx_strict=False),
               "floor division": dict(trunc_div=False)}


def differs(entry, model=MODEL, pyramid=PM.pyramid) -> bool:
    sb, met = model.detect(*content(entry[2], *entry[0]), *entry[1], pyramid=pyramid)
    want_sb, want_met, _ = expected(*entry)
    return sb.tobytes() != want_sb.tobytes() or met != list(want_met)


@pytest.mark.parametrize("name", list(PYRAMID_VARIANTS) + list(DG_VARIANTS))
def test_dg_sweep_discriminates(name):
    """A deliberately wrong model changes at least one expected value of the sweep: the inputs can tell."""
    small = [e for e in SWEEP if e[0] != BIG]
    assert not any(differs(e) for e in small[:5])  # (the model itself does not)
    if name in PYRAMID_VARIANTS:
        wrong = functools.partial(PM.pyramid, **PYRAMID_VARIANTS[name])
        assert any(differs(e, pyramid=wrong) for e in small), name
    else:
        wrong = type("WrongDg", (DM.DgModel,), DG_VARIANTS[name])()
        assert any(differs(e, model=wrong) for e in small), name


# ----------------------------------------------------------------------------
# GPU: svtme_dg_detect against the model
# ----------------------------------------------------------------------------
def assert_equal_to_model(mets, sb, k, want_sb, want_met, what):
    if sb is not None:
        for f in ("sad", "mv_x", "mv_y"):
            bad = np.flatnonzero(sb[k][f] != want_sb[f])
            assert bad.size == 0, (what, f, "SB", int(bad[0]), sb[k][bad[0]], want_sb[bad[0]], len(bad))
    assert metrics_rows([mets[k]])[0] == list(want_met), what


@pytest.mark.gpu
@pytest.mark.parametrize("entry", SWEEP, ids=entry_id)
def test_dg_sweep_equals_model(svtme, gpu, entry):
    size, area, kind = entry
    cur, ref = content(kind, *size)
    want_sb, want_met, _ = expected(*entry)
    gpu.upload(BASE + 201, cur)
    gpu.upload(BASE + 202, ref)
    try:
        mets, sb = gpu.dg_detect([(BASE + 201, BASE + 202)], *area)
        assert sb.shape == (1, len(want_sb))
        assert_equal_to_model(mets, sb, 0, want_sb, want_met, entry)
        mets2, none = gpu.dg_detect([(BASE + 201, BASE + 202)], *area, with_sb=False)
        assert none is None
        assert_equal_to_model(mets2, None, 0, want_sb, want_met, entry)
    finally:
        gpu.release(BASE + 201)
        gpu.release(BASE + 202)


@pytest.mark.gpu
def test_dg_full_batch_of_mixed_contents(svtme, gpu):
    """SVTME_DG_MAX_PAIRS pairs of mixed contents in one call equal the single calls and the model;
    one pair searches a picture against itself."""
    size, area = (136, 72), (64, 64)
    kinds = ("noise", "ramp+-", "sat", "same", "tile_skew", "thr", "flat", "ramp--")
    assert len(kinds) == svtme.DG_MAX_PAIRS == 8
    pairs, used = [], []
    for k, kind in enumerate(kinds):
        cur, ref = content(kind, *size)
        c, r = BASE + 300 + 2 * k, BASE + 301 + 2 * k
        gpu.upload(c, cur)
        used.append(c)
        if kind == "same":
            r = c  # cur == ref: one resident picture
        else:
            gpu.upload(r, ref)
            used.append(r)
        pairs.append((c, r))
    try:
        mets, sb = gpu.dg_detect(pairs, *area)
        for k, kind in enumerate(kinds):
            want_sb, want_met, _ = expected(size, area, kind)
            assert_equal_to_model(mets, sb, k, want_sb, want_met, kind)
            m1, sb1 = gpu.dg_detect([pairs[k]], *area)
            assert sb1.tobytes() == sb[k:k + 1].tobytes() and metrics_rows(m1) == metrics_rows(mets[k:k + 1]), kind
    finally:
        for pn in used:
            gpu.release(pn)


@pytest.mark.gpu
def test_dg_10bit_pair_equals_model_on_msb_planes(svtme, gpu):
    w, h, area = 121, 67, (64, 64)
    rng = np.random.default_rng(10)
    cur, ref = (rng.integers(0, 1024, (h, w), dtype=np.uint16) for _ in range(2))
    want_sb, want_met = MODEL.detect(cur, ref, *area)
    assert want_sb.tobytes() == MODEL.detect((cur >> 2).astype(np.uint8), (ref >> 2).astype(np.uint8), *area)[0].tobytes()
    gpu.upload(BASE + 401, cur)  # svtme_picture_upload_10bit
    gpu.upload(BASE + 402, ref)
    try:
        mets, sb = gpu.dg_detect([(BASE + 401, BASE + 402)], *area)
        assert_equal_to_model(mets, sb, 0, want_sb, want_met, "10 bit")
    finally:
        gpu.release(BASE + 401)
        gpu.release(BASE + 402)


@pytest.mark.gpu
def test_dg_after_device_async_upload_equals_model(svtme, gpu):
    """Both pictures through svtme_picture_upload_device_async and no sync: the call waits on the GPU."""
    import torch

    size, area, kind = (200, 136), (128, 128), "noise"
    w, h = size
    stride, off = w + 13, 3
    want_sb, want_met, _ = expected(size, area, kind)
    keep = []
    for pic in content(kind, w, h):
        buf = np.full(off + stride * h, 0xA5, np.uint8)
        buf[off:].reshape(h, stride)[:, :w] = pic
        keep.append(torch.from_numpy(buf).cuda())
    torch.cuda.synchronize()  # the planes are on the device before the upload stream reads them
    for k, t in enumerate(keep):
        gpu.upload_device_async(BASE + 501 + k, t.data_ptr() + off, stride, w, h)
    mets, sb = gpu.dg_detect([(BASE + 501, BASE + 502)], *area)
    for k in range(2):
        assert gpu.lib.svtme_picture_release(gpu.ctx, BASE + 501 + k) == 0
    gpu.sync()
    assert_equal_to_model(mets, sb, 0, want_sb, want_met, "device async")
