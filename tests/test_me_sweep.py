"""The seeded sweep of the picture job (tests/me_sweep.py): the committed list against the
generator, the oracle against the reference's checksums (tests/golden/me_sweep.json, made by
make_golden_me_sweep.py from libsvtref with C and AVX2 kernels), the coverage the list
reaches, the host dispatch predicates over the list; and on the GPU every case under
paths 0 and under every single kernel-path bit that changes its dispatch, with and without
per-SB results, against the oracle and the reference's checksum, plus a batch of 16 jobs
of different dispatch classes."""
import json
import os
import sys

import pytest

from conftest import ref_available

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
for p in (GOLD, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import me_sweep as M  # noqa: E402

FIXTURE = M.fixture()
ENTRIES = FIXTURE["cases"]
BASE = 20000  # picture numbers of this file's GPU tests: BASE + 100 * case index + time
oracle_of = M.oracle_of  # the oracle's outputs of case k, computed once per process and shared


def test_committed_list_is_the_generator(svtme):
    assert [e["case"] for e in ENTRIES] == M.cases()
    assert [e["case"] for e in ENTRIES[:len(M.SWEEP_SEEDS)]] == [M.sweep_case(s) for s in M.SWEEP_SEEDS]
    assert json.loads(json.dumps(M.cases())) == M.cases()  # JSON-serialisable as it stands
    names = [e["case"]["name"] for e in ENTRIES]
    assert len(set(names)) == len(names)
    for case in M.cases():  # the fixed parts of the space
        assert len(case["l0"]) + len(case["l1"]) <= 7 and 1 <= len(case["l0"]) <= 4 and len(case["l1"]) <= 3
        assert "num_hme_sa_w" not in case["mut"] and "num_hme_sa_h" not in case["mut"]
    big = sum((e["case"]["w"], e["case"]["h"]) == M.BIG for e in ENTRIES)
    assert big * 6 <= len(ENTRIES), big


@pytest.mark.parametrize("k", range(len(ENTRIES)), ids=lambda k: ENTRIES[k]["case"]["name"])
def test_oracle_reproduces_reference_checksum(svtme, k):
    S = svtme
    ctrl, recs, sbr = oracle_of(S, k)
    assert S.records_checksum(recs, sbr) == ENTRIES[k]["checksum"]
    assert M.coverage(S, ENTRIES[k]["case"], ctrl, recs, sbr) == ENTRIES[k]["coverage"]


def test_every_coverage_key_is_reached():
    total = FIXTURE["total"]
    assert sorted(total) == sorted(M.COVERAGE_KEYS)
    assert not [k for k, v in total.items() if v <= 0]
    for k in M.COVERAGE_KEYS:
        assert sum(e["coverage"][k] for e in ENTRIES) == total[k], k


@pytest.mark.skipif(not ref_available(), reason="reference harness not built")
def test_one_case_regenerates_from_the_reference(svtme):
    import make_golden_me_sweep as G

    k = next(i for i, e in enumerate(ENTRIES) if e["case"]["name"] == "d_safe_zz_fused")
    assert G.golden_entry(ENTRIES[k]["case"]) == ENTRIES[k]


def dispatches(S):
    lib = M.lib_of(S)
    out = []
    for e in ENTRIES:
        job = M.job_of(S, e["case"], M.controls_of(S, e["case"]))
        d = M.dispatch_of(S, lib, job)
        out.append((job, d, M.paths_of(S, job, d)))
    return out


def test_dispatch_predicates_take_all_their_values(svtme):
    ds = [d for _, d, _ in dispatches(svtme)]
    for name in ("fused", "rt", "l1_full", "fp_wide_lds", "k32", "l0_full"):
        assert {d[name] for d in ds} == {False, True}, name
    assert {d["waves"] for d in ds} == {3, 4}
    parts = {d["parts"] for d in ds}
    assert 0 in parts and 1 in parts and max(parts) > 1 and 16 in parts and parts & {2, 3, 4}, parts


def test_every_path_bit_applies_to_some_case(svtme):
    seen = set()
    for _, _, paths in dispatches(svtme):
        seen.update(paths)
    assert seen == set(M.PATH_BITS)


def test_cases_stay_inside_what_validate_job_accepts(svtme):
    """The limits validate_job refuses (test_job_validation_errors), as values: no case reaches them."""
    import ctypes as C

    lib = M.lib_of(svtme)
    lib.svtme_fp_area_bound.argtypes = [C.POINTER(svtme.Controls), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.svtme_fp_area_bound.restype = None
    for e in ENTRIES:
        c = M.controls_of(svtme, e["case"])
        assert c.num_hme_sa_w == 2 and c.num_hme_sa_h == 2
        assert c.hme_l2_sa.width <= 8192
        w, h = C.c_uint32(), C.c_uint32()
        lib.svtme_fp_area_bound(C.byref(c), C.byref(w), C.byref(h))
        assert c.enable_me_sr_adjustment != 2 or w.value <= 1016, e["case"]["name"]
        if c.enable_me_sr_adjustment and c.enable_hme_flag and not e["case"]["tf"]:
            assert c.stationary_me_sr_divisor and c.me_sr_divisor_for_low_hme_sad, e["case"]["name"]


# ----------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------
def batch_selection(S):
    """16 sweep cases moved to one picture size (whole pictures; controls as derived for their
    own size), of as many launch classes as the list has there: one case of every class in
    list order, then the rest. -> (size, cases, classes)"""
    lib = M.lib_of(S)
    best = None
    for w, h in M.SIZES:
        moved = []
        for e in ENTRIES:
            c = e["case"]
            res = c["res"] if c["res"] is not None else S.input_resolution_of(c["w"], c["h"])
            c = dict(c, w=w, h=h, sb_begin=0, sb_count=0, res=res)
            job = M.job_of(S, c, M.controls_of(S, c))
            moved.append((M.launch_class(M.dispatch_of(S, lib, job)), c))
        first, seen = [], set()
        for cls, c in moved:
            if cls not in seen:
                seen.add(cls)
                first.append(c)
        picked = (first + [c for _, c in moved if c not in first])[:16]
        if best is None or (len(seen), w * h) > best[0]:  # most classes, then the larger picture
            best = ((len(seen), w * h), (w, h), picked)
    classes = len({M.launch_class(M.dispatch_of(S, lib, M.job_of(S, c, M.controls_of(S, c)))) for c in best[2]})
    return best[1], best[2], classes


def test_batch_selection_has_sixteen_jobs_of_many_classes(svtme):
    size, picked, classes = batch_selection(svtme)
    assert len(picked) == 16 and classes > 2 and all((c["w"], c["h"]) == size for c in picked)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(ENTRIES)), ids=lambda k: ENTRIES[k]["case"]["name"])
def test_gpu_case_under_every_applicable_path(svtme, gpu, k):
    S = svtme
    case = ENTRIES[k]["case"]
    ctrl, orecs, osbr = oracle_of(S, k)
    base = BASE + 100 * k
    job = M.job_of(S, case, ctrl, base)
    lib = M.lib_of(S)
    paths = M.paths_of(S, job, M.dispatch_of(S, lib, job))
    frames = M.frames_of(S, case)
    got = {}
    for t, f in frames.items():
        gpu.upload(base + t, f)
    try:
        for name in [None] + paths:
            gpu.set_paths(getattr(S, "PATH_" + name) if name else 0)
            recs, sbr = gpu.submit(job)
            recs_only, _ = gpu.submit(job, with_sb_results=False)
            got[name] = (recs, sbr, recs_only)
    finally:
        gpu.set_paths(0)
        for t in frames:
            gpu.release(base + t)
    for name, (recs, sbr, recs_only) in got.items():
        errs = S.compare_records(orecs, recs, osbr, sbr)
        assert not errs, (name, errs[:5])
        errs = S.compare_records(orecs, recs_only)
        assert not errs, (name, "records only", errs[:5])
        assert S.records_checksum(recs, sbr) == ENTRIES[k]["checksum"], name
        assert S.records_checksum(recs_only, sbr) == ENTRIES[k]["checksum"], (name, "records only")


@pytest.mark.gpu
def test_gpu_batch_of_sixteen_dispatch_classes(svtme, gpu):
    """16 sweep jobs of one picture size, of as many launch classes (svtme_launch_key) as the list
    has at that size, in one svtme_submit_batch_device: each job's outputs equal its own
    submission's and the oracle's, and the batch went out as more than two launch groups."""
    S = svtme
    size, picked, classes = batch_selection(S)
    assert len(picked) == 16 and classes > 2, (size, len(picked), classes)
    jobs, frames, oracle = [], {}, []
    for k, case in enumerate(picked):
        base = BASE + 100 * (len(ENTRIES) + k)
        ctrl = M.controls_of(S, case)
        jobs.append(M.job_of(S, case, ctrl, base))
        fr = M.frames_of(S, case)
        frames.update({base + t: f for t, f in fr.items()})
        oracle.append(M.run_cpu(S, case, "oracle", frames=fr, ctrl=ctrl))
    for pn, f in frames.items():
        gpu.upload(pn, f)
    try:
        single = [gpu.submit(j) for j in jobs]
        gpu.set_timing(True)
        gpu.timing_read()
        got = gpu.submit_batch(jobs)
        groups, _ = gpu.timing_read()
    finally:
        gpu.set_timing(False)
        for pn in frames:
            gpu.release(pn)
    assert groups > 2, groups
    assert groups == classes, (groups, classes)
    for case, (recs, sbr), (srecs, ssbr), (orecs, osbr) in zip(picked, got, single, oracle):
        assert not S.compare_records(orecs, recs, osbr, sbr), case["name"]
        assert not S.compare_records(srecs, recs, ssbr, sbr), case["name"]
        assert S.records_checksum(recs, sbr) == S.records_checksum(srecs, ssbr) == S.records_checksum(orecs, osbr)
