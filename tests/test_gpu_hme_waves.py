"""k_hme in workgroups of three wavefronts (svtme_hme_waves) against the same job
forced to four (PATH_HME_4WAVES) and against the CPU oracle, byte for byte: the
records and the per-SB results. Pictures of 3 x 3 SBs, 192 x 136: the width a
multiple of 64 (the fused path), the last SB row 8 lines high (the partial-height
branches of every tile loop). Reference counts below, equal to and above the
wave count, preset-8 and preset-6 controls (HME-L2: the full-resolution source
block loaded by one wave in two passes), content with every reference searched
and with some pruned (both branches of the full-pel record assignment), 10-bit
input, a TF-ME job, the real-time tune's second A1 round, records alone, and a
batch whose jobs differ in svtme_hme_waves."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 192, 136
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def lib_of(S):
    lib = S.load_product()
    lib.svtme_hme_waves.argtypes = [C.POINTER(S.Job)]
    lib.svtme_hme_waves.restype = C.c_uint32
    lib.svtme_hme_fused.argtypes = [C.POINTER(S.Job)]
    lib.svtme_hme_fused.restype = C.c_bool
    lib.svtme_fp_parts.argtypes = [C.POINTER(S.Controls)]
    lib.svtme_fp_parts.restype = C.c_uint32
    return lib


def controls(S, name: str):
    res = S.input_resolution_of(W, H)
    if name in ("p8", "p6"):
        return S.derive_controls(int(name[1]), 35, res, 1)
    if name in ("p8_all", "p6_all"):  # no reference pruned: every record searches
        c = S.derive_controls(int(name[1]), 35, res, 1)
        c.enable_me_hme_ref_pruning = 0
        c.zz_sad_th = c.phme_sad_th = 0
        return c
    if name == "tf3":  # TF-ME with sub-sampled rows (hme_me_level 3)
        return S.derive_controls_tf(3, 0, 35, res)
    if name == "rt":  # the real-time tune's HME-L0 reduction, as the golden case stores it
        with open(os.path.join(GOLD, "me_cases.json")) as fh:
            case = next(c for c in json.load(fh) if c["name"] == "pan320_p8_rt200")
        return S.Controls.from_dict(case["ctrl"])
    raise ValueError(name)


# name, controls, content, list 0, list 1, job extras, 10-bit, every record searched (None: not checked)
CASES = [
    ("p8-1+0", "p8", "pan", (7,), (), {}, False, True),
    ("p8-1+1", "p8", "pan", (7,), (9,), {}, False, True),
    ("p8-2+1", "p8", "pan", (7, 6), (9,), {}, False, False),
    ("p8-2+2", "p8", "pan", (7, 6), (9, 10), {}, False, False),
    ("p8-4+3", "p8", "pan", (7, 6, 5, 4), (9, 10, 11), {}, False, False),
    ("p8-4+4", "p8", "pan", (7, 6, 5, 4), (9, 10, 11, 12), {}, False, False),
    ("p8-2+1-all", "p8_all", "noise", (7, 6), (9,), {}, False, True),
    ("p8-2+2-all", "p8_all", "hpan", (7, 6), (9, 10), {}, False, True),
    ("p8-4+4-hpan", "p8", "hpan", (7, 6, 5, 4), (9, 10, 11, 12), {}, False, False),  # up to 7 records search
    ("p8-2+2-stripes", "p8", "stripes", (7, 6), (9, 10), {}, False, False),
    ("p8-2+2-flat-gm", "p8", "flat", (7, 6), (9, 10), {"gm": True}, False, None),
    ("p6-1+1", "p6", "pan", (7,), (9,), {}, False, True),
    ("p6-2+2", "p6", "noise", (7, 6), (9, 10), {}, False, False),
    ("p6-2+2-all", "p6_all", "hpan", (7, 6), (9, 10), {}, False, True),
    ("p6-4+3", "p6", "pan", (7, 6, 5, 4), (9, 10, 11), {}, False, False),
    ("p6-1+1-10bit", "p6", "pan10", (7,), (9,), {}, True, True),
    ("p8-2+2-10bit", "p8", "pan10", (7, 6), (9, 10), {}, True, False),
    ("tf3-exit", "tf3", "pan", (7,), (), {"me_type": "mctf", "tf_me_exit_th": 2600}, False, None),
    ("tf3-noexit", "tf3", "noise", (9,), (), {"me_type": "mctf", "tf_me_exit_th": 0}, False, True),
    ("rt-2+2", "rt", "pan", (7, 6), (9, 10), {}, False, None),
    ("rt-2+1-vpan", "rt", "vpan", (7, 6), (9,), {}, False, None),
]


def frames_of(S, kind, ts):
    if kind == "pan10":
        syn = S.Synth(W, H)
        return {t: syn.frame10(t) for t in ts}
    return S.test_frames(kind, W, H, ts)


def make(S, ctrl, base, l0, l1, extra):
    kw = dict(extra)
    if kw.get("me_type") == "mctf":
        kw["me_type"] = S.ME_MCTF
    job = S.case_job(ctrl, W, H, base + 8, [base + t for t in l0], [base + t for t in l1], 1, **kw)
    return job


def oracle(S, ctrl, frames, l0, l1, extra):
    pyr = {t: S.build_host_pyramid(f, "oracle") for t, f in frames.items()}
    refs = {(0, i): pyr[t] for i, t in enumerate(l0)}
    refs.update({(1, i): pyr[t] for i, t in enumerate(l1)})
    return S.run_checker(make(S, ctrl, 0, l0, l1, extra), pyr[8], refs, "oracle", nthreads=8)


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_three_waves_equal_four_waves_and_oracle(svtme, gpu, case):
    S = svtme
    name, cname, kind, l0, l1, extra, ten, all_searched = case
    ctrl = controls(S, cname)
    lib = lib_of(S)
    base = 8000
    frames = frames_of(S, kind, sorted(set([8] + list(l0) + list(l1))))
    job = make(S, ctrl, base, l0, l1, extra)
    # the case runs the whole-pass k_hme
    assert lib.svtme_hme_fused(C.byref(job)) and lib.svtme_fp_parts(C.byref(job.ctrl)) == 1
    for t, f in frames.items():
        gpu.upload(base + t, f)
    try:
        gpu.set_paths(0)
        recs, sbr = gpu.submit(job)
        recs_only, _ = gpu.submit(job, with_sb_results=False)
        gpu.set_paths(S.PATH_HME_4WAVES)
        recs4, sbr4 = gpu.submit(job)
        recs4_only, _ = gpu.submit(job, with_sb_results=False)
    finally:
        gpu.set_paths(0)
        for t in frames:
            gpu.release(base + t)
    orecs, osbr = oracle(S, ctrl, frames, l0, l1, extra)
    if all_searched is not None:  # the case takes the branch of the record assignment it is here for
        assert bool(orecs["searched"].all()) == all_searched
    errs = S.compare_records(orecs, recs, osbr, sbr)
    assert not errs, errs[:5]
    for got in (recs, recs_only, recs4, recs4_only):
        assert same_bytes(orecs, got)
    assert same_bytes(sbr, sbr4) and same_bytes(osbr, sbr)


def test_batch_of_jobs_with_different_waves(svtme, gpu):
    """Two jobs of one batch whose svtme_hme_waves differ go to two launches
    (svtme_launch_key) and both equal the oracle."""
    S = svtme
    lib = lib_of(S)
    ctrl = controls(S, "p8")
    base = 8100
    lists = [((7, 6), (9, 10)), ((7, 6, 5, 4), (9, 10, 11))]
    frames = frames_of(S, "pan", [4, 5, 6, 7, 8, 9, 10, 11])
    jobs = [make(S, ctrl, base, l0, l1, {}) for l0, l1 in lists]
    waves = [lib.svtme_hme_waves(C.byref(j)) for j in jobs]
    assert sorted(waves) == [3, 4], waves
    for t, f in frames.items():
        gpu.upload(base + t, f)
    try:
        gpu.set_timing(True)
        gpu.timing_read()
        got = gpu.submit_batch(jobs)
        groups, _ = gpu.timing_read()
        gpu.set_timing(False)
        same = gpu.submit_batch([jobs[0], jobs[0]])
    finally:
        gpu.set_timing(False)
        for t in frames:
            gpu.release(base + t)
    assert groups == 2, groups
    for (l0, l1), (recs, sbr) in zip(lists, got):
        orecs, osbr = oracle(S, ctrl, frames, l0, l1, {})
        assert not S.compare_records(orecs, recs, osbr, sbr)
        assert same_bytes(orecs, recs) and same_bytes(osbr, sbr)
    assert same_bytes(same[0][0], got[0][0]) and same_bytes(same[1][1], got[0][1])
