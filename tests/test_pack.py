"""Packed host output (svtme_submit_picture_packed_async, include/svtme.h
svtme_pack_layout): the bytes the encoder glue scatters (integration/
svtme_svt_glue.c) equal the numpy restatement of the documented layout
(svtme.pack_outputs) over the job's full outputs.

CPU: the oracle job API (oracle/liboraclejob.so, the encoder tests' backend).
GPU: k_pack behind the ticket API of libsvtme.so, several jobs in flight on
both submission lanes, the ticket limit, and jobs after svtme_reserve.

The second half pins the packed path to the oracle ("Packed output"): every case of
the ME sweep (tests/me_sweep.py, whose oracle outputs tests/test_me_sweep.py pins to the
reference's checksums) is packed under the layouts of tests/golden/pack_layouts.json and decoded
by tests/pack_model.py, a decoder written from the header's layout comment alone; plus recycled
ticket buffers, mixed batches, refusals that must leave no ticket behind, svtme_ticket_wait_timed,
a pageable destination and svtme_host_register.
"""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

import svtme as S

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(HERE, "golden"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import me_sweep as M  # noqa: E402
import pack_model as PM  # noqa: E402
import pyramid_model as PYR  # noqa: E402

W, H = 640, 360
# (n_pus, max_cand, max_refs, full_records, sb_results): PA-ME allocations of
# pcs.c:91-117 (85 / 21 / 5 PUs; 2+1 refs: 3 MVs, 3 + 2 + 1 = 6 candidates) and TF-ME's
LAYOUTS = [(85, 6, 3, 0, 1), (21, 6, 3, 0, 1), (5, 23, 7, 0, 1), (85, 6, 3, 1, 1), (0, 0, 0, 1, 0)]


def _layout(t):
    L = S.PackLayout()
    L.n_pus, L.max_cand, L.max_refs, L.full_records, L.sb_results = t
    return L


def _setup(api, base):
    frames = S.test_frames("pan", W, H, [6, 7, 8, 9])
    for t, f in frames.items():
        api.upload(base + t, f)
    ctrl = S.derive_controls(8, 35, S.input_resolution_of(W, H), 1)
    return S.make_job(W, H, ctrl, base + 8, (base + 7, base + 6), (base + 9,), temporal_layer_index=1,
                      ref_count_used=(2, 1))


def test_reserve_arguments_oracle_backend():
    api = S.GpuME(0, lib=S.load_oracle_job())
    api.reserve(W, H, 8, 4)
    for bad in ((0, H, 8, 4), (W, H, 0, 4), (W, H, 9, 4), (W, H, 8, S.MAX_TICKETS + 1)):
        with pytest.raises(RuntimeError):
            api.reserve(*bad)
    api.close()


def test_packed_layout_oracle_backend():
    api = S.GpuME(0, lib=S.load_oracle_job())
    job = _setup(api, 0)
    recs, sbr = api.submit(job)
    for t in LAYOUTS:
        L = _layout(t)
        got = api.submit_packed(job, L)
        assert got == S.pack_outputs(recs, sbr if L.sb_results else None, L), t
    api.close()


@pytest.mark.gpu
def test_packed_output_gpu(gpu):
    job = _setup(gpu, 7000)
    recs, sbr = gpu.submit(job)
    for t in LAYOUTS:
        L = _layout(t)
        assert gpu.submit_packed(job, L, lane=t[0] & 1) == S.pack_outputs(recs, sbr if L.sb_results else None, L), t
    # several jobs in flight on both lanes, retired out of order
    L = _layout(LAYOUTS[0])
    exp = S.pack_outputs(recs, sbr, L)
    pend = [gpu.submit_packed(job, L, lane=k & 1, wait=False) for k in range(6)]
    for p in reversed(pend):
        assert gpu.wait_packed(*p) == exp
    # at most SVTME_MAX_TICKETS outstanding: one thread holding them all is refused the
    # next one (nobody retires a ticket within the grace period), the context keeps serving
    pend = [gpu.submit_packed(job, L, lane=k & 1, wait=False) for k in range(S.MAX_TICKETS)]
    with pytest.raises(RuntimeError, match="outstanding"):
        gpu.submit_packed(job, L, wait=False)
    for p in pend:
        assert gpu.wait_packed(*p) == exp
    assert gpu.submit_packed(job, L) == exp
    # more submitting threads than ticket slots (the reference's up to 25 ME threads plus
    # TF threads, each with a job in flight): a submission finding every slot taken waits
    # for another thread's svtme_ticket_wait instead of failing
    import threading

    errs, done = [], []

    def worker(k):
        try:
            for _ in range(3):
                if gpu.submit_packed(job, L, lane=k & 1) != exp:
                    errs.append(f"thread {k}: packed bytes differ")
            done.append(k)
        except Exception as e:  # noqa: BLE001
            errs.append(f"thread {k}: {e}")
    th = [threading.Thread(target=worker, args=(k,)) for k in range(S.MAX_TICKETS + 16)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    assert not errs and len(done) == S.MAX_TICKETS + 16, errs[:3]
    # reserved for a larger picture (every lane's scratch, the first tickets' buffers):
    # the same bytes, and a picture beyond the reservation still grows what it needs
    gpu.reserve(W, H // 2, 3, 2)
    gpu.reserve(2 * W, 2 * H, 8, 6)
    for t in LAYOUTS:
        L = _layout(t)
        assert gpu.submit_packed(job, L, lane=1 - (t[0] & 1)) == S.pack_outputs(recs, sbr if L.sb_results else None, L), t
    for bad in ((0, H, 8, 4), (W, H, 9, 4), (W, H, 8, S.MAX_TICKETS + 1)):
        with pytest.raises(RuntimeError):
            gpu.reserve(*bad)
    for t in (6, 7, 8, 9):
        gpu.release(7000 + t)


# ----------------------------------------------------------------------------
# the packed path against the oracle: the sweep's cases, decoded by tests/pack_model.py
# ----------------------------------------------------------------------------
ENTRIES = M.fixture()["cases"]
with open(os.path.join(HERE, "golden", "pack_layouts.json")) as _fh:
    LAYOUT_LIST = json.load(_fh)
PBASE = 40000  # picture numbers of these tests: PBASE + 100 * index + time
BAD_PARAMETER = 0x80001005
IDS = [e["case"]["name"] for e in ENTRIES]


def case_layouts(k: int) -> list:
    """[(kind, layout tuple)] of committed case k."""
    row = LAYOUT_LIST["cases"][k]
    return [(kind, tuple(row[kind])) for kind in ("glue", "drawn", "directed") if kind in row]


_packed = {}


def packed_by_restatement(k: int, t: tuple) -> bytes:
    """svtme.pack_outputs over the oracle's outputs of case k, once per process."""
    if (k, t) not in _packed:
        _, recs, sbr = M.oracle_of(S, k)
        _packed[k, t] = S.pack_outputs(recs, sbr if t[4] else None, _layout(t))
    return _packed[k, t]


def assert_decodes_to(buf: bytes, t: tuple, recs, sbr, what):
    """The packed bytes, decoded by the model, are the outputs (records made canonical) cut to the
    layout: every field exactly, the pad bytes of records and tails zero, every slack byte zero."""
    n_sb, R = recs.shape
    assert len(buf) == n_sb * PM.stride_of(t, R), what
    got = PM.unpack(buf, t, R, n_sb)
    errs = PM.mismatches(got, PM.expect(recs, sbr, t))
    assert not errs, (what, errs[:5])
    assert not got[0]["pad"].any(), (what, "record pad bytes")
    assert not got[1]["slack"].any(), (what, "slack bytes", np.argwhere(got[1]["slack"])[0].tolist())


def test_layout_list_is_the_generator():
    assert LAYOUT_LIST == PM.golden(M.cases())
    assert [r["name"] for r in LAYOUT_LIST["cases"]] == IDS
    for k, e in enumerate(ENTRIES):
        case, row = e["case"], LAYOUT_LIST["cases"][k]
        assert 2 <= len(case_layouts(k)) <= 3
        job = M.job_of(S, case, M.controls_of(S, case))
        assert row["R"] == S.ref_slots(job)
        glue = tuple(row["glue"])
        if case["tf"]:
            assert job.me_type == S.ME_MCTF and glue == (0, 0, 0, 1, 0)
        else:  # what layout_of (integration/svtme_svt_glue.c) reads from the picture: the job carries the same
            n_pus = 85 if job.enable_me_16x16 and job.enable_me_8x8 else 21 if job.enable_me_16x16 else 5
            assert glue == (n_pus, job.max_cand, job.max_refs, 0, 1), case["name"]
        for _, t in case_layouts(k):  # the header's svtme_packed_sb_bytes, restated twice
            assert PM.stride_of(t, row["R"]) == S.packed_sb_bytes(_layout(t), row["R"]) and PM.stride_of(t, row["R"]) % 16 == 0
            if t[4]:
                assert 1 <= t[0] <= 85 and 1 <= t[1] <= 23 and 1 <= t[2] <= 7, t


def test_layout_list_coverage():
    rows = [(e["case"], LAYOUT_LIST["cases"][k]["R"], t) for k, e in enumerate(ENTRIES) for _, t in case_layouts(k)]
    assert {R for _, R, _ in rows} == set(range(1, 8))
    strides = {PM.stride_of(t, R) for _, R, t in rows}
    assert min(strides) == 32 and max(strides) > 9000, sorted(strides)
    with_sb = [(R, t) for _, R, t in rows if t[4]]
    assert any(t[2] < R for R, t in with_sb) and any(t[2] == R for R, t in with_sb) and any(t[2] > R for R, t in with_sb)
    assert {(t[3], t[4]) for _, _, t in rows} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c["sb_begin"] > 0 for c, _, _ in rows) and any(c["bits"] == 10 for c, _, _ in rows)
    assert any(c["tf"] and t[4] for c, _, t in rows)  # SB results of a TF-ME job
    drawn = [tuple(r["drawn"]) for r in LAYOUT_LIST["cases"]]
    assert {t[0] for t in drawn} == set(PM.N_PUS)


@pytest.mark.parametrize("k", range(len(ENTRIES)), ids=IDS)
def test_unpack_round_trip(k):
    """unpack(pack_outputs(oracle outputs)) gives the outputs back, under every layout of the case."""
    _, recs, sbr = M.oracle_of(S, k)
    for kind, t in case_layouts(k):
        assert_decodes_to(packed_by_restatement(k, t), t, recs, sbr, (IDS[k], kind))


def oracle_job_subset() -> list:
    """Indices of 8-bit cases up to 208x136 (the oracle job backend has no 10-bit upload), taken in
    list order while they add one of: n_pus 5 / 21 / 85 of the glue's layout, R = 1, 2, 5, 7, a TF-ME
    job, an SB band."""
    want = {("n_pus", 5), ("n_pus", 21), ("n_pus", 85), ("R", 1), ("R", 2), ("R", 5), ("R", 7), "tf", "band"}
    out = []
    for k, e in enumerate(ENTRIES):
        c = e["case"]
        if c["bits"] != 8 or c["w"] > 208 or c["h"] > 136:
            continue
        has = {("R", PM.slots_of(c)), "tf" if c["tf"] else ("n_pus", PM.glue_layout(c)[0])}
        if c["sb_begin"] > 0:
            has.add("band")
        if has & want:
            want -= has
            out.append(k)
    return out


ORACLE_JOB_SUBSET = oracle_job_subset()


def test_oracle_job_subset_coverage():
    cs = [ENTRIES[k]["case"] for k in ORACLE_JOB_SUBSET]
    assert all(c["bits"] == 8 and c["w"] <= 208 and c["h"] <= 136 for c in cs) and len(cs) <= 9
    assert {PM.glue_layout(c)[0] for c in cs if not c["tf"]} >= {5, 21, 85}
    assert {PM.slots_of(c) for c in cs} >= {1, 2, 5, 7}
    assert any(c["tf"] for c in cs) and any(c["sb_begin"] > 0 and c["sb_count"] for c in cs)


@pytest.mark.parametrize("k", ORACLE_JOB_SUBSET, ids=lambda k: IDS[k])
def test_oracle_job_backend_packs_the_same_bytes(k):
    """pack_sb of oracle/svtme_oraclejob.c (the encoder tests' backend) against svtme.pack_outputs."""
    case = ENTRIES[k]["case"]
    ctrl, _, _ = M.oracle_of(S, k)
    api = S.GpuME(0, lib=S.load_oracle_job())
    try:
        for t, f in M.frames_of(S, case).items():
            api.upload(t, f)
        job = M.job_of(S, case, ctrl)
        for kind, t in case_layouts(k):
            assert api.submit_packed(job, _layout(t)) == packed_by_restatement(k, t), (IDS[k], kind)
    finally:
        api.close()


# deliberately wrong decoders, each one change to the model: (unpack's arguments, expect's arguments)
WRONG_DECODERS = {
    "tail offset 672": ({}, dict(tail_offset=672)),
    "tail offset 688": ({}, dict(tail_offset=688)),
    "me_mv_array rows 7 wide": (dict(mv_row=7), {}),
    "candidate rows 23 wide": (dict(cand_row=23), {}),
    "flags before me_distortion": (dict(order=("dist6", "flags", "me_distortion", "me_mv_array", "total", "cands")), {}),
    "total after the candidates": (dict(order=("dist6", "me_distortion", "me_mv_array", "flags", "cands", "total")), {}),
    "stride rounded to 8": (dict(align=8), {}),
    "n_pus taken as 85": (dict(npus=85), {}),
    "records slot-major over SBs": (dict(slot_major=True), {}),
}


def decoder_differs(k: int, t: tuple, unpack_kw: dict, expect_kw: dict) -> bool:
    _, recs, sbr = M.oracle_of(S, k)
    n_sb, R = recs.shape
    grecs, gf = PM.unpack(packed_by_restatement(k, t), t, R, n_sb, **unpack_kw)
    wrecs, wf = PM.expect(recs, sbr, t, **expect_kw)
    # (a decoder that takes n_pus as 85 returns more rows: the ones the layout has are compared)
    gf = {name: v[tuple(slice(0, n) for n in wf[name].shape)] if name in wf else v for name, v in gf.items()}
    return bool(PM.mismatches((grecs, gf), (wrecs, wf)))


@pytest.mark.parametrize("name", list(WRONG_DECODERS))
def test_case_list_discriminates_decoders(name):
    """A decoder with one wrong offset, width or order changes a decoded value of some committed case."""
    pairs = [(k, t) for k in range(len(ENTRIES)) for _, t in case_layouts(k)]
    assert not any(decoder_differs(k, t, {}, {}) for k, t in pairs[:6])  # (the model itself does not)
    hits = [(IDS[k], t) for k, t in pairs if decoder_differs(k, t, *WRONG_DECODERS[name])]
    assert hits, name


# ----------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------
def upload_case(gpu, case, base: int) -> list:
    frames = M.frames_of(S, case)
    for t, f in frames.items():
        gpu.upload(base + t, f)
    return [base + t for t in frames]


def release_all(gpu, pns):
    for pn in pns:
        gpu.release(pn)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(ENTRIES)), ids=IDS)
def test_gpu_packed_case_equals_oracle(gpu, k):
    """Every sweep case (kernel paths 0) through svtme_submit_picture_packed_async under each of its
    layouts, the lanes alternating: the decoded bytes are the oracle's outputs, exactly; this
    includes best_sad == 0xFFFFFFFF on slots that were not searched and zero pad bytes."""
    case = ENTRIES[k]["case"]
    ctrl, orecs, osbr = M.oracle_of(S, k)
    base = PBASE + 100 * k
    job = M.job_of(S, case, ctrl, base)
    pns = upload_case(gpu, case, base)
    try:
        got = [(kind, t, gpu.submit_packed(job, _layout(t), lane=(k + i) & 1))
               for i, (kind, t) in enumerate(case_layouts(k))]
    finally:
        release_all(gpu, pns)
    for kind, t, buf in got:
        assert_decodes_to(buf, t, orecs, osbr, (IDS[k], kind))


def moved_selection():
    """test_me_sweep.batch_selection: 16 sweep cases moved to one picture size, one of every launch
    class there first -> (cases, number of classes, {name: index in the committed list})."""
    from test_me_sweep import batch_selection

    _, picked, classes = batch_selection(S)
    return picked, classes, {name: k for k, name in enumerate(IDS)}


_moved_oracle = {}


def moved_oracle(case):
    if case["name"] not in _moved_oracle:
        ctrl = M.controls_of(S, case)
        _moved_oracle[case["name"]] = (ctrl,) + tuple(M.run_cpu(S, case, "oracle", ctrl=ctrl))
    return _moved_oracle[case["name"]]


@pytest.mark.gpu
def test_gpu_recycled_ticket_buffer_leaves_nothing_behind(gpu):
    """A ticket's device buffer (records | SB results | packed bytes) is reused by the next job of
    any size and launch class. One case of every launch class the sweep reaches at one picture
    size (the fused k_hme, the split path, k_fp_wide, TF-ME's direct records that skip k_stage_e),
    packed through the ticket slot a poison job (noise, R = 7, the largest layout) has just used,
    gives the very bytes it gives on a context that never ran the poison job."""
    picked, classes, _ = moved_selection()
    first = picked[:classes]
    w, h = first[0]["w"], first[0]["h"]
    src = next(e["case"] for e in ENTRIES if e["case"]["name"] == "d_cand23")
    poison = dict(src, w=w, h=h, sb_begin=0, sb_count=0, res=S.input_resolution_of(src["w"], src["h"]))
    assert poison["content"] == "noise" and PM.slots_of(poison) == 7
    fresh = S.GpuME(0)
    try:
        pbase = PBASE + 100 * (len(ENTRIES) + 40)
        ppns = upload_case(gpu, poison, pbase)
        pjob = M.job_of(S, poison, M.controls_of(S, poison), pbase)
        for i, case in enumerate(first):
            base = PBASE + 100 * (len(ENTRIES) + 41 + i)
            job = M.job_of(S, case, M.controls_of(S, case), base)
            pns = upload_case(gpu, case, base)
            upload_case(fresh, case, base)
            try:
                for t in (PM.glue_layout(case), PM.LARGEST):
                    gpu.submit_packed(pjob, _layout(PM.LARGEST), lane=i & 1)
                    after_poison = gpu.submit_packed(job, _layout(t), lane=i & 1)
                    alone = fresh.submit_packed(job, _layout(t), lane=i & 1)
                    assert len(after_poison) == len(alone) > 0
                    bad = np.flatnonzero(np.frombuffer(after_poison, np.uint8) != np.frombuffer(alone, np.uint8))
                    assert bad.size == 0, (case["name"], t, "first byte", int(bad[0]), len(bad))
            finally:
                release_all(gpu, pns)
                release_all(fresh, pns)
        release_all(gpu, ppns)
    finally:
        fresh.close()


@pytest.mark.gpu
def test_gpu_mixed_packed_batches(gpu):
    """One svtme_submit_pictures_packed_async of 16 jobs of more than two launch classes, the
    layouts alternating between the glue's and the drawn ones (jobs with and without SB results in
    one launch), a second batch on the other lane before the first is waited for, the 32 tickets
    retired in a shuffled order: every output decodes to the oracle's."""
    picked, classes, index = moved_selection()
    assert len(picked) == 16 and classes > 2
    jobs, pns, oracle = [], [], []
    for i, case in enumerate(picked):
        base = PBASE + 100 * (len(ENTRIES) + i)
        ctrl, recs, sbr = moved_oracle(case)
        jobs.append(M.job_of(S, case, ctrl, base))
        oracle.append((recs, sbr))
        pns += upload_case(gpu, case, base)
    both = [(PM.glue_layout(c), PM.drawn_layout(index[c["name"]])) for c in picked]
    batches = [[pair[i & 1] for i, pair in enumerate(both)], [pair[1 - (i & 1)] for i, pair in enumerate(both)]]
    for ls in batches:  # with and without SB results, whole records and tails, in one launch
        assert {t[4] for t in ls} == {0, 1} and {t[3] for t in ls} == {0, 1}
    try:
        pend = []
        for lane, ls in enumerate(batches):
            out = gpu.submit_packed_batch(jobs, [_layout(t) for t in ls], lane=lane)
            assert len({p[0] for p in out}) == 16 and all(p[0] for p in out)
            pend += [(i, t, p) for i, (t, p) in enumerate(zip(ls, out))]
        g = M.Rng(5)
        order = sorted(range(len(pend)), key=lambda _: g.next())
        assert order != sorted(order)
        got = {q: gpu.wait_packed(*pend[q][2]) for q in order}
    finally:
        release_all(gpu, pns)
    for q, buf in got.items():
        i, t, _ = pend[q]
        assert_decodes_to(buf, t, *oracle[i], (picked[i]["name"], t, "batch", q // 16))


def tiny_job(gpu, base: int):
    """A 64x64 job with one reference (and its pictures, resident) -> (job, layout, picture numbers)."""
    for t in (7, 8):
        gpu.upload(base + t, S.test_frames("pan", 64, 64, [t])[t])
    ctrl = S.derive_controls(8, 35, S.input_resolution_of(64, 64), 1)
    job = S.make_job(64, 64, ctrl, base + 8, (base + 7,), (), temporal_layer_index=1, ref_count_used=(1, 0))
    return job, (85, 1, 1, 0, 1), [base + 7, base + 8]


def raw_batch(gpu, jobs, layouts, ptrs, n=None, lane: int = 0):
    """svtme_submit_pictures_packed_async as called -> (status, last error)."""
    m = len(jobs)
    tickets = (C.c_uint64 * m)()
    st = gpu.lib.svtme_submit_pictures_packed_async(gpu.ctx, lane, m if n is None else n, (S.Job * m)(*jobs),
                                                    (S.PackLayout * m)(*[_layout(t) for t in layouts]),
                                                    (C.c_void_p * m)(*ptrs), tickets)
    assert not any(tickets), "a refused submission returns no ticket"
    return st & 0xFFFFFFFF, gpu.lib.svtme_last_error().decode(errors="replace")


REFUSALS = ["n = 0", "n = 17", "null host_out 1", "n_pus 0", "n_pus 86", "max_cand 0", "max_cand 24", "max_refs 0",
            "max_refs 8", "job 1: reference not resident", "job 1: band outside the picture"]


@pytest.mark.gpu
@pytest.mark.parametrize("what", REFUSALS)
def test_gpu_refused_batch_takes_no_ticket(gpu, what):
    """Each refusal of svtme_submit_pictures_packed_async is SVTME_ERR_BAD_PARAMETER and consumes no
    ticket: afterwards SVTME_MAX_TICKETS submissions without a wait all succeed and the next one is
    refused ("outstanding")."""
    job, t, pns = tiny_job(gpu, PBASE + 100 * (len(ENTRIES) + 60))
    nbytes = PM.stride_of(t, 1)
    m = 17 if what == "n = 17" else 2
    ptrs = [gpu.lib.svtme_host_alloc(nbytes) for _ in range(m)]
    try:
        assert all(ptrs)
        jobs, layouts, args, n = [job] * m, [t] * m, list(ptrs), None
        if what in ("n = 0", "n = 17"):
            n = int(what[4:])
        elif what == "null host_out 1":
            args[1] = None
        elif what.startswith("job 1: reference"):
            bad = S.Job.from_buffer_copy(job)
            bad.ref_picture_number[0][0] = pns[0] + 50  # never uploaded
            jobs = [job, bad]
        elif what.startswith("job 1: band"):
            bad = S.Job.from_buffer_copy(job)
            bad.sb_begin, bad.sb_count = 1, 1  # the picture has one SB
            jobs = [job, bad]
        else:
            field, v = what.split()
            wrong = dict(zip(("n_pus", "max_cand", "max_refs"), t))
            wrong[field] = int(v)
            layouts = [t, (wrong["n_pus"], wrong["max_cand"], wrong["max_refs"], 0, 1)]
        st, msg = raw_batch(gpu, jobs, layouts, args, n)
        assert st == BAD_PARAMETER, (what, hex(st), msg)
        L = _layout(t)
        pend = [gpu.submit_packed(job, L, lane=k & 1, wait=False) for k in range(S.MAX_TICKETS)]
        with pytest.raises(RuntimeError, match="outstanding"):
            gpu.submit_packed(job, L, wait=False)
        bufs = [gpu.wait_packed(*p) for p in pend]
        assert len(set(bufs)) == 1 and bufs[0] == gpu.submit_packed(job, L)
    finally:
        for p in ptrs:
            gpu.lib.svtme_host_free(p)
        release_all(gpu, pns)


@pytest.mark.gpu
def test_gpu_ticket_wait_timed(gpu):
    """svtme_ticket_wait_timed: finite GPU-side times and the right bytes; a second wait on the
    ticket, ticket 0 and a ticket never issued are SVTME_ERR_BAD_PARAMETER and the context serves on."""
    k = IDS.index("d_npus5_single")
    case = ENTRIES[k]["case"]
    ctrl, orecs, osbr = M.oracle_of(S, k)
    base = PBASE + 100 * (len(ENTRIES) + 61)
    job = M.job_of(S, case, ctrl, base)
    t = PM.glue_layout(case)
    pns = upload_case(gpu, case, base)
    try:
        ticket, ptr, nbytes = gpu.submit_packed(job, _layout(t), lane=1, wait=False)
        try:
            gpu_ms, copy_ms = C.c_float(float("nan")), C.c_float(float("nan"))
            st = gpu.lib.svtme_ticket_wait_timed(gpu.ctx, ticket, C.byref(gpu_ms), C.byref(copy_ms))
            assert st == 0, gpu.lib.svtme_last_error()
            print("gpu_ms", gpu_ms.value, "copy_ms", copy_ms.value)
            assert math.isfinite(gpu_ms.value) and gpu_ms.value > 0
            assert math.isfinite(copy_ms.value) and copy_ms.value >= 0
            assert_decodes_to(C.string_at(ptr, nbytes), t, orecs, osbr, "timed wait")
            for bad in (ticket, 0, ticket + 1000):
                st = gpu.lib.svtme_ticket_wait_timed(gpu.ctx, bad, C.byref(gpu_ms), C.byref(copy_ms))
                assert st & 0xFFFFFFFF == BAD_PARAMETER, bad
                st = gpu.lib.svtme_ticket_wait(gpu.ctx, bad)
                assert st & 0xFFFFFFFF == BAD_PARAMETER, bad
        finally:
            gpu.lib.svtme_host_free(ptr)
        assert_decodes_to(gpu.submit_packed(job, _layout(t)), t, orecs, osbr, "after the refused waits")
    finally:
        release_all(gpu, pns)


@pytest.mark.gpu
def test_gpu_pageable_host_out(gpu):
    """host_out "should be page-locked": a plain numpy buffer holds the same bytes after svtme_ticket_wait."""
    k = IDS.index("d_npus5_general")
    case = ENTRIES[k]["case"]
    ctrl, orecs, osbr = M.oracle_of(S, k)
    base = PBASE + 100 * (len(ENTRIES) + 62)
    job = M.job_of(S, case, ctrl, base)
    pns = upload_case(gpu, case, base)
    try:
        for kind, t in case_layouts(k):
            locked = gpu.submit_packed(job, _layout(t))
            out = np.full(len(locked), 0xA5, np.uint8)
            ticket = C.c_uint64()
            st = gpu.lib.svtme_submit_picture_packed_async(gpu.ctx, 0, C.byref(job), C.byref(_layout(t)),
                                                           out.ctypes.data, C.byref(ticket))
            assert st == 0 and ticket.value, gpu.lib.svtme_last_error()
            assert gpu.lib.svtme_ticket_wait(gpu.ctx, ticket.value) == 0, gpu.lib.svtme_last_error()
            assert out.tobytes() == locked, kind
            assert_decodes_to(locked, t, orecs, osbr, kind)
    finally:
        release_all(gpu, pns)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(72, 40), (200, 136)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_registered_host_memory(gpu, size):
    """svtme_host_register: svtme_picture_upload_async from a registered, page-aligned numpy buffer
    builds the pyramid of tests/pyramid_model.py, a job on the pictures equals the oracle, and after
    svtme_sync the range is unregistered; null and zero-byte arguments are refused."""
    w, h = size
    case = M._case(f"registered_{w}x{h}", w, h, "pan", (7,), (9,), 8, {}, tl=1)
    frames = M.frames_of(S, case)
    ctrl = M.controls_of(S, case)
    orecs, osbr = M.run_cpu(S, case, "oracle", frames=frames, ctrl=ctrl)
    base = PBASE + 100 * (len(ENTRIES) + 63)
    page = 4096
    nbytes = (len(frames) * w * h + page - 1) // page * page
    keep = np.zeros(nbytes + page, np.uint8)
    a = (-keep.ctypes.data) % page
    buf = keep[a:a + nbytes]
    assert buf.ctypes.data % page == 0
    lib = gpu.lib
    for p, n in ((None, nbytes), (buf.ctypes.data, 0)):
        assert lib.svtme_host_register(p, n) & 0xFFFFFFFF == BAD_PARAMETER
    assert lib.svtme_host_unregister(None) & 0xFFFFFFFF == BAD_PARAMETER
    assert lib.svtme_host_register(buf.ctypes.data, nbytes) == 0, lib.svtme_last_error()
    registered, pns = True, []
    try:
        for i, (t, f) in enumerate(sorted(frames.items())):
            view = buf[i * w * h:(i + 1) * w * h].reshape(h, w)
            view[:] = f
            gpu.upload_async(base + t, view)
            pns.append(base + t)
        gpu.sync()
        for t, f in frames.items():
            for lv, want in enumerate(PYR.pyramid(f)):
                assert np.array_equal(gpu.download(base + t, lv), want), (t, lv)
        job = M.job_of(S, case, ctrl, base)
        tl = PM.glue_layout(case)
        assert_decodes_to(gpu.submit_packed(job, _layout(tl)), tl, orecs, osbr, case["name"])
        gpu.sync()
        assert lib.svtme_host_unregister(buf.ctypes.data) == 0, lib.svtme_last_error()
        registered = False
    finally:
        if registered:
            gpu.sync()
            lib.svtme_host_unregister(buf.ctypes.data)
        release_all(gpu, pns)
