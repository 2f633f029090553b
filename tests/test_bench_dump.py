"""bench.py --dump-outputs on CPU: dump_outputs turns the bytes of a step's
output buffer (per picture its records, then its per-SB results) into one
float .npy per field; every value exact, padding left out, a fixed sample of
the rows when the whole exceeds the size limit."""
import os

import numpy as np
import pytest

import bench


def _buffer(S, n_pic, count, R, with_sb, seed=1):
    rec_bytes = count * R * S.REF_RECORD_DTYPE.itemsize
    chunk = (rec_bytes + (count * S.SB_RESULT_DTYPE.itemsize if with_sb else 0) + 255) & ~255
    raw = np.random.default_rng(seed).integers(0, 256, n_pic * chunk, dtype=np.uint8)
    for p in range(n_pic):  # hme_sad, the one 64-bit field, is a SAD: within float64's 53 bits
        np.frombuffer(raw, S.REF_RECORD_DTYPE, count * R, p * chunk)["hme_sad"] >>= 11
    return raw, chunk, rec_bytes


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("with_sb", (True, False))
def test_dump_is_exact(svtme, tmp_path, with_sb):
    S = svtme
    n_pic, count, R, begin = 3, 37, 2, 5
    raw, chunk, rec_bytes = _buffer(S, n_pic, count, R, with_sb)
    bench.dump_outputs(str(tmp_path), S, raw, n_pic, chunk, rec_bytes, begin, count, R, with_sb)
    out = _load(tmp_path)
    want = {"rows"} | {"records_" + f for f in S.REF_RECORD_DTYPE.names if f != "pad"}
    if with_sb:
        want |= {"sb_" + f for f in S.SB_RESULT_DTYPE.names if not f.startswith("pad")}
    assert set(out) == want
    rows = out["rows"]
    assert np.array_equal(rows[:, 0], np.repeat(np.arange(n_pic), count))
    assert np.array_equal(rows[:, 1], np.tile(begin + np.arange(count), n_pic))
    for p in range(n_pic):
        recs = np.frombuffer(raw, S.REF_RECORD_DTYPE, count * R, p * chunk).reshape(count, R)
        sl = slice(p * count, (p + 1) * count)
        for f in S.REF_RECORD_DTYPE.names:
            if f == "pad":
                continue
            a = out["records_" + f][sl]
            assert a.dtype == (np.float64 if recs[f].dtype.itemsize >= 4 else np.float32)
            exp = recs[f].copy()
            if f == "best_sad":  # undefined where the reference was not searched
                exp[recs["searched"] == 0] = 0xFFFFFFFF
            assert np.array_equal(a, exp) and np.array_equal(a.astype(exp.dtype), exp)
        if with_sb:
            sbr = np.frombuffer(raw, S.SB_RESULT_DTYPE, count, p * chunk + rec_bytes)
            for f in S.SB_RESULT_DTYPE.names:
                if not f.startswith("pad"):
                    assert np.array_equal(out["sb_" + f][sl].astype(sbr[f].dtype), sbr[f])


def test_dump_samples_within_the_limit(svtme, tmp_path, monkeypatch):
    S = svtme
    n_pic, count, R = 2, 64, 4
    raw, chunk, rec_bytes = _buffer(S, n_pic, count, R, True)
    monkeypatch.setattr(bench, "DUMP_BYTES", 400_000)  # less than the 128 rows need
    a, b = tmp_path / "a", tmp_path / "b"
    for d in (a, b):
        bench.dump_outputs(str(d), S, raw, n_pic, chunk, rec_bytes, 0, count, R, True)
    oa, ob = _load(a), _load(b)
    rows = oa["rows"]
    k = len(rows)
    assert 0 < k < n_pic * count
    assert sum(os.path.getsize(a / f) - 128 for f in os.listdir(a)) <= 400_000  # (128: a .npy header)
    flat = rows[:, 0] * count + rows[:, 1]
    assert np.all(np.diff(flat) > 0)  # distinct rows in ascending order
    for name in oa:  # the same rows in every run
        assert len(oa[name]) == k and np.array_equal(oa[name], ob[name])
    p, sb = int(rows[k // 2, 0]), int(rows[k // 2, 1])
    sbr = np.frombuffer(raw, S.SB_RESULT_DTYPE, count, p * chunk + rec_bytes)
    assert np.array_equal(oa["sb_me_mv_array"][k // 2], sbr["me_mv_array"][sb])


def test_dump_default_limit():
    assert bench.DUMP_BYTES <= 64_000_000
