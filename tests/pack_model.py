"""A numpy decoder of the packed job output (svtme_submit_picture(s)_packed_async), written from the
layout comment of include/svtme.h (svtme_pack_layout) alone.

Independent of svtme.pack_outputs / svtme.packed_sb_bytes and of k_pack: the stride, the section
offsets and the structs are restated here. SB k of a job starts at byte k * stride:
    R records (704 bytes each) or R record tails (the last 24 bytes of a record)
    when sb_results: 6 uint32 | me_distortion[85] | me_mv_array[n_pus][max_refs] |
                     2 flag bytes, 2 zero bytes | total_me_candidate_index[n_pus] |
                     me_candidate_array[n_pus][max_cand]
    zero bytes up to the next multiple of 16.

unpack() decodes a buffer, expect() cuts a job's full outputs (records [n_sb][R], SB results
[n_sb]) to what a layout carries, mismatches() compares the two. The keyword arguments of unpack()
and expect() build deliberately wrong decoders (the discrimination test of tests/test_pack.py);
the defaults are the model.

layouts_of() gives the layouts every case of tests/me_sweep.py is packed with: the one the
encoder glue passes (layout_of, integration/svtme_svt_glue.c), a seeded draw, and for a few cases
a directed one; tests/golden/pack_layouts.json lists them.
"""
import numpy as np

from me_sweep import Rng

PU_COUNT = 85
U32 = 0xFFFFFFFF

TAIL_FIELDS = [("hme_sad", "<u8"), ("hme_sc_x", "<i2"), ("hme_sc_y", "<i2"), ("zz_sad", "<u4"), ("searched", "u1"),
               ("do_ref", "u1"), ("tf_early_exit", "u1"), ("pad", "u1", (5,))]
TAIL_DTYPE = np.dtype(TAIL_FIELDS)  # svtme_record_tail
REF_RECORD_DTYPE = np.dtype([("best_sad", "<u4", (PU_COUNT,)), ("best_mv", "<u4", (PU_COUNT,))] + TAIL_FIELDS)
assert TAIL_DTYPE.itemsize == 24 and REF_RECORD_DTYPE.itemsize == 704
TAIL_OFFSET = REF_RECORD_DTYPE.itemsize - TAIL_DTYPE.itemsize  # 680: a tail is a record's last 24 bytes

DIST6 = ["me_8x8_cost_variance", "rc_me_distortion", "me_64x64_distortion", "me_32x32_distortion",
         "me_16x16_distortion", "me_8x8_distortion"]
ORDER = ("dist6", "me_distortion", "me_mv_array", "flags", "total", "cands")  # the SB-result sections


def layout_tuple(layout) -> tuple:
    """(n_pus, max_cand, max_refs, full_records, sb_results) of a 5-sequence or of a svtme_pack_layout."""
    if hasattr(layout, "n_pus"):
        return (layout.n_pus, layout.max_cand, layout.max_refs, layout.full_records, layout.sb_results)
    return tuple(int(v) for v in layout)


def sections(layout, R: int, order=ORDER, align: int = 16, npus=None):
    """-> ({section: byte offset in the SB's block}, bytes used, stride)."""
    n_pus, max_cand, max_refs, full, sb = layout_tuple(layout)
    if npus is not None:
        n_pus = npus
    o = R * (REF_RECORD_DTYPE.itemsize if full else TAIL_DTYPE.itemsize)
    off = {}
    if sb:
        size = {"dist6": 4 * 6, "me_distortion": 4 * PU_COUNT, "me_mv_array": 4 * n_pus * max_refs, "flags": 4,
                "total": n_pus, "cands": n_pus * max_cand}
        for name in order:
            off[name] = o
            o += size[name]
    return off, o, (o + align - 1) // align * align


def stride_of(layout, R: int) -> int:
    return sections(layout, R)[2]


def unpack(buf, layout, R: int, n_sb: int, *, order=ORDER, align: int = 16, mv_row=None, cand_row=None, npus=None,
           slot_major: bool = False):
    """-> (records or tails [n_sb][R], {field: array with a leading n_sb axis}); `slack` holds every
    byte the layout defines as zero. Raises ValueError when the buffer is not n_sb strides long."""
    n_pus, max_cand, max_refs, full, sb = layout_tuple(layout)
    wrong = (order, align, mv_row, cand_row, npus, slot_major) != (ORDER, 16, None, None, None, False)
    if npus is not None:
        n_pus = npus
    off, used, stride = sections(layout, R, order, align, npus)
    a = np.frombuffer(bytes(buf), np.uint8)
    if a.size != n_sb * stride and not wrong:
        raise ValueError(f"{a.size} bytes for {n_sb} SBs of {stride}")
    # (the wrong decoders read past an SB's block, or past the buffer: those bytes read as zero)
    width = stride + 4 * PU_COUNT * 8 + PU_COUNT * 24
    flat = np.concatenate([a, np.zeros(1, np.uint8)])
    blocks = flat[np.minimum(np.arange(n_sb)[:, None] * stride + np.arange(width)[None, :], a.size)]

    def u8(o):
        return blocks[:, np.asarray(o)]

    def u32(o):
        o = np.asarray(o)
        return sum(blocks[:, o + b].astype(np.uint32) << np.uint32(8 * b) for b in range(4))

    dt = REF_RECORD_DTYPE if full else TAIL_DTYPE
    recs = np.ascontiguousarray(blocks[:, :R * dt.itemsize]).view(dt).reshape(n_sb, R)
    if slot_major:
        recs = recs.reshape(R, n_sb).T
    f = {}
    if sb:
        for i, name in enumerate(DIST6):
            f[name] = u32(off["dist6"] + 4 * i)
        f["me_distortion"] = u32(off["me_distortion"] + 4 * np.arange(PU_COUNT))
        pu = np.arange(n_pus)[:, None]
        f["me_mv_array"] = u32(off["me_mv_array"] + 4 * (pu * (mv_row or max_refs) + np.arange(max_refs)[None, :]))
        f["stationary_block_present"] = u8(off["flags"])
        f["rc_me_allow_gm"] = u8(off["flags"] + 1)
        f["total_me_candidate_index"] = u8(off["total"] + np.arange(n_pus))
        f["me_candidate_array"] = u8(off["cands"] + pu * (cand_row or max_cand) + np.arange(max_cand)[None, :])
        f["slack"] = np.concatenate([u8(off["flags"] + 2 + np.arange(2)), blocks[:, used:stride]], axis=1)
    else:
        f["slack"] = blocks[:, used:stride]
    return recs, f


def tails_of(recs: np.ndarray, tail_offset: int = TAIL_OFFSET) -> np.ndarray:
    """svtme_record_tail of every record: its last 24 bytes."""
    raw = np.frombuffer(recs.tobytes() + bytes(TAIL_DTYPE.itemsize), np.uint8)
    start = np.arange(recs.size) * REF_RECORD_DTYPE.itemsize + tail_offset
    return raw[start[:, None] + np.arange(TAIL_DTYPE.itemsize)[None, :]].copy().view(TAIL_DTYPE).reshape(recs.shape)


def canonical(recs: np.ndarray) -> np.ndarray:
    """The records with best_sad = 0xFFFFFFFF on every slot that was not searched: the header's
    promise; the reference leaves those words undefined (svtme.records_checksum does the same)."""
    r = recs.copy()
    r["best_sad"][~r["searched"].astype(bool)] = U32
    return r


def expect(recs: np.ndarray, sbr, layout, tail_offset: int = TAIL_OFFSET):
    """A job's full outputs cut to the layout: what unpack() must return, without `slack`."""
    n_pus, max_cand, max_refs, full, sb = layout_tuple(layout)
    recs = canonical(recs)
    f = {}
    if sb:
        for name in DIST6 + ["me_distortion", "stationary_block_present", "rc_me_allow_gm"]:
            f[name] = sbr[name]
        f["me_mv_array"] = sbr["me_mv_array"][:, :n_pus, :max_refs]
        f["total_me_candidate_index"] = sbr["total_me_candidate_index"][:, :n_pus]
        f["me_candidate_array"] = sbr["me_candidate_array"][:, :n_pus, :max_cand]
    return (recs if full else tails_of(recs, tail_offset)), f


def mismatches(got, want) -> list:
    """Every field of the records / tails (their pad bytes included) and of the SB results, exactly."""
    (grecs, gf), (wrecs, wf) = got, want
    errs = []
    if grecs.shape != wrecs.shape or grecs.dtype != wrecs.dtype:
        return [f"records {grecs.shape} {grecs.dtype.itemsize} vs {wrecs.shape} {wrecs.dtype.itemsize}"]
    for name in wrecs.dtype.names:
        if not np.array_equal(grecs[name], wrecs[name]):
            idx = tuple(np.argwhere(grecs[name] != wrecs[name])[0])
            errs.append(f"{name} at {idx}: {grecs[name][idx]} vs {wrecs[name][idx]}")
    if sorted(k for k in gf if k != "slack") != sorted(wf):
        return errs + ["fields " + ",".join(sorted(gf)) + " vs " + ",".join(sorted(wf))]
    for name, w in wf.items():
        g = gf[name]
        if g.shape != w.shape:
            errs.append(f"sb.{name} {g.shape} vs {w.shape}")
        elif not np.array_equal(g, w):
            idx = tuple(np.argwhere(g != w)[0])
            errs.append(f"sb.{name} at {idx}: {g[idx]} vs {w[idx]}")
    return errs


# ----------------------------------------------------------------------------
# the layouts of the sweep's cases
# ----------------------------------------------------------------------------
N_PUS = [1, 4, 5, 20, 21, 64, 84, 85]
LAYOUT_SEED = 7000  # case k draws with Rng(LAYOUT_SEED + k)

# the largest block (R = 7, whole records, every PU, MV and candidate slot: 9728 bytes), which no
# draw reached; also the poison job of the stale-bytes test
LARGEST = (85, 23, 7, 1, 1)
DIRECTED = {"d_cand23": LARGEST}


def slots_of(case) -> int:
    return len(case["l0"]) + len(case["l1"])


def glue_layout(case) -> tuple:
    """layout_of (integration/svtme_svt_glue.c) for the case's job: TF-ME reads whole records alone;
    open-loop ME reads tails and the SB results its MeSbResults allocation holds (pcs.c:91-117,
    svt_aom_get_max_allocated_me_refs over the reference counts)."""
    if case["tf"]:
        return (0, 0, 0, 1, 0)
    n0, n1 = max(len(case["l0"]), 1), len(case["l1"])
    max_cand = n0 + n1 + n0 * n1 + (n0 - 1) + (1 if n1 == 3 else 0)
    return (85 if case["e16"] and case["e8"] else 21 if case["e16"] else 5, max_cand, n0 + n1, 0, 1)


def drawn_layout(k: int) -> tuple:
    g = Rng(LAYOUT_SEED + k)
    return (g.pick(N_PUS), 1 + g.below(23), 1 + g.below(7), g.below(2), g.below(2))


def layouts_of(case, k: int) -> dict:
    out = {"glue": list(glue_layout(case)), "drawn": list(drawn_layout(k))}
    if case["name"] in DIRECTED:
        out["directed"] = list(DIRECTED[case["name"]])
    return out


def golden(cases) -> dict:
    """The content of tests/golden/pack_layouts.json for the sweep's case list."""
    rows = [dict({"name": c["name"], "R": slots_of(c)}, **layouts_of(c, k)) for k, c in enumerate(cases)]
    return {"fields": ["n_pus", "max_cand", "max_refs", "full_records", "sb_results"], "seed": LAYOUT_SEED,
            "cases": rows}


if __name__ == "__main__":  # rewrite the committed list: python tests/pack_model.py
    import json
    import os

    import me_sweep

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_layouts.json"), "w") as fh:
        g = golden(me_sweep.cases())
        head = json.dumps({k: v for k, v in g.items() if k != "cases"})
        fh.write(head[:-1] + ', "cases": [\n' + ",\n".join(json.dumps(r) for r in g["cases"]) + "\n]}\n")
