"""k_hme's tile loops after the VALU cuts, against the CPU oracle byte for byte (records and
per-SB results): the wave-uniform votes of the 1/16 and HME-L1 tiles (no position test where
every tile of a wavefront lies inside its area, no row selects in a full-height SB) and the
general paths they leave.

  192 x 136 (3 x 3 SBs, the last SB row 8 lines high): every SB has a pre-HME region or an
      HME-L0 quadrant clamped at the picture border and the last row is partial-height;
  the smallest picture (width and height multiples of 64) in which some SB has all its
      pre-HME regions and HME-L0 quadrants inside the padded 1/16 plane for a reference at
      distance 1, derived below from prehme_sa_cfg, hme_l0_sa and the plane padding;
  the same picture 56 lines lower: interior columns meet a partial-height last row;
  records alone, and the four-wave instance (PATH_HME_4WAVES).

The static counts of scripts/isa_phase_count.py are checked without a GPU."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QSAD_PARENT = 944  # v_qsad* of k_hme<true,true,true,false,3> before the cuts


def lib_of(S):
    lib = S.load_product()
    lib.svtme_hme_fused.argtypes = [C.POINTER(S.Job)]
    lib.svtme_hme_fused.restype = C.c_bool
    lib.svtme_fp_parts.argtypes = [C.POINTER(S.Controls)]
    lib.svtme_fp_parts.restype = C.c_uint32
    return lib


def controls(S, preset, w, h):
    return S.derive_controls(preset, 35, S.input_resolution_of(w, h), 1)


def inside_mask(S, ctrl, w, h):
    """Per SB (rows x columns): every pre-HME region and the whole HME-L0 area of a reference at
    distance 1 lies inside the padded 1/16 plane, that is prehme_core and hme_level_0 clamp
    nothing (their tests, restated: the left / top edge against the padding less one, the
    right / bottom edge against the plane)."""
    pw, ph, pad = w // 4, h // 4, S.PAD_SIXTEENTH - 1
    sox = np.arange((w + 63) // 64)[None, :] * 16
    soy = np.arange((h + 63) // 64)[:, None] * 16
    f = 1  # scaled_dist(1): 5 / 8 rounded up
    ok = np.ones((soy.shape[0], sox.shape[1]), bool)

    def inside(x0, y0, aw, ah):
        return (x0 >= -pad) & (x0 <= pw - 1) & (x0 + aw <= pw) & (y0 >= -pad) & (y0 <= ph - 1) & (y0 + ah <= ph)

    for k in range(2):  # prehme_core: the area centred on the block's origin
        a = ctrl.prehme_sa_cfg[k]
        aw = min(a.sa_min.width * f, a.sa_max.width)
        ah = min(a.sa_min.height * f, a.sa_max.height)
        ok &= inside(sox - (aw >> 1), soy - (ah >> 1), aw, ah)
    # get_hme_l0_search_area at distance 1 for list 0, reference 0 (no reduction), then the
    # num_hme_sa_w x num_hme_sa_h quadrants of hme_level_0 (width rounded up to 8)
    a = ctrl.hme_l0_sa
    nw, nh = ctrl.num_hme_sa_w, ctrl.num_hme_sa_h
    qw = min(((a.sa_min.width // nw) * f + 15) & ~15, ((a.sa_max.width // nw) + 15) & ~15)
    qh = min((a.sa_min.height // nh) * f, a.sa_max.height // nh)
    qw = (qw + 7) & ~7
    ok &= inside(sox - ((qw * nw) >> 1), soy - ((qh * nh) >> 1), qw * nw, qh * nh)
    return ok


@functools.lru_cache(maxsize=None)
def inner_size(S):
    """The smallest (width, height), multiples of 64, with an SB that inside_mask accepts."""
    best = None
    for h in range(64, 2049, 64):
        for w in range(64, 1025, 64):
            if inside_mask(S, controls(S, 8, w, h), w, h).any():
                if best is None or w * h < best[0] * best[1]:
                    best = (w, h)
                break
    assert best is not None
    return best


def make(S, ctrl, w, h, base, l0, l1):
    return S.case_job(ctrl, w, h, base + 8, [base + t for t in l0], [base + t for t in l1], 1)


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def run_case(S, gpu, w, h, preset, kind, l0, l1, paths=0, with_sb_results=True):
    ctrl = controls(S, preset, w, h)
    lib = lib_of(S)
    base = 9000
    frames = S.test_frames(kind, w, h, sorted(set([8] + list(l0) + list(l1))))
    job = make(S, ctrl, w, h, base, l0, l1)
    # the case runs the whole-pass k_hme
    assert lib.svtme_hme_fused(C.byref(job)) and lib.svtme_fp_parts(C.byref(job.ctrl)) == 1
    for t, f in frames.items():
        gpu.upload(base + t, f)
    try:
        gpu.set_paths(paths)
        recs, sbr = gpu.submit(job, with_sb_results=with_sb_results)
    finally:
        gpu.set_paths(0)
        for t in frames:
            gpu.release(base + t)
    pyr = {t: S.build_host_pyramid(f, "oracle") for t, f in frames.items()}
    refs = {(0, i): pyr[t] for i, t in enumerate(l0)}
    refs.update({(1, i): pyr[t] for i, t in enumerate(l1)})
    orecs, osbr = S.run_checker(make(S, ctrl, w, h, 0, l0, l1), pyr[8], refs, "oracle", nthreads=8)
    assert same_bytes(orecs, recs), S.compare_records(orecs, recs)[:5]
    if with_sb_results:
        errs = S.compare_records(orecs, recs, osbr, sbr)
        assert not errs, errs[:5]
        assert same_bytes(osbr, sbr)


REFS = {"1+1": ((7,), (9,)), "2+2": ((7, 6), (9, 10))}


def test_sizes(svtme):
    """The picture sizes the GPU cases stand on: no SB of 192 x 136 has every 1/16 window inside
    the plane; the derived size has one that does and one that does not, also 56 lines lower."""
    S = svtme
    assert not inside_mask(S, controls(S, 8, 192, 136), 192, 136).any()
    assert not inside_mask(S, controls(S, 6, 192, 136), 192, 136).any()
    w, h = inner_size(S)
    assert w % 64 == 0 and h % 64 == 0
    for hh in (h, h - 56):
        m = inside_mask(S, controls(S, 8, w, hh), w, hh)
        assert m.any() and not m.all(), (w, hh, m)
    # no smaller picture has one
    for ww, hh in ((w - 64, h), (w, h - 64)):
        if ww >= 64 and hh >= 64:
            assert not inside_mask(S, controls(S, 8, ww, hh), ww, hh).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["pan", "noise"])
@pytest.mark.parametrize("preset,refs", [(8, "2+2"), (6, "1+1")])
def test_clamped_partial_height(svtme, gpu, preset, refs, kind):
    run_case(svtme, gpu, 192, 136, preset, kind, *REFS[refs])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["pan", "hpan"])
@pytest.mark.parametrize("refs", ["1+1", "2+2"])
def test_inner_waves(svtme, gpu, refs, kind):
    w, h = inner_size(svtme)
    run_case(svtme, gpu, w, h, 8, kind, *REFS[refs])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["pan", "hpan"])
@pytest.mark.parametrize("refs", ["1+1", "2+2"])
def test_inner_columns_partial_height(svtme, gpu, refs, kind):
    w, h = inner_size(svtme)
    run_case(svtme, gpu, w, h - 56, 8, kind, *REFS[refs])


@pytest.mark.gpu
def test_records_alone(svtme, gpu):
    w, h = inner_size(svtme)
    run_case(svtme, gpu, w, h, 8, "pan", *REFS["2+2"], with_sb_results=False)


@pytest.mark.gpu
def test_forced_four_waves(svtme, gpu):
    w, h = inner_size(svtme)
    run_case(svtme, gpu, w, h - 56, 8, "hpan", *REFS["2+2"], paths=svtme.PATH_HME_4WAVES)


def test_static_counts():
    """scripts/isa_phase_count.py finds the three-wave whole-pass instance; it has no more
    v_qsad* than before the cuts, 64 VGPRs and no scratch."""
    spec = importlib.util.spec_from_file_location("isa_phase_count", os.path.join(ROOT, "scripts", "isa_phase_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = mod.count(mod.compile_asm(), "k_hme<true,true,true,false,3>")
    assert r is not None
    assert r["total"]["qsad"] <= QSAD_PARENT, r["total"]
    assert r["vgprs"] == 64 and r["scratch"] == 0, (r["vgprs"], r["scratch"])
