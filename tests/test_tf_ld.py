"""Low-delay temporal filtering: svtme_tf_filter_ld and svtme_tf_window_ld (include/svtme.h), the path of
produce_temporally_filtered_pic_ld: co-located prediction, 32x32 luma variances, the zz-based weights, at 8
and 10 bit, luma alone or with 4:2:0 chroma.

Expected values are the fixtures tests/golden/tfld_cases.{json,npz}, made by the reference's own functions
(tests/golden/make_golden_tfld.py). Beside them stands a model in numpy and Python integers
(tests/tfld_model.py) that shares no code with the generator. CPU tests pin the ABI, the argument checks that
need no context, the fixtures and the model to the fixtures; GPU tests compare the calls with the fixtures,
the model, each other and the calls that were there before. Every comparison is exact.
"""
import ctypes as C
import itertools
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
import make_golden_tfld as GL  # noqa: E402
import test_tf_window as TW  # noqa: E402  (its window helpers; its tests are collected from its own file)
import test_tff_10bit_chroma as TC  # noqa: E402  (its download helpers, likewise)
import tfld_model as ML  # noqa: E402

DOC = json.load(open(os.path.join(GOLD, "tfld_cases.json")))
CASES = DOC["cases"]
BAD_PARAMETER = 0x80001005
BASE = 17000  # picture numbers of this file's uploads
OUT = 900     # + BASE: the result picture of a window into a fresh number
SYMBOLS = ("svtme_tf_filter_ld", "svtme_tf_window_ld")
MODES = [(bd, chroma) for bd, chroma, _ in GL.MODES]
MODE_IDS = [f"{bd}bit{'_yuv' if chroma else ''}" for bd, chroma in MODES]


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLD, "tfld_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def case_by_id(name):
    return next(c for c in CASES if c["id"] == name)


def plane_names(ctl: dict):
    return ("y", "cb", "cr") if ctl["chroma"] else ("y",)


# ----------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------
def test_tfld_symbols_exported(svtme):
    lib = svtme.load_product()
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []


_STRUCTS = {"svtme_tf_ld_controls": ("TfLdControls", 16), "svtme_tf_ld_out": ("TfLdOut", 48)}

# each new function assigned to a pointer of the type the Python prototypes assume: a header that
# differs does not compile
_PROTO_PROGRAM = r"""
svtme_status (*p_filter)(svtme_ctx *, uint64_t, const uint64_t *, uint32_t, uint32_t, uint32_t,
                         const svtme_tf_ld_controls *, const svtme_tf_ld_out *) = svtme_tf_filter_ld;
svtme_status (*p_window)(svtme_ctx *, uint64_t, const uint64_t *, uint32_t, uint32_t, uint32_t,
                         const svtme_tf_ld_controls *, uint64_t, const svtme_tf_ld_out *) = svtme_tf_window_ld;
"""


def test_tfld_struct_sizes_offsets_and_prototypes_equal_the_header(svtme, tmp_path):
    lines = []
    for cname, (pyname, _) in _STRUCTS.items():
        lines.append(f'printf("sizeof {cname} %zu\\n", sizeof({cname}));')
        for field, _ in getattr(svtme, pyname)._fields_:
            lines.append(f'printf("{cname}.{field} %zu\\n", offsetof({cname}, {field}));')
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svtme.h"\n' + _PROTO_PROGRAM +
                   "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "abi.o")], check=True)  # the prototypes; the functions themselves are not linked
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svtme.h"\nint main(void) {\n' + "\n".join(lines) +
                   "\nreturn 0;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        key, val = line.rsplit(" ", 1)
        got[key] = int(val)
    for cname, (pyname, size) in _STRUCTS.items():
        st = getattr(svtme, pyname)
        assert got["sizeof " + cname] == C.sizeof(st) == size, cname
        for field, _ in st._fields_:
            assert got[f"{cname}.{field}"] == getattr(st, field).offset, (cname, field)
    lib, vp, u32, u64 = svtme.load_product(), C.c_void_p, C.c_uint32, C.c_uint64
    head = [vp, u64, C.POINTER(u64), u32, u32, u32, C.POINTER(svtme.TfLdControls)]
    want = {"svtme_tf_filter_ld": head + [C.POINTER(svtme.TfLdOut)],
            "svtme_tf_window_ld": head + [u64, C.POINTER(svtme.TfLdOut)]}
    for name, argtypes in want.items():
        assert list(getattr(lib, name).argtypes) == argtypes, name
        assert getattr(lib, name).restype is C.c_int32, name
    ctl = svtme.TfLdControls.from_dict({"tf_decay_factor_fp16": [1, 2, 3], "sub_sampling_shift": 1, "bit_depth": 10,
                                        "chroma": 1})
    assert ctl.as_dict() == {"tf_decay_factor_fp16": [1, 2, 3], "sub_sampling_shift": 1, "bit_depth": 10, "chroma": 1}


def _controls(svtme, **over):
    d = dict({"tf_decay_factor_fp16": [GL.MID, GL.MID2, 1023], "sub_sampling_shift": 1, "bit_depth": 8, "chroma": 1},
             **over)
    return svtme.TfLdControls.from_dict(d)


def _ld_call(svtme, lib, ctx, window, refs=(BASE + 7,), n=None, ctl=None, null=None, w=128, h=128, centre=BASE + 8,
             strides=None, out_pn=BASE + OUT):
    """-> the status of svtme_tf_filter_ld (window False) or svtme_tf_window_ld; on an error no output
    may be touched."""
    ctl = ctl if ctl is not None else _controls(svtme)
    slots = max(len(refs), svtme.MAX_BATCH_JOBS + 1)
    arr = (C.c_uint64 * slots)(*refs)
    W, H = svtme.align8(max(w, 1)), svtme.align8(max(h, 1))
    sy, scb, scr = strides or (w, (w + 1) >> 1, (w + 1) >> 1)
    bufs = [np.full(H * max(sy, W) + 64, 0x5A5A, np.uint16) for _ in range(3)]
    var32 = np.full(slots * svtme.sb_total(W, H) * 4, 0x5A5A5A5A, np.uint32)
    out = svtme.TfLdOut(y=None if null == "y" else bufs[0].ctypes.data, cb=bufs[1].ctypes.data, cr=bufs[2].ctypes.data,
                        y_stride=sy, cb_stride=scb, cr_stride=scr, var32=var32.ctypes.data)
    args = [None if null == "ctx" else ctx, centre, None if null == "refs" else arr, len(refs) if n is None else n, w, h,
            None if null == "controls" else C.byref(ctl)]
    if window:
        st = lib.svtme_tf_window_ld(*args, out_pn, None if null == "out" else C.byref(out))
    else:
        st = lib.svtme_tf_filter_ld(*args, None if null == "out" else C.byref(out))
    if st:
        assert all((b == 0x5A5A).all() for b in bufs) and (var32 == 0x5A5A5A5A).all()
        assert lib.svtme_last_error().decode() != ""
    return st & 0xFFFFFFFF


def _bad_calls(svtme, window: bool):
    """The refusals that need no context: (what, keyword arguments of _ld_call)."""
    many = tuple(BASE + 20 + k for k in range(svtme.MAX_BATCH_JOBS + 1))
    for null in ("ctx", "refs", "controls") + (() if window else ("out", "y")):
        yield "null " + null, dict(null=null)
    yield "n 0", dict(n=0)
    yield "n 17", dict(refs=many)
    if window:
        for w, h in ((0, 128), (128, 0), (16385, 128), (128, 16385)):
            yield f"source size {w}x{h}", dict(w=w, h=h)
        yield "the result among the references", dict(refs=(BASE + 7, BASE + OUT))
    else:
        for w, h in ((0, 128), (128, 0), (124, 128), (128, 67), (16392, 128), (128, 16392)):
            yield f"size {w}x{h}", dict(w=w, h=h)
    for bd in (0, 9, 12, 16):
        yield f"bit_depth {bd}", dict(ctl=_controls(svtme, bit_depth=bd))
    yield "chroma 2", dict(ctl=_controls(svtme, chroma=2))
    yield "sub_sampling_shift 2", dict(ctl=_controls(svtme, sub_sampling_shift=2))
    yield "pad 1", dict(ctl=_controls(svtme, pad=1))
    yield "y_stride under the width", dict(strides=(127, 64, 64))
    yield "cb_stride under the chroma width", dict(strides=(128, 63, 64))
    yield "cr_stride under the chroma width", dict(strides=(128, 64, 63))
    yield "the centre among the references", dict(refs=(BASE + 7, BASE + 8))


def _context_free_errors(svtme, lib, ctx):
    for window in (False, True):
        for what, kw in _bad_calls(svtme, window):
            assert _ld_call(svtme, lib, ctx, window, **kw) == BAD_PARAMETER, (window, what)


def test_tfld_bad_parameters_without_a_device(svtme):
    """The checks that need no context run before the context is touched: a block of zero bytes
    stands in for it."""
    lib = svtme.load_product()
    fake = C.create_string_buffer(64)
    _context_free_errors(svtme, lib, C.cast(fake, C.c_void_p))
    assert fake.raw == bytes(64)


def test_tfld_case_list_matches_generator():
    assert CASES == GL.case_dicts()
    shapes = {(c["w"], c["h"], len(c["refs"]), c["controls"]["bit_depth"], c["controls"]["chroma"]) for c in CASES}
    for bd, chroma in MODES:
        assert shapes >= {(64, 64, 1, bd, chroma), (72, 40, 1, bd, chroma), (136, 72, 3, bd, chroma)}
        assert ((8, 8, 1, bd, chroma) in shapes) == bool(chroma)  # yuv only
    assert all(c["controls"]["sub_sampling_shift"] == 1 for c in CASES if c["base"] == "ld72")
    kinds = {(c["kind"], c["controls"]["bit_depth"]) for c in CASES}
    assert kinds >= {("same", 8), ("same", 10), ("dc", 8), ("dc", 10), ("clip", 10)} and ("clip", 8) not in kinds
    decays = {d for c in CASES for d in c["controls"]["tf_decay_factor_fp16"]}
    assert decays == {0, 1023, GL.MID, GL.MID2, 0x7FFFFFFF}


def test_tfld_coverage_counts_are_all_non_zero():
    assert set(DOC["coverage"]) == set(GL.COVERAGE_KEYS) | set(GL.BETWEEN_DISTINCT)
    assert [k for k in GL.COVERAGE_KEYS if not DOC["coverage"][k] > 0] == []
    assert [k for k in GL.BETWEEN_DISTINCT if DOC["coverage"][k] < 3] == []
    assert set(DOC["coverage_per_case"]) == {c["id"] for c in CASES}
    for k in GL.COVERAGE_KEYS:
        assert sum(c.get(k, 0) for c in DOC["coverage_per_case"].values()) == DOC["coverage"][k], k


def test_tfld_fixture_shapes_and_contents(svtme, gold):
    names = [f"{c['id']}.{s}" for c in CASES for s in plane_names(c["controls"]) + ("var32",)]
    assert sorted(gold) == sorted(names + ["weights.in", "weights.out"])
    for case in CASES:
        W, H = svtme.align8(case["w"]), svtme.align8(case["h"])
        bd, name = case["controls"]["bit_depth"], case["id"]
        assert gold[name + ".y"].shape == (H, W)
        assert gold[name + ".var32"].shape == (len(case["refs"]), svtme.sb_total(W, H), 4)
        for plane in plane_names(case["controls"]):
            a = gold[f"{name}.{plane}"]
            assert a.dtype == (np.uint16 if bd == 10 else np.uint8) and a.max() < 1 << bd
            assert plane == "y" or a.shape == (H // 2, W // 2)
        if case["kind"] in ("same", "dc"):  # variance 0 although, in dc, the SSE is large
            frames = GL.luma_frames(case)
            diff = frames[case["refs"][-1]].astype(np.int64) - frames[case["centre"]]
            assert (gold[name + ".var32"] == 0).all() and (diff == diff[0, 0]).all()
            assert (diff[0, 0] != 0) == (case["kind"] == "dc")
        if case["kind"] == "clip":
            assert all((f == 0).any() and (f == 1023).any() for f in GL.luma_frames(case).values())
    assert os.path.getsize(os.path.join(GOLD, "tfld_cases.npz")) < 300_000


_model_results = {}


def model_case(case):
    if case["id"] not in _model_results:
        pics = GL.case_inputs(case)
        W, H = (case["w"] + 7) & ~7, (case["h"] + 7) & ~7
        _model_results[case["id"]] = ML.filter_window(pics[case["centre"]], [pics[r] for r in case["refs"]],
                                                      case["controls"], W, H)
    return _model_results[case["id"]]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_tfld_model_equals_fixture(gold, case):
    res = model_case(case)
    for name in plane_names(case["controls"]) + ("var32",):
        want = gold[f"{case['id']}.{name}"]
        assert res[name].dtype == want.dtype and np.array_equal(res[name], want), name
    cover, _ = GL.coverage_of(case, res, ML.variance32)
    assert {k: v for k, v in cover.items() if v} == DOC["coverage_per_case"][case["id"]]


def test_tfld_model_equals_fixture_weights(gold):
    tuples = gold["weights.in"]
    assert np.array_equal(tuples, GL.weight_tuples()) and tuples.shape == (500, 3)
    got = ML.model_weights(tuples)
    assert np.array_equal(got, gold["weights.out"])
    import tff_model as M
    for bd in (0, 113):  # the first 2 x 113 tuples walk the exp table, at 8 and at 10 bit
        assert got[bd:bd + 113].tolist() == [(e * 1000) >> 17 for e in M.EXP_TAB]
    assert got.max() == 500 and got.min() == 0 and ML.EXP_TAB == M.EXP_TAB


def test_tfld_variance_landmarks():
    """A constant offset has variance 0 at any size of the offset; the kept rows alone decide with the shift;
    the 10-bit variance clamps where its rounded terms cross."""
    rng = np.random.default_rng(5)
    c = rng.integers(100, 600, (32, 32))
    assert ML.variance32(c + 100, c, 0, 8) == ML.variance32(c + 100, c, 1, 8) == 0
    p = c.copy()
    p[1::2] += rng.integers(-50, 50, (16, 32))
    assert ML.variance32(p, c, 1, 8) == ML.variance32(p, c, 1, 10) == 0 and ML.variance32(p, c, 0, 8) > 0
    q = c + 52
    q[1, 1] -= 1
    q[4, 6] -= 1
    assert ML.variance32(q, c, 0, 10) == 0 and ML.variance32(q, c, 0, 8) == 2  # 10 bit: 173043 - 173056 before the clamp
    assert ML.weight(0, 0, 8) == ML.weight(3, 0, 8) == ML.weight(63, 0, 10) == 500
    assert ML.weight(4 * 112, 0, 8) == 0 and ML.weight(1 << 20, 0x7FFFFFFF, 8) == 500


@pytest.mark.skipif(not (ref_available() and GF.reference_headers()),
                    reason="oracle/_ref not built or the reference's headers absent (the offsetof probe needs them)")
def test_tfld_fixture_regenerates(gold):
    ar = GL.RefArithLD()
    for name in ("ld72_8c", "ld136_10c", "ld8_8c", "ld64_dc_10", "ld64_clip_10c"):
        case = case_by_id(name)
        res = GL.run_case(case, ar)
        for key in plane_names(case["controls"]) + ("var32",):
            assert res[key].tobytes() == gold[f"{name}.{key}"].tobytes(), (name, key)
    tuples = gold["weights.in"]
    assert GL.reference_weights(tuples[::7], ar).tobytes() == np.ascontiguousarray(gold["weights.out"][::7]).tobytes()


# ----------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------
def upload_case(gpu, case, base=BASE, luma=None, chroma=None) -> list:
    """The pictures of a case as its mode reads them: 8 bit the pyramid (and 8-bit chroma), 10 bit the MSB
    pyramid with the 16-bit plane (and 16-bit chroma) attached. -> the picture numbers less base."""
    ctl = case["controls"]
    luma = GL.luma_frames(case) if luma is None else luma
    uv = (GL.chroma_frames(case) if chroma is None else chroma) if ctl["chroma"] else None
    for t, f in luma.items():
        gpu.upload(base + t, f)
        if ctl["bit_depth"] == 10:
            gpu.attach_10bit(base + t, f)
        if uv is not None and ctl["bit_depth"] == 10:
            gpu.attach_chroma_10bit(base + t, uv[t][0], uv[t][1], case["w"], case["h"])
        elif uv is not None:
            gpu.upload_chroma(base + t, uv[t][0], uv[t][1], case["w"], case["h"])
    return list(luma)


def ld_controls(svtme, case):
    return svtme.TfLdControls.from_dict(case["controls"])


def run_filter(svtme, gpu, case, refs=None, **kw):
    refs = case["refs"] if refs is None else refs
    return gpu.tf_filter_ld(BASE + case["centre"], [BASE + r for r in refs], svtme.align8(case["w"]),
                            svtme.align8(case["h"]), ld_controls(svtme, case), **kw)


def state_keys(ctl: dict) -> list:
    """The planes a result picture of the mode holds (test_tff_10bit_chroma.state_of's names)."""
    keys = ["l0", "l1", "l2"] + (["y16"] if ctl["bit_depth"] == 10 else [])
    if ctl["chroma"]:
        keys += ["cb16", "cr16"] if ctl["bit_depth"] == 10 else ["cb8", "cr8"]
    return sorted(keys)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_tfld_filter_equals_the_fixture(svtme, gpu, gold, case):
    numbers = upload_case(gpu, case)
    try:
        res = run_filter(svtme, gpu, case)
    finally:
        TC.release(gpu, numbers, BASE)
    assert sorted(res) == sorted(plane_names(case["controls"]) + ("var32",))
    assert np.array_equal(res["var32"], gold[case["id"] + ".var32"]), case["id"]
    for name in plane_names(case["controls"]):
        TC.assert_planes_equal(res[name], gold[f"{case['id']}.{name}"], f"{case['id']} {name}")


def sweep_case(w, h, refs, bd, chroma, ss, seed) -> dict:
    rng = np.random.default_rng(seed)
    pick = lambda: int(rng.choice((0, 1023, 1024, GL.MID, GL.MID2, 20 << 10, 5000 << 10, 0x7FFFFFFF, 0xFFFFFFFF)))  # noqa: E731
    return {"id": f"sweep{seed}", "base": f"sweep{seed}", "kind": "frac", "w": w, "h": h, "centre": 8, "refs": list(refs),
            "controls": {"tf_decay_factor_fp16": [pick(), pick(), pick()], "sub_sampling_shift": ss, "bit_depth": bd,
                         "chroma": chroma}}


# size, references, sub-sampling shift, through the window call
SWEEP = [(64, 64, (7,), 0, False), (72, 40, (7, 9, 6), 1, False), (121, 67, (9,), 1, True), (121, 67, (7, 9, 6), 0, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("w,h,refs,ss,window", SWEEP, ids=[f"{w}x{h}_n{len(r)}_ss{s}" for w, h, r, s, _ in SWEEP])
def test_tfld_random_sweep_vs_model(svtme, gpu, w, h, refs, ss, window, mode):
    """Seeded controls on moving content against the model; the odd size goes through the window call, which
    aligns it itself and copies the true size out."""
    case = sweep_case(w, h, refs, mode[0], mode[1], ss, 1000 * w + 10 * len(refs) + ss)
    numbers = upload_case(gpu, case)
    try:
        if window:
            got = gpu.tf_window_ld(BASE + 8, [BASE + r for r in refs], w, h, ld_controls(svtme, case), BASE + OUT,
                                   want=("y", "cb", "cr", "var32"))
        else:
            got = run_filter(svtme, gpu, case)
    finally:
        TC.release(gpu, numbers + [OUT], BASE)
    pics = GL.case_inputs(case)
    want = ML.filter_window(pics[8], [pics[r] for r in refs], case["controls"], svtme.align8(w), svtme.align8(h))
    assert np.array_equal(got["var32"], want["var32"]), case
    for name in plane_names(case["controls"]):
        crop = want[name][:h, :w] if name == "y" else want[name][:(h + 1) >> 1, :(w + 1) >> 1]
        TC.assert_planes_equal(got[name], crop, f"{case['controls']} {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ld136_8c", "ld136_10c"])
def test_tfld_the_order_of_the_references_does_not_change_the_planes(svtme, gpu, gold, name):
    case = case_by_id(name)
    numbers = upload_case(gpu, case)
    try:
        for order in itertools.permutations(range(3)):
            res = run_filter(svtme, gpu, case, refs=[case["refs"][k] for k in order])
            for plane in ("y", "cb", "cr"):
                TC.assert_planes_equal(res[plane], gold[f"{name}.{plane}"], f"{name} {plane} {order}")
            assert np.array_equal(res["var32"], gold[name + ".var32"][list(order)]), order
    finally:
        TC.release(gpu, numbers, BASE)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ld72_8c", "ld72_10c"])
def test_tfld_strides_null_outputs_and_the_pictures_stay(svtme, gpu, gold, name):
    case = case_by_id(name)
    W, H = 72, 40
    numbers = upload_case(gpu, case)
    try:
        before = TC.state_of(gpu, numbers, BASE)
        wide = run_filter(svtme, gpu, case, strides=(W + 9, W // 2 + 5, W // 2 + 3))
        for plane, width in (("y", W), ("cb", W // 2), ("cr", W // 2)):
            TC.assert_planes_equal(np.ascontiguousarray(wide[plane]), gold[f"{name}.{plane}"], f"{name} {plane} wide")
            assert (wide[plane].base[:, width:] == 0).all(), plane  # the samples beyond the plane stay as they were
        for want in (("y",), ("y", "cr"), ("y", "cb", "var32")):
            res = run_filter(svtme, gpu, case, want=want)
            assert sorted(res) == sorted(want)
            for k in want:
                assert np.array_equal(res[k], gold[f"{name}.{k}"]), (want, k)
        # chroma off: cb and cr are not written even where given
        luma = dict(case, controls=dict(case["controls"], chroma=0))
        ctl = ld_controls(svtme, luma)
        out, bufs = gpu._tf_ld_out(ctl, 1, W, H, ("y", "cb", "cr"), None)
        bufs["cb"][:], bufs["cr"][:] = 77, 78
        arr = (C.c_uint64 * 1)(BASE + case["refs"][0])
        assert gpu.lib.svtme_tf_filter_ld(gpu.ctx, BASE + case["centre"], arr, 1, W, H, C.byref(ctl), C.byref(out)) == 0
        assert (bufs["cb"] == 77).all() and (bufs["cr"] == 78).all()
        TC.assert_planes_equal(bufs["y"], gold[name + ".y"], "luma of the yuv call")  # luma does not depend on chroma
        TC.assert_state(TC.state_of(gpu, numbers, BASE), before, "no resident picture is modified")
    finally:
        TC.release(gpu, numbers, BASE)


def repad(plane, W, H, pad):
    """What an upload leaves of true samples: replicated to the aligned size and into the margins."""
    return np.pad(plane, ((pad, pad + H - plane.shape[0]), (pad, pad + W - plane.shape[1])), mode="edge")


def attach_result(gpu, number, ctl, planes, w, h):
    """The upload / attach of filtered planes of the true size: what the window's result must equal."""
    gpu.upload(BASE + number, planes["y"])
    if ctl["bit_depth"] == 10:
        gpu.attach_10bit(BASE + number, planes["y"])
    if ctl["chroma"] and ctl["bit_depth"] == 10:
        gpu.attach_chroma_10bit(BASE + number, planes["cb"], planes["cr"], w, h)
    elif ctl["chroma"]:
        gpu.upload_chroma(BASE + number, planes["cb"], planes["cr"], w, h)


def window_case(w, h, refs, mode, ss=0):
    return dict(sweep_case(w, h, refs, mode[0], mode[1], ss, 7), controls={
        "tf_decay_factor_fp16": [GL.MID, GL.MID2, 20 << 10], "sub_sampling_shift": ss, "bit_depth": mode[0], "chroma": mode[1]})


def run_window(svtme, gpu, case, out_pn, centre_pn=None, refs_pn=None, want=()):
    centre_pn = BASE + case["centre"] if centre_pn is None else centre_pn
    refs_pn = [BASE + r for r in case["refs"]] if refs_pn is None else refs_pn
    return gpu.tf_window_ld(centre_pn, refs_pn, case["w"], case["h"], ld_controls(svtme, case), out_pn, want=want)


def filtered_true_size(svtme, gpu, case, centre_pn=None, refs_pn=None) -> dict:
    """svtme_tf_filter_ld of the window, cut to the true size."""
    w, h = case["w"], case["h"]
    centre_pn = BASE + case["centre"] if centre_pn is None else centre_pn
    refs_pn = [BASE + r for r in case["refs"]] if refs_pn is None else refs_pn
    res = gpu.tf_filter_ld(centre_pn, refs_pn, svtme.align8(w), svtme.align8(h), ld_controls(svtme, case))
    out = {k: np.ascontiguousarray(v[:(h + 1) >> 1, :(w + 1) >> 1]) for k, v in res.items() if k in ("cb", "cr")}
    return dict(out, y=np.ascontiguousarray(res["y"][:h, :w]), var32=res["var32"])


WINDOWS = [(72, 40, (7,), 1), (121, 67, (7, 9), 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("w,h,refs,ss", WINDOWS, ids=[f"{w}x{h}" for w, h, _, _ in WINDOWS])
def test_tfld_window_equals_filter_repad_upload_fresh_and_in_place(svtme, gpu, w, h, refs, ss, mode):
    """svtme_tf_window_ld against svtme_tf_filter_ld of the same pictures, the numpy re-pad and the upload /
    attach of that result, on every plane and level; in place it is the same as into a fresh number."""
    case = window_case(w, h, refs, mode, ss)
    ctl, what = case["controls"], f"{w}x{h} {mode}"
    W, H = svtme.align8(w), svtme.align8(h)
    numbers = upload_case(gpu, case)
    try:
        before = TC.state_of(gpu, numbers, BASE)
        want = filtered_true_size(svtme, gpu, case)
        got = run_window(svtme, gpu, case, BASE + OUT, want=("y", "cb", "cr", "var32"))
        assert sorted(got) == sorted(want)
        assert np.array_equal(got["var32"], want["var32"])
        for k in plane_names(ctl):
            TC.assert_planes_equal(got[k], want[k], f"{what} {k}")
        TC.assert_state(TC.state_of(gpu, numbers, BASE), before, what + ": the window's pictures stay")
        fresh = TC.state_of(gpu, [OUT], BASE)
        assert sorted(fresh[OUT]) == state_keys(ctl)
        # the numpy re-pad of the filtered planes
        y8 = (want["y"] >> 2).astype(np.uint8) if mode[0] == 10 else want["y"]
        TC.assert_planes_equal(fresh[OUT]["l0"], repad(y8, W, H, svtme.PAD_FULL), what + " level 0")
        if mode[0] == 10:
            TC.assert_planes_equal(fresh[OUT]["y16"], repad(want["y"], W, H, svtme.PAD_FULL), what + " 16-bit plane")
        for k in plane_names(ctl)[1:]:
            TC.assert_planes_equal(fresh[OUT][k + ("16" if mode[0] == 10 else "8")],
                                   repad(want[k], W // 2, H // 2, svtme.PAD_CHROMA), f"{what} {k}")
        # the upload / attach of that result
        attach_result(gpu, OUT + 1, ctl, want, w, h)
        TC.assert_state({OUT: TC.state_of(gpu, [OUT + 1], BASE)[OUT + 1]}, fresh, what + ": the resident result")
        # in place, nothing copied out
        assert run_window(svtme, gpu, case, BASE + case["centre"]) == {}
        after = TC.state_of(gpu, numbers, BASE)
        TC.assert_state({OUT: after[case["centre"]]}, fresh, what + ": in place")
        TC.assert_state({t: after[t] for t in refs}, {t: before[t] for t in refs}, what + ": the references stay")
    finally:
        TC.release(gpu, numbers + [OUT, OUT + 1], BASE)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [MODES[1], MODES[3]], ids=[MODE_IDS[1], MODE_IDS[3]])
def test_tfld_second_window_reads_the_first_windows_in_place_result(svtme, gpu, mode):
    """The low-delay chain: picture 8 is filtered in place from 7, then 9 from the filtered 8, nothing waited
    for in between. The second window equals the one whose reference was uploaded from host copies."""
    w, h = 121, 67
    first, second = window_case(w, h, (7,), mode), dict(window_case(w, h, (8,), mode, ss=1), centre=9)
    for case in (first, second):  # weights near 500 whatever the variance: what the reference holds shows in the result
        case["controls"]["tf_decay_factor_fp16"] = [0x7FFFFFFF, 5000 << 10, 0x7FFFFFFF]
    numbers = upload_case(gpu, window_case(w, h, (7, 9), mode))
    try:
        plain = filtered_true_size(svtme, gpu, second)  # from the unfiltered picture 8
        res = filtered_true_size(svtme, gpu, first)
        attach_result(gpu, OUT + 1, first["controls"], res, w, h)
        want = run_window(svtme, gpu, second, BASE + OUT + 2, refs_pn=[BASE + OUT + 1], want=("y", "cb", "cr", "var32"))
        assert run_window(svtme, gpu, first, BASE + 8) == {}  # in place, queued: returns at once
        got = run_window(svtme, gpu, second, BASE + OUT + 3, want=("y", "cb", "cr", "var32"))
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        assert not np.array_equal(want["y"], plain["y"])  # the filtered reference is what was read
        TC.assert_state({0: TC.state_of(gpu, [OUT + 3], BASE)[OUT + 3]}, {0: TC.state_of(gpu, [OUT + 2], BASE)[OUT + 2]},
                        "second result")
    finally:
        TC.release(gpu, numbers + [OUT + 1, OUT + 2, OUT + 3], BASE)


@pytest.mark.gpu
def test_tfld_refused_calls_leave_every_picture(svtme, gpu):
    """The refusals that need the context: a picture that is not resident, has another size or lacks a plane
    the mode reads; and every context-free refusal again, now with pictures that a wrong call could harm."""
    full = window_case(128, 128, (7, 9), (10, 1))
    lib, ctx = gpu.lib, gpu.ctx
    frames, uv = GL.luma_frames(full), GL.chroma_frames(full)
    numbers = upload_case(gpu, full)  # 8, 7, 9: every plane a mode can read ...
    try:
        for t in numbers:
            gpu.upload_chroma(BASE + t, (uv[t][0] >> 2).astype(np.uint8), (uv[t][1] >> 2).astype(np.uint8), 128, 128)
        gpu.upload(BASE + 6, (frames[7] >> 2).astype(np.uint8))  # ... 6: luma alone
        gpu.upload(BASE + 5, frames[7])                           # 5: the 16-bit plane, no chroma of either depth
        gpu.attach_10bit(BASE + 5, frames[7])
        gpu.upload(BASE + 4, frames[7][:64, :64])                 # 4: another size
        everything = numbers + [6, 5, 4]
        before = TC.state_of(gpu, everything, BASE)
        _context_free_errors(svtme, lib, ctx)
        for window in (False, True):
            for bd, chroma, refs, centre, message in ((8, 0, [7, 999], 8, "not resident"), (8, 0, [7], 999, "not resident"),
                                                      (8, 0, [7, 4], 8, "is 64x64"), (8, 1, [7, 6], 8, "no chroma"),
                                                      (8, 1, [7], 6, "no chroma"), (10, 0, [7, 6], 8, "no 10-bit plane"),
                                                      (10, 1, [7, 5], 8, "no 10-bit chroma"),
                                                      (10, 1, [7], 5, "no 10-bit chroma")):
                st = _ld_call(svtme, lib, ctx, window, refs=[BASE + r for r in refs], centre=BASE + centre,
                              ctl=_controls(svtme, bit_depth=bd, chroma=chroma))
                assert st == BAD_PARAMETER and message in lib.svtme_last_error().decode(), (window, bd, chroma, refs)
            assert _ld_call(svtme, lib, ctx, window, w=64, h=64) == BAD_PARAMETER  # the pictures are 128 x 128
        with pytest.raises(RuntimeError):  # no result picture was made
            gpu.download(BASE + OUT, 0)
        TC.assert_state(TC.state_of(gpu, everything, BASE), before, "refused calls")
        # and the valid forms succeed, in every mode
        for bd, chroma in MODES:
            for window in (False, True):
                assert _ld_call(svtme, lib, ctx, window, refs=[BASE + 7, BASE + 9],
                                ctl=_controls(svtme, bit_depth=bd, chroma=chroma), strides=(200, 70, 90)) == 0
    finally:
        TC.release(gpu, numbers + [6, 5, 4, OUT], BASE)


@pytest.mark.gpu
def test_tfld_existing_calls_are_unchanged_by_ld_windows_in_the_same_context(svtme, gpu):
    """Each window and filter call that was there before gives byte for byte the same before and after
    low-delay windows of every mode on other picture numbers of the context."""
    win = TC.yuv_window_10(121, 67, (7, 9))
    numbers, refs = [8, 7, 9], [BASE + 7, BASE + 9]

    def existing():
        sp, fc = TC.luma_controls(svtme, win)
        _, fcy = TC.window_controls(svtme, win)
        _, sub = TC.me_and_subpel(svtme, gpu, win, BASE + 8, refs)
        jobs = [TW.tf_job(svtme, win, BASE + 8, r) for r in refs]
        arrays = list(gpu.tf_filter(BASE + 8, refs, 121, 67, fc, sub)) + list(gpu.tf_filter_yuv(BASE + 8, refs, 121, 67, fcy, sub))
        arrays += list(gpu.tf_filter_10bit(BASE + 8, refs, 121, 67, fc, sub))
        arrays += list(gpu.tf_filter_yuv_10bit(BASE + 8, refs, 121, 67, fcy, sub))
        states = []
        for call, args in ((gpu.tf_window, (sp, fc)), (gpu.tf_window_yuv, (sp, fcy)), (gpu.tf_window_10bit, (sp, fc)),
                           (gpu.tf_window_yuv_10bit, (sp, fcy))):
            out = call(jobs, 121, 67, *args, BASE + OUT)
            arrays += [out[k] for k in sorted(out)]
            states.append(TC.state_of(gpu, [OUT], BASE)[OUT])
            gpu.release(BASE + OUT)
        return arrays, states

    ld = [dict(window_case(121, 67, (7, 9), mode), centre=8) for mode in MODES]
    try:
        TC.upload_yuv10(gpu, win, BASE, chroma8=True)
        a0, s0 = existing()
        for k, case in enumerate(ld):
            lnum = upload_case(gpu, case, base=BASE + 100 * (k + 1))
            gpu.tf_window_ld(BASE + 100 * (k + 1) + 8, [BASE + 100 * (k + 1) + r for r in (7, 9)], 121, 67,
                             ld_controls(svtme, case), BASE + 100 * (k + 1) + 8 + (k & 1) * 50)
            gpu.tf_filter_ld(BASE + 100 * (k + 1) + 9, [BASE + 100 * (k + 1) + 7], 128, 72, ld_controls(svtme, case))
            assert sorted(lnum) == [7, 8, 9]
        a1, s1 = existing()
    finally:
        TC.release(gpu, numbers + [OUT], BASE)
        for k in range(len(ld)):
            TC.release(gpu, [7, 8, 9, 58], BASE + 100 * (k + 1))
    assert len(a0) == len(a1) and all(np.array_equal(x, y) for x, y in zip(a0, a1))
    for x, y in zip(s0, s1):
        TC.assert_state({0: x}, {0: y}, "the result picture of an existing window call")
