"""Seeded sweep of the picture job (k_hme and the split-path kernels) over the job
fields, controls and kernel paths that the fixed case lists leave alone.

sweep_case(seed) draws one case: a JSON-serialisable dict of the picture size,
the content, the reference lists, the job fields, the base controls (a preset and
a resolution for svtme_derive_controls, or a TF-ME level for
svtme_derive_controls_tf) and `mut`, the control fields set on top of them.
DIRECTED holds cases of the same form written by hand for branches a draw rarely
reaches. CASES = the draws of SWEEP_SEEDS, then DIRECTED: the list
tests/golden/me_sweep.json pins to the reference (make_golden_me_sweep.py) and
tests/test_me_sweep.py runs on the oracle and on the GPU.

The draws stay inside what the kernels hold ("The ME sweep"):
  - every search window of svtme_stages.hip that is staged in LDS falls back to
    global reads when it does not fit (sad_geo's `staged`), or belongs to a kernel
    the host picks only when it fits (svtme_l0_full, svtme_l1_full,
    svtme_fp_wide_lds), so search areas are free;
  - 32-bit full-pel keys need every order below 4096: svtme_fp_k32 decides that from
    fp_area_bound, which covers the mv multiplier and the variance growth;
  - k_hme's HME-L2 tile keys hold a 13-bit column and k_stage_c's FpRef an 8-bit quad
    count: validate_job refuses wider areas; the draws stay far below;
  - a zero ME search-range divisor divides by zero in the reference: refused, not drawn;
  - num_hme_sa_w / num_hme_sa_h stay 2 (the product refuses anything else), and no
    case has 4 + 4 references (me_mv_array is 7 wide).
No case was taken off the list.
"""
import ctypes as C
import json
import os

U32 = 0xFFFFFFFF
CUR = 8  # the current picture's time; references are times around it

# picture sizes that separate the dispatch classes; the last only for a minority
SIZES = [(64, 64), (192, 136), (200, 136), (264, 72), (208, 72), (72, 40), (136, 8)]
BIG = (640, 360)
CONTENTS = ["pan", "vpan", "hpan", "noise", "flat", "sat", "stripes"]

PATH_BITS = ["NO_FUSED_HME", "NO_L1_FULL", "NO_L0_FULL", "NO_FP_WIDE", "SPLIT_PASS", "NO_A1_GATE", "HME_4WAVES"]


class Rng:
    """splitmix64: the same draws on every platform and library version"""

    def __init__(self, seed: int):
        self.s = (0xD1342543DE82EF95 * seed + 0x632BE59BD9B4E019) & 0xFFFFFFFFFFFFFFFF
        self.s = self.next()  # seeds next to each other start at unrelated states

    def next(self) -> int:
        self.s = (self.s + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return z ^ (z >> 31)

    def below(self, n: int) -> int:
        return self.next() % n

    def chance(self, num: int, den: int) -> bool:
        return self.below(den) < num

    def pick(self, seq):
        return seq[self.below(len(seq))]


# full-pel areas [min, max]: one part, 2 to 4 parts, 16 parts (64-bit keys), the derived shapes
ME_SA = [[[12, 4], [8, 3]], [[16, 8], [16, 8]], [[12, 12], [32, 16]], [[21, 21], [56, 28]], [[32, 32], [32, 32]],
         [[48, 32], [48, 32]], [[64, 32], [64, 32]], [[64, 64], [64, 64]], [[128, 64], [128, 64]],
         [[36, 36], [104, 104]], [[24, 24], [24, 24]], [[40, 12], [40, 12]]]
FPW_WIDTHS = [24, 28, 40, 44, 56, 76]  # k_fp_wide's set-split classes (test_fp_wide_set_split_parity)
HME_L0_SA = [[[8, 8], [96, 96]], [[16, 16], [64, 32]], [[32, 16], [192, 96]], [[240, 240], [480, 480]],
             [[32, 32], [32, 32]], [[96, 96], [192, 192]], [[64, 24], [64, 24]]]
HME_L1_SA = [[8, 3], [16, 16], [8, 8], [24, 5], [12, 7], [32, 9], [16, 17]]
HME_L2_SA = [[8, 3], [16, 8], [8, 5], [24, 6]]
SR_TH = [[0, 0, 0], [0xFFFFFFF, 0xFFFFFFF, U32], [0, 0xFFFFFFF, U32], [80000, 150000, 400000], [80000, 150000, U32]]


def draw_mutations(g: Rng, big: bool) -> dict:
    m = {}

    def maybe(num, den, name, values):
        if g.chance(num, den):
            m[name] = g.pick(values)

    maybe(1, 8, "enable_hme_flag", [0, 1])
    maybe(1, 6, "enable_hme_level0_flag", [0, 1])
    maybe(1, 5, "enable_hme_level1_flag", [0, 1])
    maybe(1, 4, "enable_hme_level2_flag", [0, 1])
    maybe(1, 4, "prehme_enable", [0, 1])
    maybe(1, 3, "prehme_skip_search_line", [0, 1])
    maybe(1, 3, "prehme_l1_early_exit", [0, 1])
    maybe(1, 5, "me_safe_limit_zz_th", [2000, 20000, 200000])
    maybe(1, 3, "me_early_exit_th", [0, 2048, 32768, 200000])
    maybe(1, 4, "prev_me_stage_based_exit_th", [256, 4096, 65536, 1 << 20])
    maybe(1, 3, "enable_me_hme_ref_pruning", [0, 1])
    maybe(1, 3, "prune_ref_if_hme_sad_dev_bigger_than_th", [0, 5, 15, 50, 200, 65535])
    maybe(1, 3, "prune_ref_if_me_sad_dev_bigger_than_th", [0, 10, 60, 300, 65535])
    maybe(1, 3, "zz_sad_th", [0, 20000, 81920, 1 << 22])
    maybe(1, 3, "zz_sad_pct", [0, 5, 50])
    maybe(1, 3, "phme_sad_th", [0, 40960, 1 << 22])
    maybe(1, 3, "phme_sad_pct", [0, 5, 50])
    maybe(1, 3, "enable_me_sr_adjustment", [0, 1, 2])
    if g.chance(1, 3):
        m["me_sr_div4_th"], m["me_sr_div2_th"], m["me_sr_mult2_th"] = g.pick(SR_TH)
    maybe(1, 4, "stationary_me_sr_divisor", [1, 2, 8, 16])
    maybe(1, 4, "me_sr_divisor_for_low_hme_sad", [1, 2, 8, 16])
    maybe(1, 4, "reduce_me_sr_based_on_mv_length_th", [0, 4, 64])
    maybe(1, 4, "reduce_me_sr_based_on_hme_sad_abs_th", [0, 3000, 60000])
    maybe(1, 4, "stationary_hme_sad_abs_th", [0, 3000, 60000])
    maybe(1, 4, "me_8x8_var_enabled", [0, 1])
    maybe(1, 5, "hme_search_method", [0, 1])
    maybe(1, 5, "me_search_method", [0, 1])
    if g.chance(1, 3):
        m["mv_sa_adj_enabled"] = g.below(2)
        m["mv_sa_adj_nearest_ref_only"] = g.below(2)
        m["mv_sa_adj_mv_size_th"] = g.pick([0, 4, 25])
        m["mv_sa_adj_sa_multiplier"] = g.pick([1, 2, 3])
    maybe(1, 4, "distance_based_hme_resizing", [0, 1])
    if g.chance(1, 5):  # the real-time tune's HME-L0 reduction (svtme_hme_rt)
        m["reduce_hme_l0_sr_th_min"], m["reduce_hme_l0_sr_th_max"] = g.pick([[8, 100], [8, 200], [2, 20], [16, 40]])
        m["distance_based_hme_resizing"] = 1
        if m.get("enable_me_sr_adjustment", 1) == 0:
            m["enable_me_sr_adjustment"] = 1
    maybe(1, 2 if big else 3, "hme_l0_sa", HME_L0_SA)
    maybe(1, 3, "hme_l1_sa", HME_L1_SA)
    maybe(1, 3, "hme_l2_sa", HME_L2_SA)
    if g.chance(1, 6):  # k_fp_wide: a fixed wide area, sub-sampled rows, 32-bit keys
        w = g.pick(FPW_WIDTHS)
        m["me_sa"] = [[w, 48], [w, 48]]
        m["me_8x8_var_enabled"] = 0
        m["enable_me_sr_adjustment"] = 0
        m["me_search_method"] = 0
    else:
        maybe(2 if big else 1, 3, "me_sa", ME_SA)
    # validate_job's limit of 1016 positions for the per-SB full-pel kernel: the widest derived
    # area (256) x 2 x the variance growth (3 / 2) stays below it, x 3 would not
    if m.get("enable_me_sr_adjustment") == 2 and m.get("mv_sa_adj_sa_multiplier") == 3:
        m["mv_sa_adj_sa_multiplier"] = 2
    maybe(1, 3, "prune_me_candidates_th", [0, 5, 65, 200])
    maybe(1, 3, "use_best_unipred_cand_only", [0, 1])
    return m


def sweep_case(seed: int) -> dict:
    g = Rng(seed)
    big = g.chance(1, 9)
    w, h = BIG if big else g.pick(SIZES)
    case = {"name": f"s{seed:03d}", "w": w, "h": h, "content": g.pick(CONTENTS), "bits": 10 if g.chance(1, 6) else 8}
    tf = g.chance(1, 5)
    if tf:
        case["l0"], case["l1"] = [g.pick([6, 7, 9, 10])], []
    else:
        n0, n1 = 1 + g.below(3 if big else 4), g.below(3 if big else 4)
        case["l0"] = g.pick([[7, 6, 5, 4], [7, 6, 4, 3], [7, 5, 4, 2]])[:n0]
        case["l1"] = g.pick([[9, 10, 11], [9, 10, 12], [10, 11, 13]])[:n1]
    case["tl"] = g.below(4)
    case["hl"] = g.pick([0, 1, 2, 3, 5])
    case["sbr"] = g.below(2)
    case["is_ref"] = 0 if g.chance(1, 4) else 1
    case["e8"] = g.below(2)
    case["e16"] = 0 if g.chance(1, 4) else 1
    case["gm"] = g.below(2)
    case["gm_dist"] = g.below(2)
    case["only_l_bwd"] = g.below(2)
    total = ((w + 63) // 64) * ((h + 63) // 64)
    case["sb_begin"], case["sb_count"] = 0, 0
    if total > 1 and g.chance(1, 4):
        case["sb_begin"] = g.below(total)
        case["sb_count"] = 1 + g.below(total - case["sb_begin"])
    res = g.below(7) if g.chance(1, 4) else None  # None: the picture's own resolution
    if tf:
        case["tf"] = {"level": g.below(5), "qp_opt": g.below(2), "exit_th": g.pick([0, 2600, 50000])}
        case["preset"] = None
    else:
        case["tf"] = None
        case["preset"] = g.below(14)
    case["res"] = res
    case["mut"] = draw_mutations(g, big)
    return case


def _case(name, w, h, content, l0, l1, preset, mut, tl=1, hl=5, sbr=0, is_ref=1, e8=1, e16=1, gm=0, gm_dist=0,
          only_l_bwd=1, sb_begin=0, sb_count=0, bits=8, tf=None, res=None):
    return {"name": name, "w": w, "h": h, "content": content, "bits": bits, "l0": list(l0), "l1": list(l1), "tl": tl,
            "hl": hl, "sbr": sbr, "is_ref": is_ref, "e8": e8, "e16": e16, "gm": gm, "gm_dist": gm_dist,
            "only_l_bwd": only_l_bwd, "sb_begin": sb_begin, "sb_count": sb_count, "tf": tf, "preset": preset,
            "res": res, "mut": mut}


NO_PRUNE = {"enable_me_hme_ref_pruning": 0, "zz_sad_th": 0, "phme_sad_th": 0}
WIDE_L0 = {"hme_l0_sa": [[96, 96], [192, 192]], "distance_based_hme_resizing": 0}

DIRECTED = [
    # the me_safe_limit_zz_th rule: two lists, tl >= hierarchical_levels > 0, similar brightness, flat
    # content; no other pruning, so do_ref == 0 on the slots with r > 0 is the rule's
    _case("d_safe_zz_fused", 192, 136, "flat", (7, 6), (9, 10), 8,
          dict(NO_PRUNE, me_safe_limit_zz_th=20000), tl=3, hl=3, sbr=1),
    _case("d_safe_zz_split", 200, 136, "flat", (7, 6, 5), (9, 10), 6,
          dict(NO_PRUNE, me_safe_limit_zz_th=2000, me_early_exit_th=0), tl=2, hl=1, sbr=1),
    # zz pruning alone, pre-HME pruning alone, HME-SAD pruning alone, ME-SAD pruning
    _case("d_zz_prune", 192, 136, "pan", (7, 6, 5), (9, 10), 8,
          {"zz_sad_th": 1 << 22, "zz_sad_pct": 0, "me_early_exit_th": 32768, "phme_sad_th": 0,
           "enable_me_hme_ref_pruning": 0}, tl=1),
    _case("d_prehme_prune", 192, 136, "pan", (7, 6, 5), (9, 10), 8,
          {"zz_sad_th": 0, "phme_sad_th": 1 << 22, "phme_sad_pct": 0, "enable_me_hme_ref_pruning": 0}, tl=1),
    _case("d_hme_prune", 200, 136, "pan", (7, 6, 5), (9, 10), 8,
          {"zz_sad_th": 0, "phme_sad_th": 0, "enable_me_hme_ref_pruning": 1,
           "prune_ref_if_hme_sad_dev_bigger_than_th": 0, "prune_ref_if_me_sad_dev_bigger_than_th": 65535}, tl=1),
    _case("d_me_prune", 192, 136, "noise", (7, 6, 5), (9, 10), 8,
          {"zz_sad_th": 0, "phme_sad_th": 0, "enable_me_hme_ref_pruning": 1,
           "prune_ref_if_hme_sad_dev_bigger_than_th": 65535, "prune_ref_if_me_sad_dev_bigger_than_th": 0}, tl=1),
    # finish_sb's general mode with every candidate: 4 + 3 references, all searched, no candidate
    # pruning, L0-L0 and L1-L1 pairs (only_l_bwd 0): 7 + 12 + 3 + 1 = 23
    _case("d_cand23", 192, 136, "noise", (7, 6, 5, 4), (9, 10, 11), 8,
          dict(NO_PRUNE, prune_me_candidates_th=0), tl=1, only_l_bwd=0, gm=1),
    _case("d_cand23_npus21", 200, 136, "stripes", (7, 6, 5, 4), (9, 10, 11), 6,
          dict(NO_PRUNE, prune_me_candidates_th=0), tl=2, only_l_bwd=0, e8=0),
    # npus == 5 in each of finish_sb's modes, with the GM detection's 16x16 -> 32x32 mapping
    _case("d_npus5_general", 192, 136, "pan", (7, 6), (9, 10), 8, {}, tl=1, e8=0, e16=0, gm=1, gm_dist=1),
    _case("d_npus5_mrp_off", 200, 136, "hpan", (7,), (9,), 8, {"use_best_unipred_cand_only": 1}, tl=1, e8=0, e16=0,
          gm=1),
    _case("d_npus5_single", 72, 40, "pan", (7,), (), 12, {}, tl=0, e8=1, e16=0, gm=1),
    # TF-ME: the HME-only exit set on every SB, and clear
    _case("d_tf_exit", 192, 136, "flat", (7,), (), None, {}, tl=0, tf={"level": 3, "qp_opt": 0, "exit_th": 50000}),
    _case("d_tf_noexit_l0full", 208, 72, "noise", (9,), (), None, {}, tl=0,
          tf={"level": 1, "qp_opt": 0, "exit_th": 2600}),
    # search centres past each picture edge: fast motion, wide HME-L0 areas, check_00_center on
    _case("d_edges_h", 200, 136, "hpan", (7, 6), (9, 10), 8, dict(NO_PRUNE, me_early_exit_th=0, **WIDE_L0), tl=1),
    _case("d_edges_v", 192, 136, "vpan", (7, 6), (9, 10), 8, dict(NO_PRUNE, me_early_exit_th=0, **WIDE_L0), tl=1),
    # GM flags on a fast pan, a real SB sub-range, 10-bit input
    _case("d_gm_band_10bit", 640, 360, "hpan", (7,), (9,), 4, dict(WIDE_L0), tl=1, gm=1, sb_begin=7, sb_count=19,
          bits=10),
    # HME off / HME-L0 off / pre-HME only, on the fused and the split path
    _case("d_hme_off", 192, 136, "pan", (7, 6), (9,), 8, {"enable_hme_flag": 0}, tl=1),
    _case("d_l0_off_prev_exit", 200, 136, "pan", (7, 6), (9,), 6,
          {"enable_hme_level0_flag": 0, "prev_me_stage_based_exit_th": 65536}, tl=1),
    # k_fp_wide and the banded full-pel with 64-bit keys on the large picture
    _case("d_fpw_640", 640, 360, "pan", (7,), (9,), 8,
          {"me_sa": [[44, 48], [44, 48]], "me_8x8_var_enabled": 0, "enable_me_sr_adjustment": 0}, tl=1),
    _case("d_banded16_640", 640, 360, "vpan", (7,), (), 8,
          {"me_sa": [[128, 64], [128, 64]], "enable_me_sr_adjustment": 0, "me_sr_div4_th": 0, "me_sr_div2_th": 0,
           "me_sr_mult2_th": 0}, tl=0),
]

# 48 draws; chosen with DIRECTED so that every coverage key of tests/golden/me_sweep.json is
# non-zero on the reference and every host dispatch predicate takes all its values
SWEEP_SEEDS = list(range(48))


def cases() -> list:
    return [sweep_case(s) for s in SWEEP_SEEDS] + DIRECTED


# ----------------------------------------------------------------------------
# frames, controls and the job of a case
# ----------------------------------------------------------------------------
def times(case) -> list:
    return sorted(set([CUR] + case["l0"] + case["l1"]))


def frames_of(S, case) -> dict:
    if case["bits"] == 10:
        if case["content"] == "pan":
            syn = S.Synth(case["w"], case["h"])
            return {t: syn.frame10(t) for t in times(case)}
        # the other contents as 10-bit planes: the 8-bit value in the MSBs, t in the LSBs
        f8 = S.test_frames(case["content"], case["w"], case["h"], times(case))
        return {t: (f.astype("uint16") << 2) | (t & 3) for t, f in f8.items()}
    return S.test_frames(case["content"], case["w"], case["h"], times(case))


def apply_mut(S, ctrl, mut: dict):
    for name, v in mut.items():
        cur = getattr(ctrl, name)
        if isinstance(cur, S.AreaMinMax):
            cur.sa_min.width, cur.sa_min.height = v[0]
            cur.sa_max.width, cur.sa_max.height = v[1]
        elif isinstance(cur, S.Area):
            cur.width, cur.height = v
        else:
            setattr(ctrl, name, v)
    return ctrl


def controls_of(S, case, reference: bool = False):
    """The case's controls: derived (by the product's restatement, or by the reference), then mutated."""
    res = case["res"] if case["res"] is not None else S.input_resolution_of(case["w"], case["h"])
    if case["tf"]:
        derive = S.ref_derive_controls_tf if reference else S.derive_controls_tf
        ctrl = derive(case["tf"]["level"], case["tf"]["qp_opt"], 35, res)
    else:
        derive = S.ref_derive_controls if reference else S.derive_controls
        ctrl = derive(case["preset"], 35, res, case["tl"])
    return apply_mut(S, ctrl, case["mut"])


def job_of(S, case, ctrl, base: int = 0):
    """The job with picture numbers base + time."""
    kw = {}
    if case["tf"]:
        kw = {"me_type": S.ME_MCTF, "tf_me_exit_th": case["tf"]["exit_th"]}
    l0, l1 = [base + t for t in case["l0"]], [base + t for t in case["l1"]]
    job = S.make_job(case["w"], case["h"], ctrl, base + CUR, l0, l1, temporal_layer_index=case["tl"],
                     is_ref=bool(case["is_ref"]), hierarchical_levels=case["hl"], enable_me_8x8=bool(case["e8"]),
                     ref_count_used=(max(len(l0), 1), len(l1)), only_l_bwd=bool(case["only_l_bwd"]),
                     gm_enabled=bool(case["gm"]), sb_begin=case["sb_begin"], sb_count=case["sb_count"], **kw)
    job.similar_brightness_refs = case["sbr"]
    job.enable_me_16x16 = case["e16"]
    job.gm_use_distance_based_active_th = case["gm_dist"]
    return job


def run_cpu(S, case, checker: str = "oracle", frames=None, ctrl=None):
    """The case through a CPU checker -> (records, sb_results)."""
    frames = frames if frames is not None else frames_of(S, case)
    ctrl = ctrl if ctrl is not None else controls_of(S, case, reference=checker == "ref")
    pyr = {t: S.build_host_pyramid(f, checker) for t, f in frames.items()}
    refs = {(0, i): pyr[t] for i, t in enumerate(case["l0"])}
    refs.update({(1, i): pyr[t] for i, t in enumerate(case["l1"])})
    return S.run_checker(job_of(S, case, ctrl), pyr[CUR], refs, checker, nthreads=8)


# ----------------------------------------------------------------------------
# the committed list and the oracle's outputs of its cases, shared by every test file of a process
# ----------------------------------------------------------------------------
_fixture, _oracle = [], {}


def fixture() -> dict:
    """tests/golden/me_sweep.json: the cases with the reference's checksums and coverage."""
    if not _fixture:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "me_sweep.json")) as fh:
            _fixture.append(json.load(fh))
    return _fixture[0]


def oracle_of(S, k):
    """(controls, records, SB results) of committed case k on the oracle, computed once (read-only)."""
    if k not in _oracle:
        case = fixture()["cases"][k]["case"]
        ctrl = controls_of(S, case)
        recs, sbr = run_cpu(S, case, "oracle", ctrl=ctrl)
        for a in (recs, sbr):
            a.setflags(write=False)
        _oracle[k] = (ctrl, recs, sbr)
    return _oracle[k]


# ----------------------------------------------------------------------------
# coverage: what a case exercised, from the checker's outputs and the case alone
# ----------------------------------------------------------------------------
COVERAGE_KEYS = ["safe_limit_zz", "zz_prune", "prehme_prune", "hme_sad_prune", "me_sad_prune", "records_unsearched",
                 "all_searched", "tf_exit_set", "tf_exit_clear", "finish_single", "finish_mrp_off", "finish_general",
                 "cand_ge10", "cand_ge20", "cand_23", "npus_5", "npus_21", "npus_85", "gm_allow", "gm_stationary",
                 "centre_left", "centre_right", "centre_top", "centre_bottom", "sb_subrange", "ten_bit"]


def coverage(S, case, ctrl, recs, sbr) -> dict:
    import numpy as np

    c = dict.fromkeys(COVERAGE_KEYS, 0)
    n_sb, R = recs.shape
    n0, n1 = len(case["l0"]), len(case["l1"])
    slots = [(0, r) for r in range(n0)] + [(1, r) for r in range(n1)]
    tl, tf = case["tl"], bool(case["tf"])
    hme_on = bool(ctrl.enable_hme_flag)
    zz_on = bool(ctrl.me_early_exit_th or ctrl.me_safe_limit_zz_th)
    hme_rule = hme_on and not tf and ctrl.enable_me_hme_ref_pruning and \
        ctrl.prune_ref_if_hme_sad_dev_bigger_than_th != 0xFFFF
    ph_rule = bool(ctrl.prehme_enable) and tl > 0 and ctrl.phme_sad_th > 0
    safe_pre = bool(ctrl.me_safe_limit_zz_th) and case["hl"] > 0 and n1 > 0 and tl >= case["hl"] and case["sbr"]
    total_w = (case["w"] + 7) // 8 * 8
    total_h = (case["h"] + 7) // 8 * 8
    w64 = (total_w + 63) // 64
    for k in range(n_sb):
        zz = [int(recs[k, i]["zz_sad"]) for i in range(R)]
        used = [zz[i] for i, (l, r) in enumerate(slots) if tl > 0 or l == 0]
        best = min(used) if zz_on and used else U32
        safe = bool(safe_pre and zz[0] < ctrl.me_safe_limit_zz_th and zz[n0] < ctrl.me_safe_limit_zz_th)
        if safe:
            assert all(recs[k, i]["do_ref"] == 0 for i, (l, r) in enumerate(slots) if r > 0), (case["name"], k)
            c["safe_limit_zz"] += 1
        tfx = bool(recs[k, 0]["tf_early_exit"])
        for i, (l, r) in enumerate(slots):
            rec = recs[k, i]
            zz_rule = zz_on and tl > 0 and r > 0 and best < ctrl.zz_sad_th and \
                ((zz[i] - best) * 100) & U32 > (ctrl.zz_sad_pct * best) & U32
            if zz_rule:
                assert rec["do_ref"] == 0, (case["name"], k, i)
                c["zz_prune"] += 1
            early = not rec["searched"] and not tfx and not zz_rule and not (safe and r > 0)
            if early and ph_rule and not hme_rule:
                c["prehme_prune"] += 1
            if early and hme_rule and not ph_rule:
                c["hme_sad_prune"] += 1
            if rec["searched"] and not rec["do_ref"]:
                c["me_sad_prune"] += 1
            if not rec["searched"]:
                c["records_unsearched"] += 1
            else:
                b64 = case["sb_begin"] + k
                ox, oy = (b64 % w64) * 64, (b64 // w64) * 64
                # a searched record's centre with its block past a picture edge: the HME rectangles
                # that found it and the full-pel area around it are clamped there (the pads hold
                # centres 63 pixels out at most, so check_00_center's own clamp never moves one)
                x, y = ox + int(rec["hme_sc_x"]), oy + int(rec["hme_sc_y"])
                c["centre_left"] += x < 0
                c["centre_right"] += x + min(64, total_w - ox) > total_w
                c["centre_top"] += y < 0
                c["centre_bottom"] += y + min(64, total_h - oy) > total_h
        if tf:
            c["tf_exit_set" if tfx else "tf_exit_clear"] += 1
    c["all_searched"] = int(bool(recs["searched"].all()))
    if not tf:
        mode = "finish_single" if (n0, n1) == (1, 0) else "finish_mrp_off" if (n0, n1) == (1, 1) else "finish_general"
        c[mode] = n_sb
        c["npus_85" if case["e16"] and case["e8"] else "npus_21" if case["e16"] else "npus_5"] = n_sb
        if mode == "finish_general":
            t = sbr["total_me_candidate_index"]
            c["cand_ge10"], c["cand_ge20"], c["cand_23"] = int((t >= 10).sum()), int((t >= 20).sum()), int((t == 23).sum())
        c["gm_allow"] = int(np.count_nonzero(sbr["rc_me_allow_gm"]))
        c["gm_stationary"] = int(np.count_nonzero(sbr["stationary_block_present"]))
    total = w64 * ((total_h + 63) // 64)
    c["sb_subrange"] = int(n_sb < total)
    c["ten_bit"] = int(case["bits"] == 10)
    return {k: int(v) for k, v in c.items()}


# ----------------------------------------------------------------------------
# host dispatch predicates (libsvtme.so, no GPU needed) and the paths that change a job's dispatch
# ----------------------------------------------------------------------------
def lib_of(S):
    lib = S.load_product()
    for f in ("svtme_hme_fused", "svtme_l0_full_job"):
        getattr(lib, f).argtypes = [C.POINTER(S.Job)]
        getattr(lib, f).restype = C.c_bool
    lib.svtme_hme_waves.argtypes = [C.POINTER(S.Job)]
    lib.svtme_hme_waves.restype = C.c_uint32
    for f in ("svtme_hme_rt", "svtme_l1_full", "svtme_fp_wide_lds", "svtme_fp_wide", "svtme_fp_k32"):
        getattr(lib, f).argtypes = [C.POINTER(S.Controls)]
        getattr(lib, f).restype = C.c_bool
    lib.svtme_fp_parts.argtypes = [C.POINTER(S.Controls)]
    lib.svtme_fp_parts.restype = C.c_uint32
    return lib


def plan_lib_of(S):
    """lib_of, with the functions the launch-plan helpers below call."""
    lib = lib_of(S)
    lib.svtme_fp_parts_paths.argtypes = [C.POINTER(S.Controls), C.c_uint32]
    lib.svtme_fp_parts_paths.restype = C.c_uint32
    for f in ("svtme_stage_a_list", "svtme_stage_a1_list", "svtme_stage_b_list"):
        getattr(lib, f).argtypes = [C.POINTER(S.Job), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)]
        getattr(lib, f).restype = None
    lib.svtme_job_kernels.argtypes = [C.POINTER(S.Job), C.c_uint32, C.c_int, C.POINTER(C.c_uint8),
                                      C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)]
    lib.svtme_job_kernels.restype = C.c_uint32
    lib.svtme_kernel_name.argtypes = [C.c_uint32]
    lib.svtme_kernel_name.restype = C.c_char_p
    return lib


def dispatch_of(S, lib, job) -> dict:
    c = C.byref(job.ctrl)
    return {"fused": bool(lib.svtme_hme_fused(C.byref(job))), "waves": int(lib.svtme_hme_waves(C.byref(job))),
            "rt": bool(lib.svtme_hme_rt(c)), "l1_full": bool(lib.svtme_l1_full(c)),
            "l0_full": bool(lib.svtme_l0_full_job(C.byref(job))), "fp_wide": bool(lib.svtme_fp_wide(c)),
            "fp_wide_lds": bool(lib.svtme_fp_wide_lds(c)), "k32": bool(lib.svtme_fp_k32(c)),
            "parts": int(lib.svtme_fp_parts(c)), "full_me": job.ctrl.me_search_method == S.FULL_SAD_SEARCH,
            "l2": bool(job.ctrl.enable_hme_level2_flag)}


def paths_of(S, job, d: dict) -> list:
    """The single path bits (names of PATH_BITS) that change this job's dispatch."""
    c = job.ctrl
    whole = d["fused"] and d["parts"] == 1  # the whole-pass k_hme
    out = []
    if d["fused"]:
        out.append("NO_FUSED_HME")
    if d["l1_full"] and not d["fused"]:
        out.append("NO_L1_FULL")
    if d["l0_full"] and not d["fused"]:
        out.append("NO_L0_FULL")
    if d["fp_wide_lds"]:
        out.append("NO_FP_WIDE")
    if whole:
        out.append("SPLIT_PASS")
    # k_hme's gate of the list-1 pre-HME regions (its own condition)
    if d["fused"] and not d["rt"] and c.prehme_enable and c.prehme_l1_early_exit and job.num_lists == 2:
        out.append("NO_A1_GATE")
    if whole and d["waves"] == 3:
        out.append("HME_4WAVES")
    return out


def launch_class(d: dict) -> tuple:
    """The fields svtme_launch_key separates jobs of a batch by (paths 0)."""
    whole = d["fused"] and d["parts"] == 1
    return (d["full_me"], d["parts"] != 0, d["k32"], d["l2"], d["fused"], d["parts"] == 1, d["fp_wide"], d["rt"],
            d["fp_wide_lds"], d["l1_full"] and not d["fused"], d["l0_full"] and not d["fused"],
            whole and d["waves"] == 3)


# ----------------------------------------------------------------------------
# the launch plan: what the library reports, and the same decision restated from the predicates
# ----------------------------------------------------------------------------
SLOTS = ["A", "D", "B", "C", "E"]  # the timing slots of GpuME.timing_read


def kernel_names(lib) -> list:
    """Name by kernel id; ids start at 1 and end before the first id without a name."""
    names = [None]
    while lib.svtme_kernel_name(len(names)) is not None:
        names.append(lib.svtme_kernel_name(len(names)).decode())
    return names


def plan_of(lib, job, paths: int = 0, with_sb: bool = True):
    """The library's answer for a job submitted alone -> ([(slot, kernel name)] in launch order, launch key)."""
    ids, slots, key = (C.c_uint8 * 8)(), (C.c_uint8 * 8)(), C.c_uint32()
    n = lib.svtme_job_kernels(C.byref(job), paths, int(with_sb), ids, slots, C.byref(key))
    return [(SLOTS[slots[k]], lib.svtme_kernel_name(ids[k]).decode()) for k in range(n)], key.value


def _l0_short(job) -> bool:
    """Every slot's HME-L0 quadrant has at most 8 rows: the height of get_hme_l0_search_area
    (svtme_device.h, hme_l0_area) with l00 = (0, 0), as svtme_hme_prepare takes it."""
    c = job.ctrl
    for l in range(job.num_lists):
        for r in range(job.num_refs[l]):
            dist = abs(job.picture_number - job.ref_picture_number[l][r]) & 0xFFFF
            mn, mx = c.hme_l0_sa.sa_min.height, c.hme_l0_sa.sa_max.height
            if c.enable_me_sr_adjustment and c.distance_based_hme_resizing:
                is_ver, is_still = True, False
                if c.reduce_hme_l0_sr_th_min and c.reduce_hme_l0_sr_th_max and (l or r):
                    is_ver, is_still = False, True  # |mv| = 0: below 3 * th_min, not above th_max
                yo = 4 if c.enable_me_sr_adjustment == 2 and is_still else 1 if is_ver else 2
                mn, mx = mn // (yo + r), mx // (yo + r)
            f = dist * 5 // 8 + (1 if dist % 8 else 0)
            if min(mn // c.num_hme_sa_h * f, mx // c.num_hme_sa_h) > 8:
                return False
    return True


def kernels_of(S, lib, job, paths: int = 0, with_sb: bool = True) -> list:
    """[(slot, kernel name)] of a job submitted alone, in launch order: the launcher's decision as it
    stood when it evaluated the predicates itself, restated from the exported predicates."""
    d = dispatch_of(S, lib, job)
    c = job.ctrl
    count = {}
    for f in ("a", "a1", "b"):
        buf, n = (C.c_uint8 * 64)(), C.c_uint32()
        getattr(lib, f"svtme_stage_{f}_list")(C.byref(job), buf, C.byref(n))
        count[f] = n.value
    b = lambda v: "true" if v else "false"  # noqa: E731
    full, k32, rt = d["full_me"], d["k32"], d["rt"]
    fused = d["fused"] and not paths & S.PATH_NO_FUSED_HME
    parts = lib.svtme_fp_parts_paths(C.byref(c), paths)
    wide_lds = d["fp_wide_lds"] and not paths & S.PATH_NO_FP_WIDE
    if fused and parts == 1 and not paths & S.PATH_SPLIT_PASS:
        waves = 4 if paths & S.PATH_HME_4WAVES else d["waves"]
        if waves == 3:
            return [("A", f"k_hme<true, true, {b(k32)}, false, 3>")]
        return [("A", f"k_hme<true, {b(not full)}, {b(k32)}, {b(rt)}>")]
    out = []
    if fused:
        out.append(("A", f"k_hme<false, true, true, {b(rt)}>"))
    else:
        if count["a"] and d["l0_full"] and not paths & S.PATH_NO_L0_FULL:
            out.append(("A", "k_l0_full<2>" if _l0_short(job) else "k_l0_full<4>"))
        elif count["a"]:
            out.append(("A", "k_stage_a<false>"))
        if rt:
            out.append(("A", "k_stage_d<true>"))
            if count["a1"]:
                out.append(("A", "k_stage_a<true>"))
        out.append(("D", "k_stage_d<false>"))
        if count["b"] and d["l1_full"] and not paths & S.PATH_NO_L1_FULL:
            out.append(("B", "k_l1_full"))
        elif count["b"]:
            out.append(("B", f"k_stage_b<{b(d['l2'])}>"))
    if parts:
        if wide_lds:
            out.append(("C", "k_fp_wide"))
        elif k32 and d["fp_wide"]:
            out.append(("C", f"k_stage_c1<{b(not full)}, true, true>"))
        else:
            out.append(("C", f"k_stage_c1<{b(not full)}, {b(k32)}>"))
        if not (job.me_type == S.ME_MCTF and parts == 1 and not with_sb and not wide_lds):
            out.append(("E", "k_stage_e"))
    else:
        out.append(("C", f"k_stage_c<{b(not full)}>"))
    return out


def launch_key_before(S, lib, job, paths: int = 0) -> tuple:
    """The thirteen facts svtme_launch_key packed before it became a packing of the launch plan,
    under path bits `paths` (launch_class is the same at paths 0)."""
    d = dispatch_of(S, lib, job)
    parts = lib.svtme_fp_parts_paths(C.byref(job.ctrl), paths)
    fused = d["fused"] and not paths & S.PATH_NO_FUSED_HME
    whole = fused and parts == 1 and not paths & S.PATH_SPLIT_PASS
    waves = 4 if paths & S.PATH_HME_4WAVES else d["waves"]
    return (d["full_me"], parts != 0, d["k32"], d["l2"], fused, parts == 1, d["fp_wide"], d["rt"],
            d["fp_wide_lds"] and not paths & S.PATH_NO_FP_WIDE, d["l1_full"] and not paths & S.PATH_NO_L1_FULL,
            d["l0_full"] and not paths & S.PATH_NO_L0_FULL, bool(paths & S.PATH_SPLIT_PASS), whole and waves == 3)


def _role(slot: str, name: str) -> tuple:
    """What a kernel does in its launch: its slot and, in slot A, its place in the real-time round;
    k_l0_full's rows per lane are one of the two facts a launch reduces over its jobs."""
    return (slot, {"k_stage_d<true>": 1, "k_stage_a<true>": 2}.get(name, 0))


def one_launch(a: list, b: list) -> bool:
    """Two jobs' kernel lists can be one launch: wherever both run a kernel in the same role it is the
    same kernel. A job leaves a role out when it has no work units for it (no HME levels 1 / 2: no
    slot B) or when a reducible fact says so (every record direct: no k_stage_e)."""
    ra = {_role(s, n): "k_l0_full" if n.startswith("k_l0_full") else n for s, n in a}
    rb = {_role(s, n): "k_l0_full" if n.startswith("k_l0_full") else n for s, n in b}
    return all(ra[r] == rb[r] for r in ra.keys() & rb.keys())
