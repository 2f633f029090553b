"""The launch plan against what the GPU ran: with timing on, a job submitted alone leaves a time above
0 in exactly the timing slots its plan fills (svtme_job_kernels), one job per kernel family of
svtme_stages.hip and per path bit that moves it. Pictures of at most 12 SBs."""
import pytest

import me_sweep as M

BASE = 7_300_000  # picture numbers of this module


def preset8(S, w, h, **mut):
    return M.apply_mut(S, S.derive_controls(8, 35, S.input_resolution_of(w, h), 1), mut)


def cases(S):
    """[(name, w, h, controls, job keywords, [path bit names], kernels the plan must hold at no path bit)]"""
    import workloads as W

    # TF-ME level 0 keeps HME level 2, so its HME-L1 stays with k_stage_b; level 1 is the first that k_l1_full takes
    tf0, tf1 = (S.derive_controls_tf(lvl, 0, 35, S.input_resolution_of(192, 136)) for lvl in (0, 1))
    tf = {"me_type": S.ME_MCTF, "tf_me_exit_th": 0}
    rt = preset8(S, 64, 64, enable_me_sr_adjustment=1, distance_based_hme_resizing=1, reduce_hme_l0_sr_th_min=100,
                 reduce_hme_l0_sr_th_max=200)
    return [
        ("whole_pass", 64, 64, preset8(S, 64, 64), {}, [None, "SPLIT_PASS", "NO_FUSED_HME", "HME_4WAVES"],
         ["k_hme<true, true, true, false, 3>"]),
        ("ragged", 72, 40, preset8(S, 72, 40), {}, [None], ["k_stage_a<false>", "k_stage_d<false>", "k_stage_b<false>"]),
        ("tf_level0", 192, 136, tf0, tf, [None, "NO_L0_FULL", "NO_L1_FULL"], ["k_l0_full<4>", "k_stage_b<true>"]),
        ("tf_level1", 192, 136, tf1, tf, [None, "NO_L0_FULL", "NO_L1_FULL"], ["k_l0_full<2>", "k_l1_full"]),
        ("sr_adjustment_2", 64, 64, preset8(S, 64, 64, enable_me_sr_adjustment=2), {}, [None], ["k_stage_c<true>"]),
        ("sa64", 128, 64, W.workload_controls("1080p_sa64"), {}, [None, "NO_FP_WIDE"], ["k_fp_wide", "k_stage_e"]),
        ("real_time", 64, 64, rt, {}, ["NO_FUSED_HME"], None),
    ]


@pytest.mark.gpu
def test_timing_slots_are_the_plans(svtme, gpu):
    S = svtme
    lib = M.plan_lib_of(S)
    seen = set()
    gpu.set_timing(True)
    try:
        for k, (name, w, h, ctrl, kw, bits, must) in enumerate(cases(S)):
            base = BASE + 100 * k
            l0, l1 = ([7], []) if name in ("tf_level0", "tf_level1", "sa64") else ([7, 6], [9])
            job = S.make_job(w, h, ctrl, base + 8, [base + t for t in l0], [base + t for t in l1],
                             temporal_layer_index=1, ref_count_used=(len(l0), len(l1)), **kw)
            frames = S.test_frames("pan", w, h, sorted([8] + l0 + l1))
            for t, f in frames.items():
                gpu.upload(base + t, f)
            try:
                for bit in bits:
                    paths = getattr(S, "PATH_" + bit) if bit else 0
                    plan, _ = M.plan_of(lib, job, paths)
                    names = [n for _, n in plan]
                    if bit is None:
                        assert all(n in names for n in must), (name, names)
                    seen.update(names)
                    gpu.set_paths(paths)
                    gpu.timing_read()
                    gpu.submit(job)
                    launches, ms = gpu.timing_read()
                    print(name, bit, names, ms)
                    assert launches == 1, (name, bit)
                    assert [M.SLOTS[i] for i in range(5) if ms[i] > 0] == sorted({s for s, _ in plan}, key=M.SLOTS.index), \
                        (name, bit, plan, ms)
            finally:
                gpu.set_paths(0)
                for t in frames:
                    gpu.release(base + t)
    finally:
        gpu.set_timing(False)
    # the paths the path bits lead to, and the real-time tune's second round
    for n in ("k_hme<false, true, true, false>", "k_hme<true, true, true, false>", "k_stage_a<false>", "k_stage_b<false>",
              "k_stage_c1<true, true, true>", "k_stage_d<true>", "k_stage_a<true>"):
        assert n in seen, n
