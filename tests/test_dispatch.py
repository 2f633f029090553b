"""Host-side kernel dispatch (no GPU needed: pure host functions of libsvtme.so,
svtme_dispatch.cpp). The full-pel stage: the 64x64 override (BASELINE configs[1])
takes k_fp_wide (svtme_stages.hip) with bands in groups of 4 of at most 8 rows; no
default preset's controls change path. The launch plan: the kernels the library
reports for a job, its launch key and the kernel table."""
import ctypes as C
import math

import pytest


@pytest.fixture(scope="module")
def lib(svtme):
    lib = svtme.load_product()
    for f in ("svtme_fp_wide_lds", "svtme_fp_wide", "svtme_fp_k32"):
        getattr(lib, f).argtypes = [C.POINTER(svtme.Controls)]
        getattr(lib, f).restype = C.c_bool
    lib.svtme_fp_parts.argtypes = [C.POINTER(svtme.Controls)]
    lib.svtme_fp_parts.restype = C.c_uint32
    return lib


def test_override_takes_k_fp_wide(svtme, lib):
    import workloads as W

    job = W.workload_job("1080p_sa64")
    c = job.ctrl
    assert lib.svtme_fp_wide_lds(C.byref(c))
    parts = lib.svtme_fp_parts(C.byref(c))
    h = c.me_sa.sa_max.height
    assert parts % 4 == 0 and parts >= math.ceil(h / 8) and parts <= 16
    # LDS rows of a workgroup: 4 bands + 62 (FPW_ROWS = 96)
    assert 4 * math.ceil(h / parts) + 62 <= 96


def test_no_default_preset_changes_path(svtme, lib):
    for m in range(14):
        for res in range(7):
            for tl in range(4):
                c = svtme.derive_controls(m, 35, res, tl)
                assert not lib.svtme_fp_wide_lds(C.byref(c)), (m, res, tl)
    for lvl in range(5):
        for res in range(7):
            c = svtme.derive_controls_tf(lvl, 0, 35, res)
            assert not lib.svtme_fp_wide_lds(C.byref(c)), (lvl, res)


def test_full_sad_and_64bit_keys_keep_the_register_path(svtme, lib):
    import workloads as W

    c = W.workload_job("1080p_sa64").ctrl
    c.me_search_method = svtme.FULL_SAD_SEARCH
    assert not lib.svtme_fp_wide_lds(C.byref(c))
    c = W.workload_job("1080p_sa64").ctrl
    c.me_sa.sa_max.width = c.me_sa.sa_min.width = 96  # wider than the LDS row
    assert not lib.svtme_fp_wide_lds(C.byref(c))


# ----------------------------------------------------------------------------
# The launch plan (svtme_dispatch.cpp): every job of the ME sweep and the BASELINE workloads, under
# no path bit and under each single one
# ----------------------------------------------------------------------------
# kernels of the launch table that no job below reaches, under any path bit, with or without SB results
UNREACHED = ["k_hme<true, true, true, true>", "k_hme<true, true, false, false>", "k_hme<true, true, false, false, 3>",
             "k_stage_c<false>", "k_l0_full<4>", "k_hme<true, false, true, true>", "k_hme<true, false, false, true>",
             "k_hme<true, false, false, false>", "k_hme<true, true, false, true>"]


@pytest.fixture(scope="module")
def plans(svtme):
    """[(path bits, [(job name, job, library's kernels with SB results, launch key)])]"""
    import me_sweep as M
    import workloads as W

    lib = M.plan_lib_of(svtme)
    jobs = [(c["name"], M.job_of(svtme, c, M.controls_of(svtme, c))) for c in M.cases()]
    jobs += [(n, W.workload_job(n)) for n in W.WORKLOADS]
    out = []
    for paths in [0] + [getattr(svtme, "PATH_" + b) for b in M.PATH_BITS]:
        out.append((paths, [(n, j) + M.plan_of(lib, j, paths) for n, j in jobs]))
    return lib, out


def test_kernel_list_is_the_launcher_restated_from_the_predicates(svtme, plans):
    import me_sweep as M

    lib, by_paths = plans
    for paths, rows in by_paths:
        for name, job, kernels, _ in rows:
            assert kernels == M.kernels_of(svtme, lib, job, paths), (name, paths)
            assert M.plan_of(lib, job, paths, False)[0] == M.kernels_of(svtme, lib, job, paths, False), (name, paths)


def test_launch_key_groups_jobs_as_it_always_has(svtme, plans):
    """Two jobs have equal keys exactly when the thirteen facts the key used to pack are equal
    (launch_key_before; at no path bit, launch_class), and jobs of equal keys run the same kernels.
    Equal kernel lists do not make equal keys, and never did: the key also separates jobs by facts
    that pick no kernel of theirs (LaunchPlan.cls; HME level 2 for a whole-pass k_hme job). Among
    these jobs at no path bit, 29 pairs run the same kernels under different keys."""
    import itertools

    import me_sweep as M

    lib, by_paths = plans
    for paths, rows in by_paths:
        before = [M.launch_key_before(svtme, lib, job, paths) for _, job, _, _ in rows]
        if paths == 0:  # launch_class lacks the SPLIT_PASS bit, which is a constant of the context
            assert [b[:11] + b[12:] for b in before] == [M.launch_class(M.dispatch_of(svtme, lib, j)) for _, j, _, _ in rows]
        for (x, bx), (y, by) in itertools.combinations(zip(rows, before), 2):
            assert (x[3] == y[3]) == (bx == by), (paths, x[0], y[0])
            if x[3] == y[3]:
                assert M.one_launch(x[2], y[2]), (paths, x[0], y[0])


def test_every_kernel_id_has_a_name_and_the_unreached_ones_are_listed(svtme, plans):
    import me_sweep as M

    lib, by_paths = plans
    names = M.kernel_names(lib)
    assert len(names) == 32 and len(set(names)) == 32 and lib.svtme_kernel_name(32) is None
    seen = set()
    for paths, rows in by_paths:
        for _, job, kernels, _ in rows:
            seen.update(n for _, n in kernels + M.plan_of(lib, job, paths, False)[0])
    assert seen <= set(names[1:])
    assert sorted(set(names[1:]) - seen) == sorted(UNREACHED)
