"""svtme_hme_waves (wavefronts per k_hme workgroup) is a pure function of the job
fields the launch key is made of: jobs that differ only in what the key ignores
(pictures, size, content thresholds) get the same answer, it is 3 or 4, and
SVTME_PATH_HME_4WAVES gives 4. Host code only: no GPU."""
import ctypes as C
import itertools


def test_hme_waves_is_pure_and_forced_by_the_path_bit(svtme):
    S = svtme
    lib = S.load_product()
    lib.svtme_hme_waves.argtypes = [C.POINTER(S.Job)]
    lib.svtme_hme_waves.restype = C.c_uint32
    lib.svtme_hme_waves_paths.argtypes = [C.POINTER(S.Job), C.c_uint32]
    lib.svtme_hme_waves_paths.restype = C.c_uint32
    lib.svtme_hme_rt.argtypes = [C.POINTER(S.Controls)]
    lib.svtme_hme_rt.restype = C.c_bool
    seen = {}
    lists = [((7,), ()), ((7,), (9,)), ((7, 6), (9, 10)), ((7, 6, 5), (9, 10)), ((7, 6, 5, 4), (9, 10, 11, 12))]
    for mode, res, (l0, l1) in itertools.product((4, 6, 8, 12), (S.RES_240P, S.RES_1080P, S.RES_4K), lists):
        ctrl = S.derive_controls(mode, 35, res, 1)
        for full, rt in itertools.product((0, 1), (0, 1)):
            ctrl.me_search_method = S.FULL_SAD_SEARCH if full else S.SUB_SAD_SEARCH
            ctrl.reduce_hme_l0_sr_th_min, ctrl.reduce_hme_l0_sr_th_max = (100, 200) if rt else (0, 0)
            answers = set()
            # what the key ignores: the pictures, the size, thresholds of the content decisions
            for w, h, pn, zz in ((192, 136, 8, 0), (3840, 2160, 4008, 81920), (320, 192, 77, 5)):
                c2 = S.Controls.from_buffer_copy(ctrl)
                c2.zz_sad_th = zz
                job = S.make_job(w, h, c2, pn, [pn - 8 + t for t in l0], [pn - 8 + t for t in l1],
                                 temporal_layer_index=1, ref_count_used=(max(len(l0), 1), len(l1)))
                v = lib.svtme_hme_waves(C.byref(job))
                assert v in (3, 4)
                assert lib.svtme_hme_waves(C.byref(job)) == v  # the same job again
                assert lib.svtme_hme_waves_paths(C.byref(job), 0) == v
                assert lib.svtme_hme_waves_paths(C.byref(job), S.PATH_HME_4WAVES) == 4
                assert lib.svtme_hme_waves_paths(C.byref(job), S.PATH_NO_FP_WIDE) == v  # another path's bit
                answers.add(v)
            assert len(answers) == 1, (mode, res, l0, l1, full, rt)
            key = (bool(full), bool(lib.svtme_hme_rt(C.byref(ctrl))), bool(ctrl.enable_hme_level2_flag),
                   len(l0) + len(l1))
            assert seen.setdefault(key, answers) == answers, key
    assert {3} in seen.values() and {4} in seen.values()  # both shapes are in use
