# VALU instruction and cycle counters of the k_hme stop-after builds (scripts/build_phase_libs.sh):
# the differences between consecutive builds are the phases' counts. Counters alone, no tracing.
# usage: WL=4k_p8 P=4 [PFX=stop] [PMC="SQ_... TA_..."] [O=output directory] bash scripts/gpu_phase_pmc.sh
#   PFX: the builds are svt-av1-mirror_amd/libsvtme_${PFX}K.so (another prefix: the builds of another revision)
#   FULL: the library of the last row (default svt-av1-mirror_amd/libsvtme.so)
# then: python3 scripts/phase_pmc_summary.py $O [sbs per launch] [out.json] (per-SB counts per phase)
cd "$GRAFT_REPO_ROOT"
WL=${WL:-4k_p8}; P=${P:-4}; PFX=${PFX:-stop}
O=${O:-gpurun_out/phase_pmc}
mkdir -p $O
export TMPDIR=/tmp
for k in ${KS:-1 2 3 4 5 55 6 full}; do
  lib=svt-av1-mirror_amd/libsvtme_$PFX$k.so
  [ "$k" = full ] && lib=${FULL:-svt-av1-mirror_amd/libsvtme.so}
  SVTME_LIB=$lib timeout -s KILL 120 rocprofv3 --kernel-include-regex "k_hme" \
    --pmc ${PMC:-SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_THREAD_CYCLES_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES} \
    -d "$GRAFT_REPO_ROOT/$O/stop$k" -o run --output-format csv -- python3 scripts/phase_cost.py $WL $P stop_after_$k > $O/stop$k.log 2>&1 || { echo "stop$k failed"; tail -5 $O/stop$k.log; exit 1; }
  echo "stop$k done"
done
