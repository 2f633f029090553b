# Build libsvtme_<name>.so from the product sources with FILES (default
# svtme_stages.hip) taken from git revision REV (default HEAD) -- the "A" side of
# an A/B against the working tree. FILES=all takes every source and header of csrc/ as REV has
# them, a file REV does not have included: the library of REV itself.
# usage: REV=HEAD NAME=base [FILES="svtme_submit.cpp"] [SED='s/#define HT16 3/#define HT16 4/'] bash scripts/build_ab_lib.sh
# (SED: a sed expression applied to the copy of svtme_stages.hip, for one-constant experiments)
set -e
cd "$(dirname "$0")/.."
REV=${REV:-HEAD}; NAME=${NAME:-base}
T=svt-av1-mirror_amd/.ab_src_$NAME; rm -rf "$T"; mkdir -p "$T"  # two levels below the root: the sources include ../../include/svtme.h
cp svt-av1-mirror_amd/csrc/*.hip svt-av1-mirror_amd/csrc/*.cpp svt-av1-mirror_amd/csrc/*.h "$T"/
if [ "${FILES:-}" = all ]; then
  rm -f "$T"/*
  FILES=$(git ls-tree --name-only "$REV" svt-av1-mirror_amd/csrc/ | sed 's|.*/||' | grep -E '\.(hip|cpp|h)$')
fi
for f in ${FILES:-svtme_stages.hip}; do git show "$REV":svt-av1-mirror_amd/csrc/$f > "$T"/$f; done
if [ -n "${SED:-}" ]; then sed -i "$SED" "$T"/svtme_stages.hip; fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wall -Iinclude \
  -o svt-av1-mirror_amd/libsvtme_$NAME.so "$T"/*.hip "$T"/*.cpp
rm -rf "$T"
echo "built svt-av1-mirror_amd/libsvtme_$NAME.so from $REV"
