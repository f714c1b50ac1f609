#!/bin/bash
# Build the HIP library from a source tree (a copy of include/ + approx_counter_amd/csrc/ with an
# experiment undone or applied; built with this tree's Makefile) for same-box A/B timing:
#   tools/variant_dir.sh DIR NAME ["-DFLAG ..."]  ->  build/var/NAME/libapprox_counter_amd.so
set -e
cd "$(dirname "$0")/.."
src=$1; name=$2; flags=${3:-}
make -s -j"${MAX_JOBS:-16}" lib SRC="$src" OUT=build/var/$name EXTRA_FLAGS="$flags"
echo "built build/var/$name from $src"
