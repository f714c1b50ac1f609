#!/bin/bash
# Build the HIP library of another git revision for same-box A/B timing, with that revision's own
# Makefile (so it works whatever source files the revision has):
#   tools/variant_rev.sh REV NAME ["-DFLAG ..."]  ->  build/var/NAME/libapprox_counter_amd.so
set -e
cd "$(dirname "$0")/.."
rev=$1; name=$2; flags=${3:-}
src=$(mktemp -d)
trap 'rm -rf "$src"' EXIT
git archive "$rev" Makefile approx_counter_amd/csrc include | tar -x -C "$src"
if [ -n "$flags" ] && ! grep -q EXTRA_FLAGS "$src/Makefile"; then
  echo "$rev: its Makefile has no EXTRA_FLAGS, cannot build it with '$flags'" >&2; exit 1
fi
lib=approx_counter_amd/lib/libapprox_counter_amd.so
make -s -C "$src" -j"${MAX_JOBS:-16}" $lib EXTRA_FLAGS="$flags"
out=build/var/$name; mkdir -p $out
cp "$src/$lib" $out/
echo "built $out from $rev"
