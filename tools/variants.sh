#!/bin/bash
# Build compile-time variants of the HIP library for A/B timing on the GPU box:
#   tools/variants.sh NAME "-DFLAG=.. -DFLAG2=.." [NAME2 "FLAGS2" ...]
# Each lands in build/var/NAME/libapprox_counter_amd.so; run bench.py with
# APPROX_COUNTER_AMD_LIB=build/var/NAME/libapprox_counter_amd.so.
set -e
cd "$(dirname "$0")/.."
while [ $# -gt 1 ]; do
  name=$1; flags=$2; shift 2
  make -s -j"${MAX_JOBS:-16}" lib OUT=build/var/$name EXTRA_FLAGS="$flags"
  echo "built build/var/$name"
done
