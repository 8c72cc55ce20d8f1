#!/bin/bash
# Compile one source file of naz_amd/csrc (device only) and print the kernel resource remarks whose
# function name matches a pattern:
#   scripts/part_resources.sh <coupling.hip|made_ar.hip|made_ar_bwd.hip|...> <grep pattern> [extra flags]
src=$1; pat=$2; shift 2
cd "$(dirname "$0")/.."
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Iinclude -c "naz_amd/csrc/$src" \
  -o "/tmp/resources_${src%.*}.o" -fno-slp-vectorize --offload-device-only \
  -Rpass-analysis=kernel-resource-usage "$@" 2>&1 | grep "remark" | \
  awk -v pat="$pat" '/Function Name/ {show = ($0 ~ pat); if (show) print $NF > "/dev/stderr"} show && /VGPRs|Scratch|Occupancy|AGPRs/ {sub(/.*remark: +/, "  "); print}'
