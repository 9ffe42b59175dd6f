#!/bin/bash
# A host harness (tools/<name>/main.cpp: state_bands_host, state_gases_host, state_pointing_host, ils_host, absorber_table_host, limb_plan_host, many_gases_host, solar_source_host, solar_jacobian_host, diffuse_source_host, diffuse_jacobian_host, diffuse_optics_host, diffuse_columns_host)
# built as a stand-alone program with AddressSanitizer and UBSan against the library's own kernel and plan files, and run.
# usage: tools/host_sim/run.sh <name>
set -e
name=${1:?usage: tools/host_sim/run.sh <name>}
root=$(cd "$(dirname "$0")/../.." && pwd)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
# (-Wno-psabi: sr_solar_tile.inc's helpers return four doubles as a vector, inlined within the one unit: no ABI is crossed)
${CXX:-/opt/rocm/lib/llvm/bin/clang++} -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
  -Wno-psabi -pthread -I"$root/spectrobot_amd/csrc" -I"$root/tools/host_sim" "$root/tools/$name/main.cpp" -o "$tmp/$name"
"$tmp/$name"
