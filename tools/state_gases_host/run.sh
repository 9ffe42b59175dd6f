#!/bin/bash
# The state kernel's instances for several level-factored gases and their host plan on the host, under AddressSanitizer
# and UBSan (see main.cpp).  usage: tools/state_gases_host/run.sh
set -e
here=$(cd "$(dirname "$0")" && pwd)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
python3 "$here/../state_bands_host/extract.py" "$tmp"
${CXX:-/opt/rocm/lib/llvm/bin/clang++} -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -pthread -I"$tmp" \
  "$here/main.cpp" -o "$tmp/state_gases_host"
"$tmp/state_gases_host"
