#!/bin/bash
# The state kernel's band epilogue on the host, under AddressSanitizer and UBSan (see main.cpp).  usage: tools/state_bands_host/run.sh
set -e
here=$(cd "$(dirname "$0")" && pwd)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
python3 "$here/extract.py" "$tmp"
${CXX:-/opt/rocm/lib/llvm/bin/clang++} -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -pthread -I"$tmp" \
  "$here/main.cpp" -o "$tmp/state_bands_host"
"$tmp/state_bands_host"
