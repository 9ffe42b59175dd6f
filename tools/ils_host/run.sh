#!/bin/bash
# The tabulated line shape's weights kernel on the host, under AddressSanitizer and UBSan (see main.cpp).  usage: tools/ils_host/run.sh
set -e
here=$(cd "$(dirname "$0")" && pwd)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
python3 "$here/extract.py" "$tmp"
${CXX:-/opt/rocm/lib/llvm/bin/clang++} -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
  -I"$tmp" "$here/main.cpp" -o "$tmp/ils_host"
"$tmp/ils_host"
