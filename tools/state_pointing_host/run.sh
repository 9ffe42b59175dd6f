#!/bin/bash
# The state kernel's text and its host plan with the hidden column slots of the pointing derivative on the host, under
# AddressSanitizer and UBSan (see main.cpp).  usage: tools/state_pointing_host/run.sh
set -e
here=$(cd "$(dirname "$0")" && pwd)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
python3 "$here/../state_bands_host/extract.py" "$tmp"
${CXX:-/opt/rocm/lib/llvm/bin/clang++} -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -pthread -I"$tmp" \
  "$here/main.cpp" -o "$tmp/state_pointing_host"
"$tmp/state_pointing_host"
