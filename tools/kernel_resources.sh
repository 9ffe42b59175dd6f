#!/bin/bash
# Per-kernel register / LDS / scratch use and instruction count: compiles sr_kernels.hip device-only (same flags as
# spectrobot_amd/build.py) and reads the code object's metadata and disassembly.
# usage: tools/kernel_resources.sh [pattern [other_sr_kernels.hip [old=new ...]]]
# With another version of the source (e.g. `git show HEAD~1:spectrobot_amd/csrc/sr_kernels.hip` in a directory with its
# headers) every kernel is also compared, instruction for instruction, with the other version's kernel of the same
# name; old=new pairs rename the other version's kernels first (re.sub on the demangled name).
# SR_SOURCE=sr_limb_many.hip: another translation unit of spectrobot_amd/csrc instead of sr_kernels.hip.
set -e
root=$(cd "$(dirname "$0")/.." && pwd)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
build() { # source, name
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fno-gpu-rdc \
    --cuda-device-only -c "$1" -o "$tmp/$2.co" ${SR_EXTRA_FLAGS:-}
  /opt/rocm/lib/llvm/bin/clang-offload-bundler --unbundle --type=o --input="$tmp/$2.co" \
    --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output="$tmp/$2.elf"
  /opt/rocm/lib/llvm/bin/llvm-readelf --notes "$tmp/$2.elf" > "$tmp/$2.notes"
  /opt/rocm/lib/llvm/bin/llvm-objdump -d --no-show-raw-insn --no-leading-addr "$tmp/$2.elf" > "$tmp/$2.dis"
}
build "$root/spectrobot_amd/csrc/${SR_SOURCE:-sr_kernels.hip}" k
[ -n "$2" ] && build "$2" other
python3 - "$tmp" "$@" <<'EOF'
import os, sys, re, subprocess
tmp, pat, renames = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else ""), [a.split("=", 1) for a in sys.argv[4:]]
def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"^void sr::", "", n).rsplit("(", 1)[0] for n in out[:len(names)]]
def load(tag):  # demangled name -> (metadata block, [instructions])
    blocks = open(os.path.join(tmp, tag + ".notes")).read().split("- .agpr_count")[1:]
    meta = {re.search(r"\.name:\s*(\S+)", b)[1]: b for b in blocks}
    code, cur = {}, None
    for line in open(os.path.join(tmp, tag + ".dis")):
        m = re.match(r"^[0-9a-f]* ?<(\S+)>:", line)
        if m:
            cur = code.setdefault(m[1], [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s+", " ", line.split("//")[0]).strip())
    for c in code.values():  # (the padding behind a kernel's last instruction)
        while c and c[-1].startswith(("s_nop", "s_code_end")):
            c.pop()
    sym = list(meta)
    return {d: (meta[s], code.get(s, [])) for s, d in zip(sym, demangle(sym))}
mine = load("k")
other = load("other") if os.path.exists(os.path.join(tmp, "other.dis")) else None
if other:
    for old, new in renames:
        other = {re.sub(old, new, k): v for k, v in other.items()}
for name, (blk, ins) in mine.items():
    if pat not in name:
        continue
    g = lambda k, b=blk: (re.search(r"\." + k + r":\s*(\S+)", b) or [None, "?"])[1]
    line = "%-58s vgpr %4s sgpr %4s lds %6s scratch %5s insns %5d" % (name[:58], g("vgpr_count"), g("sgpr_count"), g("group_segment_fixed_size"), g("private_segment_fixed_size"), len(ins))
    if other is not None:
        o = other.get(name)
        line += "  " + ("new" if o is None else "identical" if o[1] == ins else "differs (other: vgpr %s sgpr %s scratch %s insns %d)" % (g("vgpr_count", o[0]), g("sgpr_count", o[0]), g("private_segment_fixed_size", o[0]), len(o[1])))
    print(line)
if other is not None:
    for name in other:
        if pat in name and name not in mine:
            print("%-58s gone" % name[:58])
EOF
