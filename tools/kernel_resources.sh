#!/bin/bash
# Per-kernel register / LDS / scratch use and instruction count: compiles every translation unit of spectrobot_amd/csrc
# but the host API's (sr_api.hip holds no kernel) device-only, SR_JOBS (16) at a time, with the flags of
# spectrobot_amd/build.py, and reads the code objects' metadata and disassembly.
# usage: tools/kernel_resources.sh [pattern [other_csrc [old=new ...]]]
# With another tree's csrc directory (e.g. `git archive HEAD~1 spectrobot_amd/csrc include | tar -x -C <dir>`, then
# <dir>/spectrobot_amd/csrc), whatever units that tree has, every kernel is also compared, instruction for instruction,
# with the other tree's kernel of the same demangled name, whichever unit holds it on either side; old=new pairs rename
# the other tree's kernels first (re.sub on the demangled name).  A last line counts the kernels identical, new, gone
# and differing.  A kernel that two units of one tree hold is an error: the union would hide one of them.
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
export -f build
export tmp SR_EXTRA_FLAGS
units() { ls "$1"/*.hip | grep -v '/sr_api\.hip$'; }
build_tree() { # csrc directory, tag: its units side by side
  local src unit
  units "$1" | xargs -P "${SR_JOBS:-16}" -I{} bash -c \
    'unit=$1.$(basename "$0" .hip); build "$0" "$unit" 2> "$tmp/$unit.log" && touch "$tmp/$unit.ok"' {} "$2" || true
  for src in $(units "$1"); do
    unit=$2.$(basename "$src" .hip)
    [ -e "$tmp/$unit.ok" ] || { cat "$tmp/$unit.log" >&2; echo "$src did not compile" >&2; exit 1; }
  done
}
build_tree "$root/spectrobot_amd/csrc" k
[ -n "$2" ] && build_tree "$2" other
python3 - "$tmp" "$@" <<'EOF'
import glob, os, sys, re, subprocess
tmp, pat, renames = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else ""), [a.split("=", 1) for a in sys.argv[4:]]
def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"^void sr::", "", n).rsplit("(", 1)[0] for n in out[:len(names)]]
def load_unit(stem):  # demangled name -> (metadata block, [instructions])
    blocks = open(stem + ".notes").read().split("- .agpr_count")[1:]
    meta = {re.search(r"\.name:\s*(\S+)", b)[1]: b for b in blocks}
    code, cur = {}, None
    for line in open(stem + ".dis"):
        m = re.match(r"^[0-9a-f]* ?<(\S+)>:", line)
        if m:
            cur = code.setdefault(m[1], [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s+", " ", line.split("//")[0]).strip())
    for c in code.values():  # (the padding behind a kernel's last instruction; "...": padding objdump left out; a zero
        # word of padding between two kernels decodes as v_cndmask_b32_e32 v0, s0, v0, vcc)
        while c and (c[-1].startswith(("s_nop", "s_code_end", "...")) or c[-1] == "v_cndmask_b32_e32 v0, s0, v0, vcc"):
            c.pop()
    sym = list(meta)
    return {d: (meta[s], code.get(s, [])) for s, d in zip(sym, demangle(sym))}
def load(tag):  # the union over the tree's units
    all_ = {}
    for notes in sorted(glob.glob(os.path.join(tmp, tag + ".*.notes"))):
        unit = load_unit(notes[:-len(".notes")])
        twice = unit.keys() & all_.keys()
        if twice:
            sys.exit("in more than one unit (%s among them): %s" % (os.path.basename(notes).split(".")[1], ", ".join(sorted(twice))))
        all_.update(unit)
    return all_
mine = load("k")
other = load("other") if len(sys.argv) > 3 else None
if other:
    for old, new in renames:
        other = {re.sub(old, new, k): v for k, v in other.items()}
count = {"identical": 0, "new": 0, "gone": 0, "differs": 0}
for name, (blk, ins) in mine.items():
    if pat not in name:
        continue
    g = lambda k, b=blk: (re.search(r"\." + k + r":\s*(\S+)", b) or [None, "?"])[1]
    line = "%-58s vgpr %4s sgpr %4s lds %6s scratch %5s insns %5d" % (name[:58], g("vgpr_count"), g("sgpr_count"), g("group_segment_fixed_size"), g("private_segment_fixed_size"), len(ins))
    if other is not None:
        o = other.get(name)
        verdict = "new" if o is None else "identical" if o[1] == ins else "differs"
        count[verdict] += 1
        line += "  " + (verdict if verdict != "differs" else "differs (other: vgpr %s sgpr %s scratch %s insns %d)" % (g("vgpr_count", o[0]), g("sgpr_count", o[0]), g("private_segment_fixed_size", o[0]), len(o[1])))
    print(line)
if other is not None:
    for name in other:
        if pat in name and name not in mine:
            count["gone"] += 1
            print("%-58s gone" % name[:58])
    print("%d identical, %d new, %d gone, %d differ" % (count["identical"], count["new"], count["gone"], count["differs"]))
EOF
