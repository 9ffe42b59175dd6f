#!/usr/bin/env python3
"""The text of sr_limb_jac_state_kernel, of what it calls and of its host plan (level_jac_plan), cut out of the sources
for the host build of main.cpp: usage extract.py <output directory>."""
import os
import re
import sys

out_dir = sys.argv[1]
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "spectrobot_amd", "csrc") + os.sep
dev = open(root + "sr_device.hpp").read()
ker = open(root + "sr_kernels.hip").read()
hpp = open(root + "sr_kernels.hpp").read()
def between(s, a, b):
    i = s.index(a); j = s.index(b, i)
    return s[i:j]
out = []
out.append(between(dev, "constexpr double kTref", "constexpr double kAvogadro"))
out.append(between(dev, "struct Atten {", "// Regions 3 and 4 at c2"))
out.append(between(hpp, "struct LimbOpts {", "// prof[g] = sum_p"))
out.append(between(hpp, "struct __attribute__((aligned(16))) LevelEnt {", "int launch_limb_jac_state("))
out.append(between(ker, "__device__ inline double limb_initial(", "// Block -> (point block, ray)"))
out.append(between(ker, "__device__ inline bool limb_block(", "__host__ inline unsigned limb_grid"))
out.append(between(ker, "template <int NG>\n__device__ __forceinline__ void limb_load_coef", "template <int NG>\n__global__ __launch_bounds__(256) void sr_limb_kernel"))
out.append(between(ker, "struct FoldBands {", "// Derivatives w.r.t. LEVEL parameters"))
out.append(between(ker, "template <int NG, int NP, bool COLS, bool ROWS, bool BANDS, bool INSTR, class... RowSpectra>", "// The radiance budget of a ray batch"))
txt = "\n".join(out)
txt = re.sub(r'if constexpr \(COLS\) asm volatile\(""[^;]*;', "", txt)
open(os.path.join(out_dir, "kernel_text.inc"), "w").write(txt)
api = open(root + "sr_api.hip").read()
plan = between(api, "std::vector<int> order_by_level(int n, const int32_t *level) {", "struct LosShape {")
plan += between(api, "struct LevelJacPlan {", "// What the entries below do once their arguments are checked")
open(os.path.join(out_dir, "plan_text.inc"), "w").write(plan)
