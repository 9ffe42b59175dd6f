#!/usr/bin/env python3
"""The text of sr_lowres_weights_tab_kernel cut out of sr_kernels.hip for the host build of main.cpp:
usage extract.py <output directory>."""
import os
import sys

out_dir = sys.argv[1]
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "spectrobot_amd", "csrc") + os.sep
ker = open(root + "sr_kernels.hip").read()
a = ker.index("template <bool INSTR>\n__global__ __launch_bounds__(256) void sr_lowres_weights_tab_kernel(")
b = ker.index("constexpr int kLowresBands", a)
open(os.path.join(out_dir, "kernel_text.inc"), "w").write(ker[a:b])
