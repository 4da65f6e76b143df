#!/bin/bash
# builds tools/kbench_select_bin (gfx950) against the current object files (run `python -m mpopis_amd.build` first)
set -e
cd "$(dirname "$0")/.."
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-result -c tools/kbench_select.hip -o tools/kbench_select.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 tools/kbench_select.o mpopis_amd/lib/obj/kernels_select.o mpopis_amd/lib/obj/kernels_reweight.o mpopis_amd/lib/obj/kernels_ce.o -o tools/kbench_select_bin
ls -la tools/kbench_select_bin
