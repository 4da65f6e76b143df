#!/bin/bash
# builds tools/kbench_mfma_bin (gfx950) against the current object files (run `python -m mpopis_amd.build` first)
set -e
cd "$(dirname "$0")/.."
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-result -c tools/kbench_mfma.hip -o tools/kbench_mfma.o
# (launch_ce_cov_general lives beside the handle in engine_ais.o, so the whole library's objects are linked)
/opt/rocm/bin/hipcc --offload-arch=gfx950 tools/kbench_mfma.o mpopis_amd/lib/obj/*.o -ldl -o tools/kbench_mfma_bin
ls -la tools/kbench_mfma_bin
