#!/bin/bash
# builds tools/kbench_dense_bin (gfx950) against the current object files (run `python -m mpopis_amd.build` first)
set -e
cd "$(dirname "$0")/.."
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-result -c tools/kbench_dense.hip -o tools/kbench_dense.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 tools/kbench_dense.o mpopis_amd/lib/obj/*.o -ldl -o tools/kbench_dense_bin
ls -la tools/kbench_dense_bin
