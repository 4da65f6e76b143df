#!/bin/bash
# builds tools/kbench_loop_bin (gfx950) against the current object files (run `python -m mpopis_amd.build` first)
set -e
cd "$(dirname "$0")/.."
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-result -c tools/kbench_loop.hip -o tools/kbench_loop.o
# (launch_env_step's custom-env branch and the other launchers reach into the rest of the library, so the whole library's objects are linked)
/opt/rocm/bin/hipcc --offload-arch=gfx950 tools/kbench_loop.o mpopis_amd/lib/obj/*.o -ldl -o tools/kbench_loop_bin
ls -la tools/kbench_loop_bin
