#!/bin/bash
# builds tools/kbench_rollout_bin (gfx950) against the current object files (run `python -m mpopis_amd.build` first)
set -e
cd "$(dirname "$0")/.."
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-result -c tools/kbench_rollout.hip -o tools/kbench_rollout.o
# (the launchers of kernels_rollout.o reach into the rest of the library -- coop_max_workgroups, the handle -- so the whole library's objects are linked)
/opt/rocm/bin/hipcc --offload-arch=gfx950 tools/kbench_rollout.o mpopis_amd/lib/obj/*.o -ldl -o tools/kbench_rollout_bin
ls -la tools/kbench_rollout_bin
