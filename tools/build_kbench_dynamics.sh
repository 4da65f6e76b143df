#!/bin/bash
# builds tools/kbench_dynamics_bin (gfx950); header-only: includes mpopis_amd/csrc/car_dynamics.h and links nothing of the library
set -e
cd "$(dirname "$0")/.."
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-result -c tools/kbench_dynamics.hip -o tools/kbench_dynamics.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 tools/kbench_dynamics.o -o tools/kbench_dynamics_bin
ls -la tools/kbench_dynamics_bin
