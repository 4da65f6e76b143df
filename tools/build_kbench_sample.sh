#!/bin/bash
# builds tools/kbench_sample_bin (gfx950) against the current object files (run `python -m mpopis_amd.build` first); the probe kernels of the
# harness include mpopis_amd/csrc/philox.h and are compiled with the library's contraction flag
set -e
cd "$(dirname "$0")/.."
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast -Wno-unused-result -c tools/kbench_sample.hip -o tools/kbench_sample.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 tools/kbench_sample.o mpopis_amd/lib/obj/kernels_sample.o mpopis_amd/lib/obj/kernels_reweight.o -o tools/kbench_sample_bin
ls -la tools/kbench_sample_bin
