#!/bin/bash
# builds tools/kbench_<name>_bin (gfx950), one of the kernel harnesses that share tools/kbench_io.h / kbench_dev.h, against the current object
# files (run `python -m mpopis_amd.build` first; dynamics needs none).        usage: tools/build_kbench.sh <name>
set -e
cd "$(dirname "$0")/.."
name=$1
flags=""
obj=mpopis_amd/lib/obj
case "$name" in
    select)   link="$obj/kernels_select.o $obj/kernels_reweight.o $obj/kernels_ce.o" ;;
    # the probe kernels of the harness include mpopis_amd/csrc/philox.h and are compiled with the library's contraction flag
    sample)   link="$obj/kernels_sample.o $obj/kernels_reweight.o"; flags="-ffp-contract=fast" ;;
    # the probe kernels include mpopis_amd/csrc/strat.h (and philox.h through it): the library's contraction flag again
    strat)    link="$obj/kernels_strat.o $obj/kernels_sample.o"; flags="-ffp-contract=fast" ;;
    # header-only: includes mpopis_amd/csrc/car_dynamics.h and links nothing of the library
    dynamics) link="" ;;
    # the launchers reach into the rest of the library (launch_ce_cov_general beside the handle in engine_ais.o, coop_max_workgroups, launch_env_step's
    # custom-env branch), so the whole library's objects are linked
    mfma|adapt|dense|rollout|loop) link="$obj/*.o -ldl" ;;
    # the risk aggregate of a scenario handle: one launcher, one object
    risk)     link="$obj/kernels_risk.o" ;;
    *) echo "usage: $0 select|mfma|adapt|dense|dynamics|rollout|sample|strat|loop|risk"; exit 2 ;;
esac
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 $flags -Wno-unused-result -c tools/kbench_$name.hip -o tools/kbench_$name.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 tools/kbench_$name.o $link -o tools/kbench_${name}_bin
ls -la tools/kbench_${name}_bin
