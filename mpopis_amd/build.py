"""Builds libmpopis_hip.so (gfx950) in-tree with hipcc.  `python -m mpopis_amd.build`.
`build_env(source)` compiles a caller's env (include/mpopis_env.h) to the gfx950 code object that mpopis_create_custom loads."""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libmpopis_hip.so")
SOURCES = ["engine_api.hip", "engine_ais.hip", "engine_harness.hip", "engine_comm.hip", "kernels_rollout.hip", "kernels_rollout_slots.hip", "kernels_rollout_fleet.hip", "kernels_reweight.hip",
           "kernels_sample.hip", "kernels_strat.hip", "kernels_linalg.hip", "kernels_select.hip", "kernels_ce.hip", "kernels_cma.hip", "kernels_invsqrt.hip", "kernels_mfma.hip",
           "kernels_nes.hip", "kernels_plan.hip", "kernels_trace.hip", "kernels_harness.hip", "kernels_risk.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-Wall", "-Wno-unused-function"]
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
ENV_FLAGS = ["--genco", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-I", INCLUDE]      # the library's own optimisation flags


def _newer(a, deps):
    return os.path.exists(a) and all(os.path.getmtime(a) >= os.path.getmtime(d) for d in deps)


def build(force=False, verbose=False):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(LIBDIR, exist_ok=True)
    objdir = os.path.join(LIBDIR, "obj")
    os.makedirs(objdir, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers += [os.path.join(INCLUDE, "mpopis.h"), os.path.join(INCLUDE, "mpopis_env.h")]
    objs, procs = [], []
    for src in SOURCES:
        sp = os.path.join(CSRC, src)
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        objs.append(obj)
        deps = []
        _quoted_includes(sp, deps)                      # (kernels_rollout_slots.hip includes kernels_rollout.hip)
        if not force and _newer(obj, deps + headers):
            continue
        cmd = [hipcc] + FLAGS + ["-c", sp, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    failed = False
    for src, p in procs:
        out = p.communicate()[0].decode()
        if p.returncode != 0:
            failed = True
            sys.stderr.write("hipcc failed for %s:\n%s\n" % (src, out))
        elif verbose and out.strip():
            print(out)
    if failed:
        raise RuntimeError("hipcc compilation failed")
    if procs or not os.path.exists(LIB):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-ldl"]
        subprocess.check_call(cmd)
    return LIB


def _quoted_includes(path, seen):
    """`path` and every file it reaches through #include "..." (next to the including file, or under include/)."""
    if path in seen:
        return
    seen.append(path)
    with open(path, errors="replace") as f:
        names = re.findall(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', f.read(), flags=re.M)
    for n in names:
        for d in (os.path.dirname(path), INCLUDE):
            cand = os.path.normpath(os.path.join(d, n))
            if os.path.isfile(cand):
                _quoted_includes(cand, seen)
                break


def build_env(src_path, out_dir=None, force=False, verbose=False):
    """An env written against include/mpopis_env.h -> gfx950 code object (hipcc --genco; no GPU needed).  Returns the path of
    <out_dir>/<source stem>.hsaco (default out_dir: next to the library).  Rebuilds when the source, mpopis_env.h or any file the source
    includes with quotes is newer, and when the output was made from another source of the same name (<output>.dep records the source)."""
    src_path = os.path.realpath(src_path)
    if not os.path.isfile(src_path):
        raise FileNotFoundError(src_path)
    out_dir = os.path.abspath(out_dir) if out_dir else LIBDIR
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, os.path.splitext(os.path.basename(src_path))[0] + ".hsaco")
    deps = []
    _quoted_includes(src_path, deps)
    if os.path.join(INCLUDE, "mpopis_env.h") not in deps:
        deps.append(os.path.join(INCLUDE, "mpopis_env.h"))
    stamp = out + ".dep"
    same_source = os.path.exists(stamp) and open(stamp).read().strip() == src_path
    if not force and same_source and _newer(out, deps):
        return out
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + ENV_FLAGS + [src_path, "-o", out]
    if verbose:
        print(" ".join(cmd))
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if p.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (src_path, p.stdout.decode()))
    with open(stamp, "w") as f:
        f.write(src_path + "\n")
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
