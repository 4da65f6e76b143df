"""Building and running the kernel harnesses (tools/kbench_<x>_bin) from the GPU tests.  The rule for a shared GPU lives in run(): after a hang or
a fault nothing more is started on the card, so the pytest session ends there (exit status 3) with what the process left."""
import os, shutil, subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(name, library=True):
    """tools/kbench_<name>_bin, built by tools/build_kbench.sh; library: build the library first (the harness links its object files)"""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available to build the harness")
    if library:
        from mpopis_amd import build as lib
        lib.build()
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "build_kbench.sh"), name], capture_output=True, text=True, timeout=600)
    exe = os.path.join(ROOT, "tools", "kbench_%s_bin" % name)
    assert out.returncode == 0 and os.path.exists(exe), out.stdout + out.stderr
    return exe


def run(cmd, timeout=120, env=None):
    """one process on the GPU -> its CompletedProcess; a hang, a crash, an abort or a `HIP error` line ends the session"""
    tool = os.path.relpath(cmd[0], ROOT)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired as t:
        pytest.exit("%s hung: %s" % (tool, str(t.stdout)[-2000:]), returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139) or "HIP error" in r.stdout:
        pytest.exit("%s died (%s): %s" % (tool, r.returncode, (r.stdout + r.stderr)[-2000:]), returncode=3)
    return r


def run_case(exe, tmp_path, data, env=None):
    """writes case.bin, runs `exe case.bin result.bin` -> the bytes of result.bin"""
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(fin, "wb") as f:
        f.write(data)
    if os.path.exists(fout):
        os.remove(fout)
    r = run([exe, fin, fout], env=env)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    with open(fout, "rb") as f:
        return f.read()
