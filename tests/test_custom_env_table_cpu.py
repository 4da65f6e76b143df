"""CPU-side checks (no GPU) of custom envs with a data table (MPOPIS_DEFINE_ENV_TABLE of include/mpopis_env.h, mpopis_set_env_table):
  - the two test envs and the shipped example build to gfx950 code objects with the four table kernels (and none of the plain ones), without
    scratch memory in either rollout kernel, and for the host;
  - the host build of mapnav follows tests/helpers/mapnav_ref.py step by step, the host build of cartpole_tab the oracle's CartPole -- which
    pins the references of the GPU tests to the env sources;
  - the seeds of the GPU tests keep every looked-up position clear of the map's cell edges (the condition their comparisons stand on);
  - the header declares the new call under the unchanged ABI version, _lib.py binds it, and plain MPOPIS_DEFINE_ENV envs build as before."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

from tests.helpers import mapnav_ref as MN
from tests.helpers import mapnav_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = os.path.join(ROOT, "tests", "helpers", "envs")
INCLUDE = os.path.join(ROOT, "include")
dp = C.POINTER(C.c_double)

TABLE_KERNELS = (b"mpopis_env_rollout_tab", b"mpopis_env_rollout_gtab", b"mpopis_env_step_tab", b"mpopis_env_query_tab")


def table_env_sources():
    from mpopis_amd import mapnav_source
    return {"cartpole_tab_sdk": os.path.join(ENVS, "cartpole_tab_sdk.hip"), "mapnav_sdk": os.path.join(ENVS, "mapnav_sdk.hip"),
            "mapnav": mapnav_source()}


def has_symbol(blob, name):
    """`name` as a whole symbol (NUL-terminated in the string table), not as the head of a longer one"""
    return name + b"\0" in blob


@pytest.mark.parametrize("name", ["cartpole_tab_sdk", "mapnav_sdk", "mapnav"])
def test_table_env_builds_to_the_four_table_kernels(name, tmp_path):
    from mpopis_amd import build
    out = build.build_env(table_env_sources()[name], out_dir=str(tmp_path))
    blob = open(out, "rb").read()
    assert blob[:4] == b"\x7fELF" or blob.startswith(b"__CLANG_OFFLOAD_BUNDLE__")
    for sym in TABLE_KERNELS + (b"mpopis_env_table_abi", b"mpopis_env_abi"):
        assert has_symbol(blob, sym), sym
    for sym in (b"mpopis_env_rollout", b"mpopis_env_step", b"mpopis_env_query"):
        assert not has_symbol(blob, sym), sym


@pytest.mark.parametrize("name", ["cartpole_tab_sdk", "mapnav_sdk", "mapnav"])
def test_table_rollout_kernels_use_no_scratch(name, tmp_path):
    from mpopis_amd import build
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.ENV_FLAGS + ["-Rpass-analysis=kernel-resource-usage", table_env_sources()[name],
                                                                              "-o", str(tmp_path / "env.hsaco")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    scratch, fn = {}, None
    for line in p.stdout.decode().splitlines():
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            fn = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and fn:
            scratch[fn] = int(m.group(1))
    assert scratch.get("mpopis_env_rollout_tab") == 0 and scratch.get("mpopis_env_rollout_gtab") == 0, scratch


def _host_shim(name, src=None):
    src = src or os.path.join(ENVS, name + ".hip")
    so = os.path.join(ROOT, "tests", "shim", "lib" + name + "_host.so")
    deps = [src, os.path.join(INCLUDE, "mpopis_env.h")] + ([table_env_sources()["mapnav"]] if name == "mapnav_sdk" else [])
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-x", "c++", "-O2", "-fPIC", "-shared", "-std=c++17", "-I", INCLUDE, "-o", so, src])
    S = C.CDLL(so)
    S.mpopis_env_host_step.argtypes = [dp, C.POINTER(C.c_int), C.POINTER(C.c_int), dp, dp, dp, C.c_int]
    S.mpopis_env_host_step.restype = None
    S.mpopis_env_host_reward.argtypes = [dp, C.c_int, C.c_int, dp, dp, C.c_int]
    S.mpopis_env_host_reward.restype = C.c_double
    return S


def _tabp(tab):
    return tab.ctypes.data_as(dp) if tab.size else None            # ntab == 0: a pointer that must not be dereferenced


def mapnav_host_rollout(x0, U, E, p, tab, lo=MN.LO, hi=MN.HI):
    """simulate_model through the HOST build of tests/helpers/envs/mapnav_sdk.hip: cost (K,) and trajectories (K, T, 4)"""
    S = _host_shim("mapnav_sdk")
    p, tab = np.ascontiguousarray(p, dtype=np.float64), np.ascontiguousarray(tab, dtype=np.float64)
    K, cs = E.shape
    T = cs // MN.AS
    cost, traj = np.zeros(K), np.zeros((K, T, MN.SS))
    for k in range(K):
        s = np.array(x0, dtype=np.float64)
        t, done = C.c_int(0), C.c_int(0)
        for i in range(T):
            a = np.clip(U[MN.AS * i:MN.AS * i + MN.AS] + E[k, MN.AS * i:MN.AS * i + MN.AS], lo, hi)
            S.mpopis_env_host_step(s.ctypes.data_as(dp), C.byref(t), C.byref(done), a.ctypes.data_as(dp), p.ctypes.data_as(dp), _tabp(tab), tab.size)
            cost[k] -= S.mpopis_env_host_reward(s.ctypes.data_as(dp), t.value, done.value, p.ctypes.data_as(dp), _tabp(tab), tab.size)
            traj[k, i] = s
    return cost, traj


@pytest.mark.parametrize("P,G,pad", [(1, 1, 0), (0, 64, 1), (7, 5, 0), (0, 0, 0)])
def test_mapnav_numpy_reference_follows_the_sdk_env_on_the_host(P, G, pad):
    """tolerances of test_pointmass_numpy_reference_follows_the_sdk_env_on_the_host (1e-14; t and done exact)"""
    S = _host_shim("mapnav_sdk")
    assert tuple((C.c_int32 * 4).in_dll(S, "mpopis_env_abi")) == (1, MN.SS, MN.AS, MN.NP)
    assert tuple((C.c_int32 * 2).in_dll(S, "mpopis_env_table_abi")) == (1, 4096)
    rng = np.random.default_rng(100 + 10 * P + G)
    p = MN.params(P, G, max_steps=7)                              # done at t = 7
    tab = MN.make_table(P, G, rng, pad)
    s = np.array([0.71, -0.63, 0.9, -0.8])                        # on its way out of the map: the clamp is hit on the way
    t, done = C.c_int(0), C.c_int(0)
    ref_s, ref_t, margin, left = s.copy(), 0, np.inf, False
    for i in range(14):
        a = np.clip(rng.normal(0, 1.5, 2), MN.LO, MN.HI)
        S.mpopis_env_host_step(s.ctypes.data_as(dp), C.byref(t), C.byref(done), a.ctypes.data_as(dp), p.ctypes.data_as(dp), _tabp(tab), tab.size)
        ref_s, ref_t, ref_done, m1 = MN.step(ref_s, ref_t, a, p, tab)
        assert np.max(np.abs(s - ref_s)) <= 1e-14 and t.value == ref_t and done.value == ref_done == int(i + 1 >= 7)
        r = S.mpopis_env_host_reward(s.ctypes.data_as(dp), t.value, done.value, p.ctypes.data_as(dp), _tabp(tab), tab.size)
        ref_r, m2 = MN.reward(ref_s, p, tab)
        assert abs(r - ref_r) <= 1e-14 * max(1.0, abs(r))
        margin = min(margin, m1, m2)
        left |= bool(np.any(np.abs(ref_s[:2]) > 1.0))
    assert margin >= MN.MARGIN and left


def test_cartpole_tab_follows_the_oracle_env_on_the_host(oracle):
    """as test_sdk_env_follows_the_oracle_env_on_the_host does for cartpole_sdk; the parameters travel in the table"""
    S = _host_shim("cartpole_tab_sdk")
    assert tuple((C.c_int32 * 4).in_dll(S, "mpopis_env_abi")) == (1, 4, 1, 0)
    assert tuple((C.c_int32 * 2).in_dll(S, "mpopis_env_table_abi")) == (1, 4096)
    tab = np.ascontiguousarray(oracle.cartpole_default_params(), dtype=np.float64)
    rng = np.random.default_rng(11)
    steps, dones, run = 0, 0, 0
    while steps < 200:
        env = oracle.OracleEnv("cartpole")
        env.state = rng.uniform(-0.05, 0.05, 4)
        s = np.array(env.state, dtype=np.float64)
        t, done = C.c_int(0), C.c_int(0)
        run += 1
        while steps < 200:
            a = np.array([float(np.clip(rng.normal(0.5 if run % 2 else 0.0, 0.8), -1, 1))])
            env.step(a)
            S.mpopis_env_host_step(s.ctypes.data_as(dp), C.byref(t), C.byref(done), a.ctypes.data_as(dp), None, tab.ctypes.data_as(dp), tab.size)
            steps += 1
            assert np.max(np.abs(s - env.state)) <= 1e-13
            assert t.value == env.e.t and done.value == env.e.done
            assert S.mpopis_env_host_reward(s.ctypes.data_as(dp), t.value, done.value, None, tab.ctypes.data_as(dp), tab.size) == env.reward()
            if done.value:
                dones += 1
                break
    assert steps == 200 and dones >= 1


@pytest.fixture(scope="module")
def level1_references():
    """the NumPy reference of every (table, K) the GPU suite rolls out, computed once"""
    return {(tb, K): MC.level1_reference(MC.level1_case(tb, K)) for tb in MC.TABLES for K in MC.LEVEL1_K}


def test_seeds_of_the_gpu_tests_keep_clear_of_cell_edges(level1_references):
    for key, (cost, traj, margin, outside) in level1_references.items():
        assert margin >= MN.MARGIN, (key, margin)
        assert outside > 0, key                                  # ... and some rollouts do leave the map: the clamp is part of every case
        assert np.all(np.isfinite(cost)) and np.ptp(cost) > 0.0 or cost.shape[1] == 1
    assert MC.level1_reference(MC.empty_table_case())[2] >= MN.MARGIN
    c = MC.mirror_case()                                          # the one env step of the Python-mirror test is checked there, on the action taken
    assert c["tab"].size == 2 * 6 + 64


def test_host_build_agrees_with_the_reference_on_a_gpu_case(level1_references):
    """one whole case of the GPU suite through the host build: the reference's rollout loop (clamp, cost sign, logger) against the env source"""
    case = MC.level1_case("g64pad", 64)
    cost, traj = mapnav_host_rollout(case["x0"][1], case["U"][1], case["E"][1], case["p"], case["tab"])
    ref = level1_references[("g64pad", 64)]
    assert np.max(np.abs(cost - ref[0][1]) / np.abs(ref[0][1])) <= 1e-12
    assert np.max(np.abs(traj - ref[1][1])) <= 1e-12


def test_header_declares_the_call_and_keeps_the_abi_version():
    hdr = open(os.path.join(INCLUDE, "mpopis.h")).read()
    assert "#define MPOPIS_ABI_VERSION 5" in hdr
    assert re.search(r"int\s+mpopis_set_env_table\(mpopis_handle \*h, const double \*data, int64_t n, int32_t per_slot\);", hdr)
    sdk = open(os.path.join(INCLUDE, "mpopis_env.h")).read()
    assert "#define MPOPIS_ENV_SDK_VERSION 1" in sdk and "#define MPOPIS_ENV_TABLE_VERSION 1" in sdk
    assert "#define MPOPIS_ENV_MAX_TABLE (1 << 20)" in sdk and "MPOPIS_DEFINE_ENV_TABLE(SS, AS, NP, STEP, REWARD)" in sdk


def test_python_binds_the_call_and_refuses_without_a_handle():
    from mpopis_amd import build, _lib
    build.build()
    L = _lib.lib()
    assert "mpopis_set_env_table" in _lib.ABI_SYMBOLS
    assert L.mpopis_set_env_table.argtypes == [C.c_void_p, dp, C.c_int64, C.c_int32]
    assert L.mpopis_set_env_table(None, None, 0, 0) == -1
    import mpopis_amd as M
    assert os.path.exists(M.mapnav_source()) and hasattr(M.Engine, "set_env_table") and hasattr(M.CustomEnv, "set_table")


@pytest.mark.parametrize("name", ["cartpole_sdk", "pointmass_sdk"])
def test_plain_envs_still_build_to_the_three_plain_kernels(name, tmp_path):
    from mpopis_amd import build
    blob = open(build.build_env(os.path.join(ENVS, name + ".hip"), out_dir=str(tmp_path)), "rb").read()
    for sym in (b"mpopis_env_rollout", b"mpopis_env_step", b"mpopis_env_query", b"mpopis_env_abi"):
        assert has_symbol(blob, sym), sym
    for sym in TABLE_KERNELS + (b"mpopis_env_table_abi",):
        assert not has_symbol(blob, sym), sym
