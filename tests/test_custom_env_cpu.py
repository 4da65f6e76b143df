"""CPU-side checks (no GPU) of the caller-supplied env seam (include/mpopis_env.h, mpopis_create_custom):
  - mpopis_amd.build.build_env cross-compiles every test env to a gfx950 code object and does not recompile an up-to-date one;
  - mpopis_create_custom validates its arguments before it looks for a device (each error is MPOPIS_ERR_ARG with a telling message; valid
    arguments end in MPOPIS_ERR_HIP "no HIP device" here), and mpopis_create points env_kind = 3 at the new entry point;
  - the SDK restatements of CartPole and MountainCar (tests/helpers/envs), compiled for the HOST through MPOPIS_ENV_FN, follow the
    oracle's envs step by step -- which pins the envs the GPU tests use to check the new path against the oracle."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = os.path.join(ROOT, "tests", "helpers", "envs")
INCLUDE = os.path.join(ROOT, "include")
dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def L():
    from mpopis_amd import build, _lib
    build.build()
    return _lib.lib()


def _has_device(L):
    """does the library itself see a HIP device?  (a built-in handle with valid arguments is created, or refused with MPOPIS_ERR_HIP)"""
    cfg = _cfg()
    cfg.env_kind = 2
    h = C.c_void_p()
    rc = L.mpopis_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        L.mpopis_destroy(h)
    assert rc in (0, -4), (rc, L.mpopis_last_error(None))
    return rc == 0


@pytest.mark.parametrize("name", ["cartpole_sdk", "mountaincar_sdk", "pointmass_sdk"])
def test_build_env_makes_a_code_object_once(name, tmp_path):
    from mpopis_amd import build
    src = os.path.join(ENVS, name + ".hip")
    out = build.build_env(src, out_dir=str(tmp_path))
    assert out == os.path.join(str(tmp_path), name + ".hsaco") and os.path.getsize(out) > 64
    blob = open(out, "rb").read()
    assert blob[:4] == b"\x7fELF" or blob.startswith(b"__CLANG_OFFLOAD_BUNDLE__")
    for sym in (b"mpopis_env_rollout", b"mpopis_env_step", b"mpopis_env_query", b"mpopis_env_abi"):
        assert sym in blob, sym
    stamp = os.stat(out).st_mtime_ns
    assert build.build_env(src, out_dir=str(tmp_path)) == out
    assert os.stat(out).st_mtime_ns == stamp                     # up to date: not compiled again
    os.utime(out, ns=(0, 0))                                     # older than its source: compiled again
    build.build_env(src, out_dir=str(tmp_path))
    assert os.stat(out).st_mtime_ns > 0


def test_build_env_tracks_included_files_and_the_source_behind_a_name(tmp_path):
    from mpopis_amd import build
    body = open(os.path.join(ENVS, "pendulum_sdk.hip")).read()
    a, b, out_dir = tmp_path / "a", tmp_path / "b", tmp_path / "out"
    a.mkdir(); b.mkdir()
    (a / "dyn.inc").write_text(body)
    (a / "env.hip").write_text('#include "dyn.inc"\n')
    (b / "env.hip").write_text(body.replace("MPOPIS_DEFINE_ENV(2, 1, 0,", "MPOPIS_DEFINE_ENV(2, 1, 3,"))
    out = build.build_env(str(a / "env.hip"), out_dir=str(out_dir))
    first = open(out, "rb").read()
    os.utime(out, ns=(10 ** 18, 10 ** 18))
    os.utime(str(a / "dyn.inc"), ns=(2 * 10 ** 18, 2 * 10 ** 18))          # the included file is newer than the output: compiled again
    build.build_env(str(a / "env.hip"), out_dir=str(out_dir))
    assert os.stat(out).st_mtime_ns != 10 ** 18 and open(out, "rb").read() == first
    os.utime(str(a / "dyn.inc"), ns=(10 ** 18, 10 ** 18))
    assert build.build_env(str(b / "env.hip"), out_dir=str(out_dir)) == out   # same stem, another source: not the first env's code object
    assert open(out, "rb").read() != first


def test_default_output_sits_next_to_the_library():
    from mpopis_amd import build
    out = build.build_env(os.path.join(ENVS, "pointmass_sdk.hip"))
    assert os.path.dirname(out) == build.LIBDIR and out.endswith("pointmass_sdk.hsaco")


def _cfg(policy="gmppi", K=8, T=4):
    from mpopis_amd import _lib
    cfg = _lib.Config()
    cfg.env_kind, cfg.num_cars, cfg.policy = 3, 0, _lib.POLICY_IDS[policy]
    cfg.num_samples, cfg.horizon, cfg.batch, cfg.ais_its = K, T, 1, 2
    cfg.lambda_, cfg.alpha, cfg.lambda_ais, cfg.elite_threshold, cfg.cma_sigma = 1.0, 1.0, 20.0, 0.8, 0.01
    return cfg


def _create_custom(L, cfg, blob, nbytes, ss, as_, npar):
    h = C.c_void_p()
    buf = (C.c_char * max(1, len(blob))).from_buffer_copy(blob or b"\0")
    rc = L.mpopis_create_custom(C.byref(cfg), buf, nbytes, ss, as_, npar, None, C.byref(h))
    msg = L.mpopis_last_error(None)
    if rc == 0:
        L.mpopis_destroy(h)
    else:
        assert h.value is None
    return rc, msg


@pytest.fixture(scope="module")
def cartpole_blob():
    from mpopis_amd import build
    return open(build.build_env(os.path.join(ENVS, "cartpole_sdk.hip")), "rb").read()


def test_create_custom_argument_errors(L, cartpole_blob):
    blob = cartpole_blob
    ok = (4, 1, 11)
    rc, msg = _create_custom(L, _cfg(), blob, 0, *ok)
    assert rc == -1 and b"too small" in msg
    rc, msg = _create_custom(L, _cfg(), bytes(64), 64, *ok)
    assert rc == -1 and b"magic" in msg
    for ss in (0, 65):
        rc, msg = _create_custom(L, _cfg(), blob, len(blob), ss, 1, 11)
        assert rc == -1 and b"state_size" in msg, (ss, msg)
    for as_ in (0, 17):
        rc, msg = _create_custom(L, _cfg(), blob, len(blob), 4, as_, 11)
        assert rc == -1 and b"action_size" in msg, (as_, msg)
    rc, msg = _create_custom(L, _cfg(), blob, len(blob), 4, 1, -1)
    assert rc == -1 and b"nparams" in msg
    for cut in (len(blob) // 2, len(blob) - 1, 100):             # a truncated buffer never reaches the runtime, which takes no length
        rc, msg = _create_custom(L, _cfg(), blob[:cut], cut, *ok)
        assert rc == -1 and b"truncated" in msg, (cut, msg)
    from mpopis_amd import build
    elf = open(os.path.join(build.LIBDIR, "libmpopis_hip.so"), "rb").read()[:4096]      # an ELF header whose section table lies far behind 4096 bytes
    rc, msg = _create_custom(L, _cfg(), elf, len(elf), *ok)
    assert rc == -1 and b"truncated" in msg
    rc, msg = _create_custom(L, _cfg("nesmppi", T=103), blob, len(blob), 4, 5, 11)      # cs = 515 > 512
    assert rc == -1 and b"nesmppi" in msg and b"512" in msg
    rc, msg = _create_custom(L, _cfg("nesmppi", T=102), blob, len(blob), 4, 5, 11)      # cs = 510 passes the cap (and fails later: no device, or AS mismatch)
    assert b"control space" not in msg
    h = C.c_void_p()
    assert L.mpopis_create_custom(None, blob, len(blob), 4, 1, 11, None, C.byref(h)) == -1
    assert L.mpopis_create_custom(C.byref(_cfg()), None, len(blob), 4, 1, 11, None, C.byref(h)) == -1
    assert L.mpopis_create_custom(C.byref(_cfg()), blob, len(blob), 4, 1, 11, None, None) == -1


def test_create_custom_with_valid_arguments_needs_a_device(L, cartpole_blob):
    rc, msg = _create_custom(L, _cfg(), cartpole_blob, len(cartpole_blob), 4, 1, 11)
    if _has_device(L):
        assert rc == 0, msg
    else:
        assert rc == -4 and b"no HIP device" in msg, (rc, msg)


def test_plain_create_points_env_kind_3_at_the_new_entry_point(L):
    h = C.c_void_p()
    assert L.mpopis_create(C.byref(_cfg()), C.byref(h)) == -1 and h.value is None
    assert b"mpopis_create_custom" in L.mpopis_last_error(None)


def test_header_keeps_the_abi_and_names_the_addition():
    hdr = open(os.path.join(INCLUDE, "mpopis.h")).read()
    assert "#define MPOPIS_ABI_VERSION 5" in hdr and "MPOPIS_ENV_CUSTOM = 3" in hdr
    assert "mpopis_env_rollout" not in hdr and "mpopis_env_abi" not in hdr      # the kernel names live in mpopis_env.h only


# ---- host shim: the SDK envs against the oracle's ---------------------------------------------------------------------------------------------

def _host_shim(name):
    src = os.path.join(ENVS, name + ".hip")
    so = os.path.join(ROOT, "tests", "shim", "lib" + name + "_host.so")
    deps = [src, os.path.join(INCLUDE, "mpopis_env.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-x", "c++", "-O2", "-fPIC", "-shared", "-std=c++17", "-I", INCLUDE, "-o", so, src])
    S = C.CDLL(so)
    S.mpopis_env_host_step.argtypes = [dp, C.POINTER(C.c_int), C.POINTER(C.c_int), dp, dp]
    S.mpopis_env_host_step.restype = None
    S.mpopis_env_host_reward.argtypes = [dp, C.c_int, C.c_int, dp]
    S.mpopis_env_host_reward.restype = C.c_double
    return S


@pytest.mark.parametrize("kind,sizes", [("cartpole", (1, 4, 1, 11)), ("mountaincar", (1, 2, 1, 8))])
def test_sdk_env_follows_the_oracle_env_on_the_host(oracle, kind, sizes):
    S = _host_shim(kind + "_sdk")
    assert tuple((C.c_int32 * 4).in_dll(S, "mpopis_env_abi")) == sizes
    p = oracle.cartpole_default_params() if kind == "cartpole" else oracle.mountaincar_default_params()
    p = np.ascontiguousarray(p, dtype=np.float64)
    rng = np.random.default_rng(11 if kind == "cartpole" else 12)
    steps, dones = 0, 0
    run = 0
    while steps < 200:
        env = oracle.OracleEnv(kind)
        env.state = rng.uniform(-0.05, 0.05, 4) if kind == "cartpole" else [rng.uniform(-0.6, -0.4), 0.0]
        s = np.array(env.state, dtype=np.float64)
        t, done = C.c_int(0), C.c_int(0)
        run += 1
        while steps < 200:
            a = np.array([float(np.clip(rng.normal(0.5 if run % 2 else 0.0, 0.8), -1, 1))])
            env.step(a)
            S.mpopis_env_host_step(s.ctypes.data_as(dp), C.byref(t), C.byref(done), a.ctypes.data_as(dp), p.ctypes.data_as(dp))
            steps += 1
            assert np.max(np.abs(s - env.state)) <= 1e-13
            assert t.value == env.e.t and done.value == env.e.done
            assert S.mpopis_env_host_reward(s.ctypes.data_as(dp), t.value, done.value, p.ctypes.data_as(dp)) == env.reward()
            if done.value:
                dones += 1
                break
    assert steps == 200
    if kind == "cartpole":
        assert dones >= 1                                        # random pushes drop the pole well inside 200 steps


def test_pointmass_numpy_reference_follows_the_sdk_env_on_the_host():
    """tests/helpers/pointmass_ref.py is the reference of the GPU tests on the point mass (SS = 5, AS = 3): pin it to the env source itself."""
    from tests.helpers import pointmass_ref as PM
    S = _host_shim("pointmass_sdk")
    assert tuple((C.c_int32 * 4).in_dll(S, "mpopis_env_abi")) == (1, PM.SS, PM.AS, PM.NP)
    rng = np.random.default_rng(5)
    p = PM.PARAMS.copy(); p[8] = 7.0                              # done at t = 7
    s = rng.uniform(-1, 1, 5); s[4] = abs(s[4])
    t, done = C.c_int(0), C.c_int(0)
    ref_s, ref_t = s.copy(), 0
    for i in range(12):
        a = np.clip(rng.normal(0, 0.8, 3), PM.LO, PM.HI)
        S.mpopis_env_host_step(s.ctypes.data_as(dp), C.byref(t), C.byref(done), a.ctypes.data_as(dp), p.ctypes.data_as(dp))
        ref_s, ref_t, ref_done = PM.step(ref_s, ref_t, a, p)
        assert np.max(np.abs(s - ref_s)) <= 1e-14 and t.value == ref_t and done.value == ref_done == int(i + 1 >= 7)
        r = S.mpopis_env_host_reward(s.ctypes.data_as(dp), t.value, done.value, p.ctypes.data_as(dp))
        assert abs(r - PM.reward(ref_s, p)) <= 1e-14 * max(1.0, abs(r))


# ---- an env whose functions are called `step` and `reward`, with no parameters ---------------------------------------------------------------

def pendulum_host_rollout(x0, U, E, T):
    """simulate_model through the HOST build of tests/helpers/envs/pendulum_sdk.hip: cost (K,) and the state after the last step (K, 2)"""
    S = _host_shim("pendulum_sdk")
    K = E.shape[0]
    cost, last = np.zeros(K), np.zeros((K, 2))
    for k in range(K):
        s = np.array(x0, dtype=np.float64)
        t, done = C.c_int(0), C.c_int(0)
        for i in range(T):
            a = np.clip(U[i:i + 1] + E[k, i:i + 1], -1.0, 1.0)
            S.mpopis_env_host_step(s.ctypes.data_as(dp), C.byref(t), C.byref(done), a.ctypes.data_as(dp), None)
            cost[k] -= S.mpopis_env_host_reward(s.ctypes.data_as(dp), t.value, done.value, None)
        last[k] = s
    return cost, last


def compare_pendulum_device_with_host():
    """the generated kernels of the step / reward-named env against its host build (needs a device)"""
    import types
    from mpopis_amd import build, engine
    rng = np.random.default_rng(8)
    K, T = 70, 6
    env = types.SimpleNamespace(code_object=build.build_env(os.path.join(ENVS, "pendulum_sdk.hip")), state_size=2, action_size=1,
                                params=np.zeros(0), lo=None, hi=None, reset_state=[0.3, -0.2])
    eng = engine.Engine("custom", 0, "gmppi", K, T, batch=1, lam=1.0, cov=[0.5], log_trajectories=True, custom_env=env)
    x0, _, _ = eng.get_state()
    assert np.array_equal(x0[0], [0.3, -0.2])                    # reset_state
    U, E = rng.uniform(-0.3, 0.3, T), rng.standard_normal((1, K, T))
    ref, last = pendulum_host_rollout(x0[0], U, E[0], T)
    got = eng.rollout_costs(U[None], E)
    assert np.min(ref) > 0.5 and np.ptp(ref) > 0.1               # the dynamics and the reward are in the cost, and it differs by sample
    assert np.max(np.abs(got[0] - ref) / np.abs(ref)) < 1e-12
    assert np.max(np.abs(eng.get_trajectories()[0][:, -1] - last)) < 1e-13
    r = eng.env_step([[0.4]])                                    # the step kernel
    ref1, last1 = pendulum_host_rollout(x0[0], np.array([0.4]), np.zeros((1, 1)), 1)
    assert abs(r[0] + ref1[0]) < 1e-14 and np.max(np.abs(eng.get_state()[0][0] - last1[0])) < 1e-15
    assert abs(eng.env_query()[0][0] + ref1[0]) < 1e-14          # the query kernel
    eng.close()


def test_functions_named_step_and_reward_build_for_host_and_device(L):
    from mpopis_amd import build
    S = _host_shim("pendulum_sdk")
    assert tuple((C.c_int32 * 4).in_dll(S, "mpopis_env_abi")) == (1, 2, 1, 0)
    ref, last = pendulum_host_rollout([0.3, -0.2], np.zeros(4), np.zeros((1, 4)), 4)
    s = np.array([0.3, -0.2])                                    # the same four steps restated
    for _ in range(4):
        s[1] += 0.1 * (0.0 - 0.5 * s[1] - np.sin(s[0])); s[0] += 0.1 * s[1]
    assert np.max(np.abs(last[0] - s)) < 1e-15 and ref[0] > 1.0
    blob = open(build.build_env(os.path.join(ENVS, "pendulum_sdk.hip")), "rb").read()
    assert b"mpopis_env_rollout" in blob
    if _has_device(L):
        compare_pendulum_device_with_host()
