""":nesmppi without a GPU: the ABI constant, the Python mirror, create-time argument checks, and the two anchors of the NumPy reference
(tests/helpers/nes_ref.py) -- against the oracle's :gmppi call and against the per-sample Gaussian score gradients of
src/mppi_mpopi_policies.jl:872-878."""
import ctypes as C
import inspect
import os
import re
import numpy as np
import pytest

from tests.helpers.nes_ref import nes_ref, nes_gradients, inv_from_chol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from mpopis_amd import build, _lib
    build.build()
    return _lib.lib()


def test_nes_policy_id_header_lib_and_mirror_agree():
    from mpopis_amd import _lib
    import mpopis_amd
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpopis.h")).read(), flags=re.S)
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"(MPOPIS_POL_\w+)\s*=\s*(\d+)", hdr)}
    assert enum["MPOPIS_POL_NESMPPI"] == 8
    assert _lib.POLICY_IDS["nesmppi"] == 8
    cls = mpopis_amd.NESMPPI_Policy
    assert cls._kind == "nesmppi"
    sig = inspect.signature(cls.__init__)
    assert sig.parameters["opt_its"].default == 10                 # :842
    assert sig.parameters["step_factor"].default == 0.01           # :843
    assert inspect.signature(mpopis_amd.Engine.__init__).parameters["step_factor"].default == 0.01
    assert re.search(r"double\s+cma_sigma;\s*/\*[^*]*step_factor \(:nesmppi\)", open(os.path.join(ROOT, "include", "mpopis.h")).read())


def test_nes_create_argument_checks_then_no_device(L):
    from mpopis_amd._lib import Config
    cfg = Config()
    cfg.env_kind, cfg.num_cars, cfg.policy = 1, 1, 8
    cfg.num_samples, cfg.horizon, cfg.batch, cfg.ais_its = 8, 4, 1, 3
    cfg.lambda_, cfg.alpha, cfg.cma_sigma = 10.0, 1.0, 0.01
    h = C.c_void_p()
    cfg.num_samples = 1                                             # diff(cost) of one sample: the reference throws
    assert L.mpopis_create(C.byref(cfg), C.byref(h)) == -1 and h.value is None
    cfg.num_samples = 8
    cfg.cma_sigma = float("nan")
    assert L.mpopis_create(C.byref(cfg), C.byref(h)) == -1
    cfg.cma_sigma = 0.01
    cfg.num_cars, cfg.horizon = 3, 100                              # cs = 600
    assert L.mpopis_create(C.byref(cfg), C.byref(h)) == -1
    cfg.num_cars, cfg.horizon = 1, 4
    import torch
    rc = L.mpopis_create(C.byref(cfg), C.byref(h))
    if not torch.cuda.is_available():
        assert rc == -4 and h.value is None
        assert b"no HIP device" in L.mpopis_last_error(None)
    else:
        assert rc == 0, L.mpopis_last_error(None)
        L.mpopis_destroy(h)


def _gmppi(oracle, track, K, T, lam=10.0, alpha=1.0, cov=(0.0625, 0.1)):
    env = oracle.OracleEnv("car", 1, track=track)
    pol = oracle.OraclePolicy("gmppi", env, K, T, lam=lam, alpha=alpha, U0=[0.0, 0.0], cov=list(cov), N=1)
    return env, pol


@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_nes_ref_one_iteration_is_gmppi(oracle, track, alpha):
    """opt_its = 1: no update runs, so the NES call is the :gmppi call (same E = chol(Σ) Z, same tail and roll)."""
    K, T, lam = 64, 12, 10.0
    rng = np.random.default_rng(5)
    envA, polA = _gmppi(oracle, track, K, T, lam, alpha)
    envB, polB = _gmppi(oracle, track, K, T, lam, alpha)
    for pol in (polA, polB):
        pol.U = 0.1 * np.sin(np.arange(pol.cs))
    for step in range(2):
        Z = rng.standard_normal((1, K, polA.cs))
        ref = polA(envA, Z)
        got = nes_ref(polB, envB, Z, 1, 0.01, lam, gamma=lam * (1 - alpha))
        assert ref["status"] == 0 and got["iters_run"] == 1
        for key in ("control", "cost", "weights"):
            assert np.max(np.abs(got[key] - ref[key]) / (np.abs(ref[key]) + 1.0)) < 1e-12, key
        assert np.max(np.abs(got["E"] - ref["E"])) < 1e-12
        assert np.max(np.abs(polB.U - polA.U)) < 1e-12


def test_nes_closed_form_equals_score_function_sum():
    """Σ_k c_k (∇Σ_k + ∇Σ_k') with ∇Σ_k = ½ Σ^-1 E_k E_k' Σ^-1 - ½ Σ^-1 (:872-874) and Σ_k c_k Σ^-1 E_k (:871), summed sample by sample."""
    rng = np.random.default_rng(11)
    for cs, K in ((6, 40), (17, 9)):
        X = rng.standard_normal((cs, cs))
        S = X @ X.T + cs * np.eye(cs)
        Sinv = inv_from_chol(np.linalg.cholesky(S))
        E = rng.standard_normal((cs, K))
        c = rng.standard_normal(K) * 30.0 - 5.0                   # either sign
        G, Sg = nes_gradients(E, c, Sinv)
        Gs = np.zeros((cs, cs)); gs = np.zeros(cs)
        for k in range(K):
            e = E[:, k:k + 1]
            dS = 0.5 * Sinv @ e @ e.T @ Sinv - 0.5 * Sinv
            Gs += (dS + dS.T) * c[k]
            gs += (Sinv @ e)[:, 0] * c[k]
        scale = np.max(np.abs(Gs))
        assert np.max(np.abs(G - Gs)) / scale < 1e-12
        assert np.max(np.abs(Sg - gs)) / np.max(np.abs(gs)) < 1e-12
