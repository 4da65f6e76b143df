"""CPU-side checks of the 5..8-car limits: create's argument validation (before it looks for a device), the header constant and the
Python env's bound.  Without a GPU, arguments that pass validation end in MPOPIS_ERR_HIP "no HIP device"."""
import ctypes as C
import os
import re
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from mpopis_amd import build, _lib
    build.build()
    return _lib.lib()


def _create(L, ncars, policy, horizon, K=8):
    from mpopis_amd._lib import Config
    cfg = Config()
    cfg.env_kind, cfg.num_cars, cfg.policy = 1, ncars, policy
    cfg.num_samples, cfg.horizon, cfg.batch, cfg.ais_its = K, horizon, 1, 2
    cfg.lambda_, cfg.alpha, cfg.lambda_ais, cfg.elite_threshold, cfg.cma_sigma = 10.0, 1.0, 20.0, 0.8, 0.75
    h = C.c_void_p()
    rc = L.mpopis_create(C.byref(cfg), C.byref(h))
    msg = L.mpopis_last_error(None)
    if rc == 0:
        L.mpopis_destroy(h)
    return rc, msg


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_header_defines_max_cars():
    hdr = open(os.path.join(ROOT, "include", "mpopis.h")).read()
    assert re.search(r"^#define MPOPIS_MAX_CARS 8\b", hdr, re.MULTILINE)


@pytest.mark.parametrize("ncars", [5, 6, 7, 8])
def test_five_to_eight_cars_pass_validation(L, ncars):
    from mpopis_amd import _lib
    for pol in ("gmppi", "musigmaaismppi", "cemppi", "pmcmppi", "cmamppi", "nesmppi"):
        rc, msg = _create(L, ncars, _lib.POLICY_IDS[pol], 20)
        if _has_gpu():
            assert rc == 0, (pol, msg)
        else:
            assert rc == -4 and b"no HIP device" in msg, (pol, rc, msg)


def test_nine_cars_refused(L):
    rc, msg = _create(L, 9, 1, 10)
    assert rc == -1 and b"num_cars must be 1..8" in msg


@pytest.mark.parametrize("pol,ncars,horizon", [("cemppi", 8, 51), ("musigmaaismppi", 8, 64), ("pmcmppi", 7, 58), ("cemppi", 4, 101)])
def test_scatter_policies_refuse_cs_above_800(L, pol, ncars, horizon):
    """cs = 2 N H beyond the covariance scatter's 800 rows: refused, with the bound in the message (also for <= 4 cars, which used to give a wrong Σ′)"""
    from mpopis_amd import _lib
    assert 2 * ncars * horizon > 800
    rc, msg = _create(L, ncars, _lib.POLICY_IDS[pol], horizon)
    assert rc == -1 and b"cs <= 800" in msg, msg
    rc, msg = _create(L, ncars, _lib.POLICY_IDS[pol], 800 // (2 * ncars))
    assert rc == (0 if _has_gpu() else -4), msg


@pytest.mark.parametrize("pol,horizon,bound", [("cmamppi", 45, b"cmamppi: control space too large"), ("nesmppi", 33, b"cs <= 512")])
def test_existing_cs_bounds_hold_at_eight_cars(L, pol, horizon, bound):
    from mpopis_amd import _lib
    rc, msg = _create(L, 8, _lib.POLICY_IDS[pol], horizon)       # cs 720 > 710 / cs 528 > 512
    assert rc == -1 and bound in msg, msg


def test_python_env_bound():
    from mpopis_amd import envs
    from mpopis_amd._lib import MPOPISError, ERR_ARG
    assert envs.MAX_CARS == 8
    with pytest.raises(MPOPISError) as ei:
        envs.MultiCarRacingEnv(9)
    assert ei.value.code == ERR_ARG
    with pytest.raises(MPOPISError):
        envs.MultiCarRacingEnv(0)
