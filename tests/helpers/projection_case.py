"""Helper process for tests/test_gpu_rollout_projection.py: mpopis_rollout_costs for the inputs in an .npz file (track, ncars, x0, U, E); writes the
costs to a second .npz.  MPOPIS_ROLLOUT_DUO is read once per process by the library, hence the subprocess.
usage: projection_case.py <in.npz> <out.npz>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from mpopis_amd.engine import Engine

d = np.load(sys.argv[1])
ncars, (B, K, cs) = int(d["ncars"]), d["E"].shape
T = cs // (2 * ncars)
eng = Engine("car", ncars, "gmppi", K, T, batch=B, lam=10.0, cov=np.tile([0.0625, 0.1], ncars), track=(d["tx"], d["ty"], d["tw"]))
cost = eng.rollout_costs(d["U"], d["E"], x0=d["x0"])
eng.close()
np.savez(sys.argv[2], cost=cost)
