"""Helper process for tests/test_gpu_many_cars.py: 5- and 8-car handles in the few-waves regime (one- or two-wave rollout kernel, by
MPOPIS_ROLLOUT_DUO, read once per process), a few policy steps each, on the default track and on a 960-point track whose tables do not fit
LDS; prints one JSON line with the controls, costs and weights as hex (bit patterns)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from mpopis_amd.engine import Engine

out = {}
for name, pol, K, B, track, ncars in (("cars5", "musigmaaismppi", 250, 2, None, 5), ("cars8", "gmppi", 333, 1, None, 8),
                                     ("cars5_big", "imppi", 200, 2, 960, 5), ("cars8_big", "cemppi", 150, 2, 960, 8)):
    eng = Engine("car", ncars, pol, K, 20, batch=B, lam=10.0, ais_its=3, cov=np.tile([0.0625, 0.1], ncars), seed=4343)
    if track:
        th = np.linspace(0, 2 * np.pi, track, endpoint=False)
        r = 40.0 + 6.0 * np.sin(3 * th)
        mid = np.stack([r * np.cos(th), r * np.sin(th)], 1)
        eng.set_track(mid[:, 0], mid[:, 1], np.full(track, 8.0))
        x0 = np.zeros((B, 8 * ncars))
        for c in range(ncars):
            p = mid[(3 * c) % track]
            x0[:, 8 * c:8 * c + 4] = [p[0], p[1], np.pi / 2, 5.0]
        eng.set_state(x0)
    rec = []
    for _ in range(3):
        got = eng.policy_step(None)
        rec.append(got["control"].tobytes().hex() + got["cost"].tobytes().hex() + got["weights"].tobytes().hex())
    out[name] = rec
    eng.close()
print(json.dumps(out))
