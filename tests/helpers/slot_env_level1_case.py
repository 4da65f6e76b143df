"""Helper process for tests/test_gpu_slot_env.py: the Level-1 cases of a per-slot-env handle (test_level1_per_slot, test_mixed_track_sizes) against the
oracle, for a run under MPOPIS_ROLLOUT_DUO=0 -- the library reads that variable once per process, hence the subprocess.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mpopis_amd.engine import Engine
from oracle import oracle as O
from tests.helpers import slot_env_cases as SC

O.build()
tracks, params = SC.tracks3(O.load_track()), SC.car_params4(O)
worst, cases = 0.0, 0
for nc in (1, 3, 8):
    S = 64 // nc
    for T in (1, 5):
        for K in (S - 1, S, S + 1, 1024 + S + 1):
            worst = max(worst, SC.level1_check(Engine, O, tracks, SC.TRACK_OF_SLOT, params, nc, K, T, seed=1000 * nc + K))
            cases += 1
for sizes in ((5, 190, 191), (2, 2048)):
    for nc in (1, 3):
        worst = max(worst, SC.level1_check(Engine, O, SC.mixed_tracks(sizes), list(range(len(sizes))), params[:len(sizes)], nc, 64 // nc + 1, 3, seed=5 + nc))
        cases += 1
print(json.dumps({"cases": cases, "worst": worst}))
