"""The small closed-loop study of DESIGN.md section 18 (dev tool): C3 (1-car :cemppi, K = 150, H = 50, N = 10), 64 trials seeded 1 .. 64, 200 steps,
under each noise kind -- reward per step and the first lap time with their quantile_ci.  Prints one JSON line per kind.
usage: python tools/noise_kind_study.py [num_trials] [num_steps]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mpopis_amd.examples import simulate_car_racing, quantile_ci


def main():
    trials = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    for kind in ("philox", "antithetic", "lhs"):
        rec, _ = simulate_car_racing(num_trials=trials, num_steps=steps, policy_type="cemppi", num_samples=150, horizon=50, ais_its=10, seed=0,
                                     quiet=True, noise=kind)
        rps, lap = rec[:, 3], rec[:, 4]                            # (column 0 is the trial id: reward per step, lap 1)
        done = lap[lap > 0]
        out = dict(kind=kind, trials=trials, steps=steps, reward_per_step=[round(float(v), 3) for v in quantile_ci(rps)],
                   reward_per_step_mean=round(float(rps.mean()), 3), laps_finished=int(done.size),
                   lap1_time=[round(float(v), 2) for v in quantile_ci(done)] if done.size else None, status_bad=int(np.sum(rec[:, 16] != 0)))
        print(json.dumps(out))


if __name__ == "__main__":
    main()
