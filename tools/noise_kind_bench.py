"""One noise kind at one shape, in a process of its own (dev tool): the whole step from mpopis_bench_policy_steps and the time
per launch of the "sample" class from mpopis_timing_read.  Prints one JSON line.  Run the kinds alternately, each several times, and read the spread.
usage: python tools/noise_kind_bench.py <philox|antithetic|lhs> <c5|c3> <batch> [steps]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpopis_amd.engine import Engine

SHAPES = {"c5": ("musigmaaismppi", 4096), "c3": ("cemppi", 150)}


def main():
    kind, shape, B = sys.argv[1], sys.argv[2], int(sys.argv[3])
    steps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
    policy, K = SHAPES[shape]
    eng = Engine("car", 1, policy, K, 50, batch=B, lam=10.0, ais_its=10, lam_ais=20.0, elite_threshold=0.8, cov=[0.0625, 0.1], seed=20240000)
    eng.set_noise_kind(kind)
    eng.bench_policy_steps(steps)                                   # warm-up: code objects, the stream check of the part chains
    runs = sorted(eng.bench_policy_steps(steps)[0] / steps for _ in range(5))
    eng.timing_enable(True); eng.timing_reset()
    eng.bench_policy_steps(steps)
    ms, n = eng.timing_read()["sample"]
    eng.timing_enable(False)
    print(json.dumps(dict(kind=kind, shape=shape, batch=B, K=K, ms_per_step_median=round(runs[2], 4), ms_per_step_min=round(runs[0], 4),
                          ms_per_step_max=round(runs[4], 4), sample_us_per_launch=round(1e3 * ms / max(n, 1), 2), sample_launches_per_step=n // steps)))
    eng.close()


if __name__ == "__main__":
    main()
