""":nesmppi step time against the :μΣaismppi step at the C5 shape (1 car, K = 4096, H = 50, N = 10, 64 trials, device RNG, the default
schedule; step_factor 1e-7, with which every slot runs all ten iterations) through mpopis_bench_policy_steps, plus the per-class kernel time of each (HIP events, one-stream pass).  Each policy is measured in
a child process of its own under `timeout`, and a failing child ends the run.
usage: python tools/nes_step_bench.py [--trials 64] [--steps 20]          (one policy: --one nesmppi)"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(policy, trials, steps):
    from mpopis_amd.engine import Engine
    eng = Engine("car", 1, policy, 4096, 50, batch=trials, lam=10.0, ais_its=10, lam_ais=20.0, step_factor=1e-7, cov=[0.0625, 0.1], seed=20240000)
    eng.bench_policy_steps(steps)                                    # warm-up (code objects, stream check)
    runs = sorted(eng.bench_policy_steps(steps)[0] / steps for _ in range(5))
    eng.set_overlap(1)
    eng.timing_enable(True); eng.timing_reset()
    eng.bench_policy_steps(10)
    tm = eng.timing_read()
    eng.timing_enable(False)
    eng.close()
    print(json.dumps(dict(policy=policy, trials=trials, ms_per_step=runs[2], ms_runs=runs,
                          classes_ms_per_step={k: v[0] / 10 for k, v in tm.items() if v[1]})))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--trials", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.trials, a.steps)
        return
    res = {}
    for pol in ("musigmaaismppi", "nesmppi"):
        p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), "--one", pol, "--trials", str(a.trials),
                            "--steps", str(a.steps)], capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit("%s: child exited with %d" % (pol, p.returncode))
        res[pol] = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps(res[pol]))
    print(json.dumps(dict(nes_over_musigma=res["nesmppi"]["ms_per_step"] / res["musigmaaismppi"]["ms_per_step"])))


if __name__ == "__main__":
    main()
