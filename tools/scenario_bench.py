"""What scenario rollouts cost: the C5 shape (:μΣaismppi, K = 4096, T = 50, N = 10, one car) at 64 trial slots and at one,
with M = 1, 2, 4, 8 scenarios against the SAME handle without scenarios, in one process.

Per (slots, M): ms per MPC step on the default schedule (mpopis_bench_policy_steps: median, min and max of REPEATS regions of STEPS steps after a
warm-up region), the rollout class's time per step on one stream (mpopis_set_overlap(h, 1) + mpopis_timing_read: the events bracket the M rollout
launches and the risk kernel of every rollout), and the model step(M) = step(0) + (M - 1) x rollout(0) with the measured deviation from it.
The risk kernel's own time comes from tools/kbench_risk_bin on planes of the same size (events around 200 launches).
usage (GPU box): python tools/scenario_bench.py [slots,slots] [M,M,...]        prints one line per measurement and one JSON line at the end"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                    # noqa: E402
from mpopis_amd.engine import Engine                  # noqa: E402
from tests.helpers import harness_io as IO            # noqa: E402

K, T, N = 4096, 50, 10
STEPS, REPEATS = 10, 5


def models(M):
    """M car models around the defaults: mass -20 .. +20 %, tyre friction down to 0.7"""
    from mpopis_amd.envs import CarRacingEnvParams
    p = np.tile(CarRacingEnvParams().vector(0.1, 0.01), (M, 1))
    for m in range(M):
        f = m / max(M - 1, 1)
        p[m, 0] *= 0.8 + 0.4 * f
        p[m, 9] *= 1.0 - 0.3 * f
        p[m, 10] *= 1.0 - 0.3 * f
    return p


def step_ms(eng):
    eng.bench_policy_steps(STEPS)
    r = sorted(eng.bench_policy_steps(STEPS)[0] / STEPS for _ in range(REPEATS))
    return dict(median=r[len(r) // 2], min=r[0], max=r[-1])


def rollout_class_ms(eng):
    """the rollout class per MPC step with every launch alone on the chip (one stream)"""
    eng.set_overlap(1)
    eng.bench_policy_steps(2)
    eng.timing_enable(2); eng.timing_reset()
    eng.bench_policy_steps(STEPS)
    ms, launches = eng.timing_read()["rollout"]
    eng.timing_enable(False)
    one = eng.bench_policy_steps(STEPS)[0] / STEPS
    eng.set_overlap(0)
    return dict(per_step=ms / STEPS, brackets_per_step=launches / STEPS, step_one_stream=one)


def risk_kernel_us(B, M, exe):
    """launch_risk alone on [M][B][K] planes (mean; cmin and status given, as the C5 handle passes them)"""
    rng = np.random.default_rng(1)
    c = rng.uniform(0.0, 500.0, (M, B, K))
    data = IO.pack_case(b"RSKCASE1", 0, B, [M, B, 0, K, 0, M, 1, 1], [0.0],
                        [(IO.I32, np.ones(B, dtype=np.int32)), (IO.F64, c), (IO.U64, np.full(B, 2 ** 64 - 1, dtype=np.uint64)), (IO.I32, np.zeros(B, dtype=np.int32))])
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "case.bin"), os.path.join(d, "result.bin")
        with open(fin, "wb") as f:
            f.write(data)
        r = subprocess.run([exe, fin, fout, "200"], capture_output=True, text=True, timeout=120)
    if r.returncode != 0:
        raise RuntimeError("kbench_risk_bin failed (%d): %s" % (r.returncode, r.stdout + r.stderr))
    return float([ln for ln in r.stdout.splitlines() if ln.startswith("TIME_US")][0].split()[1])


def main():
    slots = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "64,1").split(",")]
    Ms = [int(v) for v in (sys.argv[2] if len(sys.argv) > 2 else "1,2,4,8").split(",")]
    exe = os.path.join(ROOT, "tools", "kbench_risk_bin")
    out = []
    for B in slots:
        eng = Engine("car", 1, "musigmaaismppi", K, T, batch=B, lam=10.0, ais_its=N, lam_ais=20.0, cov=[0.0625, 0.1], seed=20240000)
        base = step_ms(eng)
        base_roll = rollout_class_ms(eng)
        again = step_ms(eng)                          # the same measurement once more: the run-to-run spread of the baseline itself
        print("slots %2d M 0: step %.3f ms (min %.3f max %.3f; repeated: %.3f), rollout class %.3f ms/step on one stream (step there %.3f)"
              % (B, base["median"], base["min"], base["max"], again["median"], base_roll["per_step"], base_roll["step_one_stream"]), flush=True)
        out.append(dict(slots=B, M=0, step_ms=base, step_ms_repeat=again, rollout=base_roll))
        for M in Ms:
            eng.set_scenarios(models(M))
            st = step_ms(eng)
            ro = rollout_class_ms(eng)
            us = risk_kernel_us(B, M, exe) if os.path.exists(exe) else None
            model = base_roll["step_one_stream"] + (M - 1) * base_roll["per_step"]
            dev = ro["step_one_stream"] / model - 1.0
            print("slots %2d M %d: step %.3f ms (min %.3f max %.3f), one stream %.3f ms vs step(0) + (M - 1) rollout(0) = %.3f ms (%+.1f %%), "
                  "rollout class %.3f ms/step, risk kernel %s us/launch"
                  % (B, M, st["median"], st["min"], st["max"], ro["step_one_stream"], model, 100 * dev, ro["per_step"], "n/a" if us is None else "%.1f" % us), flush=True)
            out.append(dict(slots=B, M=M, step_ms=st, rollout=ro, model_one_stream_ms=model, deviation=dev, risk_kernel_us=us))
        eng.set_scenarios(None)
        back = step_ms(eng)
        print("slots %2d M 0 again: step %.3f ms" % (B, back["median"]), flush=True)
        out.append(dict(slots=B, M=0, after=True, step_ms=back))
        eng.close()
    print(json.dumps(dict(shape=dict(policy="musigmaaismppi", K=K, T=T, N=N, cars=1), steps=STEPS, repeats=REPEATS, results=out)))


if __name__ == "__main__":
    main()
