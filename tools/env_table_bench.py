"""Rollout-kernel time of custom envs with and without a data table (include/mpopis_env.h), K = 4096, T = 50, 64 trials, :gmppi, device noise:
  cartpole       mpopis_env_rollout       SDK CartPole, parameters in p (one wave per workgroup)          } the cost of the table kernel's shape:
  cartpole_tab   mpopis_env_rollout_tab   the same env, parameters in an 11-double table staged in LDS     } four-wave workgroups, one barrier
  mapnav_lds     mpopis_env_rollout_tab   waypoint-and-map env, a 64 x 64 map = 4096 doubles staged in LDS } what staging buys against reading
  mapnav_global  mpopis_env_rollout_gtab  the same table padded by one double: read from global memory     } the table from global memory
Kernel times come from `rocprofv3 --kernel-trace --stats`, each variant in a child process of its own under `timeout` (a failing child ends
the run), the variants alternating over --rounds rounds; one JSON line per run and a summary (mean and max - min per variant) at the end.
usage: python tools/env_table_bench.py [--rounds 3] [--steps 50] [--out bench_outputs/env_table_bench]       (one variant, no profiler: --one NAME)"""
import argparse
import csv
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENVS = os.path.join(ROOT, "tests", "helpers", "envs")
KERNEL = {"cartpole": "mpopis_env_rollout", "cartpole_tab": "mpopis_env_rollout_tab", "mapnav_lds": "mpopis_env_rollout_tab",
          "mapnav_global": "mpopis_env_rollout_gtab"}
CARTPOLE = [9.8, 1.0, 0.1, 1.1, 0.5, 0.05, 10.0, 0.02, 0.20943951023931953, 2.4, 200.0]      # the built-in CartPole's defaults (mpopis.h order)


def one(variant, steps, B=64, K=4096, T=50):
    import numpy as np
    from mpopis_amd import build
    from mpopis_amd.engine import Engine
    from tests.helpers import mapnav_ref as MN

    def desc(name, ss, as_, params, table=None, lo=None, hi=None):
        return types.SimpleNamespace(code_object=build.build_env(os.path.join(ENVS, name + ".hip")), state_size=ss, action_size=as_,
                                     params=np.array(params, dtype=np.float64), lo=lo, hi=hi, reset_state=None, table=table)
    rng = np.random.default_rng(1)
    if variant == "cartpole":
        env, cov, x0 = desc("cartpole_sdk", 4, 1, CARTPOLE), [1.5], rng.uniform(-0.05, 0.05, (B, 4))
    elif variant == "cartpole_tab":
        env, cov, x0 = desc("cartpole_tab_sdk", 4, 1, [], table=np.array(CARTPOLE)), [1.5], rng.uniform(-0.05, 0.05, (B, 4))
    else:
        tab = MN.make_table(0, 64, rng, pad=int(variant == "mapnav_global"))
        env, cov = desc("mapnav_sdk", MN.SS, MN.AS, MN.params(0, 64), table=tab, lo=MN.LO, hi=MN.HI), [0.3, 0.3]
        x0 = np.concatenate([rng.uniform(-0.8, 0.8, (B, 2)), rng.uniform(-0.3, 0.3, (B, 2))], axis=1)
    eng = Engine("custom", 0, "gmppi", K, T, batch=B, lam=0.1, cov=cov, seed=7, custom_env=env)
    eng.set_overlap(1)
    eng.set_state(x0)
    first = eng.policy_step()                                       # warm-up; its cost sum identifies the work
    eng.timing_enable(2); eng.timing_reset()                        # the "rollout" class by HIP events as a second opinion
    eng.bench_policy_steps(steps)
    ms, n = eng.timing_read()["rollout"]
    eng.close()
    print(json.dumps(dict(variant=variant, cost_sum=float(first["cost"].sum()), event_us_per_launch=1e3 * ms / max(n, 1), launches=n)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "env_table_bench"))
    a = ap.parse_args()
    if a.one:
        one(a.one, a.steps)
        return
    os.makedirs(a.out, exist_ok=True)
    runs = {v: [] for v in KERNEL}
    for r in range(a.rounds):
        for v in KERNEL:
            d = os.path.join(a.out, "%s_%d" % (v, r))
            p = subprocess.run(["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "p", "--",
                                sys.executable, os.path.abspath(__file__), "--one", v, "--steps", str(a.steps)], capture_output=True, text=True)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit("%s: child exited with %d" % (v, p.returncode))
            child = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            stats = [os.path.join(dp, f) for dp, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
            row = [x for x in csv.DictReader(open(stats[0])) if x["Name"].split("(")[0].strip() == KERNEL[v]]
            if len(row) != 1:
                sys.exit("%s: kernel %s not found once in %s" % (v, KERNEL[v], stats[0]))
            rec = dict(child, round=r, kernel=KERNEL[v], calls=int(row[0]["Calls"]), avg_us=float(row[0]["AverageNs"]) / 1e3,
                       min_us=float(row[0]["MinNs"]) / 1e3, max_us=float(row[0]["MaxNs"]) / 1e3)
            runs[v].append(rec)
            print(json.dumps(rec), flush=True)
    summary = {v: dict(kernel=KERNEL[v], avg_us=[round(x["avg_us"], 2) for x in rs], mean_us=round(sum(x["avg_us"] for x in rs) / len(rs), 2),
                       spread_us=round(max(x["avg_us"] for x in rs) - min(x["avg_us"] for x in rs), 2)) for v, rs in runs.items()}
    print(json.dumps(dict(summary=summary)))
    with open(os.path.join(a.out, "summary.json"), "w") as f:
        json.dump(dict(runs=runs, summary=summary), f, indent=1)


if __name__ == "__main__":
    main()
