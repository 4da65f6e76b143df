"""simulate_car_racing / simulate_mountaincar (src/examples/car_example.jl:51-416,
mountaincar_example.jl:49-207): the trial loop runs as ONE device-resident batch per rank (all trials are
independent, car_example.jl:170), optionally sharded over ranks (trial k -> rank (k-1) mod G) with one RCCL
gather of the per-trial summary records (mpopis_gather_summary behind the C ABI when the process group is
nccl == RCCL; torch.distributed's own gather for the gloo CPU tests).  Prints the reference's tables."""
import math
import time
import warnings
import numpy as np

from .engine import Engine, default_track
from ._lib import MPOPISError, ERR_ARG, RECORD_LEN, noise_id
from .scenarios import parse_risk


def quantile_ci(x, p=0.05, q=0.5):
    """src/examples/example_utils.jl:2-10 (order-statistic CI of the median, normal approximation)."""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = len(x)
    zm, zp = -1.959963984540054, 1.959963984540054          # quantile(Normal(), p/2), p = 0.05
    if p != 0.05:
        from statistics import NormalDist
        zm, zp = NormalDist().inv_cdf(p / 2), NormalDist().inv_cdf(1 - p / 2)
    j = max(int(math.ceil(n * q + zm * math.sqrt(n * q * (1 - q)))), 1)
    k = min(int(math.ceil(n * q + zp * math.sqrt(n * q * (1 - q)))), n)
    return x[j - 1], float(np.quantile(x, q)), x[k - 1]


def _summary(rows):
    """AVE/STD/MED/L95/U95/MIN/MAX per column (car_example.jl:328-410)."""
    rows = np.asarray(rows, dtype=np.float64)
    out = {}
    out["AVE"] = rows.mean(0)
    out["STD"] = rows.std(0, ddof=1) if rows.shape[0] > 1 else np.full(rows.shape[1], np.nan)
    q = np.array([quantile_ci(rows[:, c]) for c in range(rows.shape[1])])
    out["MED"], out["L95"], out["U95"] = q[:, 1], q[:, 0], q[:, 2]
    out["MIN"], out["MAX"] = rows.min(0), rows.max(0)
    return out


def _gather_records(rec, dist):
    """One collective for summary stats only: RCCL gather to rank 0."""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return rec
    import torch
    dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    # ranks may hold different numbers of trials: pad to the maximum (row id 0 marks padding)
    n = torch.tensor([rec.shape[0]], device=dev)
    dist.all_reduce(n, op=dist.ReduceOp.MAX)
    nmax, width = int(n.item()), rec.shape[1]
    pad = np.zeros((nmax, width))
    pad[:rec.shape[0]] = rec
    t = torch.from_numpy(pad).to(dev)
    gl = [torch.zeros_like(t) for _ in range(dist.get_world_size())] if dist.get_rank() == 0 else None
    dist.gather(t, gl, dst=0)
    if dist.get_rank() != 0:
        return None
    out = np.concatenate([g.cpu().numpy() for g in gl], axis=0)
    return out[out[:, 0] > 0]


def assemble_gathered(parts, world):
    """Rows of the summary table from what mpopis_gather_summary hands rank 0: parts[g] = (n_g, RECORD_LEN) records of rank g's
    trials in slot order, i.e. of trials g+1, g+1+world, ... (shard_trials).  Column layout of the result: [trial id, record[0:15],
    0, Ex Time] -- the sending rank stored its wall time in record slot 15 (the status slot, unused after a successful run)."""
    rows = []
    for g, part in enumerate(parts):
        for i, row in enumerate(np.asarray(part, dtype=np.float64).reshape(-1, RECORD_LEN)):
            rows.append(np.concatenate([[1 + g + i * world], row[:15], [0.0], [row[15]]]))
    return np.array(rows).reshape(-1, RECORD_LEN + 2)


def shard_trials(num_trials, rank, world):
    """trial k (1-based) -> rank (k-1) mod world; returns this rank's 1-based trial ids."""
    return [k for k in range(1, num_trials + 1) if (k - 1) % world == rank]


def split_per_trial(value, num_trials, rank=0, world=1, cov=False):
    """What one rank passes for a keyword that may be given per trial.  Returns (shared, per_slot), one of them None:
    a scalar (cov: a vector = one diagonal, or a square matrix) keeps its meaning and comes back as `shared`; a sequence of length num_trials
    (cov: num_trials vectors or matrices; an array that is square in 2-D is ONE matrix, so pass (num_trials, n, n) when num_trials == n) gives
    trial k (1-based) entry k - 1, and `per_slot` holds the entries of this rank's trials (shard_trials) in slot order.
    A scalar keyword takes a scalar or a 1-D sequence and nothing else.  A square 2-D cov with num_trials rows that is not symmetric cannot be
    one covariance matrix and was most likely meant as per-trial diagonals: it is still read as one matrix, as before, with a warning."""
    a = np.asarray(value, dtype=np.float64)
    shared_ndim = 1 if cov else 0
    if not cov and a.ndim > 1:
        raise ValueError("a per-trial value is a scalar or one value per trial (%d), got shape %s" % (num_trials, a.shape))
    if a.ndim <= shared_ndim or (cov and a.ndim == 2 and a.shape[0] == a.shape[1]):
        if cov and a.ndim == 2 and a.shape[0] == num_trials and num_trials > 1 and not np.array_equal(a, a.T):
            warnings.warn("cov_mat of shape %s is read as ONE matrix for all %d trials although it is not symmetric; per-trial diagonals of this "
                          "size go as shape (%d, %d, %d)" % (a.shape, num_trials, num_trials, a.shape[1], a.shape[1]), stacklevel=3)
        return value, None
    if a.ndim > shared_ndim + 2 or a.shape[0] != num_trials:
        raise ValueError("a per-trial value needs one entry per trial (%d), got shape %s" % (num_trials, a.shape))
    return None, a[[k - 1 for k in shard_trials(num_trials, rank, world)]]


def _is_track_triple(t):
    """(x, y, w): three 1-D coordinate arrays of one length (at least 2 points)."""
    if isinstance(t, str) or not hasattr(t, "__len__") or len(t) != 3 or any(isinstance(v, str) for v in t):
        return False
    try:
        arrs = [np.asarray(v, dtype=np.float64) for v in t]
    except (TypeError, ValueError):
        return False
    return all(a.ndim == 1 for a in arrs) and arrs[0].size == arrs[1].size == arrs[2].size >= 2


def split_tracks_per_trial(track, num_trials, rank=0, world=1):
    """What one rank passes for the `track` keyword.  Returns (shared, per_slot), one of them None: a bundled name or one (x, y, w) triple
    comes back as `shared`; a sequence of num_trials names or triples gives trial k (1-based) entry k - 1, and `per_slot` is
    (tracks, track_of_slot) for Engine.set_tracks -- the distinct entries among this rank's trials (shard_trials) in order of first use, equal
    entries (the same name, or triples with the same numbers) once, and for every slot of the rank the index of its track."""
    if isinstance(track, str) or _is_track_triple(track):
        return track, None
    if not hasattr(track, "__len__") or len(track) != num_trials or not all(isinstance(t, str) or _is_track_triple(t) for t in track):
        raise ValueError("track: a bundled name, one (x, y, w) triple of equal-length 1-D arrays, or a sequence of one of either per trial (%d)" % num_trials)
    tracks, index, track_of_slot = [], {}, []
    for k in shard_trials(num_trials, rank, world):
        t = track[k - 1]
        key = ("name", t) if isinstance(t, str) else ("xyw",) + tuple(np.asarray(v, dtype=np.float64).tobytes() for v in t)
        if key not in index:
            index[key] = len(tracks)
            tracks.append(t)
        track_of_slot.append(index[key])
    return None, (tracks, track_of_slot)


def split_env_params_per_trial(value, n, num_trials, rank=0, world=1):
    """What one rank passes for `car_params` / `env_params`.  Returns (shared, per_slot), one of them None (both for value None = the env's
    defaults): a vector of n values (include/mpopis.h lists them per env kind) is `shared`; an array of shape (num_trials, n) gives trial k
    (1-based) row k - 1, and `per_slot` holds the rows of this rank's trials (shard_trials) in slot order, for Engine.set_env_params_slots."""
    if value is None:
        return None, None
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 1 and a.size == n:
        return a, None
    if a.ndim != 2 or a.shape != (num_trials, n):
        raise ValueError("env parameters: %d values, or one row of %d per trial (%d), got shape %s" % (n, n, num_trials, a.shape))
    return None, a[[k - 1 for k in shard_trials(num_trials, rank, world)]]


def split_model_params_per_trial(value, n, num_trials, rank=0, world=1):
    """What one rank passes for `model_params` to Engine.set_scenarios, as (params, per_slot) (None, False: no scenarios): (M, n) as it is -- every
    trial plans against those M models --, or from (num_trials, M, n) the blocks of this rank's trials (shard_trials) in slot order."""
    if value is None:
        return None, False
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 2 and a.shape[1] == n and a.shape[0] >= 1:
        return a, False
    if a.ndim != 3 or a.shape[0] != num_trials or a.shape[2] != n or a.shape[1] < 1:
        raise ValueError("model_params: shape (M, %d), or one block per trial (%d, M, %d), got %s" % (n, num_trials, n, a.shape))
    return a[[k - 1 for k in shard_trials(num_trials, rank, world)]], True


def _apply_scenarios(eng, model, per_slot, risk):
    """Engine.set_scenarios / set_risk from split_model_params_per_trial and the harness's risk= keyword."""
    if model is None:
        return
    eng.set_scenarios(model, per_slot=per_slot)
    kind, tail, theta = parse_risk(risk)
    eng.set_risk(kind, tail=tail, theta=theta)


def split_fleet_per_trial(value, num_cars, num_trials, rank=0, world=1):
    """What one rank passes for `car_fleet` to Engine.set_env_params_cars (None: no fleet): (num_cars, 20) as it is -- every trial drives that
    fleet --, or from (num_trials, num_cars, 20) the fleets of this rank's trials (shard_trials) in slot order."""
    if value is None:
        return None
    a = np.asarray(value, dtype=np.float64)
    if a.shape == (num_cars, 20):
        return a
    if a.shape != (num_trials, num_cars, 20):
        raise ValueError("car_fleet: shape (num_cars, 20) = (%d, 20), or one fleet per trial (%d, %d, 20), got %s" % (num_cars, num_trials, num_cars, a.shape))
    return a[[k - 1 for k in shard_trials(num_trials, rank, world)]]


def _resolve_track(t):
    return default_track(name=t) if isinstance(t, str) else tuple(np.asarray(v, dtype=np.float64) for v in t)


def _apply_per_trial(eng, per, cov_slots, policy):
    """Engine.set_slot_hyper / set_Sigma_slots from the per_slot halves of split_per_trial (None: that keyword is shared)."""
    if any(v is not None for v in per.values()):
        eng.set_slot_hyper(lam=per["λ"], alpha=per["α"], lam_ais=per["λ_ais"],
                           **{"step_factor" if policy == "nesmppi" else "cma_sigma": per["cma_σ"]})
    if cov_slots is not None:
        eng.set_Sigma_slots(cov_slots)


def simulate_car_racing(num_trials=1, num_steps=200, num_cars=1, policy_type="cemppi", laps=2, num_samples=150, horizon=50,
                        λ=10.0, α=1.0, U0=None, cov_mat=None, ais_its=10, λ_ais=20.0, ce_elite_threshold=0.8, ce_Σ_est="ss",
                        cma_σ=0.75, cma_elite_threshold=0.8, state_x_sigma=0.0, state_y_sigma=0.0, state_ψ_sigma=0.0,
                        seed=None, log_runs=True, device=0, dist=None, quiet=False, track="curve", car_params=None, trace=None, car_fleet=None, noise="philox", model_params=None,
                        risk="mean"):
    """Returns (records, summary) on rank 0 (None elsewhere).  Differences from the reference harness, all
    forced by the platform: plotting/GIF options are not offered (out of scope); the state noise (single car only,
    car_example.jl:224-236) is drawn from the trial's device stream instead of the env's MersenneTwister.
    λ, α, λ_ais and cma_σ also take a sequence of num_trials values, and cov_mat a sequence of num_trials vectors or matrices
    (split_per_trial): trial k runs with entry k - 1, all trials of a rank still in one resident batch -- a hyper-parameter sweep in one call.
    track: a bundled name (engine.BUNDLED_TRACKS) or an (x, y, w) triple, or a sequence of num_trials of either -- a policy over several tracks
    in one resident batch, every distinct track uploaded once (split_tracks_per_trial).  car_params: the 20 values of CarRacingEnvParams + dt, δt
    (include/mpopis.h), or (num_trials, 20) for one vector per trial (split_env_params_per_trial).  car_fleet (num_cars > 1): one such vector per
    CAR, (num_cars, 20) for every trial or (num_trials, num_cars, 20), sharded like car_params (split_fleet_per_trial); not together with car_params.
    ce_Σ_est defaults to :ss like the reference (car_example.jl:66); :mle is the other supported estimator.
    trace: as Engine.run_trials takes it (True, or dict(plan_every, top[, fields])) -- the run is recorded on the device, what plot_steps /
    save_gif / plot_traj of the reference draw, and the call returns (records, summary, trace) with the trace of THIS rank's trials in slot
    order (trial ids: shard_trials; traces are not gathered; an empty dict on a rank without trials).
    noise: how every trial draws its proposal's normals -- "philox" (default), "antithetic" or "lhs" (Engine.set_noise_kind); one kind per call.
    model_params: plan against M car models at once (Engine.set_scenarios) -- (M, 20) for every trial, or (num_trials, M, 20), sharded like
    car_params (split_model_params_per_trial) -- while the car that is driven keeps car_params; risk: how a sample's M costs become its cost,
    "mean", "worst", ("cvar", tail) or ("entropic", θ) (Engine.set_risk).  Not together with car_fleet."""
    pt = str(policy_type).lstrip(":")
    noise_id(noise)                                    # (an unknown kind is refused before the library is reached)
    parse_risk(risk)
    rank = dist.get_rank() if (dist is not None and dist.is_initialized()) else 0
    world = dist.get_world_size() if (dist is not None and dist.is_initialized()) else 1
    if seed is None:
        seed = int(np.random.default_rng().integers(1, 10 ** 10))
    U0 = np.zeros(num_cars * 2) if U0 is None else np.asarray(U0, dtype=np.float64)
    cov_mat = np.tile([0.0625, 0.1], num_cars) if cov_mat is None else cov_mat
    if world > 1:
        sd = [seed]                                    # the seed must be common to all ranks
        dist.broadcast_object_list(sd, src=0)
        seed = sd[0]
    mine = shard_trials(num_trials, rank, world)
    kw = {"λ": λ, "α": α, "λ_ais": λ_ais, "cma_σ": cma_σ}
    split = {k: split_per_trial(v, num_trials, rank, world) for k, v in kw.items()}
    # (the handle's own scalar of a per-trial keyword is never in force: trial 1's entry stands in for it at create)
    λ, α, λ_ais, cma_σ = [v if split[k][1] is None else float(np.asarray(v, dtype=np.float64)[0]) for k, v in kw.items()]
    cov_shared, cov_slots = split_per_trial(cov_mat, num_trials, rank, world, cov=True)
    trk_shared, trk_slots = split_tracks_per_trial(track, num_trials, rank, world)
    if car_params is not None and car_fleet is not None:
        raise ValueError("car_params and car_fleet: give one of the two (one vector per slot, or one per car)")
    par_shared, par_slots = split_env_params_per_trial(car_params, 20, num_trials, rank, world)
    fleet = split_fleet_per_trial(car_fleet, num_cars, num_trials, rank, world)
    if model_params is not None and car_fleet is not None:
        raise ValueError("model_params and car_fleet: scenarios give all cars of a slot one vector, a fleet one per car")
    model, model_per_slot = split_model_params_per_trial(model_params, 20, num_trials, rank, world)
    t0 = time.time()
    # every rank keeps a handle (even with no trials: it takes part in the collective); all of a rank's trials
    # k0, k0+G, ... live in ONE resident batch, slot i seeded like the reference's trial k_i: seed!(pol, seed + k) (:187-188)
    eng = Engine("car", num_cars, pt, num_samples, horizon, batch=max(len(mine), 1), lam=λ, alpha=α, ais_its=ais_its, lam_ais=λ_ais,
                 elite_threshold=(cma_elite_threshold if pt == "cmamppi" else ce_elite_threshold), sigma_est=str(ce_Σ_est).lstrip(":"),
                 cma_sigma=cma_σ, seed=seed, device=device, cov=cov_shared, U0=U0,
                 track=None if trk_shared is None else _resolve_track(trk_shared), env_params=par_shared)
    r = np.zeros((0, RECORD_LEN))
    tr_out = {}
    traced = (lambda *res: res + (tr_out,)) if not (trace is None or trace is False) else (lambda *res: res)
    if mine:
        _apply_per_trial(eng, {k: v[1] for k, v in split.items()}, cov_slots, pt)
        if trk_slots is not None:
            eng.set_tracks([_resolve_track(t) for t in trk_slots[0]], trk_slots[1])
        if par_slots is not None:
            eng.set_env_params_slots(par_slots)
        if fleet is not None:
            eng.set_env_params_cars(fleet)
        _apply_scenarios(eng, model, model_per_slot, risk)
        eng.seed_slots([seed + k for k in mine])
        if noise_id(noise) != 0:
            eng.set_noise_kind(noise)
        eng.set_state_noise(state_x_sigma, state_y_sigma, state_ψ_sigma)
        if trace is None or trace is False:
            r = eng.run_trials(num_steps, laps)
        else:
            r, tr_out = eng.run_trials(num_steps, laps, trace=trace)
    ex_time = time.time() - t0                 # Ex Time of this rank's batch (its trials run concurrently)
    n_max = (num_trials + world - 1) // world
    if world > 1 and dist.get_backend() == "nccl":
        # RCCL gather behind the C ABI (mpopis_gather_summary); slot 15 of a record (status) carries the rank's Ex Time
        r = r.copy()
        r[:, 15] = ex_time
        eng.comm_init_from_dist(dist)
        parts = eng.gather_summary(r, n_max)
        eng.close()
        if parts is None:
            return traced(None, None)
        allrec = assemble_gathered(parts, world)
    else:
        eng.close()
        rec = np.array([np.concatenate([[k], r[i], [ex_time]]) for i, k in enumerate(mine)]).reshape(-1, RECORD_LEN + 2)
        allrec = _gather_records(rec, dist)
    if allrec is None:
        return traced(None, None)
    allrec = allrec[np.argsort(allrec[:, 0])]
    cols = [1, 2, 3] + [4 + i for i in range(laps)] + [8, 9, 10, 11, 12, 13] + ([14] if num_cars > 1 else []) + [allrec.shape[1] - 1]
    table = allrec[:, cols]
    summ = _summary(table)
    if log_runs and not quiet:
        hdr = "Trial    #: %12s : %7s: %12s" % ("Reward", "Steps", "Reward/Step")
        hdr += "".join(" : %6s%d" % ("lap ", i + 1) for i in range(laps))
        hdr += " : %7s : %7s : %7s : %7s : %7s : %7s" % ("Mean V", "Max V", "Mean β", "Max β", "β Viol", "T Viol")
        hdr += (" : %7s" % "C Viol" if num_cars > 1 else "") + " : %7s" % "Ex Time"
        print(hdr)
        for row, full in zip(table, allrec):
            print("Trial %4d: " % int(full[0]) + " : ".join("%12.2f" % v if i in (0, 2) else "%7.2f" % v for i, v in enumerate(row)))
        print("-----------------------------------")
        for name in ("AVE", "STD", "MED", "L95", "U95", "MIN", "MAX"):
            print("Trials %3s: " % name + " : ".join("%12.2f" % v if i in (0, 2) else "%7.2f" % v for i, v in enumerate(summ[name])))
    return traced(allrec, summ)


def _simulate_simple(env_kind, ss, num_trials=1, num_steps=200, policy_type="cemppi", num_samples=20, horizon=15, λ=0.1, α=1.0, U0=(0.0,),
                         cov_mat=(1.5,), ais_its=5, λ_ais=0.1, ce_elite_threshold=0.8, ce_Σ_est="mle", cma_σ=0.75,
                         cma_elite_threshold=0.8, seed=None, x0=None, log_runs=True, device=0, quiet=False, env_params=None, trace=None, noise="philox",
                         model_params=None, risk="mean"):
    pt = str(policy_type).lstrip(":")
    noise_id(noise)                                    # (an unknown kind is refused before the library is reached)
    parse_risk(risk)
    model, model_per_slot = split_model_params_per_trial(model_params, 11 if env_kind == "cartpole" else 8, num_trials)
    par_shared, par_slots = split_env_params_per_trial(env_params, 11 if env_kind == "cartpole" else 8, num_trials)
    if seed is None:
        seed = int(np.random.default_rng().integers(1, 10 ** 10))
    kw = {"λ": λ, "α": α, "λ_ais": λ_ais, "cma_σ": cma_σ}
    split = {k: split_per_trial(v, num_trials) for k, v in kw.items()}              # per-trial values: see simulate_car_racing
    λ, α, λ_ais, cma_σ = [v if split[k][1] is None else float(np.asarray(v, dtype=np.float64)[0]) for k, v in kw.items()]
    cov_shared, cov_slots = split_per_trial(cov_mat, num_trials, cov=True)
    eng = Engine(env_kind, 0, pt, num_samples, horizon, batch=num_trials, lam=λ, alpha=α, ais_its=ais_its, lam_ais=λ_ais,
                 elite_threshold=(cma_elite_threshold if pt == "cmamppi" else ce_elite_threshold), sigma_est=str(ce_Σ_est).lstrip(":"),
                 cma_sigma=cma_σ, seed=seed, device=device, cov=None if cov_shared is None else np.asarray(cov_shared, dtype=np.float64),
                 U0=np.asarray(U0, dtype=np.float64), env_params=par_shared)
    _apply_per_trial(eng, {k: v[1] for k, v in split.items()}, cov_slots, pt)
    if par_slots is not None:
        eng.set_env_params_slots(par_slots)
    _apply_scenarios(eng, model, model_per_slot, risk)
    if x0 is not None:
        eng.set_state(np.asarray(x0, dtype=np.float64).reshape(num_trials, ss))
    if noise_id(noise) != 0:
        eng.set_noise_kind(noise)
    t0 = time.time()
    traced = not (trace is None or trace is False)
    rec, tr_out = eng.run_trials(num_steps, 0, trace=trace) if traced else (eng.run_trials(num_steps, 0), None)
    ex = time.time() - t0
    eng.close()
    table = np.concatenate([rec[:, :3], np.full((num_trials, 1), ex)], 1)
    summ = _summary(table)
    if log_runs and not quiet:
        print("Trial    #: %12s : %7s: %12s : %7s" % ("Reward", "Steps", "Reward/Step", "Ex Time"))
        for k, row in enumerate(table):
            print("Trial %4d: %12.2f : %7d: %12.2f : %7.2f" % (k + 1, row[0], int(row[1]), row[2], row[3]))
        print("-----------------------------------")
        for name in ("AVE", "STD", "MED", "L95", "U95", "MIN", "MAX"):
            print("Trials %3s: %12.2f : %7.2f: %12.2f : %7.2f" % ((name,) + tuple(summ[name])))
    return (rec, summ, tr_out) if traced else (rec, summ)


_SIMPLE_KW = dict(num_trials=1, num_steps=200, policy_type="cemppi", num_samples=20, horizon=15, λ=0.1, α=1.0, U0=(0.0,),
                  cov_mat=(1.5,), ais_its=5, λ_ais=0.1, ce_elite_threshold=0.8, ce_Σ_est="mle", cma_σ=0.75,
                  cma_elite_threshold=0.8, seed=None, x0=None, log_runs=True, device=0, quiet=False, env_params=None, trace=None, noise="philox",
                  model_params=None, risk="mean")


def simulate_mountaincar(**kw):
    """mountaincar_example.jl:49-207 (same keyword arguments and defaults); x0: per-trial start positions
    (the reference draws x ~ U(-0.6,-0.4) from an unseeded RNG; default here -0.5).  env_params: the 8 values include/mpopis.h lists for
    MountainCar, or (num_trials, 8) for one vector per trial.  trace: as simulate_car_racing; the call then returns (records, summary, trace).
    noise: "philox" (default), "antithetic" or "lhs", as simulate_car_racing.  model_params ((M, 8) or (num_trials, M, 8)) / risk: plan against M
    models while env_params stays the plant, as simulate_car_racing."""
    a = dict(_SIMPLE_KW); _check_kw(a, kw); a.update(kw)
    if a["x0"] is not None:
        x = np.asarray(a["x0"], dtype=np.float64).reshape(a["num_trials"])
        a["x0"] = np.stack([x, np.zeros(a["num_trials"])], 1)
    return _simulate_simple("mountaincar", 2, **a)


def simulate_cartpole(**kw):
    """cartpole_example.jl:8-190 (same keyword arguments and defaults); x0: (num_trials, 4) start states
    [x, xdot, theta, thetadot].  The reference draws 0.1*rand(4) - 0.05 from an unseeded MersenneTwister (:111);
    default here: the same box drawn from numpy's default_rng(seed + k).  env_params: the 11 values include/mpopis.h lists for CartPole, or
    (num_trials, 11) for one vector per trial.  trace: as simulate_car_racing; the call then returns (records, summary, trace).
    noise: "philox" (default), "antithetic" or "lhs", as simulate_car_racing.  model_params ((M, 11) or (num_trials, M, 11)) / risk: plan against M
    models while env_params stays the plant, as simulate_car_racing."""
    a = dict(_SIMPLE_KW); _check_kw(a, kw); a.update(kw)
    if a["seed"] is None:
        a["seed"] = int(np.random.default_rng().integers(1, 10 ** 10))
    if a["x0"] is None:
        a["x0"] = np.stack([0.1 * np.random.default_rng(a["seed"] + k + 1).random(4) - 0.05 for k in range(a["num_trials"])])
    return _simulate_simple("cartpole", 4, **a)


def _check_kw(allowed, kw):
    bad = [k for k in kw if k not in allowed]
    if bad:
        raise TypeError("unexpected keyword argument(s): %s" % ", ".join(bad))
