/*
 * mpopis.h -- C ABI of the MI355X-native MPPI/MPOPI sampling engine (libmpopis_hip.so).
 *
 * Drop-in boundary for the rollout-and-reweight hot path of sisl/MPOPIS
 * (src/mppi_mpopi_policies.jl).  The reference has NO FFI; its plug-in seam is Julia dispatch on
 * (policy type, env type) -- it already specialises these three functions for EnvpoolEnv
 * (src/mppi_mpopi_policies.jl:148,240; src/utils.jl:103).  Each entry point below replaces the
 * reference interface cited next to it; julia/MPOPISHip.jl and INTEGRATION.md show the ccall
 * methods a maintainer adds.  All file:line citations are relative to the reference repo root.
 *
 * Conventions
 *   - plain C: pointers + sizes, FP64 everywhere (the reference hard-codes Float64,
 *     src/mppi_mpopi_policies.jl:3-5,13,110-111), Julia column-major layouts, no repacking.
 *   - a handle owns B = cfg.batch independent "trial slots" (independent env + policy pairs =
 *     the `for k in 1:num_trials` axis of src/examples/car_example.jl:170); every array argument
 *     is the concatenation over slots b = 0..B-1 of the per-trial reference array.
 *   - the caller owns all host arrays; the library copies in/out during the call and never
 *     retains host pointers.  Calls are synchronous (return after the stream has drained).
 *   - return 0 on success; negative codes mirror the reference's error()/exception sites:
 *       MPOPIS_ERR_ARG     (-1) size/argument errors     src/mppi_mpopi_policies.jl:55,64,73,79-80
 *       MPOPIS_ERR_NOT_PD  (-2) PosDefException from MvNormal(Sigma')   :447,551,723,796
 *       MPOPIS_ERR_ACTION  (-3) "Action is not in action space" / NaN   src/envs/car_racing.jl:239
 *       MPOPIS_ERR_HIP     (-4) HIP runtime failure / no device
 *       MPOPIS_ERR_NUMERIC (-5) :cmamppi only: Σ^-0.5 δw (:580-581) could not be formed because Σ, tr(Σ^-1) or δw is not finite.
 *                               (Until ABI 4 also raised when cond(Σ) exceeded the 1e14 the Lanczos quadrature resolves; since ABI 5 such a
 *                               slot is answered by a dense symmetric eigen-solve on the device, like the reference's eigen-based Σ^-0.5,
 *                               and a non-positive eigenvalue there is MPOPIS_ERR_NOT_PD.)
 *     mpopis_last_error() returns a human readable message for the last failure.
 *   - a handle is not thread-safe; distinct handles are independent (own HIP stream).
 */
#ifndef MPOPIS_H
#define MPOPIS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ABI history.  1: round-1 surface.  2: + mpopis_seed_slots, mpopis_get_Sigma, mpopis_set_overlap, mpopis_comm_unique_id / _init / _destroy,
 * mpopis_gather_summary, and the error code MPOPIS_ERR_NUMERIC.  A version-1 caller keeps working against a version-2 library (nothing was
 * removed or changed in meaning); a caller that needs the newer entry points checks mpopis_abi_version() >= 2.
 * Error precedence when several slots / kernels fail in one call: MPOPIS_ERR_HIP > MPOPIS_ERR_ACTION > MPOPIS_ERR_NOT_PD > MPOPIS_ERR_NUMERIC --
 * the version-1 codes keep their order (numeric minimum) and are never hidden by MPOPIS_ERR_NUMERIC.
 * 3: + mpopis_policy_call (control = pol(env) with a single host wait).  Nothing removed or changed in meaning.
 * 4: no new entry point; the execution knob mpopis_set_overlap changed: the default (on <= 0) is now the engine's own choice of schedule for the
 *    handle's shape instead of one stream, and on = 1 means "one stream" instead of "two halves".  Results never depended on the knob (bit-identical
 *    per slot in every schedule), so a version-3 caller sees the same numbers, sooner.
 * 5: + mpopis_comm_count (the number of ranks RCCL itself reports for the handle's communicator).  Limits lifted, nothing changed in meaning: any K for
 *    :cemppi / :cmamppi / :pmcmppi (were <= 8192 / 7168), and cond(Σ) beyond 1e14 under :cmamppi is computed instead of MPOPIS_ERR_NUMERIC.
 *    Later gained the enum value MPOPIS_POL_NESMPPI = 8 and nothing else (no entry point, mpopis_config unchanged): a library without it answers
 *    policy = 8 with MPOPIS_ERR_ARG / "No policy_type of that kind", which is how a caller detects support.
 *    Later still, num_cars up to MPOPIS_MAX_CARS = 8 (was 4), and nothing else: a library that predates it answers num_cars = 5..8 with
 *    MPOPIS_ERR_ARG / "num_cars must be 1..4".  Since then :cemppi, :μΣaismppi and :pmcmppi refuse cs > 800 at create (MPOPIS_ERR_ARG): their
 *    covariance scatter stages at most 800 rows, and earlier libraries returned a wrong Σ′ there (past 512 rows) instead of refusing.
 *    Later gained the env kind MPOPIS_ENV_CUSTOM = 3 and ONE entry point, mpopis_create_custom (a handle on a caller-supplied env compiled to a
 *    gfx950 code object, include/mpopis_env.h); mpopis_config and every other entry point are unchanged.  A library that predates it does not
 *    export the symbol, which is how a caller detects support (env_kind = 3 was "unknown env kind" to mpopis_create before and is still refused
 *    there, now with a message that names the new entry point).
 *    Later gained ONE more entry point, mpopis_set_env_table: a read-only table of doubles (a path, an obstacle list, a cost grid, a lookup
 *    curve), per handle or per trial slot, for custom envs built with MPOPIS_DEFINE_ENV_TABLE of include/mpopis_env.h, whose two functions take
 *    (..., const double *tab, int ntab).  MPOPIS_DEFINE_ENV, its kernels, mpopis_config and every other entry point are unchanged; a library
 *    that predates it does not export the symbol, which is how a caller detects support (its mpopis_create_custom refuses such a code object:
 *    it finds none of the kernels it looks for).
 *    Later gained THREE more entry points, mpopis_set_slot_hyper, mpopis_get_slot_hyper and mpopis_set_Sigma_slots: λ, α, λ_ais, σ (step_factor
 *    under :nesmppi) and pol.Σ per trial slot, so that one resident batch can sweep them.  mpopis_config and every other entry point are unchanged,
 *    and a handle that never calls them runs what it ran before; a library that predates them does not export the symbols, which is how a caller
 *    detects support.
 *    Later gained TWO more entry points, mpopis_set_env_params_slots and mpopis_set_tracks: the parameter vector of the built-in envs and the
 *    track of the car env per trial slot, so that one resident batch can hold a policy's trials on several tracks or a robustness study over
 *    car parameters.  mpopis_config and every other entry point are unchanged, and a handle that never calls them runs what it ran before; a
 *    library that predates them does not export the symbols, which is how a caller detects support.
 *    Later gained ONE more entry point, mpopis_get_plan: the control sequence the last policy step chose, the states it predicts, and the step's
 *    highest-weight sample rollouts, read out on request from what is still resident after the step.  mpopis_config and every other entry point
 *    are unchanged, and a handle that never calls it allocates and launches nothing new; a library that predates it does not export the
 *    symbol, which is how a caller detects support.
 *    Later gained ONE more entry point, mpopis_run_trials_traced, and the struct mpopis_trace it takes: the closed loop of mpopis_run_trials that
 *    also records each step's driven state, reward, iteration count, lane / β read-out and, every plan_every steps, the plan of mpopis_get_plan,
 *    all from inside the resident loop.  mpopis_config and every other entry point are unchanged, mpopis_run_trials enqueues what it enqueued
 *    before; a library that predates it does not export the symbol, which is how a caller detects support.
 *    Later gained ONE more entry point, mpopis_set_env_params_cars: one parameter vector per CAR of a multi-car slot, as every env.envs[i] of the
 *    reference's MultiCarRacingEnv owns its params (a heavy car beside a light one, worn tyres beside fresh ones).  mpopis_config and every other
 *    entry point are unchanged, and a handle that never calls it launches what it launched before; a library that predates it does not export
 *    the symbol, which is how a caller detects support (it gives every car of a slot the slot's one vector).
 *    Later gained THREE more entry points, mpopis_set_noise_kind, mpopis_get_noise_kind and mpopis_draw_normals, and the enum MPOPIS_NOISE_*: the
 *    proposal's standard normals drawn on the device by antithetic pairs or Latin-hypercube strata instead of plain Philox / Box-Muller, and a
 *    read-out of the normals the handle draws.  mpopis_config and every other entry point are unchanged, and a handle that never leaves
 *    MPOPIS_NOISE_PHILOX (or returns to it) launches what it launched before, bit for bit; a library that predates them does not export the
 *    symbols, which is how a caller detects support.
 *    Later gained FOUR more entry points, mpopis_set_scenarios, mpopis_set_risk, mpopis_get_scenarios and mpopis_get_scenario_costs, and the enum
 *    MPOPIS_RISK_*: every rollout of a policy step scored under up to 16 model parameter vectors that need not be the plant's, the K costs the
 *    step sees being a risk aggregate (mean, worst case, tail mean / CVaR, entropic) of the per-model costs.  mpopis_config and every other entry
 *    point are unchanged, and a handle that never calls mpopis_set_scenarios (or ends the mode with M = 0) launches what it launched before, bit
 *    for bit; a library that predates them does not export the symbols, which is how a caller detects support. */
#define MPOPIS_ABI_VERSION 5

enum { MPOPIS_OK = 0, MPOPIS_ERR_ARG = -1, MPOPIS_ERR_NOT_PD = -2, MPOPIS_ERR_ACTION = -3, MPOPIS_ERR_HIP = -4, MPOPIS_ERR_NUMERIC = -5 };

/* env kinds: RL.jl MountainCarEnv(continuous=true) + src/examples/mountaincar_example.jl:4-22;
 * CarRacingEnv src/envs/car_racing.jl (num_cars==1) / MultiCarRacingEnv src/envs/multi-car_racing.jl;
 * RL.jl CartPoleEnv(continuous=true) + src/examples/cartpole_example.jl:3-6 (state [x,xdot,theta,thetadot]) */
enum { MPOPIS_ENV_MOUNTAINCAR = 0, MPOPIS_ENV_CAR = 1, MPOPIS_ENV_CARTPOLE = 2,
       MPOPIS_ENV_CUSTOM = 3 };      /* any env written against include/mpopis_env.h: only through mpopis_create_custom */
/* largest num_cars of the car env (MultiCarRacingEnv(N) takes any N in the reference) */
#define MPOPIS_MAX_CARS 8

/* policy kinds = get_policy symbols, src/examples/example_utils.jl:20-128 */
enum { MPOPIS_POL_MPPI = 0,            /* :mppi       MPPI_Policy      :107-216 */
       MPOPIS_POL_GMPPI = 1,           /* :gmppi      GMPPI_Policy     :284-315 */
       MPOPIS_POL_IMPPI = 2,           /* :imppi      IMPPI_Policy     :321-373 */
       MPOPIS_POL_CEMPPI = 3,          /* :cemppi     CEMPPI_Policy    :379-472 */
       MPOPIS_POL_CMAMPPI = 4,         /* :cmamppi    CMAMPPI_Policy   :478-606 */
       MPOPIS_POL_MUAISMPPI = 5,       /* :μaismppi   μAISMPPI_Policy  :612-671 */
       MPOPIS_POL_MUSIGMAAISMPPI = 6,  /* :μΣaismppi  μΣAISMPPI_Policy :677-742 */
       MPOPIS_POL_PMCMPPI = 7,         /* :pmcmppi    PMCMPPI_Policy   :748-817 */
       MPOPIS_POL_NESMPPI = 8 };       /* :nesmppi    NESMPPI_Policy   :819-893 (exported, src/MPOPIS.jl:34; not a get_policy symbol)
                                        *   opt_its in ais_its, step_factor in cma_sigma; K >= 2, cs <= 512 */

enum { MPOPIS_SIGMA_EST_MLE = 0, MPOPIS_SIGMA_EST_SS = 1, MPOPIS_SIGMA_EST_LW = 2, MPOPIS_SIGMA_EST_RBLW = 3,
       MPOPIS_SIGMA_EST_OAS = 4 };   /* CEMPPI Σ_est :414-426 (:mle exact; shrinkage estimators restate CovarianceEstimation.jl, unpinned) */

/* Car parameter vector (20 doubles) = CarRacingEnvParams fields in declaration order
 * (src/envs/car_racing.jl:2-21) followed by dt, δt (:33-34).  MountainCar: 8 doubles
 * {min_pos,max_pos,max_speed,goal_pos,goal_velocity,power,gravity,max_steps}.  CartPole: 11 doubles
 * {gravity,masscart,masspole,totalmass,halflength,polemasslength,forcemag,dt,thetathreshold,xthreshold,max_steps}. */
#define MPOPIS_CAR_NPARAMS 20
#define MPOPIS_MOUNTAINCAR_NPARAMS 8
#define MPOPIS_CARTPOLE_NPARAMS 11

typedef struct mpopis_handle mpopis_handle;

/* Mirrors the keyword arguments of MPPI_Policy_Params (:36-47) and of the per-policy
 * constructors (:337-340,:407-412,:506-511,:630-634,:695-699,:766-770). */
typedef struct {
    int32_t device;            /* HIP device ordinal                                              */
    int32_t env_kind;          /* MPOPIS_ENV_*                                                    */
    int32_t num_cars;          /* car env: 1 => CarRacingEnv, 2..MPOPIS_MAX_CARS => MultiCarRacingEnv(N)
                                  (cs = 2 num_cars H: :cemppi / :μΣaismppi / :pmcmppi need cs <= 800,
                                  :cmamppi cs <= 710, :nesmppi cs <= 512; MPOPIS_ERR_ARG otherwise) */
    int32_t policy;            /* MPOPIS_POL_*                                                    */
    int32_t num_samples;       /* K                                                               */
    int32_t horizon;           /* H (T in the reference code)                                     */
    int32_t batch;             /* B resident independent trials                                   */
    int32_t ais_its;           /* opt_its / ais_its N (ignored for :mppi/:gmppi)                  */
    int32_t sigma_est;         /* MPOPIS_SIGMA_EST_* (:cemppi)                                    */
    int32_t log_trajectories;  /* params.log: keep K x H x ss model trajectories (MPPI_Logger)   */
    /* λ, α, λ_ais and cma_sigma hold in every slot until mpopis_set_slot_hyper gives the slots their own */
    double lambda;             /* λ                                                               */
    double alpha;              /* α ; γ = λ(1-α)                                                  */
    double lambda_ais;         /* λ_ais (:μaismppi/:μΣaismppi/:pmcmppi)                           */
    double elite_threshold;    /* ce_elite_threshold / elite_perc_threshold (always shared)       */
    double cma_sigma;          /* σ (:cmamppi) / step_factor (:nesmppi)                           */
    uint64_t seed;             /* trial slot b draws from seed+b+1 (seed!(pol, seed+k), car_example.jl:188) */
} mpopis_config;

/* Injected randomness for results-parity runs (NULL => device Philox4x32-10 streams).
 * The reference draws from Julia's MersenneTwister, which is not reproduced; parity is defined
 * on identical standard normals / resampling draws. */
typedef struct {
    const double *Z;        /* G-variants: B x N x (cs x K col-major randn! matrix, :308,:448,:556,:657,:724,:797)
                               :mppi: B x (K*T*as), element ((t*K+k)*as+a)  (rand(rng,P,K,T), :193)  */
    const int32_t *res_i0;  /* :pmcmppi: B x (N-1) x K uniform ints in [0,K) (0-based)  (:805)   */
    const double *res_u;    /* :pmcmppi: B x (N-1) x K uniforms in [0,1)                          */
} mpopis_noise;

/* ---- lifetime ---------------------------------------------------------------------------- */
int  mpopis_abi_version(void);
const char *mpopis_last_error(const mpopis_handle *h);     /* h may be NULL: last create() error  */

/* XPolicy(env; kwargs...) + env construction: src/mppi_mpopi_policies.jl:116-119,298-301,...;
 * src/examples/car_example.jl:172-185.  Defaults after create: env params = reference
 * defaults, track = none (must be set for car envs), bounds = [-1,1], U = 0, Sigma = I. */
int  mpopis_create(const mpopis_config *cfg, mpopis_handle **out);
/* XPolicy(env; kwargs...) for ANY env: the reference runs every policy on every AbstractEnv that has env(a), reward(env), state(env) and
 * action_space(env) (rollout_model(env::AbstractEnv, ...) src/utils.jl:129-144; simulate_model(pol, env::AbstractEnv, ...)
 * src/mppi_mpopi_policies.jl:261-278).  Here env(a) and reward(env) are two device functions compiled with include/mpopis_env.h into a
 * gfx950 code object (hipcc --genco); the engine loads it and launches its kernels where it launches its own rollout / env-step kernels.
 *   cfg            as for mpopis_create; env_kind and num_cars are ignored (the handle's env kind is MPOPIS_ENV_CUSTOM)
 *   code_object    nbytes bytes: the ELF or clang offload bundle hipcc wrote; copied by the runtime, not retained
 *   state_size 1..64, action_size 1..16, nparams 0..64: must equal what the code object was built with (cs = action_size H obeys the
 *                  per-policy limits listed at mpopis_config.num_cars)
 *   reset_state    state_size doubles that mpopis_reset restores in every slot (with t = 0, done = 0), or NULL for zeros
 * A code object built with MPOPIS_DEFINE_ENV_TABLE also takes a data table: mpopis_set_env_table below.
 * On such a handle mpopis_set_env_params takes exactly nparams doubles (default: zeros), mpopis_set_action_bounds holds per action
 * (default [-1, 1]), mpopis_env_query returns reward(env) and within = 1, mpopis_run_trials ends a slot when the env sets done, and
 * mpopis_set_track / mpopis_set_state_noise have no effect; everything else works as on a built-in env.  The module is unloaded by
 * mpopis_destroy; handles with different code objects coexist. */
int  mpopis_create_custom(const mpopis_config *cfg, const void *code_object, uint64_t nbytes,
                          int32_t state_size, int32_t action_size, int32_t nparams,
                          const double *reset_state /* state_size doubles or NULL => zeros */, mpopis_handle **out);
void mpopis_destroy(mpopis_handle *h);

/* ---- env description (the env protocol the path consumes) ------------------------ */
int  mpopis_set_env_params(mpopis_handle *h, const double *p, int32_t n);   /* env.params, env.dt, env.δt */
/* The data table of a custom env built with MPOPIS_DEFINE_ENV_TABLE (include/mpopis_env.h): what the reference keeps in the fields of its env
 * struct beside the state -- env.track of CarRacingEnv (src/envs/car_racing.jl:28-40) is one -- handed to the env's step and reward functions as
 * (tab, ntab) and indexable at run time.
 *   n         doubles per slot, 0..MPOPIS_ENV_MAX_TABLE (2^20); n = 0 clears the table (data may then be NULL): the env runs with ntab == 0,
 *             as it does before the first call
 *   per_slot  0: data holds n doubles that every slot sees; otherwise B*n doubles, slot b sees data[b*n .. b*n+n)
 * May be called any number of times, with a different n each time; the call waits for everything the handle has queued before the table is
 * replaced.  Values are the caller's business (non-finite ones are not refused).  Tables of up to MPOPIS_ENV_TABLE_LDS_DOUBLES (4096) doubles are
 * staged in LDS by the rollout kernel, larger ones are read from global memory; results do not depend on which.
 * MPOPIS_ERR_ARG: a handle that is not custom, a code object without a table, n out of range, NULL data with n > 0. */
int  mpopis_set_env_table(mpopis_handle *h, const double *data, int64_t n, int32_t per_slot);
int  mpopis_set_track(mpopis_handle *h, const double *x, const double *y, const double *w, int32_t P);
                                                                  /* env.track.{x′,y′,lane_width′} car_racing_tracks.jl:21-23 */
/* Per-slot env parameters and tracks: slot b behaves like a handle given p[b*n .. b*n+n) through mpopis_set_env_params and track
 * track_of_slot[b] through mpopis_set_track.  They hold for mpopis_rollout_costs, mpopis_policy_step, mpopis_policy_call, mpopis_env_step,
 * mpopis_env_query, mpopis_run_trials and mpopis_bench_policy_steps.  Action bounds, K, H and N stay shared.
 *   mpopis_set_env_params_slots  B vectors of n doubles: n = 20 on a car handle (all cars of a multi-car slot share the slot's vector; one per car: mpopis_set_env_params_cars), 8 on
 *                                MountainCar, 11 on CartPole.  MPOPIS_ERR_ARG: another n, NULL p, a custom handle (per-slot data of a custom
 *                                env goes through mpopis_set_env_table(..., per_slot)).  mpopis_set_env_params afterwards returns the handle
 *                                to one shared vector.
 *   mpopis_set_tracks            car handles only.  ntracks tracks, track i with P[i] points (2..2048 each); x, y, w hold them one after the
 *                                other (sum of P doubles each).  Slot b drives on track track_of_slot[b] (0-based); NULL: ntracks must equal
 *                                B and slot b gets track b.  Every track is uploaded once, however many slots refer to it.  MPOPIS_ERR_ARG
 *                                with the offending track or slot in mpopis_last_error: a P[i] or a track_of_slot[b] out of range, a NULL
 *                                array, a handle of another env kind.  Either this call or mpopis_set_track satisfies the calls that need a
 *                                track; mpopis_set_track afterwards returns the handle to one shared track.
 * Every slot of a launch runs one rollout kernel, chosen by the handle's LARGEST track (every table in LDS up to 190 points, beyond that the
 * ring table only); a slot's costs can therefore differ in the last bits from those of a one-slot handle on the same track when the two fall on
 * different sides of that limit.
 * The tracks of every mpopis_set_track / mpopis_set_tracks call stay allocated until mpopis_destroy (about 170 bytes per track point): a
 * study that swaps track sets very many times should do so on fresh handles.
 * Setup calls like mpopis_set_slot_hyper below: they wait for everything the handle has queued before they write; a refused call leaves the
 * handle as it was; the per-slot arrays are allocated at the first call (MPOPIS_ERR_HIP when that fails, the handle then stays shared). */
int  mpopis_set_env_params_slots(mpopis_handle *h, const double *p /* B*n */, int32_t n);
int  mpopis_set_tracks(mpopis_handle *h, int32_t ntracks, const int32_t *P, const double *x, const double *y, const double *w,
                       const int32_t *track_of_slot /* B or NULL */);
/* A fleet: every car of a multi-car slot with its own parameter vector (MultiCarRacingEnv(N; car_params = [...]) and env.envs[i] of
 * src/envs/multi-car_racing.jl:23-45; env(a) steps car i with its own params, reward(env) sums every car's own reward, :145-158, :200-207).
 * Car handles only, n = MPOPIS_CAR_NPARAMS.
 *   per_slot  0: p holds num_cars*20 doubles and every slot gets that fleet; otherwise B*num_cars*20.  Car c of slot b then behaves like a
 *             CarRacingEnv constructed with p[(b*num_cars + c)*20 ..].
 * It holds for mpopis_rollout_costs, mpopis_policy_step, mpopis_policy_call, mpopis_env_step, mpopis_env_query, mpopis_get_plan,
 * mpopis_run_trials (a car counts as beyond the β limit when it exceeds ITS OWN), mpopis_run_trials_traced and mpopis_bench_policy_steps.
 * dt and δt (entries 18, 19) must be equal across the cars of one slot -- a MultiCarRacingEnv has one of each -- and may differ between slots.
 * A fleet handle runs a rollout kernel of its own (one wave per car); with equal vectors its costs agree with a shared handle's to rounding,
 * not necessarily to the bit.  mpopis_set_env_params or mpopis_set_env_params_slots afterwards return the handle to one vector per slot, with
 * the results of a handle that never had a fleet.  Independent of mpopis_set_track / mpopis_set_tracks: a fleet handle may carry per-slot tracks.
 * On a num_cars == 1 handle the call is mpopis_set_env_params (per_slot == 0) or mpopis_set_env_params_slots.
 * A setup call like mpopis_set_env_params_slots (waits for what is queued, allocates at the first call -- MPOPIS_ERR_HIP when that fails --, a
 * refused or failed call leaves the handle as it was).  MPOPIS_ERR_ARG: another env kind, a custom handle, n != 20, NULL p, dt or δt that
 * differ inside a slot (mpopis_last_error names the slot and the car). */
int  mpopis_set_env_params_cars(mpopis_handle *h, const double *p /* [B*]num_cars*n */, int32_t n /* 20 */, int32_t per_slot);
/* Scenarios: score every rollout of a policy step under M model parameter vectors and hand the step a risk aggregate.
 *   mpopis_set_scenarios  M = 1..MPOPIS_MAX_SCENARIOS vectors of n doubles (n as for mpopis_set_env_params_slots; all cars of a multi-car slot share
 *     the scenario's vector).  per_slot == 0: p holds M*n doubles for every slot; otherwise B*M*n, slot b / scenario m at p[(b*M+m)*n].  From then on
 *     every rollout of a policy step of slot b (mpopis_policy_step, mpopis_policy_call, mpopis_rollout_costs, mpopis_run_trials[_traced],
 *     mpopis_bench_policy_steps) runs once per scenario -- same start state, pol.U, noise and control cost -- and the K costs the rest of the step
 *     sees (weights, elite sort, resampling, moments, the `cost` outputs, the non-finite check) are the aggregate J of the M scenario costs of each
 *     sample.  Nothing else of any policy changes.  THE REAL ENV IS UNTOUCHED: mpopis_env_step, mpopis_env_query, mpopis_reset, the bookkeeping of
 *     mpopis_run_trials and the state noise keep the handle's own parameters (shared or per slot), and mpopis_set_env_params[_slots] after this call
 *     change the plant only -- M = 1 is "model != plant".  Scenario 0 is the nominal model: the rollouts of mpopis_get_plan and of the trace's
 *     plans run under it.  M = 0 (p may be NULL) ends the mode: results are then again, bit for bit, those of a handle that never had scenarios.
 *     A setup call like mpopis_set_env_params_slots (waits for what is queued, allocates at the first call and when M grows -- MPOPIS_ERR_HIP when
 *     that fails --, a refused call leaves the handle as it was).  It resets the risk to the mean (MPOPIS_RISK_TAIL_MEAN, tail = M).
 *     MPOPIS_ERR_ARG: M outside 0..16, a wrong n, NULL p with M > 0, a custom handle, a handle created with log_trajectories (the logger has one
 *     trajectory per sample), a fleet handle (mpopis_set_env_params_cars in force).  mpopis_set_env_params_cars on a scenario handle is refused too.
 *   mpopis_set_risk  with the scenario costs c_0..c_{M-1} of one sample:
 *     MPOPIS_RISK_TAIL_MEAN, tail in 1..M (0 means M): J = the mean of the `tail` largest costs, summed from the largest down.  tail = M is the
 *       expectation, tail = 1 the worst case (the bits of that input), tail = ceil(qM) the discrete CVaR_q.  Any NaN among the c_m gives NaN;
 *       otherwise plain IEEE arithmetic (an infinity takes part in the sort and the sum).
 *     MPOPIS_RISK_ENTROPIC, finite theta != 0: J = c* + (1/theta) log((1/M) sum_m exp(theta (c_m - c*))), c* = max c_m for theta > 0 (risk-averse),
 *       min c_m for theta < 0.  If any c_m is not finite, J is the IEEE sum of the non-finite c_m: NaN if one is NaN or both infinities occur,
 *       else that infinity.
 *     A non-finite J raises MPOPIS_ERR_ACTION in the slot's status where a non-finite rollout cost does.
 *     MPOPIS_ERR_ARG: no scenarios set, an unknown kind, tail outside 0..M, theta zero or non-finite (MPOPIS_RISK_ENTROPIC).
 *   mpopis_get_scenarios  M (0: off), kind, tail (as resolved: 1..M) and theta in force; any pointer may be NULL.
 *   mpopis_get_scenario_costs  out[(b*M+m)*K+k]: the scenario costs behind the slot's current `cost`, i.e. of the last rollout the slot executed
 *     (slots that broke early keep those of their last iteration).  A getter like mpopis_draw_normals.  MPOPIS_ERR_ARG without scenarios. */
#define MPOPIS_MAX_SCENARIOS 16
enum { MPOPIS_RISK_TAIL_MEAN = 0, MPOPIS_RISK_ENTROPIC = 1 };
int  mpopis_set_scenarios(mpopis_handle *h, int32_t M, const double *p /* [B*]M*n */, int32_t n, int32_t per_slot);
int  mpopis_set_risk(mpopis_handle *h, int32_t kind, int32_t tail, double theta);
int  mpopis_get_scenarios(mpopis_handle *h, int32_t *M, int32_t *kind, int32_t *tail, double *theta);
int  mpopis_get_scenario_costs(mpopis_handle *h, double *out /* B*M*K */);
int  mpopis_set_action_bounds(mpopis_handle *h, const double *lo, const double *hi); /* action_space(env) */
int  mpopis_reset(mpopis_handle *h);                       /* reset!(env) per slot: car_racing.jl:215-223, multi :160-180 */
int  mpopis_set_state(mpopis_handle *h, const double *x /* B*ss */, const int32_t *t, const int32_t *done);
int  mpopis_get_state(mpopis_handle *h, double *x /* B*ss */, int32_t *t, int32_t *done);

/* ---- policy state ---------------------------------------------------------------------------- */
int  mpopis_set_U(mpopis_handle *h, const double *U /* B*cs */);            /* pol.U                */
int  mpopis_get_U(mpopis_handle *h, double *U /* B*cs */);
int  mpopis_set_Sigma(mpopis_handle *h, const double *Sigma, int32_t n);    /* pol.Σ : n = as (mppi, or block-replicated :76-78) or cs; col-major, shared by all slots
                                                                             * (after mpopis_set_Sigma_slots: returns the handle to ONE shared Σ).
                                                                             * A refused call (size, not positive definite) leaves the handle as it was:
                                                                             * the Σ in force, its factor and the sampler's scales are replaced only
                                                                             * once the new matrix has passed every check. */
/* Per-slot policy hyper-parameters and pol.Σ: slot b behaves like a handle created with lambda[b], alpha[b], lambda_ais[b], cma_sigma[b]
 * and given Sigma[b] through mpopis_set_Sigma (γ_b = λ_b (1 - α_b); :imppi weighs its AIS iterations with λ_b).  They hold for
 * mpopis_policy_step, mpopis_policy_call, mpopis_run_trials, mpopis_bench_policy_steps and mpopis_rollout_costs (γ_b scales the one
 * Sigma_inv that call is given).  K, H, N, elite_threshold, the estimator and action bounds stay shared (env parameters and tracks: mpopis_set_env_params_slots / mpopis_set_tracks above).
 *   mpopis_set_slot_hyper   each pointer is B doubles, or NULL = "the config's value in every slot"; four NULLs return the handle to the
 *                           shared scalars.  Accepts what mpopis_create accepts for the same fields (MPOPIS_ERR_ARG only for a non-finite
 *                           step_factor under :nesmppi).  With per-slot lambda_ais, :μΣaismppi on a car env computes the AIS weights in a launch
 *                           of their own instead of inside the moments kernel (a different summation: last-bits differences).
 *   mpopis_get_slot_hyper   what is in force, B doubles each; any pointer may be NULL
 *   mpopis_set_Sigma_slots  B matrices, each n x n col-major, n = as (block-replicated, and the only size for :mppi) or cs, checked per slot
 *                           like mpopis_set_Sigma: MPOPIS_ERR_ARG "Covariance matrix size problem", MPOPIS_ERR_NOT_PD with the slot number in
 *                           mpopis_last_error.  The diagonal sampler is used only when EVERY slot's Σ is diagonal.  mpopis_get_Sigma returns each
 *                           slot's own pol.Σ for the policies that keep Σ fixed.  mpopis_set_Sigma afterwards returns to the shared Σ.
 * Setup calls like mpopis_set_env_table: they wait for everything the handle has queued before they write; a refused call leaves the handle
 * as it was; buffers are allocated at the first call (MPOPIS_ERR_HIP when that fails, the handle then stays shared).  After the handle has
 * returned to the shared values its results are again those of a handle that was never switched. */
int  mpopis_set_slot_hyper(mpopis_handle *h, const double *lambda, const double *alpha,
                           const double *lambda_ais, const double *cma_sigma /* σ of :cmamppi, step_factor of :nesmppi */);
int  mpopis_get_slot_hyper(mpopis_handle *h, double *lambda, double *alpha, double *lambda_ais, double *cma_sigma);
int  mpopis_set_Sigma_slots(mpopis_handle *h, const double *Sigma /* B*n*n */, int32_t n);
int  mpopis_seed(mpopis_handle *h, uint64_t seed);                          /* seed!(pol, seed) src/MPOPIS.jl:54 */
/* Per-slot seeds: slot b draws from seeds[b] (B values).  The reference seeds trial k with seed!(pol, seed + k),
 * src/examples/car_example.jl:187-188; a rank that holds the trials k0, k0+G, k0+2G, ... of a sharded run
 *  passes {seed + k0, seed + k0 + G, ...} so that all of them stay in ONE resident batch. */
int  mpopis_seed_slots(mpopis_handle *h, const uint64_t *seeds /* B */);
/* How the handle draws the proposal's standard normals on the device, i.e. wherever noise == NULL: mpopis_policy_step, mpopis_policy_call,
 * mpopis_run_trials, mpopis_run_trials_traced and mpopis_bench_policy_steps, for every policy (:mppi included) and every env kind.  One kind per
 * handle.  Injected noise is consumed as it is; the resampling draws of :pmcmppi and the state noise stay Philox draws.
 * Per slot b, Z row r (r = t*as + a in both layouts of mpopis_noise.Z), sample k, MPC step and AIS iteration n:
 *   MPOPIS_NOISE_PHILOX      (default) Z = randn from the slot's Philox4x32-10 stream (step, n) and Box-Muller
 *   MPOPIS_NOISE_ANTITHETIC  with h = ceil(K/2): column k < h is, bit for bit, the MPOPIS_NOISE_PHILOX normal of (r, k); column k >= h is the exact
 *                            negation of column k - h (odd K: column h - 1 has no partner)
 *   MPOPIS_NOISE_LHS         Latin hypercube: sample k of row r falls in stratum j = pi_r(k), a keyed bijection of [0, K) evaluated per element
 *                            (four Feistel rounds over the even number of bits that covers K, cycle walking; round keys = Philox words of
 *                            (seed, step, n, r)); Z = Phi^-1((j + xi) / K) with the jitter xi = (x + 0.5) 2^-32 from a Philox word x of
 *                            (seed, step, n, r, k).  Stratum j with jitter xi and stratum K - 1 - j with jitter 1 - xi give exact negatives.
 *                            K <= 2^20 (MPOPIS_ERR_ARG beyond).
 * The new kinds always draw plain standard normals into memory and scale / unwhiten them with the kernels an injected step runs, so a device step
 * and a step with the same normals injected compute the same bits; results do not depend on the schedule (mpopis_set_overlap).
 *   mpopis_set_noise_kind  a setup call like mpopis_set_slot_hyper: it waits for everything the handle has queued; a refused call (an unknown
 *                          kind, MPOPIS_NOISE_LHS with K > 2^20: MPOPIS_ERR_ARG) leaves the handle as it was.  After a return to
 *                          MPOPIS_NOISE_PHILOX the handle's results are those of a handle that never switched.
 *   mpopis_get_noise_kind  the kind in force
 *   mpopis_draw_normals    the standard normals the handle would draw for MPC step mpc_step and AIS iteration `iteration` (0-based) under its current
 *                          kind and slot seeds, all three kinds, every slot: Z is B x (cs x K col-major) -- one iteration of mpopis_noise.Z --,
 *                          for :mppi B x (K*T*as), element ((t*K+k)*as+a).  A policy step given these as injected noise reproduces the device
 *                          step of the new kinds bit for bit (under MPOPIS_NOISE_PHILOX to rounding: dense shapes draw inside the unwhitening kernel).
 *                          A getter: it advances no RNG position, writes nothing a later call reads and keeps the source of mpopis_get_plan.
 *                          MPOPIS_ERR_ARG: NULL Z, a negative iteration; MPOPIS_ERR_HIP when its B*cs*K-double staging buffers cannot be allocated. */
enum { MPOPIS_NOISE_PHILOX = 0, MPOPIS_NOISE_ANTITHETIC = 1, MPOPIS_NOISE_LHS = 2 };
int  mpopis_set_noise_kind(mpopis_handle *h, int32_t kind);
int  mpopis_get_noise_kind(mpopis_handle *h, int32_t *kind);
int  mpopis_draw_normals(mpopis_handle *h, uint32_t mpc_step, int32_t iteration /* 0-based */, double *Z);
/* Σ′ of the proposal MvNormal the LAST executed AIS iteration of the last policy step drew from, per slot:
 * B x (cs x cs col-major).  (:447,:723,:796 `P = MvNormal(Σ′)`; :cmamppi with N > 1: σ²·Σ′, :550-554; policies
 * that keep pol.Σ fixed return pol.Σ; :nesmppi: A′'A′ of the last executed iteration, pol.Σ when the call broke at n = 1.)  Lets a caller compare the adapted covariance, which the reference
 * only exposes indirectly through the next draw. */
int  mpopis_get_Sigma(mpopis_handle *h, double *Sigma_out /* B*cs*cs */);

/* ---- Level 1: simulate_model(pol, env, E, Σ_inv, U_orig) -> trajectory_cost  (:261-278) ------
 * x0: B*ss (NULL: resident env state); U: B*cs current AIS mean (pol.U); U_orig: B*cs (NULL => U);
 * E: B x (cs x K col-major); Sigma_inv: cs x cs col-major or NULL (required only when γ != 0);
 * cost: B*K out. */
int  mpopis_rollout_costs(mpopis_handle *h, const double *x0, const double *U, const double *U_orig,
                          const double *E, const double *Sigma_inv, double *cost);

/* ---- Level 2: control = pol(env)  (:121-146 for :mppi, :221-238 for the G-variants) ------------
 * Runs calculate_trajectory_costs for the configured policy, the weighted control update and
 * get_controls_roll_U! (src/utils.jl:88-101) for every slot.  Resident env state is used (set it
 * with mpopis_set_state) and pol.U is rolled in place on the device.
 * Outputs (any may be NULL): control B*as; cost B*K; weights B*K; E_out B x (cs x K) after the
 * final shift (:468,:602,:668,:739,:814) [:mppi: B x K*T*as]; resample_idx0 B x (N-1) x K 0-based;
 * iters_run B (AIS iterations executed, CE/CMA may break early :459-461,:567-569). */
int  mpopis_policy_step(mpopis_handle *h, const mpopis_noise *noise,
                        double *control, double *cost, double *weights, double *E_out,
                        int32_t *resample_idx0, int32_t *iters_run);

/* control = pol(env) exactly as the reference's harness calls it once per MPC step, synchronously, for one env the HOST owns
 * (src/examples/car_example.jl:203-207 `act = pol(env); env(act)`; mountaincar_example.jl:150-153): in ONE call and ONE host wait
 *   x, t, done   -> state(env), env.t, env.done of every slot (B*ss, B, B; x NULL: keep the resident state; t / done may be NULL)
 *   U_inout      -> in: pol.U (B*cs) before the call; out: the rolled pol.U (get_controls_roll_U!, src/utils.jl:88-101).  NULL: the
 *                   resident pol.U is used and rolled on the device only
 *   noise        -> NULL: device Philox streams (the production path); non-NULL: as mpopis_policy_step
 *   control B*as, cost B*K, weights B*K, iters_run B: outputs, any may be NULL
 * Equivalent to mpopis_set_state + mpopis_set_U + mpopis_policy_step + mpopis_get_U (four host waits); the small arrays travel through a
 * pinned, device-mapped mailbox owned by the handle instead of copy commands. */
int  mpopis_policy_call(mpopis_handle *h, const double *x, const int32_t *t, const int32_t *done, double *U_inout,
                        const mpopis_noise *noise, double *control, double *cost, double *weights, int32_t *iters_run);

/* env(action) for the resident real envs + reward(env): src/envs/car_racing.jl:238-250,201-213;
 * multi-car_racing.jl:200-207,145-158; mountaincar_example.jl:4-22.  action B*as, reward B out. */
int  mpopis_env_step(mpopis_handle *h, const double *action, double *reward);

/* reward(env), within_track(env), calculate_β(env) for the resident envs WITHOUT stepping
 * (src/envs/car_racing.jl:178-213; car_racing_tracks.jl:68-92; multi-car_racing.jl:122-158).
 * reward B; within B (car: all cars inside the lane, multi-car :122-128; MountainCar: 1);
 * dist / beta: B x num_cars (distance to the centre line, atan(Vy,Vx)); any pointer may be NULL. */
int  mpopis_env_query(mpopis_handle *h, double *reward, int32_t *within, double *dist, double *beta);

/* pol.logger.trajectories (src/mppi_mpopi_policies.jl:92-95, src/utils.jl:139-141): B x K x (H x ss),
 * state after each model step of the LAST simulate_model call; needs cfg.log_trajectories. */
int  mpopis_get_trajectories(mpopis_handle *h, double *out);

/* The plan of the last policy step and its best samples: what the reference's plot(env, pol, perc) draws (src/envs/plots.jl:96-169: the
 * trajectories in the order sortperm(pol.logger.traj_weights, rev=true)), plus the trajectory of the chosen plan itself, which is no sample.
 * Needs no cfg.log_trajectories and adds nothing to a policy step: on request the `top` highest-weight samples are picked on the device, their
 * control sequences and the plan's are rolled out once more (top + 1 rollouts per slot, no control-cost term) and only those come back.
 *   top        0 .. min(K, MPOPIS_PLAN_MAX_TOP); 0 returns the plan alone.  Anything else: MPOPIS_ERR_ARG.
 *   controls   B*cs           weighted_controls = U_orig + weighted noise of the last step (:137,:230), UNCLAMPED and before the roll: the same
 *                             addition the step performed, so controls[as:] equals the rolled pol.U[:cs-as] and clamp(controls[:as]) the returned
 *                             control, bit for bit
 *   traj       B x (top+1) x (H x ss col-major, as mpopis_get_trajectories): entry 0 = the states the plan predicts from the state the step
 *                             started from, entry j = those of sample idx0[j-1]
 *   cost       B x (top+1)    -sum of the rewards along each of those rollouts; NO control-cost term, whatever γ is
 *   idx0       B x top        0-based sample indices in descending weight, equal weights with the lower index first: the stable order of
 *                             sortperm(weights, rev=true)[1:top].  Exact.  (Ties are the normal case: with a small λ most weights underflow to 0.)
 *   weights    B x top        weights[idx0[j]]
 * Any output pointer may be NULL.  Entry 0 is rolled out from controls itself; entry j from U_orig + E_out[:, idx0[j-1]], with E_out the noise
 * "after the final shift" that mpopis_policy_step returns, so a caller can reproduce every rollout from U_orig and E_out.
 * Source and validity: the call reads the last successful mpopis_policy_step / mpopis_policy_call of the handle, which stays readable only
 * until another call writes to the handle.  The getters keep it: mpopis_get_state, mpopis_get_U, mpopis_get_Sigma, mpopis_get_slot_hyper,
 * mpopis_get_trajectories, mpopis_env_query, mpopis_last_error, mpopis_timing_read, mpopis_get_noise_kind, mpopis_draw_normals, mpopis_get_scenarios, mpopis_get_scenario_costs and mpopis_get_plan itself.  EVERY other entry point ends it
 * (mpopis_env_step, mpopis_set_state, mpopis_set_U, mpopis_reset, mpopis_rollout_costs, mpopis_run_trials, mpopis_bench_policy_steps, every
 * setter, the timing switches, the communicator calls), and so does a step that returned an error.  Without a valid source the call returns
 * MPOPIS_ERR_ARG and mpopis_last_error says which of the three applies: no step yet, the last step failed, or which call wrote.
 * The call is synchronous and changes nothing a later step reads: pol.U, the RNG position, cost, weights, E, the logger's trajectories and the
 * iteration counts stay as they are, and a handle that calls it computes the same bits afterwards as one that never does.  Its device buffers
 * (B (top+1) (cs + H ss + 1) doubles and a little more) are allocated at the first call and grown when a later call asks for a larger top;
 * MPOPIS_ERR_HIP when that fails, the handle stays usable. */
#define MPOPIS_PLAN_MAX_TOP 64
int  mpopis_get_plan(mpopis_handle *h, int32_t top, double *controls /* B*cs */, double *traj /* B*(top+1)*H*ss */,
                     double *cost /* B*(top+1) */, int32_t *idx0 /* B*top */, double *weights /* B*top */);

/* ---- Level 3: the closed-loop trial harness, device resident ------------------------------------
 * simulate_car_racing / simulate_mountaincar trial loop (src/examples/car_example.jl:170-326,
 * mountaincar_example.jl:125-180) for all B slots at once, device RNG, no host round trips per
 * MPC step.  One record per slot (MPOPIS_RECORD_LEN doubles):
 *   [0] rew [1] steps [2] rew/step [3..6] lap_t[1..4] [7] mean_v [8] max_v [9] mean_β [10] max_β
 *   [11] β_viol [12] T_viol [13] C_viol [14] rollouts executed [15] status            (:144-155,287-302) */
#define MPOPIS_RECORD_LEN 16
/* state_x_sigma, state_y_sigma, state_ψ_sigma of simulate_car_racing (src/examples/car_example.jl:38-40,224-236): after
 * every real-env step of mpopis_run_trials, single-car slots get x += σx z0, y += σy z1, ψ += δψ (δψ = σψ z2) and (Vx, Vy)
 * rotated passively by δψ.  z from the slot's Philox stream (mpc_step, 0x40000000).  Default 0 (no draws).  Multi-car and
 * non-car envs: ignored, like the reference (`sim_type == :cr` only). */
int  mpopis_set_state_noise(mpopis_handle *h, double sigma_x, double sigma_y, double sigma_psi);
int  mpopis_run_trials(mpopis_handle *h, int32_t num_steps, int32_t laps, double *records /* B*16 */,
                       double *actions /* NULL or B x (num_steps+1) x as */);

/* mpopis_run_trials that also records the run: where every slot's env stood at each MPC step, what the step earned, where the violations
 * happened, and what the controller intended -- what plot_steps / save_gif / plot_traj of src/examples/car_example.jl draw and the per-step
 * rew, v, β its trial loop keeps.  Everything is recorded on the device from inside the resident loop (no host round trip per step, the host
 * still looks at the batch every eighth step) and downloaded once, at the end of the call.
 * S = num_steps + 1 MPC steps per slot at the most; num_cars = 1 on the envs that are no car env.
 *   plan_every   0: no plans.  p > 0: the plan of the MPC steps s = 0, p, 2p, ... <= num_steps; nplans = num_steps / p + 1
 *   top          0 .. min(K, MPOPIS_PLAN_MAX_TOP): that many best samples beside each recorded plan
 *   states       B x (S+1) x ss   [s] the state MPC step s started from, [s+1] the state after env(act) and the state noise
 *   rewards      B x S            reward(env) after step s: the terms mpopis_run_trials sums into records[0]
 *   iters        B x S            AIS iterations step s executed
 *   within       B x S            as mpopis_env_query on states[s+1]
 *   dist, beta   B x S x num_cars as mpopis_env_query on states[s+1] (0 on the envs for which mpopis_env_query returns none)
 *   plan_controls B x nplans x cs, plan_traj B x nplans x (top+1) x (H x ss), plan_cost B x nplans x (top+1), plan_idx0 B x nplans x top,
 *   plan_weights B x nplans x top: entry j is the plan of MPC step j * plan_every -- the fields of mpopis_get_plan, same meaning, same layout
 *                                 per entry
 * Any pointer may be NULL; what is not asked for is neither computed nor stored.
 * A slot that executed n_b = records[b][1] + 1 MPC steps has its entries s < n_b filled (states: s <= n_b) and its plans j * plan_every < n_b;
 * everything past them is zero, like `actions`.  A recorded plan is what mpopis_get_plan(top) returns when called right after that step's policy
 * step and before its env step, bit for bit in every field.  records and actions are the bits mpopis_run_trials returns for the same handle,
 * seed and arguments, whatever the trace asks for; trace == NULL is exactly mpopis_run_trials.  A run that ends on an error status returns what
 * was recorded up to the step at which the host saw it; the return code is that of mpopis_run_trials.
 * MPOPIS_ERR_ARG (reason in mpopis_last_error, handle unchanged): plan_every < 0, top out of range, top > 0 or a plan pointer set with
 * plan_every == 0, and anything mpopis_run_trials refuses.  The trace lives in device memory for the length of the call --
 *   8 B [(S+1) ss + S (2 + 2 num_cars)] + 8 B cs (top+1) + 8 nplans B [cs + (top+1)(H ss + 1) + 1.5 top] bytes at the most, plus the largest
 *   plan field once more for the copy-out (only what is asked for is allocated) --
 * MPOPIS_ERR_HIP when that cannot be allocated; the handle stays usable.  Like mpopis_run_trials the call ends the source of mpopis_get_plan. */
typedef struct {
    int32_t plan_every;
    int32_t top;
    double  *states;
    double  *rewards;
    int32_t *iters;
    int32_t *within;
    double  *dist, *beta;
    double  *plan_controls;
    double  *plan_traj;
    double  *plan_cost;
    int32_t *plan_idx0;
    double  *plan_weights;
} mpopis_trace;
int  mpopis_run_trials_traced(mpopis_handle *h, int32_t num_steps, int32_t laps, double *records, double *actions,
                              const mpopis_trace *trace /* NULL: exactly mpopis_run_trials */);

/* ---- the one collective: summary records to rank 0 over RCCL/xGMI ---------------------
 * Trials shard over GPUs at trial granularity: trial k -> rank (k-1) mod G (`for k in 1:num_trials`,
 * src/examples/car_example.jl:170, has no cross-trial dependency), each rank runs its trials as one resident batch
 * (mpopis_seed_slots + mpopis_run_trials) and nothing is exchanged until the per-trial records
 * (src/examples/car_example.jl:144-155,287-302) are gathered for the AVE/STD/MED/... table (:328-410).
 *   mpopis_comm_unique_id : rank 0 creates the 128-byte RCCL id; the host distributes it (MPI / Distributed.jl / a file)
 *   mpopis_comm_init      : every rank, same id; binds an RCCL communicator to the handle's device and stream
 *                           (world == 1 with id == NULL: no RCCL is loaded, the gather is a copy;
 *                           world == 1 with an id: a real one-rank RCCL communicator)
 *   mpopis_gather_summary : every rank passes its n_local records (rows of MPOPIS_RECORD_LEN doubles); n_max = the largest
 *                           n_local over ranks (ceil(num_trials / world)).  Rank 0 receives out[world][n_max][RECORD_LEN]
 *                           and counts[world] (rows valid per rank); other ranks may pass NULL for both.
 *   mpopis_comm_count     : *ranks = what ncclCommCount reports for the handle's communicator, 0 when no RCCL communicator is bound
 *                           (lets a launcher prove the gather really spans its N ranks; replaces nothing in the reference, whose
 *                           trial loop is serial: src/examples/car_example.jl:170)
 * librccl is bound with dlopen at the first comm call; single-GPU users never load it. */
#define MPOPIS_COMM_ID_BYTES 128
int  mpopis_comm_unique_id(char *id128);
int  mpopis_comm_init(mpopis_handle *h, const char *id128, int32_t rank, int32_t world);
int  mpopis_gather_summary(mpopis_handle *h, const double *records, int32_t n_local, int32_t n_max,
                           double *out, int32_t *counts);
int  mpopis_comm_count(mpopis_handle *h, int32_t *ranks);
int  mpopis_comm_destroy(mpopis_handle *h);

/* Execution knob.  A handle can split its batch into parts that run as independent chains on their own HIP streams, so that
 * the latency-bound links of one chain (Cholesky, sort, alias table) and the tail of its rollout launch hide under another chain's
 * throughput kernels: 5-30 % of an MPC step for the adaptive policies from ~48 resident K = 4096 trials on, nothing below.
 * Default (on <= 0): the engine picks the measured optimum for the handle's shape (one stream for small batches and for :mppi / :gmppi).
 * on = 1: one stream (what a per-kernel profile wants); 2..4: that many parts.  (Until round 4 the default was one stream and on = 1
 * meant two halves.)  Results do not depend on it (bit-identical per slot). */
int  mpopis_set_overlap(mpopis_handle *h, int32_t on);

/* ---- measurement hooks (bench.py; HIP events on the engine's own stream) ----------------------- */
int  mpopis_timing_enable(mpopis_handle *h, int32_t on);   /* 0 off; 1 every kernel class; else a mask: bit (i + 1) = class i of
                                                              * mpopis_timing_read's name list (2 = "rollout" only: 2 events per launch) */
/* accumulated since enable/reset: per kernel class average launch duration.
 * names: semicolon separated list; ms_total[i], launches[i] for i < *n (in: capacity). */
int  mpopis_timing_read(mpopis_handle *h, char *names, int32_t names_cap, double *ms_total,
                        int64_t *launches, int32_t *n);
int  mpopis_timing_reset(mpopis_handle *h);

/* Synthetic-workload entry used by bench.py: run `steps` policy steps (device RNG, resident
 * state, env not advanced) back to back on the stream; returns wall ms measured with HIP events
 * around the whole region and the number of model rollouts executed. */
int  mpopis_bench_policy_steps(mpopis_handle *h, int32_t steps, double *ms, double *rollouts);

#ifdef __cplusplus
}
#endif
#endif
