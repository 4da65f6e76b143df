"""Part-chains that outlive an MPC step: a multi-step call (mpopis_bench_policy_steps, mpopis_run_trials) forks the parts once, lets every part run
step after step on its own stream and joins when the host needs the whole batch.  A slot's bits must not depend on that: the multi-step call on four
parts, separate single-step calls (fork and join per call) and the one-stream schedule give the same pol.U and Σ′, the closed loop the same records and
actions -- across the harness' eighth-step join, with a slot that ends its trial early (the `alive` gate then works on a part's own stream) and with
a CE loop that breaks early.  B = 8 (four parts of two slots) and B = 5 (uneven parts 2/1/1/1)."""
import numpy as np
import pytest

from tests.test_gpu_baseline_shapes import start_states

pytestmark = pytest.mark.gpu

K, T, N = 128, 10, 3


@pytest.fixture(scope="module")
def eng_mod():
    from mpopis_amd import build
    build.build()
    from mpopis_amd import engine
    return engine


def make(eng_mod, track, B, kind="musigmaaismppi", K=K, cov=(0.0625, 0.1), overlap=4, x0=None):
    eng = eng_mod.Engine("car", 1, kind, K, T, batch=B, lam=10.0, ais_its=N, lam_ais=20.0, elite_threshold=0.8, cov=list(cov), track=track, seed=777)
    eng.set_overlap(overlap)
    if x0 is not None:
        eng.set_state(x0)
    return eng


@pytest.mark.parametrize("B", [8, 5])
def test_multi_step_call_equals_single_step_calls(eng_mod, oracle, track, B):
    x0 = start_states(oracle, track, 1, B)                     # a different start state per slot: the slots' U and Σ′ differ
    outs = []
    for overlap, multi in ((4, True), (4, False), (1, True), (1, False)):
        eng = make(eng_mod, track, B, overlap=overlap, x0=x0)
        if multi:
            _, rollouts = eng.bench_policy_steps(3)
            assert rollouts == 3 * B * N * K
        else:
            for _ in range(3):
                eng.policy_step(None, minimal=True)
        outs.append((eng.get_U(), eng.get_Sigma()))
        eng.close()
    U0, S0 = outs[0]
    assert np.all(np.isfinite(U0)) and np.all(np.isfinite(S0))
    assert not np.array_equal(U0[0], U0[1]) and not np.array_equal(S0[0], S0[B - 1])
    for U, S in outs[1:]:
        assert np.array_equal(U, U0) and np.array_equal(S, S0)


@pytest.mark.parametrize("B", [8, 5])
def test_closed_loop_across_the_eighth_step_join(eng_mod, oracle, track, B):
    # (the later mid-lap start states sit beyond the lane's edge with this short-horizon controller: those trials end on `T_viol > 10`,
    #  car_example.jl:277-279, after eleven MPC steps -- between the two joins -- while the others run on)
    x0 = start_states(oracle, track, 1, B)
    outs = []
    for overlap in (4, 1):
        eng = make(eng_mod, track, B, overlap=overlap, x0=x0)
        rec, acts = eng.run_trials(num_steps=14, laps=2, log_actions=True)      # 15 MPC steps: the host looks at steps 7 and 14
        outs.append((rec, acts, eng.get_U(), eng.get_state()[0]))
        eng.close()
    rec, acts = outs[0][0], outs[0][1]
    assert np.all(rec[:, 15] == 0) and np.all(np.isfinite(rec))
    steps = rec[:, 1]
    print("\n[chains] B=%d steps per slot: %s" % (B, steps))
    early = np.where(steps < 14)[0]
    assert len(early) > 0 and np.all(rec[early, 12] > 10)      # some slots ended early, on track violations ...
    assert steps[0] == 14 and steps[1] == 14                   # ... others ran to the end, also in the first part
    for b in early:
        assert np.all(acts[b, int(steps[b]) + 1:] == 0)        # a frozen slot logs nothing more
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("B", [8, 5])
def test_nine_step_closed_loop(eng_mod, oracle, track, B):
    """num_steps = 9: one join inside the call (step 7) and the final one two steps later.  One slot starts at the lane's edge a few metres before the
    finish line and ends its trial on its first lap (ten steps are too few for the violation counters to end one): from then on its part's kernels
    skip it through the `alive` gate, on that part's own stream."""
    x0 = start_states(oracle, track, 1, B)
    x0[B - 1] = [6.5, -3.0, np.pi / 2, 10.0, 0.0, 0.0, 0.0, 0.0]
    outs = []
    for overlap in (4, 1):
        eng = make(eng_mod, track, B, overlap=overlap, x0=x0)
        outs.append(eng.run_trials(num_steps=9, laps=1, log_actions=True))
        eng.close()
    rec, acts = outs[0]
    print("\n[chains] nine steps, B=%d: steps per slot %s" % (B, rec[:, 1]))
    assert np.array_equal(rec, outs[1][0]) and np.array_equal(acts, outs[1][1])
    assert np.all(rec[:, 15] == 0)
    assert rec[B - 1, 1] < 9 and rec[B - 1, 3] > 0             # the slot before the line finished its lap early ...
    assert np.max(rec[:, 1]) == 9                              # ... while others ran all ten MPC steps
    assert np.all(acts[B - 1, int(rec[B - 1, 1]) + 1:] == 0)


@pytest.mark.parametrize("cov,breaks", [((1e-12, 1e-12), True), ((0.0625, 0.1), False)])
def test_early_break_per_slot(eng_mod, oracle, track, cov, breaks):
    """:cemppi leaves its loop when the elite costs agree to 1e-2 (:458-461): with a vanishing proposal every slot does so after its first iteration,
    on whatever stream its part runs; the executed iterations are the same per slot in every schedule"""
    B, Kc = 5, 150
    x0 = start_states(oracle, track, 1, B)
    iters, rolls, recs = [], [], []
    for overlap in (4, 1):
        eng = make(eng_mod, track, B, kind="cemppi", K=Kc, cov=cov, overlap=overlap, x0=x0)
        iters.append(np.stack([eng.policy_step(None, minimal=True)["iters_run"] for _ in range(2)]))
        rolls.append(eng.bench_policy_steps(3)[1])
        recs.append(eng.run_trials(num_steps=9, laps=2))
        eng.close()
    assert np.array_equal(iters[0], iters[1]) and rolls[0] == rolls[1] and np.array_equal(recs[0], recs[1])
    if breaks:
        assert np.all(iters[0] == 1) and rolls[0] < 3 * B * N * Kc
    else:
        assert np.all(iters[0] >= 1) and np.all(iters[0] <= N)
