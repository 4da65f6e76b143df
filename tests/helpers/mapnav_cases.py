"""Inputs of the tests that compare the device with tests/helpers/mapnav_ref.py, by name, so that the CPU suite can check the condition those
comparisons stand on -- no looked-up position within mapnav_ref.MARGIN of a cell edge -- for exactly the seeds the GPU suite uses
(tests/test_custom_env_table_cpu.py::test_seeds_of_the_gpu_tests_keep_clear_of_cell_edges)."""
import numpy as np

from tests.helpers import mapnav_ref as MN

# name -> (P, G, padding doubles): 3 doubles; 4096 = the last size the LDS kernel stages; the same content + 1 = the first global size; 20 000
TABLES = {"p1g1": (1, 1, 0), "g64": (0, 64, 0), "g64pad": (0, 64, 1), "p5000g100": (5000, 100, 0)}
TABLE_SIZES = {"p1g1": 3, "g64": 4096, "g64pad": 4097, "p5000g100": 20000}
LEVEL1_K = [1, 64, 255, 256, 257, 600]
LEVEL1_B, LEVEL1_T = 2, 11


def level1_seed(table, K):
    """one seed per (table content, K), checked on the reference alone by the CPU test named above; "g64pad" shares "g64"'s, so that the
    LDS kernel and the global one see the same numbers"""
    content = "g64" if table == "g64pad" else table
    return 1000 * (sorted(TABLES).index(content) + 1) + K


def level1_case(table, K):
    """-> dict(p, tab, x0 (B, 4), U (B, cs), E (B, K, cs)): noise with an eighth of the samples far out, and slot 1 starting at the map's
    corner on its way out, so that the clamp of the cell index is hit in every case"""
    P, G, pad = TABLES[table]
    rng = np.random.default_rng(level1_seed(table, K))
    B, T = LEVEL1_B, LEVEL1_T
    cs = MN.AS * T
    tab = MN.make_table(P, G, rng, pad)
    assert tab.size == TABLE_SIZES[table]
    x0 = np.concatenate([rng.uniform(-0.8, 0.8, (B, 2)), rng.uniform(-0.3, 0.3, (B, 2))], axis=1)
    x0[1] = [0.93, -0.91, 0.6, -0.7]
    U = rng.uniform(-0.3, 0.3, (B, cs))
    E = rng.standard_normal((B, K, cs)) * 0.6
    E[:, :max(1, K // 8)] *= 8.0
    return dict(p=MN.params(P, G), tab=tab, x0=x0, U=U, E=E)


def level1_reference(case):
    """-> (cost (B, K), trajectories (B, K, T, 4), edge margin, positions outside the map)"""
    B = case["x0"].shape[0]
    out = [MN.rollout_costs(case["x0"][b], case["U"][b], case["E"][b], case["p"], case["tab"]) for b in range(B)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), min(o[2] for o in out), sum(o[3] for o in out))


EMPTY_SEED = 77


def empty_table_case():
    """a table env before any table is set: P = 0 and G = 0 (no path term, a map that is 0 everywhere: mapnav.hip defines both)"""
    rng = np.random.default_rng(EMPTY_SEED)
    B, K, T = 2, 100, 7
    cs = MN.AS * T
    x0 = np.concatenate([rng.uniform(-0.8, 0.8, (B, 2)), rng.uniform(-0.3, 0.3, (B, 2))], axis=1)
    return dict(p=MN.params(0, 0), tab=np.zeros(0), x0=x0, U=rng.uniform(-0.3, 0.3, (B, cs)), E=rng.standard_normal((B, K, cs)) * 0.6)


MIRROR_SEED = 5
MIRROR_X0 = np.array([0.21, -0.33, 0.15, 0.1])


def mirror_case():
    """the Python mirror: P = 6 waypoints, an 8 x 8 map"""
    rng = np.random.default_rng(MIRROR_SEED)
    return dict(p=MN.params(6, 8), tab=MN.make_table(6, 8, rng))
