"""Random request batches for the device SBMPC services (shipsim_sbmpc_eval, shipsim_sbmpc_eval_multi), their oracle
answers, and the perturbation family that decides whether a device answer off the oracle's is explained.

The SBMPC cost is discontinuous (dist < d_safe, the phi_o sectors) and its argmin takes the lowest scenario on an
exact tie, so a request that sits on such an edge can flip its answer under a libm ulp. Whether a batch holds such
requests is a property of the oracle alone: FAMILY moves own-ship x, own-ship y and the first obstacle's x, one at a
time, by the relative factors of gpu_harness.PERTURBATIONS and their negatives. tests/test_sbmpc_inputs_cpu.py asserts
that no answer of the GPU tests' batches changes under it (so the GPU tests may ask for exact equality); a device
answer that differs from the oracle's is explained only if some member of the family gives the oracle that answer."""
import functools

import numpy as np

import gpu_harness as H
import oracle_ffi as O
from ast_sac_amd import shipsim_abi as abi

FACTORS = tuple(sorted({s * p for p in H.PERTURBATIONS if p for s in (1.0, -1.0)}))
COLUMNS = (4, 5, 10)  # own-ship x, own-ship y, the first obstacle's x (the same columns in both services' rows)
FAMILY = tuple((c, f) for c in COLUMNS for f in FACTORS)


def random_requests(rng, n, K):
    """(n, SBMPC_MULTI_IN) requests with K obstacles: half of the obstacles on a collision course, sizes varied"""
    os_ = np.stack([rng.uniform(0, 20000, n), rng.uniform(0, 10000, n), rng.uniform(-np.pi, np.pi, n),
                    rng.uniform(0, 6, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.01, 0.01, n)], 1)
    u_d, chi_d = rng.uniform(3, 5, n), rng.uniform(-4, 4, n)
    slots = np.zeros((n, 7 * abi.MAX_OBS))
    for k in range(K):
        ang, rad = rng.uniform(-np.pi, np.pi, n), rng.uniform(20, 4000, n)
        ob = np.stack([os_[:, 0] + rad * np.cos(ang), os_[:, 1] + rad * np.sin(ang), rng.uniform(-np.pi, np.pi, n),
                       rng.uniform(0, 6, n), rng.uniform(-0.5, 0.5, n)], 1)
        ahead = rng.uniform(size=n) < 0.5  # on a collision course: ahead of the nominal course, heading back
        r2, ax = rng.uniform(300, 1900, n), chi_d + rng.uniform(-0.6, 0.6, n)
        ob[ahead] = np.stack([os_[:, 0] - r2 * np.sin(ax), os_[:, 1] + r2 * np.cos(ax),
                              chi_d + np.pi + rng.uniform(-0.5, 0.5, n), rng.uniform(2, 6, n),
                              rng.uniform(-0.3, 0.3, n)], 1)[ahead]
        slots[:, 7 * k:7 * k + 5] = ob
        slots[:, 7 * k + 5] = np.where(rng.uniform(size=n) < 0.3, rng.uniform(40, 140, n), 80.0)
        slots[:, 7 * k + 6] = np.where(rng.uniform(size=n) < 0.3, rng.uniform(8, 30, n), 16.0)
    last = np.stack([rng.choice([0.4, 0.6, 0.8, 1.0], n), np.deg2rad(rng.choice(np.arange(-30, 31, 10), n))], 1)
    return np.concatenate([last, u_d[:, None], chi_d[:, None], os_, slots], 1)


def random_single_requests(rng, n):
    """(n, SBMPC_IN) near-encounter requests of the single-obstacle service"""
    os_ = np.stack([rng.uniform(0, 20000, n), rng.uniform(0, 10000, n), rng.uniform(-np.pi, np.pi, n),
                    rng.uniform(0, 6, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.01, 0.01, n)], 1)
    ang, rad = rng.uniform(-np.pi, np.pi, n), rng.uniform(20, 2200, n)
    ob = np.stack([os_[:, 0] + rad * np.cos(ang), os_[:, 1] + rad * np.sin(ang), rng.uniform(-np.pi, np.pi, n),
                   rng.uniform(0, 6, n), rng.uniform(-0.5, 0.5, n)], 1)
    last = np.stack([rng.choice([0.4, 0.6, 0.8, 1.0], n), np.deg2rad(rng.choice(np.arange(-30, 31, 10), n))], 1)
    return np.concatenate([last, rng.uniform(3, 5, (n, 1)), rng.uniform(-4, 4, (n, 1)), os_, ob,
                           np.full((n, 1), 80.0), np.full((n, 1), 16.0)], 1)


def oracle_multi_one(r, K, tf=1000, dt=20):
    return O.sbmpc_multi(r[0], r[1], r[2], r[3], r[4:10], r[10:10 + 7 * K].reshape(K, 7), tf, dt)[0]


def oracle_single_one(r):
    return O.sbmpc(r[0], r[1], r[2], r[3], r[4:10], r[10:15], r[15], r[16])[0]


def oracle_multi(reqs, K, tf=1000, dt=20):
    return np.array([oracle_multi_one(r, K, tf, dt) for r in reqs])


# The batches of the GPU tests, by name: (requests, the oracle's answers, the oracle for one request). Made once per
# process and shared (read-only) by every test that needs them.
MULTI_SEED, MULTI_N = 100, 2048  # test_sbmpc_eval_multi_matches_oracle: PCG64(100 + K)
SINGLE_SEED, SINGLE_N = 5, 4096  # test_sbmpc_eval_matches_oracle
HORIZON_SEED, HORIZON_N, HORIZON_TF, HORIZON_DT = 200, 512, 600.0, 30.0  # the non-default horizon: PCG64(200 + K)


@functools.lru_cache(maxsize=None)
def multi_batch(K):
    req = random_requests(np.random.Generator(np.random.PCG64(MULTI_SEED + K)), MULTI_N, K)
    one = functools.partial(oracle_multi_one, K=K)
    ref = np.array([one(r) for r in req])
    for a in (req, ref):
        a.setflags(write=False)
    return req, ref, one


@functools.lru_cache(maxsize=None)
def single_batch():
    req = random_single_requests(np.random.Generator(np.random.PCG64(SINGLE_SEED)), SINGLE_N)
    ref = np.array([oracle_single_one(r) for r in req])
    for a in (req, ref):
        a.setflags(write=False)
    return req, ref, oracle_single_one


@functools.lru_cache(maxsize=None)
def horizon_batch(K):
    req = random_requests(np.random.Generator(np.random.PCG64(HORIZON_SEED + K)), HORIZON_N, K)
    one = functools.partial(oracle_multi_one, K=K, tf=HORIZON_TF, dt=HORIZON_DT)
    ref = np.array([one(r) for r in req])
    for a in (req, ref):
        a.setflags(write=False)
    return req, ref, one


def perturbed(r, col, factor):
    p = np.array(r, np.float64)
    p[col] *= 1 + factor
    return p


def oracle_answers_under_family(r, one):
    """the oracle's answers for request r under every member of FAMILY"""
    return [one(perturbed(r, c, f)) for c, f in FAMILY]


def explain(req, got, ref, one):
    """Rows where the device's answer `got` differs from the oracle's `ref`, split into those some member of FAMILY
    explains (a perturbed oracle call returns the device's answer) and those none does: (explained, unexplained)."""
    explained, unexplained = [], []
    for i in np.nonzero((np.asarray(got) != np.asarray(ref)).any(axis=1))[0]:
        hit = any(np.array_equal(a, got[i]) for a in oracle_answers_under_family(req[i], one))
        (explained if hit else unexplained).append(int(i))
    return explained, unexplained


def assert_no_unexplained(what, req, got, ref, one, cap):
    """Zero unexplained mismatches; the explained ones counted, printed, and at most `cap`. Returns their count."""
    explained, unexplained = explain(req, got, ref, one)
    print(f"\n[{what}] {len(req)} requests: {len(explained)} mismatches explained by a perturbed oracle call, "
          f"{len(unexplained)} unexplained")
    assert not unexplained, (what, unexplained[:5], [(req[i], got[i], ref[i]) for i in unexplained[:2]])
    assert len(explained) <= cap, (what, explained[:10])
    return len(explained)
