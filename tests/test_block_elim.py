"""Block-restricted elimination of the n <= 64 IPM (k_ipm64.hpp): the factorisation updates only the 16-column chunks
at and right of the pivot's, and the solves are a four-block substitution. The code branches on where n and the pivots
fall relative to the 16 / 32 / 48 column boundaries and on the n > 60 padding path, so every such condensed size runs
here, on small batches, through both fp64 paths (fused k_solve64 and condense + stand-alone k_ipm64), against the CPU
oracle at the project's fp64 bar (test_gpu_parity.py), and fused against unfused bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20221125
B = 4
# (horizon, condensed size n = 3 * stance legs over the horizon)
SIZES = [(1, 3), (1, 12),
         (5, 15), (5, 18), (5, 48), (5, 51), (5, 60),
         (10, 30), (10, 33), (10, 45), (10, 48), (10, 51), (10, 57), (10, 60), (10, 63)]


def rel_err(u, ur):
    return float(np.max(np.abs(u - ur)) / max(1.0, float(np.max(np.abs(ur)))))


def contacts(N, n, batch=B):
    """Random contact tables with exactly n / 3 stance legs: one random stance leg per step (a step without one is
    CMPC_INVALID_CONTACT), then random extra ones."""
    assert n % 3 == 0 and N <= n // 3 <= 4 * N
    rng = np.random.default_rng(1000 * N + n)
    c = np.zeros((batch, N, 4), dtype=np.uint8)
    for b in range(batch):
        for k in range(N):
            c[b, k, rng.integers(4)] = 1
        free = np.flatnonzero(c[b].reshape(-1) == 0)
        extra = rng.choice(free, size=n // 3 - N, replace=False)
        c[b].reshape(-1)[extra] = 1
        assert int(c[b].sum()) == n // 3
    return c


_CASES = {}


def case(op, N, n):
    """Inputs of one size (generate(seed, gait 0) with the contact table replaced) and the oracle's cold solve;
    computed once and shared, never modified."""
    key = (N, n)
    if key not in _CASES:
        mo = op.default_model(N)
        x0, xref, foot, _ = op.generate(mo, SEED, B, gait=0)
        contact = contacts(N, n)
        ur, _, sr, itr = op.solve_batch(mo, op.default_settings(), x0, xref, foot, contact, nthreads=4, want_x=False)
        for a in (x0, xref, foot, contact, ur, sr, itr):
            a.setflags(write=False)
        _CASES[key] = (x0, xref, foot, contact, ur, sr, itr)
    return _CASES[key]


@pytest.mark.parametrize("N,n", SIZES)
def test_fp64_both_paths_match_oracle(cm, op, N, n):
    x0, xref, foot, contact, ur, sr, itr = case(op, N, n)
    assert np.all(sr == 0), sr
    m = cm.default_model(N)
    out = []
    for path in (None, {cm.PATH_FUSED64: 0}):
        eng = cm.Engine(m, precision=0, max_batch=B) if path is None else \
            cm.Engine(m, precision=0, max_batch=B, path=path)
        u, _, st, it = eng.solve(x0, xref, foot, contact, want_x=False)
        err = max(rel_err(u[q], ur[q]) for q in range(B))
        print(f"N={N} n={n} path={'fused' if path is None else 'unfused'} status={st.tolist()} iters={it.tolist()} "
              f"oracle iters={itr.tolist()} rel_err={err:.3e}")
        assert np.array_equal(st, sr), (st, sr)
        assert err < 1e-8, err
        assert np.all(u[contact == 0] == 0.0)  # swing legs exactly zero
        out.append((u, st, it))
    (uf, sf, itf), (uu, su, itu) = out
    assert np.array_equal(uf.view(np.uint8), uu.view(np.uint8)), "fused and unfused u differ"
    assert np.array_equal(sf, su) and np.array_equal(itf, itu)


def test_fp32_chunk_boundaries(cm, op):
    """fp32 at n = 48, 60, 63 (N = 10), at the tolerance of test_gpu_parity.py::test_solve_fp32_n20."""
    N = 10
    m, mo = cm.default_model(N), op.default_model(N)
    s = cm.default_settings(tol_stat=1e-3, tol_ineq=1e-3, tol_comp=1e-4)  # fp32: ulp(5000 N bound) = 4.9e-4
    eng = cm.Engine(m, settings=s, precision=1, max_batch=B)
    for n in (48, 60, 63):
        x0, xref, foot, contact = case(op, N, n)[:4]
        ur, _, sr, _ = op.solve_batch(mo, op.tight_settings(), x0, xref, foot, contact, nthreads=4, want_x=False)
        u, _, st, it = eng.solve(x0, xref, foot, contact, want_x=False)
        err = max(rel_err(u[q], ur[q]) for q in range(B))
        print(f"fp32 n={n} status={st.tolist()} iters={it.tolist()} rel_err={err:.3e}")
        assert np.all(sr == 0)
        assert np.all(st == 0), st
        assert err < 2e-3, err
        assert np.all(u[contact == 0] == 0.0)


def test_warm_start_n51(cm, op):
    """cmpc_solve_batch_warm (Engine.solve with u_init under warm_start = 1, as test_warm_start.py) at n = 51."""
    N, n = 10, 51
    m, mo = cm.default_model(N), op.default_model(N)
    x0, xref, foot, contact, u, sr, _ = case(op, N, n)
    assert np.all(sr == 0)
    rng = np.random.default_rng(2)
    guess = u * (1.0 + 0.05 * rng.standard_normal(u.shape)) + 0.5 * rng.standard_normal(u.shape)
    ws = op.default_settings(warm_start=1)
    ur, _, srw, itr = op.solve_batch(mo, ws, x0, xref, foot, contact, nthreads=4, want_x=False, u_init=guess)
    eng = cm.Engine(m, settings=cm.default_settings(warm_start=1), precision=0, max_batch=B)
    ud, _, sd, itd = eng.solve(x0, xref, foot, contact, want_x=False, u_init=guess)
    err = max(rel_err(ud[q], ur[q]) for q in range(B))
    print(f"warm n={n} status={sd.tolist()} iters={itd.tolist()} oracle iters={itr.tolist()} rel_err={err:.3e}")
    assert np.all(srw == 0)
    assert np.array_equal(sd, srw), (sd, srw)
    assert err < 1e-8, err
