"""NumPy restatement of NESMPPI_Policy's call (src/mppi_mpopi_policies.jl:855-893 + the G functor :221-238), the test reference of
:nesmppi.  The oracle has no NES; its :gmppi policy supplies simulate_model (:261-278) and pol.U / pol.Σ.

Per call, from U_orig = pol.U, Σ′ = pol.Σ, A′ = sqrt(pol.Σ) (:849, symmetric square root through eigh), for n = 1..N:
  L = chol(Σ′), E = L Z_n, Σ^-1 = L^-T L^-1                                  (:864-866, MvNormal / invcov)
  c = simulate_model(pol.U, E, Σ^-1, U_orig)                                  (:867)
  break if max |c_{k+1} - c_k| < 10e-3 (NaN never breaks)                     (:868-870)
  n < N:  G = Σ^-1 M Σ^-1 - C Σ^-1 with M = Σ c_k E_k E_k', C = Σ c_k -- the score-function sum Σ_k c_k (∇Σ_k + ∇Σ_k') of :872-874, whose
          halves and factor 2 cancel;  A′ -= (sf/K²) A′ G;  Σ′ = A′'A′;  pol.U -= (sf/K) Σ^-1 g with g = Σ c_k E_k      (:875-878)
then E += pol.U - U_orig, pol.U = U_orig, w = compute_weights(λ, c), the weighted controls, the clamp and the roll (src/utils.jl:88-101:
U[1:end-as] = wc[as+1:end]; the tail keeps its value because pol.U aliases params.U₀ there).
"""
import numpy as np


def sym_sqrt(S):
    lam, V = np.linalg.eigh(S)
    return (V * np.sqrt(lam)) @ V.T


def inv_from_chol(L):
    Li = np.linalg.inv(L)
    return Li.T @ Li


def nes_gradients(E, c, Sinv):
    """(G, Σ^-1 g) in the closed form above."""
    g = E @ c
    M = (E * c) @ E.T
    G = Sinv @ M @ Sinv - c.sum() * Sinv
    return G, Sinv @ g


def nes_ref(pol, env, Z, opt_its, step_factor, lam, gamma=0.0, A0=None, lo=-1.0, hi=1.0):
    """pol: oracle.OraclePolicy("gmppi", env, K, T, ...) holding pol.U and pol.Σ (rolled in place like the engine's).
    Z: (N', K, cs) standard normals, row k = sample k (N' >= opt_its).  Returns dict(control, cost, weights, E (cs x K), iters_run,
    Sigma_last, U)."""
    K, cs, as_ = pol.K, pol.cs, pol.as_
    Sigma = pol.Sigma
    U_orig = pol.U.copy()
    U = U_orig.copy()
    Sp = Sigma.copy()
    Ap = sym_sqrt(Sigma) if A0 is None else A0.copy()
    iters = 0
    for n in range(opt_its):
        L = np.linalg.cholesky(Sp)
        E = L @ np.asarray(Z[n], dtype=np.float64).T
        Sinv = inv_from_chol(L)
        cost = pol.simulate_model(U, E, Sinv if gamma != 0.0 else None, U_orig)
        Slast, iters = Sp, n + 1
        if np.max(np.abs(np.diff(cost))) < 10e-3:
            break
        if n < opt_its - 1:
            G, Sg = nes_gradients(E, cost, Sinv)
            Ap = Ap - step_factor / K * (Ap @ G) / K
            Sp = Ap.T @ Ap
            Sp = 0.5 * (Sp + Sp.T)
            U = U - step_factor / K * Sg
    E = E + (U - U_orig)[:, None]
    rho = np.min(cost)
    w = np.exp(-1.0 / lam * (cost - rho))
    w = w / w.sum()
    wc = U_orig + E @ w
    control = np.clip(wc[:as_], lo, hi)
    Unew = U_orig.copy()
    if cs > as_:
        Unew[:cs - as_] = wc[as_:]
    else:
        Unew = wc
    pol.U = Unew
    return dict(control=control, cost=cost, weights=w, E=E, iters_run=iters, Sigma_last=Slast, Sinv_last=Sinv, U=Unew)
