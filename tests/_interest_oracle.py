"""Oracle for the design for parameters of interest (tests/test_interest_host.py pins it against NumPy;
tests/test_gpu_interest.py compares the device results with it).  The rows y come from the product's own
eval_over_all_parameters; on them and on the cloud's rows the blocks are formed in long double, in two passes, as
tests/_predictive_oracle.py forms its moments, together with the conditioning sums the tolerances are stated in."""
import numpy as np

import _predictive_oracle as pred


def blocks(y, theta, w):
    """y (C, N), theta (R, N), w (N,) -> dict of float64: m (C,), t (R,), V (R,), S (C, C), K (R, C) and the
    conditioning sums B_S (C, C) = sum w |dy_c| |dy_c'| / W, B_K (R, C) = sum w |dtheta_d| |dy_c| / W,
    A_c (C,) = sum w |y_c| / W, A_d (R,) = sum w |theta_d| / W.  Cleaned weights: NaN and negative weights are zero,
    and a particle of zero weight is left out whatever its y or theta."""
    y, theta = np.atleast_2d(np.asarray(y, dtype=np.float64)), np.atleast_2d(np.asarray(theta, dtype=np.float64))
    keep, wk = pred.kept(np.arange(y.shape[1]), w)           # (the indices of the particles that count)
    keep = keep.astype(np.int64)
    y, theta, wk = y[:, keep].astype(np.longdouble), theta[:, keep].astype(np.longdouble), wk.astype(np.longdouble)
    with np.errstate(invalid="ignore", over="ignore"):
        sw = wk.sum()
        m = (wk * y).sum(axis=1) / sw
        t = (wk * theta).sum(axis=1) / sw
        dy, dt = y - m[:, None], theta - t[:, None]
        out = dict(m=m, t=t, V=(wk * dt * dt).sum(axis=1) / sw,
                   S=np.einsum("n,cn,dn->cd", wk, dy, dy) / sw, K=np.einsum("n,rn,cn->rc", wk, dt, dy) / sw,
                   B_S=np.einsum("n,cn,dn->cd", wk, np.abs(dy), np.abs(dy)) / sw,
                   B_K=np.einsum("n,rn,cn->rc", wk, np.abs(dt), np.abs(dy)) / sw,
                   A_c=(wk * np.abs(y)).sum(axis=1) / sw, A_d=(wk * np.abs(theta)).sum(axis=1) / sw)
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}


def tolerances(b):
    """(tol_S (C, C), tol_K (R, C), tol_V (R,)): the project's 1e-10 on the conditioning of each sum, with
    _predictive_oracle.var_tolerance's floor for exactly degenerate clouds."""
    return (1e-10 * b["B_S"] + 1e-20 * np.outer(b["A_c"], b["A_c"]),
            1e-10 * b["B_K"] + 1e-20 * np.outer(b["A_d"], b["A_c"]),
            1e-10 * b["V"] + 1e-20 * b["A_d"] ** 2)


def gain(S, K, nu):
    """(G (R,), u (R, C), cond): G_d = k_d^T (S + diag nu)^-1 k_d by np.linalg.solve, u_d the solution, cond the
    2-norm condition number of S + diag nu.  S (C, C), K (R, C), nu (C,)."""
    a = np.asarray(S, dtype=np.float64) + np.diag(np.asarray(nu, dtype=np.float64).reshape(-1))
    u = np.linalg.solve(a, np.asarray(K, dtype=np.float64).T).T
    return np.einsum("rc,rc->r", K, u), u, float(np.linalg.cond(a))


def gain_tolerance(K, u):
    """|dG_d| <= 1e-10 sum_c |u_c| |k_c| on the blocks as given."""
    return 1e-10 * np.einsum("rc,rc->r", np.abs(u), np.abs(K))


def gain_tolerance_end_to_end(K, u, tol_S, tol_K, nu):
    """... and against blocks that are themselves within (tol_S, tol_K): G(k + dk, S + dS) - G(k, S) = 2 u . dk -
    u^T dS u to first order.  Where the reference row k_d is itself within tol_K of zero (a cloud of one particle: every
    theta - t and y - m is zero up to the rounding of the means) u_d is as small and the first order says nothing;
    there, and only there, the term of second order in dk, dk^T (S + diag nu)^-1 dk <= |dk|^2 / min nu, is as large
    and is added."""
    K = np.asarray(K, dtype=np.float64)
    first = 2.0 * np.einsum("rc,rc->r", np.abs(u), tol_K) + np.einsum("rc,cd,rd->r", np.abs(u), tol_S, np.abs(u))
    second = np.where(np.all(np.abs(K) <= tol_K, axis=1), np.sum(tol_K ** 2, axis=1) / np.min(nu), 0.0)
    return first + second + gain_tolerance(K, u)


def utility(G, V, a, cost):
    """U = [sum_d a_d G_d / V_d] / cost, a term with V_d == 0 being 0.  G (R, n_x), V (R,), a (R,), cost scalar or
    (n_x,)."""
    G, V, a = np.asarray(G, dtype=np.float64), np.asarray(V, dtype=np.float64), np.asarray(a, dtype=np.float64)
    total = np.zeros(G.shape[1])
    for d in range(G.shape[0]):
        if V[d] != 0.0:
            total = total + a[d] * G[d] / V[d]
    return total / cost
