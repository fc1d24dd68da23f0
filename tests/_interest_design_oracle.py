"""Oracle for the design of a batch of measurements for parameters of interest (tests/test_interest_design_host.py pins
it against its own independent direct solve; tests/test_gpu_interest_design.py compares the device results with it).
The rows y come from the product's own eval_over_all_parameters; on them and on the cloud's rows the blocks are formed in
long double by tests/_design_oracle.py (X, the output with the output) and tests/_interest_oracle.py (S, K, V).  The
recurrence of obe_design_interest_step (csrc/obe_design.hip) is restated here in NumPy, with K left unconditioned in the
T rows as include/obe_hip.h writes it:
    a(c, x)   = X_c'c(p, x) - sum_{m' < m} L_m'(c, x) L_m'(c', p)        g = a(c', p) + nu_c'(p)
    L_m(c, x) = a(c, x) / sqrt(g)      b(d) = K_dc'(p) - sum_{m' < m} T_m'(d) L_m'(c', p)      T_m(d) = b(d) / sqrt(g)
    S_cc''(x) -= L_m(c, x) L_m(c'', x)      K_dc(x) -= T_m(d) L_m(c, x)      Vleft_d -= T_m(d)^2
and next to it the same quantities are computed independently through np.linalg.solve on K_AA + N_A (direct,
direct_gain).

Tolerances, by the project's conventions.  The recurrence alone, on inputs as given, is held to 1e-10 of the sum of the
magnitudes of the terms of each quantity (recurrence_tolerance): |S| + sum_m |L_m L_m| for S, |K| + sum_m |T_m| |L_m| for
K, V + sum_m T_m^2 for Vleft, (|K_dc'(p)| + sum_m' |T_m'| |L_m'(c', p)|) / sqrt(g) for T_m.  A gain formed from such S
and K is held to _interest_oracle.gain_tolerance_end_to_end with those tolerances in the place of the blocks'
(gain_tolerance_of_state).  End to end, against the direct solve on the oracle's own blocks, the block tolerances are
propagated to first order as _design_oracle.end_to_end_tolerance propagates them: with A = K_AA + N_A, k_d the covariance
of the picked rows with theta_d and u_d = A^-1 k_d,
    Vleft_d = V_d - k_d^T A^-1 k_d      dVleft_d = dV_d - 2 u_d^T dk_d + u_d^T dA u_d
    |dVleft_d| <= tol_V + 2 |u_d|^T tol_k + |u_d|^T tol_A |u_d|
plus the recurrence's own tolerance (end_to_end_tolerance)."""
import numpy as np

import _design_oracle as des
import _interest_oracle as ioracle
from _design_oracle import Cov, cross_blocks, first_finite_maximum, margin     # noqa: F401  (the tests reach them here)
from _interest_oracle import blocks, gain, utility                              # noqa: F401


class Joint:
    """The joint covariance of (theta_D, every y_c(x)) over the rows y (n_x, C, N) and theta (R, N): cov, a
    _design_oracle.Cov (the output with the output), S (C, C, n_x), K (R, C, n_x), V (R,) and their tolerances."""

    def __init__(self, y, theta, w):
        y = np.asarray(y, dtype=np.float64)
        self.cov = Cov(y, w)
        self.n_x, self.n_c = self.cov.n_x, self.cov.n_c
        bs = [blocks(y[s], theta, w) for s in range(self.n_x)]
        tols = [ioracle.tolerances(b) for b in bs]
        self.S, self.K = np.stack([b["S"] for b in bs], axis=-1), np.stack([b["K"] for b in bs], axis=-1)
        self.tol_S, self.tol_K = np.stack([t[0] for t in tols], axis=-1), np.stack([t[1] for t in tols], axis=-1)
        self.V, self.tol_V = bs[0]["V"], tols[0][2]
        self.n_sel = self.V.shape[0]


def start(S, K, V):
    """The state before any pick: S (C, C, n_x), K (R, C, n_x), V (R,)."""
    S, K, V = (np.array(a, dtype=np.float64) for a in (S, K, V))
    return dict(S=S, K=K, K0=K.copy(), left=V.copy(), L=[], T=[], terms_S=np.abs(S), terms_K=np.abs(K),
                terms_left=np.abs(V), terms_T=[])


def condition(state, cross, p, nu):
    """One obe_design_interest_step on the pivot p: cross (C, C, n_x) = X_c'c(p, x), nu (C, n_x)."""
    n_c = cross.shape[0]
    for cp in range(n_c):
        a = cross[cp].copy()
        for row in state["L"]:
            a = a - row * row[cp, p]
        g = a[cp, p] + nu[cp, p]
        with np.errstate(invalid="ignore", divide="ignore"):
            g = g if g > 0.0 and np.isfinite(g) else np.nan
            row = a / np.sqrt(g)
            b, terms_b = state["K0"][:, cp, p].copy(), np.abs(state["K0"][:, cp, p])
            for t, earlier in zip(state["T"], state["L"]):
                b = b - t * earlier[cp, p]
                terms_b = terms_b + np.abs(t * earlier[cp, p])
            t = b / np.sqrt(g)
            state["L"].append(row)
            state["T"].append(t)
            state["terms_T"].append(terms_b / np.sqrt(g))
            state["S"] = state["S"] - row[:, None, :] * row[None, :, :]
            state["terms_S"] = state["terms_S"] + np.abs(row[:, None, :] * row[None, :, :])
            state["K"] = state["K"] - t[:, None, None] * row[None, :, :]
            state["terms_K"] = state["terms_K"] + np.abs(t[:, None, None] * row[None, :, :])
            state["left"] = state["left"] - t * t
            state["terms_left"] = state["terms_left"] + t * t
    return state


def recurrence_tolerance(state):
    """(tol_S (C, C, n_x), tol_K (R, C, n_x), tol_left (R,), tol_T list of (R,))."""
    return (1e-10 * state["terms_S"], 1e-10 * state["terms_K"], 1e-10 * state["terms_left"],
            [1e-10 * t for t in state["terms_T"]])


def gains(S, K, nu):
    """(G (R, n_x), u (R, C, n_x), the largest cond(S + diag nu)) by _interest_oracle.gain, a setting at a time; NaN
    where S + diag nu is not finite."""
    n_sel, n_c, n_x = K.shape
    G, u, worst = np.full((n_sel, n_x), np.nan), np.full((n_sel, n_c, n_x), np.nan), 1.0
    for s in range(n_x):
        if np.all(np.isfinite(S[:, :, s])) and np.all(np.isfinite(K[:, :, s])):
            G[:, s], u[:, :, s], cond = gain(S[:, :, s], K[:, :, s], nu[:, s])
            worst = max(worst, cond)
    return G, u, worst


def gain_tolerance_of_state(state, nu):
    """(R, n_x): the tolerance of a gain formed from S and K that are within recurrence_tolerance of the state's."""
    tol_S, tol_K = recurrence_tolerance(state)[:2]
    _, u, _ = gains(state["S"], state["K"], nu)
    out = np.full(state["K"][:, 0].shape, np.nan)
    for s in range(out.shape[1]):
        if np.all(np.isfinite(u[:, :, s])):
            out[:, s] = ioracle.gain_tolerance_end_to_end(state["K"][:, :, s], u[:, :, s], tol_S[:, :, s], tol_K[:, :, s],
                                                         nu[:, s])
    return out


def greedy(joint, nu, a, cost, n, distinct=False):
    """The design by the recurrence on a Joint: dict(indices (n,), utility (n,) of each pick when it was made, margins
    (n,), U and G lists of the (n_x,) utilities and (R, n_x) gains each pick was made from, variance_left (n, R) by the
    gain route (V minus the gains at the picks), left_T list of Vleft by the T route before each pick, state after
    conditioning on the first n - 1 picks, states list of the terms each pick's tolerance needs)."""
    n_x, n_c = joint.n_x, joint.n_c
    nu = des._noise(nu, n_c, n_x)
    state = start(joint.S, joint.K, joint.V)
    taken = np.zeros(n_x, dtype=bool)
    out = dict(indices=np.full(n, -1, dtype=np.int64), utility=np.full(n, np.nan), margins=np.full(n, np.nan),
               variance_left=np.full((n, joint.n_sel), np.nan), U=[], G=[], left_T=[], tol_G=[])
    left = joint.V.copy()
    for j in range(n):
        if j:
            state = condition(state, joint.cov.row(pick), pick, nu)
        G, _, _ = gains(state["S"], state["K"], nu)
        u = utility(G, joint.V, a, cost)
        pick = first_finite_maximum(u, taken if distinct else None)
        out["U"].append(u)
        out["G"].append(G)
        out["left_T"].append(state["left"].copy())
        out["tol_G"].append(gain_tolerance_of_state(state, nu))
        out["margins"][j] = margin(u, taken if distinct else None)
        if pick < 0:
            break
        out["indices"][j], out["utility"][j] = pick, u[pick]
        left = left - G[:, pick]
        out["variance_left"][j] = left
        taken[pick] = True
    out["state"] = state
    return out


def direct(joint, nu, picks):
    """Independently of the recurrence: (Vleft (R,) after readings at the picks — a setting picked twice is two readings
    —, cond(K_AA + N_A), A^-1, u (rows, R))."""
    n_x, n_c = joint.n_x, joint.n_c
    nu = des._noise(nu, n_c, n_x)
    picks = [int(p) for p in picks]
    if not picks:
        return joint.V.copy(), 1.0, np.zeros((0, 0)), np.zeros((0, joint.n_sel))
    rows = [(p, c) for p in picks for c in range(n_c)]
    k_aa = np.array([[joint.cov.row(p)[c, d, q] for q, d in rows] for p, c in rows])
    a = k_aa + np.diag([nu[c, p] for p, c in rows])
    k = np.array([joint.K[:, c, p] for p, c in rows])                          # (rows, R)
    u = np.linalg.solve(a, k)
    return joint.V - np.einsum("rd,rd->d", k, u), float(np.linalg.cond(a)), np.linalg.inv(a), u


def direct_gain(joint, nu, picks, x):
    """G_d(x | A) of the joint Gaussian, without S or K conditioned: what one more reading at x removes of Vleft."""
    return direct(joint, nu, picks)[0] - direct(joint, nu, list(picks) + [int(x)])[0]


def end_to_end_tolerance(joint, nu, picks, terms_left):
    """(R,): the tolerance of the device's Vleft after the picks against direct() on the oracle's blocks — the block
    tolerances propagated to first order (module docstring) plus the recurrence's own, 1e-10 terms_left."""
    picks = [int(p) for p in picks]
    rec = 1e-10 * np.asarray(terms_left, dtype=np.float64)
    if not picks:
        return joint.tol_V + rec
    rows = [(p, c) for p in picks for c in range(joint.n_c)]
    u = np.abs(direct(joint, nu, picks)[3])
    tol_a = np.array([[joint.cov.tol_row(p)[c, d, q] for q, d in rows] for p, c in rows])
    tol_k = np.array([joint.tol_K[:, c, p] for p, c in rows])
    return joint.tol_V + 2.0 * np.einsum("rd,rd->d", u, tol_k) + np.einsum("rd,rq,qd->d", u, tol_a, u) + rec


def utility_tolerance(tol_G, G, V, tol_V, a, cost):
    """The tolerance of U = [sum_d a_d G_d / V_d] / cost at one setting from those of G (R,) and V (R,), to first
    order: sum_d a_d (tol_G_d + G_d tol_V_d / V_d) / V_d / cost."""
    total = 0.0
    for d in range(len(V)):
        if V[d] != 0.0:
            total = total + a[d] * (tol_G[d] + abs(G[d]) * tol_V[d] / V[d]) / V[d]
    return total / cost
