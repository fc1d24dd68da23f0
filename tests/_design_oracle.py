"""Oracle for the design of a batch of measurements (tests/test_design_host.py pins it against NumPy;
tests/test_gpu_design.py compares the device results with it).  The rows y come from the product's own
eval_over_all_parameters; on them the output-output covariance blocks are formed in long double, in two passes, as
tests/_interest_oracle.py forms its blocks, together with the conditioning sums the tolerances are stated in.  The
greedy recurrence of csrc/obe_design.hip is restated here in NumPy, and next to it the same quantities are computed
independently: the conditional variances through np.linalg.solve on K_AA + N_A, the information through slogdet.

Tolerances.  A block entry is held to the project's 1e-10 of its conditioning, |dX_c'c(p, x)| <= 1e-10 B_X + 1e-20
A_c(x) A_c'(p) (cross_tolerance).  The recurrence alone, on inputs as given, is held to 1e-10 of the sum of the
magnitudes of its terms: S_cc + sum_m L_m^2 for v, sum_m |log(g_m / nu_m) / 2|, floored at 1, for the information
(recurrence_tolerance).  End to end, against the direct solve on the oracle's own blocks, the block tolerances are
propagated to first order as _interest_oracle.gain_tolerance_end_to_end propagates them: with A = K_AA + N_A, k the
covariance of the picked rows with (c, x) and u = A^-1 k,
    v = S - k^T A^-1 k         dv   = dS - 2 u^T dk + u^T dA u      |dv|   <= tol_S + 2 |u|^T tol_k + |u|^T tol_A |u|
    info = log det(N^-1 A) / 2  dinfo = tr(A^-1 dA) / 2              |dinfo| <= sum |A^-1| tol_A / 2
plus the recurrence's own tolerance (end_to_end_tolerance)."""
import numpy as np

import _predictive_oracle as pred


def _kept(y, w):
    keep, wk = pred.kept(np.arange(y.shape[-1]), w)          # (the indices of the particles that count)
    return keep.astype(np.int64), wk.astype(np.longdouble)


def cross_blocks(y_pivots, y, w):
    """y_pivots (n_p, C, N), y (n_x, C, N), w (N,) -> dict of float64: X (n_p, C, C, n_x) with X[j, c', c, s] = sum w
    (y_c'(p_j) - m_c'(p_j)) (y_c(x_s) - m_c(x_s)) / W, B_X the same with absolute values, m (n_x, C), m_p (n_p, C),
    A (n_x, C) = sum w |y_c| / W, A_p (n_p, C).  Cleaned weights: NaN and negative weights are zero, and a particle
    of zero weight is left out whatever its y."""
    y_pivots, y = np.asarray(y_pivots, dtype=np.float64), np.asarray(y, dtype=np.float64)
    keep, wk = _kept(y, w)
    yp, yx = y_pivots[:, :, keep].astype(np.longdouble), y[:, :, keep].astype(np.longdouble)
    with np.errstate(invalid="ignore", over="ignore"):
        sw = wk.sum()
        m_p, m = (wk * yp).sum(axis=2) / sw, (wk * yx).sum(axis=2) / sw
        dp, dx = yp - m_p[:, :, None], yx - m[:, :, None]
        out = dict(X=np.einsum("n,jdn,scn->jdcs", wk, dp, dx) / sw,
                   B_X=np.einsum("n,jdn,scn->jdcs", wk, np.abs(dp), np.abs(dx)) / sw,
                   m=m, m_p=m_p, A=(wk * np.abs(yx)).sum(axis=2) / sw, A_p=(wk * np.abs(yp)).sum(axis=2) / sw)
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}


def cross_tolerance(b):
    """(n_p, C, C, n_x): 1e-10 B_X + 1e-20 A_c(x) A_c'(p)."""
    return 1e-10 * b["B_X"] + 1e-20 * np.einsum("jd,sc->jdcs", b["A_p"], b["A"])


class Cov:
    """The joint covariance of every (setting, channel) with every other over the rows y (n_x, C, N), formed a pivot's
    block at a time and kept: row(p) (C, C, n_x) = X_c'c(p, x) with its tolerance tol_row(p), S() (C, n_x) its
    diagonal X_cc(x, x) with tol_S()."""

    def __init__(self, y, w):
        self.y, self.w = np.asarray(y, dtype=np.float64), np.asarray(w, dtype=np.float64)
        self.n_x, self.n_c = self.y.shape[0], self.y.shape[1]
        self._rows = {}
        keep, wk = _kept(self.y, self.w)
        yx = self.y[:, :, keep].astype(np.longdouble)
        sw = wk.sum()
        d = yx - ((wk * yx).sum(axis=2) / sw)[:, :, None]
        a = (wk * np.abs(yx)).sum(axis=2) / sw
        self._S = np.asarray(((wk * d * d).sum(axis=2) / sw).T, dtype=np.float64)
        self._tol_S = 1e-10 * self._S + 1e-20 * np.asarray(a * a, dtype=np.float64).T

    def _block(self, p):
        p = int(p)
        if p not in self._rows:
            b = cross_blocks(self.y[p:p + 1], self.y, self.w)
            self._rows[p] = b["X"][0], cross_tolerance(b)[0]
        return self._rows[p]

    def row(self, p):
        return self._block(p)[0]

    def tol_row(self, p):
        return self._block(p)[1]

    def S(self):
        return self._S.copy()

    def tol_S(self):
        return self._tol_S.copy()

    def dense(self):
        """(n_x, C, n_x, C): K[p, c', x, c]."""
        return np.stack([np.transpose(self.row(p), (0, 2, 1)) for p in range(self.n_x)])


def _noise(nu, n_c, n_x):
    return np.array(np.broadcast_to(np.asarray(nu, dtype=np.float64).reshape(n_c, -1), (n_c, n_x)))


def utility(v, nu, cost):
    """U (n_x,) = [sum_c v_c / nu_c] / cost."""
    return np.sum(v / nu, axis=0) / cost


def first_finite_maximum(u, taken=None):
    """The first index of the largest finite entry that is not taken; -1 if there is none."""
    u = np.asarray(u, dtype=np.float64)
    ok = np.isfinite(u) if taken is None else np.isfinite(u) & ~np.asarray(taken, dtype=bool)
    if not np.any(ok):
        return -1
    return int(np.flatnonzero(ok & (u == np.max(u[ok])))[0])


def margin(u, taken=None):
    """The relative margin between the best and the second-best finite utility (inf with one candidate)."""
    u = np.asarray(u, dtype=np.float64)
    ok = np.isfinite(u) if taken is None else np.isfinite(u) & ~np.asarray(taken, dtype=bool)
    top = np.sort(u[ok])[::-1]
    return np.inf if top.size < 2 else float((top[0] - top[1]) / abs(top[0]))


def condition(state, cross, p, nu):
    """One obe_design_step on the pivot p: state = dict(v (C, n_x), L list of (C, n_x) rows, info, terms_v (C, n_x),
    terms_info), cross (C, C, n_x) = X_c'c(p, x).  The recurrence of csrc/obe_design.hip, restated."""
    n_c = cross.shape[0]
    for cp in range(n_c):
        a = cross[cp].copy()
        for row in state["L"]:
            a = a - row * row[cp, p]
        g = a[cp, p] + nu[cp, p]
        with np.errstate(invalid="ignore", divide="ignore"):
            g = g if g > 0.0 and np.isfinite(g) else np.nan
            row = a / np.sqrt(g)
            state["L"].append(row)
            state["v"] = state["v"] - row * row
            state["terms_v"] = state["terms_v"] + row * row
            state["info"] += 0.5 * np.log(g / nu[cp, p])
            state["terms_info"] += abs(0.5 * np.log(g / nu[cp, p]))
    return state


def start(S_diag):
    v = np.array(S_diag, dtype=np.float64)
    return dict(v=v, L=[], info=0.0, terms_v=np.abs(v), terms_info=0.0)


def recurrence_tolerance(state):
    """(tol_v (C, n_x), tol_info)."""
    return 1e-10 * state["terms_v"], 1e-10 * max(1.0, state["terms_info"])


def greedy(cov, nu, cost, n, distinct=False):
    """The design by the recurrence on the joint covariance (a Cov): dict(indices (n,), utility (n,) of each
    pick when it was made, information (n,) after each pick, margins (n,), U list of the (n_x,) utilities each pick was
    made from, v list of the (C, n_x) conditional variances each pick was made from, state)."""
    n_x, n_c = cov.n_x, cov.n_c
    nu = _noise(nu, n_c, n_x)
    state = start(cov.S())
    taken = np.zeros(n_x, dtype=bool)
    out = dict(indices=np.empty(n, dtype=np.int64), utility=np.empty(n), information=np.empty(n), margins=np.empty(n),
               U=[], v=[])
    for j in range(n):
        u = utility(state["v"], nu, cost)
        pick = first_finite_maximum(u, taken if distinct else None)
        out["U"].append(u)
        out["v"].append(state["v"].copy())
        out["indices"][j], out["utility"][j] = pick, u[pick] if pick >= 0 else np.nan
        out["margins"][j] = margin(u, taken if distinct else None)
        if pick < 0:
            break
        taken[pick] = True
        state = condition(state, cov.row(pick), pick, nu)
        out["information"][j] = state["info"]
    out["state"] = state
    return out


def direct(cov, nu, picks):
    """Independently of the recurrence: (v (C, n_x) conditioned on readings at the picks — a setting picked twice is
    two readings —, info = log det(I + N^-1/2 K_AA N^-1/2) / 2, cond(K_AA + N_A), A^-1, u (rows, C, n_x))."""
    n_x, n_c = cov.n_x, cov.n_c
    nu = _noise(nu, n_c, n_x)
    picks = [int(p) for p in picks]
    S = cov.S()
    if not picks:
        return S, 0.0, 1.0, np.zeros((0, 0)), np.zeros((0, n_c, n_x))
    rows = [(p, c) for p in picks for c in range(n_c)]
    k_aa = np.array([[cov.row(p)[c, d, q] for q, d in rows] for p, c in rows])
    noise = np.array([nu[c, p] for p, c in rows])
    a = k_aa + np.diag(noise)
    k = np.array([cov.row(p)[c] for p, c in rows])           # (rows, C, n_x)
    u = np.linalg.solve(a, k.reshape(len(rows), -1)).reshape(k.shape)
    v = S - np.einsum("rcs,rcs->cs", k, u)
    scaled = a / np.sqrt(np.outer(noise, noise))
    sign, logdet = np.linalg.slogdet(scaled)
    return v, 0.5 * logdet, float(np.linalg.cond(a)), np.linalg.inv(a), u


def end_to_end_tolerance(cov, nu, picks, state):
    """(tol_v (C, n_x), tol_info) of the device's design against direct() on the oracle's blocks: the block tolerances
    propagated to first order (module docstring) plus the recurrence's own."""
    picks = [int(p) for p in picks]
    tol_S = cov.tol_S()
    rec_v, rec_info = recurrence_tolerance(state)
    if not picks:
        return tol_S + rec_v, rec_info
    n_c = cov.n_c
    rows = [(p, c) for p in picks for c in range(n_c)]
    _, _, _, a_inv, u = direct(cov, nu, picks)
    tol_a = np.array([[cov.tol_row(p)[c, d, q] for q, d in rows] for p, c in rows])
    tol_k = np.array([cov.tol_row(p)[c] for p, c in rows])
    au = np.abs(u)
    tol_v = tol_S + 2.0 * np.einsum("rcs,rcs->cs", au, tol_k) + np.einsum("rcs,rq,qcs->cs", au, tol_a, au)
    return tol_v + rec_v, 0.5 * float(np.sum(np.abs(a_inv) * tol_a)) + rec_info
