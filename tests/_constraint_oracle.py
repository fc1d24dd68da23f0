"""NumPy oracle of the declarative parameter bounds (set_parameter_bounds): the reference's semantics — zero the
violators' weights, divide by the new sum only if anything was zeroed (obe_noiseparam.py:65-79) — for a box per row."""
import numpy as np


def violators(particles, lower, upper, lower_open, upper_open):
    """bool (N,): the particle is outside the bounds on some row.  An inclusive end is violated by ``v < lower`` /
    ``v > upper``, an exclusive one by ``v <= lower`` / ``v >= upper``; every comparison is False for NaN."""
    particles = np.asarray(particles, dtype=np.float64)
    bad = np.zeros(particles.shape[1], dtype=bool)
    with np.errstate(invalid="ignore"):
        for r, row in enumerate(particles):
            bad |= (row <= lower[r]) if lower_open[r] else (row < lower[r])
            bad |= (row >= upper[r]) if upper_open[r] else (row > upper[r])
    return bad


def apply_bounds(particles, weights, lower, upper, lower_open, upper_open):
    """``(weights after the constraint, number of particles zeroed)``; 0 / 0 = NaN if every particle violates."""
    bad = violators(particles, lower, upper, lower_open, upper_open)
    w = np.array(weights, dtype=np.float64)
    count = int(np.count_nonzero(bad))
    if count:
        w[bad] = 0
        with np.errstate(invalid="ignore", divide="ignore"):
            w = w / np.sum(w)
    return w, count


def full(n_dims, bounds, lower_open=(), upper_open=()):
    """Arrays of n_dims from {row: (lower, upper)} (None = absent) and the rows whose ends are exclusive."""
    lower, upper = np.full(n_dims, -np.inf), np.full(n_dims, np.inf)
    for r, (lo, hi) in bounds.items():
        lower[r] = -np.inf if lo is None else lo
        upper[r] = np.inf if hi is None else hi
    lo_open, hi_open = np.zeros(n_dims, dtype=bool), np.zeros(n_dims, dtype=bool)
    lo_open[list(lower_open)] = True
    hi_open[list(upper_open)] = True
    return lower, upper, lo_open, hi_open


def install_hook(oracle_obj, lower, upper, lower_open, upper_open, counts=None):
    """Give an oracle object (oracle.OracleOptBayesExpt*) the bounds as the NumPy hook a user of the reference
    would write; ``counts`` (a list) receives the number of particles each call zeroed."""
    def enforce_parameter_constraints():
        w, n = apply_bounds(np.asarray(oracle_obj.parameters), oracle_obj.particle_weights, lower, upper, lower_open,
                            upper_open)
        oracle_obj.particle_weights = w
        if counts is not None:
            counts.append(n)
    oracle_obj.enforce_parameter_constraints = enforce_parameter_constraints
    return oracle_obj
