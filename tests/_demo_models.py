"""This project's own model functions for the experiments the reference's demos and tests measure (a Lorentzian peak or
dip, a straight line, Rabi oscillations, the impedance of a coil), in the plain-Python form the reference asks of a
model function: three arguments (settings, parameters, constants).  Between them they use what models.from_function
meets in such scripts: tuple unpacking and indexing of the arguments, entries the model ignores (a noise parameter),
module-level helpers, two settings, np.exp / np.cos / np.hypot, a two-channel result and, to be refused, complex
arithmetic.  golden/demo_model_functions.npz holds what the demos' own functions return on the inputs of
demo_inputs(); tests/test_reference_demo_models.py compares each model here with that to rounding."""
import numpy as np


def lorentz_peak(x, centre, height, offset, fwhm):
    return offset + height / (1.0 + (2.0 * (x - centre) / fwhm) ** 2)


def excited_fraction(t, detuning, b1):
    rate = np.hypot(detuning, b1)
    return b1 ** 2 / (b1 ** 2 + detuning ** 2) * (1.0 - np.cos(2.0 * np.pi * rate * t)) / 2.0


def peak_fitted_width(s, p, c):
    """Lorentzian whose full width is a fourth parameter."""
    (x,) = s
    centre, height, offset, fwhm = p
    return lorentz_peak(x, centre, height, offset, fwhm)


def peak_half_width(s, p, c):
    """Lorentzian with its half width as the one constant."""
    x = s[0]
    centre, height, offset = p
    half = c[0]
    return offset + height / (1.0 + ((x - centre) / half) ** 2)


def peak_indexed(s, p, c):
    """The same peak through the helper, every argument taken by index."""
    return lorentz_peak(s[0], p[0], p[1], p[2], 2.0 * c[0])


def peak_full_width(s, p, c):
    """Lorentzian with its full width as the one constant."""
    (x,) = s
    centre, height, offset = p
    (fwhm,) = c
    return lorentz_peak(x, centre, height, offset, fwhm)


def peak_with_noise_parameter(s, p, c):
    """Lorentzian, half width constant; the fourth parameter is the measurement noise, not part of the model."""
    (x,) = s
    centre, height, offset, _noise = p
    return offset + height / (1.0 + ((x - centre) / c[0]) ** 2)


def dip_below_one(s, p, c):
    """A Lorentzian dip of the given depth and full width below a baseline of one."""
    (f,) = s
    f0, depth, fwhm = p
    return 1.0 - lorentz_peak(f, f0, depth, 0.0, fwhm)


def line_with_noise_parameter(s, p, c):
    (x,) = s
    slope, intercept, _noise = p
    return intercept + slope * x


def straight_line(s, p, c):
    return p[0] + p[1] * s[0]


def rabi_signal(s, p, c):
    """Fluorescence after a pulse of length t at drive frequency f: Rabi oscillations damped by t1."""
    t, f = s
    b1, f0 = p
    level, depth, t1 = c
    return level * (1.0 - depth * np.exp(-t / t1) * excited_fraction(t, f - f0, b1))


def coil_impedance(s, p, c):
    """A coil (inductance in series with its resistance) in parallel with a capacitance, as (real, imaginary)."""
    (omega,) = s
    ind, res, cap, _noise = p
    z_coil = res + 1j * omega * ind
    z = z_coil / (1.0 + 1j * omega * cap * z_coil)
    return np.array([np.real(z), np.imag(z)])


def demo_models():
    """{"<file of the reference's demos or tests>:<line of its model function>": (the model here of the same
    experiment, n_settings, n_parameters, n_constants)}: one entry per model function the reference defines there."""
    line = (straight_line, 1, 2, 1)
    return {"demos/find_peak/seqLor_pdfevolve.py:31": (peak_fitted_width, 1, 4, 1),
            "demos/find_peak/sequentialLorentzian.py:53": (peak_half_width, 1, 3, 1),
            "demos/fit_vs_obe/fit_vs_obe_makedata.py:58": (peak_indexed, 1, 3, 1),
            "demos/line_plus_noise/line_plus_noise.py:36": (line_with_noise_parameter, 1, 3, 1),
            "demos/lockin/lockin_of_coil.py:63": (coil_impedance, 1, 4, 1),
            "demos/numba/numbaLorentzian.py:106": (peak_full_width, 1, 3, 1),
            "demos/pipulse/pipulse.py:37": (rabi_signal, 2, 2, 3),
            "demos/server/server_script.py:16": (dip_below_one, 1, 3, 1),
            "demos/sweeper/sweeper.py:42": (peak_with_noise_parameter, 1, 4, 1),
            "tests/server_script_61982.py:10": line,
            "tests/server_script_61983.py:11": line,
            "tests/server_script_61984.py:11": line,
            "tests/test_optbayesexpt.py:11": line,
            "tests/test_server.py:11": line,
            "tests/test_utils.py:11": line}


def demo_inputs(key, n=257):
    """The seeded inputs a model of ``demo_models()`` is evaluated on in the fixture: settings, parameters and
    constants as arrays of n values each, uniform in [0.5, 2)."""
    _, n_s, n_p, n_c = demo_models()[key]
    g = np.random.default_rng(sum(map(ord, key)))
    return tuple(g.uniform(0.5, 2.0, n) for _ in range(n_s)), tuple(g.uniform(0.5, 2.0, n) for _ in range(n_p)), \
        tuple(g.uniform(0.5, 2.0, n) for _ in range(n_c))
