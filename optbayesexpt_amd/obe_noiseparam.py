"""OptBayesExptNoiseParameter — measurement noise as an unknown (particle) parameter.

Mirrors optbayesexpt/obe_noiseparam.py:5-136: the likelihood takes sigma from a
parameter row (per particle), the utility's noise variance is the weighted mean of
sigma^2, and after every resample particles with sigma <= 0 get zero weight.  All
three run in libobe_hip kernels (K2 with ``h_noise_rows``, the K3 moment block, K6).
"""
import numpy as np
import torch

from . import _bounds, _lib
from .obe_base import OptBayesExpt, _overridden
from ._devcall import ptr as _ptr


class OptBayesExptNoiseParameter(OptBayesExpt):
    """``noise_parameter_index``: int or tuple, one parameter row per output channel
    (obe_noiseparam.py:45-55)."""

    def __init__(self, measurement_model, setting_values, parameter_samples,
                 constants, noise_parameter_index=None, **kwargs):
        OptBayesExpt.__init__(self, measurement_model, setting_values,
                              parameter_samples, constants, **kwargs)
        self.noise_parameter_index = np.atleast_1d(noise_parameter_index)
        if len(self.noise_parameter_index) != self.n_channels:
            raise RuntimeError(f"noise_parameter_index is not compatible with"
                               f" {self.n_channels} measurement channels")
        self._noise_rows = np.zeros(max(_lib.OBE_MAX_DIMS, self.n_channels), dtype=np.int32)
        rows = np.asarray(self.noise_parameter_index, dtype=np.int64)
        rows = np.where(rows < 0, rows + self.n_dims, rows)          # NumPy negative indexing
        if np.any(rows < 0) or np.any(rows >= self.n_dims):
            raise IndexError("noise_parameter_index out of range")
        self._noise_rows[:self.n_channels] = rows

    # -- likelihood: sigma is a parameter row (obe_noiseparam.py:81-120) --------------
    def _likelihood_inputs(self, measurement_record):
        y_meas = measurement_record[1]
        n, yy, _ = self._record_channels(y_meas, None)
        return n, yy, None, self._noise_rows

    def _likelihood_overridden(self):
        return _overridden(self, "likelihood", OptBayesExpt, OptBayesExptNoiseParameter)

    def likelihood(self, y_model, measurement_record):
        """Per-particle-sigma Gaussian likelihood; same device kernel as the base class,
        with sigma read from the noise parameter rows."""
        return OptBayesExpt.likelihood(self, y_model, measurement_record)

    # -- constraint: sigma > 0 (obe_noiseparam.py:57-79) ------------------------------
    # enforce_parameter_constraints(), the gather that applies the constraint itself and last_constraint_count are the
    # base class's (obe_base.py): this class says which constraint.
    def _effective_bounds(self, normal):
        """The user's bounds AND this class's sigma > 0 on the noise rows, as one set of bounds."""
        if normal is None:
            return None
        return _bounds.intersect_positive(normal, self._noise_rows[:self.n_channels])

    def _device_constraint(self):
        """Without bounds: zero the weight of every particle whose noise parameter is <= 0 and renormalise, by the
        entry points written for exactly that (obe_mask_nonpositive*).  With set_parameter_bounds(): one mask of the
        intersection (_effective_bounds), by the bounds' entry points."""
        bounded = OptBayesExpt._device_constraint(self)
        if bounded is not None:
            return bounded
        return ("obe_mask_nonpositive", "obe_resample_particles_aos_masked",
                (self._hargs.ptr_keep(self._noise_rows), self.n_channels), False)

    # -- noise model: weighted mean of sigma^2 (obe_noiseparam.py:122-136) ------------
    def yvar_noise_model(self):
        """(C, 1) weighted mean of sigma^2, reduced on the device (K3 block)."""
        t, _ = OptBayesExptNoiseParameter._noise_var_device(self, values=True)
        return t.cpu().numpy().reshape((self.n_channels, 1))

    def _noise_token(self):
        # (the noise variance is a function of the cloud alone: nothing else to compare)
        if _overridden(self, "yvar_noise_model", OptBayesExpt, OptBayesExptNoiseParameter) \
                or self._parameters is not self._particles:
            return None
        return "cloud"

    def _noise_var_device(self, values=False):
        """What a sweep takes as its noise variance: the K3 block itself with the noise rows encoded in the
        leading dimension (include/obe_hip.h: OBE_NOISE_FROM_MOMENTS) — the kernel that forms the utility divides
        m2[row] by sum w itself; ``values``: the C variances as a device vector (yvar_noise_model())."""
        if _overridden(self, "yvar_noise_model", OptBayesExptNoiseParameter):
            return OptBayesExpt._noise_var_device(self)
        if self._parameters is self._particles:
            mom = self._moments_on_device()
            if not values and self._device_model is not None:
                code = self.__dict__.get("_noise_ld_code")
                if code is None:
                    # (5 bits per channel, OBE_MAX_CHANNELS channels: rows below 32 — any other object hands the
                    # sweep the variances as values instead)
                    rows = [int(r) for r in self._noise_rows[:self.n_channels]]
                    if max(rows) < 32 and len(rows) <= _lib.OBE_MAX_CHANNELS:
                        code = self._noise_ld_code = -1 - sum(r << (5 * c) for c, r in enumerate(rows))
                    else:
                        code = self._noise_ld_code = 0
                if code:
                    return mom, code
        else:
            # stale alias after set_pdf(): the reference averages the rows of
            # ``parameters`` (old samples) with the current weights
            par, w = self._parameters.tensor(), self._weights.tensor()
            if par.shape[1] != w.shape[0]:
                raise ValueError("parameters and particle_weights have different lengths")
            mom = torch.zeros_like(self._moments_dev)
            self._lib.call("obe_moments", _ptr(par), par.shape[1], self.n_dims, par.shape[1], _ptr(w), 0,
                           _ptr(mom), None, _ptr(self._ws), self._ws_bytes, self._stream())
        self._lib.call("obe_noise_var_from_moments", _ptr(mom), self.n_dims, _lib.host_ptr(self._noise_rows),
                       self.n_channels, _ptr(self._noise_dev), self._stream())
        self._noise_cache = None
        return self._noise_dev, 0
