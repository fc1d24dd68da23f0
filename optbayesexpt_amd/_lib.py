"""ctypes binding of libobe_hip.so (the C ABI declared in include/obe_hip.h).

There is no CPU fallback: if the shared library is missing or cannot be loaded the
import of the product classes fails with an explicit error.  PyTorch is imported first
so that the process ends up with a single HIP runtime (torch bundles libamdhip64.so.7,
the library's NEEDED entry resolves to the already-loaded copy).
"""
import ctypes
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libobe_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "obe_hip.h")



def _header_constants(path=HEADER_PATH):
    """The #define'd integers of include/obe_hip.h (one source of truth for limits and the ABI version)."""
    text = open(path).read()
    return {k: int(v) for k, v in re.findall(r"^#define\s+(OBE_[A-Z_]+)\s+(-?\d+)\s*(?:/\*.*)?$", text, flags=re.M)}


_H = _header_constants()
OBE_ABI_VERSION = _H["OBE_ABI_VERSION"]
OBE_MAX_CONSTS = _H["OBE_MAX_CONSTS"]
OBE_MAX_CHANNELS = _H["OBE_MAX_CHANNELS"]
OBE_MAX_SETDIMS = _H["OBE_MAX_SETDIMS"]
OBE_MAX_DIMS = _H["OBE_MAX_DIMS"]
OBE_FAST_DIMS = _H["OBE_FAST_DIMS"]                  # cloud kernels compiled for the exact row count up to here
OBE_CLOUD_MAX_DIMS = _H["OBE_CLOUD_MAX_DIMS"]        # what the tiled cloud kernels take (ParticlePDF alone)
OBE_BINOMIAL_MAX_CHANNELS = _H["OBE_BINOMIAL_MAX_CHANNELS"]      # channels of a model of yes/no outcomes
OBE_POISSON_MAX_CAP = _H["OBE_POISSON_MAX_CAP"]      # the largest censoring count of a counted reading's information
# count-aware scoring (K20): the largest count_max / shots / scored count, the levels of one call, the two laws
OBE_COUNT_MAX_OUTCOMES, OBE_COUNT_MAX_LEVELS = _H["OBE_COUNT_MAX_OUTCOMES"], _H["OBE_COUNT_MAX_LEVELS"]
OBE_COUNT_BINOMIAL, OBE_COUNT_POISSON = _H["OBE_COUNT_BINOMIAL"], _H["OBE_COUNT_POISSON"]
OBE_WS_RESULT_OFFSET = _H["OBE_WS_RESULT_OFFSET"]    # doubles
# bits of obe_sweep_utility's `shifted` argument
OBE_SWEEP_SHIFTED, OBE_SWEEP_SAFE = _H["OBE_SWEEP_SHIFTED"], _H["OBE_SWEEP_SAFE"]
OBE_SWEEP_SPECULATIVE, OBE_SWEEP_NOWAIT = _H["OBE_SWEEP_SPECULATIVE"], _H["OBE_SWEEP_NOWAIT"]
OBE_SWEEP_CELLS = _H["OBE_SWEEP_CELLS"]
# the cell form: half-width 1 / OBE_CELL_RHO_INV, OBE_CELL_ORDER coefficients per moment, at most OBE_CELL_MAX cells
OBE_CELL_RHO_INV, OBE_CELL_ORDER, OBE_CELL_MAX = _H["OBE_CELL_RHO_INV"], _H["OBE_CELL_ORDER"], _H["OBE_CELL_MAX"]
OBE_CELL_MIN_GAIN = _H["OBE_CELL_MIN_GAIN"]
# the bin form: the same half-width and order on the particles' axis, at most OBE_BIN_MAX bins
OBE_SWEEP_BINS, OBE_BIN_MAX = _H["OBE_SWEEP_BINS"], _H["OBE_BIN_MAX"]
# ... whose grouping obe_sweep_utility_keep() keeps in a buffer of the caller's from one sweep to the next
OBE_SWEEP_BINS_KEPT = _H["OBE_SWEEP_BINS_KEPT"]
HOST_SENTINEL = 0x7ff8c0dec0dec0de     # the value of an armed host result word (csrc/obe_common.h: kHostSentinel)

c_void_p, c_int, c_int32, c_int64, c_double = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int32,
                                               ctypes.c_int64, ctypes.c_double)


class MomentLayout:
    """Where the K3 moment block of ``n_dims`` parameter rows (include/obe_hip.h: obe_moments) keeps what, and where
    the host blocks that carry it put it."""

    def __init__(self, n_dims):
        d = n_dims
        # [sum w, sum w^2, mean, m1, m2, std] (the first moments), then the D x D covariance
        self.mean, self.std, self.cov = slice(2, 2 + d), slice(2 + 3 * d, 2 + 4 * d), slice(2 + 4 * d, 2 + 4 * d + d * d)
        self.first_len = 2 + 4 * d
        self.total_len = 2 + 4 * d + d * d            # obe_moments_len(n_dims)
        # the fused update's host block: [sum t, sum w'^2, the first moments, the resample decision (enqueued form)]
        self.update_decision = 4 + 4 * d
        self.update_len = 5 + 4 * d
        # obe_resample_begin's h_f64: [sum w, the K3 block]
        self.resample_k3 = 1


class ObeHipError(RuntimeError):
    """A libobe_hip call returned a non-zero status (``status``: -1 = the call was refused on its arguments
    BEFORE anything was launched, include/obe_hip.h; anything else is a hipError_t of a launch or a wait)."""

    def __init__(self, message, status=None):
        RuntimeError.__init__(self, message)
        self.status = status

    @property
    def refused_before_launch(self):
        return self.status == -1


class ObeModelStruct(ctypes.Structure):
    """Mirror of ``struct obe_model`` (include/obe_hip.h)."""
    _fields_ = [("id", c_int32), ("aux", c_int32), ("n_params", c_int32),
                ("n_setdims", c_int32), ("n_channels", c_int32), ("n_consts", c_int32),
                ("consts", c_double * OBE_MAX_CONSTS)]


def declared_symbols(header_path=HEADER_PATH):
    """Every function name the header declares (used by the symbol-export test)."""
    text = open(header_path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(obe_[a-z0-9_]+)\s*\(", text)))


_SCALARS = {"int": c_int, "int32_t": c_int32, "int64_t": c_int64, "double": c_double}
# (callers pass the structure itself: ctypes passes it by reference)
_POINTERS = {"obe_model*": ctypes.POINTER(ObeModelStruct), "char*": ctypes.c_char_p}


def _ctype(c_type):
    """How a C type of the header is bound (``const`` aside): the scalars and the pointers named above as such, every
    other pointer as an address.  A type outside this rule is refused, never guessed."""
    m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\**)", c_type)
    if m and m[2]:
        return _POINTERS.get(m[1] + m[2], c_void_p)
    if m and m[1] in _SCALARS:
        return _SCALARS[m[1]]
    raise TypeError(f"no ctypes binding for the C type {c_type!r} of include/obe_hip.h")


def _prototypes(header_path=HEADER_PATH):
    """name -> (restype, [(ctype, parameter name), ...]) of every OBE_API declaration of the header."""
    text = re.sub(r"/\*.*?\*/", "", open(header_path).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"^OBE_API\s+([^(]+?)\s*\b(obe_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        args = []
        for param in [] if params.strip() == "void" else params.split(","):
            m = re.fullmatch(r"(.+?)\s*\b(\w+)", param.strip())
            if m is None:
                raise TypeError(f"{name}: cannot read the parameter {param.strip()!r} of include/obe_hip.h")
            args.append((_ctype(m[1]), m[2]))
        protos[name] = (_ctype(ret), args)
    return protos


PROTOTYPES = _prototypes()


# entry points whose code depends on the model: a plugin library serves these
MODEL_ENTRY_POINTS = ("obe_model_validate", "obe_workspace_bytes", "obe_sweep_settings_per_lane",
                      "obe_sweep_settings_per_lane_for", "obe_bayes_update_model",
                      "obe_bayes_update_model_moments", "obe_bayes_update_model_moments_enqueue",
                      "obe_strict_sums",
                      "obe_bayes_update_sweep",
                      "obe_eval_over_particles",
                      "obe_eval_over_settings", "obe_sweep_utility", "obe_sweep_kernel_time", "obe_sweep_timing",
                      "obe_sweep_utility_keep", "obe_sweep_bins_keep_bytes", "obe_sweep_bins_keep_records_bytes",
                      "obe_eval_draws",
                      "obe_predictive_workspace_bytes", "obe_predictive_moments", "obe_predictive_quantiles",
                      "obe_predictive_score_workspace_bytes", "obe_predictive_logpdf", "obe_predictive_tails",
                      "obe_predictive_reading_workspace_bytes", "obe_predictive_reading_quantiles",
                      "obe_output_covariance_workspace_bytes", "obe_output_covariance",
                      "obe_records_loglik_workspace_bytes", "obe_records_loglik",
                      "obe_output_cross_covariance_workspace_bytes", "obe_output_cross_covariance",
                      "obe_signal_noise_likelihood", "obe_signal_noise_workspace_bytes", "obe_signal_noise_variance",
                      "obe_binomial_likelihood", "obe_binomial_workspace_bytes", "obe_binomial_information",
                      "obe_poisson_likelihood", "obe_poisson_workspace_bytes", "obe_poisson_information",
                      "obe_signal_noise_records_loglik_workspace_bytes", "obe_signal_noise_records_loglik",
                      "obe_binomial_records_loglik_workspace_bytes", "obe_binomial_records_loglik",
                      "obe_poisson_records_loglik_workspace_bytes", "obe_poisson_records_loglik",
                      "obe_count_workspace_bytes", "obe_count_table", "obe_count_tails", "obe_count_quantiles",
                      "obe_count_logpmf",
                      "obe_signal_noise_logpdf", "obe_signal_noise_tails", "obe_signal_noise_reading_quantiles")


class HipLib:
    """Loaded library with typed entry points; ``call(name, *args)`` raises on error."""

    def __init__(self, path=LIB_PATH, plugin=False, allow_variant=False):
        if not os.path.exists(path):
            raise ImportError(
                f"{path} not found: the HIP library has not been built.  Run "
                "`python -m optbayesexpt_amd.build` (needs hipcc).  optbayesexpt_amd has "
                "no CPU fallback.")
        import torch  # noqa: F401  (loads the HIP runtime the library will bind to)
        self.path = path
        self.cdll = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL if plugin else ctypes.RTLD_GLOBAL)
        names = MODEL_ENTRY_POINTS + ("obe_abi_version", "obe_last_error", "obe_source_fingerprint") if plugin \
            else tuple(PROTOTYPES)
        for name in names:
            restype, params = PROTOTYPES[name]
            fn = getattr(self.cdll, name)
            fn.restype = restype
            fn.argtypes = [ctype for ctype, _ in params]
        abi = self.cdll.obe_abi_version()
        if abi != OBE_ABI_VERSION:
            raise ImportError(f"libobe_hip ABI {abi} does not match this package ({OBE_ABI_VERSION})")
        from . import build
        built_from = self.cdll.obe_source_fingerprint().decode()
        #: extra compiler flags of a tools/build_variant.py library ("" for the product build); such a
        #: library is only accepted when the caller asks for it by path with allow_variant=True
        self.variant_flags = built_from.partition("+")[2]
        if allow_variant:
            built_from = built_from.partition("+")[0]
        if built_from != build._source_fingerprint():
            raise ImportError(f"{path} was built from other kernel sources ({built_from}) than the ones next to it "
                              f"({build._source_fingerprint()}): run `python -m optbayesexpt_amd.build`")

    def last_error(self):
        msg = self.cdll.obe_last_error()
        return msg.decode() if msg else ""

    def call(self, name, *args):
        rc = getattr(self.cdll, name)(*args)
        if rc != 0:
            raise ObeHipError(f"{name} failed (status {rc}): {self.last_error()}", rc)
        if _AUDIT_ON:
            audit.after_call(name, args)          # OBE_CHECK_DELIVERY=1 (_audit.py): which host words are armed now
        return rc

    def workspace_bytes(self, n_particles, n_settings, n_channels, n_dims):
        return int(self.cdll.obe_workspace_bytes(n_particles, n_settings, n_channels, n_dims))

    def moments_len(self, n_dims):
        return int(self.cdll.obe_moments_len(n_dims))

    def device_info(self):
        buf = ctypes.create_string_buffer(256)
        ncu, mem = c_int(0), c_int64(0)
        rc = self.cdll.obe_device_info(buf, 256, ctypes.byref(ncu), ctypes.byref(mem))
        return dict(name=buf.value.decode(), n_cu=ncu.value, hbm_bytes=mem.value, is_gfx950=(rc == 0))


class DeviceBound:
    """A HipLib (or plugin) bound to one GPU.  The C ABI launches on the calling thread's *current*
    HIP device with the stream and pointers it is given; an object created with ``device='cuda:1'``
    while device 0 is current would otherwise launch on the wrong GPU.  Every call through this
    wrapper runs with the object's device current (a no-op test when it already is)."""

    def __init__(self, lib, device):
        import torch
        self._lib = lib._lib if isinstance(lib, DeviceBound) else lib
        self._torch = torch
        self.index = device.index if device.index is not None else torch.cuda.current_device()
        # one visible GPU: the current device cannot be another one
        self._single = torch.cuda.device_count() == 1 and self.index == 0

    def guard(self):
        if self._torch.cuda.current_device() == self.index:
            return _NO_GUARD
        return self._torch.cuda.device(self.index)

    def call(self, name, *args):
        if self._single:
            return self._lib.call(name, *args)
        with self.guard():
            return self._lib.call(name, *args)

    def device_info(self):
        with self.guard():
            return self._lib.device_info()

    def __getattr__(self, name):          # cdll, path, workspace_bytes, moments_len, last_error
        return getattr(self._lib, name)


import contextlib                         # noqa: E402
from ._audit import audit                 # noqa: E402  (here: _audit imports names defined above from this module)
_AUDIT_ON = audit.on
_NO_GUARD = contextlib.nullcontext()

_LIB = None
_PLUGINS = {}


def load_plugin(path):
    """A per-model plugin library (optbayesexpt_amd.build.build_plugin), loaded once."""
    if path not in _PLUGINS:
        _PLUGINS[path] = HipLib(path, plugin=True)
    return _PLUGINS[path]


def load():
    """The process-wide library instance (loaded on first use).  If the in-tree library has
    not been built yet and hipcc is present it is built now; otherwise HipLib raises —
    there is no CPU fallback."""
    global _LIB
    if _LIB is None:
        from . import build
        if os.path.exists(build.HIPCC) and build.library_is_stale():
            # before the first dlopen (a loaded library cannot be replaced); serialised across the
            # ranks of a multi-GPU job by build()'s file lock, silent on stdout
            build.build(only_if_stale=True)
        _LIB = HipLib()
    return _LIB


def host_ptr(arr):
    """Address of a C-contiguous NumPy array (kept alive by the caller)."""
    return c_void_p(arr.ctypes.data)          # (data_as() costs twice as much: 2.2 vs 1.2 us per call)


class HostArgs:
    """Small host arrays that an object passes to the library call after call (record values,
    settings, result scalars), with their addresses made once: ``arr.ctypes`` builds a helper
    object every time it is touched (~1 us), and a cycle passes five such arrays."""

    def __init__(self):
        self._known = {}

    def keep(self, arr):
        self._known[id(arr)] = (arr, host_ptr(arr))          # (the array is kept alive with its address)
        return arr

    def ptr(self, arr):
        hit = self._known.get(id(arr))
        return hit[1] if hit is not None else host_ptr(arr)

    def ptr_keep(self, arr):
        """ptr() that remembers a long-lived array the first time it sees it."""
        hit = self._known.get(id(arr))
        if hit is None:
            self.keep(arr)
            hit = self._known[id(arr)]
        return hit[1]


# Page-locked landing zones outlive the objects that own them until the device has drained.  Kernels write their
# results straight into such memory, and some of them are deliberately not waited for (the sweep enqueued behind an
# update, the sum(w) of a small draw, the moments behind a constraint mask): when their object is garbage-collected
# with such a kernel still in flight, torch's caching host allocator — which knows nothing of kernels that write host
# memory themselves — would hand the block to the NEXT pin_memory() call at once, i.e. the next object's landing
# zone, and the late kernel would write into it (found by tools/soak_ranks.py once it mixed object classes: a
# spurious "Probabilities do not sum to 1").  So a released block goes to a limbo list instead, with the device
# whose kernels write it, and the list is emptied only behind a synchronisation of exactly those devices.
# (Device memory needs no such care: torch's device allocator reuses a block on the stream it was used on, and every
# kernel of this package runs on that stream or on a side stream that is joined back before the call returns.)
_LIMBO = []                # (keeper, device index)
_LIMBO_MAX = 64
_NO_LIMBO = os.environ.get("OBE_NO_LIMBO") == "1"


def _current_device_index():
    import torch
    try:
        return torch.cuda.current_device() if torch.cuda.is_available() else None
    except Exception:
        return None


def _retire_pinned(keeper, device):
    audit.zone_released(keeper)
    if _NO_LIMBO:            # (test hook: the behaviour before round 5's fix — the block goes straight back to the allocator)
        audit.zone_freed(keeper, drained=False)
        return
    _LIMBO.append((keeper, device))


def _purge_limbo(force=False):
    """Empties the limbo list once it holds _LIMBO_MAX blocks: synchronises the devices those blocks belong to —
    and no others: a rank of a multi-GPU job sees every GPU of the node, and touching one it does not use would
    create a context there — and only then lets the allocator have them."""
    if len(_LIMBO) < _LIMBO_MAX and not force:
        return
    import torch
    try:
        for d in sorted({d for _, d in _LIMBO if d is not None}):
            torch.cuda.synchronize(d)
    except Exception:        # (interpreter shutdown, a device that is gone: keep the blocks)
        return
    for keeper, _ in _LIMBO:
        audit.zone_freed(keeper, drained=True)
    del _LIMBO[:]


def pinned_array(n, dtype=np.float64, device=None):
    """A zeroed page-locked host array (NumPy view of a pinned torch tensor, which it keeps alive).
    The kernels that end a call write their few result scalars straight into such memory; a pageable
    array works too, through a small device-to-host copy."""
    import torch
    import weakref
    _purge_limbo()
    t = torch.zeros(n, dtype=torch.from_numpy(np.zeros(0, dtype=dtype)).dtype).pin_memory()
    raw = t.numpy()                       # the array every view of the zone has as its base: it keeps the storage alive ...
    dev = _current_device_index() if device is None else device
    weakref.finalize(raw, _retire_pinned, t, dev)          # ... and when the last view has gone, the limbo list does
    a = audit.wrap(raw)
    audit.zone_created(t.data_ptr(), t.numel() * t.element_size(), t)
    return a


def device_ptr_of_pinned(lib, arr):
    """The address kernels use for a ``pinned_array`` (obe_host_device_pointer): what to pass where
    the C ABI takes a *device* pointer and the result should land in host memory directly."""
    d = c_void_p()
    lib.call("obe_host_device_pointer", host_ptr(arr), ctypes.byref(d))
    return c_void_p(d.value)


def f64(values, n=None):
    """Small host array of float64 for by-value style arguments."""
    a = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1))
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} values, got {a.size}")
    return a
