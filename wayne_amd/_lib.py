"""ctypes binding of libwayne_hip.so (include/wayne_hip.h).

The library is the only compute path.  If it is missing it is built with
hipcc (wayne_amd/build.py); if that fails, or no gfx950 GPU is present when a
context is requested, this raises -- there is no CPU fallback.
"""
import ctypes as C
import os
import threading
import weakref

import numpy as np

from . import build as _build

# status codes (wayne_hip.h)
OK, E_INVALID, E_NEGATIVE, E_OVERFLOW, E_NOMEM, E_HIP, E_NODEVICE, E_STATE = 0, -1, -2, -3, -4, -5, -6, -7
RNG_REPLAY, RNG_PHILOX, RNG_SPLIT = 0, 1, 2
F_ADD_FLAT = 1 << 0
F_ADD_GAIN_VARIATIONS = 1 << 1
F_ADD_NON_LINEAR = 1 << 2
F_CLIP_DET_LIMITS = 1 << 3
F_ADD_READ_NOISE = 1 << 4
F_ADD_STELLAR_NOISE = 1 << 5
F_ADD_DARK = 1 << 6
F_ADD_INITIAL_BIAS = 1 << 7
F_OUT_F64 = 1 << 16
F_OUT_U16 = 1 << 18
# the reads' sample types: numpy dtype -> descriptor flag (float32 is the absence of one)
OUT_FLAGS = {np.dtype(np.float32): 0, np.dtype(np.float64): F_OUT_F64, np.dtype(np.uint16): F_OUT_U16}
F_EXACT_SAMPLERS = 1 << 17
PROF_KERNELS = 8
ABI_VERSION = 7
EXPECT_COUNTS, EXPECT_MEAN = 1, 2   # modes of the expected image (WAYNE_EXPECT_*)
EXPECT_MODES = {"counts": EXPECT_COUNTS, "mean": EXPECT_MEAN}
EXPECT_NAMES = {0: None, EXPECT_COUNTS: "counts", EXPECT_MEAN: "mean"}
MAX_SOURCES = 8   # contaminants per exposure (WAYNE_MAX_SOURCES)
MAX_TRAP_RATES = 4096   # points of a charge-trap start table (WAYNE_MAX_TRAP_RATES)
# wayne_extract_desc.steps (WAYNE_X_*)
X_LINEARISE, X_DARK, X_GAIN, X_SKY, X_LAST_READ, X_ALL = 1, 2, 4, 8, 16, 31
EXTRACT_PRODUCTS = 17   # row windows a wayne_extract_desc holds
C_FLAT = 1              # wayne_channels_desc.flags (WAYNE_C_*)
MAX_CHANNELS = 256      # WAYNE_MAX_CHANNELS
MAX_CHANNEL_HULL = 384  # WAYNE_MAX_CHANNEL_HULL
MAX_OPTIMAL_HALF_WIDTH = 16  # WAYNE_MAX_OPTIMAL_HALF_WIDTH


class WayneError(RuntimeError):
    def __init__(self, status, msg):
        RuntimeError.__init__(self, "wayne_hip status %d: %s" % (status, msg))
        self.status = status


class WayneNoDeviceError(WayneError):
    pass


_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)


class GrismDesc(C.Structure):
    _fields_ = [("trace_coeff", C.c_double * 9), ("wl_solution", C.c_double * 9),
                ("psf_ratio_poly", C.c_double * 4), ("psf_sigmal_poly", C.c_double * 4),
                ("psf_sigmah_poly", C.c_double * 4), ("n_sens", C.c_int),
                ("sens_wl_um", _dp), ("sens_val", _dp),
                ("flat_wmin", C.c_double), ("flat_wmax", C.c_double)]


class Calibration(C.Structure):
    _fields_ = [("subarray", C.c_int), ("n_reads", C.c_int), ("flat", _fp * 4), ("pfl", _fp),
                ("sky", _fp), ("lin", _fp * 4), ("dark_sci", _fp), ("dark_err", _fp),
                ("zero_read", _dp)]


class ExposureDesc(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("exposure_index", C.c_uint32), ("rng_mode", C.c_int),
                ("threads_compat", C.c_int), ("flags", C.c_uint32), ("sub_scale", C.c_int),
                ("n_wl", C.c_int), ("wl_um", _dp), ("flux", _dp), ("depth", _dp),
                ("n_samples", C.c_int), ("x_ref", _dp), ("y_ref", _dp), ("dur_ms", _dp),
                ("replay_seed", _ip), ("sample_read", _ip),
                ("n_reads", C.c_int), ("read_dt_s", _dp),
                ("sky_ct_s", C.c_double), ("cosmic_rate", C.c_double), ("scale_factor", C.c_double),
                ("noise_mean", C.c_double), ("noise_std", C.c_double),
                ("thrower_margin", C.c_int), ("thrower_splits", C.c_int),
                ("lc_z", _dp), ("lc_hidden", _dp), ("lc_rp", _dp), ("lc_ld", C.c_double * 4)]


class SourceDesc(C.Structure):
    _fields_ = [("tag", C.c_uint32), ("n_wl", C.c_int), ("wl_um", _dp), ("flux", _dp),
                ("dx", C.c_double), ("dy", C.c_double)]


class TrapDesc(C.Structure):
    _fields_ = [("n_traps", C.c_double * 2), ("efficiency", C.c_double * 2), ("lifetime_s", C.c_double * 2),
                ("n_rate", C.c_int), ("rate_lo", C.c_double), ("rate_hi", C.c_double), ("start", _dp * 2)]


class TrapHistoryDesc(C.Structure):
    _fields_ = [("gap_s", C.c_double), ("lit", C.c_int), ("fill", C.c_double * 2)]


class ExtractDesc(C.Structure):
    _fields_ = [("steps", C.c_uint32), ("row_lo", C.c_int * EXTRACT_PRODUCTS), ("row_hi", C.c_int * EXTRACT_PRODUCTS),
                ("bg_col_lo", C.c_int), ("bg_col_hi", C.c_int)]


class CrrejDesc(C.Structure):
    _fields_ = [("k", C.c_double), ("read_noise_e", C.c_double)]


class ChannelsDesc(C.Structure):
    _fields_ = [("n_channels", C.c_int), ("edges_um", _dp), ("wl_a", _dp), ("wl_b", _dp), ("flags", C.c_uint32)]


class VarianceDesc(C.Structure):
    _fields_ = [("read_noise", C.c_double)]


class RampFitDesc(C.Structure):
    _fields_ = [("steps", C.c_uint32), ("read_noise_e", C.c_double), ("k_jump", C.c_double), ("saturation_dn", C.c_double)]


class ImaDesc(C.Structure):
    _fields_ = [("steps", C.c_uint32), ("units", C.c_int), ("read_noise_e", C.c_double), ("saturation_dn", C.c_double)]


class SpotsDesc(C.Structure):
    _fields_ = [("n", C.c_int32), ("cx", C.c_double * 8), ("cy", C.c_double * 8), ("radius", C.c_double * 8),
                ("contrast", C.POINTER(C.c_double)), ("px", C.POINTER(C.c_double)), ("py", C.POINTER(C.c_double))]


class IpcDesc(C.Structure):
    _fields_ = [("k", (C.c_double * 3) * 3)]


class OptimalDesc(C.Structure):
    _fields_ = [("half_width", C.c_int)]


class Profile(C.Structure):
    _fields_ = [("name", C.c_char_p * PROF_KERNELS), ("launches", C.c_uint64 * PROF_KERNELS),
                ("ms", C.c_double * PROF_KERNELS), ("electrons", C.c_uint64)]


# every symbol include/wayne_hip.h declares: name -> (restype, argtypes)
_vp = C.c_void_p
SYMBOLS = {
    "wayne_abi_version": (C.c_int, []),
    "wayne_strerror": (C.c_char_p, [C.c_int]),
    "wayne_build_flags": (C.c_char_p, []),
    "wayne_device_count": (C.c_int, []),
    "wayne_ctx_create": (_vp, [C.c_int, C.POINTER(C.c_int)]),
    "wayne_ctx_destroy": (None, [_vp]),
    "wayne_last_error": (C.c_char_p, [_vp]),
    "wayne_ctx_synchronize": (C.c_int, [_vp]),
    "wayne_ctx_stream": (_vp, [_vp]),
    "wayne_ctx_set_knob": (C.c_int, [_vp, C.c_char_p, C.c_longlong]),
    "wayne_ctx_get_knob": (C.c_int, [_vp, C.c_char_p, C.POINTER(C.c_longlong)]),
    "wayne_psf_apply": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int,
                                  C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint32, _vp]),
    "wayne_psf_apply_ex": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int,
                                     C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, _vp]),
    "wayne_ctx_set_grism": (C.c_int, [_vp, C.POINTER(GrismDesc)]),
    "wayne_ctx_set_calibration": (C.c_int, [_vp, C.POINTER(Calibration)]),
    "wayne_ctx_slots": (C.c_int, [_vp]),
    "wayne_exposure_upload": (C.c_int, [_vp, C.c_int, C.POINTER(ExposureDesc)]),
    "wayne_exposure_run": (C.c_int, [_vp, C.c_int]),
    "wayne_exposure_run_checked": (C.c_int, [_vp, C.c_int]),
    "wayne_exposure_status": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int)]),
    "wayne_ctx_reruns": (C.c_ulonglong, [_vp]),
    "wayne_exposure_download": (C.c_int, [_vp, C.c_int, _vp]),
    "wayne_exposure_fetch_async": (C.c_int, [_vp, C.c_int]),
    "wayne_exposure_wait": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_void_p)]),
    "wayne_exposure_device_reads": (_vp, [_vp, C.c_int]),
    "wayne_exposure_synthesize": (C.c_int, [_vp, C.POINTER(ExposureDesc), _vp]),
    "wayne_exposure_debug_fetch": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp]),
    "wayne_exposure_debug_depth": (C.c_int, [_vp, C.c_int, _vp]),
    "wayne_exposure_debug_boxes": (C.c_int, [_vp, C.c_int, _vp, _vp, C.POINTER(C.c_int)]),
    "wayne_exposure_run_front": (C.c_int, [_vp, C.c_int]),
    "wayne_exposure_run_back": (C.c_int, [_vp, C.c_int]),
    "wayne_exposure_ramp_variant": (C.c_int, [_vp, C.c_int, C.c_char_p, C.c_int]),
    "wayne_exposure_set_sources": (C.c_int, [_vp, C.c_int, C.POINTER(SourceDesc), C.c_int]),
    "wayne_source_seed": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "wayne_exposure_set_traps": (C.c_int, [_vp, C.c_int, C.POINTER(TrapDesc)]),
    "wayne_ctx_trap_state_reset": (C.c_int, [_vp, _dp]),
    "wayne_ctx_trap_state_upload": (C.c_int, [_vp, _vp]),
    "wayne_ctx_trap_state_download": (C.c_int, [_vp, _vp]),
    "wayne_exposure_set_trap_history": (C.c_int, [_vp, C.c_int, C.POINTER(TrapHistoryDesc)]),
    "wayne_exposure_debug_fetch_source": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "wayne_exposure_set_extraction": (C.c_int, [_vp, C.c_int, C.POINTER(ExtractDesc)]),
    "wayne_exposure_fetch_spectra_async": (C.c_int, [_vp, C.c_int]),
    "wayne_exposure_wait_spectra": (C.c_int, [_vp, C.c_int, C.POINTER(_dp), C.POINTER(_dp)]),
    "wayne_exposure_download_spectra": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "wayne_exposure_set_crrej": (C.c_int, [_vp, C.c_int, C.POINTER(CrrejDesc)]),
    "wayne_exposure_rejected": (C.c_int, [_vp, C.c_int, C.POINTER(C.POINTER(C.c_uint32))]),
    "wayne_exposure_download_crmask": (C.c_int, [_vp, C.c_int, _vp]),
    "wayne_exposure_set_channels": (C.c_int, [_vp, C.c_int, C.POINTER(ChannelsDesc)]),
    "wayne_exposure_channels": (C.c_int, [_vp, C.c_int, C.POINTER(_dp)]),
    "wayne_exposure_set_variance": (C.c_int, [_vp, C.c_int, C.POINTER(VarianceDesc)]),
    "wayne_exposure_variances": (C.c_int, [_vp, C.c_int, C.POINTER(_dp), C.POINTER(_dp), C.POINTER(_dp)]),
    "wayne_exposure_set_optimal": (C.c_int, [_vp, C.c_int, C.POINTER(OptimalDesc)]),
    "wayne_exposure_optimal": (C.c_int, [_vp, C.c_int, C.POINTER(_dp), C.POINTER(_dp)]),
    "wayne_exposure_deliver_profile": (C.c_int, [_vp, C.c_int, C.c_int]),
    "wayne_exposure_set_optimal_profile": (C.c_int, [_vp, C.c_int, _dp, C.POINTER(C.c_int)]),
    "wayne_exposure_set_optimal_profile_tagged": (C.c_int, [_vp, C.c_int, _dp, C.POINTER(C.c_int), C.c_uint64]),
    "wayne_ctx_profile_uploads": (C.c_ulonglong, [_vp]),
    "wayne_exposure_set_optimal_channels": (C.c_int, [_vp, C.c_int, C.c_int]),
    "wayne_exposure_optimal_channels": (C.c_int, [_vp, C.c_int, C.POINTER(_dp), C.POINTER(_dp)]),
    "wayne_exposure_fetch_profile": (C.c_int, [_vp, C.c_int]),
    "wayne_exposure_profile": (C.c_int, [_vp, C.c_int, C.POINTER(_dp), C.POINTER(C.c_size_t)]),
    "wayne_extract_profile": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "wayne_fits_layout": (C.c_int, [C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                    C.POINTER(C.c_int)]),
    "wayne_exposure_set_fits": (C.c_int, [_vp, C.c_int, C.c_int]),
    "wayne_exposure_fetch_fits_async": (C.c_int, [_vp, C.c_int]),
    "wayne_exposure_wait_fits": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_void_p)]),
    "wayne_exposure_download_fits": (C.c_int, [_vp, C.c_int, _vp]),
    "wayne_fits_profile": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "wayne_exposure_set_expected": (C.c_int, [_vp, C.c_int, C.c_int]),
    "wayne_exposure_download_expected": (C.c_int, [_vp, C.c_int, _dp]),
    "wayne_expected_profile": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "wayne_exposure_set_rampfit": (C.c_int, [_vp, C.c_int, C.POINTER(RampFitDesc)]),
    "wayne_exposure_download_rampfit": (C.c_int, [_vp, C.c_int, _dp, _dp, C.POINTER(C.c_uint32)]),
    "wayne_rampfit_profile": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "wayne_ima_layout": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "wayne_exposure_set_ima": (C.c_int, [_vp, C.c_int, C.POINTER(ImaDesc)]),
    "wayne_exposure_download_ima": (C.c_int, [_vp, C.c_int, _vp]),
    "wayne_ima_profile": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "wayne_ipc_weights": (C.c_int, [C.POINTER(IpcDesc), C.POINTER(C.c_int32)]),
    "wayne_exposure_set_ipc": (C.c_int, [_vp, C.c_int, C.POINTER(IpcDesc)]),
    "wayne_ipc_profile": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "wayne_exposure_set_limb_darkening": (C.c_int, [_vp, C.c_int, _dp, C.c_int]),
    "wayne_exposure_set_spots": (C.c_int, [_vp, C.c_int, C.POINTER(SpotsDesc), C.c_int, C.c_int]),
    "wayne_spot_lens_basis": (None, [C.c_double] * 6 + [_dp]),
    "wayne_spot_rule": (None, [_dp, _dp]),
    "wayne_spots_profile": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "wayne_profile_enable": (C.c_int, [_vp, C.c_int]),
    "wayne_profile_select": (C.c_int, [_vp, C.c_uint]),
    "wayne_profile_reset": (C.c_int, [_vp]),
    "wayne_profile_get": (C.c_int, [_vp, C.POINTER(Profile)]),
    "wayne_philox4x32": (None, [_vp, _vp, _vp]),
    "wayne_host_sample_draws": (None, [C.c_uint32, C.c_uint32, C.c_int, _vp, _vp, _vp]),
}

_lib = None


def load():
    """Load (building first if needed) libwayne_hip.so.  Raises on failure."""
    global _lib, _lib_path
    if _lib is None:
        path = _build.LIB
        override = os.environ.get("WAYNE_HIP_LIB")
        if override:
            # a library built elsewhere with other flags (A/B builds, the negative-control build of
            # tests/test_extremes_gpu.py): loaded as it is, never rebuilt; a missing file is an OSError
            path = override
        elif _build.stale():
            if os.path.exists(_build.HIPCC):
                _build.build(verbose=False)
            elif not os.path.exists(path):
                raise ImportError("libwayne_hip.so is not built and hipcc is unavailable (%s)" % _build.HIPCC)
        L = C.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            f = getattr(L, name)  # AttributeError if the ABI lost a symbol
            f.restype = res
            f.argtypes = args
        if L.wayne_abi_version() != ABI_VERSION:
            raise ImportError("libwayne_hip.so ABI version mismatch")
        flags = L.wayne_build_flags().decode().split()
        if flags and os.environ.get("WAYNE_ALLOW_FLAGGED_LIB", "") != "1":
            # a negative-control or timing build (its sources say "wrong frames"): never by accident
            raise ImportError("%s was built with %s: not the product's library (tests and measurement scripts that mean "
                              "to load it set WAYNE_ALLOW_FLAGGED_LIB=1)" % (path, " ".join(flags)))
        _lib = L
        _lib_path = path
    return _lib


_lib_path = None


def library_info():
    """(path, build flags) of the loaded library: what a measurement or a written file names as its producer."""
    L = load()
    return _lib_path or _build.LIB, L.wayne_build_flags().decode().strip()


def ptr(a, ctype=None):
    """Raw pointer of a C-contiguous numpy array (None -> NULL)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    if ctype is None:
        return a.ctypes.data_as(C.c_void_p)
    return a.ctypes.data_as(C.POINTER(ctype))


def out_dtype_of(flags):
    """The numpy dtype of the reads a descriptor with these flags delivers."""
    return np.dtype(np.float64 if flags & F_OUT_F64 else np.uint16 if flags & F_OUT_U16 else np.float32)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


KNOBS = ("tile_ints", "batch", "thin", "no_acc_box", "lane_reach", "throw_wgs", "keep_narrow", "no_fuse", "fork_narrow",
         "streams", "upload_timing", "ramp_reads", "narrow_compact", "lane_tight_tile",
         "fuse_thrower", "prep_wl_per_run")
_live_contexts = weakref.WeakSet()
_knob_defaults = {}


def set_knob_all(name, value):
    """Set a tuning / test knob on every live context of this process and on those created later (None: back to the
    library's own choice).  The explicit, per-process replacement of editing WAYNE_* environment variables under a
    running context -- the library reads those once, in wayne_ctx_create."""
    if name not in KNOBS:
        raise KeyError("no knob named %r" % (name,))
    if value is None:
        _knob_defaults.pop(name, None)
    else:
        _knob_defaults[name] = int(value)
    for c in list(_live_contexts):
        if getattr(c, "_h", None):
            c.set_knob(name, value)


def reset_knobs_all():
    for name in list(_knob_defaults):
        set_knob_all(name, None)


class Context(object):
    """One wayne_ctx: a GPU, a HIP stream and the HBM buffers of the path."""

    def __init__(self, device=0):
        self._L = load()
        st = C.c_int(0)
        self._h = self._L.wayne_ctx_create(int(device), C.byref(st))
        if not self._h:
            msg = self._L.wayne_strerror(st.value).decode()
            cls = WayneNoDeviceError if st.value == E_NODEVICE else WayneError
            raise cls(st.value, "wayne_ctx_create(device=%d): %s -- the HIP path is the only path, "
                                "there is no CPU fallback" % (device, msg))
        self.device = device
        self._slot_meta = {}     # slot -> (K, W, R, dtype of the reads) of the descriptor uploaded last
        self._slot_src = {}      # slot -> bins of each of its contaminants
        self._slot_crrej = set() # slots whose extraction rejects cosmic rays
        self._slot_chan = {}     # slot -> channels of its extraction (set_channels succeeded)
        self._slot_var = set()   # slots whose extraction delivers variances (set_variance succeeded)
        self._slot_opt = set()   # slots whose extraction delivers the optimal values too (set_optimal succeeded)
        self._slot_optch = set() # slots whose extraction delivers the optimal channels (set_optimal_channels succeeded)
        self._slot_prof = set()  # slots whose runs write the profile planes too (deliver_profile succeeded)
        self._slot_fits = {}     # slot -> (plane_bytes, stride, bitpix) of its FITS payload (set_fits succeeded)
        self._slot_expected = {} # slot -> mode name of its expected image (set_expected succeeded)
        self._slot_rampfit = {}  # slot -> rampfit.RampFit of its ramp fit (set_rampfit succeeded)
        self._slot_ima = {}      # slot -> (ima.Ima, ima.Layout) of its calibrated reads (set_ima succeeded)
        _live_contexts.add(self)
        for name, value in _knob_defaults.items():
            self.set_knob(name, value)

    def close(self):
        if getattr(self, "_h", None):
            self._L.wayne_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def check(self, status):
        if status != OK:
            raise WayneError(status, self._L.wayne_last_error(self._h).decode())

    def synchronize(self):
        """Wait for everything enqueued and settle it: afterwards every slot's reads are complete (an exposure that
        met a bin beyond its launch sequence's reach has been run a second time; see wayne_ctx_synchronize)."""
        self.check(self._L.wayne_ctx_synchronize(self._h))

    def set_knob(self, name, value):
        """Tuning / test knob of THIS context (value None or < 0: the library's own choice).  The environment
        (WAYNE_<NAME>) is read once, at creation."""
        self.check(self._L.wayne_ctx_set_knob(self._h, name.encode(), -1 if value is None else int(value)))

    def get_knob(self, name):
        v = C.c_longlong(0)
        self.check(self._L.wayne_ctx_get_knob(self._h, name.encode(), C.byref(v)))
        return None if v.value < 0 else int(v.value)

    @property
    def stream(self):
        return self._L.wayne_ctx_stream(self._h)

    # -- inner boundary -----------------------------------------------------
    def psf_apply(self, counts, x, y, ratio, sl, sh, nr, nc, seed, threads=1, rng_mode=RNG_REPLAY,
                  exposure=0, subsample=0, exact_samplers=False):
        counts = i32(counts)
        x, y, ratio, sl, sh = f64(x), f64(y), f64(ratio), f64(sl), f64(sh)
        n = counts.size
        if not all(a.size == n for a in (x, y, ratio, sl, sh)):
            raise ValueError("apply_psf: arrays differ in length")
        out = np.empty(max(int(nr) * int(nc), 0), dtype=np.int32)
        self.check(self._L.wayne_psf_apply_ex(self._h, ptr(counts), n, ptr(x), ptr(y), ptr(ratio), ptr(sl),
                                              ptr(sh), int(nr), int(nc), int(seed) & 0xFFFFFFFF, int(threads),
                                              int(rng_mode), int(exposure), int(subsample),
                                              F_EXACT_SAMPLERS if exact_samplers else 0, ptr(out)))
        return out

    # -- grism / calibration --------------------------------------------------
    def set_grism(self, trace_coeff, wl_solution, psf_ratio_poly, psf_sigmal_poly, psf_sigmah_poly,
                  sens_wl_um, sens_val, flat_wmin, flat_wmax):
        g = GrismDesc()
        g.trace_coeff[:] = list(map(float, trace_coeff))
        g.wl_solution[:] = list(map(float, wl_solution))
        g.psf_ratio_poly[:] = list(map(float, psf_ratio_poly))
        g.psf_sigmal_poly[:] = list(map(float, psf_sigmal_poly))
        g.psf_sigmah_poly[:] = list(map(float, psf_sigmah_poly))
        wl, val = f64(sens_wl_um), f64(sens_val)
        if wl.size != val.size:
            raise ValueError("sensitivity table: wl and val differ in length")
        g.n_sens = wl.size
        g.sens_wl_um = ptr(wl, C.c_double)
        g.sens_val = ptr(val, C.c_double)
        g.flat_wmin, g.flat_wmax = float(flat_wmin), float(flat_wmax)
        self.check(self._L.wayne_ctx_set_grism(self._h, C.byref(g)))

    def set_calibration(self, subarray, n_reads, flat=None, pfl=None, sky=None, lin=None, dark_sci=None,
                        dark_err=None, zero_read=None):
        N = 1014 if subarray == 1024 else subarray
        S = N + 10
        k = Calibration()
        k.subarray, k.n_reads = int(subarray), int(n_reads)
        keep = []

        def plane(a, shape, name, dt=np.float32):
            a = np.ascontiguousarray(a, dtype=dt)
            if a.shape != shape:
                raise ValueError("%s: expected shape %s, got %s" % (name, shape, a.shape))
            keep.append(a)
            return a

        if flat is not None:
            for i in range(4):
                k.flat[i] = ptr(plane(flat[i], (N, N), "flat[%d]" % i), C.c_float)
        if pfl is not None:
            k.pfl = ptr(plane(pfl, (N, N), "pfl"), C.c_float)
        if sky is not None:
            k.sky = ptr(plane(sky, (N, N), "sky"), C.c_float)
        if lin is not None:
            for i in range(4):
                k.lin[i] = ptr(plane(lin[i], (S, S), "lin[%d]" % i), C.c_float)
        if dark_sci is not None and dark_err is not None:
            k.dark_sci = ptr(plane(dark_sci, (n_reads, S, S), "dark_sci"), C.c_float)
            k.dark_err = ptr(plane(dark_err, (n_reads, S, S), "dark_err"), C.c_float)
        if zero_read is not None:
            k.zero_read = ptr(plane(zero_read, (S, S), "zero_read", np.float64), C.c_double)
        self.check(self._L.wayne_ctx_set_calibration(self._h, C.byref(k)))
        self.N, self.S, self.R = N, S, int(n_reads)

    # -- exposures -------------------------------------------------------------
    def make_desc(self, *a, **k):
        return make_desc(*a, **k)

    def upload(self, slot, desc):
        """Stage the descriptor in `slot`; contaminants and charge traps it carries (make_desc(sources=..., traps=...))
        are set with it, and with traps.CarriedTraps their history (set_trap_history)."""
        self.check(self._L.wayne_exposure_upload(self._h, int(slot), C.byref(desc)))
        self._slot_meta[slot] = (desc.n_samples, desc.n_wl, desc.n_reads, out_dtype_of(desc.flags))
        self._slot_src[slot] = ()
        self._slot_crrej.discard(slot)
        self._slot_chan.pop(slot, None)
        self._slot_var.discard(slot)
        self._slot_opt.discard(slot)
        self._slot_prof.discard(slot)
        self._slot_optch.discard(slot)
        self._slot_fits.pop(slot, None)
        self._slot_expected.pop(slot, None)
        self._slot_rampfit.pop(slot, None)
        self._slot_ima.pop(slot, None)
        sources = getattr(desc, "_sources", None)
        if sources:
            self.set_sources(slot, sources)
        traps = getattr(desc, "_traps", None)
        if traps is not None:
            self.set_traps(slot, traps)
            if getattr(traps, "gap_s", None) is not None:      # traps.CarriedTraps: the history rides with the traps
                self.set_trap_history(slot, traps)
        extraction = getattr(desc, "_extraction", None)
        if extraction is not None:
            self.set_extraction(slot, extraction)
        if getattr(desc, "_device_fits", False):
            self.set_fits(slot)
        expected = getattr(desc, "_expected", None)
        if expected is not None:
            self.set_expected(slot, expected)
        ramp_fit = getattr(desc, "_ramp_fit", None)
        if ramp_fit is not None:
            self.set_rampfit(slot, ramp_fit)
        ima = getattr(desc, "_ima", None)
        if ima is not None:
            self.set_ima(slot, ima)
        ld_table = getattr(desc, "_ld_table", None)
        if ld_table is not None:
            self.set_limb_darkening(slot, ld_table)
        ipc = getattr(desc, "_ipc", None)
        if ipc is not None:
            self.set_ipc(slot, ipc)
        lc_spots = getattr(desc, "_spots", None)       # (behind the table: the spots are checked against its coefficients)
        if lc_spots is not None:
            self.set_spots(slot, lc_spots)

    # -- star spots ------------------------------------------------------------------
    def set_spots(self, slot, geometry):
        """Star spots in the slot's device light curve (spots.SpotGeometry: the planet's track [K], centres, radii and
        the contrast [n, W]); k_lightcurve_spots then rewrites the depth matrix behind the light-curve launch.  None
        clears; after upload, which clears it too, and after set_limb_darkening.  See wayne_exposure_set_spots."""
        if geometry is None:
            self.check(self._L.wayne_exposure_set_spots(self._h, int(slot), None, 0, 0))
            return
        n = int(geometry.n)
        if n > 8:
            raise ValueError("set_spots: at most 8 spots, got %d" % n)
        contrast, px, py = f64(geometry.contrast), f64(geometry.X), f64(geometry.Y)
        if contrast.ndim != 2 or contrast.shape[0] != n or px.shape != py.shape or px.ndim != 1:
            raise ValueError("set_spots: contrast [n, W] and a track X, Y [K] are expected")
        d = SpotsDesc()
        d.n = n
        for i in range(n):
            d.cx[i], d.cy[i], d.radius[i] = float(geometry.cx[i]), float(geometry.cy[i]), float(geometry.radius[i])
        d.contrast, d.px, d.py = ptr(contrast, C.c_double), ptr(px, C.c_double), ptr(py, C.c_double)
        self.check(self._L.wayne_exposure_set_spots(self._h, int(slot), C.byref(d), contrast.shape[1], px.size))

    def _kernel_profile(self, which, as_dict=True):
        """wayne_<which>_profile: launches and milliseconds by HIP events since profile_reset."""
        n, ms = C.c_uint64(0), C.c_double(0.0)
        self.check(getattr(self._L, "wayne_%s_profile" % which)(self._h, C.byref(n), C.byref(ms)))
        return {"launches": int(n.value), "ms": float(ms.value)} if as_dict else (int(n.value), float(ms.value))

    def spots_profile(self):
        """(launches, total milliseconds) of k_lightcurve_spots since profile_reset.  See wayne_spots_profile."""
        return self._kernel_profile("spots", as_dict=False)

    # -- limb darkening per wavelength bin -------------------------------------------
    def set_limb_darkening(self, slot, ld):
        """Claret coefficients per wavelength bin of the slot's device light curve, an array [W, 4] (k_lightcurve_ld in
        place of k_lightcurve); None clears; after upload, which clears it too.  See wayne_exposure_set_limb_darkening."""
        if ld is None:
            self.check(self._L.wayne_exposure_set_limb_darkening(self._h, int(slot), None, 0))
            return
        ld = f64(ld)
        if ld.ndim != 2 or ld.shape[1] != 4:
            raise ValueError("set_limb_darkening: expected an array [W, 4], got shape %s" % (ld.shape,))
        self.check(self._L.wayne_exposure_set_limb_darkening(self._h, int(slot), ptr(ld, C.c_double), ld.shape[0]))

    # -- the noise-free expected image ---------------------------------------------
    def set_expected(self, slot, mode):
        """Every run of the slot also renders its noise-free expected image: mode "counts" (the conditional expectation
        of the accumulators given the bin counts the run drew) or "mean" (the unconditional one); None clears; after
        upload, which clears it too.  See wayne_exposure_set_expected."""
        self._slot_expected.pop(slot, None)
        code = expected_mode(mode)
        self.check(self._L.wayne_exposure_set_expected(self._h, int(slot), code))
        if code:
            self._slot_expected[slot] = EXPECT_NAMES[code]

    def has_expected(self, slot):
        """Whether the slot's runs render the expected image (set_expected succeeded since its last upload)."""
        return slot in self._slot_expected

    def expected(self, slot):
        """The slot's expected image [R, S, S] float64, in electrons per read interval (not cumulative), blocking:
        waits for the slot's run and settles it as download() does."""
        K, W, R, _ = self._slot_meta[slot]
        if slot not in self._slot_expected:
            raise WayneError(E_STATE, "expected: no expected image set for the slot")
        out = np.empty((R, self.S, self.S), dtype=np.float64)
        self.check(self._L.wayne_exposure_download_expected(self._h, int(slot), ptr(out, C.c_double)))
        return out

    def expected_profile(self):
        """{"launches", "ms"} of k_expect by HIP events (profile_enable; since profile_reset)."""
        return self._kernel_profile("expected")

    # -- the ramp fit --------------------------------------------------------------
    def set_rampfit(self, slot, ramp_fit):
        """Every run of the slot also fits its ramps (k_ramp_fit): a rampfit.RampFit, True for its defaults; None or
        False clears; after upload, which clears it too.  A refusal leaves the slot running without the fit.  See
        wayne_exposure_set_rampfit."""
        from . import rampfit as _rampfit
        self._slot_rampfit.pop(slot, None)
        fit = _rampfit.as_ramp_fit(ramp_fit)
        if fit is None:
            self.check(self._L.wayne_exposure_set_rampfit(self._h, int(slot), None))
            return
        d = fit.desc()
        self.check(self._L.wayne_exposure_set_rampfit(self._h, int(slot), C.byref(d)))
        self._slot_rampfit[slot] = fit

    def has_rampfit(self, slot):
        """Whether the slot's runs fit its ramps (set_rampfit succeeded since its last upload)."""
        return slot in self._slot_rampfit

    def rampfit(self, slot):
        """The slot's (rate [S, S] float64 in e-/s, var [S, S] float64, word [S, S] uint32 = K << 16 | jump), blocking:
        waits for the slot's run and settles it as download() does."""
        if slot not in self._slot_rampfit:
            raise WayneError(E_STATE, "rampfit: no ramp fit set for the slot")
        rate = np.empty((self.S, self.S), dtype=np.float64)
        var = np.empty((self.S, self.S), dtype=np.float64)
        word = np.empty((self.S, self.S), dtype=np.uint32)
        self.check(self._L.wayne_exposure_download_rampfit(self._h, int(slot), ptr(rate, C.c_double), ptr(var, C.c_double),
                                                           ptr(word, C.c_uint32)))
        return rate, var, word

    def rampfit_profile(self):
        """{"launches", "ms"} of k_ramp_fit by HIP events (profile_enable; since profile_reset)."""
        return self._kernel_profile("rampfit")

    # -- the calibrated reads ------------------------------------------------------
    def set_ima(self, slot, ima):
        """Every run of the slot also forms its calibrated reads (k_ima): an ima.Ima, True for its defaults, "rate" or
        "counts"; None or False clears; after upload, which clears it too.  A refusal leaves the slot running without the
        option.  See wayne_exposure_set_ima."""
        from . import ima as _ima
        self._slot_ima.pop(slot, None)
        opt = _ima.as_ima(ima)
        if opt is None:
            self.check(self._L.wayne_exposure_set_ima(self._h, int(slot), None))
            return
        d = opt.desc()
        self.check(self._L.wayne_exposure_set_ima(self._h, int(slot), C.byref(d)))
        K, W, R, _ = self._slot_meta[slot]
        self._slot_ima[slot] = (opt, _ima.layout(self.S, R))

    def has_ima(self, slot):
        """Whether the slot's runs form its calibrated reads (set_ima succeeded since its last upload)."""
        return slot in self._slot_ima

    def ima(self, slot):
        """The slot's calibrated reads, blocking: an ima.Payload -- the payload as one uint8 array of the caller's own
        with sci(k) / err(k) / dq(k) views of it.  Waits for the slot's run and settles it as download() does."""
        from . import ima as _ima
        if slot not in self._slot_ima:
            raise WayneError(E_STATE, "ima: no calibrated reads set for the slot")
        opt, lay = self._slot_ima[slot]
        buf = np.empty(lay.nbytes, dtype=np.uint8)
        self.check(self._L.wayne_exposure_download_ima(self._h, int(slot), buf.ctypes.data_as(C.c_void_p)))
        return _ima.Payload(buf, lay, opt)

    def ima_profile(self):
        """{"launches", "ms"} of k_ima by HIP events (profile_enable; since profile_reset)."""
        return self._kernel_profile("ima")

    # -- device-side FITS words ----------------------------------------------------
    def set_fits(self, slot, on=True):
        """Every run of the slot also forms its reads' FITS words on the device (on=False clears; after upload, which
        clears it too).  See wayne_exposure_set_fits."""
        self._slot_fits.pop(slot, None)
        self.check(self._L.wayne_exposure_set_fits(self._h, int(slot), 1 if on else 0))
        if on:
            K, W, R, dtype = self._slot_meta[slot]
            self._slot_fits[slot] = fits_layout(self.S, R, dtype)

    def has_fits(self, slot):
        """Whether the slot's runs form FITS words (set_fits succeeded since its last upload)."""
        return slot in self._slot_fits

    def fits_layout_of(self, slot):
        """(plane_bytes, stride, bitpix) of the slot's payload (fits_layout); KeyError without set_fits."""
        return self._slot_fits[slot]

    def fetch_fits_async(self, slot):
        """Enqueue the copy of the slot's FITS words into their pinned host mirror (returns at once)."""
        self.check(self._L.wayne_exposure_fetch_fits_async(self._h, int(slot)))

    def wait_fits(self, slot):
        """Block until the slot's work is done -> its payload, (R + 1) * stride bytes, as a uint8 numpy VIEW of the pinned
        mirror (valid until the slot's next fetch_fits_async or upload)."""
        p = C.c_void_p()
        self.check(self._L.wayne_exposure_wait_fits(self._h, int(slot), C.byref(p)))
        K, W, R, _ = self._slot_meta[slot]
        n = (R + 1) * self._slot_fits[slot][1]
        return np.frombuffer((C.c_ubyte * n).from_address(p.value), dtype=np.uint8)

    def download_fits(self, slot):
        """The slot's payload, blocking; a uint8 array of the caller's own."""
        K, W, R, _ = self._slot_meta[slot]
        if slot not in self._slot_fits:
            raise WayneError(E_STATE, "download_fits: no FITS words set for the slot")
        out = np.empty((R + 1) * self._slot_fits[slot][1], dtype=np.uint8)
        self.check(self._L.wayne_exposure_download_fits(self._h, int(slot), ptr(out)))
        return out

    def fits_profile(self):
        """{"launches", "ms"} of k_fits_words by HIP events (profile_enable; since profile_reset)."""
        return self._kernel_profile("fits")

    def set_crrej(self, slot, crrej):
        """Cosmic-ray rejection of the slot's extraction: an extraction.CosmicRejection (k, read_noise) -- None clears;
        after set_extraction, which clears it too.  See wayne_exposure_set_crrej."""
        self._slot_crrej.discard(slot)           # (a refusal leaves the slot extracting without rejection)
        if crrej is None:
            self.check(self._L.wayne_exposure_set_crrej(self._h, int(slot), None))
            return
        self.check(self._L.wayne_exposure_set_crrej(self._h, int(slot), C.byref(crrej.desc())))
        self._slot_crrej.add(slot)

    def has_crrej(self, slot):
        """Whether the slot's extraction rejects cosmic rays (set_crrej succeeded since its last set_extraction)."""
        return slot in self._slot_crrej

    def rejected(self, slot):
        """n_rejected [R + 1] (uint32; a copy) of the slot's last wait_spectra / download_spectra: the flags in each
        product's window, (pixel, interval) pairs for the last-read product."""
        K, W, R, _ = self._slot_meta[slot]
        pn = C.POINTER(C.c_uint32)()
        self.check(self._L.wayne_exposure_rejected(self._h, int(slot), C.byref(pn)))
        return np.ctypeslib.as_array(pn, shape=(R + 1,)).copy()

    def download_crmask(self, slot):
        """The flag plane [S, S] (uint16, bit j = read interval j) of the slot's last run, blocking; 0 outside the mask
        rows."""
        mask = np.empty((self.S, self.S), dtype=np.uint16)
        self.check(self._L.wayne_exposure_download_crmask(self._h, int(slot), ptr(mask)))
        return mask

    def set_extraction(self, slot, extraction):
        """Spectral extraction of the slot's uploaded exposure: an extraction.Extraction (row windows of the R read
        intervals and of the last read, background columns, step mask; its `crrej`, if any, is set with it) -- None clears.  The back half of every run of
        the slot then forms spectra [R + 1, S] and sky [R + 1] on the device.  See wayne_exposure_set_extraction."""
        self._slot_crrej.discard(slot)
        self._slot_chan.pop(slot, None)
        self._slot_var.discard(slot)
        self._slot_opt.discard(slot)
        self._slot_prof.discard(slot)
        self._slot_optch.discard(slot)
        if extraction is None:
            self.check(self._L.wayne_exposure_set_extraction(self._h, int(slot), None))
            return
        self.check(self._L.wayne_exposure_set_extraction(self._h, int(slot), C.byref(extraction.desc())))
        if getattr(extraction, "crrej", None) is not None:
            self.set_crrej(slot, extraction.crrej)
        if getattr(extraction, "channels", None) is not None:
            self.set_channels(slot, extraction.channels, extraction.row_solution)
        if getattr(extraction, "variance", None) is not None:
            self.set_variance(slot, extraction.variance)
        if getattr(extraction, "optimal", None) is not None:
            self.set_optimal(slot, extraction.optimal)

    def set_variance(self, slot, variance):
        """Variances with the slot's extraction: an extraction.Variances (the read noise of a difference of two reads, in
        electrons) or True for its default -- None clears; after set_extraction, which clears it too (set_crrej and
        set_channels do not).  See wayne_exposure_set_variance."""
        self._slot_var.discard(slot)             # (a refusal leaves the slot extracting without variances)
        self._slot_opt.discard(slot)             # (the optimal extraction stands on them: set_optimal comes after)
        self._slot_prof.discard(slot)
        self._slot_optch.discard(slot)
        if variance is None or variance is False:
            self.check(self._L.wayne_exposure_set_variance(self._h, int(slot), None))
            return
        if variance is True:
            d = VarianceDesc(20.0)
        else:
            d = variance.desc() if hasattr(variance, "desc") else VarianceDesc(float(variance))
        self.check(self._L.wayne_exposure_set_variance(self._h, int(slot), C.byref(d)))
        self._slot_var.add(slot)

    def has_variance(self, slot):
        """Whether the slot's extraction delivers variances (set_variance succeeded since its last set_extraction)."""
        return slot in self._slot_var

    def variances(self, slot):
        """(spectra_var [R + 1, S], sky_var [R + 1], channels_var [R + 1, C] or None without channels) -- float64 copies --
        of the slot's last wait_spectra / download_spectra."""
        K, W, R, _ = self._slot_meta[slot]
        ps, pk, pc = _dp(), _dp(), _dp()
        self.check(self._L.wayne_exposure_variances(self._h, int(slot), C.byref(ps), C.byref(pk), C.byref(pc)))
        spectra_var = np.ctypeslib.as_array(ps, shape=(R + 1, self.S)).copy()
        sky_var = np.ctypeslib.as_array(pk, shape=(R + 1,)).copy()
        n_ch = self._slot_chan.get(slot)
        channels_var = np.ctypeslib.as_array(pc, shape=(R + 1, n_ch)).copy() if (pc and n_ch) else None
        return spectra_var, sky_var, channels_var

    def set_optimal(self, slot, optimal):
        """Optimal (profile-weighted) extraction beside the slot's box extraction: an extraction.Optimal (the profile's
        half width in columns), True for its default or an int -- None clears; after set_variance, which clears it too
        (set_crrej and set_channels do not).  See wayne_exposure_set_optimal."""
        self._slot_opt.discard(slot)             # (a refusal leaves the slot extracting without it)
        self._slot_prof.discard(slot)          # (the profile planes and a supplied profile go with it)
        self._slot_optch.discard(slot)
        if optimal is None or optimal is False:
            self.check(self._L.wayne_exposure_set_optimal(self._h, int(slot), None))
            return
        if optimal is True:
            d = OptimalDesc(8)
        else:
            d = optimal.desc() if hasattr(optimal, "desc") else OptimalDesc(int(optimal))
        self.check(self._L.wayne_exposure_set_optimal(self._h, int(slot), C.byref(d)))
        self._slot_opt.add(slot)
        if getattr(optimal, "profile", None) is not None:
            self.set_optimal_profile(slot, optimal.profile)
        if getattr(optimal, "deliver_profile", False):
            self.deliver_profile(slot)
        if getattr(optimal, "channels", False):
            self.set_optimal_channels(slot)

    def has_optimal(self, slot):
        """Whether the slot's extraction delivers the optimal values (set_optimal succeeded since its last set_variance)."""
        return slot in self._slot_opt

    def optimal(self, slot):
        """(optimal [R + 1, S], optimal_var [R + 1, S]) -- float64 copies -- of the slot's last wait_spectra /
        download_spectra."""
        K, W, R, _ = self._slot_meta[slot]
        po, pv = _dp(), _dp()
        self.check(self._L.wayne_exposure_optimal(self._h, int(slot), C.byref(po), C.byref(pv)))
        return (np.ctypeslib.as_array(po, shape=(R + 1, self.S)).copy(),
                np.ctypeslib.as_array(pv, shape=(R + 1, self.S)).copy())

    def set_optimal_profile(self, slot, profile):
        """Extract the slot optimally with a supplied profile: an extraction.Profile (the planes, float64, and the window
        heights they were made for) -- None goes back to the exposure's own profile; after set_optimal, which clears it
        too.  The planes are copied.  A run of a slot whose windows have other heights is refused (E_INVALID).  See
        wayne_exposure_set_optimal_profile."""
        if profile is None:
            self.check(self._L.wayne_exposure_set_optimal_profile(self._h, int(slot), None, None))
            return
        if isinstance(profile, dict):
            raise ValueError("set_optimal_profile: one Profile, not {profile_key: Profile} (extraction.pick_profile chooses)")
        planes = np.ascontiguousarray(profile.planes, dtype=np.float64)
        rows = (C.c_int * len(profile.rows))(*[int(r) for r in profile.rows])
        K, W, R, _ = self._slot_meta[slot]
        if len(profile.rows) != R + 1 or planes.size != sum(profile.rows) * self.S:
            raise ValueError("set_optimal_profile: the profile holds %d windows and %d values; the slot has %d windows of "
                             "%d columns" % (len(profile.rows), planes.size, R + 1, self.S))
        # (the Profile's tag names its content: a slot that already holds it copies nothing)
        self.check(self._L.wayne_exposure_set_optimal_profile_tagged(self._h, int(slot), planes.ctypes.data_as(_dp), rows,
                                                                     int(getattr(profile, "tag", 0))))

    def set_optimal_channels(self, slot, on=True):
        """The optimal channels beside the slot's channels and optimal values (on=False clears; after set_channels and
        set_optimal -- and set_optimal_profile -- which clear them too).  See wayne_exposure_set_optimal_channels."""
        self._slot_optch.discard(slot)
        self.check(self._L.wayne_exposure_set_optimal_channels(self._h, int(slot), 1 if on else 0))
        if on:
            self._slot_optch.add(slot)

    def has_optimal_channels(self, slot):
        return slot in self._slot_optch

    def optimal_channels(self, slot):
        """(channels_opt [R + 1, C], channels_opt_var [R + 1, C]) -- float64 copies -- of the slot's last wait_spectra /
        download_spectra."""
        K, W, R, _ = self._slot_meta[slot]
        pc, pv = _dp(), _dp()
        self.check(self._L.wayne_exposure_optimal_channels(self._h, int(slot), C.byref(pc), C.byref(pv)))
        n_ch = self._slot_chan[slot]
        return (np.ctypeslib.as_array(pc, shape=(R + 1, n_ch)).copy(), np.ctypeslib.as_array(pv, shape=(R + 1, n_ch)).copy())

    def profile_uploads(self):
        """Profiles set_optimal_profile has copied to the device (a slot that already holds the same one copies nothing)."""
        return int(self._L.wayne_ctx_profile_uploads(self._h))

    def deliver_profile(self, slot, on=True):
        """Every run of the slot also writes the profile planes S1 of its windows (on=False clears; after set_optimal,
        which clears it too).  See wayne_exposure_deliver_profile."""
        self._slot_prof.discard(slot)
        self.check(self._L.wayne_exposure_deliver_profile(self._h, int(slot), 1 if on else 0))
        if on:
            self._slot_prof.add(slot)

    def delivers_profile(self, slot):
        """Whether the slot's runs write profile planes (deliver_profile succeeded since its last set_optimal)."""
        return slot in self._slot_prof

    def fetch_profile(self, slot):
        """Enqueue the copy of the slot's profile planes into pinned host memory (returns at once); after the run's
        wait_spectra / download_spectra."""
        self.check(self._L.wayne_exposure_fetch_profile(self._h, int(slot)))

    def profile_planes(self, slot):
        """The planes fetch_profile asked for (it is called here if nobody has), blocking: a float64 copy [sum_p rows_p,
        S], the windows of the R + 1 products one behind the other."""
        pp, n = _dp(), C.c_size_t(0)
        rc = self._L.wayne_exposure_profile(self._h, int(slot), C.byref(pp), C.byref(n))
        if rc == E_STATE and slot in self._slot_prof:
            self.fetch_profile(slot)
            rc = self._L.wayne_exposure_profile(self._h, int(slot), C.byref(pp), C.byref(n))
        self.check(rc)
        if n.value == 0:
            return np.zeros((0, self.S))
        return np.ctypeslib.as_array(pp, shape=(n.value // self.S, self.S)).copy()

    def set_channels(self, slot, channels, row_solution=None):
        """Wavelength-binned channels of the slot's extraction: an extraction.Channels (edges in um, flat on / off) and
        the rows' wavelength solution (wl_a [S], wl_b [S]): lambda_y(u) = wl_a[y] + wl_b[y] u at bordered column
        coordinate u -- None clears; after set_extraction, which clears it too (set_crrej does not).  The arrays are
        copied.  See wayne_exposure_set_channels."""
        self._slot_chan.pop(slot, None)          # (a refusal leaves the slot extracting without channels)
        self._slot_optch.discard(slot)           # (the optimal channels are the channels': set_optimal_channels comes after)
        if channels is None:
            self.check(self._L.wayne_exposure_set_channels(self._h, int(slot), None))
            return
        if row_solution is None:
            raise ValueError("set_channels: the rows' wavelength solution (wl_a, wl_b) is needed")
        edges = np.ascontiguousarray(channels.edges_um, dtype=np.float64)
        wl_a = np.ascontiguousarray(row_solution[0], dtype=np.float64)
        wl_b = np.ascontiguousarray(row_solution[1], dtype=np.float64)
        if wl_a.shape != (self.S,) or wl_b.shape != (self.S,):
            raise ValueError("set_channels: wl_a and wl_b must have one entry per bordered row (%d)" % self.S)
        d = ChannelsDesc()
        d.n_channels = len(edges) - 1
        d.edges_um, d.wl_a, d.wl_b = edges.ctypes.data_as(_dp), wl_a.ctypes.data_as(_dp), wl_b.ctypes.data_as(_dp)
        d.flags = C_FLAT if channels.flat else 0
        self.check(self._L.wayne_exposure_set_channels(self._h, int(slot), C.byref(d)))
        self._slot_chan[slot] = d.n_channels

    def has_channels(self, slot):
        """Whether the slot's extraction is binned into channels (set_channels succeeded since its last set_extraction)."""
        return slot in self._slot_chan

    def channels(self, slot):
        """channels [R + 1, C] (float64; a copy) of the slot's last wait_spectra / download_spectra."""
        K, W, R, _ = self._slot_meta[slot]
        pc = _dp()
        self.check(self._L.wayne_exposure_channels(self._h, int(slot), C.byref(pc)))
        n_ch = self._slot_chan.get(slot)
        if n_ch is None:
            raise WayneError(-7, "channels: no channels set for the slot")
        return np.ctypeslib.as_array(pc, shape=(R + 1, n_ch)).copy()

    def fetch_spectra_async(self, slot):
        """Enqueue the copy of the slot's spectra (never its reads) into pinned host memory (returns at once)."""
        self.check(self._L.wayne_exposure_fetch_spectra_async(self._h, int(slot)))

    def wait_spectra(self, slot):
        """Block until the slot's work is done -> (spectra [R + 1, S], sky [R + 1]) as numpy VIEWS of the pinned buffer
        (valid until the slot is uploaded again; copy them to keep them)."""
        K, W, R, _ = self._slot_meta[slot]
        ps, pk = _dp(), _dp()
        self.check(self._L.wayne_exposure_wait_spectra(self._h, int(slot), C.byref(ps), C.byref(pk)))
        spectra = np.ctypeslib.as_array(ps, shape=(R + 1, self.S))
        sky = np.ctypeslib.as_array(pk, shape=(R + 1,))
        return spectra, sky

    def download_spectra(self, slot):
        """(spectra [R + 1, S], sky [R + 1]) of the slot, blocking; arrays of the caller's own."""
        K, W, R, _ = self._slot_meta[slot]
        spectra = np.empty((R + 1, self.S), dtype=np.float64)
        sky = np.empty(R + 1, dtype=np.float64)
        self.check(self._L.wayne_exposure_download_spectra(self._h, int(slot), ptr(spectra), ptr(sky)))
        return spectra, sky

    def extract_profile(self):
        """{"launches", "ms"} of the extraction's kernels by HIP events (profile_enable; since profile_reset)."""
        return self._kernel_profile("extract")

    def set_ipc(self, slot, ipc):
        """Inter-pixel capacitance of the slot's uploaded exposure: an ipc.InterpixelCapacitance (or a 3 x 3 array of
        weights) -- None clears.  See wayne_exposure_set_ipc."""
        if ipc is None:
            self.check(self._L.wayne_exposure_set_ipc(self._h, int(slot), None))
            return
        self.check(self._L.wayne_exposure_set_ipc(self._h, int(slot), C.byref(ipc_desc(ipc))))

    def ipc_profile(self):
        """(coupled exposures, total milliseconds) of k_ipc and k_ipc_clear since profile_reset.  See wayne_ipc_profile."""
        return self._kernel_profile("ipc", as_dict=False)

    def set_traps(self, slot, traps):
        """Charge traps of the slot's uploaded exposure: a traps.ExposureTraps (the model and this exposure's start tables
        [2, G]) -- None clears.  See wayne_exposure_set_traps."""
        if traps is None:
            self.check(self._L.wayne_exposure_set_traps(self._h, int(slot), None))
            return
        m, table = traps.traps, np.ascontiguousarray(traps.table, dtype=np.float64)
        if table.ndim != 2 or table.shape[0] != 2:
            raise ValueError("charge traps: the start tables have shape (2, G)")
        t = TrapDesc()
        t.n_traps[:] = [float(v) for v in m.array("n_traps")]
        t.efficiency[:] = [float(v) for v in m.array("efficiency")]
        t.lifetime_s[:] = [float(v) for v in m.array("lifetime_s")]
        t.n_rate, t.rate_lo, t.rate_hi = int(table.shape[1]), float(m.rate_lo), float(m.rate_hi)
        rows = [np.ascontiguousarray(table[0]), np.ascontiguousarray(table[1])]
        t.start[0], t.start[1] = ptr(rows[0], C.c_double), ptr(rows[1], C.c_double)
        self.check(self._L.wayne_exposure_set_traps(self._h, int(slot), C.byref(t)))

    def set_trap_history(self, slot, history):
        """A carried history of the slot's trapped exposure: an object with gap_s, lit and fill [2] (traps.CarriedTraps) --
        None clears; after set_traps, which clears it too.  The exposure then starts from the context's trap state and
        leaves its own behind.  See wayne_exposure_set_trap_history."""
        if history is None:
            self.check(self._L.wayne_exposure_set_trap_history(self._h, int(slot), None))
            return
        h = TrapHistoryDesc()
        h.gap_s, h.lit = float(history.gap_s), int(bool(history.lit))
        h.fill[:] = [float(v) for v in history.fill]
        self.check(self._L.wayne_exposure_set_trap_history(self._h, int(slot), C.byref(h)))

    def trap_state_reset(self, initial):
        """Every pixel of the context's trap state := initial (slow, fast).  See wayne_ctx_trap_state_reset."""
        v = (C.c_double * 2)(float(initial[0]), float(initial[1]))
        self.check(self._L.wayne_ctx_trap_state_reset(self._h, v))

    def trap_state_upload(self, state):
        """The context's trap state from a [S, S, 2] float32 array (bordered coordinates; [..., 0] slow, [..., 1] fast)."""
        if not getattr(self, "S", 0):
            raise WayneError(E_STATE, "trap_state_upload: set the calibration first")
        state = np.ascontiguousarray(state, dtype=np.float32)
        if state.shape != (self.S, self.S, 2):
            raise ValueError("trap state: expected shape (%d, %d, 2), got %s" % (self.S, self.S, state.shape))
        self.check(self._L.wayne_ctx_trap_state_upload(self._h, state.ctypes.data_as(C.c_void_p)))

    def trap_state_download(self):
        """The context's trap state, [S, S, 2] float32."""
        if not getattr(self, "S", 0):
            raise WayneError(E_STATE, "trap_state_download: set the calibration first")
        out = np.empty((self.S, self.S, 2), dtype=np.float32)
        self.check(self._L.wayne_ctx_trap_state_download(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def set_sources(self, slot, sources):
        """Contaminating field stars of the slot's uploaded exposure: a sequence of objects with tag, wl, flux, dx, dy
        (sources.Contaminant) -- [] clears.  See wayne_exposure_set_sources."""
        sources = list(sources)
        arr = (SourceDesc * max(len(sources), 1))()
        keep = []
        for i, s in enumerate(sources):
            wl, fl = f64(s.wl), f64(s.flux)
            if wl.size != fl.size:
                raise ValueError("contaminant %d: wl and flux differ in length" % i)
            keep += [wl, fl]
            arr[i].tag, arr[i].n_wl = int(s.tag), wl.size
            arr[i].wl_um, arr[i].flux = ptr(wl, C.c_double), ptr(fl, C.c_double)
            arr[i].dx, arr[i].dy = float(s.dx), float(s.dy)
        self._slot_src[slot] = ()        # (a refused list leaves the slot with the target alone)
        self.check(self._L.wayne_exposure_set_sources(self._h, int(slot), arr, len(sources)))
        self._slot_src[slot] = tuple(int(k.size) for k in keep[0::2])

    def debug_fetch_source(self, slot, source):
        """(counts, x_pos, y_pos) [K, W_i] of source `source` of the slot's last run (0 = the target)."""
        K, W, R, _ = self._slot_meta[slot]
        if source > 0:
            W = self._slot_src[slot][source - 1]
        counts = np.empty((K, W), dtype=np.int32)
        x = np.empty((K, W), dtype=np.float64)
        y = np.empty((K, W), dtype=np.float64)
        self.check(self._L.wayne_exposure_debug_fetch_source(self._h, int(slot), int(source), ptr(counts), ptr(x), ptr(y)))
        return counts, x, y

    def run(self, slot):
        self.check(self._L.wayne_exposure_run(self._h, int(slot)))

    def run_checked(self, slot):
        """run + wait for the slot + settle it: its reads in HBM are complete on return."""
        self.check(self._L.wayne_exposure_run_checked(self._h, int(slot)))

    def run_front(self, slot):
        self.check(self._L.wayne_exposure_run_front(self._h, int(slot)))

    def run_back(self, slot):
        self.check(self._L.wayne_exposure_run_back(self._h, int(slot)))

    def ramp_variant(self, slot):
        """Name of the k_ramp instantiation the slot's back half launches, as a kernel trace prints it."""
        buf = C.create_string_buffer(128)
        self.check(self._L.wayne_exposure_ramp_variant(self._h, int(slot), buf, len(buf)))
        return buf.value.decode()

    def status(self, slot):
        """Status word of the slot's last run (0 = complete; see wayne_exposure_status).  Synchronises."""
        st = C.c_int(0)
        self.check(self._L.wayne_exposure_status(self._h, int(slot), C.byref(st)))
        return st.value

    @property
    def reruns(self):
        """Exposures this context ran a second time (a bin beyond the first launch sequence's reach)."""
        return int(self._L.wayne_ctx_reruns(self._h))

    def download(self, slot):
        K, W, R, dtype = self._slot_meta[slot]
        out = np.empty((R + 1, self.S, self.S), dtype=dtype)
        self.check(self._L.wayne_exposure_download(self._h, int(slot), ptr(out)))
        return out

    def fetch_async(self, slot):
        """Enqueue the copy of the slot's reads into its pinned host buffer (returns at once)."""
        self.check(self._L.wayne_exposure_fetch_async(self._h, int(slot)))

    def wait(self, slot):
        """Block until the slot's work is done -> its reads as a numpy VIEW of the pinned buffer
        (valid until the slot is uploaded again; copy it to keep it)."""
        K, W, R, dtype = self._slot_meta[slot]
        p = C.c_void_p()
        self.check(self._L.wayne_exposure_wait(self._h, int(slot), C.byref(p)))
        n = (R + 1) * self.S * self.S
        buf = (C.c_ubyte * (n * dtype.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype).reshape(R + 1, self.S, self.S)

    def synthesize(self, desc):
        self.upload(0, desc)
        self.run(0)
        return self.download(0)

    def debug_depth(self, slot):
        K, W, R, _ = self._slot_meta[slot]
        out = np.empty((K, W), dtype=np.float64)
        self.check(self._L.wayne_exposure_debug_depth(self._h, int(slot), ptr(out)))
        return out

    def debug_boxes(self, slot):
        """(use_box, boxes[16, 4], segments[16]): which accumulators k_ramp loads for the slot's exposure."""
        boxes = np.zeros((16, 4), dtype=np.int32)
        seg = np.zeros(16, dtype=np.int32)
        use = C.c_int(0)
        self.check(self._L.wayne_exposure_debug_boxes(self._h, int(slot), ptr(boxes), ptr(seg), C.byref(use)))
        return bool(use.value), boxes, seg

    def debug_fetch(self, slot, acc=False):
        K, W, R, _ = self._slot_meta[slot]
        counts = np.empty((K, W), dtype=np.int32)
        x = np.empty((K, W), dtype=np.float64)
        y = np.empty((K, W), dtype=np.float64)
        a = np.empty((R, self.S, self.S), dtype=np.float64) if acc else None
        self.check(self._L.wayne_exposure_debug_fetch(self._h, int(slot), ptr(counts), ptr(x), ptr(y), ptr(a)))
        return counts, x, y, a

    # -- measurement -----------------------------------------------------------
    def profile_enable(self, on=True):
        self.check(self._L.wayne_profile_enable(self._h, 1 if on else 0))

    def profile_select(self, names=None):
        """Time only the named kernels (e.g. ["k_ramp"]; "k_extract": the extraction, extract_profile); None = all."""
        if names is None:
            mask = 0xFFFFFFFF
        else:
            order = list(self.profile_get().keys())[:PROF_KERNELS] + ["k_extract", "k_fits_words", "k_expect", "k_ramp_fit", "k_ima", "k_ipc",
                                                                     "k_lightcurve_spots"]
            mask = 0
            for n in names:
                mask |= 1 << order.index(n)
        self.check(self._L.wayne_profile_select(self._h, mask))

    def profile_reset(self):
        self.check(self._L.wayne_profile_reset(self._h))

    def profile_get(self):
        p = Profile()
        self.check(self._L.wayne_profile_get(self._h, C.byref(p)))
        out = {}
        for i in range(PROF_KERNELS):
            out[p.name[i].decode()] = {"launches": int(p.launches[i]), "ms": float(p.ms[i])}
        out["electrons"] = int(p.electrons)
        return out


def ipc_desc(ipc):
    """ipc.InterpixelCapacitance, or a 3 x 3 array of weights -> IpcDesc."""
    k = np.asarray(getattr(ipc, "kernel", ipc), dtype=np.float64)
    if k.shape != (3, 3):
        raise ValueError("inter-pixel capacitance: the kernel has shape (3, 3), got %s" % (k.shape,))
    d = IpcDesc()
    for i in range(3):
        for j in range(3):
            d.k[i][j] = float(k[i, j])
    return d


def ipc_weights(kernel):
    """The nine integer weights [3, 3] int32 of a kernel (wayne_ipc_weights: host arithmetic, no device); ValueError for
    a kernel the library refuses."""
    w = (C.c_int32 * 9)()
    d = ipc_desc(kernel)
    if load().wayne_ipc_weights(C.byref(d), w) != 0:
        raise ValueError("inter-pixel capacitance: neighbour weights must be finite, >= 0 and sum to at most 1")
    return np.array(list(w), dtype=np.int32).reshape(3, 3)


def make_desc(seed, exposure_index, flags, sub_scale, wl_um, flux, depth, x_ref, y_ref, dur_ms,
              sample_read, read_dt_s, replay_seed=None, rng_mode=RNG_PHILOX, threads_compat=1,
              sky_ct_s=0.0, cosmic_rate=-1.0, scale_factor=1.0, noise_mean=0.0, noise_std=0.0,
              thrower_margin=0, thrower_splits=0, lc_z=None, lc_hidden=None, lc_rp=None, lc_ld=None, sources=None,
              traps=None, extraction=None, device_fits=False, expected=None, lc_ld_table=None, ramp_fit=None, ima=None,
              ipc=None, lc_spots=None):
    """The exposure descriptor.  `sources`: contaminating field stars (sources.Contaminant), carried beside the C struct
    and set by Context.upload (wayne_exposure_set_sources); None or [] = the target alone.  `traps`: charge traps
    (traps.ExposureTraps, or a traps.ChargeTraps whose table is flat at `initial`), set by Context.upload
    (wayne_exposure_set_traps); None = no trapping.  `extraction`: the spectral extraction of the exposure
    (extraction.Extraction), set by Context.upload (wayne_exposure_set_extraction); None = reads only.  `device_fits`: the reads' FITS words are formed on the device too,
    set by Context.upload (wayne_exposure_set_fits).  `expected`: "counts" or "mean" -- the noise-free expected image is
    rendered with every run, set by Context.upload (wayne_exposure_set_expected); None = none.  `lc_ld_table`: Claret
    coefficients per wavelength bin [W, 4] of the device light curve, carried beside the C struct and set by
    Context.upload (wayne_exposure_set_limb_darkening); None = lc_ld for every bin.  `lc_spots`: star spots of the device
    light curve (spots.SpotGeometry on the descriptor's W bins), set by Context.upload (wayne_exposure_set_spots); None =
    a clean star.  `ramp_fit`: a rampfit.RampFit, or
    True for its defaults -- every run also fits the reads' ramps (rate, variance and flag word per pixel), set by
    Context.upload (wayne_exposure_set_rampfit); None = none.  `ima`: an ima.Ima, True, "rate" or "counts" -- every run
    also forms the calibrated reads (SCI, ERR and DQ of an `_ima` file), set by Context.upload (wayne_exposure_set_ima);
    None = none."""
    d = ExposureDesc()
    keep = []

    def arr(a, conv):
        a = conv(a)
        keep.append(a)
        return a

    wl_um, flux = arr(wl_um, f64), arr(flux, f64)
    x_ref, y_ref, dur_ms = arr(x_ref, f64), arr(y_ref, f64), arr(dur_ms, f64)
    sample_read, read_dt_s = arr(sample_read, i32), arr(read_dt_s, f64)
    W, K = wl_um.size, x_ref.size
    if flux.size != W or y_ref.size != K or dur_ms.size != K or sample_read.size != K:
        raise ValueError("exposure descriptor: inconsistent array lengths")
    d.seed, d.exposure_index = int(seed) & 0xFFFFFFFF, int(exposure_index) & 0xFFFFFFFF
    d.rng_mode, d.threads_compat = int(rng_mode), int(threads_compat)
    d.flags, d.sub_scale = int(flags), int(sub_scale)
    d.n_wl, d.wl_um, d.flux = W, ptr(wl_um, C.c_double), ptr(flux, C.c_double)
    if depth is not None:
        depth = arr(depth, f64)
        if depth.shape != (K, W):
            raise ValueError("depth must have shape (K, W)")
        d.depth = ptr(depth, C.c_double)
    d.n_samples = K
    d.x_ref, d.y_ref, d.dur_ms = ptr(x_ref, C.c_double), ptr(y_ref, C.c_double), ptr(dur_ms, C.c_double)
    if replay_seed is not None:
        replay_seed = arr(replay_seed, i32)
        d.replay_seed = ptr(replay_seed, C.c_int32)
    d.sample_read = ptr(sample_read, C.c_int32)
    d.n_reads, d.read_dt_s = read_dt_s.size, ptr(read_dt_s, C.c_double)
    d.sky_ct_s, d.cosmic_rate = float(sky_ct_s), float(cosmic_rate)
    d.scale_factor, d.noise_mean, d.noise_std = float(scale_factor), float(noise_mean), float(noise_std)
    d.thrower_margin, d.thrower_splits = int(thrower_margin), int(thrower_splits)
    if lc_z is not None:
        if depth is not None:
            raise ValueError("give either depth or lc_z")
        lc_z, lc_rp = arr(lc_z, f64), arr(lc_rp, f64)
        if lc_z.size != K or lc_rp.size != W:
            raise ValueError("lc_z must have K and lc_rp W elements")
        d.lc_z, d.lc_rp = ptr(lc_z, C.c_double), ptr(lc_rp, C.c_double)
        if lc_hidden is not None:
            lc_hidden = arr(lc_hidden, f64)
            d.lc_hidden = ptr(lc_hidden, C.c_double)
        d.lc_ld[:] = [float(v) for v in lc_ld]
    if lc_ld_table is not None:
        if lc_z is None:
            raise ValueError("lc_ld_table needs the device light curve (lc_z)")
        lc_ld_table = f64(lc_ld_table)
        if lc_ld_table.shape != (W, 4):
            raise ValueError("lc_ld_table must have shape (W, 4)")
    d._ld_table = lc_ld_table
    if lc_spots is not None:
        if lc_z is None:
            raise ValueError("lc_spots needs the device light curve (lc_z)")
        if lc_spots.contrast.shape[1] != W or lc_spots.X.size != len(lc_z):
            raise ValueError("lc_spots must have contrast [n, W] and a track of K points")
    d._spots = lc_spots
    d._keep = keep
    d._sources = tuple(sources) if sources else ()
    if traps is not None:
        from . import traps as _traps
        traps = _traps.for_exposure(traps)
    d._traps = traps
    d._extraction = extraction
    d._device_fits = bool(device_fits)
    d._expected = EXPECT_NAMES[expected_mode(expected)] if expected is not None else None
    from . import rampfit as _rampfit
    d._ramp_fit = _rampfit.as_ramp_fit(ramp_fit)
    from . import ima as _ima
    d._ima = _ima.as_ima(ima)
    from . import ipc as _ipc
    d._ipc = _ipc.as_ipc(ipc)      # (inter-pixel capacitance, set by Context.upload: wayne_exposure_set_ipc; None = none)
    return d


def expected_mode(mode):
    """The library's code of an expected-image mode: None / 0 -> 0, "counts" -> EXPECT_COUNTS, "mean" -> EXPECT_MEAN
    (the codes themselves pass); anything else: ValueError."""
    if mode is None or (mode == 0 and not isinstance(mode, str)):
        return 0
    if isinstance(mode, str) and mode in EXPECT_MODES:
        return EXPECT_MODES[mode]
    if not isinstance(mode, (str, bool)) and mode in EXPECT_NAMES:
        return int(mode)
    raise ValueError('expected: None, "counts" or "mean", not %r' % (mode,))


def device_count():
    return load().wayne_device_count()


def philox4x32(ctr, key):
    ctr = np.ascontiguousarray(ctr, dtype=np.uint32)
    key = np.ascontiguousarray(key, dtype=np.uint32)
    out = np.empty(4, dtype=np.uint32)
    load().wayne_philox4x32(ptr(ctr), ptr(key), ptr(out))
    return out


def fits_layout(S, R, dtype):
    """(plane_bytes, stride, bitpix) of the FITS payload of R + 1 reads of bordered side S and sample type `dtype`
    (float32, float64 or uint16; or a descriptor's flag word): see wayne_fits_layout.  Needs no device."""
    flags = int(dtype) if isinstance(dtype, (int, np.integer)) else OUT_FLAGS[np.dtype(dtype)]
    pb, stride, bitpix = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
    rc = load().wayne_fits_layout(int(S), int(R), flags, C.byref(pb), C.byref(stride), C.byref(bitpix))
    if rc != OK:
        raise WayneError(rc, "fits_layout: no layout for S = %d, R = %d, flags %#x" % (S, R, flags))
    return int(pb.value), int(stride.value), int(bitpix.value)


def source_seed(seed, tag):
    """The visit seed of contaminant `tag` (tag 0: `seed` itself); see wayne_source_seed."""
    return int(load().wayne_source_seed(int(seed) & 0xFFFFFFFF, int(tag) & 0xFFFFFFFF))


def host_sample_draws(seed, exposure, n_samples):
    """(z_x, z_y, rand_seed) of the Philox HOST stage for one exposure."""
    zx = np.empty(n_samples, dtype=np.float64)
    zy = np.empty(n_samples, dtype=np.float64)
    rs = np.empty(n_samples, dtype=np.int32)
    load().wayne_host_sample_draws(int(seed) & 0xFFFFFFFF, int(exposure) & 0xFFFFFFFF, int(n_samples),
                                   ptr(zx), ptr(zy), ptr(rs))
    return zx, zy, rs


_default_ctx = {}
_default_ctx_lock = threading.Lock()


def default_context(device=0):
    """Process-wide context per device (created on first use; creation is serialised)."""
    with _default_ctx_lock:
        if device not in _default_ctx:
            ctx = Context(device)
            ctx.call_lock = threading.Lock()   # for callers that share it between threads (pyparallel.apply_psf)
            _default_ctx[device] = ctx
        return _default_ctx[device]


def spot_lens_basis(P, C_, p, r):
    """Q_0 .. Q_4 of the spots' lens rule from the library's own host arithmetic (wayne_spot_lens_basis): no GPU."""
    out = np.zeros(5)
    load().wayne_spot_lens_basis(float(P[0]), float(P[1]), float(C_[0]), float(C_[1]), float(p), float(r),
                                 ptr(out, C.c_double))
    return out


def spot_rule():
    """The library's Gauss-Legendre nodes and weights of that rule (wayne_spot_rule)."""
    g, w = np.zeros(10), np.zeros(10)
    load().wayne_spot_rule(ptr(g, C.c_double), ptr(w, C.c_double))
    return g, w
