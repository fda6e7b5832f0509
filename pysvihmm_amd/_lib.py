"""ctypes binding of the C ABI in include/svihmm.h (libsvihmm_hip.so).

There is no CPU fallback: if the shared library is missing or no HIP device is
visible, using the engine raises ``RuntimeError``.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsvihmm_hip.so")

ABI_VERSION = 3                   # include/svihmm.h SVIHMM_ABI_VERSION this binding was written against
NKERN = 12
PROF_SLOTS = 0x40000000          # svihmm_profile_enable: only the slots whose bits follow
MASK_AS_NAN = 1
TRANS_WRAP = 2
USE_HOST_LLIKS = 4
KEEP_LBETA = 8
SVI_KEEP_WINDOW = 16
SVI_MIN_PSEUDOCOUNT = 2.5e-3      # include/svihmm.h: smaller Dirichlet pseudo-counts take the per-call route
LTRAN_LINEAR_MIN = -600.0
NIW_MAX_D = 96                    # wider observations: host-evaluated lliks (generic plugin route)
DIAG_MAX_D = 128                  # diagonal family on the device up to this width
MCAT_MAX_D = 128                  # multi-column Categorical family: columns ...
MCAT_MAX_F = 1024                 # ... and features (sum of the columns' symbol counts)
POISSON_MAX_D = 128               # Poisson count family: columns ...
POISSON_MAX_COUNT = (1 << 20) - 1 # ... and the largest count the logfact table may reach
PGAUSS_MAX_D = 128                # Gaussian tracks with missing entries: columns
PGAUSS_ABSENT = 1e150             # ... an entry is present when -PGAUSS_ABSENT < x < PGAUSS_ABSENT
LTRAN_F32_MIN = -60.0
F64, F32 = 0, 1
GROW_METHOD = {"auto": 0, "literal": 1, "products": 2}     # SVIHMM_GROW_* of include/svihmm.h
# svihmm_set_variant's slots: the SVIHMM_VAR_* enumerators of include/svihmm_debug.h, lower-cased (their codes are
# documented there)
VARIANT = {
    "svi_loop": 0, "stats": 1, "fb": 2, "emission_mt": 3, "pipeline": 4, "emission_orbit": 5, "chain": 6,
    "sweep_family": 7, "stats_chunks": 8, "centring": 9, "stats_tiling": 10, "allreduce_coords": 11,
    "stats_lds3": 12, "wide_sweeps": 13, "wide_tran_block": 14, "wide_posterior": 15, "renorm4": 16,
    "msg_layout": 17,
}
# codes of slot "emission_orbit" the tests name (include/svihmm_debug.h: SVIHMM_EMISSION_ORBIT_*)
EMISSION_ORBIT_128 = 2
EMISSION_ORBIT_GENERIC_EDGES = 6       # k_emission_orbit: the generic staging and epilogue in every workgroup
EMISSION_ORBIT_128_GENERIC_EDGES = 7   # 2 and 6 together

_lib = None

_c_double_p = C.POINTER(C.c_double)
_c_int64_p = C.POINTER(C.c_int64)
_c_uint8_p = C.POINTER(C.c_uint8)

# name -> (restype, argtypes); mirrors include/svihmm.h one to one
SIGNATURES = {
    "svihmm_last_error": (C.c_char_p, []),
    "svihmm_abi_version": (C.c_int, []),
    "svihmm_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "svihmm_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "svihmm_destroy": (C.c_int, [C.c_void_p]),
    "svihmm_sync": (C.c_int, [C.c_void_p]),
    "svihmm_set_precision": (C.c_int, [C.c_void_p, C.c_int32]),
    "svihmm_get_precision": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "svihmm_set_obs": (C.c_int, [C.c_void_p, _c_double_p, C.c_int64, C.c_int32, _c_uint8_p]),
    "svihmm_set_globals": (C.c_int, [C.c_void_p, C.c_int32, _c_double_p, _c_double_p]),
    "svihmm_set_emission_niw": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _c_double_p,
                                          _c_double_p, _c_double_p, _c_double_p]),
    "svihmm_set_emission_diag": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _c_double_p,
                                           _c_double_p, _c_double_p, _c_double_p]),
    "svihmm_set_lliks": (C.c_int, [C.c_void_p, _c_double_p, C.c_int32, C.c_int32]),
    "svihmm_loglik": (C.c_int, [C.c_void_p, _c_int64_p, C.c_int32, C.c_int32, C.c_uint32,
                                _c_double_p]),
    "svihmm_forward_backward": (C.c_int, [C.c_void_p, _c_int64_p, C.c_int32, C.c_int32,
                                          C.c_uint32, _c_double_p, _c_double_p, _c_double_p,
                                          _c_double_p]),
    "svihmm_packed_size": (C.c_int64, [C.c_int32, C.c_int32]),
    "svihmm_estep_minibatch": (C.c_int, [C.c_void_p, _c_int64_p, C.c_int32, C.c_int32,
                                         C.c_uint32, _c_double_p]),
    "svihmm_read_packed": (C.c_int, [C.c_void_p, _c_double_p]),
    "svihmm_suffstats": (C.c_int, [C.c_void_p, _c_int64_p, C.c_int32, C.c_int32, C.c_uint32,
                                   _c_double_p, _c_double_p]),
    "svihmm_estep_minibatch_ex": (C.c_int, [C.c_void_p, _c_int64_p, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_int32, C.c_uint32, _c_double_p]),
    "svihmm_set_sequences": (C.c_int, [C.c_void_p, _c_int64_p, C.c_int32]),
    "svihmm_estep_sequences": (C.c_int, [C.c_void_p, C.c_uint32, _c_double_p, _c_double_p, _c_double_p]),
    "svihmm_estep_sequence_subset": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_uint32, _c_double_p,
                                               _c_double_p, _c_double_p]),
    "svihmm_set_labels": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "svihmm_set_state_sets": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int32]),
    "svihmm_viterbi_sequences": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, _c_double_p]),
    "svihmm_ffbs_sequences": (C.c_int, [C.c_void_p, C.c_uint32, _c_double_p, C.c_int32, _c_double_p, C.c_uint64,
                                        C.c_void_p, _c_double_p]),
    "svihmm_svi_begin": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [_c_double_p] * 11 + [C.c_int32, C.c_double]),
    "svihmm_svi_iteration": (C.c_int, [C.c_void_p, C.c_int32, _c_int64_p, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_uint32, C.c_double, C.c_double, C.c_double]),
    "svihmm_svi_sequences": (C.c_int, [C.c_void_p, _c_double_p, _c_double_p]),
    "svihmm_svi_iteration_sequences": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_uint32,
                                                 C.c_double, C.c_double]),
    "svihmm_svi_read_elbo": (C.c_int, [C.c_void_p, C.c_int32, _c_double_p, _c_double_p]),
    "svihmm_svi_begin_diag": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [_c_double_p] * 4 + [C.c_int32]),
    "svihmm_svi_begin_cat": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [_c_double_p] * 4 + [C.c_int32]),
    "svihmm_svi_begin_mcat": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32)] + [_c_double_p] * 4
                              + [C.c_int32]),
    "svihmm_svi_begin_poisson": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [_c_double_p] * 5
                                 + [C.c_int32, C.c_int32]),
    "svihmm_svi_read_factors": (C.c_int, [C.c_void_p] + [_c_double_p] * 3),
    "svihmm_svi_set_adagrad": (C.c_int, [C.c_void_p, _c_double_p]),
    "svihmm_svi_read_adagrad": (C.c_int, [C.c_void_p, _c_double_p]),
    "svihmm_svi_read_state": (C.c_int, [C.c_void_p] + [_c_double_p] * 6),
    "svihmm_read_globals": (C.c_int, [C.c_void_p, _c_double_p, _c_double_p]),
    "svihmm_set_emission_cat": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _c_double_p]),
    "svihmm_set_emission_mcat": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), _c_double_p]),
    "svihmm_set_emission_poisson": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _c_double_p, _c_double_p, _c_double_p,
                                              C.c_int32]),
    "svihmm_set_emission_pgauss": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _c_double_p, _c_double_p, _c_double_p,
                                             _c_double_p]),
    "svihmm_packed_len": (C.c_int64, [C.c_void_p]),
    "svihmm_pred_logprob": (C.c_int, [C.c_void_p, _c_int64_p, C.c_int32, C.c_int32, C.c_uint32, _c_double_p]),
    "svihmm_heldout_rows": (C.c_int, [C.c_void_p, _c_double_p, _c_double_p]),
    "svihmm_heldout_entries": (C.c_int, [C.c_void_p, C.c_int64, _c_int64_p, C.POINTER(C.c_int32), _c_double_p,
                                         _c_double_p, _c_double_p]),
    "svihmm_posterior_expect": (C.c_int, [C.c_void_p, C.c_int32, _c_double_p, _c_double_p]),
    "svihmm_posterior_expect_entries": (C.c_int, [C.c_void_p, C.c_int32, _c_double_p, C.c_int64, _c_int64_p,
                                                  C.POINTER(C.c_int32), _c_double_p]),
    "svihmm_alloc_obs": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32]),
    "svihmm_set_obs_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _c_double_p, C.c_void_p]),
    "svihmm_shift_obs": (C.c_int, [C.c_void_p, _c_double_p]),
    "svihmm_get_shift": (C.c_int, [C.c_void_p, _c_double_p]),
    "svihmm_set_emission_prior": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _c_double_p, _c_double_p]),
    "svihmm_niw_vlb_terms": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _c_double_p, _c_double_p, _c_double_p,
                                       _c_double_p, _c_double_p]),
    "svihmm_generate": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, _c_double_p, _c_double_p,
                                  _c_double_p, C.c_uint64]),
    "svihmm_read_generated": (C.c_int, [C.c_void_p, C.c_void_p, _c_double_p]),
    "svihmm_state_argmax": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "svihmm_viterbi": (C.c_int, [C.c_void_p, _c_int64_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p,
                                 _c_double_p]),
    "svihmm_ffbs_windows": (C.c_int, [C.c_void_p, _c_int64_p, C.c_int32, C.c_int32, C.c_uint32, _c_double_p,
                                      C.c_int32, _c_double_p, C.c_uint64, C.c_void_p, _c_double_p]),
    "svihmm_grow_windows": (C.c_int, [C.c_void_p, _c_int64_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_double, C.c_int32, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p,
                                      _c_double_p, C.c_int32]),
    "svihmm_read_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, _c_double_p]),
    "svihmm_read_intermediate": (C.c_int, [C.c_void_p, C.c_int32, _c_double_p]),
    "svihmm_ffbs": (C.c_int, [C.c_void_p, _c_double_p, _c_double_p, C.c_uint32, _c_int64_p,
                              _c_double_p]),
    "svihmm_ffbs_sample": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _c_double_p, _c_double_p,
                                     _c_double_p, _c_int64_p]),
    "svihmm_comm_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "svihmm_comm_unique_id": (C.c_int, [C.c_char_p]),
    "svihmm_comm_init": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32]),
    "svihmm_comm_destroy": (C.c_int, [C.c_void_p]),
    "svihmm_allreduce_packed": (C.c_int, [C.c_void_p]),
    "svihmm_export_packed": (C.c_int, [C.c_void_p, _c_double_p]),
    "svihmm_import_packed": (C.c_int, [C.c_void_p, _c_double_p]),
    "svihmm_allreduce_host": (C.c_int, [C.c_void_p, _c_double_p, C.c_int64, C.c_int32]),
    "svihmm_profile_enable": (C.c_int, [C.c_void_p, C.c_int32]),
    "svihmm_profile_reset": (C.c_int, [C.c_void_p]),
    "svihmm_profile_read": (C.c_int, [C.c_void_p, _c_double_p, _c_int64_p]),
    "svihmm_kernel_name": (C.c_char_p, [C.c_int32]),
    "svihmm_last_kernel_name": (C.c_char_p, [C.c_void_p, C.c_int32]),
    "svihmm_set_variant": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "svihmm_svi_recoveries": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "svihmm_selftest_mfma": (C.c_int, [C.c_void_p, _c_double_p, _c_double_p, _c_double_p]),
}


def load():
    """Load libsvihmm_hip.so (once) and attach the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    # developer override for A/B runs of differently built HIP libraries (still the HIP path)
    LIB_PATH = os.environ.get("SVIHMM_HIP_LIB", globals()["LIB_PATH"])
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "HIP extension not built: %s is missing. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C pysvihmm_amd/csrc` (there is no CPU fallback)." % LIB_PATH)
    try:
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:
        raise RuntimeError("cannot load %s: %s" % (LIB_PATH, e))
    try:
        lib.svihmm_abi_version.restype = C.c_int
        got = lib.svihmm_abi_version()
    except AttributeError:
        got = None
    if got != ABI_VERSION:
        raise RuntimeError("%s has ABI version %s, this package needs %d: rebuild it "
                           "(`make -C pysvihmm_amd/csrc`)" % (LIB_PATH, got, ABI_VERSION))
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            # (a measurement hook added within ABI version 3 -- svihmm_debug.h -- may be absent from an older
            #  build loaded through SVIHMM_HIP_LIB for an A/B run; the drop-in boundary itself must be complete)
            if name == "svihmm_last_kernel_name" and "SVIHMM_HIP_LIB" in os.environ:
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error():
    return load().svihmm_last_error().decode("utf-8", "replace")


def check(rc, what=""):
    if rc != 0:
        raise RuntimeError("%s failed: %s" % (what or "svihmm call", last_error()))


def dptr(a):
    return None if a is None else a.ctypes.data_as(_c_double_p)


def i64ptr(a):
    return None if a is None else a.ctypes.data_as(_c_int64_p)


def u8ptr(a):
    return None if a is None else a.ctypes.data_as(_c_uint8_p)


def as_state_table(table, K, who):
    """``table`` of the posterior-expectation calls as a contiguous float64 ``[K, F]`` array (``[K]`` counts as
    F = 1)."""
    t = np.asarray(table, dtype=np.float64)
    if t.ndim == 1:
        t = t[:, None]
    if t.ndim != 2 or t.shape[0] != K or t.shape[1] < 1:
        raise ValueError("%s: table must be a [K = %d, F] array (or [K] for F = 1), got %s"
                         % (who, K, np.shape(table)))
    return np.ascontiguousarray(t)


def as_f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise RuntimeError("expected array of shape %s, got %s" % (shape, a.shape))
    return a
