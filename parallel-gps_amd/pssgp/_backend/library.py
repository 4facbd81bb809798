"""libpgps.so: where it is, how it is loaded, and the ctypes signature of every function of include/pgps.h.

The signatures are declared in ONE table, applied once by load_library(); tests/test_abi.py holds the table against the
header's prototypes.  A function the loaded library lacks (A/B runs load older builds through PGPS_LIB) is skipped here and
refused by _require() where it is called."""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))         # pssgp/: the Makefile writes the library there
_LIB_PATH = os.environ.get("PGPS_LIB", os.path.join(_HERE, "libpgps.so"))

PGPS_OK = 0
E_UNSUPPORTED_DIM = -2
E_NUMERIC = -5
PGPS_K_NAMES = None
COMM_ID_BYTES = 128             # PGPS_COMM_ID_BYTES

c_void_p, c_int, c_long, c_double, c_float = (ctypes.c_void_p, ctypes.c_int, ctypes.c_long,
                                              ctypes.c_double, ctypes.c_float)


class PgpsError(RuntimeError):
    def __init__(self, code, what, detail=""):
        self.code = code
        super().__init__(f"libpgps: {what} (code {code}){': ' + detail if detail else ''}")


# One letter per parameter.  Scalars map to exactly the header's type; R is the `real` of the name's suffix (double for
# _f64, float for _f32); P is any data or handle pointer; the lower-case letters and H are out-parameters taken by byref().
_TYPES = {"I": c_int, "L": c_long, "D": c_double, "F": c_float, "Z": ctypes.c_size_t, "U": ctypes.c_ulonglong,
          "P": c_void_p, "S": ctypes.c_char_p, "H": ctypes.POINTER(c_void_p),
          "i": ctypes.POINTER(c_int), "l": ctypes.POINTER(c_long), "d": ctypes.POINTER(c_double)}
_STRING_RETURNS = ("pgps_strerror", "pgps_last_hip_error", "pgps_kernel_name")

# (names, parameters): {dev} expands to "" and "_dev", {suf} to "f64" and "f32"; several names may share one row.
_SIGNATURES = (
    # library and context
    ("pgps_version", ""),
    ("pgps_strerror pgps_kernel_name", "I"),
    ("pgps_last_hip_error pgps_destroy pgps_use_own_stream pgps_synchronize", "P"),
    ("pgps_device_count", "i"),
    ("pgps_create", "IH"),
    ("pgps_set_stream pgps_free", "PP"),
    ("pgps_status", "Pi"),
    ("pgps_malloc", "PZH"),
    ("pgps_memcpy_h2d pgps_memcpy_d2h", "PPPZ"),
    # knobs and diagnostics
    ("pgps_set_chunk pgps_set_stage pgps_set_family pgps_set_block pgps_set_dma pgps_set_resident pgps_set_shortcut "
     "pgps_set_rc_scan pgps_set_one_launch pgps_set_f32_policy pgps_set_batch_form pgps_profile_enable pgps_profile_sample", "PI"),
    ("pgps_set_single_pass", "PII"),
    ("pgps_set_grad_pack", "PL"),
    ("pgps_set_batch_scratch", "PZ"),
    ("pgps_resident_stamps pgps_resident_wave_stamps", "PPIi"),
    ("pgps_debug_resident_delay", "PIII"),
    ("pgps_get_geometry", "PLIiii"),
    ("pgps_get_chunk", "PLii"),
    ("pgps_get_batch_chunk", "PILii"),
    ("pgps_get_panel_chunk", "PLi"),
    ("pgps_get_family", "PLIIIi"),
    ("pgps_profile_calibrate", "Pd"),
    ("pgps_profile_read", "PdlI"),
    # LGSSM arrays: discretisation, filter, smoother, draws, joint covariance
    ("pgps_discretise{dev}_{suf}", "PLIPPPRPP"),
    ("pgps_pkf{dev}_{suf}", "PLIPPPPRPPPP"),
    ("pgps_pks{dev}_{suf}", "PLIPPPPPP"),
    ("pgps_pkfs{dev}_{suf} pgps_pkfs_seg_dev_{suf}", "PLIPPPPRPPPPPP"),
    ("pgps_pks_sample{dev}_{suf}", "PLIPPPPILUPPP"),
    ("pgps_sample_normals_dev_{suf}", "PLIILUP"),
    ("pgps_pks_cov{dev}_{suf}", "PLIPPPPLPPP"),
    ("pgps_pks_cov_gains_dev_{suf}", "PLIPPPLPP"),
    ("pgps_cov_fill_dev_{suf}", "PLIPPPP"),
    # fused path: (lam, N1, N2, Pinf, H) in place of the arrays
    ("pgps_gp{dev}_{suf}", "PLIDPPPPDPDPPPPPP"),
    ("pgps_gp_predict{dev}_{suf}", "PLLIDPPPPDPPDPPPP"),
    ("pgps_gp_ll_multi{dev}_f64 pgps_gp_ll_grad_multi{dev}_f64", "PLIIDPPPPDPPDP"),
    ("pgps_gp_predict_multi{dev}_f64", "PLLIIDPPPPDPPDPPPP"),
    ("pgps_gp_whiten_multi_f64 pgps_gp_gram_multi_f64", "PLIIDPPPPDPPDPdl"),
    ("pgps_gp_whiten_multi_dev_f64 pgps_gp_gram_multi_dev_f64", "PLIIDPPPPDPPDPPP"),
    ("pgps_gp_ll_het{dev}_f64", "PLIDPPPPDPPPDP"),
    ("pgps_gp_predict_het{dev}_f64", "PLLIDPPPPDPPPDPPPP"),
    ("pgps_gp_ll_grad_adj_het{dev}_f64", "PLIDPPPPDPDPPP"),
    ("pgps_gp_loo{dev}_f64", "PLIDPPPPDPPDPPPPP"),
    ("pgps_gp_newton{dev}_f64", "PLIDPPPPIDPPPPPDPPPPPP"),
    ("pgps_lik_sites{dev}_f64", "PLIDPPPPPDPPPPP"),
    ("pgps_gp_ll_grad{dev}_f64", "PLIIPPDPP"),
    ("pgps_gp_ll_grad_blocks{dev}_f64", "PLIIPIPPDPP"),
    ("pgps_gp_ll_grad_adj_dev_f64", "PLIDPPPPDPDPP"),
    # general LTI models (F, Pinf, H)
    ("pgps_lti_ll{dev}_f64 pgps_lti_ll_grad{dev}_f64", "PLIPPPDPPDP"),
    ("pgps_lti_predict{dev}_f64 pgps_lti_predict_cov{dev}_f64", "PLLIPPPDPPDPPPP"),
    ("pgps_lti_predict_lin{dev}_f64", "PLLIIPPPPDPPDPPPP"),
    ("pgps_lti_sample{dev}_f64", "PLLIPPPDPPDPILUPP"),
    # B models at once
    ("pgps_gp_ll_batch{dev}_{suf} pgps_gp_ll_grad_adj_batch{dev}_f64", "PILIPPDPP"),
    ("pgps_lti_ll_batch{dev}_f64 pgps_lti_ll_grad_batch{dev}_f64", "PILIPPPDP"),
    ("pgps_gp_predict_batch{dev}_{suf} pgps_lti_predict_batch{dev}_f64", "PILLIPPPDPPPP"),
    ("pgps_mix_moments_dev_f64", "PILPPPPP"),
    # S series at once, each on its own clock
    ("pgps_gp_panel_ll{dev}_f64 pgps_gp_panel_ll_grad{dev}_f64", "PLPIIPPPPP"),
    ("pgps_gp_panel_predict{dev}_f64", "PLPPIIPPPPPPPP"),
    ("pgps_gp_panel_loo{dev}_f64", "PLPIIPPPPPPPPP"),
    ("pgps_gp_panel_gram{dev}_f64", "PLPIIPIPPPP"),
    ("pgps_gp_panel_residual_dev_f64", "PLPIPPP"),
    ("pgps_gp_panel_trend_solve{dev}_f64", "PLIPPP"),
    ("pgps_gp_panel_profile_grad_f64", "PLPIIPIPPPPPP"),
    ("pgps_gp_panel_profile_grad_dev_f64", "PLPIIPIPPPPPPP"),
    ("pgps_gp_panel_laplace{dev}_f64", "PLPIIPIIPPPDIPPPPP"),
    ("pgps_gp_panel_laplace_grad{dev}_f64", "PLPIIPIIPPPPPPPP"),
    ("pgps_gp_panel_fit{dev}_f64", "PLPIPPPPPPPPDIPP"),
    # a series kept on the device
    ("pgps_series_create_f64", "PLPPDH"),
    ("pgps_series_set_queries_f64", "PLP"),
    ("pgps_series_info", "Pll"),
    ("pgps_series_destroy", "P"),
    ("pgps_series_gp_ll_f64 pgps_series_gp_ll_grad_adj_f64", "PIDPPPPDP"),
    ("pgps_series_gp_predict_f64", "PIDPPPPDPPP"),
    ("pgps_series_lti_ll_f64 pgps_series_lti_ll_grad_f64", "PIPPPDP"),
    ("pgps_series_lti_predict_f64", "PIPPPDPPP"),
    ("pgps_series_gp_ll_grad_f64 pgps_series_lti_ll_batch_f64 pgps_series_gp_ll_grad_adj_batch_f64 "
     "pgps_series_lti_ll_grad_batch_f64", "PIIPP"),
    ("pgps_series_gp_predict_batch_f64 pgps_series_lti_predict_batch_f64", "PIIPPPPP"),
    # a series sharded over GPUs: the segment phases and the communicator
    ("pgps_seg_record_len", "Iii"),
    ("pgps_seg_filter_reduce_dev_{suf}", "PLIIIPPPPRPP"),
    ("pgps_seg_filter_apply_dev_{suf}", "PLIIIPPPPRPPPPP"),
    ("pgps_seg_smoother_apply_dev_{suf}", "PLIIIPPPPPPPP"),
    ("pgps_comm_get_unique_id pgps_comm_destroy", "P"),
    ("pgps_comm_init", "PPII"),
    ("pgps_comm_info pgps_comm_count", "Pii"),
    ("pgps_comm_library", "SZ"),
    ("pgps_comm_allgather_dev", "PPPZ"),
    # host twins (no context)
    ("pgps_seq_kf_{suf}", "LIPPPPRPPPPPP"),
    ("pgps_seq_kf_het_{suf}", "LIPPPPPPPPPPP"),
    ("pgps_seq_ks_{suf}", "LIPPPPPPP"),
    ("pgps_seq_ks_sample_{suf}", "LIPPPPILUPPP"),
    ("pgps_seq_sample_normals_{suf}", "LIILUP"),
    ("pgps_seq_ks_cov_{suf}", "LIPPPPLPPP"),
    ("pgps_host_balance_f64", "IPIP"),
)


def signatures():
    """{function name: [ctypes type of each parameter]} -- the table above, expanded."""
    table = {}
    for names, params in _SIGNATURES:
        for template in names.split():
            for dev in ("", "_dev") if "{dev}" in template else ("",):
                for suf, real in (("f64", "D"), ("f32", "F")) if "{suf}" in template else (("f64", "D"),):
                    table[template.format(dev=dev, suf=suf)] = [_TYPES[c] for c in params.replace("R", real)]
    return table


def _declare(lib):
    for name, argtypes in signatures().items():
        fn = getattr(lib, name, None)
        if fn is not None:                  # (absent from an older build: _require() refuses the call)
            fn.argtypes = argtypes
            if name in _STRING_RETURNS:
                fn.restype = ctypes.c_char_p
    return lib


_lib = None
_lib_lock = threading.Lock()


def load_library():
    """Load libpgps.so (once).  Raises if it has not been built (`python __graft_entry__.py`)."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(_LIB_PATH):
                raise PgpsError(-100, "library not built", f"{_LIB_PATH} missing; run "
                                "`make -C parallel-gps_amd/csrc` (or __graft_entry__.build())")
            _lib = _declare(ctypes.CDLL(_LIB_PATH))
        return _lib


def check(ctx, code, what):
    if code != PGPS_OK:
        lib = load_library()
        msg = lib.pgps_strerror(code).decode()
        detail = lib.pgps_last_hip_error(ctx.handle).decode() if ctx is not None and code in (-3, -7) else ""
        raise PgpsError(code, f"{what}: {msg}", detail)


def _require(ctx, symbol, family):
    """`ctx`, for a call of an entry-point family that older builds of the library lack."""
    if not hasattr(ctx.lib, symbol):
        raise RuntimeError(f"this libpgps has no {family} entry points")
    return ctx
