"""Host arrays on their way into a call: dtype, contiguity, pointers, and the checks every entry point shares."""
import ctypes

import numpy as np

from .library import c_double, c_float, c_void_p


def _suffix(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return "f64", c_double
    if dtype == np.float32:
        return "f32", c_float
    raise TypeError(f"unsupported dtype {dtype}; use float32 or float64")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def _prep(a, dtype, shape=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _float_dtype(a):
    """The dtype a call runs in: float32 stays, everything else becomes float64."""
    dt = np.asarray(a).dtype
    return dt if dt in (np.float32, np.float64) else np.dtype(np.float64)


def _check_rows(ys, N, what="series"):
    if ys.shape[0] != N:
        raise ValueError(f"observations has {ys.shape[0]} rows, the {what} {N} steps")


def _series_inputs(ts, ys, tq=None, rs=None, keep_f32=False, columns=False):
    """The series as the entry points take it: `ts`, `ys` -- and the query times `tq`, the per-observation variances `rs`
    where given -- contiguous in one dtype (that of `ts` with `keep_f32`, as _float_dtype has it; else float64), their
    lengths checked against the N of `ts`.  `columns`: ys is Y (N, M).  Returns (ts, ys, [tq,] [rs,] N)."""
    dtype = _float_dtype(ts) if keep_f32 else np.float64
    ts_a = _prep(ts, dtype, (-1,))
    N = ts_a.shape[0]
    ys_a = _prep(ys, dtype, None if columns else (-1,))
    tq_a = None if tq is None else _prep(tq, dtype, (-1,))
    rs_a = None if rs is None else _prep(rs, dtype, (-1,))
    if columns:
        if ys_a.ndim != 2 or ys_a.shape[0] != N:
            raise ValueError(f"observations must be (N, M) with N = {N} rows, got shape {ys_a.shape}")
    elif rs is not None:
        if ys_a.shape[0] != N or rs_a.shape[0] != N:
            raise ValueError(f"observations has {ys_a.shape[0]} rows, observation variances {rs_a.shape[0]}, the series {N} steps")
    else:
        _check_rows(ys_a, N)
    return tuple(a for a in (ts_a, ys_a, tq_a, rs_a) if a is not None) + (N,)


def _scalar_out():
    """(v, p): a c_double and its address as the void* a `double*` out-parameter takes; read v.value after the call."""
    v = c_double(0.0)
    return v, ctypes.cast(ctypes.byref(v), c_void_p)
