"""Host tests that pin the reference of the multi-output geometry tests (multi_refs.ss_multi: ONE covariance, a (d, M) matrix
of means) before test_gpu_multi_geometries.py holds the device to it: against the single-column state-space reference
het_refs.ss_het column by column (1e-12 relative: the same recursion), against dense conditioning (het_refs.dense_het, at
kernel_zoo's 1e-6 for the Matern family), and the merge that carries the source rows.  No device is needed."""
import functools

import numpy as np
import pytest

from het_refs import MATERNS, R, dense_het, merged, queries, rel, sde_of, ss_het
from multi_refs import merged_rows, multi_series, ss_multi

N, K, M = 300, 40, 5
SPACING = 0.05
KNAMES = ("m12", "m32", "m52")


@functools.lru_cache(maxsize=None)
def _case():
    t, Y = multi_series(N, M, SPACING)
    tq = queries(t, K)
    for a in (t, Y, tq):
        a.setflags(write=False)
    return t, Y, tq


@functools.lru_cache(maxsize=None)
def _ref(kname):
    t, Y, tq = _case()
    out = ss_multi(sde_of(kname), t, Y, R, tq)
    for a in out:
        a.setflags(write=False)
    return out


def test_the_data_is_what_the_tests_need():
    t, Y, tq = _case()
    nan = np.isnan(Y)
    assert Y.shape == (N, M) and np.all(np.diff(t) > 0)
    assert np.array_equal(nan.any(axis=1), nan.all(axis=1))
    assert nan[0, 0] and nan[N - 1, 0] and not nan[N // 2, 0] and 0.12 < nan[:, 0].mean() < 0.28
    assert tq[0] < t[0] and tq[-1] > t[-1] and np.intersect1d(tq, t).size >= 5
    _, extra = multi_series(N, M, SPACING, extra_missing=range(100, 110))
    assert np.all(np.isnan(extra[100:110])) and np.array_equal(np.isnan(extra[:100]), nan[:100])
    # the columns differ (each has its own amplitude and noise)
    seen = ~nan[:, 0]
    assert all(not np.allclose(Y[seen, 0], Y[seen, j]) for j in range(1, M))


@pytest.mark.parametrize("kname", KNAMES)
def test_equals_the_single_column_reference(kname):
    t, Y, tq = _case()
    ll, mean, var = _ref(kname)
    assert ll.shape == (M,) and mean.shape == (K, M) and var.shape == (K,)
    only_ll = ss_multi(sde_of(kname), t, Y, R)
    for j in range(M):
        w_ll, w_mean, w_var = ss_het(sde_of(kname), t, Y[:, j], R, np.zeros(N), tq)
        e = (abs(ll[j] - w_ll) / abs(w_ll), rel(mean[:, j], w_mean), rel(var, w_var))
        e_ll = abs(only_ll[j] - ss_het(sde_of(kname), t, Y[:, j], R, np.zeros(N))) / abs(w_ll)
        print(f"{kname} column {j} against ss_het: ll {e[0]:.2e} mean {e[1]:.2e} var {e[2]:.2e}; without queries ll {e_ll:.2e}")
        assert max(e) <= 1e-12 and e_ll <= 1e-12, (j, e, e_ll)


@pytest.mark.parametrize("kname", KNAMES)
def test_equals_the_dense_gp(kname):
    _, spec, tol = MATERNS[kname]
    assert tol == 1e-6
    t, Y, tq = _case()
    ll, mean, var = _ref(kname)
    first_var = None
    for j in range(M):
        d_ll, d_mean, d_var = dense_het(spec, t, Y[:, j], R, np.zeros(N), tq)
        print(f"{kname} column {j} against the dense GP: ll {abs(ll[j] - d_ll):.2e} mean {np.max(np.abs(mean[:, j] - d_mean)):.2e} "
              f"var {np.max(np.abs(var - d_var)):.2e}")
        np.testing.assert_allclose(ll[j], d_ll, atol=tol, rtol=tol)
        np.testing.assert_allclose(mean[:, j], d_mean, atol=tol, rtol=tol)
        np.testing.assert_allclose(var, d_var, atol=tol, rtol=tol)
        # the variance is the same for every column: the dense one depends on the missing pattern alone
        first_var = d_var if first_var is None else first_var
        np.testing.assert_allclose(d_var, first_var, atol=1e-12, rtol=0)


def test_a_row_missing_in_all_columns_leaves_the_merge_of_the_others():
    t, Y, tq = _case()
    tm, Ym, isq = merged_rows(t, Y, tq)
    # the merge is het_refs.merged of every column
    for j in range(M):
        w_t, w_y, _, w_isq = merged(t, Y[:, j], np.full(N, R), tq)
        assert np.array_equal(tm, w_t) and np.array_equal(isq, w_isq)
        assert np.array_equal(np.isnan(Ym[:, j]), np.isnan(w_y)) and np.array_equal(Ym[~np.isnan(w_y), j], w_y[~np.isnan(w_y)])
    assert isq.sum() == K and np.all(np.isnan(Ym[isq]))
    # an observed row between two others that no query ties on (a query at its time would keep its step in the series)
    row = int(np.flatnonzero(~np.isnan(Y[:, 0]) & ~np.isin(t, tq))[17])
    gone = Y.copy()
    gone[row] = np.nan
    tm2, Ym2, isq2 = merged_rows(t, gone, tq)
    at = int(np.flatnonzero(~isq)[row])                    # the merged step of that training row
    assert np.array_equal(tm2, tm) and np.array_equal(isq2, isq) and tm[at] == t[row]
    others = np.arange(tm.size) != at
    assert np.all(np.isnan(Ym2[at])) and np.array_equal(Ym2[others], Ym[others], equal_nan=True)
    # ... and a row that is missing is a row that is not there: the filter steps over it (F and Q of two steps compose)
    keep = np.arange(N) != row
    a = ss_multi(sde_of("m32"), t, gone, R, tq)
    b = ss_multi(sde_of("m32"), t[keep], Y[keep], R, tq)
    e = (float(np.max(np.abs(a[0] - b[0]) / np.abs(b[0]))), rel(a[1], b[1]), rel(a[2], b[2]))
    print(f"row {row} missing against row {row} absent: ll {e[0]:.2e} mean {e[1]:.2e} var {e[2]:.2e}")
    assert max(e) <= 1e-10, e
