"""GPU tests of the panel kernels (one workgroup per series: k_gpp_one, k_gpp_gone, k_gpp_loo, k_gpp_fit, k_gpp_newton; DESIGN.md
sections 4aa, 4ab, 4ac, 4af) at launch geometries their own modules never pin: staged, ragged and empty waves inside one
workgroup, with a neighbour's slice directly behind the series' own.

The panel (panel_geometry_refs.py): lengths 800, 1, 1100, 37, 1400, 1700, 256, 1900, 700 with 50, 1, 50, 0, 0, 50, 4, 100, 50
queries, a seed per series, rows 250..261 of series 0 missing; pgps_set_chunk pinned to 0, 4, 8 and 16.  The steps per lane of
every series at every pin are read from pgps_get_panel_chunk and held, with the wave classes they give, to the table of
panel_geometry_refs.py: 4, 5, 6, 7, 8 and 16 steps per lane, and in every launch a series whose staged waves are followed by a
ragged and an empty one (by a ragged one alone at pin 0).  The reversed order, the one-byte budget and the middle budget put
such a series directly in front of the 1-row and the 37-row series' slices.

Before any device call each test asserts from numpy (het_refs.workgroup_forgetting at a span of one wave) that the launch
holds the rows it is meant to hold: with per-series models the Matern-1/2 rows alternate between the default setting, whose
interior wave totals have log2 max|A| <= -40, and (0.4, 2.5, 0.5), whose wave totals stay >= -24 up to 8 steps per lane --
so a wrong term beyond the nearest wave in the fold over wave totals moves a d = 1 result; and (predictive checks) that the
cavity subtraction is benign, (R_k - v) / R_k >= 0.05 (smallest: 0.091, the 1-row series).

References, none the code under test: het_refs.ss_het and loo_refs.ss_checks at the project's 1e-9 (max norm relative to the
largest entry; relative for sums), het_refs.dense_het and loo_refs.dense_checks at the zoo's 1e-6, the single-series device
calls under chunk 0 at 1e-9, fit_each's first accepted trial from log_likelihoods_and_grads under chunk 0 at 1e-12, the
single-series Laplace route at laplace_panel_refs.TOL_SEARCH.  Bit-for-bit: a series alone, the panel reversed, one series
per group, groups of uneven size -- under the same pin.

Measured on an MI355X, the largest over kernels, noise forms and pins.  k_gpp_one / k_gpp_gone: ll
7.0e-15, mean 7.9e-14, var 1.9e-13 against ss_het with one model, 3.1e-14, 1.3e-13, 2.4e-13 with per-series models; gradient
rows 2.4e-14, mean 5.3e-15, var 7.3e-15 against the single-series calls.  k_gpp_loo: 8.2e-14 against ss_checks, 1.5e-13 against
dense_checks, 5.6e-15 against gp_loo; per-series models 1.6e-13 and 1.8e-13.  k_gpp_fit: the first accepted trial 2.2e-16, the
recomputed projected gradient norm 3.0e-7 (gtol 1e-6).  k_gpp_newton: 2.6e-14 against the single-series route.  Every bit
check held; 10 .. 18 launches for the three calls under the middle budget, 7 for the checks."""
import functools
import warnings

import numpy as np
import pytest

import laplace_panel_refs as PR
import laplace_refs as LR
import panel_fit_refs as FR
import panel_geometry_refs as G
from het_refs import MATERNS, rel
from loo_refs import FIELDS, err
from tests import test_gpu_laplace_panel as L
from tests import test_gpu_panel as P
from tests import test_gpu_panel_checks as C
from tests import test_gpu_panel_fit as F
from tests.test_gpu_batch_geometries import _Knobs

pytestmark = pytest.mark.gpu

TOL = 1e-9
KNAMES = G.KNAMES
HET = pytest.mark.parametrize("het", [False, True], ids=["scalar", "rs"])
PIN = pytest.mark.parametrize("pin", G.PINS)
S = len(G.LENGTHS)


# ---- geometry, bands ----------------------------------------------------------------------------------------------------------
def _geometry(pin, lengths, want=None):
    """((steps per lane, wave classes) per length) with the steps per lane read from the library under the pin; held to
    `want` (a row of a table of panel_geometry_refs) where given, to the formula otherwise."""
    from pssgp import _backend as Bk
    with _Knobs(chunk=pin) as ctx:
        lcs = [ctx.get_panel_chunk(m) for m in lengths]
    row = tuple((lc, G.wave_classes(m, lc)) for m, lc in zip(lengths, lcs))
    print(f"pin {pin}: " + "  ".join(f"{m}: {lc} {w}" for m, (lc, w) in zip(lengths, row)))
    assert [lc for lc, _ in row] == [G.steps_per_lane(m, pin) for m in lengths], (pin, row)
    if want is not None:
        assert row == want, (pin, row, want)
    assert Bk.get_context().get_panel_chunk(lengths[0]) == G.steps_per_lane(lengths[0], 0)      # (the pin is gone)
    return row


def _panel_geometry(pin, with_queries):
    """The panel's table rows under the pin, from the library, held to the issue's text; each launch holds a staged wave next to
    a ragged and an empty one."""
    assert G.TABLE_TRAIN == G.ISSUE_TRAIN and G.TABLE_MERGED == G.issue_merged()
    rows = [_geometry(pin, G.LENGTHS, G.TABLE_TRAIN[pin])]
    if with_queries:
        rows.append(_geometry(pin, G.MERGED_LENGTHS, G.TABLE_MERGED[pin]))
    for row in rows:
        assert G.staged_next_to_ragged_and_empty(row, pin), (pin, row)


def _bands(kname, settings, het, pin, with_queries):
    """The two kinds of Matern-1/2 row, from the reference; the settings' process noise is within the matrix exponential's
    reach."""
    for setting in set(settings):
        G.max_lam_dt(kname, setting)
    found = (0, 0)
    for wq in ((False, True) if with_queries else (False,)):
        found = G.assert_bands(kname, settings, het, pin, wq)
    if kname == "m12" and len(settings) > 1:
        # remembering rows: 800, 1100, 1400, 700; forgetting rows with interior waves: 1700, 1900.  At pin 16 a wave is 1024
        # steps: no series has an interior wave and none remembers (panel_geometry_refs.py)
        assert pin == 16 or (found[0] >= 3 and found[1] >= 1), found
    return found


def _models(kname, settings, order=None):
    rows = [P._model(kname, s[2], s[0], s[1]) for s in settings]
    return rows if order is None or len(rows) == 1 else [rows[i] for i in order]


def _setting(settings, i):
    return settings[i] if len(settings) > 1 else settings[0]


def test_the_getter_is_the_rule_and_refuses_what_a_panel_refuses():
    """pgps_get_panel_chunk at every merged length up to PGPS_PANEL_MAX_STEPS = 2048 under every pin, against the rule as
    include/pgps.h states it; m < 1 and m > 2048 are PGPS_E_INVALID and leave the pin as it was."""
    from pssgp import _backend as Bk
    for pin in G.PINS + (1, 3, 7):
        with _Knobs(chunk=pin) as ctx:
            got = [ctx.get_panel_chunk(m) for m in range(1, 2049)]
            for bad in (0, -5, 2049, 1 << 40):
                with pytest.raises(Bk.PgpsError) as refused:
                    ctx.get_panel_chunk(bad)
                assert refused.value.code == P.E_INVALID
            assert ctx.get_panel_chunk(2048) == max(8, pin)
        assert got == [G.steps_per_lane(m, pin) for m in range(1, 2049)], pin


# ---- 1, 2: ll, gradient rows, predict -------------------------------------------------------------------------------------------
def _check_refs(got, kname, settings, het, what, dense=True):
    """Every series of (ll, predict, gradient rows, qoffs) against ss_het at TOL and dense_het at the zoo's tolerance; the
    predict call's ll of every series, the ones without queries too.  Returns the largest errors [ll, mean, var]."""
    ll, (mean, var, llp), rows, qoffs = got
    assert ll.shape == llp.shape == (S,) and mean.shape == var.shape == (sum(G.QUERIES),)
    tol = MATERNS[kname][2]
    worst = [0.0, 0.0, 0.0]
    for i, (t, _, _, tq) in enumerate(G.panel()):
        ref_ss, ref_d = G.predict_refs(kname, _setting(settings, i), het, i)
        sl = slice(qoffs[i], qoffs[i + 1])
        e = [max(P._rel_ll(g, ref_ss[0]) for g in (ll[i], llp[i], rows[i, 0])), 0.0, 0.0]
        if tq.size:
            e[1:] = [rel(mean[sl], ref_ss[1]), rel(var[sl], ref_ss[2])]
        print(f"{what} series {i} (n {t.size}, k {tq.size}) against the state-space reference [ll mean var] "
              + " ".join(f"{x:.2e}" for x in e))
        assert max(e) <= TOL, (what, i, e)
        worst = [max(a, b) for a, b in zip(worst, e)]
        if dense:
            for g in (ll[i], llp[i], rows[i, 0]):
                np.testing.assert_allclose(g, ref_d[0], atol=tol, rtol=tol)
            if tq.size:
                np.testing.assert_allclose(mean[sl], ref_d[1], atol=tol, rtol=tol)
                np.testing.assert_allclose(var[sl], ref_d[2], atol=tol, rtol=tol)
    return worst


def _run(kname, settings, het, pin, order=None, scratch=0):
    with _Knobs(chunk=pin, scratch=scratch):
        return P._calls(_models(kname, settings, order), G.panel(), het, order)


def _against_refs_and_singles(kname, settings, het, pin, dense):
    _panel_geometry(pin, True)
    _bands(kname, settings, het, pin, True)
    for i in range(S):
        G.predict_refs(kname, _setting(settings, i), het, i)           # (numpy, before the device is touched)
    what = f"{kname} rs {het} pin {pin}" + (" per-series models" if len(settings) > 1 else "")
    got = _run(kname, settings, het, pin)
    worst = _check_refs(got, kname, settings, het, what, dense)
    print(f"{what}: the largest errors against the state-space reference [ll mean var] " + " ".join(f"{x:.2e}" for x in worst))
    models = _models(kname, settings)
    P._check_against_singles(got, lambda i: models[i] if len(models) > 1 else models[0], G.panel(), het, what)     # (chunk 0)


@pytest.mark.parametrize("kname", KNAMES)
@HET
@PIN
def test_ll_gradient_rows_and_predict_at_every_pin(kname, het, pin):
    _against_refs_and_singles(kname, (G.DEFAULT,), het, pin, dense=True)


@pytest.mark.parametrize("kname", KNAMES)
@HET
@PIN
def test_per_series_models_at_every_pin(kname, het, pin):
    _against_refs_and_singles(kname, G.per_series_settings(kname), het, pin, dense=False)


# ---- 3. a row's bits depend on its series alone ----------------------------------------------------------------------------------
def _up(nbytes):
    return (nbytes + 255) // 256 * 256


def _pad(n):
    return (n + 31) // 32 * 32                  # kPanelAlign


def _records(d):
    """(NFILT, NSMTH) doubles of a filter and of a smoother scan record (pgps_math.h Dim<D>)"""
    sym = d * (d + 1) // 2
    return d * d + d + sym + sym + d, d * d + d + sym


def _predict_bytes(d, m, het):
    """What ONE series of m merged steps adds to launch_gp_panel's predict layout (panel_lay, pgps_panel_inst.hip): merged
    times, values (and variances), query slots, filtered means and covariances, the workgroup's and the 256 lanes' scan
    records of both scans, the log-likelihood partial.  Every part is rounded up to 256 bytes."""
    nf, ns = _records(d)
    return ((2 + het) * _up(8 * _pad(m)) + _up(4 * _pad(m)) + _up(8 * _pad(m * d)) + _up(8 * _pad(m * d * d))
            + _up(8 * nf) + _up(8 * 256 * nf) + _up(8 * ns) + _up(8 * 256 * ns) + 256)


def _loo_bytes(d, n):
    """The same for the predictive checks: filtered moments of the n training rows, the records, two partials."""
    nf, ns = _records(d)
    return _up(8 * _pad(n * d)) + _up(8 * _pad(n * d * d)) + _up(8 * nf) + _up(8 * 256 * nf) + _up(8 * ns) + _up(8 * 256 * ns) + 512


@pytest.mark.parametrize("kname", KNAMES)
@HET
@PIN
def test_a_row_depends_on_nothing_but_its_series_at_every_pin(kname, het, pin):
    """Per-series models (the Matern-1/2 rows alternate between the forgetting and the remembering setting).  The middle
    budget is 1.25 times what the longest merged series (1900 + 100 steps) takes in the predict layout: the group that holds
    that series holds little else, the short series share groups -- and the log-likelihood call, whose series take their scan
    records only, falls into two or three groups under the same budget."""
    settings = G.per_series_settings(kname)
    _panel_geometry(pin, True)
    _bands(kname, settings, het, pin, True)
    d = len(_models(kname, settings[:1])[0][2])
    want = _run(kname, settings, het, pin)
    _check_refs(want, kname, settings, het, f"{kname} rs {het} pin {pin}", dense=False)
    back = list(range(S - 1, -1, -1))
    P._rows_equal(_run(kname, settings, het, pin, back), want, back, "reversed")
    for i in range(S):
        P._rows_equal(_run(kname, settings, het, pin, [i]), want, [i], "alone")
    with P._CountLaunches() as count:
        got = _run(kname, settings, het, pin, scratch=1)
        n = count.launches()
    assert n == 3 * S, n
    P._rows_equal(got, want, range(S), "one series per group")
    budget = 5 * _predict_bytes(d, 2000, het) // 4
    for order in (list(range(S)), back):
        with P._CountLaunches() as count:
            got = _run(kname, settings, het, pin, order, scratch=budget)
            n = count.launches()
        print(f"{kname} rs {het} pin {pin}: {n} launches for the three calls under a budget of {budget} bytes, {S} series")
        assert 3 < n < 3 * S, (n, budget)
        P._rows_equal(got, want, order, "a few series per group")


# ---- 4. predictive checks ----------------------------------------------------------------------------------------------------------
def _loo(kname, settings, het, pin, order=None, scratch=0):
    cases = G.loo_panel()
    with _Knobs(chunk=pin, scratch=scratch):
        return C._call(_models(kname, settings, order), cases if order is None else [cases[i] for i in order], het)


@pytest.mark.parametrize("kname", KNAMES)
@HET
@PIN
def test_predictive_checks_at_every_pin(kname, het, pin):
    _panel_geometry(pin, False)
    _bands(kname, (G.DEFAULT,), het, pin, False)
    cases = G.loo_panel()
    gaps = [C._refs(kname, case, het)[0]["gap"] for case in cases]      # (asserted >= 0.05 there, from numpy alone)
    print(f"{kname} rs {het}: the smallest (R_k - v) / R_k per series " + " ".join(f"{g:.3f}" for g in gaps))
    out = _loo(kname, (G.DEFAULT,), het, pin)
    C._check_panel(out, kname, cases, het, f"{kname} rs {het} pin {pin}")


@pytest.mark.parametrize("kname", KNAMES)
@HET
@PIN
def test_predictive_checks_with_per_series_models_and_bits_at_every_pin(kname, het, pin):
    """Per-series models against both references, then the bits: reversed, alone, one series per group, and a middle budget
    of 1.25 times what the longest series (1900 rows) takes in the checks' layout."""
    settings = G.per_series_settings(kname, loo=True)
    _panel_geometry(pin, False)
    _bands(kname, settings, het, pin, False)
    cases = G.loo_panel()
    refs = [G.loo_refs_of(kname, settings[i], het, i) for i in range(S)]
    want = _loo(kname, settings, het, pin)
    worst = [0.0, 0.0]
    for i, case in enumerate(cases):
        g, (ss, dn) = C._row(want, i), refs[i]
        obs = ~np.isnan(case[1])
        e_ss = max([err(g[f], ss[f]) for f in FIELDS] + [C._rel(g[k], ss[k]) for k in ("ll", "loo_lpd")])
        e_dn = max([err(np.asarray(g[f])[obs], dn[f]) for f in FIELDS] + [C._rel(g[k], dn[k]) for k in ("ll", "loo_lpd")])
        print(f"{kname} rs {het} pin {pin} series {i} (n {case[0].size}) per-series models: state-space {e_ss:.2e}, dense {e_dn:.2e}")
        worst = [max(worst[0], e_ss), max(worst[1], e_dn)]
    assert worst[0] <= TOL and worst[1] <= MATERNS[kname][2], worst
    back = list(range(S - 1, -1, -1))
    C._rows_equal(_loo(kname, settings, het, pin, back), want, back, "reversed")
    for i in range(S):
        C._rows_equal(_loo(kname, settings, het, pin, [i]), want, [i], "alone")
    with C._CountLaunches() as count:
        got = _loo(kname, settings, het, pin, scratch=1)
        n = count.launches()
    assert n == S, n
    C._rows_equal(got, want, range(S), "one series per group")
    d = len(_models(kname, settings[:1])[0][2])
    budget = 5 * _loo_bytes(d, 1900) // 4
    for order in (list(range(S)), back):
        with C._CountLaunches() as count:
            got = _loo(kname, settings, het, pin, order, scratch=budget)
            n = count.launches()
        print(f"{kname} rs {het} pin {pin}: {n} launches under a budget of {budget} bytes, {S} series")
        assert 1 < n < S, (n, budget)
        C._rows_equal(got, want, order, "a few series per group")


# ---- 5. fit_each under pins ---------------------------------------------------------------------------------------------------------
FIT_PINS = pytest.mark.parametrize("pin", [4, 8, 16])
FIT_LENGTHS = F.LENGTHS + (37,)                 # (the NaN-only series is 37 rows)


@functools.lru_cache(maxsize=None)
def _first_accepted_trial(name, noise):
    """test_gpu_panel_fit.py::test_one_step_is_the_rules_first_accepted_trial's expectation: x0 - alpha q with alpha =
    min(1, 1 / max |q|) halved until Armijo's condition holds, from log_likelihoods_and_grads under chunk 0."""
    from pssgp import fitting
    panel = F._panel(name, noise)
    data = F._data()
    t0, _, _ = F._start(len(data))
    n_obs = F._n_obs(data)
    free = np.ones(3, bool)
    with _Knobs(chunk=0):
        f, g = FR.objective(panel.log_likelihoods_and_grads, t0, n_obs, free)
        qmax = np.max(np.abs(g), axis=1)
        moving = qmax > FR.GTOL
        with np.errstate(divide="ignore"):
            alpha = np.minimum(1.0, 1.0 / qmax)
        want, done = t0.copy(), ~moving
        for _ in range(fitting.FIT_MAX_HALVINGS + 1):
            s = -alpha[:, None] * g
            trial = np.where(moving[:, None], np.exp(np.log(t0) + s), t0)
            ft, gt = FR.objective(panel.log_likelihoods_and_grads, trial, n_obs, free)
            ok = ~done & np.isfinite(ft) & np.all(np.isfinite(gt), axis=1) & (ft <= f + fitting.FIT_ARMIJO * np.sum(g * s, axis=1))
            want[ok] = trial[ok]
            done |= ok
            alpha = alpha * 0.5
            if done.all():
                break
    assert done.all() and list(np.flatnonzero(~moving)) == [F.NAN_ONLY]
    want.setflags(write=False)
    return want, moving


@pytest.mark.parametrize("name,noise", F.CASES)
@FIT_PINS
def test_fit_each_one_step_is_the_rules_first_accepted_trial_under_a_pin(name, noise, pin):
    from pssgp import fitting
    _geometry(pin, FIT_LENGTHS)
    want, moving = _first_accepted_trial(name, noise)
    panel = F._panel(name, noise)
    with _Knobs(chunk=pin), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        fit = panel.fit_each(gtol=FR.GTOL, max_iter=1)
    gap = float(np.max(np.abs(fit.thetas - want) / np.abs(want)))
    print(f"{name} {noise} pin {pin}: the first accepted trial against the rule's from chunk 0 {gap:.2e} (bound 1e-12)")
    assert np.all(np.abs(fit.thetas - want) <= 1e-12 * np.abs(want)), (fit.thetas, want)
    assert list(fit.status) == [fitting.STATUS_MAX_ITER if m else fitting.STATUS_CONVERGED for m in moving]
    assert list(fit.iterations) == [1 if m else 0 for m in moving]


@pytest.mark.parametrize("name,noise", [("Matern12", "rs"), ("Matern32", "scalar"), ("Matern52", "rs")])
@FIT_PINS
def test_fit_each_under_a_pin(name, noise, pin):
    """The whole fit under the pin, judged under chunk 0 by code the fit does not run: log_likelihoods(fit.thetas) at 1e-9, the
    recomputed projected gradient norm <= 2 gtol; and the rows' bits against a permuted panel under the same pin."""
    _geometry(pin, FIT_LENGTHS)
    data = F._data()
    n = len(data)
    perm = [6, 0, 7, 3, 1, 5, 2, 4]
    panel, permuted = F._panel(name, noise), F._panel(name, noise, [data[i] for i in perm])
    with _Knobs(chunk=pin), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        fit = panel.fit_each(gtol=FR.GTOL, max_iter=FR.MAX_ITER)
        other = permuted.fit_each(gtol=FR.GTOL, max_iter=FR.MAX_ITER)
    print(name, noise, "pin", pin, "iterations", fit.iterations, "status", fit.status, "max |q|", fit.grad_norm)
    for x, y in zip(other, fit):
        assert np.array_equal(x, y[perm], equal_nan=True), (x, y[perm])
    t0, lo, hi = F._start(n)
    lls = panel.log_likelihoods(fit.thetas)
    seen = lls != 0.0                           # (the series without an observed row: both are 0)
    e = float(np.max(np.abs(fit.log_likelihoods - lls)[seen] / np.abs(lls)[seen]))
    g = FR.objective(panel.log_likelihoods_and_grads, fit.thetas, F._n_obs(data), np.ones(3, bool))[1]
    q = FR.projected_gradient_norm(g, fit.thetas, lo, hi)
    print(f"{name} {noise} pin {pin}: log-likelihoods against log_likelihoods(thetas) {e:.2e} (bound 1e-9), recomputed max |q| {q}")
    assert np.all(np.abs(fit.log_likelihoods - lls) <= 1e-9 * np.abs(lls)), (fit.log_likelihoods, lls)
    assert np.all(q <= 2.0 * FR.GTOL), q


# ---- 6. the Laplace panel with neighbours -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _laplace_singles(kname, lik):
    """fit_mode() of the single-series route on every series of laplace_panel_refs.panel(lik), under chunk 0: computed once."""
    with _Knobs(chunk=0):
        return tuple(L._single(kname, lik, t, y).fit_mode() for t, y in PR.panel(lik))


@pytest.mark.parametrize("lik", PR.LIKELIHOODS)
@pytest.mark.parametrize("kname", KNAMES)
@pytest.mark.parametrize("pin", [4, 8])
def test_laplace_panel_with_neighbours_under_a_pin(kname, lik, pin):
    cases = PR.panel(lik)
    row = _geometry(pin, PR.LENGTHS)
    assert any(w.startswith("s") and "r" in w for _, w in row), row      # (700 rows: ssre at pin 4, sree at pin 8)
    singles = _laplace_singles(kname, lik)
    with _Knobs(chunk=pin):
        offs, got = L._call(kname, lik, cases)
        alone = [L._call(kname, lik, [case])[1] for case in cases]
    assert np.all(got["info"][:, 5] == 1.0), got["info"]
    worst = 0.0
    for i, ((t, y), fit) in enumerate(zip(cases, singles)):
        a, b = offs[i], offs[i + 1]
        ev = got["info"][i, 0] + got["info"][i, 1] + LR.lik_constant(lik, y)
        e = [PR.err(got["f"][a:b], fit["f"]), PR.err(got["v"][a:b], fit["v"]), PR.err(got["zs"][a:b], fit["z"]),
             PR.err(got["ss"][a:b], fit["s"]), abs(ev - fit["log_evidence"]) / max(1.0, abs(fit["log_evidence"]))]
        print(f"{kname} {lik} pin {pin} n {t.size}: against the single-series route " + " ".join(f"{x:.1e}" for x in e))
        assert max(e) <= PR.TOL_SEARCH, (i, e)
        worst = max(worst, max(e))
        for k in L.ROWS:
            assert np.array_equal(L._bits(got[k][a:b]), L._bits(alone[i][k])), (k, i)
        assert np.array_equal(L._bits(got["info"][i]), L._bits(alone[i]["info"][0])), ("info", i)
    print(f"{kname} {lik} pin {pin}: the largest error against the single-series route {worst:.1e} (bound {PR.TOL_SEARCH:.0e})")
