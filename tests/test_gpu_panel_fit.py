"""StateSpaceGPPanel.fit_each on the device (pgps_gp_panel_fit_*: one workgroup per series runs the whole projected-BFGS search
of csrc/pgps_fit.h inside ONE launch).

One panel of 8 series: lengths 1, 2, 37, 256, 257, 700, 2048 -- one lane, a partial wave, 1 / 2 / 3 / 8 steps per lane, the panel's
limit -- with 10 % NaN rows, and one series of NaN only.  d = 1, 2, 3 (Matern-1/2, -3/2, -5/2), scalar noise and per-observation
noise variances.  gtol = 1e-6, max_iter = 60.  What the fit returns is judged by code this feature does not add: the
projected gradient is recomputed from log_likelihoods_and_grads(fit.thetas), the log-likelihoods from log_likelihoods."""
import warnings

import numpy as np
import pytest

import panel_fit_refs as R
from pssgp import fitting

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 37, 256, 257, 700, 2048)
SEEDS = {1: 0, 2: 2, 37: 2, 256: 3, 257: 4, 700: 5, 2048: 6}       # (tests/test_panel_fit_host.py: the oracle converges on them)
NAN_ONLY = len(LENGTHS)                                             # the index of the series without an observed row
CASES = [(name, noise) for name in R.KERNELS for noise in ("scalar", "rs")]
_made = {}


def _data():
    return [R.series(n, SEEDS[n]) for n in LENGTHS] + [R.series(37, 9, nan_only=True)]


def _panel(name, noise, data=None):
    from pssgp.panel import StateSpaceGPPanel
    data = _data() if data is None else data
    return StateSpaceGPPanel([(t, y) for t, y, _ in data], R.KERNELS[name](variance=R.START[0], lengthscales=R.START[1]),
                             noise_variance=R.START[2], observation_variances=[s for _, _, s in data] if noise == "rs" else None)


def _fitted(name, noise):
    """(panel, fit in the kernel, fit by the twin) of a case, made once and shared by the tests (never changed)."""
    key = (name, noise)
    if key not in _made:
        panel = _panel(name, noise)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)         # (the tests assert on status themselves)
            dev = panel.fit_each(gtol=R.GTOL, max_iter=R.MAX_ITER)
            twin = panel.fit_each(gtol=R.GTOL, max_iter=R.MAX_ITER, in_kernel=False)
        _made[key] = (panel, dev, twin)
    return _made[key]


def _n_obs(data):
    return np.array([np.count_nonzero(~np.isnan(y)) for _, y, _ in data], np.float64)


def _start(S):
    t0 = np.tile(np.array(R.START), (S, 1))
    return t0, t0 * 1e-4, t0 * 1e4


@pytest.mark.parametrize("name,noise", CASES)
def test_stationarity_by_the_existing_gradient(name, noise):
    panel, fit, _ = _fitted(name, noise)
    data = _data()
    S = len(data)
    t0, lo, hi = _start(S)
    print(name, noise, "iterations", fit.iterations, "evaluations", fit.evaluations, "status", fit.status, "max |q|", fit.grad_norm)
    assert np.all(fit.status == fitting.STATUS_CONVERGED), fit.status
    assert np.all(fit.iterations <= R.MAX_ITER)
    g = R.objective(panel.log_likelihoods_and_grads, fit.thetas, _n_obs(data), np.ones(3, bool))[1]
    q = R.projected_gradient_norm(g, fit.thetas, lo, hi)
    print(name, noise, "recomputed max |q|", q)
    assert np.all(q <= 2.0 * R.GTOL), q
    lls = panel.log_likelihoods(fit.thetas)
    assert np.all(np.abs(fit.log_likelihoods - lls) <= 1e-9 * np.abs(lls)), (fit.log_likelihoods, lls)
    lls0 = panel.log_likelihoods(t0)
    assert np.all(fit.log_likelihoods >= lls0)
    assert np.all(np.abs(fit.start_log_likelihoods - lls0) <= 1e-9 * np.abs(lls0))
    assert np.all(fit.thetas >= lo) and np.all(fit.thetas <= hi)
    # no observed row: the start comes back, status 0, 0 iterations
    assert np.array_equal(fit.thetas[NAN_ONLY], t0[NAN_ONLY]) and fit.iterations[NAN_ONLY] == 0 and fit.evaluations[NAN_ONLY] == 1
    # the panel's own parameters are untouched
    assert (panel.kernel.variance, panel.kernel.lengthscales, panel.noise_variance) == R.START


@pytest.mark.parametrize("name,noise", CASES)
def test_one_step_is_the_rules_first_accepted_trial(name, noise):
    """max_iter = 1: the returned theta is x0 - alpha q with alpha = min(1, 1 / max |q|) halved until Armijo's condition holds,
    computed here from the existing gradient call at the start."""
    panel = _fitted(name, noise)[0]
    data = _data()
    S = len(data)
    t0, lo, hi = _start(S)
    n_obs = _n_obs(data)
    free = np.ones(3, bool)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        fit = panel.fit_each(gtol=R.GTOL, max_iter=1)
    f, g = R.objective(panel.log_likelihoods_and_grads, t0, n_obs, free)
    qmax = np.max(np.abs(g), axis=1)                                    # (the start is interior: q = g)
    moving = qmax > R.GTOL
    assert list(np.flatnonzero(~moving)) == [NAN_ONLY]
    with np.errstate(divide="ignore"):
        alpha = np.minimum(1.0, 1.0 / qmax)
    want, done = t0.copy(), ~moving
    for _ in range(fitting.FIT_MAX_HALVINGS + 1):
        s = -alpha[:, None] * g
        trial = np.where(moving[:, None], np.exp(np.log(t0) + s), t0)
        ft, gt = R.objective(panel.log_likelihoods_and_grads, trial, n_obs, free)
        ok = ~done & np.isfinite(ft) & np.all(np.isfinite(gt), axis=1) & (ft <= f + fitting.FIT_ARMIJO * np.sum(g * s, axis=1))
        want[ok] = trial[ok]
        done |= ok
        alpha = alpha * 0.5
        if done.all():
            break
    assert done.all()
    assert np.all(np.abs(fit.thetas - want) <= 1e-12 * np.abs(want)), (fit.thetas, want)
    assert list(fit.status) == [fitting.STATUS_MAX_ITER if m else fitting.STATUS_CONVERGED for m in moving]
    assert list(fit.iterations) == [1 if m else 0 for m in moving]


@pytest.mark.parametrize("name,noise", CASES)
def test_the_launch_against_the_twin(name, noise):
    """Series with n >= 37: max |x_dev - x_twin| <= 2 sqrt(P) gtol / lam_min + 1e-8, lam_min the smallest eigenvalue of the Hessian
    of f in x at the twin's optimum (central differences, step 1e-4, of the existing gradient call); the inputs have
    lam_min >= 1e-3.  Both routes stop at |q| <= gtol, so each lies within sqrt(P) gtol / lam_min of the optimum."""
    panel, dev, twin = _fitted(name, noise)
    data = _data()
    rows = [i for i, n in enumerate(LENGTHS) if n >= 37]
    assert np.all(twin.status == fitting.STATUS_CONVERGED), twin.status
    lam_min = R.hessian_min_eigenvalues(panel.log_likelihoods_and_grads, twin.thetas, _n_obs(data), np.ones(3, bool))[rows]
    gap = np.max(np.abs(np.log(dev.thetas[rows]) - np.log(twin.thetas[rows])), axis=1)
    print(name, noise, "lam_min", lam_min, "max |x_dev - x_twin|", gap, "evaluations", dev.evaluations, twin.evaluations)
    assert np.all(lam_min >= 1e-3), lam_min
    assert np.all(gap <= 2.0 * np.sqrt(3.0) * R.GTOL / lam_min + 1e-8), (gap, lam_min)


@pytest.mark.parametrize("noise", ("scalar", "rs"))
def test_bounds_and_wrt(noise):
    name = "Matern32"
    panel, free_fit, _ = _fitted(name, noise)
    S = panel.num_series
    t0, lo, hi = _start(S)
    # an upper bound on the lengthscale below its optimum: the fit ends ON the bound, converged
    row = LENGTHS.index(257)
    cap = 0.5 * free_fit.thetas[row, 1]
    hi2, start = hi.copy(), t0.copy()
    hi2[row, 1], start[row, 1] = cap, 0.25 * cap
    fit = panel.fit_each(start, bounds=(np.minimum(lo, start * 1e-4), hi2), gtol=R.GTOL, max_iter=R.MAX_ITER)
    assert fit.status[row] == fitting.STATUS_CONVERGED and fit.thetas[row, 1] == cap, (fit.status, fit.thetas[row], cap)
    g = R.objective(panel.log_likelihoods_and_grads, fit.thetas, _n_obs(_data()), np.ones(3, bool))[1]
    assert g[row, 1] < 0.0                                              # (the likelihood still pulls it up)
    assert np.all(R.projected_gradient_norm(g, fit.thetas, np.minimum(lo, start * 1e-4), hi2) <= 2.0 * R.GTOL)
    assert np.all(fit.status == fitting.STATUS_CONVERGED), fit.status  # (the other rows too, under the widened lower bounds)
    # a fixed noise_variance comes back bit for bit -- 0 with given variances
    fixed = t0.copy()
    fixed[:, 2] = np.where(np.arange(S) % 2 == 0, 0.13, 0.0 if noise == "rs" else 0.29)
    fit = panel.fit_each(fixed, wrt=[0, 1], gtol=R.GTOL, max_iter=R.MAX_ITER)
    assert np.array_equal(fit.thetas[:, 2], fixed[:, 2])
    assert np.all(fit.status == fitting.STATUS_CONVERGED), fit.status
    lls = panel.log_likelihoods(fit.thetas)
    assert np.all(np.abs(fit.log_likelihoods - lls) <= 1e-9 * np.abs(lls))
    # ... and so does a fixed lengthscale
    fit = panel.fit_each(fixed, wrt=[0], gtol=R.GTOL, max_iter=R.MAX_ITER)
    assert np.array_equal(fit.thetas[:, 1:], fixed[:, 1:]) and np.all(fit.status == fitting.STATUS_CONVERGED)


class _Scratch:
    """pgps_set_batch_scratch for the block, restored on every exit."""

    def __init__(self, nbytes):
        from pssgp import _backend as Bk
        self.ctx, self.nbytes = Bk.get_context(), nbytes

    def __enter__(self):
        self.ctx.set_batch_scratch(self.nbytes)

    def __exit__(self, *exc):
        self.ctx.set_batch_scratch(0)


class _CountLaunches:
    """The context's launch counter on the slot the fit kernel is charged to (PGPS_K_FILTER_APPLY = 1); .launches() reads and
    resets (as tests/test_gpu_panel.py counts its groups)."""

    def __init__(self):
        from pssgp import _backend as Bk
        self.ctx = Bk.get_context()
        self.name = self.ctx.lib.pgps_kernel_name(1).decode()

    def __enter__(self):
        self.ctx.profile_enable(2)
        self.ctx.profile_read(reset=True)
        return self

    def launches(self):
        return int(self.ctx.profile_read(reset=True)[self.name][1])

    def __exit__(self, *exc):
        self.ctx.profile_enable(0)
        self.ctx.profile_read(reset=True)


# A budget that holds a few of the panel's series per group, by state dimension (the scratch of one adjoint pass grows with d:
# pgps_panel_site_lay.h gives groups of 3, 2, 1, 1, 1 series at d = 1, of 3, 3, 2 at d = 2 and d = 3 under these, in the panel's order)
MIDDLE_BUDGET = {"Matern12": 64 << 10, "Matern32": 200 << 10, "Matern52": 400 << 10}


@pytest.mark.parametrize("name,noise", [("Matern12", "rs"), ("Matern32", "scalar"), ("Matern52", "rs")])
def test_a_row_depends_on_its_series_alone(name, noise):
    _, fit, _ = _fitted(name, noise)
    data = _data()
    S = len(data)

    def same(a, b, rows):
        for x, y in zip(a, b):
            assert np.array_equal(x, y[rows], equal_nan=True), (x, y[rows])

    def run(order, panel=None):
        panel = _panel(name, noise, [data[i] for i in order]) if panel is None else panel
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return panel.fit_each(gtol=R.GTOL, max_iter=R.MAX_ITER)

    same(run(list(range(S))), fit, list(range(S)))                      # a repeat
    perm = [6, 0, 7, 3, 1, 5, 2, 4]
    same(run(perm), fit, perm)                                          # a permuted panel
    sub = [5, 2, 6]
    same(run(sub), fit, sub)                                            # a sub-panel
    # Several groups, counted: a fit is ONE launch per group.  A budget of one byte: no second series ever fits, every series is
    # a group of its own (every series that iterates sits behind a first-series offset of its own, and reuses the scratch the
    # group before it left); a middle budget: groups of uneven size.  In the permuted order too, so that the long series are
    # not the last ones
    for order in (list(range(S)), perm):
        panel = _panel(name, noise, [data[i] for i in order])
        with _Scratch(1), _CountLaunches() as count:
            got = run(order, panel)
            n = count.launches()
        assert n == S, n
        same(got, fit, order)
        with _Scratch(MIDDLE_BUDGET[name]), _CountLaunches() as count:
            got = run(order, panel)
            n = count.launches()
        print(f"{name} {noise}: {n} groups under {MIDDLE_BUDGET[name]} bytes")
        assert 1 < n < S, n
        same(got, fit, order)
        with _CountLaunches() as count:                                 # (and the default budget holds the panel: one launch)
            got = run(order, panel)
            n = count.launches()
        assert n == 1, n
        same(got, fit, order)


def test_c_abi_errors_and_forms():
    """Every refusal returns its code and leaves the outputs untouched; the host form and the _dev form agree bit for bit."""
    from pssgp import _backend as Bk
    name, d = "Matern52", 3
    data = _data()[2:5]
    S = len(data)
    offs = np.concatenate([[0], np.cumsum([t.size for t, _, _ in data])]).astype(np.int64)
    ts, ys, rs = (np.concatenate([c[i] for c in data]) for i in range(3))
    P1, H1, N1, N2 = R.unit52()
    unit = np.concatenate([[1.0], N1.reshape(-1), N2.reshape(-1), P1.reshape(-1), H1.reshape(-1), [0.0]])
    t0, lo, hi = _start(S)
    free = np.ones(3, np.int32)
    ctx = Bk.get_context()
    P = Bk._ptr
    thetas, info = np.full((S, 3), -7.0), np.full((S, 8), -7.0)

    def call(S_=S, offs_=offs, d_=d, unit_=unit, ts_=ts, ys_=ys, rs_=None, t0_=t0, lo_=lo, hi_=hi, free_=free, gtol=R.GTOL,
             max_iter=R.MAX_ITER, thetas_=thetas, info_=info):
        return ctx.lib.pgps_gp_panel_fit_f64(ctx.handle, S_, P(offs_), d_, P(unit_), P(ts_), P(ys_), P(rs_), P(t0_), P(lo_), P(hi_),
                                             P(free_), gtol, max_iter, P(thetas_), P(info_))

    def at(a, i, j, v):
        b = a.copy()
        b[i, j] = v
        return b

    bad_offs, long_offs, empty = offs.copy(), np.array([0, 2049], np.int64), offs.copy()
    bad_offs[0] = 1
    empty[1] = empty[2]
    fixed_noise = np.array([1, 1, 0], np.int32)
    bad_unit = unit.copy()
    bad_unit[0] = 0.0
    bad_rs = rs.copy()
    bad_rs[int(np.flatnonzero(~np.isnan(ys))[0])] = -1.0
    INVALID, DIM = -1, Bk.E_UNSUPPORTED_DIM
    refusals = [
        (dict(S_=0), INVALID), (dict(offs_=None), INVALID), (dict(ts_=None), INVALID), (dict(ys_=None), INVALID),
        (dict(t0_=None), INVALID), (dict(lo_=None), INVALID), (dict(hi_=None), INVALID), (dict(free_=None), INVALID),
        (dict(thetas_=None), INVALID), (dict(info_=None), INVALID), (dict(unit_=None), INVALID), (dict(unit_=bad_unit), INVALID),
        (dict(d_=0), DIM), (dict(d_=4), DIM),
        (dict(offs_=bad_offs), INVALID), (dict(offs_=empty), INVALID), (dict(S_=1, offs_=long_offs), INVALID),
        (dict(t0_=at(t0, 1, 0, 0.0)), INVALID), (dict(t0_=at(t0, 1, 1, np.nan)), INVALID), (dict(t0_=at(t0, 0, 2, np.inf)), INVALID),
        (dict(lo_=at(lo, 2, 1, 0.0)), INVALID), (dict(hi_=at(hi, 2, 1, np.inf)), INVALID), (dict(lo_=at(lo, 0, 0, hi[0, 0])), INVALID),
        (dict(free_=fixed_noise, t0_=at(t0, 1, 2, 0.0)), INVALID),              # noise fixed at 0 without rs
        (dict(free_=fixed_noise, t0_=at(t0, 1, 2, -0.1), rs_=rs), INVALID),
        (dict(free_=np.array([0, 1, 1], np.int32), t0_=at(t0, 1, 0, 0.0)), INVALID),
        (dict(rs_=bad_rs), INVALID),                                            # (the host form's scan of rs)
        (dict(gtol=-1.0), INVALID), (dict(gtol=np.nan), INVALID), (dict(max_iter=0), INVALID), (dict(max_iter=201), INVALID),
    ]
    for kwargs, code in refusals:
        assert call(**kwargs) == code, (kwargs, code)
        assert np.all(thetas == -7.0) and np.all(info == -7.0), kwargs
    for rs_ in (None, rs):
        for free_, start in ((free, t0), (fixed_noise, at(t0, 1, 2, 0.0) if rs_ is not None else t0)):
            assert call(rs_=rs_, free_=free_, t0_=start) == 0
            pd = Bk.PanelData(offs, ts, ys, rs_)
            th_dev, info_dev = Bk.panel.gp_panel_fit_dev(pd, d, unit, start, lo, hi, free_, R.GTOL, R.MAX_ITER)
            pd.close()
            assert np.array_equal(th_dev, thetas) and np.array_equal(info_dev, info)
            assert np.all(info[:, 4] == 0.0) and np.all(info[:, 7] == 0.0)
            assert list(info[:, 6]) == [float(np.count_nonzero(~np.isnan(y))) for _, y, _ in data]
    # the _dev form refuses the same way, before anything is queued (the device outputs keep what they held)
    pd = Bk.PanelData(offs, ts, ys, None)
    keep = np.full(S * 11, -7.0)
    with ctx.lock:
        dout = pd._buffer("fit", keep.nbytes)
        ctx.h2d(dout, keep)
        for kwargs in (dict(gtol=-1.0), dict(max_iter=0), dict(lo=at(lo, 0, 0, hi[0, 0])), dict(theta0=at(t0, 1, 0, np.nan))):
            a = dict(theta0=t0, lo=lo, hi=hi, gtol=R.GTOL, max_iter=R.MAX_ITER)
            a.update(kwargs)
            rc = ctx.lib.pgps_gp_panel_fit_dev_f64(ctx.handle, S, P(offs), d, P(unit), pd.ts, pd.ys, None, P(a["theta0"]), P(a["lo"]),
                                                   P(a["hi"]), P(free), a["gtol"], a["max_iter"], dout, dout + 8 * 3 * S)
            assert rc == INVALID, kwargs
        back = np.empty_like(keep)
        ctx.d2h(back, dout)
    pd.close()
    assert np.all(back == -7.0)
