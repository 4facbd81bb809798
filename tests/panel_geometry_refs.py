"""Data and tables of tests/test_gpu_panel_geometries.py: one panel of nine series whose lengths, under the pinned chunks
PINS, put LDS-staged waves next to ragged and empty ones inside one workgroup, with a 1-row and a 37-row neighbour's slice
behind them.  Nothing here is a device call: the wave classes come from the formula the kernels state
(pgps_fused.hip.h: a wave is staged iff all of its 64 x Lc rows exist and Lc is a whole number of 4-step sub-tiles), the bands
from het_refs.workgroup_forgetting at a span of one wave, the references from het_refs.ss_het / dense_het and
loo_refs.ss_checks / dense_checks.  Everything is computed once and handed out read-only.

The panel: series i is het_refs.series(n_i, seed=i), queries het_refs.queries(t, k_i, seed=i); series 0 also has rows 250..261
missing, a run across the boundary of waves 0 and 1 at four steps per lane (row 256).

Steps per lane and wave classes (s staged, r ragged or unstaged, e empty) of the TRAINING lengths, per pin:

    pin   800      1        1100     37       1400     1700     256      1900     700
    0     4 sssr   1 reee   5 rrrr   1 reee   6 rrrr   7 rrrr   1 rrrr   8 sssr   3 rrrr
    4     4 sssr   4 reee   5 rrrr   4 reee   6 rrrr   7 rrrr   4 seee   8 sssr   4 ssre
    8     8 sree   8 reee   8 ssre   8 reee   8 ssre   8 sssr   8 reee   8 sssr   8 sree
    16    16 reee  16 reee  16 sree  16 reee  16 sree  16 sree  16 reee  16 sree  16 reee

The MERGED lengths n + k (what a predict filters) keep these classes, except that 256 + 4 = 260 takes 2 rrre at pin 0 and
4 sree at pin 4.  TABLE_TRAIN / TABLE_MERGED are computed from the formula and held to this text (ISSUE_TRAIN, the two
exceptions) by test_panel_geometry_refs_host.py and, with the library's own steps per lane, by the GPU module.

Settings (variance, lengthscale, R).  DEFAULT is the tests' (1, 0.5, 0.1): with it every Matern-1/2 wave total of these
series has forgotten (log2 max|A| <= FORGETS = -40 at every interior wave of a series with n >= 700; measured -49 .. -124),
so for the d = 1 kernels a wrong term beyond the nearest wave in the fold over wave totals moves nothing.  REMEMBERING is
batch_refs' Matern-1/2 row (0.4, 2.5, 0.5): log2 max|A| and log2 max|E| of every wave that has a successor are held to
>= REMEMBERS = -24 (measured -6 .. -20), about 60 times the 1e-9 bound (2^-30), at every series' own steps per lane and at
pins 4 and 8; at pin 16 a wave is 1024 steps and forgets at this setting too (about -32: printed, not asserted).
Matern-3/2 and -5/2 remember at the default setting.  Nothing in the kernels branches on these figures; the bands only
prove that both kinds of row are in the launch.

The process noise of the references: O.get_ssm takes Q_k from a 2d x 2d matrix exponential that loses Q_k once lam dt reaches
a few tens (batch_refs.py).  The longest step here is the first one of a short series (from 0 to t_0 <= 1.05); with the
shortest lengthscale drawn (0.3) lam dt stays below LAM_DT_MAX = 12 (e^12 of 2^53 leaves eleven digits), asserted in
max_lam_dt() for every setting a test uses: no repair is needed on [0, 1.2]."""
import functools

import numpy as np

import batch_refs
from het_refs import MATERNS, dense_het, merged, queries, series, ss_het, workgroup_forgetting
from loo_refs import dense_checks, ss_checks

LANES, WAVE, SUBTILE = 256, 64, 4
LENGTHS = (800, 1, 1100, 37, 1400, 1700, 256, 1900, 700)
QUERIES = (50, 1, 50, 0, 0, 50, 4, 100, 50)
PINS = (0, 4, 8, 16)
RUN = (250, 12)                             # series 0: rows 250 .. 261 missing
KNAMES = ("m12", "m32", "m52")
DEFAULT = (1.0, 0.5, 0.1)
REMEMBERING = batch_refs.M12_EXTRA          # (0.4, 2.5, 0.5)
REMEMBERS, FORGETS = -24.0, -40.0
REMEMBERS_UP_TO = 8                         # steps per lane: a wave of 16 x 64 steps forgets even at REMEMBERING (about -32)
LONG = 700                                  # the bands are asserted on the series from this length on
LAM_DT_MAX = 12.0
MIN_GAP = 0.05                              # (R_k - v) / R_k of the leave-one-out cavity (tests/test_gpu_panel_checks.py)

# the table of the module docstring, as text: {pin: ((steps per lane, classes) per series)}
ISSUE_TRAIN = {
    0: ((4, "sssr"), (1, "reee"), (5, "rrrr"), (1, "reee"), (6, "rrrr"), (7, "rrrr"), (1, "rrrr"), (8, "sssr"), (3, "rrrr")),
    4: ((4, "sssr"), (4, "reee"), (5, "rrrr"), (4, "reee"), (6, "rrrr"), (7, "rrrr"), (4, "seee"), (8, "sssr"), (4, "ssre")),
    8: ((8, "sree"), (8, "reee"), (8, "ssre"), (8, "reee"), (8, "ssre"), (8, "sssr"), (8, "reee"), (8, "sssr"), (8, "sree")),
    16: ((16, "reee"), (16, "reee"), (16, "sree"), (16, "reee"), (16, "sree"), (16, "sree"), (16, "reee"), (16, "sree"),
         (16, "reee")),
}
ISSUE_MERGED_EXCEPTIONS = {(0, 6): (2, "rrre"), (4, 6): (4, "sree")}


def steps_per_lane(m, pin):
    """The panel's rule as include/pgps.h states it: max(1, ceil(m / 256)), or the pinned chunk where pin x 256 >= m."""
    return pin if pin > 0 and pin * LANES >= m else max(1, -(-m // LANES))


def wave_classes(m, lc):
    """One letter per wave of the series' one workgroup: base of wave w is 64 w lc; s iff base + 64 lc <= m and lc % 4 == 0,
    r iff base < m, else e."""
    out = ""
    for w in range(LANES // WAVE):
        base = WAVE * w * lc
        out += "s" if base + WAVE * lc <= m and lc % SUBTILE == 0 else ("r" if base < m else "e")
    return out


def _table(lengths):
    return {pin: tuple((steps_per_lane(m, pin), wave_classes(m, steps_per_lane(m, pin))) for m in lengths) for pin in PINS}


MERGED_LENGTHS = tuple(n + k for n, k in zip(LENGTHS, QUERIES))
TABLE_TRAIN = _table(LENGTHS)
TABLE_MERGED = _table(MERGED_LENGTHS)


def issue_merged():
    """ISSUE_TRAIN with the two exceptions of the merged lengths."""
    out = {pin: list(row) for pin, row in ISSUE_TRAIN.items()}
    for (pin, i), v in ISSUE_MERGED_EXCEPTIONS.items():
        out[pin][i] = v
    return {pin: tuple(row) for pin, row in out.items()}


def staged_next_to_ragged_and_empty(row, pin):
    """Does a launch with these (steps per lane, classes) hold a series with a staged wave followed by a ragged and an empty
    one -- or, at pin 0 (a series' own steps per lane leave no wave empty from 257 rows on), by a ragged one alone?"""
    return any("sre" in w or (pin == 0 and w.endswith("sr")) for _, w in row)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def panel():
    """((t, y, s, tq),) of the nine series, read-only."""
    out = []
    for i, (n, k) in enumerate(zip(LENGTHS, QUERIES)):
        t, y, s = series(n, seed=i, run=RUN if i == 0 else None)
        out.append(_frozen(t, y, s, queries(t, k, seed=i)))
    return tuple(out)


def loo_panel():
    """((t, y, s),): the same series without their queries (the predictive checks have none)."""
    return tuple(c[:3] for c in panel())


# ---- settings -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def per_series_settings(kname, loo=False):
    """One (variance, lengthscale, R) per series.  Matern-1/2: DEFAULT and REMEMBERING in turn, REMEMBERING on the even
    series (800, 1100, 1400, 256, 700 rows), DEFAULT on 1, 37, 1700, 1900.  Matern-3/2 and -5/2: drawn as
    test_gpu_panel.py::test_per_series_models draws them (loo: as test_gpu_panel_checks.py's, whose R starts at 0.08 for the
    cavity's gap)."""
    if kname == "m12":
        return tuple(REMEMBERING if i % 2 == 0 else DEFAULT for i in range(len(LENGTHS)))
    rng = np.random.RandomState(5)
    return tuple((rng.uniform(0.5, 2.0), rng.uniform(0.3, 1.0), rng.uniform(0.08 if loo else 0.05, 0.3)) for _ in LENGTHS)


@functools.lru_cache(maxsize=None)
def sde(kname, setting):
    return batch_refs.sde(kname, setting)


def spec(kname, setting):
    return (MATERNS[kname][1][0], setting[0], setting[1])


def max_lam_dt(kname, setting):
    """The largest lam dt over the steps of every merged series of the panel (the first step starts at 0); asserted below
    LAM_DT_MAX, where the reference's matrix-exponential process noise is still good to eleven digits."""
    lam = float(np.max(np.abs(np.linalg.eigvals(np.asarray(sde(kname, setting).F, np.float64)))))
    worst = 0.0
    for t, _, _, tq in panel():
        tm = np.sort(np.concatenate([t, tq]))
        worst = max(worst, lam * float(np.max(np.diff(np.concatenate([[0.0], tm])))))
    assert worst <= LAM_DT_MAX, (kname, setting, worst)
    return worst


# ---- the bands --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forgetting(kname, setting, i, het, with_queries, lc):
    """het_refs.workgroup_forgetting of series i (merged with its queries or not) at a span of one wave, 64 lc steps:
    (non-empty waves, 2) log2 max|A|, log2 max|E|."""
    t, y, s, tq = panel()[i]
    Rk = setting[2] + (s if het else np.zeros(t.size))
    if with_queries and tq.size:
        t, y, Rk, _ = merged(t, y, Rk, tq)
    return _frozen(workgroup_forgetting(sde(kname, setting), t, y, Rk, WAVE * lc))[0]


def assert_bands(kname, settings, het, pin, with_queries, log=print):
    """From numpy alone: every series of LONG rows or more whose row is REMEMBERING remembers at each wave that has a
    successor, and (Matern-1/2) every such series at DEFAULT forgets at each interior wave.  Returns (rememberers, forgetters)
    found; the caller asserts on what its launch must hold."""
    found = [0, 0]
    for i, n in enumerate(LENGTHS):
        if n < LONG:
            continue
        setting = settings[i] if len(settings) > 1 else settings[0]
        m = n + (QUERIES[i] if with_queries else 0)
        lc = steps_per_lane(m, pin)
        f = forgetting(kname, setting, i, het, with_queries, lc)
        log(f"{kname} series {i} (m {m}) pin {pin} {setting}: log2 max|A| " + " ".join(f"{x:.0f}" for x in f[:, 0])
            + "  log2 max|E| " + " ".join(f"{x:.0f}" for x in f[:, 1]))
        if f.shape[0] < 2:
            continue
        if setting == REMEMBERING and lc > REMEMBERS_UP_TO:
            log(f"{kname} series {i}: no wave of {WAVE * lc} steps remembers at this setting (the one exception): not asserted")
        elif setting == REMEMBERING:
            assert np.all(f[:-1] >= REMEMBERS), (kname, i, pin, f)
            found[0] += 1
        elif kname == "m12" and setting == DEFAULT and f.shape[0] >= 3:
            assert np.all(f[1:-1, 0] <= FORGETS), (kname, i, pin, f)
            found[1] += 1
    return tuple(found)


# ---- references -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def predict_refs(kname, setting, het, i):
    """((ll, mean, var) of het_refs.ss_het, of het_refs.dense_het) for series i; (ll,) each where it has no query."""
    t, y, s, tq = panel()[i]
    s = s if het else np.zeros(t.size)
    q = tq if tq.size else None
    a = ss_het(sde(kname, setting), t, y, setting[2], s, q)
    b = dense_het(spec(kname, setting), t, y, setting[2], s, q)
    return (a, b) if q is not None else ((a,), (b,))


@functools.lru_cache(maxsize=None)
def loo_refs_of(kname, setting, het, i):
    """(loo_refs.ss_checks, loo_refs.dense_checks) of series i; the cavity's gap is asserted here."""
    t, y, s = loo_panel()[i]
    Rk = setting[2] + s if het else setting[2]
    ss = ss_checks(sde(kname, setting), t, y, Rk)
    assert ss["gap"] >= MIN_GAP, (kname, setting, het, i, ss["gap"])
    return ss, dense_checks(spec(kname, setting), t, y, Rk)

