"""Host test of tests/panel_geometry_refs.py (the tables and bands tests/test_gpu_panel_geometries.py rests on): the
wave-class tables computed from the formula equal the table as written, every pin's launch holds a staged wave next to a
ragged and an empty one, and the two Matern-1/2 bands hold on the reference.  No device, no library."""
import numpy as np
import pytest

import panel_geometry_refs as G


def test_the_tables_are_the_formula():
    assert G.TABLE_TRAIN == G.ISSUE_TRAIN
    assert G.TABLE_MERGED == G.issue_merged()
    assert G.MERGED_LENGTHS[6] == 260 and max(G.MERGED_LENGTHS) <= 2048
    for pin in G.PINS:
        assert G.staged_next_to_ragged_and_empty(G.TABLE_TRAIN[pin], pin)
        assert G.staged_next_to_ragged_and_empty(G.TABLE_MERGED[pin], pin)
    steps = {lc for pin in G.PINS for lc, _ in G.TABLE_TRAIN[pin]}
    assert {1, 3, 4, 5, 6, 7, 8, 16} <= steps


def test_the_panel():
    cases = G.panel()
    assert [c[0].size for c in cases] == list(G.LENGTHS) and [c[3].size for c in cases] == list(G.QUERIES)
    assert np.all(np.isnan(cases[0][1][250:262])) and not np.isnan(cases[0][1][400])
    assert all(not a.flags.writeable for c in cases for a in c)
    assert not np.array_equal(cases[3][1][:1], cases[1][1])             # (a seed per series)


@pytest.mark.parametrize("pin", G.PINS)
def test_the_bands(pin):
    found = G.assert_bands("m12", G.per_series_settings("m12"), False, pin, True, log=lambda s: None)
    assert found == ((4, 2) if pin < 16 else (0, 0)), found
    found = G.assert_bands("m12", (G.DEFAULT,), True, pin, False, log=lambda s: None)
    assert found[0] == 0 and (found[1] >= 4 or pin == 16), found


def test_the_settings_stay_within_the_matrix_exponentials_reach():
    for kname in G.KNAMES:
        for loo in (False, True):
            for setting in set(G.per_series_settings(kname, loo)) | {G.DEFAULT}:
                assert G.max_lam_dt(kname, setting) <= G.LAM_DT_MAX
