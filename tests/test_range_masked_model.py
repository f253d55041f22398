"""CPU model of the range search under row bitmaps (host logic, no GPU): which cases of tests/test_range_masked.py may pin
their route counters.  The scan route answers a query itself only while its pool holds every survivor of the int8 bound;
tests/range_masked_cases.through restates that bound (tests/test_range_model.py) and the threshold (range_cases.range_thr)
in numpy and counts, per scan-route query of the table of six, the ALLOWED rows they let through at every radius used."""
import numpy as np
import pytest

import masked_multi_cases as mmc
import range_masked_cases as rmc


@pytest.mark.parametrize("d", rmc.DIMS)
@pytest.mark.parametrize("metric", mmc.METRICS)
def test_scan_route_cases_stay_within_half_a_pool(d, metric):
    X, Q, tab, of, lists = rmc.six(d, metric)
    assert mmc.scans(tab).nonzero()[0].tolist() == list(rmc.SCAN_MASKS)   # the cut of 1024: four masks scan, two are listed
    at = np.nonzero(np.isin(of, rmc.SCAN_MASKS))[0]
    assert len(at) == 64 and len(Q) - len(at) == 32
    for rank in rmc.RANKS:
        n = rmc.through(d, metric)[rank]
        assert (n >= 0).all(), (d, metric, rank, "a query the bound does not serve")
        # every member is let through (soundness), and nobody comes near an overflow: the counters of this case are pinned
        r = rmc.radii_at(lists, len(Q), rank)
        members = np.array([w[2] for w in rmc.want(lists, len(Q), r, rmc.MAX_RESULTS)])[at]
        assert (members >= rank).all() and (n >= members).all(), (d, metric, rank)
        assert n.max() <= rmc.POOL // 2 and rmc.pinned(d, metric, rank), (d, metric, rank, int(n.max()))


def test_radii_and_truth_under_an_empty_and_a_short_mask():
    X, Q, tab, of, lists = rmc.six(128, "l2")
    r = rmc.radii_at(lists, len(Q), 300)
    w = rmc.want(lists, len(Q), r, rmc.MAX_RESULTS)
    assert all(w[i][2] == 0 and w[i][0] == [] for i in np.nonzero(of == 4)[0])          # empty
    assert all(w[i][2] == 300 and len(w[i][0]) == 256 for i in np.nonzero(of == 3)[0])  # few: its last distance, truncated
    for i in range(len(Q)):
        assert tab[of[i], w[i][0]].all()                                                # allowed rows only
