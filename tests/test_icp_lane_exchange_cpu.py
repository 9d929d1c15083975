"""The premises of tests/icp_lane_exchange_cases.py, with numpy alone (no GPU):
  * every island's winner under the brute force is the point the case names, in both storages; ties are exact ties as the device forms d2
    in either storage, the points ON a radius are on it to the bit; the quad case places the nearest point at every place of every
    island size, the wave case at every one of the 64 places;
  * the array-end inputs: the last cell of the cell-sorted order holds exactly the stated number of points and so does the last range of
    the replica, which is the range the corner queries scan; every corner query's match is
    one of them, the stale points are nearer, target and stale cloud ask the pool for one block class with the slack included, every
    residual of the brute force's matches is zero (the registration stands still);
  * the slack behind a searched array covers what a batch of the scan loop can load beyond a range: (loads in flight - 1) strides of
    at most 64 elements, both storages -- and the header says the same number."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_lane_exchange_cases as lc  # noqa: E402
import icp_scan_loop_cases as sc  # noqa: E402
import icp_search_restatement as rs  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "open3d_slam_amd", "csrc")


@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("name", list(lc.builders()))
def test_winners_and_ties(name, storage):
    c, owner, want = lc.builders()[name]()
    m = rs.nearest_within(c.src, c.tgt, c.T, c.r, storage)
    assert np.array_equal(m.idx, lc.winners(c, owner, want))
    assert len(want) == len(c.src) == owner.max() + 1
    r2 = rs.r2_storage(c.r, storage)
    n_ties = n_on = 0
    for q in range(len(c.src)):
        mine = np.flatnonzero(owner == q)
        d2 = sc.d2_storage(c.src[q], c.tgt[mine], storage)
        n_ties += int((d2 == d2.min()).sum() == 2 and d2.min() < r2)
        n_on += int((d2 == r2).any())
        if m.idx[q] >= 0:  # the winner is nearer than every other island's points and than the anchors
            assert m.d2[q] == d2.min() and (m.gap[q] == 0.0) == ((d2 == d2.min()).sum() > 1)
    assert (n_ties, n_on) == {"quad": (12, 1), "quad-radius": (0, 3), "wave": (lc.WAVE, 0)}[name]


def test_the_nearest_point_stands_at_every_place():
    _, owner, want = lc.quad_case()
    at = 0
    for n in lc.QUAD_COUNTS:
        assert sorted(want[at:at + n].tolist()) == list(range(n)) and all((owner == i).sum() == n for i in range(at, at + n))
        at += n
    _, owner, want = lc.wave_case()
    assert want[:lc.WAVE].tolist() == list(range(lc.WAVE)) and all((owner == i).sum() == lc.WAVE for i in range(2 * lc.WAVE))
    # the first 64 islands open the array: each is one run of 64 consecutive, 64-aligned original indices (one wavefront of the scatter)
    assert all(np.array_equal(np.flatnonzero(owner == i), np.arange(64 * i, 64 * i + 64)) for i in range(lc.WAVE))


@pytest.mark.parametrize("n_last", lc.END_LENGTHS)
def test_array_end_inputs(n_last):
    c, stale = lc.array_end_case(n_last)
    assert lc.last_cell_count(c.tgt) == n_last
    assert lc.last_super_row(c.tgt, c.src[:64]) == (n_last, True), "the corner queries' replica range is the replica's last, and holds the last cell alone"
    for storage in rs.STORAGES:
        m = rs.nearest_within(c.src, c.tgt, c.T, c.r, storage)
        corner = m.idx[:64]
        assert ((corner >= 1) & (corner <= n_last)).all() and np.array_equal(m.idx[64:], np.arange(100, 100 + lc.END_FILL))
        ms = rs.nearest_within(c.src[:64], stale, c.T, c.r, storage)
        assert (ms.d2 < m.d2[:64]).all(), "a stale point is nearer to every corner query than any target point"
        t, n = rs.to_storage(c.tgt, storage), c.nrm
        res = ((m.q - t[m.idx]) * n[m.idx]).sum(axis=1)
        assert (res == 0.0).all(), "every residual is zero: the registration stands still"
        b = lc.POINT_BYTES[storage]
        assert sc.pool_reuses(sc.pool_block(b * len(stale) + lc.SCAN_SLACK_BYTES), b * len(c.tgt) + lc.SCAN_SLACK_BYTES)
        assert sc.pool_reuses(sc.pool_block(9 * b * len(stale) + lc.SCAN_SLACK_BYTES), 9 * b * len(c.tgt) + lc.SCAN_SLACK_BYTES)


def test_the_slack_covers_what_a_batch_loads_beyond_a_range():
    for storage in rs.STORAGES:
        for stride in (4, 64):
            # the first load of a batch lies inside the range; the k-th lies k strides behind it
            beyond = (lc.IN_FLIGHT[storage] - 1) * stride * lc.POINT_BYTES[storage]
            assert beyond <= lc.SCAN_SLACK_BYTES
    assert (lc.IN_FLIGHT[rs.F32] - 1) * 64 * lc.POINT_BYTES[rs.F32] == 3072 and (lc.IN_FLIGHT[rs.F64] - 1) * 64 * lc.POINT_BYTES[rs.F64] == 2048
    src = open(os.path.join(CSRC, "icp_kernels.hpp")).read()
    assert int(re.search(r"constexpr size_t kScanSlackBytes = (\d+);", src).group(1)) == lc.SCAN_SLACK_BYTES
    assert re.search(r"kScanMaxBytes = \(\(size_t\)1 << 32\) - kScanSlackBytes;", src), "offsets into the slack do not wrap"
    assert "kInFlight = sizeof(R) == 8 ? 2 : 4" in src
