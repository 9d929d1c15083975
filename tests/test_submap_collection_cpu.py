"""SubmapCollection's host logic without a device: AdjacencyMatrix (against the reference's own AdjacencyMatrix.cpp where the checkout
is), the six filters of PlaceRecognition::getLoopClosureCandidatesIdxs on hand-built collections, the parent walk of
SubmapCollection::transform, the switching decisions on stub submaps, and the new parameters."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from open3d_slam_amd import parameters as P
from open3d_slam_amd.adjacency_matrix import INT_MAX, AdjacencyMatrix
from open3d_slam_amd.optimization_problem import OptimizedTransform
from open3d_slam_amd.submap_collection import SubmapCollection, TimestampedSubmapId, getLoopClosureCandidatesIdxs

from oracle import ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(ref.REFERENCE, "open3d_slam", "open3d_slam")  # the reference checkout (oracle/ref.py)


# ---------------------------------------------------------------------------------------------------------- AdjacencyMatrix
def test_distance_is_int_max_while_nothing_was_ever_in_an_edge():
    m = AdjacencyMatrix()
    assert m.getDistanceToNearestLoopClosureSubmap(0) == INT_MAX == 2**31 - 1
    assert m.isAdjacent(3, 3) and not m.isAdjacent(3, 4)


def test_bfs_distance_is_hops_minus_one():
    m = AdjacencyMatrix()
    for a in range(6):  # chain 0-1-2-3-4-5-6
        m.addEdge(a, a + 1)
    m.markAsLoopClosureSubmap(0)
    assert [m.getDistanceToNearestLoopClosureSubmap(i) for i in range(7)] == [0, 0, 1, 2, 3, 4, 5]
    m.addEdge(6, 2)  # a shortcut: 6 is now three hops from 0 (6 - 2 - 1 - 0)
    assert m.getDistanceToNearestLoopClosureSubmap(6) == 2
    m.markAsLoopClosureSubmap(5)
    assert m.getDistanceToNearestLoopClosureSubmap(6) == 0
    assert m.isAdjacent(2, 6) and m.isAdjacent(6, 2) and not m.isAdjacent(0, 2)


def test_unmarked_graph_reports_the_hops_to_the_last_submap_searched():
    m = AdjacencyMatrix()
    m.addEdge(0, 1)
    m.addEdge(1, 2)
    assert m.getDistanceToNearestLoopClosureSubmap(2) == 1  # BFS ends at 0, two hops: max(0, 2 - 1)
    assert m.getDistanceToNearestLoopClosureSubmap(1) == 0


def test_add_edge_resets_the_marks_of_both_ends():
    m = AdjacencyMatrix()
    m.addEdge(0, 1)
    m.addEdge(1, 2)
    m.markAsLoopClosureSubmap(0)
    m.markAsLoopClosureSubmap(2)
    assert m.getDistanceToNearestLoopClosureSubmap(2) == 0
    m.addEdge(2, 3)  # 2 loses its mark
    assert m.getDistanceToNearestLoopClosureSubmap(3) == 2  # 3 -> 2 -> 1 -> 0
    m.addEdge(0, 5)  # and 0 too: nothing is marked any more
    assert m.isLoopClosureSubmap_ == {0: False, 1: False, 2: False, 3: False, 5: False}


def test_unknown_ids_throw():
    m = AdjacencyMatrix()
    with pytest.raises(KeyError):
        m.markAsLoopClosureSubmap(0)
    m.addEdge(0, 1)
    with pytest.raises(KeyError):
        m.markAsLoopClosureSubmap(7)
    with pytest.raises(KeyError):
        m.getDistanceToNearestLoopClosureSubmap(7)
    m.clear()  # the edges go, the marks stay: the search then fails on the first .at() of the adjacency
    with pytest.raises(KeyError):
        m.getDistanceToNearestLoopClosureSubmap(0)


def _random_ops(rng, n_ops=120, n_ids=12):
    ops = []
    for _ in range(n_ops):
        r = rng.random()
        a, b = int(rng.integers(0, n_ids)), int(rng.integers(0, n_ids))
        if r < 0.4:
            ops.append(("E", a, b))
        elif r < 0.55:
            ops.append(("M", a))
        elif r < 0.85:
            ops.append(("D", a))
        else:
            ops.append(("A", a, b))
    return ops


def _python_answers(ops):
    m, out = AdjacencyMatrix(), []
    for op in ops:
        try:
            if op[0] == "E":
                m.addEdge(op[1], op[2])
            elif op[0] == "M":
                m.markAsLoopClosureSubmap(op[1])
            elif op[0] == "D":
                out.append(str(m.getDistanceToNearestLoopClosureSubmap(op[1])))
            else:
                out.append("1" if m.isAdjacent(op[1], op[2]) else "0")
        except KeyError:
            out.append("THROW")
    return out


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "src", "AdjacencyMatrix.cpp")) or shutil.which("g++") is None,
                    reason="the reference checkout (or g++) is not present")
def test_matches_the_references_own_adjacency_matrix_on_random_graphs(tmp_path):
    exe = str(tmp_path / "adjacency_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(HERE, "cpp", "ref_shim"), "-I" + os.path.join(REF, "include"),
                    os.path.join(REF, "src", "AdjacencyMatrix.cpp"), os.path.join(HERE, "cpp", "adjacency_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    rng = np.random.default_rng(7)
    for trial in range(40):
        ops = _random_ops(rng, n_ids=4 + trial % 12)
        text = "\n".join(" ".join(str(x) for x in op) for op in ops) + "\n"
        got = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60).stdout.split()
        assert got == _python_answers(ops), (trial, ops)


# ---------------------------------------------------------------------------------------------------------- candidate filters
class _Stub:
    def __init__(self, id_, center, parent=None):
        self.id_, self.parentId_ = id_, (id_ - 1 if parent is None else parent)
        self.center = np.array(center, dtype=np.float64)
        self.moves = []

    def getMapToSubmapCenter(self):
        return self.center

    def transform(self, T):
        self.moves.append(np.array(T))


def _params(search=20.0, radius=2.0, min_between=2):
    p = P.MapperParameters()
    p.placeRecognition_.loopClosureSearchRadius_ = search
    p.submaps_.radius_ = radius
    p.placeRecognition_.minSubmapsBetweenLoopClosures_ = min_between
    return p


def _lone():
    """no edge between the stubs; the finished submap 5 hangs off a tail of three others, so that filter 6 passes (distance 2)"""
    adj = AdjacencyMatrix()
    adj.addEdge(5, 30)
    adj.addEdge(30, 31)
    adj.addEdge(31, 32)
    return adj


def _chain(n, spacing=0.5):
    subs = [_Stub(i, [spacing * i, 0.0, 0.0]) for i in range(n)]
    adj = AdjacencyMatrix()
    for i in range(1, n):
        adj.addEdge(i - 1, i)
    return subs, adj


def test_candidates_of_a_plain_chain():
    subs, adj = _chain(12)
    p = _params(search=4.0, radius=2.0)  # consecutive threshold ceil(4 / 2) = 2
    # last finished 9, active 11: 11 (active), 10 (adjacent to the active), 8 (|i - 9| = 1 and adjacent), 9 (|i - 9| = 0 <= 2) and 7
    # (|i - 9| = 2) go; every other submap is within 4 m of 9 (4.5 m away: 0 is not)
    assert getLoopClosureCandidatesIdxs(subs, adj, 9, 11, p) == [1, 2, 3, 4, 5, 6]


def test_filter_1_skips_the_active_submap():
    subs, adj = _chain(12)
    adj2 = AdjacencyMatrix()  # no edges at all: only the index-based filters act (and filter 6 sees INT_MAX)
    p = _params(search=100.0, radius=100.0)  # threshold 1
    assert 11 not in getLoopClosureCandidatesIdxs(subs, adj2, 5, 11, p)
    assert 11 in getLoopClosureCandidatesIdxs(subs, adj2, 5, 10, p)


def test_filter_2_skips_submaps_adjacent_to_the_active_one_by_id():
    subs, _ = _chain(12)
    adj = _lone()
    p = _params(search=100.0, radius=100.0)
    base = getLoopClosureCandidatesIdxs(subs, adj, 5, 11, p)
    assert 2 in base
    adj.addEdge(2, 11)
    assert 2 not in getLoopClosureCandidatesIdxs(subs, adj, 5, 11, p)
    subs[3].id_ = 10  # compared by id, not by index: a submap whose id is the active one's counts as adjacent (isAdjacent(a, a))
    assert 3 not in getLoopClosureCandidatesIdxs(subs, adj, 5, 10, p)


def test_filter_3_skips_neighbours_of_the_finished_submap():
    subs, _ = _chain(12)
    adj = _lone()
    p = _params(search=100.0, radius=100.0)
    got = getLoopClosureCandidatesIdxs(subs, adj, 5, 11, p)
    assert 4 not in got and 6 not in got and 2 in got  # |i - 5| == 1
    adj.addEdge(2, 5)  # adjacent by index to the finished one
    assert 2 not in getLoopClosureCandidatesIdxs(subs, adj, 5, 11, p)


def test_filter_4_skips_submaps_beyond_the_search_radius():
    subs, _ = _chain(12)
    adj = _lone()
    p = _params(search=2.0, radius=100.0)  # threshold ceil(2 / 100) = 1
    assert getLoopClosureCandidatesIdxs(subs, adj, 5, 11, p) == [1, 2, 3, 7, 8, 9]  # |0.5 * (i - 5)| <= 2, strict >
    subs[1].center = np.array([0.5 - 1e-9, 0.0, 0.0])  # 2 m + 1e-9 from submap 5 (at 2.5): too far
    assert 1 not in getLoopClosureCandidatesIdxs(subs, adj, 5, 11, p)


def test_filter_5_skips_consecutive_submaps():
    subs, _ = _chain(12, spacing=0.0)
    adj = _lone()
    assert getLoopClosureCandidatesIdxs(subs, adj, 5, 11, _params(search=6.0, radius=2.0)) == [0, 1, 9, 10]  # threshold 3
    assert getLoopClosureCandidatesIdxs(subs, adj, 5, 11, _params(search=6.1, radius=2.0)) == [0, 10]  # ceil(3.05) = 4


def test_filter_6_skips_when_a_loop_was_closed_too_recently():
    subs, adj = _chain(12, spacing=0.0)
    p = _params(search=4.0, radius=2.0, min_between=2)
    assert getLoopClosureCandidatesIdxs(subs, adj, 9, 11, p) == [0, 1, 2, 3, 4, 5, 6]  # nothing marked: BFS reaches 0, 9 - 1 = 8
    adj.markAsLoopClosureSubmap(7)  # two hops from 9: distance 1 < 2
    assert getLoopClosureCandidatesIdxs(subs, adj, 9, 11, p) == []
    adj.addEdge(7, 6)  # the mark goes again
    adj.markAsLoopClosureSubmap(6)  # three hops: distance 2, enough
    assert getLoopClosureCandidatesIdxs(subs, adj, 9, 11, p) == [0, 1, 2, 3, 4, 5, 6]


# ---------------------------------------------------------------------------------------------------------- transform's parent walk
class _StubCollection(SubmapCollection):
    def __init__(self, stubs):  # (no device: only what transform touches)
        self.submaps_ = stubs
        self.overlapScansBuffer_ = []


def test_transform_walks_parents_to_the_first_submap_in_the_graph():
    stubs = [_Stub(0, [0, 0, 0], parent=0), _Stub(1, [0, 0, 0], parent=0), _Stub(2, [0, 0, 0], parent=1), _Stub(3, [0, 0, 0], parent=2),
             _Stub(4, [0, 0, 0], parent=1)]
    T = [np.eye(4) for _ in range(2)]
    T[0][0, 3], T[1][0, 3] = 1.0, 2.0
    coll = _StubCollection(stubs)
    coll.transform([OptimizedTransform(T[0], 0), OptimizedTransform(T[1], 1)])  # submaps 2, 3, 4 are not in the graph
    assert [len(s.moves) for s in stubs] == [1, 1, 1, 1, 1]
    assert stubs[0].moves[0][0, 3] == 1.0 and stubs[1].moves[0][0, 3] == 2.0
    assert stubs[2].moves[0][0, 3] == 2.0 and stubs[3].moves[0][0, 3] == 2.0 and stubs[4].moves[0][0, 3] == 2.0  # 3 -> 2 -> 1
    assert coll.overlapScansBuffer_ == []


def test_transform_parent_walk_detects_a_cycle():
    stubs = [_Stub(0, [0, 0, 0], parent=0), _Stub(1, [0, 0, 0], parent=1)]
    with pytest.raises(RuntimeError, match="Stuck in a loop"):
        _StubCollection(stubs).transform([OptimizedTransform(np.eye(4), 0)])


# ---------------------------------------------------------------------------------------------------------- switching decisions
class _SwitchStub:
    def __init__(self, id_, center, hits=0):
        self.id_, self.center, self.hits = id_, np.array(center, dtype=np.float64), hits

    def getMapToSubmapCenter(self):
        return self.center

    def countVoxelMapHits(self, scan, T):
        return self.hits


class _Scan:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


class _SwitchCollection(SubmapCollection):
    def __init__(self, stubs, active, p):  # (no device: updateActiveSubmap's decisions only)
        self.submaps_, self.activeSubmapIdx_, self.params_ = stubs, active, p
        self.adjacencyMatrix_ = AdjacencyMatrix()
        self.numScansMergedInActiveSubmap_ = p.submaps_.minNumRangeData_
        self.isForceNewSubmapCreation_ = False
        self.submapId_ = len(stubs)
        self.created = []

    def createNewSubmap(self, mapToSubmap):
        self.created.append(np.array(mapToSubmap)[:3, 3].copy())
        self.submaps_.append(_SwitchStub(self.submapId_, mapToSubmap[:3, 3]))
        self.submapId_ += 1
        self.activeSubmapIdx_ = len(self.submaps_) - 1


def _at(x, y=0.0):
    T = np.eye(4)
    T[0, 3], T[1, 3] = x, y
    return T


def test_update_active_submap_decisions_in_the_reference_order():
    p = _params(radius=2.0)
    scan = _Scan(100)
    # fewer than minNumRangeData_ scans merged: nothing, even far away
    c = _SwitchCollection([_SwitchStub(0, [0, 0, 0])], 0, p)
    c.numScansMergedInActiveSubmap_ = p.submaps_.minNumRangeData_ - 1
    c.mapToRangeSensor_ = _at(50.0)
    c.updateActiveSubmap(c.mapToRangeSensor_, scan)
    assert c.activeSubmapIdx_ == 0 and not c.created
    # the closest is the active one, within the radius: nothing
    c = _SwitchCollection([_SwitchStub(0, [0, 0, 0]), _SwitchStub(1, [5, 0, 0])], 0, p)
    c.mapToRangeSensor_ = _at(1.9)
    c.updateActiveSubmap(c.mapToRangeSensor_, scan)
    assert c.activeSubmapIdx_ == 0 and not c.created
    # no submap within the radius: a new one at the pose
    c.mapToRangeSensor_ = _at(2.5, 3.0)
    c.updateActiveSubmap(c.mapToRangeSensor_, scan)
    assert c.activeSubmapIdx_ == 2 and np.allclose(c.created[0], [2.5, 3.0, 0.0])
    # another submap closest, within the radius, adjacent, fitness 41 / 100 > 0.4: switch to it
    c = _SwitchCollection([_SwitchStub(0, [0, 0, 0]), _SwitchStub(1, [3, 0, 0], hits=41)], 0, p)
    c.adjacencyMatrix_.addEdge(0, 1)
    c.mapToRangeSensor_ = _at(2.0)
    c.updateActiveSubmap(c.mapToRangeSensor_, scan)
    assert c.activeSubmapIdx_ == 1 and not c.created
    # ... fitness exactly 0.4 is not enough (strict), and the pose is within the radius of the active one: nothing
    c = _SwitchCollection([_SwitchStub(0, [0, 0, 0]), _SwitchStub(1, [3, 0, 0], hits=40)], 0, p)
    c.adjacencyMatrix_.addEdge(0, 1)
    c.mapToRangeSensor_ = _at(1.8)
    c.updateActiveSubmap(c.mapToRangeSensor_, scan)
    assert c.activeSubmapIdx_ == 0 and not c.created
    # ... not adjacent, and more than the radius from the active one: a new submap
    c = _SwitchCollection([_SwitchStub(0, [0, 0, 0]), _SwitchStub(1, [3, 0, 0], hits=100)], 0, p)
    c.mapToRangeSensor_ = _at(2.2)
    c.updateActiveSubmap(c.mapToRangeSensor_, scan)
    assert c.activeSubmapIdx_ == 2 and len(c.created) == 1
    # equally close submaps: the first wins (std::min_element, strict <)
    c = _SwitchCollection([_SwitchStub(0, [0, 0, 0]), _SwitchStub(1, [-2, 0, 0]), _SwitchStub(2, [2, 0, 0])], 0, p)
    c.mapToRangeSensor_ = _at(0.0, 1.0)
    assert c.findClosestSubmap(c.mapToRangeSensor_) == 0
    c.mapToRangeSensor_ = _at(0.0, 10.0)
    c.submaps_[0].center = np.array([0.0, -1.0, 0.0])
    assert c.findClosestSubmap(c.mapToRangeSensor_) == 1
    # localisation mode never switches
    p2 = _params(radius=2.0)
    p2.isUseInitialMap_ = True
    c = _SwitchCollection([_SwitchStub(0, [0, 0, 0])], 0, p2)
    c.mapToRangeSensor_ = _at(50.0)
    c.updateActiveSubmap(c.mapToRangeSensor_, scan)
    assert c.activeSubmapIdx_ == 0 and not c.created


def test_timestamped_ids_and_new_parameters():
    t = TimestampedSubmapId(3, 1.5)
    assert (t.submapId_, t.time_) == (3, 1.5)
    s = P.SubmapParameters()
    assert (s.radius_, s.minNumRangeData_, s.minSecondsBetweenFeatureComputation_, s.adjacencyBasedRevisitingMinFitness_,
            s.numScansOverlap_) == (20.0, 5, 5.0, 0.4, 3)
    m = P.MapperParameters()
    assert m.submaps_.radius_ == 20.0 and m.isAttemptLoopClosures_ is True
    assert P.MapperParameters().submaps_ is not m.submaps_
