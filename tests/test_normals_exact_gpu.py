"""estimate_normals held to its brute-force restatement (tests/normals_restatement.py) bit for bit, for EVERY point: in f32 storage, whose
selection has code of its own (the index in the key's low word, nrm_less<false>, the bound recovered from the key's high word, the occ5
instantiation, X widened in LDS), and on grids that do not suit the cloud -- a cell remembered from a cloud of another density, a cloud of
two densities, a radius beyond the cloud --, which is where the sweeps over several rings, the split rows, the chunked rounds, the
regula-falsi tightening, merge<4, true> and the 7-step segment search run.  Needs an MI355X.

The f32 path is deterministic -- d2 = (dx*dx + dy*dy) + dz*dz in f32 without contraction, order (d2 bits, index), f64 arithmetic on the
stored values after the selection --, so it is held as sharply as the f64 path: equality of bits, no tolerance.  A failure names the points
that differ, their neighbour counts and whether their restated lists tie at the last place.

Handles are the module's own, so what a handle remembers is known: normals_t keeps the cell it chose (h->nrm_cell) with (radius, max_nn),
the cloud's size and an age, and REUSES it for the next cloud when radius and max_nn repeat, the size is within 25 % of the remembered one
and fewer than 32 calls have passed since the pilot -- whatever the new cloud's density.  The reuse tests rest on exactly that.

Observed on an MI355X, every comparison equal in every bit (python -m pytest -s prints the table): points compared / of them with lists
shorter than max_nn / of them with a tie at the last place that only f32 makes (equal f32 d2, different f64 d2 of the stored values):
  a. per point           f32 63 847 / 27 818 / 4 578      f64 11 432 / 7 523 / -
  b. ragged sizes        f32  4 268 /    171 /     0      f64  4 268 /   171 / -
  c. reused grid         f32 18 100 /  2 900 /     0      f64 18 100 / 2 900 / -     (the short lists are the lonely cloud's: one point each)
  d. mixed density       f32  3 000 /     16 /     0      f64  3 000 /    16 / -
  e. radius beyond       f32  3 128 /      0 /     0      f64  3 128 /     0 / -
  f. degenerate grids    f32 12 192 /     22 /     0      f64 12 192 /    22 / -
  g. size in flight      f32  5 814 /  3 013 /     0      size in flight (before, after) estimate_normals: (True, False) for both scans
The f32-only ties are the offset lattice's (4 568) and the near-duplicates' (10); the scan and the seeded sheets have none, which is why
tests/test_normals_restatement_cpu.py demands them of the cases built for it.
One-line faults tried on copies of the kernel (never committed), each against this module and the three older normals tests:
  * nrm_d2 with fp contraction allowed: duplicates-f64 (1.0, 32) fails -- one point, tie at the last place, another neighbour --, the
    older tests pass, the statistical f32 one included;
  * f32 storage accepting d2 <= r^2: lattice (0.5, 48), duplicates (0.5, 48) and offset (0.5, 30) fail in f32, the older tests pass;
  * `left` without its `+ 2e-7f * worst_hi`, and `wx` without its `(1 + 1e-5) + 1e-6`: nothing fails anywhere -- each slack is covered by
    the other roundings towards letting through on these clouds (the points on cell faces included), so neither is shown to be needed.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_restatement as nr  # noqa: E402
from normals_restatement import F32, F64  # noqa: E402

from open3d_slam_amd import backend  # noqa: E402

pytestmark = pytest.mark.gpu

PREC = {F32: backend.PRECISION_F32, F64: backend.PRECISION_F64}
STATS = {}  # group -> [points compared, short lists, f32-only ties at the last place]


@pytest.fixture(scope="module")
def shared():
    """one handle per storage for the cases that hold on any cell; prints what the module compared when it is done"""
    bes = {s: backend.Backend(0, p) for s, p in PREC.items()}
    yield bes
    for be in bes.values():
        be.close()
    for group, (n, short, ties) in STATS.items():
        print(f"\n[normals exact] {group}: {n} points compared, {short} with short lists, {ties} with f32-only ties at the last place", end="")
    print()


class _Fresh:
    """handles that have estimated nothing yet; closed when the test is over"""

    def __init__(self):
        self.made = []

    def __call__(self, storage):
        be = backend.Backend(0, PREC[storage])
        self.made.append(be)
        return be

    def close(self):
        for be in self.made:
            be.close()


@pytest.fixture()
def fresh():
    f = _Fresh()
    yield f
    f.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _estimate(be, pts, radius, knn):
    c = be.upload(pts)
    be.estimate_normals(c, radius, knn)
    stored, got = be.download(c)
    be.free(c)
    return stored, got


def _hold(got, ref, lists, what):
    differ = np.flatnonzero(np.any(_bits(got) != _bits(ref), axis=1))
    assert len(differ) == 0, (what, nr.describe(differ, lists), got[differ[:3]].tolist(), ref[differ[:3]].tolist())


def _count(group, pts, lists, knn, storage):
    s = STATS.setdefault(group, [0, 0, 0])
    s[0] += len(lists.cnt)
    s[1] += int((lists.cnt < knn).sum())
    if storage == F32:
        s[2] += int(nr.f32_only_ties(pts, lists).sum())


def _run_case(be, case, storage, group, oracle=None):
    pts = case.cloud()
    for radius, knn in case.params:
        L, ref, r = nr.reference(case.name, radius, knn, storage)
        stored, got = _estimate(be, pts, r, knn)
        assert (_bits(stored) == _bits(nr.to_storage(pts, storage))).all()
        _hold(got, ref, L, (case.name, storage, r, knn))
        if oracle is not None:  # f64 storage: the oracle's own search as well
            _hold(got, oracle.estimate_normals(pts, r, knn), L, (case.name, "oracle", r, knn))
        _count(group, pts, L, knn, storage)


def _disturb(be):
    """what test_estimate_normals_f32_storage_and_repeatability does between its two runs: blocks of other sizes go through the device pool,
    so the index build's scratch and the atomic scatter's arrival order are not the first run's"""
    junk = [be.upload(np.random.default_rng(i).normal(size=(150_000 + 777 * i, 3))) for i in range(3)]
    for j in junk:
        be.free(j)


# ---------------------------------------------------------------------------------------------------------------- a. per point
@pytest.mark.parametrize("case", nr.PER_POINT, ids=lambda c: c.name)
def test_every_normal_is_the_restatement_s(shared, oracle, case):
    """a. f32 storage per point: the thinned scan, the lattice (every full list ends inside a shell of equal distances), the shuffled lattice
    with duplicates -- some of them distinct in f64 and equal in f32 --, and a lattice 1e5 / 2e5 m from the origin whose shells tie in f32
    only; max_nn 1, 2, 3 (identity covariance below three neighbours), 20, 32 | 33 (normals_kernel_occ5<P4, 32> | normals_kernel<P4, 128>),
    48, 128 and one beyond the cloud.  f64 storage at max_nn 32, 33 and 128, against the oracle's own search as well."""
    for storage in case.storages:
        _run_case(shared[storage], case, storage, f"a. per point, {storage}", oracle if storage == F64 else None)


# ---------------------------------------------------------------------------------------------------------------- b. ragged sizes
@pytest.mark.parametrize("storage", nr.STORAGES)
def test_ragged_sizes(shared, storage):
    """b. n = 1, 2, 3, 5, 15, 17, 63, 65, 4097: wavefronts whose groups have no point beside groups that have one, a last workgroup with one
    point, clouds smaller than max_nn and smaller than three points"""
    for case in nr.RAGGED:
        _run_case(shared[storage], case, storage, f"b. ragged sizes, {storage}")


# ---------------------------------------------------------------------------------------------------------------- c. + h. reused grid
@pytest.mark.parametrize("storage", nr.STORAGES)
@pytest.mark.parametrize("pair", nr.REUSE, ids=lambda p: p[0])
def test_a_cell_remembered_from_a_cloud_of_another_density(fresh, pair, storage):
    """c. A fresh handle estimates cloud A and then cloud B with the same (3.0, 20).  The second call finds h->nrm_cell > 0, the same radius and
    max_nn, an age of 0 and B's size within 25 % of A's (normals_t's `reuse`), so B is searched on the cell A's density pilot chose:
      clump-then-spread: A lies in one pilot cell, its cell clamps to radius / 64; B (20 x 20 x 1 m) then has its 20th neighbours some twenty
                         cells out on a table of four million cells -- sweeps that jump rings on the `reach` guess, rows split in two by the
                         block searched before, rin up to rmax_cells;
      lonely-then-clump: A has one point per pilot cell, its cell is the largest the heuristic gives at max_nn 20 (0.315 radius: the clamp
                         to `radius` itself needs max_nn > 64 pi); all of B lies in two cells per axis -- three thousand candidates in round
                         one, chunk after chunk of 64, the regula falsi, merge<4, true>.
    B must be the restatement's, and what a handle that never saw A gives.  A is held too (the clump on its own cell is the crowded case).
    h. B is estimated again on the remembered cell after the device pool has been disturbed: the same bytes."""
    name, first, second = pair
    radius, knn = nr.REUSE_PARAMS
    A, B = first(), second()
    key = {nr.clump_cloud: "clump", nr.spread_cloud: "spread", nr.lonely_cloud: "lonely"}
    LA, refA, _ = nr.reference(key[first], radius, knn, storage)
    LB, refB, _ = nr.reference(key[second], radius, knn, storage)
    be = fresh(storage)
    _, gotA = _estimate(be, A, radius, knn)
    b = be.upload(B)
    be.estimate_normals(b, radius, knn)  # on A's cell
    _, gotB = be.download(b)
    _disturb(be)
    be.estimate_normals(b, radius, knn)  # again on A's cell (age 1)
    _, againB = be.download(b)
    be.free(b)
    _, freshB = _estimate(fresh(storage), B, radius, knn)
    _hold(gotA, refA, LA, (name, storage, "A on its own cell"))
    _hold(gotB, refB, LB, (name, storage, "B on A's cell"))
    _hold(freshB, refB, LB, (name, storage, "B on its own cell"))
    assert gotB.tobytes() == freshB.tobytes()
    assert gotB.tobytes() == againB.tobytes()
    for pts, L in ((A, LA), (B, LB), (B, LB)):
        _count(f"c. reused grid, {storage}", pts, L, knn, storage)


# ---------------------------------------------------------------------------------------------------------------- d. + h. mixed density
@pytest.mark.parametrize("storage", nr.STORAGES)
def test_two_densities_on_one_fresh_cell(fresh, storage):
    """d. half of the points in a 5 cm clump, half on a sheet 30 m across: the pilot's mean occupancy suits neither, so one launch serves
    cells of 1500 points and neighbourhoods three rings deep, and the four groups of a wavefront finish at different times.
    h. estimated again after the pool has been disturbed (on the cell the handle now remembers): the same bytes."""
    case = nr.MIXED[0]
    radius, knn = case.params[0]
    L, ref, _ = nr.reference(case.name, radius, knn, storage)
    be = fresh(storage)
    c = be.upload(case.cloud())
    be.estimate_normals(c, radius, knn)
    _, got = be.download(c)
    _disturb(be)
    be.estimate_normals(c, radius, knn)
    _, again = be.download(c)
    be.free(c)
    _hold(got, ref, L, (case.name, storage))
    assert got.tobytes() == again.tobytes()
    _count(f"d. mixed density, {storage}", case.cloud(), L, knn, storage)


# ---------------------------------------------------------------------------------------------------------------- e. radius beyond the cloud
@pytest.mark.parametrize("storage", nr.STORAGES)
def test_a_radius_beyond_the_cloud_s_diagonal(fresh, storage):
    """e. radius = 1.001 * diagonal + 1e-3, as the k-NN route of the generalized estimator sets it (normals_t, knn_raw): nothing is ever ruled
    out by the radius, the pilot grid is eight cells across and every list is full -- pure 20-NN, held per point"""
    _run_case(fresh(storage), nr.BEYOND[0], storage, f"e. radius beyond the cloud, {storage}")


# ---------------------------------------------------------------------------------------------------------------- f. degenerate grids
@pytest.mark.parametrize("storage", nr.STORAGES)
@pytest.mark.parametrize("case", nr.DEGENERATE, ids=lambda c: c.name)
def test_degenerate_grids(fresh, case, storage):
    """f. a planar cloud (nz == 1), a collinear one (ny == nz == 1, covariances of rank one), and a lattice whose points all sit on the corners
    of the cells of the grid a fresh handle builds (cell = radius / 64 = the lattice's spacing), the outermost ones in the cells ix = 0 and
    nx - 1: fractions of exactly 0, rows and cells clipped at the grid's faces"""
    _run_case(fresh(storage), case, storage, f"f. degenerate grids, {storage}")


# ---------------------------------------------------------------------------------------------------------------- g. size in flight
def test_normals_of_a_cloud_whose_size_is_in_flight(fresh):
    """g. VoxelDownSample and estimate_normals queued one behind the other, the size not asked for in between, as
    test_random_down_sample_of_a_cloud_whose_size_is_in_flight does: the second scan of a handle meets a remembered cell and
    h->voxel_count_hint, so normals_t neither waits for the size nor runs a pilot, and the kernels take the count from the device word
    (n_dev) under a launch sized for the upper bound (4096 for some 2900 voxels).  The stream is kept busy with eight VoxelDownSamples of two
    million other points meanwhile -- a small cloud's size is otherwise published before the next call has crossed the host -- and
    size_bound, which never waits, tells whether the size was still in flight once estimate_normals had returned (printed, not asserted:
    it is a matter of timing).  The normals are the restatement's on the points the device hands back."""
    from open3d_slam_amd import synthetic as syn

    be = fresh(F32)
    scene = syn.make_scene()
    busy = be.upload_f32(np.random.default_rng(7).random((2_000_000, 3), dtype=np.float32) * np.float32(100.0))
    flight = []
    for k, yaw in enumerate((0.0, 0.2)):
        T = np.eye(4)
        T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
        T[:3, 3] = [0.4 * k, -0.3 * k, 0.0]
        raw = np.ascontiguousarray(syn.os128_scan(scene, T, n_az=32), dtype=np.float32)  # 4096 points
        r = be.upload_f32(raw)
        junk = [be.voxel_down_sample(busy, 0.05) for _ in range(8)]  # (queued, never looked at)
        v = be.voxel_down_sample(r, 0.3)
        before = be.size_bound(v)
        be.estimate_normals(v, 3.0, 20)
        lo, up = be.size_bound(v)
        flight.append((before[0] < before[1], lo < up))
        p, got = be.download(v)
        assert 2000 < len(p) < 4096
        L = nr.search(p, 3.0, 20, F32)
        assert (L.cnt == 20).sum() > 1000 and (L.cnt < 20).sum() > 1000
        _hold(got, nr.normals_from(p, L, F32), L, ("in flight", k, len(p)))
        _count("g. size in flight, f32", p, L, 20, F32)
        for x in [r, v] + junk:
            be.free(x)
    be.free(busy)
    print(f"\n[normals exact] g. size still in flight (before, after) estimate_normals, per scan: {flight}", end="")
