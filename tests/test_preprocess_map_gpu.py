"""Scan pre-processing and map-fusion kernels vs the CPU oracle, through the C-ABI (needs an MI355X)."""
import numpy as np
import pytest

import placed_binning_cases as pb
from child_process import run_child
from open3d_slam_amd import backend, synthetic as syn

pytestmark = pytest.mark.gpu
ME = "test_preprocess_map_gpu"  # (the module a child process imports as `t`)


def _match(got, ref, tol):
    """Order-insensitive comparison of two clouds that hold the same voxel set in different orders (the reference's own
    order is unordered_map iteration order): returns perm with got[perm[i]] <-> ref[i], asserting a bijection within tol.
    (Sorting by coordinates is not robust: wall points share x to 1e-7 and the order flips under rounding.)"""
    from scipy.spatial import cKDTree

    assert len(got) == len(ref)
    d, j = cKDTree(got).query(ref, k=1)
    assert d.max() <= tol, d.max()
    assert len(np.unique(j)) == len(ref)
    return j


@pytest.fixture(scope="module")
def scan():
    scene = syn.make_scene()
    return syn.os128_scan(scene, np.eye(4), n_az=256)  # 32 768 raw points


@pytest.mark.parametrize("kind,kw", [
    (backend.CROP_MAX_RADIUS, dict(rmax=12.0)),
    (backend.CROP_MIN_RADIUS, dict(rmin=6.0)),
    (backend.CROP_MIN_MAX_RADIUS, dict(rmin=2.0, rmax=30.0)),
    (backend.CROP_CYLINDER, dict(rmax=15.0, zmin=-1.0, zmax=3.0)),
    (backend.CROP_CYLINDER, dict(rmax=15.0, zmin=-1.0, zmax=3.0, invert=True)),
    (backend.CROP_NONE, dict()),
])
def test_crop_matches_oracle_exactly(backend_f64, oracle, scan, kind, kw):
    nrm = np.roll(scan, 1, axis=1)  # any per-point attribute: must be compacted with the points
    c = backend_f64.upload(scan, nrm)
    crop = backend.make_crop(kind, center=(0.5, -0.25, 0.1), **kw)
    ocrop = oracle.make_crop(kind, center=(0.5, -0.25, 0.1), **kw)
    out = backend_f64.crop_cloud(c, crop)
    xyz, n = backend_f64.download(out)
    keep = oracle.crop_indices(scan, ocrop)
    np.testing.assert_array_equal(xyz, scan[keep])  # stable compaction, bit-exact in f64 storage
    np.testing.assert_array_equal(n, nrm[keep])
    backend_f64.free(c)
    backend_f64.free(out)


def test_crop_boundary_inclusive(backend_f64):
    pts = np.array([[2.0, 0, 0], [1.9999999, 0, 0], [30.0, 0, 0], [30.0000001, 0, 0]])
    c = backend_f64.upload(pts)
    out = backend_f64.crop_cloud(c, backend.make_crop(backend.CROP_MIN_MAX_RADIUS, rmin=2.0, rmax=30.0))
    xyz, _ = backend_f64.download(out)
    np.testing.assert_array_equal(xyz, pts[[0, 2]])
    out2 = backend_f64.crop_cloud(c, backend.make_crop(backend.CROP_MAX_RADIUS, rmax=1.0))  # nothing left
    assert backend_f64.size(out2)[0] == 0
    for x in (c, out, out2):
        backend_f64.free(x)


def test_voxel_down_sample_f64_exact_set(backend_f64, oracle, scan):
    c = backend_f64.upload(scan)
    out = backend_f64.voxel_down_sample(c, 0.1)
    got, _ = backend_f64.download(out)
    ref = oracle.voxel_down_sample(scan, 0.1)
    # voxels in order of first appearance, each sum in cloud order, binary64: the oracle's array, bit for bit
    np.testing.assert_array_equal(got, ref)
    # voxel <= 0: unchanged copy (helpers.cpp:108-110)
    same = backend_f64.voxel_down_sample(c, 0.0)
    np.testing.assert_array_equal(backend_f64.download(same)[0], scan)
    for x in (c, out, same):
        backend_f64.free(x)


def test_voxel_down_sample_crowded_voxels_bit_identical(backend_f64, oracle):
    """voxels holding 1 ... 300 points (the member lists of more than 16 entries are heap-sorted), members scattered through the cloud,
    normals averaged without re-normalisation: equal to the oracle's output in values and order"""
    rng = np.random.default_rng(11)
    centres = rng.uniform(-20, 20, (400, 3))
    counts = rng.integers(1, 40, 400)
    counts[:6] = [300, 150, 64, 17, 16, 33]
    pts = np.vstack([c + rng.uniform(-0.049, 0.049, (k, 3)) for c, k in zip(centres, counts)])
    pts = pts[rng.permutation(len(pts))]
    nrm = rng.normal(size=pts.shape)
    c = backend_f64.upload(pts, nrm)
    out = backend_f64.voxel_down_sample(c, 0.1)
    got, gn = backend_f64.download(out)
    ref, rn = oracle.voxel_down_sample(pts, 0.1, nrm)
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(gn, rn)
    # crop + VoxelDownSample in one call = crop, then VoxelDownSample (grid anchored at the box of the INSIDE points)
    crop = backend.make_crop(backend.CROP_MIN_MAX_RADIUS, center=(1.0, 2.0, 0.0), rmin=3.0, rmax=17.0)
    keep = oracle.crop_indices(pts, oracle.make_crop(oracle.CROP_MIN_MAX_RADIUS, center=(1.0, 2.0, 0.0), rmin=3.0, rmax=17.0))
    ref2, rn2 = oracle.voxel_down_sample(pts[keep], 0.1, nrm[keep])
    out2 = backend_f64.crop_voxel_down_sample(c, crop, 0.1)
    got2, gn2 = backend_f64.download(out2)
    np.testing.assert_array_equal(got2, ref2)
    np.testing.assert_array_equal(gn2, rn2)
    for x in (c, out, out2):
        backend_f64.free(x)


def test_voxel_down_sample_with_normals_and_f32(backend_f32, oracle, scan):
    nrm = scan / np.linalg.norm(scan, axis=1, keepdims=True)
    c = backend_f32.upload(scan, nrm)
    out = backend_f32.voxel_down_sample(c, 0.25)
    got, gn = backend_f32.download(out)
    s32 = scan.astype(np.float32).astype(np.float64)  # what the device stores
    n32 = nrm.astype(np.float32).astype(np.float64)
    ref, rn = oracle.voxel_down_sample(s32, 0.25, n32)
    j = _match(got, ref, 5e-6)  # f32 storage of the means
    np.testing.assert_allclose(gn[j], rn, atol=1e-6)  # normals averaged, not re-normalised
    backend_f32.free(c)
    backend_f32.free(out)


def _eig_gap(pts, radius, knn):
    """relative gap between the two smallest covariance eigenvalues of every point's hybrid neighbourhood: where it
    is ~0 (collinear ring segments, 3-point neighbourhoods) the normal direction is not defined by the data"""
    from scipy.spatial import cKDTree

    d, j = cKDTree(pts).query(pts, k=knn, distance_upper_bound=radius)
    gap = np.ones(len(pts))
    for i in range(len(pts)):
        ok = np.isfinite(d[i]) & (d[i] ** 2 < radius * radius)
        nb = pts[j[i][ok]]
        if len(nb) < 3:
            continue  # identity covariance: defined result (0,0,1)
        mu = nb.mean(0)
        w = np.linalg.eigvalsh(nb.T @ nb / len(nb) - np.outer(mu, mu))
        gap[i] = (w[1] - w[0]) / max(w[2], 1e-300)
    return gap


def test_estimate_normals_matches_oracle(backend_f64, oracle, scan):
    """f64 storage: EVERY normal equals the oracle's bit for bit -- the neighbour set is the max_nn smallest by (d2, original
    index), the nine cumulants are summed in that order, and the eigen-solver / normalisation / orientation arithmetic is the
    oracle's operation by operation (csrc/det_math.hpp) -- degenerate neighbourhoods (collinear ring segments, planes through the
    sensor whose orientation sign hangs on the last bit) included.  (2.0, 48) runs the max_nn > 32 instantiation."""
    pts = oracle.voxel_down_sample(scan, 0.1)
    c = backend_f64.upload(pts)
    for radius, knn in ((3.0, 20), (1.0, 5), (0.5, 30), (2.0, 48)):
        backend_f64.estimate_normals(c, radius, knn)
        _, got = backend_f64.download(c)
        ref = oracle.estimate_normals(pts, radius, knn)
        differ = np.flatnonzero(np.any(got != ref, axis=1))
        assert len(differ) == 0, (radius, knn, len(differ), differ[:5], got[differ[:3]], ref[differ[:3]])
    backend_f64.free(c)


def test_estimate_normals_f32_storage_and_repeatability(backend_f32, oracle, scan):
    """f32 storage: distances are f32, so the neighbour set may differ from the f64 oracle's where two candidates tie within f32
    rounding; where the data define the direction it agrees to 1e-5.  And the result is a function of the cloud alone: it repeats
    bit for bit when the device pool has been disturbed in between (the index build's atomic scatter then orders the points of a
    cell differently -- which is what made the round-1 kernel irreproducible).
    (Against the f64 oracle this can only be statistical; tests/test_normals_exact_gpu.py holds every f32-storage normal bit for bit.)"""
    import hashlib

    pts = oracle.voxel_down_sample(scan, 0.1)[::3]  # thinned: keeps the python eig-gap loop short
    c = backend_f32.upload(pts)
    stored, _ = backend_f32.download(c)
    for radius, knn in ((3.0, 20), (1.0, 5)):
        backend_f32.estimate_normals(c, radius, knn)
        _, got = backend_f32.download(c)
        junk = [backend_f32.upload(np.random.default_rng(i).normal(size=(150_000 + 777 * i, 3))) for i in range(3)]
        for j in junk:
            backend_f32.free(j)
        backend_f32.estimate_normals(c, radius, knn)
        _, again = backend_f32.download(c)
        assert hashlib.sha1(got.tobytes()).hexdigest() == hashlib.sha1(again.tobytes()).hexdigest()
        ref = oracle.estimate_normals(stored, radius, knn)  # the oracle on the values the device stores
        dots = np.einsum("ij,ij->i", got, ref)
        view = np.abs(np.einsum("ij,ij->i", ref, stored / np.linalg.norm(stored, axis=1, keepdims=True)))
        well = _eig_gap(stored, radius, knn) > 1e-3
        assert well.mean() > 0.5
        assert (np.abs(dots[well]) > 1 - 1e-5).mean() > 0.999, (radius, knn, (np.abs(dots[well]) > 1 - 1e-5).mean())
        assert (dots[well & (view > 1e-4)] > 0).mean() > 0.999
        np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-6)
    backend_f32.free(c)


def test_normals_few_neighbours_and_errors(backend_f64):
    lone = np.array([[0.0, 0, 10.0], [100.0, 0, 0], [0, 50.0, -3.0]])
    c = backend_f64.upload(lone)
    backend_f64.estimate_normals(c, 0.5, 20)
    _, n = backend_f64.download(c)
    np.testing.assert_array_equal(n, [[0, 0, -1], [0, 0, 1], [0, 0, 1]])  # identity covariance -> (0,0,1) -> oriented to origin
    with pytest.raises(backend.BackendError):
        backend_f64.estimate_normals(c, 0.0, 20)
    with pytest.raises(backend.BackendError):
        backend_f64.estimate_normals(c, 1.0, 0)
    backend_f64.free(c)


def test_select_by_index(backend_f64, scan):
    nrm = -scan
    c = backend_f64.upload(scan, nrm)
    rng = np.random.default_rng(0)
    idx = rng.permutation(len(scan))[: len(scan) // 2]
    out = backend_f64.select_by_index(c, idx)
    xyz, n = backend_f64.download(out)
    np.testing.assert_array_equal(xyz, scan[idx])
    np.testing.assert_array_equal(n, nrm[idx])
    with pytest.raises(backend.BackendError):
        backend_f64.select_by_index(c, [len(scan)])
    backend_f64.free(c)
    backend_f64.free(out)


@pytest.mark.parametrize("which", ["f64", "f32"])
def test_random_down_sample_on_the_device_is_the_checkers_subset(backend_f64, backend_f32, scan, which):
    """o3ds_random_down_sample ([O3D] RandomDownSample, Odometry.cpp:29 / ScanToMapRegistration.cpp:39): the k = int(ratio * n) indices with
    the smallest keys of the counter-based generator, in cloud order -- the very index list oracle/pipeline.py draw_keep names, for every
    ratio and seed, with normals and colours riding along; ratio 0 keeps nothing, ratio 1 everything, a ratio outside [0, 1] is Open3D's
    error; the input is left as it is."""
    from oracle.pipeline import draw_keep

    be = backend_f64 if which == "f64" else backend_f32
    pts = scan if which == "f64" else scan.astype(np.float32).astype(np.float64)
    nrm = -pts / np.linalg.norm(pts, axis=1, keepdims=True)
    col = np.random.default_rng(3).uniform(0, 1, pts.shape)
    c = be.upload(pts, nrm)
    be.set_colors(c, col)
    n = len(pts)
    for ratio, seed in [(0.3, 1), (0.3, 2), (0.5, 0xDEADBEEFCAFEF00D), (0.999, 7), (1e-4, 7), (1.0, 9), (0.0, 9), (0.5 / n, 9), (1.5 / n, 11), ((n - 0.5) / n, 12)]:
        keep = draw_keep(seed, n, ratio)
        assert len(keep) == int(ratio * n)
        out = be.random_down_sample(c, ratio, seed)
        assert be.size(out)[0] == len(keep)
        if len(keep):
            xyz, nn = be.download(out)
            np.testing.assert_array_equal(xyz, pts[keep])
            if which == "f64":
                np.testing.assert_array_equal(nn, nrm[keep])
                np.testing.assert_array_equal(be.get_colors(out), col[keep])
            else:
                np.testing.assert_array_equal(nn, nrm.astype(np.float32).astype(np.float64)[keep])
        be.free(out)
    for bad in (-0.1, 1.0001, float("nan")):
        with pytest.raises(backend.BackendError, match="Illegal sampling_ratio"):
            be.random_down_sample(c, bad, 1)
    xyz, _ = be.download(c)
    np.testing.assert_array_equal(xyz, pts)
    empty = be.upload(np.zeros((0, 3)))
    out = be.random_down_sample(empty, 0.5, 1)
    assert be.size(out)[0] == 0
    for x in (c, empty, out):
        be.free(x)


def test_random_down_sample_of_a_cloud_whose_size_is_in_flight(backend_f32):
    """The head of a crop + VoxelDownSample chain is drawn from without its size reaching the host, and the draw's own size stays on the
    device in turn: the points are those drawn from the same cloud once its size is known, and the registration, the normal estimation
    and the insertion that follow take the result as it is.  Full size (131 072 raw points), twenty seeds."""
    from oracle.pipeline import draw_keep

    be = backend_f32
    scene = syn.make_scene()
    raw = np.ascontiguousarray(syn.os128_scan(scene, np.eye(4)), dtype=np.float32)
    crop = backend.make_crop(backend.CROP_MIN_MAX_RADIUS, rmin=2.0, rmax=30.0)
    r = be.upload_f32(raw)
    v = be.crop_voxel_down_sample(r, crop, 0.1)
    be.estimate_normals(v, 3.0, 20)
    ref_p, ref_n = be.download(v)  # (the size is known from here on)
    n = len(ref_p)
    for seed in range(20):
        r2 = be.upload_f32(raw)
        v2 = be.crop_voxel_down_sample(r2, crop, 0.1)
        be.estimate_normals(v2, 3.0, 20)
        d = be.random_down_sample(v2, 0.3, seed)  # queued behind the chain, whatever the host knows of its size
        lo, up = be.size_bound(d)
        assert up <= int(0.3 * len(raw)) and lo <= int(0.3 * n) <= up
        keep = draw_keep(seed, n, 0.3)
        p, nn = be.download(d)
        assert len(p) == len(keep) == int(0.3 * n)
        np.testing.assert_array_equal(p, ref_p[keep])
        np.testing.assert_array_equal(nn, ref_n[keep])
        for x in (r2, v2, d):
            be.free(x)
    be.free(r)
    be.free(v)


def test_random_down_sample_when_every_size_record_is_held():
    """Sixty-four clouds whose sizes are in flight hold all of the handle's records; the draw's own record is then made by settling the
    oldest holder -- here the very cloud that is drawn from, whose device word is the record the result inherits.  The draw must read the
    input as it is AFTER that (its size exact, no device word), not through the word its own last kernel overwrites."""
    from oracle.pipeline import draw_keep

    be = backend.Backend(0)  # (a handle of its own: which record is the oldest depends on everything the handle has done before)
    scene = syn.make_scene()
    raw = np.ascontiguousarray(syn.os128_scan(scene, np.eye(4), n_az=128), dtype=np.float32)  # 16 384 points
    crop = backend.make_crop(backend.CROP_MAX_RADIUS, rmax=30.0)
    r0 = be.upload_f32(raw)
    ref = be.crop_voxel_down_sample(r0, crop, 0.1)
    ref_p, _ = be.download(ref)
    be.free(r0)
    big = be.upload(np.random.default_rng(5).uniform(-15.0, 15.0, (4_000_000, 3)))
    keep = draw_keep(3, len(ref_p), 0.5)
    in_flight = []
    for attempt in range(3):  # (the first pass also fills the handle's block pool: an allocation from the driver waits for the device)
        raws = [be.upload_f32(raw) for _ in range(64)]
        be.synchronize()
        for _ in range(60):  # a backlog: none of the sizes below can have reached the host when the draw is made
            be.free(be.transform_cloud(big, np.eye(4)))
        lazy = [be.crop_voxel_down_sample(r, crop, 0.1) for r in raws]
        in_flight.append(be.size_bound(lazy[0])[1] == len(raw))  # still the bound?
        d = be.random_down_sample(lazy[0], 0.5, 3)
        p, _ = be.download(d)
        np.testing.assert_array_equal(p, ref_p[keep])
        for x in [d] + raws + lazy:
            be.free(x)
    for x in (ref, big):
        be.free(x)
    be.close()
    if not any(in_flight):
        pytest.skip("the sizes reached the host before the draw in every attempt: the case was not reached on this machine (the draws were right)")


def test_random_down_sample_overflow_of_the_candidate_list_is_an_error_not_an_empty_cloud(monkeypatch):
    """The draw lists the keys that share 22 leading bits with the k-th smallest (n / 4 M of them on average, room for 2 048).  Should
    the list ever overflow, nothing is kept -- and that must not pass for a result: the size of a cloud whose size was in flight fails
    to resolve, and the handle's next draw is refused.  Walked with the A/B library's O3DS_DRAW_LIST_CAP=0 (every draw overflows)."""
    monkeypatch.setenv("O3DS_DRAW_LIST_CAP", "0")
    be = backend.Backend(0, ab=True)
    scene = syn.make_scene()
    raw = np.ascontiguousarray(syn.os128_scan(scene, np.eye(4), n_az=256), dtype=np.float32)
    r = be.upload_f32(raw)
    v = be.crop_voxel_down_sample(r, backend.make_crop(backend.CROP_MAX_RADIUS, rmax=30.0), 0.1)
    d = be.random_down_sample(v, 0.3, 1)  # queued: nothing has failed on the host yet
    with pytest.raises(backend.BackendError):
        be.size(d)
    with pytest.raises(backend.BackendError, match="earlier draw"):
        be.random_down_sample(v, 0.3, 2)
    be.close()


def test_random_down_sample_at_a_million_points_keeps_exactly_k_in_cloud_order(backend_f32):
    """size-independent properties at 2^20 + 3 points: exactly int(ratio * n) points are kept, they are the checker's, and their order
    is the cloud's (the x coordinate carries the original index)"""
    from oracle.pipeline import draw_keep

    n = (1 << 20) + 3
    pts = np.zeros((n, 3))
    pts[:, 0] = np.arange(n)
    c = backend_f32.upload(pts)
    for ratio, seed in [(0.3, 5), (0.71, 6)]:
        out = backend_f32.random_down_sample(c, ratio, seed)
        xyz, _ = backend_f32.download(out)
        got = xyz[:, 0].astype(np.int64)
        assert len(got) == int(ratio * n) and np.all(np.diff(got) > 0)
        np.testing.assert_array_equal(got, draw_keep(seed, n, ratio))
        backend_f32.free(out)
    backend_f32.free(c)


def test_transform_and_append(backend_f64, oracle, scan):
    nrm = scan / np.linalg.norm(scan, axis=1, keepdims=True)
    T = syn.make_pose([1.0, -2.0, 0.5], [3.0, -4.0, 25.0])
    c = backend_f64.upload(scan, nrm)
    t = backend_f64.transform_cloud(c, T)
    xyz, n = backend_f64.download(t)
    # o3d_slam::transform in the reference's order of operations, one rounding each: the oracle's bits (and the numpy restatement's)
    np.testing.assert_array_equal(xyz, oracle.transform_points(scan, T))
    np.testing.assert_array_equal(n, oracle.transform_normals(nrm, T))
    np.testing.assert_array_equal(xyz, pb.place(T, scan))
    np.testing.assert_array_equal(n, pb.rotate(T, nrm))
    m = backend_f64.upload(scan[:100], nrm[:100])
    backend_f64.cloud_append(m, t)
    mx, mn = backend_f64.download(m)
    np.testing.assert_array_equal(mx[:100], scan[:100])
    np.testing.assert_array_equal(mx[100:], xyz)
    np.testing.assert_array_equal(mn[100:], n)
    # [O3D] operator+=: normals are dropped when the appended cloud has none
    bare = backend_f64.upload(scan[:10])
    backend_f64.cloud_append(m, bare)
    assert backend_f64.size(m) == (100 + len(scan) + 10, False)
    for x in (c, t, m, bare):
        backend_f64.free(x)


def _merge_ref(oracle, pts, nrm, voxel, ocrop):
    out, on, npass = oracle.voxelize_within_volume(pts, nrm, voxel, ocrop)
    return out, on, npass


def test_voxelize_within_volume_matches_oracle(backend_f64, oracle):
    scene = syn.make_scene()
    pts, nrm = syn.sample_map(scene, 120_000)
    nrm[::97] = np.nan  # NaN normals are skipped in the average (helpers.cpp:35-38)
    center = (3.0, -4.0, 0.0)
    m = backend_f64.upload(pts, nrm)
    backend_f64.voxelize_within_volume(m, 0.25, backend.make_crop(backend.CROP_MAX_RADIUS, center=center, rmax=15.0))
    got, gn = backend_f64.download(m)
    ref, rn, npass = _merge_ref(oracle, pts, nrm, 0.25, oracle.make_crop(oracle.CROP_MAX_RADIUS, center=center, rmax=15.0))
    assert len(got) == len(ref) and 0 < npass < len(ref)
    np.testing.assert_array_equal(got[:npass], ref[:npass])  # pass-through block: first, original order, untouched
    np.testing.assert_array_equal(gn[:npass], rn[:npass])
    j = _match(got[npass:], ref[npass:], 0.0)  # the voxel means are the oracle's bit for bit (sums in cloud order); only the order differs
    np.testing.assert_array_equal(got[npass:][j], ref[npass:])
    np.testing.assert_array_equal(gn[npass:][j], rn[npass:])
    # idempotence: voxel means stay in their voxels
    backend_f64.voxelize_within_volume(m, 0.25, backend.make_crop(backend.CROP_MAX_RADIUS, center=center, rmax=15.0))
    again, _ = backend_f64.download(m)
    _match(again[npass:], got[npass:], 1e-12)
    # voxel <= 0 leaves the map alone (helpers.cpp:119-123)
    backend_f64.voxelize_within_volume(m, 0.0, backend.make_crop(backend.CROP_MAX_RADIUS, center=center, rmax=15.0))
    assert backend_f64.size(m)[0] == len(got)
    backend_f64.free(m)


def test_map_insert_scan_sequence_matches_oracle(backend_f64, oracle):
    """Submap::insertScan (Submap.cpp:54,70-72) three times, then register a fourth scan against the fused map."""
    scene = syn.make_scene()
    voxel = 0.2
    m = None
    ref_p = np.zeros((0, 3))
    ref_n = np.zeros((0, 3))
    poses = [syn.make_pose([0.4 * k, 0.1 * k, 0.0], [0, 0, 3.0 * k]) for k in range(4)]
    for k in range(3):
        raw = syn.vlp16_scan(scene, poses[k], frame=k, n_az=512)
        sv = oracle.voxel_down_sample(raw, 0.1)
        sn = oracle.estimate_normals(sv, 3.0, 20)
        # oracle side
        tp, tn = oracle.transform_points(sv, poses[k]), oracle.transform_normals(sn, poses[k])
        ocrop = oracle.make_crop(oracle.CROP_MIN_MAX_RADIUS, center=poses[k][:3, 3], rmin=0.0, rmax=25.0)
        ref_p, ref_n, _ = oracle.voxelize_within_volume(np.vstack([ref_p, tp]), np.vstack([ref_n, tn]), voxel, ocrop)
        # device side
        s = backend_f64.upload(sv, sn)
        if m is None:
            m = backend_f64.upload(np.zeros((0, 3)))
        crop = backend.make_crop(backend.CROP_MIN_MAX_RADIUS, center=poses[k][:3, 3], rmin=0.0, rmax=25.0)
        backend_f64.map_insert_scan(m, s, poses[k], voxel, crop, max_corr_hint=1.0)
        backend_f64.free(s)
    got_p, got_n = backend_f64.download(m)
    j = _match(got_p, ref_p, 0.0)  # placed like the oracle places, summed in cloud order: the oracle's points bit for bit, in another order
    np.testing.assert_array_equal(got_p[j], ref_p)
    np.testing.assert_allclose(got_n[j], ref_n, atol=1e-9)
    # scan-to-map registration against the fused, device-resident map (index rebuilt by insert)
    raw = syn.vlp16_scan(scene, poses[3], frame=3, n_az=512)
    s = backend_f64.upload(raw)
    got = backend_f64.icp_point_to_plane_dev(s, m, 1.0, init=poses[2], max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
    ref = oracle.icp_point_to_plane(raw, ref_p, ref_n, 1.0, init=poses[2], max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
    dt, dr = syn.se3_error(got["transformation"], ref["transformation"])
    assert dt < 1e-6 and dr < 1e-6, (dt, dr)
    gt_t, gt_r = syn.se3_error(got["transformation"], poses[3])
    assert gt_t < 0.05 and gt_r < 5e-3
    backend_f64.free(s)
    backend_f64.free(m)


def test_full_scan_pipeline_config1(backend_f32, oracle):
    """BASELINE.json configs[0] on the device: two 64k VLP-16 scans, voxel 0.1 -> normals(knn 20, r 3) -> 10 ICP iterations."""
    a, b = syn.config1_inputs()
    ca, cb = backend_f32.upload(a), backend_f32.upload(b)
    va, vb = backend_f32.voxel_down_sample(ca, 0.1), backend_f32.voxel_down_sample(cb, 0.1)
    backend_f32.estimate_normals(vb, 3.0, 20)
    got = backend_f32.icp_point_to_plane_dev(va, vb, 1.0, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
    a32, b32 = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    av, bv = oracle.voxel_down_sample(a32, 0.1), oracle.voxel_down_sample(b32, 0.1)
    bn = oracle.estimate_normals(bv, 3.0, 20)
    ref = oracle.icp_point_to_plane(av, bv, bn, 1.0, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
    assert backend_f32.size(va)[0] == len(av) and backend_f32.size(vb)[0] == len(bv)
    dt, dr = syn.se3_error(got["transformation"], ref["transformation"])
    print("C1 pipeline gpu vs oracle:", dt, dr, got["fitness"], ref["fitness"])
    assert dt < 1e-3 and dr < 1e-3
    assert abs(got["fitness"] - ref["fitness"]) <= 4.0 / len(av)
    # source scan was taken 0.3 m ahead in x: T maps scan a (at origin) into scan b's frame => translation ~ -0.3
    assert abs(got["transformation"][0, 3] + 0.3) < 0.05
    for c in (ca, cb, va, vb):
        backend_f32.free(c)


def test_full_size_config4_dense_map_fusion_properties(backend_f32):
    """BASELINE.json configs[4] at full size -- a dense 2 M-point (multi-sensor) scan fused into a map at voxel 0.02 m -- through
    size-independent properties of Submap::insertScan / voxelizeWithinCroppingVolume (Submap.cpp:54,70-72, helpers.cpp:115-183):
    the voxel SET equals numpy's, means stay inside their voxels, pass-through points are untouched and come first, the fusion
    is idempotent, and sum(count x mean) reproduces the input sum (linearity)."""
    import time

    scene = syn.make_scene()
    pts, nrm = syn.sample_map(scene, 2_000_000, seed=77)
    voxel, center, rmax = 0.02, (2.0, -1.0, 0.0), 18.0
    pts32 = pts.astype(np.float32).astype(np.float64)  # what the device stores
    m = backend_f32.upload(np.zeros((0, 3)))
    s = backend_f32.upload(pts, nrm)
    crop = backend.make_crop(backend.CROP_MAX_RADIUS, center=center, rmax=rmax)
    backend_f32.synchronize()
    t0 = time.perf_counter()
    backend_f32.map_insert_scan(m, s, np.eye(4), voxel, crop, max_corr_hint=0.0)
    backend_f32.synchronize()
    dt = time.perf_counter() - t0
    got, gn = backend_f32.download(m)
    inside = np.linalg.norm(pts32 - np.array(center), axis=1) <= rmax
    n_pass = int((~inside).sum())
    assert 0 < n_pass < len(pts)
    np.testing.assert_array_equal(got[:n_pass], pts32[~inside])  # pass-through block: first, original order, bit-identical
    keys_in = np.floor(pts32[inside] * (1.0 / voxel)).astype(np.int64)
    uniq, inv, cnt = np.unique(keys_in, axis=0, return_inverse=True, return_counts=True)
    vox = got[n_pass:]
    assert len(vox) == len(uniq)  # one mean per occupied voxel
    # a mean of f32 points rounded to f32 can land on a voxel face, so the pairing goes through numpy's exact per-voxel means
    sums = np.zeros((len(uniq), 3))
    np.add.at(sums, inv.reshape(-1), pts32[inside])
    means = sums / cnt[:, None]
    from scipy.spatial import cKDTree

    d, j = cKDTree(means).query(vox)
    assert np.array_equal(np.sort(j), np.arange(len(uniq)))  # a bijection onto the occupied voxels
    assert d.max() < 4e-6  # f32 rounding of a mean of coordinates up to ~40 m
    # linearity: sum(count x mean) == sum of the inputs (to f32 storage rounding)
    np.testing.assert_allclose((vox * cnt[j][:, None]).sum(0), pts32[inside].sum(0), rtol=1e-6)
    # normals are re-normalised means (helpers.cpp:172)
    nn = np.linalg.norm(gn[n_pass:], axis=1)
    assert np.all((np.abs(nn - 1.0) < 1e-5) | (nn == 0.0))
    # idempotence: fusing nothing new leaves the voxel set where it is
    backend_f32.voxelize_within_volume(m, voxel, crop)
    again, _ = backend_f32.download(m)
    assert len(again) == len(got)
    d2, _ = cKDTree(again[n_pass:]).query(vox)
    assert d2.max() < 4e-6
    print(f"config4: {len(pts)} pts -> {len(vox)} voxels + {n_pass} pass-through in {dt*1e3:.2f} ms")
    backend_f32.free(s)
    backend_f32.free(m)


def test_pointcloud2_style_f32_upload_equals_the_double_route(backend_f32, backend_f64, scan):
    """o3ds_cloud_upload_f32 (float32 PointCloud2 -> device without the fp64 host detour of
    open3d_conversions.cpp:59-68): x/y/z picked out of strided records, every other field ignored; what the device stores is
    bit-identical to uploading the widened doubles."""
    n = 5000
    xyz32 = scan[:n].astype(np.float32)
    rec = np.zeros(n, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"), ("t", "<u4"), ("ring", "<u2"), ("pad", "<u2")])
    rec["x"], rec["y"], rec["z"], rec["intensity"], rec["ring"] = xyz32[:, 0], xyz32[:, 1], xyz32[:, 2], 7.0, np.arange(n) % 16
    shuffled = np.zeros(n, dtype=[("ring", "<u2"), ("pad", "<u2"), ("z", "<f4"), ("x", "<f4"), ("t", "<u4"), ("y", "<f4")])  # another field order
    shuffled["x"], shuffled["y"], shuffled["z"] = xyz32[:, 0], xyz32[:, 1], xyz32[:, 2]
    for be in (backend_f32, backend_f64):
        ref = be.upload(xyz32.astype(np.float64))
        want = be.download(ref)[0]
        for arr, offs in ((xyz32, (0, 4, 8)), (rec, (0, 4, 8)), (shuffled, (8, 16, 4))):
            c = be.upload_f32(arr, *offs)
            assert be.size(c)[0] == n
            np.testing.assert_array_equal(be.download(c)[0], want)
            be.free(c)
        be.free(ref)
    e = backend_f32.upload_f32(np.zeros((0, 3), np.float32))
    assert backend_f32.size(e)[0] == 0
    backend_f32.free(e)
    with pytest.raises(backend.BackendError):
        backend_f32.upload_f32(np.zeros((4, 2), np.float32))  # x/y/z do not fit an 8-byte step


@pytest.mark.parametrize("which", ["f64", "f32"])
def test_carving_a_merged_map_needs_no_sort_and_keeps_the_layout(backend_f64, backend_f32, which):
    """A map that an insertion's merge left is [outside points | voxel block in key order]: carving it takes its sorted (key, index) list
    from a stable partition instead of a radix sort, and the layout survives the carve so that the NEXT insertion merges instead of
    sorting the whole map.  Both must be invisible: the same sequence on a copy of the map whose layout is unknown to the backend (an
    identity `select_by_index` hands back the same points in a fresh cloud) goes through the library sort in the carve and in the
    insertion after it, and every cloud along the way must be the same bit for bit -- also when the carving voxel is not the map's, where
    the partition's order check fails on the device and the sort takes over."""
    be = backend_f64 if which == "f64" else backend_f32
    scene = syn.make_scene()
    poses = syn.figure_eight_poses(40, 0.1)
    crop_at = lambda T: backend.make_crop(backend.CROP_MIN_MAX_RADIUS, center=T[:3, 3], rmin=1.0, rmax=25.0)

    def pre(k):
        c = be.upload(syn.vlp16_scan(scene, poses[k], n_az=1024))
        v = be.crop_voxel_down_sample(c, backend.make_crop(backend.CROP_MIN_MAX_RADIUS, rmin=1.0, rmax=25.0), 0.1)
        be.estimate_normals(v, 1.0, 10)
        be.free(c)
        return v

    for carve_voxel in (0.1, 0.15):
        m = be.upload(np.zeros((0, 3)))
        for k in range(3):  # the third insertion already merges into the layout the second left
            s = pre(k)
            be.map_insert_scan(m, s, poses[k], 0.1, crop_at(poses[k]), 1.0)
            be.free(s)
        n = be.size(m)[0]
        twin = be.select_by_index(m, np.arange(n, dtype=np.uint32))  # same points and normals, layout unknown
        raw = be.upload(syn.vlp16_scan(scene, poses[3], n_az=1024))
        kw = dict(voxel=carve_voxel, max_length=20.0, truncation=0.1, min_dot=0.5)
        removed_m = be.map_carve(m, raw, poses[3], crop_at(poses[2]), **kw)
        removed_t = be.map_carve(twin, raw, poses[3], crop_at(poses[2]), **kw)
        assert removed_m == removed_t and removed_m > 0
        for a, b in zip(be.download(m), be.download(twin)):
            np.testing.assert_array_equal(a, b)
        s = pre(3)
        be.map_insert_scan(m, s, poses[3], 0.1, crop_at(poses[3]), 1.0)
        be.map_insert_scan(twin, s, poses[3], 0.1, crop_at(poses[3]), 1.0)
        for a, b in zip(be.download(m), be.download(twin)):
            np.testing.assert_array_equal(a, b)
        for c in (m, twin, raw, s):
            be.free(c)


def test_map_carve_matches_oracle(backend_f64, backend_f32, oracle):
    """Submap::carve on the device-resident sparse map (Submap.cpp:109-125, helpers.cpp:235-271) vs the oracle: same removed set,
    survivors in their original order, points outside the cropping volume untouched, with and without map normals."""
    rng = np.random.default_rng(11)
    scene = syn.make_scene()
    mp, mn = syn.sample_map(scene, 60_000)
    ghost = rng.uniform([-3.0, -3.0, 0.2], [3.0, 3.0, 1.5], size=(800, 3))  # clutter in free space
    mp = np.vstack([mp, ghost])
    mn = np.vstack([mn, rng.normal(size=(800, 3))])
    pose = syn.make_pose((0.3, -0.2, 0.5), (1.0, -2.0, 10.0))
    scan = syn.vlp16_scan(scene, pose, n_az=512)
    scan_w = pb.place(pose, scan)  # o3d_slam::transform in the reference's order of operations, as the device and the oracle place
    sensor = pose[:3, 3]
    rmax = 15.0
    subset = np.flatnonzero(np.linalg.norm(mp - sensor, axis=1) <= rmax)
    crop = backend.make_crop(backend.CROP_MAX_RADIUS, center=sensor, rmax=rmax)
    for nrm, kw in ((mn, {}), (None, {}), (mn, dict(voxel=0.2, max_length=6.0, truncation=0.3, min_dot=0.8))):
        ref = oracle.carve_flags(scan_w, sensor, mp, nrm, subset, **kw)
        m = backend_f64.upload(mp, nrm)
        s = backend_f64.upload(scan)
        removed = backend_f64.map_carve(m, s, pose, crop, **kw)
        got_p, got_n = backend_f64.download(m)
        assert removed == int(ref.sum())
        np.testing.assert_array_equal(got_p, mp[~ref])
        if nrm is not None:
            np.testing.assert_array_equal(got_n, nrm[~ref])
        assert 0 < removed < len(mp)
        # the same call that also hands back the carved points (Submap::toRemove_, Submap.cpp:119): the complement, in map order
        m2 = backend_f64.upload(mp, nrm)
        removed2, gone = backend_f64.map_carve_removed(m2, s, pose, crop, **kw)
        gone_p, gone_n = backend_f64.download(gone)
        assert removed2 == removed and len(gone_p) == removed
        np.testing.assert_array_equal(backend_f64.download(m2)[0], got_p)
        np.testing.assert_array_equal(gone_p, mp[ref])
        if nrm is not None:
            np.testing.assert_array_equal(gone_n, nrm[ref])
        backend_f64.free(m2)
        backend_f64.free(gone)
        # idempotence on what is left is NOT a property (new points become visible), but a second scan-less call is a no-op
        e = backend_f64.upload(np.zeros((0, 3)))
        assert backend_f64.map_carve(m, e, pose, crop, **kw) == 0 and backend_f64.size(m)[0] == len(got_p)
        n0, empty = backend_f64.map_carve_removed(m, e, pose, crop, **kw)  # nothing carved: an empty cloud comes back
        assert n0 == 0 and backend_f64.size(empty)[0] == 0
        backend_f64.free(empty)
        for c in (m, s, e):
            backend_f64.free(c)
    # f32 storage: the oracle on what the device holds (the map, its normals and the raw scan rounded to f32; the scan placed in double)
    mp32, mn32, scan32 = (pb.storage(x, "f32") for x in (mp, mn, scan))
    subset32 = np.flatnonzero(np.linalg.norm(mp32 - sensor, axis=1) <= rmax)
    np.testing.assert_array_equal(subset32, oracle.crop_indices(mp32, oracle.make_crop(oracle.CROP_MAX_RADIUS, center=sensor, rmax=rmax)))
    ref = oracle.carve_flags(pb.place(pose, scan32), sensor, mp32, mn32, subset32)
    m, s = backend_f32.upload(mp, mn), backend_f32.upload(scan)
    removed = backend_f32.map_carve(m, s, pose, crop)
    assert removed == int(ref.sum()) and 0 < removed < len(mp)
    got_p, got_n = backend_f32.download(m)
    np.testing.assert_array_equal(got_p, mp32[~ref])
    np.testing.assert_array_equal(got_n, mn32[~ref])
    with pytest.raises(backend.BackendError):
        backend_f32.map_carve(m, s, pose, crop, voxel=0.0)
    backend_f32.free(m)
    backend_f32.free(s)


def test_submap_mirror_insert_scan_with_carving(backend_f32):
    """Submap::insertScan(..., isPerformCarving) through the reference-named class: the gate nScansInsertedMap_ % N == 1
    (Submap.cpp:111) decides when the rays carve; clutter planted in free space is gone afterwards."""
    from open3d_slam_amd import parameters as P
    from open3d_slam_amd.pointcloud import PointCloud
    from open3d_slam_amd.submap import Submap

    scene = syn.make_scene()
    mp = P.lua_default_mapper_parameters()
    mp.mapBuilder_.carving_.carveSpaceEveryNscans_ = 2
    poses = [syn.make_pose((0.2 * k, 0.0, 0.5), (0.0, 0.0, 2.0 * k)) for k in range(3)]
    removed = []
    for with_carving in (False, True):
        sm = Submap(backend_f32)
        sm.setParameters(mp)
        for k in range(3):
            raw = syn.vlp16_scan(scene, poses[k], frame=k, n_az=512)
            if k == 0:  # plant clutter between the sensor and the walls in the first scan only
                rng = np.random.default_rng(3)
                raw = np.vstack([raw, rng.uniform([-2.5, -2.5, -0.3], [2.5, 2.5, 1.0], size=(300, 3))])
            rawc = PointCloud.from_numpy(backend_f32, raw)
            pre = PointCloud(backend_f32, backend_f32.voxel_down_sample(rawc.id, 0.1))
            backend_f32.estimate_normals(pre.id, 3.0, 20)
            before = len(sm.getMapPointCloud())
            sm.insertScan(rawc, pre, poses[k], 0.1 * k, isPerformCarving=with_carving)
            if with_carving:
                removed.append((sm.nScansInsertedMap_, before))
            rawc.release()
            pre.release()
        n = len(sm.getMapPointCloud())
        if not with_carving:
            n_plain = n
        sm.getMapPointCloud().release()
    assert n < n_plain - 30  # scan 1 (nScansInsertedMap_ == 1 at that moment) carved the clutter; scans 0 and 2 did not carve


def test_overlap_indices_match_oracle(backend_f64, backend_f32, oracle, scan):
    """computeIndicesOfOverlappingPoints (helpers.cpp:307-332) on the device vs the oracle: exact index sets in f64 storage."""
    scene = syn.make_scene()
    tgt, _ = syn.sample_map(scene, 80_000)
    src = scan[:20000]
    T = syn.ground_truth_pose()
    s, t = backend_f64.upload(src), backend_f64.upload(tgt)
    for Tm, voxel, mn in ((T, 0.5, 1), (np.eye(4), 0.3, 3), (T, 2.0, 10)):
        r_s, r_t = oracle.overlap_indices(src, tgt, Tm, voxel, mn)
        g_s, g_t = backend_f64.overlap_indices(s, t, Tm, voxel, mn)
        np.testing.assert_array_equal(g_s, r_s)  # (the oracle's are ascending)
        np.testing.assert_array_equal(g_t, r_t)
        assert np.all(np.diff(g_s.astype(np.int64)) > 0) and np.all(np.diff(g_t.astype(np.int64)) > 0)
    g_s, g_t = backend_f64.overlap_indices(s, t, np.eye(4), 0.3, 3)
    r_s, r_t = oracle.overlap_indices(src, tgt, np.eye(4), 0.3, 3)  # identity: no rounding at all in the placement
    np.testing.assert_array_equal(g_s, r_s)
    np.testing.assert_array_equal(g_t, r_t)
    far_s, far_t = backend_f64.overlap_indices(s, t, syn.make_pose((1000.0, 0.0, 0.0), (0.0, 0.0, 0.0)), 0.5, 1)
    assert len(far_s) == 0 and len(far_t) == 0
    with pytest.raises(backend.BackendError):
        backend_f64.overlap_indices(s, t, T, 0.5, 0)  # assert_ge(minNumPointsPerVoxel, 1)
    e = backend_f64.upload(np.zeros((0, 3)))
    es, et = backend_f64.overlap_indices(e, t, T, 0.5, 1)
    assert len(es) == 0 and len(et) == 0
    for c in (s, t, e):
        backend_f64.free(c)
    s32, t32 = backend_f32.upload(src), backend_f32.upload(tgt)
    g_s, g_t = backend_f32.overlap_indices(s32, t32, T, 0.5, 1)
    # f32 storage: the oracle on what the device bins -- the f32 target, and the f32 source placed in double and rounded to f32
    placed32 = pb.storage(pb.place(T, pb.storage(src, "f32")), "f32")
    r_s, r_t = oracle.overlap_indices(placed32, pb.storage(tgt, "f32"), np.eye(4), 0.5, 1)
    assert 0 < len(r_s) < len(src)
    np.testing.assert_array_equal(g_s, r_s)
    np.testing.assert_array_equal(g_t, r_t)
    backend_f32.free(s32)
    backend_f32.free(t32)


def test_dense_voxel_map_matches_oracle(backend_f64, backend_f32, oracle):
    """VoxelizedPointCloud on the device (Voxel.hpp:38-76, Voxel.cpp:18-114): incremental insertion of several clouds == the oracle's
    fusion of their concatenation (same voxel set, counts, means and un-normalised mean normals), growth of the table, placement by
    a pose, the reference's transform() as written, and order-independence (bitwise repeatable)."""
    from scipy.spatial import cKDTree

    scene = syn.make_scene()
    voxel = 0.1
    clouds = [syn.sample_map(scene, n, seed=50 + k) for k, n in enumerate((30_000, 5_000, 120_000))]  # the third insert forces a rehash
    dm = backend_f64.dense_map_create(voxel)
    assert backend_f64.dense_map_size(dm) == 0
    for p, n in clouds:
        c = backend_f64.upload(p, n)
        backend_f64.dense_map_insert(dm, c)
        backend_f64.free(c)
    allp, alln = np.vstack([c[0] for c in clouds]), np.vstack([c[1] for c in clouds])
    rp, rn, rc = oracle.dense_fuse(allp, alln, voxel)
    assert backend_f64.dense_map_size(dm) == len(rp)
    out = backend_f64.dense_map_to_cloud(dm)
    gp, gn = backend_f64.download(out)
    keys = np.floor(gp / voxel).astype(np.int64)
    assert np.all(np.diff(((keys[:, 2] * (1 << 21) + keys[:, 1]) * (1 << 21) + keys[:, 0])) > 0)  # ascending voxel key, every voxel once
    d, j = cKDTree(rp).query(gp)
    assert np.array_equal(np.sort(j), np.arange(len(rp))) and d.max() < 1e-8  # fixed-point sums: 1 nm per inserted point
    np.testing.assert_allclose(gn, rn[j], atol=1e-9)
    again = backend_f64.dense_map_to_cloud(dm)
    np.testing.assert_array_equal(backend_f64.download(again)[0], gp)
    # a second map built in another insertion order holds bit-identical sums
    dm2 = backend_f64.dense_map_create(voxel)
    for p, n in reversed(clouds):
        c = backend_f64.upload(p, n)
        backend_f64.dense_map_insert(dm2, c)
        backend_f64.free(c)
    o2 = backend_f64.dense_map_to_cloud(dm2)
    p2, n2 = backend_f64.download(o2)
    np.testing.assert_array_equal(p2, gp)
    np.testing.assert_array_equal(n2, gn)
    # placement by a pose (Submap::insertScanDenseMap), in the reference's order of operations: the oracle's voxels, counts and means
    T = syn.make_pose((1.5, -0.7, 0.2), (2.0, -1.0, 30.0))
    dm3 = backend_f64.dense_map_create(voxel)
    c = backend_f64.upload(*clouds[0])
    backend_f64.dense_map_insert(dm3, c, T)
    tp3, tn3 = pb.place(T, clouds[0][0]), pb.rotate(T, clouds[0][1])
    rp3, rn3, rc3 = oracle.dense_fuse(tp3, tn3, voxel)
    assert backend_f64.dense_map_size(dm3) == len(rp3)
    uniq3, cnt3, mean3, mean_n3, order3 = pb.dense_voxels(tp3, tn3, voxel)
    np.testing.assert_array_equal(rc3, cnt3[order3])  # (the restatement's voxels are the oracle's)
    o3 = backend_f64.dense_map_to_cloud(dm3)
    gp3, gn3 = backend_f64.download(o3)
    # voxel by voxel in ascending key order, against the mean of the oracle's members of that voxel: a member in the wrong voxel moves two
    # means (or adds or removes a voxel), so this holds the key set and the counts; the bound is that of the fixed-point sums
    assert len(gp3) == len(uniq3) and np.abs(gp3 - mean3).max() < 1e-8
    np.testing.assert_allclose(gn3, mean_n3, atol=1e-9)
    backend_f64.free(o3)
    # VoxelizedPointCloud::transform as written: keys stay, sums are moved like points (translation once; normals too)
    dm4 = backend_f64.dense_map_create(1.0)
    c4 = backend_f64.upload(np.array([[0.2, 0.2, 0.2], [0.4, 0.6, 0.8]]), np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]))
    backend_f64.dense_map_insert(dm4, c4)
    Tq = syn.make_pose((10.0, 20.0, 30.0), (0.0, 0.0, 90.0))
    backend_f64.dense_map_transform(dm4, Tq)
    o4 = backend_f64.dense_map_to_cloud(dm4)
    p4, n4 = backend_f64.download(o4)
    np.testing.assert_allclose(p4, [(Tq[:3, :3] @ np.array([0.6, 0.8, 1.0]) + Tq[:3, 3]) / 2.0], atol=1e-8)
    np.testing.assert_allclose(n4, [(Tq[:3, :3] @ np.array([1.0, 1.0, 0.0]) + Tq[:3, 3]) / 2.0], atol=1e-8)
    for cid in (out, again, o2, c, o4, c4):
        backend_f64.free(cid)
    for d_ in (dm, dm2, dm3, dm4):
        backend_f64.dense_map_free(d_)
    # f32 storage: same voxel count up to points sitting on faces after rounding to f32, no normals at all
    dmf = backend_f32.dense_map_create(voxel)
    cf = backend_f32.upload(clouds[0][0])
    backend_f32.dense_map_insert(dmf, cf)
    r32, _, _ = oracle.dense_fuse(clouds[0][0].astype(np.float32).astype(np.float64), None, voxel)
    assert backend_f32.dense_map_size(dmf) == len(r32)
    of = backend_f32.dense_map_to_cloud(dmf)
    assert backend_f32.size(of) == (len(r32), False)
    backend_f32.free(of)
    backend_f32.free(cf)
    backend_f32.dense_map_free(dmf)
    with pytest.raises(backend.BackendError):
        backend_f32.dense_map_create(0.0)


def test_full_size_config4_dense_voxel_map(backend_f32):
    """BASELINE.json configs[4] with the reference's own dense map (VoxelizedPointCloud, the 'TSDF-style' running sums): 2 M points at
    voxel 0.02 m in four insertions; voxel SET equals numpy's, total count is conserved through the means (linearity), and a second
    identical insertion doubles every count without moving any mean (idempotence of the means)."""
    import time

    from scipy.spatial import cKDTree

    scene = syn.make_scene()
    pts, _ = syn.sample_map(scene, 2_000_000, seed=78)
    pts32 = pts.astype(np.float32).astype(np.float64)
    voxel = 0.02
    dm = backend_f32.dense_map_create(voxel)
    chunks = np.array_split(np.arange(len(pts)), 4)
    ids = [backend_f32.upload(pts[c]) for c in chunks]
    backend_f32.synchronize()
    t0 = time.perf_counter()
    for c in ids:
        backend_f32.dense_map_insert(dm, c)
    backend_f32.synchronize()
    dt = time.perf_counter() - t0
    uniq, inv, cnt = np.unique(np.floor(pts32 * (1.0 / voxel)).astype(np.int64), axis=0, return_inverse=True, return_counts=True)
    assert backend_f32.dense_map_size(dm) == len(uniq)
    out = backend_f32.dense_map_to_cloud(dm)
    vox = backend_f32.download(out)[0]
    sums = np.zeros((len(uniq), 3))
    np.add.at(sums, inv.reshape(-1), pts32)
    means = sums / cnt[:, None]
    d, j = cKDTree(means).query(vox)
    assert np.array_equal(np.sort(j), np.arange(len(uniq))) and d.max() < 4e-6
    np.testing.assert_allclose((vox * cnt[j][:, None]).sum(0), pts32.sum(0), rtol=1e-6)
    for c in ids:  # everything once more: same voxels, same means
        backend_f32.dense_map_insert(dm, c)
    assert backend_f32.dense_map_size(dm) == len(uniq)
    out2 = backend_f32.dense_map_to_cloud(dm)
    np.testing.assert_array_equal(backend_f32.download(out2)[0], vox)
    print(f"config4 dense map: {len(pts)} pts -> {len(uniq)} voxels in {dt*1e3:.2f} ms")
    for c in ids + [out, out2]:
        backend_f32.free(c)
    backend_f32.dense_map_free(dm)


def test_undistort_matches_oracle(backend_f64, backend_f32, oracle, scan):
    """o3ds_cloud_undistort = ConstantVelocityMotionCompensation::undistortInputPointCloud (MotionCompensation.cpp:64-139)."""
    v, w = np.array([1.5, -0.4, 0.1]), np.array([0.02, -0.05, 0.6])
    for cw in (False, True):
        ref = oracle.undistort(scan, v, w, 0.1, cw)
        c = backend_f64.upload(scan)
        backend_f64.undistort(c, v, w, 0.1, cw)
        np.testing.assert_allclose(backend_f64.download(c)[0], ref, atol=1e-12)
        backend_f64.free(c)
    c = backend_f32.upload(scan)
    backend_f32.undistort(c, v, w, 0.1)
    np.testing.assert_allclose(backend_f32.download(c)[0], oracle.undistort(scan.astype(np.float32).astype(np.float64), v, w, 0.1), atol=4e-6)
    backend_f32.undistort(c, [0, 0, 0], [0, 0, 0], 0.1)  # no motion: a no-op
    with pytest.raises(backend.BackendError):
        backend_f32.undistort(c, v, w, 0.0)
    backend_f32.free(c)


def _azimuth_edge_points(prec):
    """about 200 hand-placed points for the phase of undistort_kernel: azimuth exactly 0 (y = +0 and y = -0 with x > 0), the same on the
    other side (x < 0: azimuth pi from either zero), the origin, the first representable azimuth either side of 0 (y = +-the smallest
    positive number of the storage type: the phase jumps from ~0 to ~1 there, or the other way round for a clockwise sensor), points on
    +-x and +-y, and the quadrants' interiors; at several ranges and heights."""
    rng = np.random.default_rng(17)
    tiny = float(np.nextafter(np.float64(0.0), np.float64(1.0)) if prec == "f64" else np.nextafter(np.float32(0.0), np.float32(1.0)))
    pts = []
    for r, z in ((0.5, 0.0), (1.0, -0.3), (3.0, 0.7), (12.0, 2.0), (19.0, -1.5)):
        # (the smallest number only where y / x is a number too: beyond that range whether atan2 gives +-0 or +-tiny is its own rounding)
        for y in (0.0, -0.0, 1e-30, -1e-30) + ((tiny, -tiny) if r <= 1.0 else (8.0 * tiny * r, -8.0 * tiny * r)):
            pts += [[r, y, z], [-r, y, z]]
        pts += [[0.0, r, z], [0.0, -r, z], [-0.0, r, z], [-0.0, -r, z], [r, r, z], [-r, r, z], [-r, -r, z], [r, -r, z]]
    pts += [[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -2.0]]  # the origin and points above and below it: azimuth 0 by atan2(+0, +0)
    ang = np.concatenate([rng.uniform(q * np.pi / 2 + 0.01, (q + 1) * np.pi / 2 - 0.01, 25) for q in range(4)])
    rad = rng.uniform(0.5, 20.0, len(ang))
    pts += np.column_stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-2.0, 3.0, len(ang))]).tolist()
    return pb.storage(np.array(pts), prec)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("clockwise", [False, True])
def test_undistort_phase_at_azimuth_zero_and_its_neighbours(backend_f64, backend_f32, oracle, prec, clockwise):
    """The phase of a point is 0 at azimuth exactly 0 (MotionCompensation.cpp:120-139: the `wrapped != 0` branch), azimuth / 2 pi after
    the wrap of negative angles, and 1 - that for a clockwise sensor -- so it jumps by a whole scan between the two numbers next to
    y = 0 on the +x side.  With |v| D >= 0.36 m, a phase taken from the wrong branch moves the point by more than 0.1 m: far outside the
    tolerances (atan2 and sincos are not specified to the bit, so those stay: 1e-12 in f64 storage, 4e-6 in f32)."""
    be = backend_f64 if prec == "f64" else backend_f32
    pts = _azimuth_edge_points(prec)
    assert 180 <= len(pts) <= 220
    tol = 1e-12 if prec == "f64" else 4e-6
    for v, w in (((3.0, -2.0, 1.0), (0.2, -0.3, 1.5)), ((-2.5, 1.5, 0.5), (-0.1, 0.2, -2.0))):  # the second with a negative yaw rate
        v, w = np.array(v), np.array(w)
        ref = oracle.undistort(pts, v, w, 0.1, clockwise)
        # the inputs do tell the branches apart: the other spin direction, and a phase of 0 everywhere, are both 0.1 m off somewhere
        assert np.abs(oracle.undistort(pts, v, w, 0.1, not clockwise) - ref).max() > 0.1
        moved = np.linalg.norm(ref - pts, axis=1)
        on_zero = (pts[:, 1] == 0.0) & (pts[:, 0] >= 0.0) & ~np.signbit(pts[:, 0])
        np.testing.assert_array_equal(ref[on_zero], pts[on_zero])  # azimuth exactly 0: phase 0, the point stays
        assert (moved > 0.1).sum() > 50
        c = be.upload(pts)
        be.undistort(c, v, w, 0.1, clockwise)
        got = be.download(c)[0]
        be.free(c)
        np.testing.assert_allclose(got, ref, rtol=0, atol=tol)


def test_dense_map_count_occupied_matches_numpy(backend_f64, scan):
    """the numerator of SubmapCollection::isSwitchingSubmapsConsistant (SubmapCollection.cpp:352-364): scan points (placed by the
    pose) whose voxel is occupied in the candidate submap's voxel map -- against a numpy set lookup on the same keys."""
    scene = syn.make_scene()
    mp, _ = syn.sample_map(scene, 150_000)
    voxel = 0.25
    dm = backend_f64.dense_map_create(voxel)
    m = backend_f64.upload(mp)
    backend_f64.dense_map_insert(dm, m)
    occ = {tuple(k) for k in np.floor(mp * (1.0 / voxel)).astype(np.int64)}
    s = backend_f64.upload(scan)
    hits_id = backend_f64.dense_map_count_occupied(dm, s)  # identity placement: no rounding in between
    want = sum(tuple(k) in occ for k in np.floor(scan * (1.0 / voxel)).astype(np.int64))
    assert hits_id == want and 0 < want <= len(scan)
    T = syn.ground_truth_pose()
    hits = backend_f64.dense_map_count_occupied(dm, s, T)
    want_T = sum(tuple(k) in occ for k in np.floor(pb.place(T, scan) * (1.0 / voxel)).astype(np.int64))  # placed as the device and the oracle place
    assert hits == want_T, (hits, want_T)
    assert 0 < want_T < want  # (this fixture is taken at the identity pose, so moving it lowers the overlap: 10686 -> 8574 of 32768)
    far = backend_f64.dense_map_count_occupied(dm, s, syn.make_pose((500.0, 0.0, 0.0), (0.0, 0.0, 0.0)))
    assert far == 0
    e = backend_f64.dense_map_create(voxel)
    assert backend_f64.dense_map_count_occupied(e, s) == 0  # empty map
    for c in (m, s):
        backend_f64.free(c)
    backend_f64.dense_map_free(dm)
    backend_f64.dense_map_free(e)


def test_dense_map_carve_matches_oracle(backend_f64, oracle):
    """Submap::carve for the dense map (Submap.cpp:126-136, helpers.cpp:347-377, VoxelHashMap.cpp:13-44) on the device table vs the
    oracle: the same set of removed voxels, voxels out of reach untouched, removed voxels gone from to_cloud / count_occupied and
    usable again by a later insert; a zero neighbourhood radius is refused (the reference's ray step would be zero)."""
    rng = np.random.default_rng(5)
    voxel = 0.1
    wall = np.stack(np.meshgrid([3.05], np.arange(-1.0, 1.0, 0.1) + 0.05, np.arange(0.0, 1.5, 0.1) + 0.05, indexing="ij"), -1).reshape(-1, 3)
    clutter = np.unique(np.floor(rng.uniform([0.5, -0.8, 0.2], [2.5, 0.8, 1.2], size=(400, 3)) / voxel), axis=0) * voxel + 0.05
    behind = wall + [0.3, 0.0, 0.0]
    pts = np.vstack([wall, clutter, behind]) + rng.uniform(-0.03, 0.03, size=(len(wall) * 2 + len(clutter), 3))  # anywhere inside the voxels
    sensor = np.array([0.013, -0.021, 0.71])
    scan = wall[rng.choice(len(wall), 200, replace=True)] + rng.normal(scale=0.004, size=(200, 3))
    for kw in (dict(radius=0.1), dict(radius=0.05, truncation=0.3), dict(radius=0.17, max_length=2.0)):
        dm = backend_f64.dense_map_create(voxel)
        m = backend_f64.upload(pts)
        backend_f64.dense_map_insert(dm, m)
        before_id = backend_f64.dense_map_to_cloud(dm)
        before = backend_f64.download(before_id)[0]  # one mean per voxel, ascending key order
        ref = oracle.dense_carve(scan, sensor, before, voxel, **kw)
        s = backend_f64.upload(scan)
        removed = backend_f64.dense_map_carve(dm, s, sensor, **kw)
        assert removed == int(ref.sum()) and 0 < removed < len(before), (kw, removed, int(ref.sum()))
        after_id = backend_f64.dense_map_to_cloud(dm)
        after = backend_f64.download(after_id)[0]
        np.testing.assert_array_equal(after, before[~ref])  # exactly the oracle's voxels are gone, the rest untouched and in order
        assert backend_f64.dense_map_size(dm) == len(before) - removed
        assert backend_f64.dense_map_carve(dm, s, sensor, **kw) == 0  # same rays, same reach, and everything in reach is already gone
        # a removed voxel can be filled again and then counts from one
        gone = before[ref][:1]
        g = backend_f64.upload(gone)
        assert backend_f64.dense_map_count_occupied(dm, g) == 0
        backend_f64.dense_map_insert(dm, g)
        assert backend_f64.dense_map_count_occupied(dm, g) == 1 and backend_f64.dense_map_size(dm) == len(before) - removed + 1
        for cid in (m, s, g, before_id, after_id):
            backend_f64.free(cid)
        backend_f64.dense_map_free(dm)
    dm = backend_f64.dense_map_create(voxel)
    s = backend_f64.upload(scan)
    assert backend_f64.dense_map_carve(dm, s, sensor) == 0  # empty map: nothing to do (Submap.cpp:128)
    with pytest.raises(backend.BackendError):
        backend_f64.dense_map_carve(dm, s, sensor, radius=0.0)
    backend_f64.free(s)
    backend_f64.dense_map_free(dm)


def test_dense_map_survives_many_carve_insert_cycles(backend_f64):
    """Carving leaves count-0 tombstones in the open-addressing table.  The load factor must be accounted in OCCUPIED slots (live +
    tombstones) and tombstones dropped on rehash, otherwise repeated carve / insert cycles fill the table and a probe never finds a
    free slot (a hang).  60 cycles, each inserting ~1000 fresh voxels into a small table and carving most of them away again."""
    voxel = 0.1
    dm = backend_f64.dense_map_create(voxel)
    sensor = np.array([0.013, -0.021, 0.013])
    live_expected = None
    for cycle in range(60):
        # a fresh slab of voxels at a new height every cycle, in front of the sensor
        ys, xs = np.meshgrid(np.arange(-1.5, 1.5, 0.1) + 0.05, np.arange(1.0, 4.0, 0.1) + 0.05, indexing="ij")
        slab = np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, 0.05 + 0.1 * cycle)], 1)
        c = backend_f64.upload(slab)
        backend_f64.dense_map_insert(dm, c)
        n_before = backend_f64.dense_map_size(dm)
        # rays to a row of points beyond the slab at the same height sweep most of it away
        far = np.stack([np.full(60, 6.0), np.linspace(-2.2, 2.2, 60), np.full(60, 0.05 + 0.1 * cycle)], 1)
        s = backend_f64.upload(far)
        removed = backend_f64.dense_map_carve(dm, s, sensor + [0.0, 0.0, 0.1 * cycle], radius=0.1, max_length=10.0)
        assert removed > 0 and backend_f64.dense_map_size(dm) == n_before - removed
        live_expected = n_before - removed
        backend_f64.free(c)
        backend_f64.free(s)
    out = backend_f64.dense_map_to_cloud(dm)
    assert backend_f64.size(out)[0] == live_expected
    backend_f64.free(out)
    backend_f64.dense_map_free(dm)


@pytest.mark.gpu
def test_f32_egress_records_pcd_and_assembled_map(backend_f32, backend_f64, scan, tmp_path):
    """o3ds_cloud_download_f32 (the way out): float32 records in the PointCloud2 layout of
    open3d_conversions::open3dToRos (open3d_conversions.cpp:19-53) and in the row layout of the binary PCD that saveToFile
    (output.cpp:39-47) writes; bit-exact against the numpy narrowing of what the double route downloads.  Then saveToFile /
    readPcd and Mapper::getAssembledMapPointCloud (Mapper.cpp:183-208) on device clouds."""
    from open3d_slam_amd import output
    from open3d_slam_amd.pointcloud import PointCloud

    n = 4097
    pts = scan[:n]
    for be in (backend_f32, backend_f64):
        c = be.upload(pts)
        v = be.voxel_down_sample(c, 0.3)
        be.estimate_normals(v, 2.0, 20)
        xyz, nrm = be.download(v)
        m = len(xyz)
        # PointCloud2 'xyz': 16-byte step, 4 bytes of zero padding
        pc2 = be.download_f32(v)
        assert pc2.shape == (m, 16) and pc2.dtype == np.uint8
        np.testing.assert_array_equal(pc2[:, :12].copy().view(np.float32).reshape(m, 3), xyz.astype(np.float32))
        assert not pc2[:, 12:].any()
        # an arbitrary layout with normals and unused bytes in between
        rec = be.download_f32(v, 40, 20, 4, 12, 24)
        f = rec.copy().view(np.float32).reshape(m, 10)
        np.testing.assert_array_equal(f[:, [5, 1, 3]], xyz.astype(np.float32))
        np.testing.assert_array_equal(f[:, 6:9], nrm.astype(np.float32))
        assert not f[:, [0, 2, 4, 9]].any()
        # the round trip through the f32 ingest is the identity on the f32 values
        back = be.upload_f32(pc2)
        np.testing.assert_array_equal(be.download(back)[0].astype(np.float32), xyz.astype(np.float32))
        be.free(back)
        # PCD file
        cloud = PointCloud(be, v, owns=False)
        assert output.saveToFile(str(tmp_path / "map"), cloud)             # '.pcd' appended
        assert output.saveToFile(str(tmp_path / "map2.pcd"), cloud)        # kept
        for name in ("map.pcd", "map2.pcd"):
            p, q, rgb = output.readPcd(str(tmp_path / name))
            assert rgb is None
            np.testing.assert_array_equal(p, xyz.astype(np.float32))
            np.testing.assert_array_equal(q, nrm.astype(np.float32))
        head = open(tmp_path / "map.pcd", "rb").read(400).split(b"DATA binary\n")[0].decode()
        assert head.splitlines()[:3] == ["# .PCD v0.7 - Point Cloud Data file format", "VERSION 0.7", "FIELDS x y z normal_x normal_y normal_z"]
        assert f"WIDTH {m}" in head and "HEIGHT 1" in head and f"POINTS {m}" in head
        bare = PointCloud(be, c, owns=False)                                # no normals: x y z rows only
        assert output.saveToFile(str(tmp_path / "raw.pcd"), bare)
        p, q, rgb = output.readPcd(str(tmp_path / "raw.pcd"))
        assert q is None and rgb is None
        np.testing.assert_array_equal(p, pts.astype(np.float32))
        # colours: the packed rgb field, (int)(255 c) for PointCloud2 and clamp / round for the PCD
        colc = np.random.default_rng(9).uniform(-0.1, 1.1, xyz.shape)
        be.set_colors(v, colc)
        pc2c = cloud.to_pointcloud2()
        assert pc2c.shape == (m, 32)
        np.testing.assert_array_equal(pc2c[:, :12].copy().view(np.float32).reshape(m, 3), xyz.astype(np.float32))
        stored = be.get_colors(v)  # what the device holds (f32-rounded in f32 storage)
        np.testing.assert_array_equal(pc2c[:, [18, 17, 16]], (255.0 * stored).astype(np.int64).astype(np.uint8))
        assert not pc2c[:, 12:16].any() and not pc2c[:, 19:].any()
        assert output.saveToFile(str(tmp_path / "col.pcd"), cloud)
        p, q, rgb = output.readPcd(str(tmp_path / "col.pcd"))
        np.testing.assert_array_equal(p, xyz.astype(np.float32))
        np.testing.assert_array_equal(q, nrm.astype(np.float32))
        np.testing.assert_array_equal(rgb, np.rint(np.clip(stored, 0.0, 1.0) * 255.0).astype(np.uint8))
        assert b"FIELDS x y z normal_x normal_y normal_z rgb\n" in open(tmp_path / "col.pcd", "rb").read(300)
        with pytest.raises(backend.BackendError) as ei:
            be.download_f32(c, 16, 0, 4, 8, None, 12, 0)                    # rgb requested, cloud has no colours
        assert ei.value.code == -6
        # ... and in: rosToOpen3d with a fourth field
        recs = np.zeros(m, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "<f4"), ("rgb", "<u4")])
        recs["x"], recs["y"], recs["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        recs["rgb"] = pc2c[:, 16:20].copy().view("<u4").reshape(m)
        back = PointCloud.from_pointcloud2(be, recs, fourth_field=("rgb", 16))
        np.testing.assert_allclose(back.colors_, pc2c[:, [18, 17, 16]] / 255.0, rtol=0, atol=1e-7 if be is backend_f32 else 0)
        lidar = np.zeros(m, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])
        lidar["x"], lidar["y"], lidar["z"], lidar["intensity"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], np.linspace(0.0, 300.0, m)
        li = PointCloud.from_pointcloud2(be, lidar, fourth_field=("intensity", 12))
        first_byte = lidar["intensity"].copy().view(np.uint8).reshape(m, 4)[:, 0].astype(np.float64)  # the reference's uint8 iterator
        np.testing.assert_array_equal(li.colors_, np.repeat(first_byte[:, None], 3, axis=1))
        back.release()
        li.release()
        be.set_colors(v, None)
        # error behaviour
        with pytest.raises(backend.BackendError) as ei:
            be.download_f32(c, 24, 0, 4, 8, 12)                             # normals requested, cloud has none
        assert ei.value.code == -2
        with pytest.raises(backend.BackendError):
            be.download_f32(v, 20, 0, 4, 8, 12)                             # normal fields do not fit the step
        with pytest.raises(backend.BackendError):
            be.download_f32(v, 8)                                           # x/y/z do not fit

        # assembled map of two submaps = their clouds, concatenated in order; display voxelisation = plain voxel_down_sample
        class _Sub:  # the one member of Submap the assembly touches
            def __init__(self, cloud):
                self._c = cloud

            def getMapPointCloud(self):
                return self._c

        c2 = be.upload(scan[n:2 * n])
        v2 = be.voxel_down_sample(c2, 0.3)
        be.estimate_normals(v2, 2.0, 20)
        xyz2, nrm2 = be.download(v2)
        whole = output.assembleMapPointCloud(be, [_Sub(PointCloud(be, v, owns=False)), _Sub(PointCloud(be, v2, owns=False))])
        wp, wn = be.download(whole.id)
        np.testing.assert_array_equal(wp, np.vstack([xyz, xyz2]))
        np.testing.assert_array_equal(wn, np.vstack([nrm, nrm2]))
        np.testing.assert_array_equal(be.download(v)[0], xyz)               # the submaps themselves are untouched
        shown = output.voxelize(be, 0.5, whole)
        ref = be.voxel_down_sample(whole.id, 0.5)
        np.testing.assert_array_equal(be.download(shown.id)[0], be.download(ref)[0])
        assert output.voxelize(be, 0.0, whole) is whole
        empty = output.assembleMapPointCloud(be, [])
        assert len(empty) == 0 and be.download_f32(empty.id).shape == (0, 16)
        for x in (shown, whole, empty):
            x.release()
        for x in (ref, c, v, c2, v2):
            be.free(x)


def test_colours_ride_along_like_the_reference(backend_f64, backend_f32, oracle, scan):
    """PointCloud::colors_ through the cloud operations (o3ds_cloud_set_colors & co.): kept by crop / select / carve, copied by
    transform, [O3D] operator+= rule on append, MEAN in VoxelDownSample, LAST point's colour in the map merge
    (helpers.cpp:40-42,61-63,83-85) -- each against the oracle; f64 storage exact, f32 storage to f32 rounding."""
    rng = np.random.default_rng(3)
    pts = scan[:20000]
    nrm = np.roll(pts, 1, axis=1)
    col = rng.uniform(0, 1, pts.shape)
    for be, tol in ((backend_f64, 0.0), (backend_f32, 1e-7)):
        def same(a, b):
            np.testing.assert_allclose(a, b, rtol=0, atol=tol)

        c = be.upload(pts, nrm)
        assert not be.has_colors(c) and be.get_colors(c) is None
        with pytest.raises(backend.BackendError) as ei:  # the raw entry point says EMPTY for an uncoloured cloud
            be._ck(be.lib.o3ds_cloud_get_colors(be.h, c, np.empty((len(pts), 3)).ctypes.data_as(backend._dp), len(pts)))
        assert ei.value.code == -6
        with pytest.raises(ValueError):
            be.set_colors(c, col[:5])
        be.set_colors(c, col)
        assert be.has_colors(c)
        same(be.get_colors(c), col)
        # crop, select: the colours of the kept points, in order
        crop = backend.make_crop(backend.CROP_MIN_MAX_RADIUS, center=(0.5, -0.25, 0.1), rmin=3.0, rmax=20.0)
        keep = oracle.crop_indices(pts, oracle.make_crop(oracle.CROP_MIN_MAX_RADIUS, center=(0.5, -0.25, 0.1), rmin=3.0, rmax=20.0))
        out = be.crop_cloud(c, crop)
        if tol == 0.0:
            np.testing.assert_array_equal(be.download(out)[0], pts[keep])
            same(be.get_colors(out), col[keep])
        else:  # f32-rounded points may change sides of a radius; the colours still belong to the points that were kept
            gp, gc = be.download(out)[0], be.get_colors(out)
            d, j = __import__("scipy.spatial", fromlist=["cKDTree"]).cKDTree(pts).query(gp)
            assert d.max() < 1e-5
            same(gc, col[j])
        idx = rng.choice(len(pts), 777, replace=False)
        sel = be.select_by_index(c, idx)
        same(be.get_colors(sel), col[idx])
        # transform: untouched
        T = syn.make_pose((1.0, 2.0, 0.5), (3.0, -2.0, 40.0))
        moved = be.transform_cloud(c, T)
        same(be.get_colors(moved), col)
        # VoxelDownSample: mean colour per voxel ([O3D] averages colours exactly like normals)
        v = be.voxel_down_sample(c, 0.4)
        ref_p, ref_c = oracle.voxel_down_sample(pts, 0.4, col)
        gp, gc = be.download(v)[0], be.get_colors(v)
        if tol == 0.0:
            j = _match(gp, ref_p, 1e-12)
            np.testing.assert_allclose(gc[j], ref_c, atol=1e-12)
        else:
            assert abs(len(gp) - len(ref_p)) <= 0.002 * len(ref_p) and gc.min() >= 0.0 and gc.max() <= 1.0
        assert be.size(v)[1] and be.has_colors(v)
        # append: colours survive only when both sides have them (or the map is empty)
        empty = be.upload(np.zeros((0, 3)))
        be.cloud_append(empty, sel)
        same(be.get_colors(empty), col[idx])
        be.cloud_append(empty, out)
        same(be.get_colors(empty)[:777], col[idx])
        assert len(be.get_colors(empty)) == 777 + be.size(out)[0]
        plain = be.upload(pts[:10], nrm[:10])
        be.cloud_append(empty, plain)
        assert not be.has_colors(empty) and be.size(empty) == (777 + be.size(out)[0] + 10, True)
        plain2 = be.upload(pts[:10], nrm[:10])
        be.cloud_append(plain2, sel)  # uncoloured map + coloured cloud: still uncoloured
        assert not be.has_colors(plain2)
        # map merge: pass-through points keep their colour, a voxel shows its LAST point's colour
        center = (3.0, -4.0, 0.0)
        m = be.upload(pts, nrm)
        be.set_colors(m, col)
        be.voxelize_within_volume(m, 0.5, backend.make_crop(backend.CROP_MAX_RADIUS, center=center, rmax=12.0))
        ocrop = oracle.make_crop(oracle.CROP_MAX_RADIUS, center=center, rmax=12.0)
        ref_p, _, npass = oracle.voxelize_within_volume(pts, nrm, 0.5, ocrop)
        ref_c = oracle.voxelize_within_volume_colors(pts, col, 0.5, ocrop)
        gp, gc = be.download(m)[0], be.get_colors(m)
        if tol == 0.0:
            assert len(gp) == len(ref_p) and 0 < npass < len(ref_p)
            np.testing.assert_array_equal(gc[:npass], ref_c[:npass])
            j = _match(gp[npass:], ref_p[npass:], 1e-12)
            np.testing.assert_array_equal(gc[npass:][j], ref_c[npass:])
        else:  # every colour of the merged map is one of the input colours (assigned, never blended)
            d, _ = __import__("scipy.spatial", fromlist=["cKDTree"]).cKDTree(col).query(gc)
            assert d.max() <= 2e-7
        # insertScan = transform + append + merge, colours included
        m2 = be.upload(np.zeros((0, 3)))
        be.map_insert_scan(m2, c, T, 0.5, backend.make_crop(backend.CROP_MAX_RADIUS, center=T[:3, 3], rmax=12.0))
        assert be.has_colors(m2)
        if tol == 0.0:
            tp = oracle.transform_points(pts, T)
            oc2 = oracle.make_crop(oracle.CROP_MAX_RADIUS, center=T[:3, 3], rmax=12.0)
            rp, _, np2 = oracle.voxelize_within_volume(tp, oracle.transform_normals(nrm, T), 0.5, oc2)
            rc = oracle.voxelize_within_volume_colors(tp, col, 0.5, oc2)
            gp2, gc2 = be.download(m2)[0], be.get_colors(m2)
            np.testing.assert_array_equal(gc2[:np2], rc[:np2])
            j = _match(gp2[np2:], rp[np2:], 1e-10)
            np.testing.assert_array_equal(gc2[np2:][j], rc[np2:])
        # clearing
        be.set_colors(c, None)
        assert not be.has_colors(c)
        for x in (c, out, sel, moved, v, empty, plain, plain2, m, m2):
            be.free(x)
    # dense voxel map: colour sums / count, like the normals (Voxel.cpp:24-26,33-35,84-87); uncoloured + coloured inserts set the flag;
    # a placed insert does not rotate colours; carving and a rehash keep them
    from scipy.spatial import cKDTree

    scene = syn.make_scene()
    clouds = [syn.sample_map(scene, n, seed=70 + k) for k, n in enumerate((20_000, 90_000))]  # the second insert forces a rehash
    cols = [rng.uniform(0, 255, c[0].shape) for c in clouds]                                 # intensity-byte colours reach 255
    dm = backend_f64.dense_map_create(0.2)
    for (p, n), cc in zip(clouds, cols):
        c = backend_f64.upload(p, n)
        backend_f64.set_colors(c, cc)
        backend_f64.dense_map_insert(dm, c)
        backend_f64.free(c)
    rp, rcol, _ = oracle.dense_fuse(np.vstack([c[0] for c in clouds]), np.vstack(cols), 0.2)
    out = backend_f64.dense_map_to_cloud(dm)
    gp, gcol = backend_f64.download(out)[0], backend_f64.get_colors(out)
    d, j = cKDTree(rp).query(gp)
    assert np.array_equal(np.sort(j), np.arange(len(rp))) and d.max() < 1e-8
    np.testing.assert_allclose(gcol, rcol[j], rtol=0, atol=1e-6)  # fixed-point colour sums: 2^-24 per inserted point
    assert backend_f64.size(out)[1]
    T = syn.make_pose((1.0, -2.0, 0.3), (5.0, -3.0, 60.0))
    dm2 = backend_f64.dense_map_create(0.2)
    c = backend_f64.upload(clouds[0][0], clouds[0][1])
    backend_f64.set_colors(c, cols[0])
    backend_f64.dense_map_insert(dm2, c, T)
    o2 = backend_f64.dense_map_to_cloud(dm2)
    rp2, rc2, _ = oracle.dense_fuse(oracle.transform_points(clouds[0][0], T), cols[0], 0.2)
    d, j = cKDTree(rp2).query(backend_f64.download(o2)[0])
    assert d.max() < 1e-8
    np.testing.assert_allclose(backend_f64.get_colors(o2), rc2[j], rtol=0, atol=1e-6)
    plain = backend_f64.dense_map_create(0.2)
    c2 = backend_f64.upload(clouds[0][0])
    backend_f64.dense_map_insert(plain, c2)
    o3 = backend_f64.dense_map_to_cloud(plain)
    assert not backend_f64.has_colors(o3) and not backend_f64.size(o3)[1]
    for x in (out, o2, o3, c, c2):
        backend_f64.free(x)
    for x in (dm, dm2, plain):
        backend_f64.dense_map_free(x)
    # carve keeps the colours of the survivors
    scene = syn.make_scene()
    mp, mn = syn.sample_map(scene, 30_000)
    ghost = rng.uniform([-3.0, -3.0, 0.2], [3.0, 3.0, 1.5], size=(400, 3))
    mp, mn = np.vstack([mp, ghost]), np.vstack([mn, rng.normal(size=(400, 3))])
    mc = rng.uniform(0, 1, mp.shape)
    pose = syn.make_pose((0.3, -0.2, 0.5), (1.0, -2.0, 10.0))
    raw = syn.vlp16_scan(scene, pose, n_az=512)
    m, s = backend_f64.upload(mp, mn), backend_f64.upload(raw)
    backend_f64.set_colors(m, mc)
    removed = backend_f64.map_carve(m, s, pose, backend.make_crop(backend.CROP_MAX_RADIUS, center=pose[:3, 3], rmax=15.0))
    gp, gc = backend_f64.download(m)[0], backend_f64.get_colors(m)
    assert removed > 0 and len(gc) == len(mp) - removed
    d, j = __import__("scipy.spatial", fromlist=["cKDTree"]).cKDTree(mp).query(gp)
    assert d.max() == 0.0
    np.testing.assert_array_equal(gc, mc[j])
    backend_f64.free(m)
    backend_f64.free(s)


def test_carried_bounding_boxes_never_lose_a_neighbour(backend_f64, backend_f32, oracle, scan):
    """Index builds take the bounding box that travels with a device cloud (set by VoxelDownSample / a previous index build, carried
    through crop, select, rigid placement and append) instead of reducing one.  A box that missed a point would put it in the wrong
    cell and the search would lose neighbours, so: build the chain voxel filter -> crop -> placement by a large rotation -> append ->
    select, and compare the exact 1-NN distances and the normals computed on the carried box with the oracle's on the downloaded
    points (f64 storage: to rounding; f32 storage: the placement rounds the stored values, which the box must absorb)."""
    from scipy.spatial import cKDTree

    T = syn.make_pose((40.0, -25.0, 3.0), (20.0, -35.0, 130.0))
    for be, tol in ((backend_f64, 1e-9), (backend_f32, 1e-4)):
        raw = be.upload(scan)
        vox = be.voxel_down_sample(raw, 0.2)                                   # sets the box
        inner = be.crop_cloud(vox, backend.make_crop(backend.CROP_MAX_RADIUS, rmax=25.0))  # subset: same box
        placed = be.transform_cloud(inner, T)                                  # box of the 8 placed corners
        other = be.transform_cloud(inner, syn.make_pose((-60.0, 10.0, -2.0), (0.0, 0.0, 45.0)))
        be.cloud_append(placed, other)                                         # union of two boxes
        n = be.size(placed)[0]
        keep = np.arange(0, n, 2, dtype=np.uint32)
        half = be.select_by_index(placed, keep)                                # subset again
        pts = be.download(half)[0]
        # (a) exact 1-NN of a shifted copy against the cloud indexed on its carried box
        q = pts[::7] + np.array([0.03, -0.02, 0.01])
        qc = be.upload(q)
        be.build_index(half, 0.5)
        be.estimate_normals(half, 1.0, 10)                                     # (drops and rebuilds the index: both on the carried box)
        r = be.icp_point_to_point_dev(qc, half, 0.5, max_iter=0)  # one correspondence pass: fitness and rmse of the exact 1-NN
        d_ref, _ = cKDTree(pts).query(q)
        assert r["fitness"] == 1.0
        np.testing.assert_allclose(r["inlier_rmse"], np.sqrt(np.mean(d_ref ** 2)), rtol=1e-6, atol=tol)
        # (b) normals of every point: the neighbour sets are the oracle's
        got = be.download(half)[1]
        ref = oracle.estimate_normals(pts, 1.0, 10)
        dots = np.abs(np.einsum("ij,ij->i", got, ref))
        assert (dots > 1 - 1e-6).mean() > 0.95, (dots > 1 - 1e-6).mean()
        for cid in (raw, vox, inner, placed, other, half, qc):
            be.free(cid)


def test_crop_voxel_down_sample_is_crop_then_voxel_bit_for_bit(backend_f64, backend_f32, scan):
    """o3ds_crop_voxel_down_sample = the first two steps of both preprocess chains (ScanToMapRegistration.cpp:36-37, Odometry.cpp:26-27)
    in one call: identical to o3ds_crop_cloud followed by o3ds_voxel_down_sample -- points, normals and colours, every volume kind,
    an empty result, and voxel <= 0 (crop only)."""
    rng = np.random.default_rng(3)
    nrm = rng.normal(size=scan.shape)
    col = rng.uniform(size=scan.shape)
    for be in (backend_f64, backend_f32):
        c = be.upload(scan, nrm)
        be.set_colors(c, col)
        for kind, kw, voxel in ((backend.CROP_MIN_MAX_RADIUS, dict(rmin=2.0, rmax=30.0), 0.1), (backend.CROP_MAX_RADIUS, dict(rmax=9.0), 0.25),
                                (backend.CROP_CYLINDER, dict(rmax=15.0, zmin=-1.0, zmax=3.0, invert=True), 0.1), (backend.CROP_NONE, dict(), 0.3),
                                (backend.CROP_MIN_RADIUS, dict(rmin=1e6), 0.1), (backend.CROP_MAX_RADIUS, dict(rmax=12.0), 0.0)):
            crop = backend.make_crop(kind, center=(0.5, -0.25, 0.1), **kw)
            a = be.crop_cloud(c, crop)
            two = be.voxel_down_sample(a, voxel) if be.size(a)[0] else be.upload(np.zeros((0, 3)))
            one = be.crop_voxel_down_sample(c, crop, voxel)
            assert be.size(one)[0] == be.size(two)[0], (kind, kw)
            if be.size(one)[0]:
                p1, n1 = be.download(one)
                p2, n2 = be.download(two)
                np.testing.assert_array_equal(p1, p2)
                np.testing.assert_array_equal(n1, n2)
                np.testing.assert_array_equal(be.get_colors(one), be.get_colors(two))
            for cid in (a, two, one):
                be.free(cid)
        be.free(c)


def _insert_sequence(be, n_frames, rmax, voxel, carve_at=(), look_at=None, scan_rmax=None, carve_voxel=0.1):
    """a short mapping run: scans along an out-and-back path (points leave the map builder's volume and come back), returns the map
    after every insertion (look_at: after these insertions only -- a map in its persistent form folds back into an array when somebody
    looks, so looking rarely is what exercises its history) as raw bytes; scan_rmax: the scans are cropped to this range first"""
    scene = syn.make_scene()
    m = be.upload(np.zeros((0, 3)))
    out = []
    for k in range(n_frames):
        t = k if k < n_frames // 2 else n_frames - 1 - k  # out and back
        T = syn.make_pose([1.5 * t, 0.4 * t, 0.0], [0.0, 0.0, 4.0 * t])
        raw = syn.vlp16_scan(scene, T, frame=k, n_az=256)
        s = be.upload(raw)
        if scan_rmax is None:
            v = be.voxel_down_sample(s, 0.1)
        else:
            v = be.crop_voxel_down_sample(s, backend.make_crop(backend.CROP_MAX_RADIUS, rmax=scan_rmax), 0.1)
        be.estimate_normals(v, 2.0, 10)
        crop = backend.make_crop(backend.CROP_MIN_MAX_RADIUS, center=T[:3, 3], rmin=0.0, rmax=rmax)
        if k in carve_at:
            be.map_carve(m, s, T, crop, voxel=carve_voxel)
        be.map_insert_scan(m, v, T, voxel, crop, max_corr_hint=1.0)
        if look_at is None or k in look_at:
            p, n = be.download(m)
            out.append((p.tobytes(), n.tobytes(), len(p)))
        be.free(s)
        be.free(v)
    be.free(m)
    return out


def _big_map_inserts(be):
    """a 3 M-point map (beyond 2^21 entries) and three scans inserted into it; checksum of the map after each insertion"""
    import hashlib

    scene = syn.make_scene()
    pts, nrm = syn.sample_map(scene, 3_000_000, seed=21)
    m = be.upload(pts, nrm)
    out = []
    for k in range(3):
        T = syn.make_pose([0.8 * k, -0.3 * k, 0.0], [0.0, 0.0, 3.0 * k])
        s = be.upload(syn.vlp16_scan(scene, T, frame=k, n_az=512))
        v = be.voxel_down_sample(s, 0.1)
        be.estimate_normals(v, 2.0, 10)
        crop = backend.make_crop(backend.CROP_MIN_MAX_RADIUS, center=T[:3, 3], rmin=0.0, rmax=18.0)
        be.map_insert_scan(m, v, T, 0.05, crop, max_corr_hint=1.0)
        p, n = be.download(m)
        out.append((len(p), hashlib.sha1(p.tobytes()).hexdigest(), hashlib.sha1(n.tobytes()).hexdigest()))
        be.free(s)
        be.free(v)
    be.free(m)
    return out


def test_map_merge_by_merging_beyond_two_million_points():
    """the merging path counts the three classes of entries with two 32-bit counters in one 64-bit scan (the third is the remainder), so it
    holds for maps of any size the 32-bit point indices allow; checked against the full sort on a 3 M-point map"""
    ref, _ = run_child(ME, "t._big_map_inserts(t.backend.Backend(0, ab=True))", env=dict(O3DS_NO_INCREMENTAL_MERGE="1"),
                       timeout=300)  # (a guard against a hang: the whole test took 2.0 s on an MI355X)
    be = backend.Backend(0)
    got = _big_map_inserts(be)
    be.close()
    assert got == ref and got[-1][0] > (1 << 21), (got, ref)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_map_merge_by_merging_is_bitwise_the_full_sort(prec, monkeypatch):
    """Submap::insertScan re-bins the whole map at every scan (helpers.cpp:115-183).  The backend builds the sorted voxel-key list of
    map + scan by MERGING the still-sorted voxel block of the previous insertion with the few keys that are new to the volume
    (voxel_reduce_t / merge_class_kernel) instead of sorting N + m keys; O3DS_NO_INCREMENTAL_MERGE=1 forces the sort.  Both must give
    the same map byte for byte after every one of 14 insertions along an out-and-back path with a small builder volume (points leave
    the volume, become pass-through, and re-enter on the way back), with a carve in between (which resets the layout)."""
    p = backend.PRECISION_F64 if prec == "f64" else backend.PRECISION_F32
    # the switch is read once per process: the reference run goes to a child process
    ref, _ = run_child(ME, f"t._insert_sequence(t.backend.Backend(0, {p}, ab=True), 14, 12.0, 0.2, carve_at=(9,))",
                       env=dict(O3DS_NO_INCREMENTAL_MERGE="1", O3DS_NO_PERSISTENT_MAP="1"),
                       timeout=300)  # (a guard against a hang: the whole test took 0.8 s on an MI355X)
    be = backend.Backend(0, p)
    got = _insert_sequence(be, 14, 12.0, 0.2, carve_at=(9,))
    be.close()
    assert [g[2] for g in got] == [r[2] for r in ref]
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == r[0] and g[1] == r[1], k
    assert got[-1][2] > 5000


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("case", ["look_rarely", "scan_inside_volume", "never_until_the_end", "carved_in_place"])
def test_persistent_map_is_bitwise_the_array_form(prec, case):
    """Submap::insertScan in time independent of the map's size (map_kernels.hpp): from its second insertion on a map lives in slot
    arrays + a voxel hash + a row-paged search index, an insertion touches only the voxels the scan falls into, and the reference's array
    [pass-through points in original order | voxel means in key order] is only formed when somebody looks.  It must be the SAME array,
    byte for byte, as re-binning the whole map at every insertion gives (O3DS_NO_PERSISTENT_MAP=1 in a child process, the path the golden
    and oracle tests hold to the reference): 24 insertions along an out-and-back path with a small builder volume -- points leave the
    volume, pass through for a while and re-enter, scan points beyond the volume join the map unmerged, means round across voxel faces,
    several old points of one voxel merge when the volume comes back over them -- looked at rarely (long histories) or only at the end,
    with a carve in between (which folds the map), and a registration against the persistent map's index after every insertion."""
    p = backend.PRECISION_F64 if prec == "f64" else backend.PRECISION_F32
    kw = {"look_rarely": dict(look_at=(3, 4, 11, 17, 23), carve_at=(14,)), "scan_inside_volume": dict(look_at=(7, 15, 23), scan_rmax=11.5),
          "never_until_the_end": dict(look_at=(23,)),
          # the carving voxel is the map's voxel: the persistent map is carved where it is (its voxel hash is the reference's table), twice
          "carved_in_place": dict(look_at=(5, 12, 23), carve_at=(8, 16), carve_voxel=0.2)}[case]
    ref, _ = run_child(ME, f"t._insert_sequence(t.backend.Backend(0, {p}, ab=True), 24, 12.0, 0.2, **{kw!r})", env=dict(O3DS_NO_PERSISTENT_MAP="1"),
                       timeout=300)  # (a guard against a hang: the whole test took 0.6 to 0.9 s per case on an MI355X)
    be = backend.Backend(0, p)
    got = _insert_sequence(be, 24, 12.0, 0.2, **kw)
    be.close()
    assert [g[2] for g in got] == [r[2] for r in ref]
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == r[0] and g[1] == r[1], k
    assert got[-1][2] > 5000


def _face_points(prec, seed):
    """500 points ON voxel faces, with unit normals: 250 lattice points k * 0.1 (k integer in [-12, 12] per axis), computed in double and
    rounded to the storage type, and the same points shifted by half a 0.1 voxel.  The world-anchored keys have the lattice points on
    their faces, the data-anchored key of VoxelDownSample (origin = min bound - voxel / 2) the shifted ones."""
    rng = np.random.default_rng(seed)
    lat = rng.integers(-12, 13, size=(250, 3)) * 0.1
    pts = np.vstack([lat, lat + 0.05])
    nrm = rng.normal(size=pts.shape)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    if prec == "f32":
        pts, nrm = pts.astype(np.float32).astype(np.float64), nrm.astype(np.float32).astype(np.float64)
    return pts, nrm


_FACE_CARVE = dict(max_length=20.0, truncation=0.1, min_dot=0.5)


def _face_carve_scan(prec):
    """rays from the origin (the sensor of an identity pose) to face points: along the axes their samples lie on faces too"""
    b, _ = _face_points(prec, 2)
    return b[np.linalg.norm(b, axis=1) > 0.0][:150]


def _face_map_sequence(be, prec, voxel, look):
    """two insertions of face points into an empty map at the identity pose (no rounding in the placement), then a carve with the
    map's voxel.  look: download the map between the insertions and the carve -- that folds a map in its persistent form into the
    array, so the carve works on the array; without it a persistent map is carved where it is."""
    crop = backend.make_crop(backend.CROP_MIN_MAX_RADIUS, rmin=0.0, rmax=1.5)
    m = be.upload(np.zeros((0, 3)))
    for seed in (1, 2):
        s = be.upload(*_face_points(prec, seed))
        be.map_insert_scan(m, s, np.eye(4), voxel, crop, max_corr_hint=1.0)
        be.free(s)
    out = {}
    if look:
        out["inserted"] = be.download(m)
    raw = be.upload(_face_carve_scan(prec))
    out["removed"] = be.map_carve(m, raw, np.eye(4), crop, voxel=voxel, **_FACE_CARVE)
    out["carved"] = be.download(m)
    be.free(raw)
    be.free(m)
    return out


def _face_map_sequences(be, prec):
    return {(voxel, look): _face_map_sequence(be, prec, voxel, look) for voxel in (0.1, 0.25) for look in (True, False)}


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_points_on_voxel_faces_fall_where_the_oracle_puts_them(backend_f64, backend_f32, oracle, prec):
    """The voxel of a point is rounded in four ways (cloud_kernels.hpp key_from_origin, key_world, key_world_int, key_by_division), each
    after another line of the reference, and they disagree only on points that lie on voxel faces -- which the scans of the other tests
    almost never hit.  Here every point lies on a face of one of the grids, and every operation that bins points is held to the oracle:
    bit for bit in f64 storage (identity poses: the placement rounds nothing; tests/test_placed_binning_gpu.py does the same under a
    general pose).  In f32 storage every decision -- what a carve removes, which points overlap, which voxels exist -- is held exactly as
    well, the oracle working on the f32-rounded values the device holds; only voxel means stored in f32 keep the neighbouring tests' bounds."""
    from scipy.spatial import cKDTree

    be = backend_f64 if prec == "f64" else backend_f32
    f64 = prec == "f64"
    a, an = _face_points(prec, 1)
    b, bn = _face_points(prec, 2)
    # the input tells the roundings apart: the oracle's VoxelDownSample and its dense map bin these points differently, and (binary64
    # lattice values only: rounded to f32 they sit 1e-9 off the faces) multiplying by 1 / v and dividing by v disagree on some
    assert len(oracle.voxel_down_sample(a, 0.1)) != len(oracle.dense_fuse(a, None, 0.1)[0])
    if f64:
        assert np.any(np.floor(a * (1.0 / 0.1)) != np.floor(a / 0.1))
    ca, cb = be.upload(a, an), be.upload(b, bn)
    crop_kw = dict(center=(0.03, -0.02, 0.01), rmax=1.3)
    keep = oracle.crop_indices(a, oracle.make_crop(oracle.CROP_MAX_RADIUS, **crop_kw))
    assert 0 < len(keep) < len(a)

    def same_cloud(cid, ref, rn):
        got, gn = be.download(cid)
        if f64:
            np.testing.assert_array_equal(got, ref)
            np.testing.assert_array_equal(gn, rn)
        else:  # (test_voxel_down_sample_with_normals_and_f32)
            j = _match(got, ref, 5e-6)
            np.testing.assert_allclose(gn[j], rn, atol=1e-6)
        be.free(cid)

    # the array form of the map sequences: the A/B library in a child process (the switch is read once per process)
    array_form, _ = run_child(ME, f"t._face_map_sequences(t.backend.Backend(0, {backend.PRECISION_F64 if f64 else backend.PRECISION_F32}, ab=True), {prec!r})",
                              env=dict(O3DS_NO_PERSISTENT_MAP="1"), timeout=300)  # (a guard against a hang: the whole test took 0.6 s on an MI355X)
    persistent = _face_map_sequences(be, prec)
    ocrop = oracle.make_crop(oracle.CROP_MIN_MAX_RADIUS, rmin=0.0, rmax=1.5)
    raw = _face_carve_scan(prec)

    for voxel in (0.1, 0.25):
        same_cloud(be.voxel_down_sample(ca, voxel), *oracle.voxel_down_sample(a, voxel, an))
        same_cloud(be.crop_voxel_down_sample(ca, backend.make_crop(backend.CROP_MAX_RADIUS, **crop_kw), voxel),
                   *oracle.voxel_down_sample(a[keep], voxel, an[keep]))

        # map_insert_scan twice, map_carve: the three routes agree byte for byte ...
        looked, unlooked, arr = persistent[(voxel, True)], persistent[(voxel, False)], array_form[(voxel, True)]
        for other in (unlooked, arr, array_form[(voxel, False)]):
            assert other["removed"] == looked["removed"]
            for name in ("carved", "inserted") if "inserted" in other else ("carved",):
                for x, y in zip(other[name], looked[name]):
                    assert x.tobytes() == y.tobytes()
        # ... and with the oracle (test_voxelize_within_volume_matches_oracle, test_map_carve_matches_oracle)
        ref_p, ref_n, _ = oracle.voxelize_within_volume(a, an, voxel, ocrop)
        ref_p, ref_n, npass = oracle.voxelize_within_volume(np.vstack([ref_p, b]), np.vstack([ref_n, bn]), voxel, ocrop)
        mp, mn = looked["inserted"]
        assert len(mp) == len(ref_p) and 0 < npass < len(ref_p)
        if f64:
            np.testing.assert_array_equal(mp[:npass], ref_p[:npass])
            j = _match(mp[npass:], ref_p[npass:], 0.0)
            np.testing.assert_array_equal(mp[npass:][j], ref_p[npass:])
            np.testing.assert_allclose(mn[npass:][j], ref_n[npass:], atol=1e-9)  # (test_map_insert_scan_sequence_matches_oracle)
        else:
            j = _match(mp, ref_p, 5e-6)
            np.testing.assert_allclose(mn[j], ref_n, atol=1e-6)
        gone = oracle.carve_flags(raw, np.zeros(3), mp, mn, oracle.crop_indices(mp, ocrop), voxel=voxel, **_FACE_CARVE)
        assert 0 < int(gone.sum()) < len(mp)
        # (the oracle works on what the device holds -- the downloaded map and the scan rounded to the storage type --, in both storages)
        assert looked["removed"] == int(gone.sum())
        np.testing.assert_array_equal(looked["carved"][0], mp[~gone])
        np.testing.assert_array_equal(looked["carved"][1], mn[~gone])

        # dense map: insert, count, carve (test_dense_voxel_map_matches_oracle, test_dense_map_carve_matches_oracle)
        dm = be.dense_map_create(voxel)
        be.dense_map_insert(dm, ca)
        rp, _, _ = oracle.dense_fuse(a, None, voxel)
        key_of = lambda pts: np.array([oracle.lib().orc_voxel_key(np.ascontiguousarray(q).ctypes.data_as(oracle._dp), voxel) for q in pts], np.int64)
        occupied = set(key_of(a).tolist())
        assert sorted(key_of(rp).tolist()) == sorted(occupied)  # (the oracle's means are fit to stand for their voxels in dense_carve)
        assert be.dense_map_size(dm) == len(rp)
        assert be.dense_map_count_occupied(dm, cb) == sum(k in occupied for k in key_of(b).tolist())
        before_id = be.dense_map_to_cloud(dm)
        before = be.download(before_id)[0]
        # fixed-point sums: 1 nm per inserted point; f32 storage of the means: half a spacing of 1.2e-7 per axis at these magnitudes
        d, j = cKDTree(rp).query(before)
        assert np.array_equal(np.sort(j), np.arange(len(rp))) and d.max() < (1e-8 if f64 else 1e-6)
        ref = oracle.dense_carve(raw, np.zeros(3), rp, voxel)[j]
        s = be.upload(raw)
        removed = be.dense_map_carve(dm, s, np.zeros(3))
        assert removed == int(ref.sum()) and 0 < removed < len(before)
        after_id = be.dense_map_to_cloud(dm)
        np.testing.assert_array_equal(be.download(after_id)[0], before[~ref])
        for cid in (before_id, after_id, s):
            be.free(cid)
        be.dense_map_free(dm)

        # overlap_indices at the identity (test_overlap_indices_match_oracle)
        g_s, g_t = be.overlap_indices(ca, cb, np.eye(4), voxel, 1)
        r_s, r_t = oracle.overlap_indices(a, b, np.eye(4), voxel, 1)
        assert 0 < len(r_s) < len(a)
        np.testing.assert_array_equal(g_s, r_s)  # (a and b are rounded to the storage type already: both storages bin the same values)
        np.testing.assert_array_equal(g_t, r_t)
    be.free(ca)
    be.free(cb)


@pytest.fixture(scope="module")
def scratch_clouds():
    """seeded samples of the synthetic scene (a 60 m x 60 m x 10 m hall), with normals, by size"""
    scene = syn.make_scene()
    return {n: syn.sample_map(scene, n, seed=100 + k) for k, n in enumerate((400, 3_000, 40_000, 1_100_000))}


def _scratch_history(be, clouds, sizes, reverse):
    """every operation that uses a scratch block the handle owns and grows (the voxel table, the chained scan's tiles, the per-cell
    counters), on one handle; `reverse`: the inputs of each kind in descending instead of ascending size.  Returns what each
    (operation, input) left, as bytes."""
    out = {}
    ids = {n: be.upload(*clouds[n]) for n in sizes}

    def look(key, cid):
        p, n = be.download(cid)
        out[key] = (p.tobytes(), n.tobytes())
        be.free(cid)

    def insert(m, k, hint):  # (the insertions of a map keep their order on both handles: a map is what its history made it)
        T = (np.eye(4), syn.make_pose([1.5, 0.4, 0.0], [0.0, 0.0, 4.0]), syn.make_pose([3.0, 0.8, 0.0], [0.0, 0.0, 8.0]))[k]
        crop = backend.make_crop(backend.CROP_MIN_MAX_RADIUS, center=T[:3, 3], rmin=0.0, rmax=12.0)
        be.map_insert_scan(m, ids[(40_000, 3_000, 40_000)[k]], T, 0.2, crop, max_corr_hint=hint)
        assert be.is_persistent_map(m) == (k >= 1)  # the second insertion enters the persistent form

    # the voxel table (1 024, 8 192, 131 072 slots: the next power of two >= 2 n; 2 m voxels: 2 499 of the 40 000 points) and the tiles
    # (1 100 000 points: 1 075 tiles, beyond the 1 024 of the first allocation); between them three insertions into one map, whose
    # persistent form shares both blocks and, entering, counts into the cell counters (hint 4 m: cells of 1 m, 7e4 of them)
    vol = backend.make_crop(backend.CROP_MAX_RADIUS, rmax=20.0)
    m = be.upload(np.zeros((0, 3)))
    for k, n in enumerate(sizes[::-1] if reverse else sizes):
        look(("voxel_down_sample", n), be.voxel_down_sample(ids[n], 2.0))
        look(("crop_voxel_down_sample", n), be.crop_voxel_down_sample(ids[n], vol, 2.0))
        if k < 3:
            insert(m, k, 4.0)
    look(("map",), m)
    # the cell counters: an index with cells of 2 m (4 500), then of 0.5 m (2.9e5: the block grows); registrations against each until it
    # has its replica (the fourth), whose counter table (nx (ny + 2) (nz + 2)) is larger than the index's
    T0 = syn.make_pose([0.05, -0.03, 0.02], [0.2, -0.1, 0.3])
    for cell in ((0.5, 2.0) if reverse else (2.0, 0.5)):
        be.build_index(ids[40_000], 1.0, cell_size=cell)
        for k in range(6):
            r = be.icp_point_to_plane_dev(ids[3_000], ids[40_000], 1.0, init=T0, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
            assert r["n_corr"] > 1000
            out[("register", cell, k)] = (r["transformation"].tobytes(), r["n_corr"])
            if be.index_replica(ids[40_000]) > 0:
                break
        assert be.index_replica(ids[40_000]) > 0
    # ... and their third user, the row table of a map entering the persistent form (hint 1 m: cells of 0.2 m, 8.6e6 of them)
    m = be.upload(np.zeros((0, 3)))
    insert(m, 0, 1.0)
    insert(m, 1, 1.0)
    look(("fresh map",), m)
    return out


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_shared_scratch_blocks_do_not_remember_their_history(prec, scratch_clouds):
    """The voxel table, the tile records and the cell counters belong to the handle, are shared by VoxelDownSample, the persistent map,
    the index build, the replica build and the row table, grow on demand and are left clean by their users instead of being cleared.
    Two handles run the same operations on the same clouds, one with the inputs of each kind in ascending size (every block grows
    step by step, every user meets what a smaller one left), one in descending size (every block is allocated once at its largest):
    the same kernels on the same data, so every result -- points and normals, the 16 pose doubles and n_corr -- is the same bytes.
    What is not reversed: the insertions into a map (a map is its history) and the order of the kinds.  The 1 100 000-point cloud, the
    smallest that outgrows the tile array's first allocation, runs with f32 storage only."""
    p = backend.PRECISION_F64 if prec == "f64" else backend.PRECISION_F32
    sizes = (400, 3_000, 40_000) + ((1_100_000,) if prec == "f32" else ())
    got = []
    for reverse in (False, True):
        be = backend.Backend(0, p)
        try:
            got.append(_scratch_history(be, scratch_clouds, sizes, reverse))
        finally:
            be.close()
    assert got[0].keys() == got[1].keys() and len(got[0]) >= 2 * len(sizes) + 2 + 8
    for key in got[0]:
        assert got[0][key] == got[1][key], key
    assert len(got[0][("map",)][0]) > 24 * 40_000  # (most points lie outside the 12 m volumes and pass through unmerged)


def test_normals_with_exact_ties_duplicates_and_tiny_clouds(backend_f64, oracle):
    """The neighbour order (d2, original index) decides everything where distances tie EXACTLY: a regular lattice (every point has
    whole shells of equidistant neighbours, so the max_nn-th place is always tied), duplicated points (d2 = 0 several times), and
    clouds smaller than max_nn / smaller than three points.  f64 storage must still equal the oracle bit for bit."""
    g = np.stack(np.meshgrid(np.arange(12) * 0.25, np.arange(12) * 0.25, np.arange(3) * 0.25, indexing="ij"), -1).reshape(-1, 3) + [3.0, -2.0, 1.0]
    rng = np.random.default_rng(3)
    dup = np.vstack([g, g[rng.choice(len(g), 40, replace=False)], g[:5], g[:5]])  # exact duplicates, some of them three times
    shuffled = dup[rng.permutation(len(dup))]
    for pts, cases in ((g, ((0.6, 7), (1.0, 20), (0.3, 30))), (shuffled, ((0.6, 7), (0.26, 5), (2.0, 40))),
                       (g[:2], ((1.0, 20),)), (g[:1], ((1.0, 5),)), (g[:7], ((5.0, 20),))):
        c = backend_f64.upload(pts)
        for radius, knn in cases:
            backend_f64.estimate_normals(c, radius, knn)
            _, got = backend_f64.download(c)
            ref = oracle.estimate_normals(pts, radius, knn)
            differ = np.flatnonzero(np.any(got != ref, axis=1))
            assert len(differ) == 0, (len(pts), radius, knn, len(differ), differ[:5], got[differ[:3]], ref[differ[:3]])
        backend_f64.free(c)


def _normals_digest_of_eight_scans():
    """(child side) eight scans of varying size down-sampled, their normals estimated and downloaded, everything freed: the digest"""
    import hashlib

    be = backend.Backend(0)
    scene = syn.make_scene()
    h = hashlib.sha1()
    for k in range(8):
        c = be.voxel_down_sample(be.upload(syn.vlp16_scan(scene, syn.make_pose([0.3 * k, 0, 0], [0, 0, 2.0 * k]), frame=k, n_az=256 + 64 * (k % 3))), 0.1)
        be.estimate_normals(c, 2.0, 10)
        h.update(be.download(c)[1].tobytes())
        be.free(c)
    return h.hexdigest()


def test_allocator_cache_is_bounded_and_survives_a_trim():
    """The handle's caching allocator gives everything cached back to the driver beyond O3DS_POOL_CAP_MB (size classes drift as a map
    grows); a tiny cap forces that path on every few calls -- results must not change."""
    outs = [run_child(ME, "t._normals_digest_of_eight_scans()", env=dict(O3DS_POOL_CAP_MB=cap),
                      timeout=300)[0]  # (a guard against a hang: the whole test, both children, took 0.8 s on an MI355X)
            for cap in ("32768", "1")]
    assert outs[0] == outs[1] and len(outs[0]) == 40


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_normals_estimated_after_the_merge_get_the_map_s_spare_room(prec):
    """A map that was merged WITHOUT normals keeps room behind its points (the next scan is placed there); normals estimated afterwards
    must get the same room, or the in-place append of o3ds_map_insert_scan writes past their end (the initial-map flow --
    voxelize, prepareInitialMap's estimateNormals, then a scan with normals).  Checked against the same steps on host copies."""
    p = backend.PRECISION_F64 if prec == "f64" else backend.PRECISION_F32
    be = backend.Backend(0, p)
    scene = syn.make_scene()
    pts, _ = syn.sample_map(scene, 60_000)
    m = be.upload(pts)
    crop = backend.make_crop(backend.CROP_MAX_RADIUS, rmax=25.0)
    be.voxelize_within_volume(m, 0.2, crop)
    be.estimate_normals(m, 2.0, 10)
    n0 = be.size(m)[0]
    p0, nn0 = be.download(m)
    for k in range(3):  # (also past the point where the map takes its persistent form)
        T = syn.make_pose([0.3 * k, 0.0, 0.0], [0.0, 0.0, 2.0 * k])
        s = be.upload(syn.vlp16_scan(scene, T, frame=k, n_az=256))
        v = be.voxel_down_sample(s, 0.1)
        be.estimate_normals(v, 2.0, 10)
        be.map_insert_scan(m, v, T, 0.2, backend.make_crop(backend.CROP_MAX_RADIUS, center=T[:3, 3], rmax=25.0), max_corr_hint=1.0)
        be.free(s)
        be.free(v)
    got_p, got_n = be.download(m)
    assert len(got_p) >= n0 and np.isfinite(got_p).all() and got_n is not None and len(got_n) == len(got_p)
    ln = np.linalg.norm(got_n, axis=1)
    assert np.all((np.abs(ln - 1.0) < 1e-5) | (ln == 0.0))  # every normal is a unit vector (or the zero vector of a degenerate voxel): no garbage
    # a second handle that repeats the steps gives the same bytes (nothing was written out of bounds into something else's memory)
    be2 = backend.Backend(0, p)
    m2 = be2.upload(p0, nn0)
    for k in range(3):
        T = syn.make_pose([0.3 * k, 0.0, 0.0], [0.0, 0.0, 2.0 * k])
        s = be2.upload(syn.vlp16_scan(scene, T, frame=k, n_az=256))
        v = be2.voxel_down_sample(s, 0.1)
        be2.estimate_normals(v, 2.0, 10)
        be2.map_insert_scan(m2, v, T, 0.2, backend.make_crop(backend.CROP_MAX_RADIUS, center=T[:3, 3], rmax=25.0), max_corr_hint=1.0)
    q_p, q_n = be2.download(m2)
    np.testing.assert_array_equal(q_p, got_p)
    np.testing.assert_array_equal(q_n, got_n)
    be.close()
    be2.close()


def test_a_persistent_map_keeps_its_record_when_every_record_is_wanted():
    """A handle has 64 pinned records for counts the host has not seen (lazily sized clouds, ingest boxes) and a persistent map holds one
    for its counters; when more than 64 sizes are in flight the oldest holder among the CLOUDS is settled -- never the map (its record
    used to be taken: the map's next look at its counters then read a scan's bounding box).  Seventy unasked VoxelDownSample results
    beside a map in its persistent form: the map must end as it does without them."""
    scene = syn.make_scene()

    def run(pressure):
        be = backend.Backend(0)
        m = be.upload(np.zeros((0, 3)))
        held = []
        for k in range(6):
            T = syn.make_pose([1.2 * k, 0.3 * k, 0.0], [0.0, 0.0, 3.0 * k])
            s = be.upload(syn.vlp16_scan(scene, T, frame=k, n_az=256))
            v = be.voxel_down_sample(s, 0.1)
            be.estimate_normals(v, 2.0, 10)
            crop = backend.make_crop(backend.CROP_MIN_MAX_RADIUS, center=T[:3, 3], rmin=0.0, rmax=12.0)
            be.map_insert_scan(m, v, T, 0.2, crop, max_corr_hint=1.0)
            if pressure and k == 3:  # the map is in its persistent form by now
                small = be.upload(syn.vlp16_scan(scene, T, frame=100, n_az=64))
                held = [be.voxel_down_sample(small, 0.1 + 0.01 * j) for j in range(70)]  # sizes nobody asks for
                be.free(small)
            be.free(s)
            be.free(v)
        p, n = be.download(m)
        sizes = [be.size(c)[0] for c in held]
        for c in held:
            be.free(c)
        be.free(m)
        be.close()
        return p.tobytes(), n.tobytes(), sizes

    p0, n0, _ = run(False)
    p1, n1, sizes = run(True)
    assert p0 == p1 and n0 == n1
    assert len(sizes) == 70 and all(0 < x < 5000 for x in sizes) and sizes[0] >= sizes[-1]


def test_a_view_carries_a_cloud_to_another_handle_while_its_owner_is_busy(scan):
    """o3ds_cloud_export_view / o3ds_cloud_import_view: the copy a second worker's handle makes of a pre-processed scan needs nothing of the
    owner's handle -- it is made here from another THREAD while the owner's thread is inside a registration on the owner's handle (what
    open3d_slam's mapping worker does while the odometry worker registers, SlamWrapper.cpp:227-236).  Points, normals and the box arrive
    bit for bit; the copy is an ordinary cloud of its handle; an empty cloud; a released view is a view of nothing."""
    import threading

    from open3d_slam_amd import backend

    owner, other = backend.Backend(0), backend.Backend(0)
    try:
        raw = owner.upload(scan)
        pre = owner.crop_voxel_down_sample(raw, backend.make_crop(backend.CROP_MIN_MAX_RADIUS, rmin=2.0, rmax=30.0), 0.1)
        owner.estimate_normals(pre, 3.0, 20)
        view = owner.export_view(pre)
        want_p, want_n = owner.download(pre)
        assert view.n == len(want_p) and view.event
        got = {}

        def importer():  # the other worker: its own handle, its own thread
            for k in range(8):
                cid = other.import_view(view)
                got[k] = other.download(cid)
                other.free(cid)

        t = threading.Thread(target=importer)
        t.start()
        for _ in range(6):  # the owner is busy on its handle meanwhile
            owner.icp_point_to_plane_dev(pre, pre, 1.0, max_iter=5, rel_fitness=0.0, rel_rmse=0.0)
        t.join()
        assert len(got) == 8
        for p, n in got.values():
            np.testing.assert_array_equal(p, want_p)
            np.testing.assert_array_equal(n, want_n)
        # the copy is a cloud like any other on its handle: it registers against itself at identity
        cid = other.import_view(view)
        r = other.icp_point_to_plane_dev(cid, cid, 1.0, max_iter=2)
        assert r["fitness"] == 1.0 and np.allclose(r["transformation"], np.eye(4), atol=1e-12)
        other.release_view(view)  # (a released view is a view of nothing)
        assert view.n == 0 and not view.event and other.size(other.import_view(view))[0] == 0
        empty = owner.upload(np.zeros((0, 3)))
        v0 = owner.export_view(empty)
        e2 = other.import_view(v0)
        assert other.size(e2)[0] == 0
        owner.release_view(v0)
    finally:
        owner.close()
        other.close()
