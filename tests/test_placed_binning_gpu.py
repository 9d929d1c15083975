"""Every operation that places a cloud with a pose and then bins it into voxels, held to the oracle element by element under a general
pose, in both storages (needs an MI355X).  The inputs (tests/placed_binning_cases.py) are aimed at voxel faces, so that a placement
which fuses a multiply-add, sums a row in another order or rounds once changes the oracle's own results (proved on the CPU by
tests/test_placed_binning_cpu.py).  The oracle always receives what the device holds: the inputs rounded to the storage type, and, where
the device rounds the placed cloud back to storage (transform_cloud, overlap_indices, dense_map_carve, map_insert_scan), the placed cloud
rounded likewise, at the identity pose.  Comparisons are equalities; the only tolerances left are those of the dense map's fixed-point
means and of voxel means rounded to f32, which are not properties of the placement."""
import numpy as np
import pytest

import placed_binning_cases as pb
from open3d_slam_amd import backend

pytestmark = pytest.mark.gpu

PRECS = ["f64", "f32"]
EYE = np.eye(4)


@pytest.fixture
def be(prec, backend_f64, backend_f32):
    """the session's handle of the storage the test is parametrised with"""
    return backend_f64 if prec == "f64" else backend_f32


_both = pytest.mark.parametrize("prec", PRECS)


def _match(got, ref, tol):
    """got[j[i]] <-> ref[i]: a bijection within tol between two clouds that hold the same voxels in different orders"""
    from scipy.spatial import cKDTree

    assert len(got) == len(ref)
    d, j = cKDTree(got).query(ref, k=1)
    assert d.max() <= tol, d.max()
    assert len(np.unique(j)) == len(ref)
    return j


@_both
@pytest.mark.parametrize("voxel", pb.VOXELS)
def test_transform_cloud_is_the_placement_bit_for_bit(be, prec, voxel):
    p, n = (pb.storage(x, prec) for x in pb.face_aimed(voxel)[:2])
    c = be.upload(p, n)
    t = be.transform_cloud(c, pb.POSE)
    xyz, nrm = be.download(t)
    np.testing.assert_array_equal(xyz, pb.storage(pb.place(pb.POSE, p), prec))
    np.testing.assert_array_equal(nrm, pb.storage(pb.rotate(pb.POSE, n), prec))
    be.free(c)
    be.free(t)


@_both
@pytest.mark.parametrize("voxel", pb.VOXELS)
def test_overlap_indices_are_the_oracles(be, prec, oracle, voxel):
    p, t = pb.storage(pb.face_aimed(voxel)[0], prec), pb.storage(pb.overlap_target(voxel), prec)
    placed = pb.storage(pb.place(pb.POSE, p), prec)  # the device rounds the placed source to its storage before it bins it
    s_id, t_id = be.upload(p), be.upload(t)
    for min_points in (1, 3):
        r_s, r_t = oracle.overlap_indices(placed, t, EYE, voxel, min_points)
        g_s, g_t = be.overlap_indices(s_id, t_id, pb.POSE, voxel, min_points)
        assert 0 < len(r_s) < len(p) and 0 < len(r_t) < len(t)
        np.testing.assert_array_equal(g_s, r_s)  # (the oracle's are ascending: np.flatnonzero)
        np.testing.assert_array_equal(g_t, r_t)
    be.free(s_id)
    be.free(t_id)


def _carve_crops(oracle):
    s = pb.CARVE_POSE[:3, 3]
    return (backend.make_crop(backend.CROP_MAX_RADIUS, center=s, rmax=pb.CARVE_RMAX),
            oracle.make_crop(oracle.CROP_MAX_RADIUS, center=s, rmax=pb.CARVE_RMAX))


@_both
@pytest.mark.parametrize("voxel", pb.VOXELS)
def test_map_carve_removes_the_oracles_points(be, prec, oracle, voxel):
    """an uploaded map (the array form), with and without normals, default and non-default parameters: the count, the survivors and the
    removed points in map order"""
    mp, mn, scan = (pb.storage(x, prec) for x in pb.carve_scene())
    s = pb.CARVE_POSE[:3, 3]
    crop, ocrop = _carve_crops(oracle)
    subset = oracle.crop_indices(mp, ocrop)
    placed = pb.place(pb.CARVE_POSE, scan)  # (the rays are cast from the placed doubles: nothing is rounded to storage in between)
    sc = be.upload(scan)
    for nrm in (mn, None):
        for kw in pb.CARVE_PARAMS:
            ref = oracle.carve_flags(placed, s, mp, nrm, subset, voxel=voxel, **kw)
            assert 0 < ref.sum() < len(subset) < len(mp)
            m = be.upload(mp, nrm)
            removed = be.map_carve(m, sc, pb.CARVE_POSE, crop, voxel=voxel, **kw)
            got_p, got_n = be.download(m)
            assert removed == int(ref.sum())
            np.testing.assert_array_equal(got_p, mp[~ref])
            m2 = be.upload(mp, nrm)
            removed2, gone = be.map_carve_removed(m2, sc, pb.CARVE_POSE, crop, voxel=voxel, **kw)
            gone_p, gone_n = be.download(gone)
            left_p, left_n = be.download(m2)
            assert removed2 == int(ref.sum())
            np.testing.assert_array_equal(gone_p, mp[ref])
            np.testing.assert_array_equal(left_p, mp[~ref])
            if nrm is not None:
                np.testing.assert_array_equal(got_n, nrm[~ref])
                np.testing.assert_array_equal(gone_n, nrm[ref])
                np.testing.assert_array_equal(left_n, nrm[~ref])
            for x in (m, m2, gone):
                be.free(x)
    be.free(sc)


def _inserted_map(be, prec, voxel, oracle=None):
    """two insertions with POSE into an empty map; with `oracle`, the oracle's map of the same insertions beside it: what it holds after
    each insertion rounded to the storage type, as the device's map is"""
    crop = backend.make_crop(backend.CROP_MAX_RADIUS, center=pb.POSE[:3, 3], rmax=pb.INSERT_RMAX)
    m = be.upload(np.zeros((0, 3)))
    ref = None
    if oracle is not None:
        ocrop = oracle.make_crop(oracle.CROP_MAX_RADIUS, center=pb.POSE[:3, 3], rmax=pb.INSERT_RMAX)
        ref = (np.zeros((0, 3)), np.zeros((0, 3)), 0)
    for k, (sp, sn) in enumerate(pb.insert_scans(voxel)):
        sp, sn = pb.storage(sp, prec), pb.storage(sn, prec)
        s = be.upload(sp, sn)
        be.map_insert_scan(m, s, pb.POSE, voxel, crop, max_corr_hint=1.0)
        be.free(s)
        assert be.is_persistent_map(m) == (k >= 1)  # the second insertion enters the persistent form
        if oracle is not None:
            tp, tn = pb.storage(pb.place(pb.POSE, sp), prec), pb.storage(pb.rotate(pb.POSE, sn), prec)
            rp, rn, npass = oracle.voxelize_within_volume(np.vstack([ref[0], tp]), np.vstack([ref[1], tn]), voxel, ocrop)
            ref = (pb.storage(rp, prec), pb.storage(rn, prec), npass)
    return m, ref


@_both
@pytest.mark.parametrize("voxel", pb.VOXELS)
def test_map_insert_scan_with_a_pose_twice(be, prec, oracle, voxel):
    m, (ref_p, ref_n, npass) = _inserted_map(be, prec, voxel, oracle)
    got_p, got_n = be.download(m)
    be.free(m)
    assert len(got_p) == len(ref_p) and 0 < npass < len(ref_p)
    np.testing.assert_array_equal(got_p[:npass], ref_p[:npass])  # pass-through block: first, in order, as placed
    np.testing.assert_array_equal(got_n[:npass], ref_n[:npass])
    if prec == "f64":  # (test_voxelize_within_volume_matches_oracle: the means are the oracle's bits, only the order of the voxels differs)
        j = _match(got_p[npass:], ref_p[npass:], 0.0)
        np.testing.assert_array_equal(got_p[npass:][j], ref_p[npass:])
        np.testing.assert_array_equal(got_n[npass:][j], ref_n[npass:])  # (summed in cloud order and re-normalised in double, like there)
    else:  # (test_voxel_down_sample_with_normals_and_f32: means and mean normals stored in f32)
        j = _match(got_p[npass:], ref_p[npass:], 5e-6)
        np.testing.assert_allclose(got_n[npass:][j], ref_n[npass:], rtol=0, atol=1e-6)


@_both
@pytest.mark.parametrize("voxel", pb.VOXELS)
def test_map_carve_of_a_persistent_map(be, prec, oracle, voxel):
    """a map that two insertions built is carved where it is (the carving voxel is the map's): the oracle's flags on a twin map built by
    the same calls and downloaded (the download folds the twin; the carved map is not looked at before the carve)"""
    twin, _ = _inserted_map(be, prec, voxel)
    tp, tn = be.download(twin)
    be.free(twin)
    m, _ = _inserted_map(be, prec, voxel)
    scan = pb.storage(pb.carve_scene()[2], prec)
    s = pb.CARVE_POSE[:3, 3]
    crop, ocrop = _carve_crops(oracle)
    subset = oracle.crop_indices(tp, ocrop)
    ref = oracle.carve_flags(pb.place(pb.CARVE_POSE, scan), s, tp, tn, subset, voxel=voxel)
    assert 0 < ref.sum() < len(subset) < len(tp)
    sc = be.upload(scan)
    assert be.is_persistent_map(m)
    removed = be.map_carve(m, sc, pb.CARVE_POSE, crop, voxel=voxel)
    assert be.is_persistent_map(m)  # carved in place
    got_p, got_n = be.download(m)
    assert removed == int(ref.sum())
    np.testing.assert_array_equal(got_p, tp[~ref])
    np.testing.assert_array_equal(got_n, tn[~ref])
    be.free(m)
    be.free(sc)


@_both
@pytest.mark.parametrize("voxel", pb.VOXELS)
def test_dense_map_insert_and_count_occupied_with_a_pose(be, prec, oracle, voxel):
    from scipy.spatial import cKDTree

    dp, dn = (pb.storage(x, prec) for x in pb.dense_scene(voxel))
    # (the dense map bins the placed doubles: nothing is rounded to storage in between)
    W, N = pb.place(pb.POSE, dp), pb.rotate(pb.POSE, dn)
    uniq, cnt, mean_p, mean_n, order = pb.dense_voxels(W, N, voxel)
    rp, rn, rc = oracle.dense_fuse(W, N, voxel)
    np.testing.assert_array_equal(rc, cnt[order])  # the restatement's voxels and counts are the oracle's
    dm = be.dense_map_create(voxel)
    c = be.upload(dp, dn)
    be.dense_map_insert(dm, c, pb.POSE)
    assert be.dense_map_size(dm) == len(rp)
    out = be.dense_map_to_cloud(dm)
    gp, gn = be.download(out)
    # Voxel by voxel in ascending key order: the device's mean against the mean of the oracle's members of that voxel.  A member in the
    # wrong voxel moves two means by a good fraction of the voxel (the members of a cluster spread over its interior), or adds or
    # removes a voxel -- so this holds the key set and the counts.  The bound is that of the fixed-point sums (2^-30 per point) and of
    # the f32 rounding of the mean.
    tol = 1e-8 if prec == "f64" else 1e-6
    assert len(gp) == len(uniq)
    assert np.abs(gp - mean_p).max() < tol, np.abs(gp - mean_p).max()
    d, j = cKDTree(rp).query(gp)  # and against the oracle's own means, as test_dense_voxel_map_matches_oracle pairs them
    assert np.array_equal(j, np.argsort(order)) and d.max() < tol
    if prec == "f64":  # (f32 storage keeps no normals in the dense map's cloud)
        np.testing.assert_allclose(gn, mean_n, rtol=0, atol=1e-9)
    be.free(out)
    be.free(c)
    be.dense_map_free(dm)
    # the occupancy count: the source placed by the pose, in a map of the target
    p, t = pb.storage(pb.face_aimed(voxel)[0], prec), pb.storage(pb.overlap_target(voxel), prec)
    occ = {tuple(k) for k in pb.keys(t, voxel)}
    want = sum(tuple(k) in occ for k in pb.keys(pb.place(pb.POSE, p), voxel))
    assert 0 < want < len(p)
    dm = be.dense_map_create(voxel)
    t_id, s_id = be.upload(t), be.upload(p)
    be.dense_map_insert(dm, t_id)
    assert be.dense_map_count_occupied(dm, s_id, pb.POSE) == want
    be.free(t_id)
    be.free(s_id)
    be.dense_map_free(dm)


@_both
@pytest.mark.parametrize("voxel", pb.VOXELS)
def test_dense_map_carve_with_a_scan_pose(be, prec, oracle, voxel):
    from scipy.spatial import cKDTree

    mp, _, scan = (pb.storage(x, prec) for x in pb.carve_scene())
    s = pb.CARVE_POSE[:3, 3]
    placed = pb.storage(pb.place(pb.CARVE_POSE, scan), prec)  # the device places the scan into a cloud of its storage and casts the rays from that
    rp, _, _ = oracle.dense_fuse(mp, None, voxel)
    m_id, sc = be.upload(mp), be.upload(scan)
    for kw in pb.DENSE_CARVE_PARAMS:
        dm = be.dense_map_create(voxel)
        be.dense_map_insert(dm, m_id)
        before_id = be.dense_map_to_cloud(dm)
        before = be.download(before_id)[0]
        d, j = cKDTree(rp).query(before)  # (test_points_on_voxel_faces_fall_where_the_oracle_puts_them)
        assert np.array_equal(np.sort(j), np.arange(len(rp))) and d.max() < (1e-8 if prec == "f64" else 1e-6)
        ref = oracle.dense_carve(placed, s, rp, voxel, **kw)[j]
        removed = be.dense_map_carve(dm, sc, s, scan_pose=pb.CARVE_POSE, **kw)
        assert removed == int(ref.sum()) and 0 < removed < len(before)
        after_id = be.dense_map_to_cloud(dm)
        np.testing.assert_array_equal(be.download(after_id)[0], before[~ref])  # exactly the oracle's voxels are gone
        for x in (before_id, after_id):
            be.free(x)
        be.dense_map_free(dm)
    be.free(m_id)
    be.free(sc)
