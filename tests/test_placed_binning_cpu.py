"""The premises of tests/placed_binning_cases.py, on the CPU: the numpy placement is the oracle's bit for bit, and the face-aimed inputs
are sharp -- the oracle's own result of every placed-then-binned operation changes when a once-rounded (fused-like) placement is put in
the step-by-step one's place, so an exact comparison of the device with the oracle on these inputs (tests/test_placed_binning_gpu.py)
can fail.  These are conditions on the inputs; nothing here measures the device."""
import numpy as np
import pytest

import placed_binning_cases as pb


def test_place_and_rotate_are_the_oracles_bit_for_bit(oracle):
    rng = np.random.default_rng(0)
    P = np.vstack([rng.uniform(-50.0, 50.0, (5000, 3)), pb.face_aimed(0.1)[0], pb.carve_scene()[2], np.zeros((1, 3)), [[1e-300, -1e30, 3.0]]])
    N = pb._unit(rng.normal(size=P.shape))
    for T in (pb.POSE, pb.CARVE_POSE, pb.inverse(pb.POSE), np.eye(4)):
        np.testing.assert_array_equal(pb.place(T, P), oracle.transform_points(P, T))
        np.testing.assert_array_equal(pb.rotate(T, N), oracle.transform_normals(N, T))
    assert np.all(pb.POSE[:3, :3] != 0.0)  # a general pose: no row of the placement is shorter than another
    for prec in ("f64", "f32"):
        x = pb.storage(P[:100], prec)
        assert x.dtype == np.float64 and np.array_equal(x, pb.storage(x, prec))
    assert np.array_equal(pb.storage(P, "f64"), P) and not np.array_equal(pb.storage(P, "f32"), P)


@pytest.mark.parametrize("voxel", pb.VOXELS)
def test_face_aimed_points_tell_the_placements_apart(voxel):
    """at least 5 % of the points change voxel when the placement is rounded once, and at least 20 % land on each side of their face"""
    for p, _, q, owner, axis in (pb.face_aimed(voxel), pb.face_aimed(voxel, seed=2, n_anchor=1000)):
        assert 2500 <= len(p) <= 4500 and len(p) % 256 != 0
        w, w1 = pb.place(pb.POSE, p), pb.place_rounded_once(pb.POSE, p)
        changed = np.any(pb.keys(w, voxel) != pb.keys(w1, voxel), axis=1)
        assert changed.mean() >= 0.05, changed.mean()
        a = axis[owner]
        face = q[np.arange(len(q)), a]
        got = w[np.arange(len(q)), a]
        assert np.abs(got - face).max() < 1e-13  # within a few ulp of the face ...
        below = (pb.keys(w, voxel) < pb.keys(q, voxel))[np.arange(len(q)), a]
        assert 0.2 <= below.mean() <= 0.8, below.mean()  # ... on either side
        assert np.abs(w - q).max() < 1e-13


def _carve_subset(oracle, mp):
    return oracle.crop_indices(mp, oracle.make_crop(oracle.CROP_MAX_RADIUS, center=pb.CARVE_POSE[:3, 3], rmax=pb.CARVE_RMAX))


def test_carving_scene_is_sharp(oracle):
    mp, mn, scan = pb.carve_scene()
    s = pb.CARVE_POSE[:3, 3]
    assert len(mp) == 6400 and len(scan) == 2000 and len(scan) % 256 != 0
    subset = _carve_subset(oracle, mp)
    assert 0 < len(subset) < len(mp)
    w, w1 = pb.place(pb.CARVE_POSE, scan), pb.place_rounded_once(pb.CARVE_POSE, scan)
    length = np.linalg.norm(w - s, axis=1)
    for voxel in pb.VOXELS:
        samples = np.ceil(np.maximum(voxel, np.minimum(length - 0.1, 20.0)) / voxel).astype(int)  # of the default parameters
        assert {0, 1, 7} <= set((samples % 8).tolist()) and samples.min() < 8 < samples.max()  # whole and partial batches of 8
        for nrm in (mn, None):
            for kw in pb.CARVE_PARAMS:
                ref = oracle.carve_flags(w, s, mp, nrm, subset, voxel=voxel, **kw)
                assert 0 < ref.sum() < len(subset)
                assert not ref[np.setdiff1d(np.arange(len(mp)), subset)].any()
                other = oracle.carve_flags(w1, s, mp, nrm, subset, voxel=voxel, **kw)
                assert np.any(ref != other), (voxel, nrm is None, kw)
        # the dense map's carving of the same scene
        rp, _, _ = oracle.dense_fuse(mp, None, voxel)
        for kw in pb.DENSE_CARVE_PARAMS:
            ref = oracle.dense_carve(w, s, rp, voxel, **kw)
            assert 0 < ref.sum() < len(rp)
            assert np.any(ref != oracle.dense_carve(w1, s, rp, voxel, **kw)), (voxel, kw)


@pytest.mark.parametrize("voxel", pb.VOXELS)
def test_overlap_dense_map_and_insertion_inputs_are_sharp(oracle, voxel):
    p, n = pb.face_aimed(voxel)[:2]
    t = pb.overlap_target(voxel)
    assert 3000 <= len(t) <= 5000 and len(t) % 256 != 0
    w, w1 = pb.place(pb.POSE, p), pb.place_rounded_once(pb.POSE, p)
    eye = np.eye(4)
    for min_points in (1, 3):
        r_s, r_t = oracle.overlap_indices(p, t, pb.POSE, voxel, min_points)
        assert 0 < len(r_s) < len(p) and 0 < len(r_t) < len(t)
        # placing first and binning at the identity is the same thing
        e_s, e_t = oracle.overlap_indices(w, t, eye, voxel, min_points)
        np.testing.assert_array_equal(r_s, e_s)
        np.testing.assert_array_equal(r_t, e_t)
        o_s, o_t = oracle.overlap_indices(w1, t, eye, voxel, min_points)
        assert not np.array_equal(r_s, o_s) and not np.array_equal(r_t, o_t)
    # the dense map: voxel set and counts of the placed cloud, and the occupancy count of the placed source in a map of the target
    dp, dn = pb.dense_scene(voxel)
    key_of = lambda P: np.array([oracle.lib().orc_voxel_key(np.ascontiguousarray(x).ctypes.data_as(oracle._dp), voxel) for x in P], np.int64)
    fused = lambda P: dict(zip(key_of(oracle.dense_fuse(P, None, voxel)[0]).tolist(), oracle.dense_fuse(P, None, voxel)[2].tolist()))
    a, b = fused(pb.place(pb.POSE, dp)), fused(pb.place_rounded_once(pb.POSE, dp))
    assert 1 < len(a) < len(dp) and a != b and set(a) != set(b)
    occ = {tuple(k) for k in pb.keys(t, voxel)}
    hits = lambda W: sum(tuple(k) in occ for k in pb.keys(W, voxel))
    assert 0 < hits(w) < len(p) and hits(w) != hits(w1)
    # two insertions into one map
    ocrop = oracle.make_crop(oracle.CROP_MAX_RADIUS, center=pb.POSE[:3, 3], rmax=pb.INSERT_RMAX)
    outs = []
    for plc in (pb.place, pb.place_rounded_once):
        mp, mn = np.zeros((0, 3)), np.zeros((0, 3))
        for sp, sn in pb.insert_scans(voxel):
            mp, mn, npass = oracle.voxelize_within_volume(np.vstack([mp, plc(pb.POSE, sp)]), np.vstack([mn, pb.rotate(pb.POSE, sn)]), voxel, ocrop)
        assert 0 < npass < len(mp)
        outs.append((mp, mn))
    assert len(outs[0][0]) != len(outs[1][0]) or not np.array_equal(np.sort(outs[0][0], axis=0), np.sort(outs[1][0], axis=0))
    # ... and the carving scene's rays through the map they built, with the map's voxel (the carve of a map in its persistent form)
    mp, mn = outs[0]
    scan, s = pb.carve_scene()[2], pb.CARVE_POSE[:3, 3]
    subset = _carve_subset(oracle, mp)
    ref = oracle.carve_flags(pb.place(pb.CARVE_POSE, scan), s, mp, mn, subset, voxel=voxel)
    assert 0 < ref.sum() < len(subset) < len(mp)
    assert np.any(ref != oracle.carve_flags(pb.place_rounded_once(pb.CARVE_POSE, scan), s, mp, mn, subset, voxel=voxel))
    # the numpy restatement of the dense map is the oracle's: same voxels in its order, same counts, same means
    W, N = pb.place(pb.POSE, dp), pb.rotate(pb.POSE, dn)
    _, cnt, mean_p, mean_n, order = pb.dense_voxels(W, N, voxel)
    rp, rn, rc = oracle.dense_fuse(W, N, voxel)
    np.testing.assert_array_equal(rc, cnt[order])
    np.testing.assert_allclose(rp, mean_p[order], rtol=0, atol=1e-13)
    np.testing.assert_allclose(rn, mean_n[order], rtol=0, atol=1e-13)
    assert cnt.max() >= 3 and (cnt == 1).any()
