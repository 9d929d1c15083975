"""The ICP neighbour search per query against brute force (needs an MI355X).

Every registration entry point rests on one device routine, the exact 1-NN within radius of icp_kernels.hpp (nn_search_group,
nn_search_wave_far, consider, scan_strided, the cached starting bound, the neighbourhood-major replica, the crop predicate, the candidate
sets of the fused kernel).  Here its per-query observable -- o3ds_icp_nn_keys: float bits of d2, rank, position, or "none" -- and the
step record of the same session state are held against tests/icp_search_restatement.py, whose agreement with the oracle
tests/test_icp_search_restatement_cpu.py proves without a GPU.  Row search and replica, f32 and f64 storage.

The checks and the derivation of their bounds are in tests/icp_search_harness.py (check_keys, check_record, check_record_gicp); every
test prints the largest observed ratio before it asserts.

The generalized estimator's record (write_record<P4, true>, gicp_record, the 32-slot LDS stride and its zeroing, the source-normal gather
at a.first + i under all three dealing orders) is held per term to rs.record_gicp twice: to the closed form the device documents
(I - k n n^T, n := e1 for x < -0.99 and for the zero vector) within REC_TOL * scale in both storages, and to Open3D's own form
(Rx diag(eps, 1, 1) Rx^T per stored normal) within (REC_TOL + 2 * DEFECT) * scale, DEFECT being the distance of the two REFERENCES on the
same stored normals (tests/test_icp_search_restatement_cpu.py: below 2e-13 in f64 storage, up to 4e-5 in f32 storage, whose normals are
unit to 6e-8 only).  scale is the restatement's: sum over the pairs of |B|_2 times the 1-norms of the columns of A (and of d).
  The derivation of REC_TOL against the cofactor inverse, as found: given its M, gicp_record's inverse is accurate to about 25 roundings
  relative to |B|_2 -- the eigenvalues of M = 2I - k (a a^T + b b^T) are 2, 2 - k (1 - c) and lambda_min = 2 - k (1 + c), c = |a . b|, so
  the two that are not lambda_min multiply to at least 2 and det M >= 2 lambda_min: the cofactors (errors of a few roundings of |M|^2 <= 4)
  over the determinant stay within tens of 2^-53 of 1 / lambda_min.  The products S^T B S, B d add under ten roundings relative to
  |B| alpha_a alpha_b each.  What the statement "a few tens of roundings" leaves out is M itself: a = R ns and the six entries of M are
  rounded (about 8 roundings of entries of size <= 2), and the inverse amplifies an error of M by |B|, so RELATIVE to |B| that part is
  8 * 2^-53 * |B|_2: nothing for random normals (|B| = O(1): the three orders of margin), 4.4e-13 at most where a = +-b and eps = 1e-3
  (|B| = 500: the "src a=b" and "src a=-b" groups of the edge case, bound 0.44, observed below), and beyond REC_TOL only for eps = 1e-6
  with 1 - |a . b| < 1e-3, which 300 random pairs do not reach (their largest |B| is about 300: bound 0.27).
  Observed on an MI355X, largest deviation / bound per group of checks (closed form f32 / f64 | Open3D's form f32 / f64):
    lattice 0.0026 / 0.0014 | 0.50 / 0.0054     stage clouds, poses, epsilons 0.0069 / 0.0078 | 0.071 / 0.0076     large 0.00032 / 0.00014 | 0.015 / 0.00047
    edge normals 0.0090 / 0.0065 | 0.078 / 0.023  (the worst group on either side is a = +-b)     crop 0.00047 / 0.0013 | 0.039 / 0.0023
    later passes 0.012 / 0.017 | 0.15 / 0.024     two shards 0.0017 / 0.00083 | 0.060 / 0.0054
  Every figure is below 0.1 but two of Open3D's form in f32 storage, and those are so by construction, not by the device: there
  |device - closed| is nothing beside DEFECT, so |device - o3d| is the distance of the two references, which for the worst pair IS
  DEFECT * scale in its worst entry -- a record of that pair alone (lattice-1) sits at DEFECT / (2 * DEFECT) = 0.5 exactly, records of
  many pairs below it.  The bound follows from |device - o3d| <= |device - closed| + |closed - o3d| <= (REC_TOL + DEFECT) * scale; the
  factor 2 on DEFECT is headroom, and the sharp statement about the device is the closed-form comparison.
  Before write_record took the zero vector for e1, the zero-normal groups of the edge case stood at 9.2e3 / 5.5e11 (target side) and
  9.3e3 / 5.5e11 (source side) times the bound against Open3D's form.
The fused kernel's generalized records are tied to the same restatement through the step-wise ABI: o3ds_icp_register_dev equals begin /
accumulate / update / finish bit for bit, and the step-wise records are the ones checked here."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_search_harness as harness  # noqa: E402
import icp_search_restatement as rs  # noqa: E402

from open3d_slam_amd import backend  # noqa: E402

pytestmark = pytest.mark.gpu

PREC, PATHS, REC_TOL = harness.PREC, harness.PATHS, harness.REC_TOL


@pytest.fixture(autouse=True)
def _eager_replica(monkeypatch):
    harness.eager_replica(monkeypatch)


@pytest.fixture(scope="module")
def ab():
    yield from harness.backends(True)


@pytest.fixture(scope="module")
def shipped():
    yield from harness.backends(False)


@functools.lru_cache(maxsize=None)
def _case(name):
    return {c.name: c for c in rs.all_cases()}[name]


@functools.lru_cache(maxsize=None)
def _ref(name, storage):
    c = _case(name)
    return rs.nearest_within(c.src, c.tgt, c.T, c.r, storage)


def _run_case(ab, monkeypatch, name, storage, first=0, count=None, rank=3):
    c = _case(name)
    m = _ref(name, storage)
    count = len(c.src) - first if count is None else count
    ses = harness.Session(ab[storage], c.src, c.tgt, c.nrm, c.r, c.cell)
    try:
        for path in PATHS:
            what = f"{name} {storage} {path} [{first},{first + count})"
            harness.set_path(path, monkeypatch)
            for method in (backend.ICP_POINT_TO_PLANE, backend.ICP_POINT_TO_POINT):
                ses.begin(c.T, path, method=method)
                keys = ses.keys(first, count, rank)
                rec = ses.record(first, count)
                harness.check_keys(keys, m, storage, c.exact, rank, len(c.tgt), first, count, what)
                harness.check_record(rec, m, c.tgt, c.nrm, storage, method, first, count, f"{what} method {method}")
    finally:
        ses.close()


def _ids(cases):
    return [c.name for c in cases]


# ---- a. lattice: exact ties, points on cell faces, one ulp to either side of a face, workgroup and wavefront boundaries
@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("n", rs.LATTICE_COUNTS)
def test_lattice_exact_bits_and_tie_rule(ab, monkeypatch, storage, n):
    _run_case(ab, monkeypatch, f"lattice-{n}", storage)


@pytest.mark.parametrize("storage", rs.STORAGES)
def test_lattice_sub_range(ab, monkeypatch, storage):
    _run_case(ab, monkeypatch, "lattice-300", storage, first=rs.LATTICE_SUBRANGE[0], count=rs.LATTICE_SUBRANGE[1])


# ---- b. the radius itself: strict
@pytest.mark.parametrize("name", _ids(rs.radius_cases()))
def test_radius_is_strict(ab, monkeypatch, name):
    for storage in _case(name).storages:
        _run_case(ab, monkeypatch, name, storage)


# ---- c. stage boundaries
@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("cell", rs.STAGE_CELLS)
@pytest.mark.parametrize("void", rs.STAGE_VOIDS)
def test_stage_boundaries(ab, monkeypatch, void, cell, storage):
    _run_case(ab, monkeypatch, f"void{void}-cell{cell}-r1.0", storage)


@pytest.mark.parametrize("storage", rs.STORAGES)
def test_matches_and_misses_in_one_workgroup(ab, monkeypatch, storage):
    _run_case(ab, monkeypatch, "void0.9-cell0.25-r0.5", storage)


# ---- d. outside the grid, far away, non-finite rows
@pytest.mark.parametrize("storage", rs.STORAGES)
def test_queries_outside_the_grid(ab, monkeypatch, storage):
    _run_case(ab, monkeypatch, "outside", storage)


# ---- e. thin and tiny
@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("name", _ids(rs.tiny_cases()))
def test_thin_and_tiny_targets(ab, monkeypatch, name, storage):
    _run_case(ab, monkeypatch, name, storage)


# ---- f. a radius beyond 64 cells
@pytest.mark.parametrize("storage", rs.STORAGES)
def test_radius_beyond_64_cells(ab, monkeypatch, storage):
    """An index built explicitly with cell c is never rebuilt for another radius, so r / c is unbounded (a map indexed for scan matching,
    then used for a loop-closure refinement at ten times the radius).  Before row_extent stopped cutting rows at +-64 cells the query 70
    cells from its neighbour reported "no match" (f32 and f64, rows and replica alike)."""
    _run_case(ab, monkeypatch, "far-radius", storage)


# ---- h. large coordinates
@pytest.mark.parametrize("name", _ids(rs.large_cases()))
def test_large_coordinates(ab, monkeypatch, name):
    for storage in _case(name).storages:
        _run_case(ab, monkeypatch, name, storage)


# ---- g. crops
@functools.lru_cache(maxsize=None)
def _crop_ref(k, storage):
    from oracle import pyoracle

    src, tgt, nrm = rs.void_cloud(rs.CROP_VOID)
    keep = pyoracle.crop_indices(rs.to_storage(tgt, storage), pyoracle.make_crop(**rs.CROPS[k]))
    return rs.nearest_within(src, tgt, np.eye(4), 1.0, storage, keep=keep)


@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("k", range(len(rs.CROPS)))
def test_crops(ab, monkeypatch, k, storage):
    src, tgt, nrm = rs.void_cloud(rs.CROP_VOID)
    m = _crop_ref(k, storage)
    crop = backend.make_crop(**rs.CROPS[k])
    ses = harness.Session(ab[storage], src, tgt, nrm, 1.0, 0.25)
    try:
        for path in PATHS:
            what = f"crop{k} {storage} {path}"
            harness.set_path(path, monkeypatch)
            ses.begin(np.eye(4), path, crop=crop)
            keys = ses.keys(rank=1)
            rec = ses.record()
            harness.check_keys(keys, m, storage, False, 1, len(tgt), 0, len(src), what)
            harness.check_record(rec, m, tgt, nrm, storage, backend.ICP_POINT_TO_PLANE, 0, len(src), what)
            if k == 0:  # [O3D] GetInformationMatrixFromPointClouds with the crop that excludes every query's nearest points
                got = ses.be.information_matrix_dev(ses.s, ses.t, 1.0, np.eye(4), target_crop=crop)
                ref = rs.information(tgt, m.idx, storage)
                assert got[3, 3] == ref[3, 3] == (m.idx >= 0).sum()
                if storage == rs.F64:  # the tolerances of test_icp_gpu.py::test_information_matrix_matches_oracle
                    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-7)
                else:
                    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-5 * np.abs(ref).max())
    finally:
        ses.close()


# ---- i. later passes: the cached bound, which may be stale
@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("method", [backend.ICP_POINT_TO_POINT, backend.ICP_POINT_TO_PLANE, backend.ICP_GENERALIZED])
@pytest.mark.parametrize("void", [0.0, 0.6])
def test_later_passes(ab, monkeypatch, void, method, storage):
    """k rounds of nn_keys / accumulate_keys / update, then the keys of round k; icp_finish returns the pose those keys were computed under
    (sessions replay bit for bit), so the brute force uses exactly that matrix.  Point-to-plane runs on random unit normals: its updates
    jump, which is what a stale bound needs.  Generalized: rounds 0, 1 and 2.. deal the queries out in the three orders of pass_order,
    and the source normal is gathered by the dealt index."""
    import torch

    src, tgt, nrm = rs.void_cloud(void)
    sn = rs.void_source_normals(void)
    n = len(src)
    ses = harness.Session(ab[storage], src, tgt, nrm, 1.0, 0.25, src_nrm=sn)
    try:
        for path in PATHS:
            harness.set_path(path, monkeypatch)
            for k in range(4):
                what = f"later void{void} method {method} {storage} {path} round {k}"
                ses.begin(rs.LATER_INIT, path, method=method)
                for _ in range(k):
                    keys = ses.keys()
                    rec = ses.record(keys=keys)
                    ses.be.icp_update(rec.data_ptr(), n)
                keys = ses.keys()
                rec_keys = ses.record(keys=keys)
                rec_foreign = ses.record(keys=keys, rank=1)
                rec_plain = ses.record()
                assert torch.equal(keys, ses.keys()), what  # the search of a state is repeatable (now from the bound its first run cached)
                T = ses.be.icp_finish()["transformation"]
                assert (T != rs.LATER_INIT).any() == (k > 0), what
                m = rs.nearest_within(src, tgt, T, 1.0, storage)
                harness.premises(m, 1.0, what)
                harness.check_keys(keys, m, storage, False, 0, len(tgt), 0, n, what)
                if method == backend.ICP_GENERALIZED:
                    harness.check_record_gicp(rec_plain, m, tgt, nrm, sn, storage, T, rs.GICP_EPSILON, 0, n, what)
                else:
                    harness.check_record(rec_plain, m, tgt, nrm, storage, method, 0, n, what)
                a, b = rec_keys.cpu().numpy(), rec_plain.cpu().numpy()
                same = np.ones(32, dtype=bool)
                same[[27, 29]] = False  # (these may carry the float-rounded d2 of the key)
                np.testing.assert_array_equal(a[same], b[same], err_msg=what)
                np.testing.assert_allclose(a[~same], b[~same], rtol=2.0 ** -23, atol=0, err_msg=what)
                assert not rec_foreign.cpu().numpy().any(), f"{what}: a record accumulated under a foreign rank is all zero"
    finally:
        ses.close()


# ---- j. two shards on one GPU
@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("name", ["lattice-300", "void0.6-cell0.25-r1.0"])
def test_two_shards(ab, monkeypatch, name, storage):
    """the element-wise minimum of the two shards' keys is the brute force over the union (a tie goes to the lower rank), the sum of the two
    accumulate_keys records is the union's record"""
    import torch

    c, m = _case(name), _ref(name, storage)
    sn = rs.lattice_source_normals(len(c.src)) if name.startswith("lattice") else rs.void_source_normals(0.6)
    h = len(c.tgt) // 2
    other = backend.Backend(0, PREC[storage], ab=True)
    parts = []
    try:
        parts += [harness.Session(ab[storage], c.src, c.tgt[:h], c.nrm[:h], c.r, c.cell, src_nrm=sn),
                  harness.Session(other, c.src, c.tgt[h:], c.nrm[h:], c.r, c.cell, src_nrm=sn)]
        for path in PATHS:
            what = f"shards {name} {storage} {path}"
            harness.set_path(path, monkeypatch)
            ks = []
            for rank, ses in enumerate(parts):
                ses.begin(c.T, path)
                ks.append(ses.keys(rank=rank))
            merged = torch.minimum(ks[0], ks[1])
            torch.cuda.synchronize()
            none, d2, rk, pos = rs.decode_keys(merged.cpu().numpy())
            np.testing.assert_array_equal(none, m.idx < 0, err_msg=what)
            np.testing.assert_array_equal(rk[~none], (m.idx[~none] >= h).astype(np.int64), err_msg=f"{what}: which shard holds the winner")
            for rank in (0, 1):
                mine = ~none & (rk == rank)
                assert (pos[mine] < (h if rank == 0 else len(c.tgt) - h)).all()
            # d2 as in the single-shard test: the merged keys against the union's matches (rank is checked above)
            dev = d2[~none]
            ref = m.d2[~none]
            if c.exact:
                np.testing.assert_array_equal(dev.view(np.uint32), ref.astype(np.float32).view(np.uint32), err_msg=what)
            elif storage == rs.F32:
                assert (np.abs(dev.astype(np.float64) - ref) <= rs.D2_F32_REL * ref).all(), what
            else:
                assert (np.abs(dev.astype(np.float64) - ref.astype(np.float32).astype(np.float64)) <= rs.ulp32(ref)).all(), what
            total = np.zeros(32)
            for rank, ses in enumerate(parts):
                total += ses.record(keys=merged, rank=rank).cpu().numpy()
            ref_rec, scale = rs.record(m.p, c.tgt, c.nrm, m.idx, storage)
            tol = np.full(32, REC_TOL)
            if storage == rs.F32:
                tol[[27, 29]] = rs.D2_F32_REL
            assert total[28] == ref_rec[28]
            assert (np.abs(total - ref_rec) <= tol * scale).all(), f"{what}: {np.abs(total - ref_rec) / np.maximum(tol * scale, 1e-300)}"
            print(f"SEARCH {what}: {int(ref_rec[28])} matches of {len(c.src)}, {int((rk[~none] == 1).sum())} in shard 1")
            # the generalized estimator: each shard gathers ITS half's normals; the sum is the union's record
            total = np.zeros(32)
            for rank, ses in enumerate(parts):
                ses.begin(c.T, path, method=backend.ICP_GENERALIZED)
                total += ses.record(keys=merged, rank=rank).cpu().numpy()
            harness.check_record_gicp(total, m, c.tgt, c.nrm, sn, storage, c.T, rs.GICP_EPSILON, 0, len(c.src), f"{what} generalized")
    finally:
        for ses in parts:
            ses.close()
        other.close()


# ---- k. a persistent-map target
@pytest.mark.parametrize("storage", rs.STORAGES)
def test_persistent_map_target(ab, storage):
    """two map_insert_scan calls with max_corr_hint leave the map in its persistent form (row-paged index, no replica); the keys and the record
    are taken against it as it is, the map is downloaded (which folds it) only afterwards, and the brute force runs against the
    downloaded points"""
    be = ab[storage]
    src, tgt, _ = rs.void_cloud(0.3)
    crop = backend.make_crop(backend.CROP_MAX_RADIUS, center=tuple(rs.VOID_CENTRE), rmax=2.5)
    mp = be.upload(np.zeros((0, 3)))
    scans = [be.upload(tgt[:10_000]), be.upload(tgt[10_000:])]
    ses = harness.Session(be, src, None, None, 1.0, None, target_id=mp)
    try:
        for sc in scans:
            be.map_insert_scan(mp, sc, np.eye(4), 0.1, crop, max_corr_hint=1.0)
        assert be.is_persistent_map(mp)
        ses.begin(np.eye(4), method=backend.ICP_POINT_TO_POINT)
        keys = ses.keys(rank=2)
        rec = ses.record()
        assert be.is_persistent_map(mp), "taking keys folded the map"
        pts, _ = be.download(mp)
        m = rs.nearest_within(src, pts, np.eye(4), 1.0, storage)
        what = f"persistent map {storage}"
        harness.premises(m, 1.0, what)
        assert 15_000 < len(pts) <= len(tgt)
        harness.check_keys(keys, m, storage, False, 2, None, 0, len(src), what)  # (positions are slots of the row-paged index, not array positions)
        harness.check_record(rec, m, pts, None, storage, backend.ICP_POINT_TO_POINT, 0, len(src), what)
    finally:
        for c in scans:
            be.free(c)
        ses.close()


# ---- l. the fused kernel (the shipped library: candidate sets on, lanes re-dealt)
def _fused_inputs():
    out = []
    for v in rs.STAGE_VOIDS:
        for cell in rs.STAGE_CELLS:
            out.append((f"void{v}-cell{cell}", v, cell, 1.0, None, np.eye(4), backend.ICP_POINT_TO_PLANE))
    out.append(("void0.9-r0.5", 0.9, 0.25, 0.5, None, np.eye(4), backend.ICP_POINT_TO_PLANE))
    for k in range(len(rs.CROPS)):
        out.append((f"crop{k}", rs.CROP_VOID, 0.25, 1.0, k, np.eye(4), backend.ICP_POINT_TO_PLANE))
    for v in (0.0, 0.6):
        for method in (backend.ICP_POINT_TO_POINT, backend.ICP_POINT_TO_PLANE, backend.ICP_GENERALIZED):
            out.append((f"later-void{v}-method{method}", v, 0.25, 1.0, None, rs.LATER_INIT, method))
    return out


FUSED = _fused_inputs()


@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("inp", FUSED, ids=[f[0] for f in FUSED])
def test_fused_kernel_counts_and_rmse(shipped, inp, storage):
    """o3ds_icp_register_dev, o3ds_icp_register_multi and o3ds_icp_register_batch (lists of one) with max_iteration 0..3 and fixed
    criteria: n_corr is the brute-force count at the returned pose, inlier_rmse is sqrt(sum d2 / n) within the d2 bound"""
    from oracle import pyoracle

    name, void, cell, r, crop_k, T0, method = inp
    be = shipped[storage]
    src, tgt, nrm = rs.void_cloud(void, query_radius=None if r == 1.0 else rs.VOID_QUERY_RADIUS_MIXED)  # (the queries of stage_case)
    crop = keep = None
    if crop_k is not None:
        crop = backend.make_crop(**rs.CROPS[crop_k])
        keep = pyoracle.crop_indices(rs.to_storage(tgt, storage), pyoracle.make_crop(**rs.CROPS[crop_k]))
    bound = rs.D2_F32_REL if storage == rs.F32 else 2.0 ** -23
    s, t = be.upload(src, rs.void_source_normals(void) if method == backend.ICP_GENERALIZED else None), be.upload(tgt, nrm)
    try:
        be.build_index(t, r, cell)
        seen = {}
        for k in range(4):
            params = be._params(r, k, 0.0, 0.0, method)
            runs = {"dev": be.icp_register_dev(s, t, r, init=T0, max_iter=k, rel_fitness=0.0, rel_rmse=0.0, target_crop=crop, method=method),
                    "multi": be.icp_register_multi(s, [t], form=be.MULTI_UNION, crop=crop, init=T0, params=params)}
            res, status = be.icp_register_batch([(s, t, crop, T0)], params)
            assert status == [0]
            runs["batch"] = res[0]
            for form, got in runs.items():
                what = f"fused {name} {storage} {form} max_iter {k}"
                key = got["transformation"].tobytes()
                if key not in seen:
                    m = rs.nearest_within(src, tgt, got["transformation"], r, storage, keep=keep)
                    harness.premises(m, r, what)
                    # (terms [28] and [29], the ones read below, are the same in every method)
                    seen[key] = rs.record(m.p, tgt, nrm, m.idx, storage, rs.METHOD_POINT_TO_POINT if method == backend.ICP_GENERALIZED else method)[0]
                ref = seen[key]
                assert got["n_corr"] == ref[28], f"{what}: n_corr {got['n_corr']}, brute force {int(ref[28])}"
                mean = ref[29] / max(ref[28], 1.0)
                dev = abs(got["inlier_rmse"] ** 2 - mean) / (bound * mean) if mean > 0 else abs(got["inlier_rmse"])
                print(f"SEARCH {what}: n_corr {got['n_corr']} of {len(src)}, rmse^2 deviation / bound {dev:.3e}")
                assert dev <= 1.0, f"{what}: inlier_rmse {got['inlier_rmse']} vs {np.sqrt(mean)}"
    finally:
        be.free(s)
        be.free(t)


@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("void", [0.0, 0.6])
def test_fused_generalized_equals_the_step_wise_abi(shipped, void, storage):
    """o3ds_icp_register_dev(method = generalized, max_iteration k), k = 0..3, equals begin / (accumulate, update) per iteration / finish
    on the same handle bit for bit: transformation, fitness, inlier_rmse, iterations, n_corr (as tests/test_icp_step_gpu.py compares).
    The step-wise records are the ones held to the restatement above, so this ties the fused kernel's -- its candidate-set path's own
    write_record call site included -- to it."""
    import torch

    be = shipped[storage]
    src, tgt, nrm = rs.void_cloud(void)
    n = len(src)
    s, t = be.upload(src, rs.void_source_normals(void)), be.upload(tgt, nrm)
    rec = torch.zeros(32, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    try:
        be.build_index(t, 1.0, 0.25)
        for k in range(4):
            kw = dict(init=rs.LATER_INIT, max_iter=k, rel_fitness=0.0, rel_rmse=0.0, method=backend.ICP_GENERALIZED)
            fused = be.icp_register_dev(s, t, 1.0, **kw)
            be.icp_begin(s, t, 1.0, **kw)
            for _ in range(k + 1):
                be.icp_accumulate(0, n, rec.data_ptr())
                be.icp_update(rec.data_ptr(), n)
                if be.icp_done():
                    break
            assert be.icp_done()
            step = be.icp_finish()
            what = f"fused generalized void{void} {storage} max_iter {k}"
            print(f"SEARCH {what}: iterations {fused['iterations']}, n_corr {fused['n_corr']}, rmse {fused['inlier_rmse']}")
            assert fused["iterations"] == k and (k == 0 or (fused["transformation"] != rs.LATER_INIT).any()), what
            fa = np.concatenate([fused["transformation"].reshape(16), [fused["fitness"], fused["inlier_rmse"]]])
            fb = np.concatenate([step["transformation"].reshape(16), [step["fitness"], step["inlier_rmse"]]])
            assert np.array_equal(fa.view(np.uint64), fb.view(np.uint64)), (what, fa, fb)
            assert (fused["iterations"], fused["n_corr"]) == (step["iterations"], step["n_corr"]), what
    finally:
        be.free(s)
        be.free(t)


# ---- m. negative control: the inputs reach the far stage
def test_negative_control_stage_three_skipped(ab, monkeypatch):
    """O3DS_DEBUG_ACC=16 (A/B library) skips stage 3.  The comparison of the stage cases must then report mismatches on the void-0.9 cloud
    and none on the void-0 cloud: the inputs reach the far stage, and the comparison notices a search that stops early.  The count per
    case is a lower bound of the queries stage 3 serves (an unproven stage-2 result is often the right one already)."""
    harness.set_path("rows", monkeypatch)
    counts = {}
    for void in rs.STAGE_VOIDS:
        for cell in (0.25, 0.1):
            name = f"void{void}-cell{cell}-r1.0"
            c, m = _case(name), _ref(name, rs.F32)
            ses = harness.Session(ab[rs.F32], c.src, c.tgt, c.nrm, c.r, c.cell)
            try:
                monkeypatch.setenv("O3DS_DEBUG_ACC", "16")
                ses.begin(c.T)
                none, d2, _, _ = rs.decode_keys(ses.keys().cpu().numpy())
                monkeypatch.delenv("O3DS_DEBUG_ACC")
            finally:
                ses.close()
            wrong = none != (m.idx < 0)
            both = ~none & (m.idx >= 0)
            wrong[both] = np.abs(d2[both].astype(np.float64) - m.d2[both]) > rs.D2_F32_REL * m.d2[both]
            counts[name] = int(wrong.sum())
            print(f"SEARCH control {name}: {counts[name]} of {len(c.src)} queries wrong without stage 3")
    assert counts["void0.9-cell0.25-r1.0"] > 0 and counts["void0.9-cell0.1-r1.0"] > 0
    assert counts["void0.0-cell0.25-r1.0"] == 0


# ---- n. the generalized estimator's record per correspondence (both forms of the restatement, see the module docstring)
_gicp_case = rs._gicp_case


def _run_gicp(ab, monkeypatch, name, storage, ranges=None, paths=PATHS):
    """the generalized record of a case on both paths; ranges: (label, first, count) sub-ranges, default the whole source"""
    c = _gicp_case(name)
    m = rs.gicp_matches(name, storage)
    defect = rs.defect(name, storage)   # the largest over ALL pairs of the case: covers every sub-range
    ranges = [("all", 0, len(c.src))] if ranges is None else ranges
    ses = harness.Session(ab[storage], c.src, c.tgt, c.nrm, c.r, c.cell, src_nrm=c.src_nrm)
    worst = 0.0
    try:
        with ses.eps(c.eps):
            for path in paths:
                harness.set_path(path, monkeypatch)
                ses.begin(c.T, path, method=backend.ICP_GENERALIZED)
                for label, first, count in ranges:
                    what = f"gicp {name} {storage} {path} {label} [{first},{first + count})"
                    rec = ses.record(first, count)
                    worst = max(worst, harness.check_record_gicp(rec, m, c.tgt, c.nrm, c.src_nrm, storage, c.T, c.eps, first, count, what, defect))
    finally:
        ses.close()
    return worst


@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("n", rs.LATTICE_COUNTS)
def test_gicp_lattice(ab, monkeypatch, storage, n):
    """workgroup boundaries under the 32-slot stride; the duplicated lattice points carry different normals, so the record shows the tie
    rule"""
    _run_gicp(ab, monkeypatch, f"lattice-{n}", storage)


@pytest.mark.parametrize("storage", rs.STORAGES)
def test_gicp_lattice_sub_range(ab, monkeypatch, storage):
    """first = 37: the source normal of query i is the one at a.first + i"""
    _run_gicp(ab, monkeypatch, "lattice-300", storage, ranges=[("sub-range",) + rs.LATTICE_SUBRANGE])


@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("name", ["void0.0-cell0.25-r1.0", "void0.9-cell0.25-r1.0", "void0.9-cell0.25-r0.5"])
def test_gicp_stage_clouds(ab, monkeypatch, name, storage):
    """the last one has matches and misses in one workgroup: a miss zeroes 32 slots, not 10"""
    _run_gicp(ab, monkeypatch, name, storage)


@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("pose", ["later-init", "yaw170"])
def test_gicp_poses(ab, monkeypatch, pose, storage):
    """the source covariance rotates with the pose (the identity is the stage clouds' pose)"""
    _run_gicp(ab, monkeypatch, f"void0.0-pose-{pose}", storage)


@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("eps", rs.GICP_EPSILONS)
def test_gicp_epsilon(ab, monkeypatch, eps, storage):
    """epsilon 1 (k = 0, M = 2I), the default and 1e-6; DEFECT is computed per value"""
    _run_gicp(ab, monkeypatch, "void0.0-cell0.25-r1.0" if eps == rs.GICP_EPSILON else f"void0.0-eps{eps:g}", storage)


@pytest.mark.parametrize("name", _ids(rs.large_cases()))
def test_gicp_large_coordinates(ab, monkeypatch, name):
    for storage in _gicp_case(name).storages:
        _run_gicp(ab, monkeypatch, name, storage)


@pytest.mark.parametrize("storage", rs.STORAGES)
def test_gicp_edge_normals(ab, monkeypatch, storage):
    """rs.gicp_edge_case as one record, then group by group through first / count (the groups are contiguous query ranges), so that a failure
    names the group.  On the library of the commit before write_record took the zero vector for e1 the whole record and the groups
    "tgt zero" and "src zero" FAIL (the closed form made their covariance I where Open3D's is diag(eps, 1, 1): terms off by 1e11 times
    the bound); every other group passed there."""
    c = _gicp_case("gicp-edge")
    _run_gicp(ab, monkeypatch, c.name, storage, ranges=[("all", 0, len(c.src))] + [g for g in c.groups if not g[0].endswith("zero")])


@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("group", ["tgt zero", "src zero"])
def test_gicp_edge_zero_normals(ab, monkeypatch, group, storage):
    """the zero-normal groups on their own (see test_gicp_edge_normals: these failed before the fix)"""
    c = _gicp_case("gicp-edge")
    _run_gicp(ab, monkeypatch, c.name, storage, ranges=[g for g in c.groups if g[0] == group])


@pytest.mark.parametrize("storage", rs.STORAGES)
def test_gicp_crop(ab, monkeypatch, storage):
    """CROPS[0] excludes every query's nearest points: the normal gathered is the one of the match the predicate leaves"""
    src, tgt, nrm = rs.void_cloud(rs.CROP_VOID)
    sn = rs.void_source_normals(rs.CROP_VOID)
    m = _crop_ref(0, storage)
    crop = backend.make_crop(**rs.CROPS[0])
    ses = harness.Session(ab[storage], src, tgt, nrm, 1.0, 0.25, src_nrm=sn)
    try:
        for path in PATHS:
            harness.set_path(path, monkeypatch)
            ses.begin(np.eye(4), path, crop=crop, method=backend.ICP_GENERALIZED)
            harness.check_record_gicp(ses.record(), m, tgt, nrm, sn, storage, np.eye(4), rs.GICP_EPSILON, 0, len(src), f"gicp crop0 {storage} {path}")
    finally:
        ses.close()
