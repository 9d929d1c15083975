"""The premises of the voxel-Gaussian (NDT) tests, held on the restatement alone (tests/ndt_restatement.py; no device): the Gaussians and
the record against independent numpy formulations, the registration on the shifted room with the documented reason for the robust loss,
the edge cloud's counters, and the interface (struct sizes, the header's declarations, the Backend's methods)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ndt_restatement as nr  # noqa: E402
from ndt_restatement import F32, F64  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("o3ds_voxel_gaussians_create", "o3ds_voxel_gaussians_free", "o3ds_voxel_gaussians_info_get", "o3ds_voxel_gaussians_download",
             "o3ds_ndt_step", "o3ds_icp_ndt_dev")
METHODS = ("voxel_gaussians_create", "voxel_gaussians_free", "voxel_gaussians_info", "voxel_gaussians_download", "ndt_step", "icp_ndt")


def _rel(got, want) -> float:
    return float(np.abs(got - want).max() / np.abs(want).max())


def test_gaussians_against_numpy():
    """mean, covariance and information of every valid voxel of the shifted noisy room (f64 storage) against np.mean / np.cov and the
    inverse (np.linalg.inv) of the matrix np.linalg.eigh's clamped values rebuild.  Per voxel and quantity the difference is the largest
    |difference| over the largest |entry|.  Measured: 3.27e-15 (an information matrix: the clamped inverse carries the condition
    1 / ratio = 100); allowed: 16x that, 5.23e-14."""
    G = nr.reference_gaussians("room", True, F64)
    P = nr.target("room", True)
    k, ok = nr.voxel_coords(P, nr.VOXEL)
    assert ok.all() and G.info["n_skipped_points"] == 0 and G.info["n_voxels"] == len(G.keys) and G.info["n_valid"] == int(G.valid.sum())
    assert (np.diff(G.packed) > 0).all() and G.counts.sum() == len(P)
    assert G.info["n_valid"] >= 100 and G.info["n_flat"] == 0
    pk = nr.pack(k)
    worst = 0.0
    for v in np.flatnonzero(G.valid):
        members = P[pk == G.packed[v]]
        assert len(members) == G.counts[v] >= nr.MIN_POINTS and (nr.pack(G.keys[v].astype(np.int64)) == G.packed[v])
        C3 = np.cov(members.T)
        lam, V = np.linalg.eigh(C3)
        clamped = np.maximum(lam, nr.RATIO * lam[2])
        B = np.linalg.inv((V * clamped) @ V.T)
        worst = max(worst, _rel(G.mean[v], members.mean(axis=0)), _rel(nr.sym3(G.cov[v]), C3), _rel(nr.sym3(G.information[v]), B))
    print(f"gaussians against numpy: worst relative difference {worst:.3e} (recorded {nr.GAUSSIAN_REL_MEASURED}, bound {nr.GAUSSIAN_REL_TOL})")
    assert nr.GAUSSIAN_REL_TOL == 16 * nr.GAUSSIAN_REL_MEASURED
    assert worst <= nr.GAUSSIAN_REL_TOL
    assert (G.information[G.valid == 0] == 0).all()


@pytest.mark.parametrize("neighbourhood", nr.NEIGHBOURHOODS)
def test_record_against_the_dense_formulation(neighbourhood):
    """the record of 257 queries on the shifted noisy room (f64 storage) against J^T B J and J^T B e as matrix products in np.longdouble,
    every loss of the step cases.  Per term the difference is taken over the sum of the addends' absolute values.  Measured: 3.76e-16
    (neighbourhood 7; 2.13e-16 with 1); allowed: 16x that, 6.02e-15."""
    G = nr.reference_gaussians("room", True, F64)
    src, T = nr.source("room", True, 257), nr.step_pose("room")
    worst = 0.0
    for kind, k in nr.STEP_LOSSES:
        rec = nr.step_record(src, G, T, neighbourhood, kind, k, F64)
        want, scale = nr.dense_longdouble(src, G, T, neighbourhood, kind, k, F64)
        assert rec[28] == want[28] and rec[28] >= 200 and (rec[30:] == 0).all()
        worst = max(worst, float((np.abs(rec[:30] - want) / np.maximum(scale, 1e-300)).max()))
    print(f"record against the dense formulation, neighbourhood {neighbourhood}: worst {worst:.3e} "
          f"(recorded {nr.RECORD_REL_MEASURED}, bound {nr.RECORD_REL_TOL})")
    assert nr.RECORD_REL_TOL == 16 * nr.RECORD_REL_MEASURED
    assert worst <= nr.RECORD_REL_TOL


def test_the_record_is_the_gauss_newton_system():
    """[0..20] x = -[21..26] is the step of sum w e^T B e: with the L2 loss the record's gradient is the finite difference of [27]"""
    G = nr.reference_gaussians("room", True, F64)
    src, T = nr.source("room", True, 257), nr.step_pose("room")
    rec = nr.step_record(src, G, T, 1, nr.L2, 0.0, F64)
    h = 1e-6
    for c in range(6):
        x = np.zeros(6)
        x[c] = h
        up = nr.step_record(src, G, nr.cr.vector6_to_matrix4(x) @ T, 1, nr.L2, 0.0, F64)
        down = nr.step_record(src, G, nr.cr.vector6_to_matrix4(-x) @ T, 1, nr.L2, 0.0, F64)
        if up[28] != rec[28] or down[28] != rec[28]:
            continue  # (a query changed its voxel: the sum is not differentiable there)
        assert abs((up[27] - down[27]) / (2 * h) - 2.0 * rec[21 + c]) <= 1e-5 * max(1.0, abs(2.0 * rec[21 + c])), c


@pytest.mark.parametrize("noisy", nr.dr.VARIANTS)
def test_registration_on_the_shifted_room(noisy):
    """from 0.20 m off, 30 updates: the own voxel with L2 and the 7-neighbourhood with Cauchy(1) end within 5 mm and 5 mrad of the truth; the
    7-neighbourhood with L2 ends worse than with Cauchy -- the neighbours' Gaussians pull at full weight -- which is why the class's default
    carries the loss"""
    src = nr.source("room", noisy, nr.LOOP_N)
    errs = {}
    for nb, (kind, k) in ((1, (nr.L2, 0.0)), (7, (nr.CAUCHY, 1.0)), (7, (nr.L2, 0.0))):
        res = nr.reference_registration("room", noisy, nb, kind, k, F64)
        errs[(nb, kind)] = nr.pose_error(res["transformation"], "room", src)
        print(f"room noisy={noisy} neighbourhood {nb} {nr.LOSS_NAMES[kind]}: {1e3 * errs[(nb, kind)][0]:.2f} mm, {1e3 * errs[(nb, kind)][1]:.2f} mrad, "
              f"fitness {res['fitness']:.4f}, iterations {res['iterations']}")
    for key in ((1, nr.L2), (7, nr.CAUCHY)):
        assert errs[key][0] <= nr.POSE_TOL[0] and errs[key][1] <= nr.POSE_TOL[1], (key, errs[key])
    assert errs[(7, nr.L2)][0] > errs[(7, nr.CAUCHY)][0]


def test_the_edge_cloud_holds_its_cases():
    for st in nr.STORAGES:
        G = nr.voxel_gaussians(nr.edge_cloud(), nr.VOXEL, nr.MIN_POINTS, nr.RATIO, st)
        by_key = {tuple(k): v for v, k in enumerate(G.keys.tolist())}
        assert G.info["n_skipped_points"] == 5 and G.info["n_flat"] == 1
        short, enough = by_key[(0, 0, 0)], by_key[(2, 0, 0)]
        assert G.counts[short] == nr.MIN_POINTS - 1 and not G.valid[short] and G.counts[enough] == nr.MIN_POINTS and G.valid[enough]
        flat = by_key[(4, 2, 0)]
        assert G.counts[flat] == nr.MIN_POINTS + 1 and not G.valid[flat] and (G.cov[flat] == 0).all()
        line = by_key[(2, 4, 6)]
        lam = np.linalg.eigvalsh(np.linalg.inv(nr.sym3(G.information[line])))
        assert G.valid[line] and np.allclose(lam[:2], nr.RATIO * lam[2], rtol=1e-6)  # two clamped values
        for k in range(-3, 5):  # a point exactly on the face x = k * 0.5 belongs to voxel k
            assert (k, 6, 0) in by_key
        assert ((1 << 20) - 1, 0, 0) in by_key and (G.keys < 0).any()
        single = by_key[(0, 0, 10)]
        assert G.counts[single] == 1 and (G.cov[single] == 0).all() and not G.valid[single]
        assert G.info["n_valid"] == int(G.valid.sum()) >= 5


def test_struct_sizes():
    from open3d_slam_amd import backend
    assert C.sizeof(backend.VoxelGaussianParams) == 24 and C.sizeof(backend.VoxelGaussiansInfo) == 32 and C.sizeof(backend.RobustLoss) == 16


def test_the_header_declares_the_functions():
    text = open(os.path.join(ROOT, "include", "o3ds_backend.h")).read()
    from open3d_slam_amd import backend
    for name in FUNCTIONS:
        assert re.search(r"^int " + name + r"\(", text, re.M), name
        assert name in backend.SIGNATURES, name
    assert "o3ds_voxel_gaussian_params; /* 24 bytes */" in text and "o3ds_voxel_gaussians_info; /* 32 bytes */" in text


def test_the_backend_has_the_methods():
    from open3d_slam_amd import backend, cloud_registration as creg
    for name in METHODS:
        assert callable(getattr(backend.Backend, name, None)), name
    reg = creg.createNdt(creg.CloudRegistrationParameters(), 0.5)
    assert isinstance(reg, creg.RegistrationNdt) and reg.voxelSize_ == 0.5 and reg.neighbourhood_ == 7 and reg.kernel_ == creg.CauchyLoss(1.0)
    assert reg.minPoints_ == 6 and reg.minEigenvalueRatio_ == 0.01
