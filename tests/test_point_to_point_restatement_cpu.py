"""The premises of tests/test_point_to_point_update_gpu.py, without a device: the longdouble reference of
tests/point_to_point_restatement.py against the two existing Umeyama restatements, the catalogue's claims about itself (which cases single
out a rotation, where the thin slabs sit about the `tiny` switch, which pairs a correspondence pass finds), that the reference alone
stays inside every assertion the GPU test makes near the origin, and that the offset cases discriminate: the header's formula on absolute
coordinates (device_form with no pivot) misses the f64 parity tolerance there by more than ten times."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_ransac_restatement as rs  # noqa: E402
import point_to_point_restatement as pp  # noqa: E402
from oracle import np_oracle  # noqa: E402

CASES = pp.cases()
NAMES = list(CASES)
NEAR = [n for n in NAMES if pp.near_origin(CASES[n])]
COMPUTED = [n for n in NAMES if CASES[n]["radius"] is not None]


@pytest.fixture(scope="module")
def refs():
    return {n: pp.umeyama_reference(c["p"], c["q"]) for n, c in CASES.items()}


def test_catalogue_holds_the_sizes_and_the_cases():
    sizes = {len(c["p"]) for c in CASES.values()}
    assert {1, 2, 3, 4, 20, 129, 300} <= sizes, sizes
    for c in CASES.values():
        bits = 60 if c["name"].startswith("near_coplanar") else (44 if "1e-8" in c["name"] else 20)
        for a in (c["p"], c["q"]):
            assert np.array_equal(a * 2.0 ** bits, np.round(a * 2.0 ** bits)), c["name"]  # dyadic inputs
        assert np.max(np.abs(c["p"])) < 2.5e5 and (c["offset"] is not None or np.max(np.abs(np.r_[c["p"], c["q"]])) < 512.0)
    assert len(COMPUTED) >= 10 and any(CASES[n]["offset"] is not None for n in COMPUTED)


def test_reference_agrees_with_the_two_existing_restatements(refs):
    for n in NEAR:
        c, ref = CASES[n], refs[n]
        if not pp.is_unique(ref):
            continue
        a = np_oracle.umeyama_update(c["p"], c["q"], np.arange(len(c["p"])))
        b = rs.umeyama(c["p"], c["q"])
        assert ref["g"] >= 1e-2 * ref["sigma"][0], n  # (an f64 LAPACK SVD against longdouble holds 1e-12 where the gap is of sigma_1's size)
        assert np.max(np.abs(a - ref["T"])) <= 1e-12 and np.max(np.abs(b - ref["T"])) <= 1e-12, (n, np.max(np.abs(a - ref["T"])))


def test_uniqueness_is_what_each_case_was_built_for(refs):
    for n, c in CASES.items():
        ref = refs[n]
        print(n, "sigma", [float(x) for x in ref["sigma"]], "s", ref["s"], "g / sigma_1", float(ref["g"] / ref["sigma"][0]) if ref["sigma"][0] > 0 else 0.0)
        assert pp.is_unique(ref) == c["unique"], n
        R = ref["R"]
        assert np.max(np.abs(R.T @ R - np.eye(3))) < 1e-17 and abs(pp._det3(R) - 1) < 1e-17, n
    assert refs["reflection_300"]["s"] == -1.0 and refs["reflection_300"]["sigma"][1] > 1.5 * refs["reflection_300"]["sigma"][2]
    e = refs["reflection_equal_128"]
    assert e["s"] == -1.0 and e["g"] == 0.0 and e["sigma"][0] > 2 * e["sigma"][1]
    for n in ("isotropic_cube_exact_8", "isotropic_cube_3deg_8"):
        s = refs[n]["sigma"]
        assert (s[0] - s[2]) / s[0] < 1e-5 and refs[n]["s"] == 1.0, n
    s = refs["isotropic_pair_128"]["sigma"]
    assert s[0] == s[1] and s[1] > 2 * s[2]
    for n in ("coplanar_axis_300", "coplanar_tilted_300"):
        assert refs[n]["sigma"][2] <= 1e-19 * refs[n]["sigma"][0], n
    for tag in ("1e-13", "1e-14", "1e-15"):
        s = refs["near_coplanar_%s_200" % tag]["sigma"]
        assert 0.5 * float(tag) < s[2] / s[0] < 2.0 * float(tag), (tag, float(s[2] / s[0]))
    assert refs["collinear_20"]["sigma"][1] <= 1e-19 * refs["collinear_20"]["sigma"][0]
    assert refs["identical_20"]["sigma"][0] == 0.0
    for n, deg in (("generic_rot90_300", 90.0), ("generic_rot179.9_300", 179.9), ("generic_rot180_300", 180.0)):
        assert abs(np.degrees(pp.angle(refs[n]["R"], np.eye(3))) - deg) < 1e-5, n
    assert abs(pp.angle(refs["generic_rot1e-8_300"]["R"], np.eye(3)) - 1e-8) < 1e-12


@pytest.mark.parametrize("name", COMPUTED)
def test_a_pass_from_the_identity_finds_exactly_the_pairs(name):
    """brute force: every query's partner is the only target point within the case's radius (targets at the partner's own coordinates,
    the `identical` case, aside), decoys included, with a margin of a tenth of the radius"""
    c = CASES[name]
    tgt = np.vstack([c["q"], pp.decoys(c)])
    d = np.linalg.norm(c["p"][:, None, :] - tgt[None, :, :], axis=2)
    r = c["radius"]
    for i in range(len(c["p"])):
        same = np.all(tgt == c["q"][i], axis=1)
        assert d[i, i] < 0.9 * r, (name, i, d[i, i])
        assert np.all(d[i, ~same] > 1.1 * r), (name, i, np.min(d[i, ~same]))
    assert np.min(d[:, len(c["q"]):]) > 4.0 * r


def test_device_form_stays_inside_the_assertions_near_the_origin_and_sets_the_constant(refs):
    worst = 0.0
    for n in NEAR:
        c = CASES[n]
        assert np.array_equal(pp.pivot_of(c["p"][0]), np.zeros(3))
        got = pp.check_update(pp.device_form(pp.record_of(c["p"], c["q"])), c, refs[n])
        print(n, {k: v for k, v in got.items() if k != "case"})
        worst = max(worst, got.get("ratio", 0.0))
    print("largest angle / (B / K) of device_form near the origin:", worst, " K =", pp.K_BOUND)
    assert 3.0 * worst <= pp.K_BOUND


def test_the_offset_cases_tell_the_two_forms_apart(refs):
    """absolute coordinates (no pivot): the patch and the triangle miss the f64 parity tolerance by more than 10x (measured here: 31x and
    61x, and the same two figures on an MI355X before the record had a pivot); relative to the pivot the same formula passes every assertion at every offset"""
    for n in NAMES:
        c = CASES[n]
        if c["offset"] is None:
            continue
        T_abs = pp.device_form(pp.record_of(c["p"], c["q"]))
        miss = max(pp.angle(T_abs, refs[n]["R"]), pp.placement(T_abs, pp._T_ld(refs[n]), c["p"])) / pp.TOL_PARITY["f64"]
        print(n, "absolute form: parity missed by a factor", miss)
        if n in ("patch_20_offset", "triangle_3_offset"):
            assert c["envelope"] and miss >= 10.0, (n, miss)
        piv = pp.pivot_of(c["p"][0])
        assert np.max(np.abs(c["p"] - piv)) < 600.0
        got = pp.check_update(pp.device_form(pp.record_of(c["p"], c["q"], piv), piv), c, refs[n], pivot=piv)
        print(n, "pivot", piv, {k: v for k, v in got.items() if k != "case"})


def test_ransac_draws_are_seldom_exempt():
    """the share of this seed's draws whose rotation the reference does not single out (a repeated or collinear sample): 6 of 512, 1.2 %,
    under the 5 % cap that keeps the GPU test from hiding a failure behind the exemption"""
    P, N, Q, NQ = pp.ransac_clouds()
    m = len(P)  # the copy's features are the cloud's: the mutual filter keeps i <-> i (the GPU test asserts the share on the pairs it gets)
    exempt = 0
    for t in range(pp.RANSAC_ITER):
        smp = rs.draw(pp.RANSAC_SEED, pp.RANSAC_N, t, m)
        exempt += not pp.is_unique(pp.umeyama_reference(P[smp], Q[smp]))
    print("exempt", exempt, "of", pp.RANSAC_ITER)
    assert exempt <= 0.05 * pp.RANSAC_ITER
