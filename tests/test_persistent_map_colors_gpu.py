"""Coloured submaps stay in the persistent form across insertions (map_kernels.hpp; needs an MI355X).

Every comparison is against the ARRAY form -- the same calls in a child process with the A/B library and O3DS_NO_PERSISTENT_MAP=1, the path
the golden and oracle tests hold to the reference -- and is byte for byte: points, normals and colours.  Every raw scan point gets a
colour of its own (frame, index); VoxelDownSample averages them per scan voxel, the frame channel (a dyadic number) stays exact, so
the winner of a map voxel -- its last member in cloud order -- cannot tie with another frame's."""
import numpy as np
import pytest

from child_process import run_child
from open3d_slam_amd import backend, synthetic as syn

pytestmark = pytest.mark.gpu

SCAN_VOXEL, MAP_VOXEL, RMAX, HINT = 0.1, 0.2, 12.0, 1.0


def _colours(k, n):  # unique per (frame, index) for n < 128 * 128
    i = np.arange(n)
    return np.stack([np.full(n, (k + 1) / 32.0), (i // 128) / 128.0, (i % 128) / 128.0], axis=1)


def _pose(k, n_frames):
    t = k if k < n_frames // 2 else n_frames - 1 - k  # out and back: the volume returns over what it left behind
    return syn.make_pose([1.5 * t, 0.4 * t, 0.0], [0.0, 0.0, 4.0 * t])


def _scan(be, scene, k, n_frames, coloured=True):
    """raw scan k and its pre-processed form: colours set on the raw scan before voxel_down_sample"""
    T = _pose(k, n_frames)
    raw = syn.vlp16_scan(scene, T, frame=k, n_az=256)
    s = be.upload(raw)
    if coloured:
        be.set_colors(s, _colours(k, len(raw)))
    v = be.voxel_down_sample(s, SCAN_VOXEL)
    be.estimate_normals(v, 2.0, 10)
    return T, s, v, backend.make_crop(backend.CROP_MIN_MAX_RADIUS, center=T[:3, 3], rmin=0.0, rmax=RMAX)


def _look(be, m):
    p, n = be.download(m)
    c = be.get_colors(m)
    return p.tobytes(), n.tobytes(), None if c is None else c.tobytes(), len(p)


def _coloured_sequence(be, n_frames, look_at, carve_at=(), carve_voxel=0.1):
    """test_preprocess_map_gpu._insert_sequence with coloured scans: the map at every look, and which form it was in after every
    insertion (asked before the look: looking folds)"""
    scene = syn.make_scene()
    m = be.upload(np.zeros((0, 3)))
    looks, form = [], []
    for k in range(n_frames):
        T, s, v, crop = _scan(be, scene, k, n_frames)
        if k in carve_at:
            be.map_carve(m, s, T, crop, voxel=carve_voxel)
        be.map_insert_scan(m, v, T, MAP_VOXEL, crop, max_corr_hint=HINT)
        form.append(be.is_persistent_map(m))
        if k in look_at:
            looks.append(_look(be, m))
        be.free(s)
        be.free(v)
    be.free(m)
    return dict(looks=looks, form=form)


def _other_cases(be, make_backend):
    """the += cases, the readers that fold, a registration: everything recorded, nothing asserted (it runs in both processes)"""
    scene = syn.make_scene()
    out = {}
    # ---- a coloured map, persistent; then an uncoloured scan (operator+= drops the map's colours), then two more
    n_frames = 8
    m = be.upload(np.zeros((0, 3)))
    form = []
    for k in range(n_frames):
        T, s, v, crop = _scan(be, scene, k, n_frames, coloured=k < 5)
        be.map_insert_scan(m, v, T, MAP_VOXEL, crop, max_corr_hint=HINT)
        form.append(be.is_persistent_map(m))
        if k == 4:
            out["coloured_before"] = be.has_colors(m)
        if k == 5:
            out["coloured_after_uncoloured_scan"] = be.has_colors(m)
            out["map_after_uncoloured_scan"] = _look(be, m)
        be.free(s)
        be.free(v)
    out["form_coloured_then_uncoloured"] = form
    out["map_after_two_more"] = _look(be, m)
    be.free(m)
    # ---- an uncoloured map, persistent; then coloured scans (their colours are ignored, as += drops them)
    m = be.upload(np.zeros((0, 3)))
    form, coloured = [], []
    for k in range(6):
        T, s, v, crop = _scan(be, scene, k, 6, coloured=k >= 3)
        be.map_insert_scan(m, v, T, MAP_VOXEL, crop, max_corr_hint=HINT)
        form.append(be.is_persistent_map(m))
        coloured.append(be.has_colors(m))
        be.free(s)
        be.free(v)
    out["form_uncoloured_then_coloured"], out["coloured_uncoloured_then_coloured"] = form, coloured
    out["map_uncoloured_then_coloured"] = _look(be, m)
    be.free(m)
    # ---- a coloured persistent map and its readers: each one after an insertion (the map is persistent again)
    n_frames = 12
    m = be.upload(np.zeros((0, 3)))
    be2 = make_backend()
    form = []
    for k in range(n_frames):
        T, s, v, crop = _scan(be, scene, k, n_frames)
        if k == 6:  # a registration against the coloured persistent map, after an insertion
            r = be.icp_point_to_plane_dev(v, m, 1.0, init=T, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
            out["registration"] = (np.asarray(r["transformation"]).tobytes(), r["fitness"], r["inlier_rmse"], r["iterations"])
            out["form_after_registration"] = be.is_persistent_map(m)
        be.map_insert_scan(m, v, T, MAP_VOXEL, crop, max_corr_hint=HINT)
        form.append(be.is_persistent_map(m))
        if k == 4:
            out["has_colors"] = be.has_colors(m)
            out["form_after_has_colors"] = be.is_persistent_map(m)
        if k == 3:
            moved = be.transform_cloud(m, syn.make_pose([0.3, -0.2, 0.1], [1.0, 2.0, 3.0]))
            out["transform_cloud"] = _look(be, moved)
            be.free(moved)
        if k == 7:
            copy = be2.copy_from(be, m)
            out["copy_across"] = _look(be2, copy)
            be2.free(copy)
        if k == 9:
            n_gone, gone = be.map_carve_removed(m, s, T, crop, voxel=MAP_VOXEL)
            c = be.get_colors(gone) if n_gone else None
            out["carve_removed"] = (n_gone, be.download(gone)[0].tobytes(), None if c is None else c.tobytes())
            be.free(gone)
            out["map_after_carve_removed"] = _look(be, m)
        be.free(s)
        be.free(v)
    out["form_readers"] = form
    out["map_at_the_end"] = _look(be, m)
    be.free(m)
    be2.close()
    return out


def _ab(prec):
    return backend.Backend(0, prec, ab=True)


def _in_child(call):
    """`call` (an expression over `t` = this module) in a child process with the array form at every insertion: the switch is read once
    per process, and only by the A/B library (t._ab)"""
    return run_child("test_persistent_map_colors_gpu", call, env=dict(O3DS_NO_PERSISTENT_MAP="1"),
                     timeout=300)[0]  # (a guard against a hang: no test of this module took more than 1.2 s on an MI355X)


_PREC = {"f64": backend.PRECISION_F64, "f32": backend.PRECISION_F32}
_CASES = {"look_rarely": dict(look_at=(3, 4, 11, 17, 23), carve_at=(14,)),  # (the carving voxel is not the map's: that carve folds)
          "never_until_the_end": dict(look_at=(23,)),
          "carved_in_place": dict(look_at=(5, 12, 23), carve_at=(8, 16), carve_voxel=MAP_VOXEL)}
_cache = {}


def _sequence_runs(prec, case):  # (got, ref) of one case: computed once, shared by the tests that look at it, left unchanged
    if (prec, case) not in _cache:
        ref = _in_child(f"t._coloured_sequence(t._ab({_PREC[prec]}), 24, **{_CASES[case]!r})")
        be = backend.Backend(0, _PREC[prec])
        got = _coloured_sequence(be, 24, **_CASES[case])
        be.close()
        _cache[(prec, case)] = (got, ref)
    return _cache[(prec, case)]


def _other_runs(prec):
    if prec not in _cache:
        ref = _in_child(f"t._other_cases(t._ab({_PREC[prec]}), lambda: t._ab({_PREC[prec]}))")
        be = backend.Backend(0, _PREC[prec])
        got = _other_cases(be, lambda: backend.Backend(0, _PREC[prec]))
        be.close()
        _cache[prec] = (got, ref)
    return _cache[prec]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("case", list(_CASES))
def test_coloured_persistent_map_is_bitwise_the_array_form(prec, case):
    """test_persistent_map_is_bitwise_the_array_form with coloured scans: 24 insertions out and back, scan voxel 0.1, map voxel 0.2,
    volume 12 m; points, normals and colours equal the array form's at every look."""
    got, ref = _sequence_runs(prec, case)
    assert [g[3] for g in got["looks"]] == [r[3] for r in ref["looks"]]
    for k, (g, r) in enumerate(zip(got["looks"], ref["looks"])):
        assert g[2] is not None and r[2] is not None, k
        assert g[0] == r[0] and g[1] == r[1], k
        assert g[2] == r[2], k
    assert got["looks"][-1][3] > 5000


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("case", list(_CASES))
def test_a_coloured_map_really_takes_the_persistent_form(prec, case):
    """from the third insertion on the coloured map is persistent after every insertion (a look or a folding carve in between only
    means the next insertion re-enters); with the switch that forces the array form it never is"""
    got, ref = _sequence_runs(prec, case)
    assert len(got["form"]) == 24 and all(got["form"][2:]), got["form"]
    assert len(ref["form"]) == 24 and not any(ref["form"]), ref["form"]


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_colours_follow_operator_plus_equals_across_the_forms(prec):
    got, ref = _other_runs(prec)
    # coloured persistent map, then one uncoloured scan: the colours go, as += drops them; two more uncoloured scans: persistent again
    assert got["coloured_before"] and got["form_coloured_then_uncoloured"][4]
    assert not got["coloured_after_uncoloured_scan"] and not ref["coloured_after_uncoloured_scan"]
    for key in ("map_after_uncoloured_scan", "map_after_two_more"):
        assert got[key][2] is None and ref[key][2] is None, key
        assert got[key][:2] == ref[key][:2] and got[key][3] == ref[key][3] > 1000, key
    assert got["form_coloured_then_uncoloured"][7], got["form_coloured_then_uncoloured"]
    # uncoloured persistent map, then coloured scans: stays persistent and uncoloured
    assert all(got["form_uncoloured_then_coloured"][2:]), got["form_uncoloured_then_coloured"]
    assert not any(got["coloured_uncoloured_then_coloured"]) and not any(ref["coloured_uncoloured_then_coloured"])
    assert got["map_uncoloured_then_coloured"] == ref["map_uncoloured_then_coloured"] and got["map_uncoloured_then_coloured"][3] > 1000
    assert not any(ref["form_coloured_then_uncoloured"]) and not any(ref["form_uncoloured_then_coloured"])


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_readers_of_a_coloured_persistent_map_see_the_folded_colours(prec):
    got, ref = _other_runs(prec)
    assert all(got["form_readers"][2:]) and not any(ref["form_readers"])  # (every reader below met a persistent map)
    assert got["has_colors"] and ref["has_colors"]
    assert got["form_after_has_colors"]  # has_colors does not fold
    for key in ("transform_cloud", "copy_across", "map_after_carve_removed", "map_at_the_end"):
        assert got[key][2] is not None, key
        assert got[key] == ref[key] and got[key][3] > 1000, key
    print("carved:", got["carve_removed"][0])
    assert got["carve_removed"] == ref["carve_removed"]  # (count, points and colours of the removed cloud)
    assert (got["carve_removed"][2] is not None) == (got["carve_removed"][0] > 0)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_registration_against_a_coloured_persistent_map_is_the_array_form_s(prec):
    """colours are not in the paged index: a registration against the coloured persistent map returns the bits it returns against
    the array form's index, and leaves the map persistent"""
    got, ref = _other_runs(prec)
    assert got["registration"] == ref["registration"], (got["registration"][1:], ref["registration"][1:])
    assert got["registration"][3] == 10 and got["registration"][1] > 0.5
    assert got["form_after_registration"] and not ref["form_after_registration"]
