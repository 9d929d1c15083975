"""Colours on the persistent submap (open3d_slam_amd/csrc/map_kernels.hpp), on the CPU: the model of
test_persistent_map_model.py with one colour per slot and the reference's rule, held to the oracle; and the interface that tells which
form a map is in.

AccumulatedPoint::AddPoint ASSIGNS the colour (helpers.cpp:40-42) and isValidColor holds for every value (helpers.cpp:83-85), so a voxel
mean shows the colour of the LAST of its members in cloud order, and a point outside the volume passes through with its own.  The
persistent form walks a voxel's members in exactly that order -- old members in pm_view_key order, then the scan's points in scan order --
so the colour is one more attribute carried through the same walk: the last scan point's if the voxel received any, the last old member's
otherwise.  Every scan point gets a colour of its own (frame, index), so a wrong winner cannot tie with the right one."""
import os
import re

import numpy as np
import pytest

from test_persistent_map_model import RAW, PersistentMapModel, Slot, _scans, contains, mean_of, pack_key


class ColouredMapModel(PersistentMapModel):
    """PersistentMapModel with a colour per slot (self.col[s], beside self.slots[s]): PmDev::col"""

    def __init__(self, pts, nrm, col, n_pass, voxel):
        super().__init__(pts, nrm, n_pass, voxel)
        self.col = [list(c) for c in col]  # pm_enter_kernel: the base keeps the array's colours
        self.old_colour_wins = 0           # merges of several old members that no scan point joined: the last OLD member's colour stays

    def insert(self, scan_p, scan_n, scan_c, crop):  # PersistentMapModel.insert, and where the colour goes at every step of it
        t = len(self.hist)
        groups, outside = {}, []
        for i, p in enumerate(scan_p):
            if contains(crop, p):
                groups.setdefault(pack_key(p, self.inv), []).append(i)
            else:
                outside.append(i)
        old = {}
        for s, sl in enumerate(self.slots):
            if not sl.dead and contains(crop, sl.p):
                old.setdefault(pack_key(sl.p, self.inv), []).append(s)
        for key in sorted(set(groups) | set(old)):
            olds, idx = old.get(key, []), groups.get(key, [])
            if not idx and len(olds) == 1:  # alone and untouched: no colour work, as no point work
                sl = self.slots[olds[0]]
                _, sl.n = mean_of([sl.p], [sl.n])
                continue
            if len(olds) > 1:
                self.merges_of_several += 1
                self.walks += sum(1 for s in olds if not self.in_block(s, t - 1))
                olds = sorted(olds, key=lambda s: (self.view_key(s, t - 1), s))
                if not idx:
                    self.old_colour_wins += 1
            p, n = mean_of([self.slots[s].p for s in olds] + [scan_p[i] for i in idx], [self.slots[s].n for s in olds] + [scan_n[i] for i in idx])
            c = list(scan_c[idx[-1]]) if idx else list(self.col[olds[-1]])  # PmAcc: every add overwrites, the mean hands it out untouched
            if olds:
                target, ts = self.slots[olds[0]], olds[0]
                for s in olds[1:]:
                    self.slots[s].dead = True  # (its colour is never read again)
            else:
                target, ts = Slot(p, n, t, key), len(self.slots)
                self.slots.append(target)
                self.col.append(None)
            target.p, target.n, target.st, target.ok = p, n, t, key
            self.col[ts] = c  # pm_store
        for i in outside:  # a scan point outside the volume becomes a raw slot with its own colour (pm_misc_kernel)
            self.slots.append(Slot(scan_p[i], scan_n[i], t, RAW | i))
            self.col.append(list(scan_c[i]))
        self.hist.append(crop)

    def array(self):  # pm_exit_t: pm_permute_kernel permutes the colours with the points and the normals
        pts, nrm, n_pass = super().array()
        return pts, nrm, np.array([self.col[s] for s in self.order]).reshape(-1, 3), n_pass


def reference_step_colors(oracle, pts, nrm, col, scan_p, scan_n, scan_c, crop_abi, crop, voxel):
    """test_persistent_map_model.reference_step with colours: oracle.voxelize_within_volume_colors returns them in the order of
    voxelize_within_volume's output, so the same permutation brings all three into the array form's order"""
    cat_p, cat_n, cat_c = np.vstack([pts, scan_p]), np.vstack([nrm, scan_n]), np.vstack([col, scan_c])
    out_p, out_n, n_pass = oracle.voxelize_within_volume(cat_p, cat_n, voxel, crop_abi)
    out_c = oracle.voxelize_within_volume_colors(cat_p, cat_c, voxel, crop_abi)
    assert len(out_c) == len(out_p)
    inv = 1.0 / voxel
    keys, seen = [], set()
    for p in cat_p:
        if contains(crop, p):
            k = pack_key(p, inv)
            if k not in seen:
                seen.add(k)
                keys.append(k)
    assert len(keys) == len(out_p) - n_pass
    order = np.argsort(np.array(keys, dtype=np.uint64), kind="stable")
    put = lambda a: np.vstack([a[:n_pass], a[n_pass:][order]])  # noqa: E731
    return put(out_p), put(out_n), put(out_c), n_pass


def scan_colours(k, n):  # unique per (frame, point index): 251 and 7 are coprime, a scan has far fewer than 1757 points
    i = np.arange(n)
    return np.stack([np.full(n, k / 32.0), (i % 251) / 251.0, (i % 7) / 7.0], axis=1)


@pytest.mark.parametrize("rebase_at", [(), (5,), (2, 9)])
def test_the_coloured_persistent_form_is_the_reference_s_array(oracle, rebase_at):
    """The sequence of test_the_persistent_form_is_the_reference_s_array -- 16 insertions out and back, n_az 48, voxel 0.4 m, volume
    7 m -- with coloured scans: points, normals AND colours byte for byte the oracle's after every insertion.  The sequence has merges of
    several old members that no scan point joins (the last old member's colour wins): 185 of its 253 merges of several, in each case."""
    from oracle import pyoracle

    voxel, rmax = 0.4, 7.0
    scans = _scans(oracle, 16, 48)
    assert max(len(sp) for sp, _, _ in scans) < 251 * 7
    ref_p, ref_n, ref_c = np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3))
    model = None
    stats = {"merges_of_several": 0, "old_colour_wins": 0, "outside": 0, "dead": 0}
    for k, (sp, sn, T) in enumerate(scans):
        sc = scan_colours(k, len(sp))
        centre = [float(x) for x in T[:3, 3]]
        crop = (centre, 0.0, rmax)
        crop_abi = pyoracle.make_crop(pyoracle.CROP_MIN_MAX_RADIUS, center=centre, rmin=0.0, rmax=rmax)
        ref_p, ref_n, ref_c, ref_np = reference_step_colors(oracle, ref_p, ref_n, ref_c, sp, sn, sc, crop_abi, crop, voxel)
        if model is None or k in rebase_at:
            if model is None:
                model = ColouredMapModel(ref_p, ref_n, ref_c, ref_np, voxel)
                continue
            got = model.array()
            stats["merges_of_several"] += model.merges_of_several
            stats["old_colour_wins"] += model.old_colour_wins
            model = ColouredMapModel(*got, voxel)
        before = len(model.slots)
        model.insert([list(map(float, p)) for p in sp], [list(map(float, n)) for n in sn], [list(map(float, c)) for c in sc], crop)
        stats["outside"] += sum(1 for sl in model.slots[before:] if sl.ok & RAW)
        got_p, got_n, got_c, got_np = model.array()
        assert got_np == ref_np and len(got_p) == len(ref_p), (k, got_np, ref_np, len(got_p), len(ref_p))
        assert got_p.tobytes() == ref_p.tobytes(), k
        assert got_n.tobytes() == ref_n.tobytes(), k
        assert got_c.tobytes() == ref_c.tobytes(), k
    stats["merges_of_several"] += model.merges_of_several
    stats["old_colour_wins"] += model.old_colour_wins
    stats["dead"] = sum(1 for sl in model.slots if sl.dead)
    print(stats)
    assert stats["outside"] > 100 and stats["dead"] > 20 and stats["merges_of_several"] > 20, stats
    assert stats["old_colour_wins"] >= 1, stats
    assert len(np.unique(ref_c, axis=0)) > 0.9 * len(ref_c)  # (colours of many frames and points survive: nothing was blended or defaulted)


def test_is_persistent_map_is_declared_exported_and_bound():
    """o3ds_cloud_is_persistent_map: in the header, exported by the built library with the declared signature, bound in backend.py"""
    from open3d_slam_amd import backend

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "o3ds_backend.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+o3ds_cloud_is_persistent_map\s*\(\s*o3ds_handle\s+h\s*,\s*o3ds_cloud\s+c\s*,\s*int\s*\*\s*persistent\s*\)\s*;", txt)
    lib = backend.load()
    assert hasattr(lib, "o3ds_cloud_is_persistent_map")
    assert "o3ds_cloud_is_persistent_map" in backend.SIGNATURES
    assert callable(getattr(backend.Backend, "is_persistent_map"))
    # a sibling of o3ds_cloud_index_replica: status codes, no compute (a null handle is rejected before anything else)
    assert lib.o3ds_cloud_is_persistent_map(None, 1, None) == backend.ERR_BAD_HANDLE
