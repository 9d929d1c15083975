"""C-ABI checks that need no GPU: the library loads, exports every symbol include/o3ds_backend.h
declares, and reports errors through status codes (no compute calls)."""
import ctypes as C
import os
import re

import pytest

from open3d_slam_amd import backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "o3ds_backend.h")


def _declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(o3ds_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_all_exported_and_bound():
    names = _declared()
    assert len(names) >= 25
    lib = backend.load()
    for n in names:
        assert hasattr(lib, n), f"{n} declared in o3ds_backend.h but not exported"
    assert sorted(backend.SIGNATURES) == names, set(names) ^ set(backend.SIGNATURES)


def test_header_is_plain_c():
    import subprocess
    import tempfile

    with tempfile.NamedTemporaryFile("w", suffix=".c", delete=False) as f:
        f.write(f'#include "{HEADER}"\nint main(void){{ o3ds_icp_params p; p.max_iteration = 1; return sizeof(o3ds_icp_result) == 160 ? p.max_iteration - 1 : 1; }}\n')
    exe = f.name + ".out"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-o", exe, f.name])
    assert subprocess.call([exe]) == 0
    os.unlink(f.name)
    os.unlink(exe)


def test_struct_layouts_match_header():
    assert C.sizeof(backend.IcpResult) == 16 * 8 + 8 + 8 + 4 + 4 + 8
    assert C.sizeof(backend.IcpParams) == 8 + 4 + 4 + 8 + 8
    assert C.sizeof(backend.Crop) == 4 + 4 + 24 + 16 + 16


def test_null_handle_is_rejected_without_gpu():
    lib = backend.load()
    assert lib.o3ds_synchronize(None) == backend.ERR_BAD_HANDLE
    assert lib.o3ds_cloud_free(None, 1) == backend.ERR_BAD_HANDLE
    assert b"null handle" in lib.o3ds_last_error(None)
    assert b"gfx950" in lib.o3ds_version()


def test_create_fails_loudly_without_device():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(backend.BackendError) as e:
        backend.Backend(0)
    assert e.value.code == backend.ERR_HIP


def test_no_product_import_of_oracle():
    """The product package must never import/call the oracle (tier rule 3)."""
    pkg = os.path.join(ROOT, "open3d_slam_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert "pyoracle" not in txt and "np_oracle" not in txt and "o3d_oracle" not in txt, os.path.join(dp, f)


def test_no_hand_written_kernel_spills_registers():
    """Every kernel of this backend keeps its working set in registers (scratch 0).  Not a performance nicety: the compiler places VGPR
    spill stores inside divergent regions and reloads them under a wider EXEC mask, which in round 4 handed lanes a garbage quantum for
    the exact record sums (f64-storage fused kernel, 32 bytes of scratch) -- wrong poses, not slow ones.  The build records the
    compiler's own resource remarks; rocPRIM's library kernels are not ours to hold to this."""
    from open3d_slam_amd import build

    if not os.path.exists(build.RESOURCES):
        build.build_backend(force=True)
    res = build.kernel_resources()
    ours = {k: v for k, v in res.items() if "4o3ds" in k and "rocprim" not in k}
    assert len(ours) > 100, len(ours)
    spilling = {k: v["scratch"] for k, v in ours.items() if v["scratch"] != 0}
    assert not spilling, spilling
    fused = [v for k, v in ours.items() if "icp_fused_kernel" in k]
    assert len(fused) == 8 and all(v["vgpr"] <= 128 and v["occupancy"] >= 4 for v in fused), fused


def test_no_kernel_reads_a_word_through_the_scalar_cache_that_it_overwrites_while_the_load_is_in_flight():
    """A uniform plain load compiles to a scalar-cache load that is only waited for where its value is first used, and the hardware does
    not order it against the wavefront's later vector STORE to the same address: pm_carve_finish_kernel read the counter it was about to
    reset as the zero of its own reset, once in ten cold starts (round 5; the carve then reported nothing removed).  Such words are read
    with load_then_store (common.hpp); scripts/check_scalar_war.py looks for the pattern in the gfx950 assembly of every kernel."""
    import importlib.util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("check_scalar_war", os.path.join(root, "scripts", "check_scalar_war.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    # the checker finds the pattern where it is (the code the round-5 kernel compiled to) ...
    seen = mod.check("_Z3foov:\n\ts_load_dwordx4 s[12:15], s[10:11], 0x2c\n\tglobal_store_dword v0, v0, s[10:11] offset:48\n\ts_waitcnt lgkmcnt(0)\n\ts_endpgm\n")
    assert len(seen) == 1
    assert not mod.check("_Z3foov:\n\ts_load_dwordx4 s[12:15], s[10:11], 0x2c\n\ts_waitcnt lgkmcnt(0)\n\tglobal_store_dword v0, v0, s[10:11] offset:48\n\ts_endpgm\n")
    # ... and nowhere in the backend
    text = mod.assembly()
    assert text.count("s_endpgm") > 300
    assert mod.check(text) == []


def test_poses_cross_the_ctypes_boundary_column_major_and_unchanged():
    """The Python side hands 4x4 poses to the library as 16 doubles in column-major order (Eigen's layout, o3ds_backend.h) and reads
    results back the same way.  The marshalling takes short cuts (one `ravel(order="F")`, a ctypes array over the buffer instead of
    `ndarray.ctypes.data_as`, a constant identity, a view for the way back): every path must deliver the same doubles."""
    import numpy as np

    rng = np.random.default_rng(3)
    T = rng.normal(size=(4, 4))
    want = [T[r, c] for c in range(4) for r in range(4)]
    for src in (T, np.asfortranarray(T), T.astype(np.float32).astype(np.float64), T[::1], [list(r) for r in T]):
        flat = backend.colmajor(src)
        assert flat.flags["C_CONTIGUOUS"] and flat.dtype == np.float64 and flat.shape == (16,)
        ref = [np.asarray(src, dtype=np.float64)[r, c] for c in range(4) for r in range(4)]
        assert list(flat) == ref
        keep, ptr = backend._d(flat)
        assert [ptr[i] for i in range(16)] == ref
    assert list(backend.colmajor(T)) == want
    ro = backend.colmajor(T)
    ro.flags.writeable = False  # read-only arrays take the slower pointer path
    keep, ptr = backend._d(ro)
    assert [ptr[i] for i in range(16)] == want
    big = rng.normal(size=(1000, 3))  # large arrays are passed in place, not copied
    keep, ptr = backend._d(big)
    assert keep is big and [ptr[i] for i in range(6)] == list(big.ravel()[:6])
    keep, ptr = backend._d(np.zeros((0, 3)))
    assert ptr is not None and keep.shape == (0, 3)  # the ABI reads NULL as "absent": empty clouds get a placeholder
    assert backend._d(None) == (None, None)
    assert [backend._IDENTITY16[i] for i in range(16)] == [1.0 if i % 5 == 0 else 0.0 for i in range(16)]
    res = backend.IcpResult()
    for i, v in enumerate(want):
        res.transformation[i] = v
    back = backend.from_colmajor(res.transformation)
    assert back.flags["C_CONTIGUOUS"] and back.flags["OWNDATA"]
    np.testing.assert_array_equal(back, T)
    res.transformation[0] = 123.0  # the result is a copy, not a view of the struct
    assert back[0, 0] == T[0, 0]


def test_the_shipped_library_reads_no_ab_switch_from_the_environment():
    """A drop-in library's results and code paths must not depend on the environment of the process that loads it: the A/B levers,
    tuning knobs and debugging aids (O3DS_ICP_MODE, O3DS_ICP_SETS, O3DS_SUM_NO_SPLIT, O3DS_VOXEL_SORT, ...) are compiled into
    lib/libo3ds_backend_ab.so only (-DO3DS_AB_SWITCHES, loaded with Backend(..., ab=True)); the shipped library knows two names, both
    memory sizing.  Checked on the binaries: the names a library can look up are the string constants it holds."""
    from open3d_slam_amd import build

    def names(path):
        return set(m.decode() for m in re.findall(rb"O3DS_[A-Z][A-Z0-9_]+", open(path, "rb").read()))

    shipped, ab = names(build.LIB), names(build.LIB_AB)
    # (O3DS_ICP_PASS_MAX_QUERIES, O3DS_ICP_SUMS_DOUBLES: error texts quoting the header's constants; O3DS_RCCL_LIB: WHICH librccl.so file a multi-GPU process
    # loads -- a deployment choice like the two memory sizes, no effect on results or code paths)
    allowed = {"O3DS_POOL_CAP_MB", "O3DS_ARENA_MB", "O3DS_ICP_PASS_MAX_QUERIES", "O3DS_ICP_SUMS_DOUBLES", "O3DS_RCCL_LIB"}
    assert shipped <= allowed, shipped - allowed
    assert {"O3DS_ICP_MODE", "O3DS_ICP_SETS", "O3DS_SUM_NO_SPLIT", "O3DS_VOXEL_SORT", "O3DS_CARVE_SORT", "O3DS_MERGE_LIBRARY_SORT"} <= ab
    assert b"A/B switches" in backend.load(ab=True).o3ds_version() and b"A/B switches" not in backend.load().o3ds_version()


def test_the_ab_library_reads_the_declared_switches_and_no_other():
    """The inventory of the A/B library's levers: the O3DS_ names it holds, less the five the shipped library may hold and less the enum
    and macro spellings of include/o3ds_backend.h that error texts quote, are exactly the list below.  A lever that was removed and
    comes back, or a new one nobody declared here, fails."""
    from open3d_slam_amd import build

    def names(text):
        return set(m.decode() for m in re.findall(rb"O3DS_[A-Z0-9_]+", text))

    shipped_may_hold = {"O3DS_POOL_CAP_MB", "O3DS_ARENA_MB", "O3DS_ICP_PASS_MAX_QUERIES", "O3DS_ICP_SUMS_DOUBLES", "O3DS_RCCL_LIB"}
    levers = names(open(build.LIB_AB, "rb").read()) - shipped_may_hold - names(open(HEADER, "rb").read())
    assert levers == {
        # the registration: form of the loop, candidate sets, launch geometry, instrumentation
        "O3DS_ICP_MODE", "O3DS_ICP_SETS", "O3DS_SET_GAIN", "O3DS_SET_MIN", "O3DS_SET_CAP", "O3DS_PASS_ROWS", "O3DS_SUM_NO_SPLIT",
        "O3DS_DEBUG_ACC", "O3DS_DEBUG_UPDATE", "O3DS_ICP_STATS", "O3DS_FUSED_TRACE", "O3DS_FUSED_TRACE_LAUNCH",
        # the search index: replica, the scan loop's slack
        "O3DS_NN_REPLICA", "O3DS_NN_REPLICA_AFTER", "O3DS_SCAN_SPACE_BYTES", "O3DS_NO_SCAN_SLACK",
        # pre-processing and the map: sorting forms, the persistent map, the draw list
        "O3DS_VOXEL_SORT", "O3DS_CARVE_SORT", "O3DS_MERGE_LIBRARY_SORT", "O3DS_SORT_WAYS", "O3DS_NO_INCREMENTAL_MERGE",
        "O3DS_NO_PERSISTENT_MAP", "O3DS_DRAW_LIST_CAP",
        # place recognition
        "O3DS_RANSAC_BATCH",
    }, levers
