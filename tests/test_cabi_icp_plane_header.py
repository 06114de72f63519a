"""CPU: include/gaussreg_hip_icp_plane.h -- PCA normals and point-to-plane ICP -- is read by the parser that reads
include/gaussreg_hip.h into _lib.ICP_PLANE_SIGNATURES, the library exports and binds what it declares, and the workspace
queries answer without a GPU.  The seven older headers and their tables stay as they were."""
import ctypes
import os
import re

from gaussreg_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PATH = os.path.join(ROOT, "include", "gaussreg_hip_icp_plane.h")
NAMES = ["gr_cloud_icp_plane", "gr_cloud_icp_plane_workspace_bytes", "gr_cloud_normals", "gr_cloud_normals_workspace_bytes"]
OLDER = (("gaussreg_hip.h", "SIGNATURES", 105), ("gaussreg_hip_train.h", "TRAIN_SIGNATURES", None),
         ("gaussreg_hip_train_matching.h", "MATCH_TRAIN_SIGNATURES", None),
         ("gaussreg_hip_train_backbone.h", "BACKBONE_TRAIN_SIGNATURES", None), ("gaussreg_hip_cloud.h", "CLOUD_SIGNATURES", 5),
         ("gaussreg_hip_icp.h", "ICP_SIGNATURES", 2), ("gaussreg_hip_feature_nn.h", "FEATURE_NN_SIGNATURES", 2))


def declared_symbols():               # as tests/test_cabi_symbols.py
    text = re.sub(r"/\*.*?\*/", "", open(PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", text)))


def test_parser_covers_the_header():
    sigs, defines = _lib.parse_header(open(PATH).read())
    assert sorted(sigs) == declared_symbols() == NAMES
    assert sigs == _lib.ICP_PLANE_SIGNATURES and defines == _lib.ICP_PLANE_DEFINES
    assert defines == {"GR_CLOUD_NORMALS_MAX_K": 64} and _lib.CLOUD_NORMALS_MAX_K == 64
    i64, f32, f64, ptr, i, sz = ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert sigs["gr_cloud_normals_workspace_bytes"] == (sz, [i64, i64, i])
    assert sigs["gr_cloud_normals"] == (i, [ptr, i64, ptr, i64, ptr, i, i, ptr, ptr, ptr, ptr, ptr, sz, ptr])
    assert sigs["gr_cloud_icp_plane_workspace_bytes"] == (sz, [i64, i64, i])
    # gr_cloud_icp's arguments with ref_normals after ref and without with_scale
    point = list(_lib.ICP_SIGNATURES["gr_cloud_icp"][1])
    assert sigs["gr_cloud_icp_plane"] == (i, point[:3] + [ptr] + point[3:6] + point[7:])
    assert sigs["gr_cloud_icp_plane"] == (i, [ptr, i64, ptr, ptr, i64, ptr, f32, i, f64, f64, ptr, ptr, ptr, ptr, ptr, ptr, ptr, sz, ptr])


def test_the_older_tables_are_untouched():
    new = set(_lib.ICP_PLANE_SIGNATURES)
    older_defines = {}
    for header, table, count in OLDER:
        text = open(os.path.join(ROOT, "include", header)).read()
        sigs, defines = _lib.parse_header(text)
        assert sigs == getattr(_lib, table) and defines == getattr(_lib, table.replace("SIGNATURES", "DEFINES")), header
        assert not new & set(sigs) and "gr_cloud_icp_plane" not in text and "gr_cloud_normals" not in text, header
        assert count is None or len(sigs) == count, (header, len(sigs))
        older_defines.update(defines)
    assert not [d for d in _lib.ICP_PLANE_DEFINES if d in older_defines]
    # the status codes are those of the point-to-point header, not redefined here
    assert "GR_CLOUD_ICP_DEGENERATE" in _lib.ICP_DEFINES and "GR_CLOUD_ICP_DEGENERATE" not in _lib.ICP_PLANE_DEFINES


def test_library_exports_every_declared_symbol_and_binds_it():
    from gaussreg_amd import build
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared_symbols():
        assert hasattr(raw, s), f"libgaussreg_hip.so does not export {s}"
    L = _lib.lib()
    for name, (res, args) in _lib.ICP_PLANE_SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name


def test_icp_plane_workspace_query_is_host_only_and_linear():
    ws = _lib.lib().gr_cloud_icp_plane_workspace_bytes
    for args in ((5, 0, 1), (-1, 5, 1), (5, 5, -1), (5, 5, 257), (2 ** 31, 5, 1), (5, 2 ** 31, 1)):   # what the call refuses
        assert ws(*args) == 0, args
    assert ws(0, 1, 0) > 0 and ws(5, 5, 256) > 0
    small, big = ws(1000, 1000, 30), ws(1_000_000, 1_000_000, 30)
    assert 16 * 2000 <= small and 16 * 2_000_000 <= big <= 64 * 2_000_000
    assert ws(1000, 1000, 0) == ws(1000, 1000, 256)                 # the rounds reuse the buffers
    assert ws(1000, 50_000, 1) < ws(50_000, 50_000, 1) and ws(50_000, 1000, 1) < ws(50_000, 50_000, 1)
    per_src = (ws(2_000_000, 1000, 1) - ws(1_000_000, 1000, 1)) / 1e6
    per_ref = (ws(1000, 2_000_000, 1) - ws(1000, 1_000_000, 1)) / 1e6
    assert 40 <= per_src <= 80 and 20 <= per_ref <= 40, (per_src, per_ref)
    # the point-to-point layout with rows of 29 instead of 18 partial sums: 11 doubles more per 2048 source points
    point = _lib.lib().gr_cloud_icp_workspace_bytes
    assert 0 <= ws(1_000_000, 1000, 1) - point(1_000_000, 1000, 1) <= 11 * 8 * 489 + 256


def test_normals_workspace_query_is_host_only():
    ws = _lib.lib().gr_cloud_normals_workspace_bytes
    for args in ((-1, 5, 8), (5, -1, 8), (5, 5, 0), (5, 5, 65), (2 ** 31, 5, 8), (5, 2 ** 31, 8)):   # what the call refuses
        assert ws(*args) == 0, args
    # nothing per point: the kernel keeps its sums in registers
    assert ws(0, 0, 1) == ws(5, 5, 64) == ws(1_000_000, 2_000_000, 8) == ws(2_000_000, 1_000_000, 8) > 0
