"""CPU: include/gaussreg_hip_gicp.h -- generalised ICP and its covariance kernels -- is read by the parser that reads
include/gaussreg_hip.h into _lib.GICP_SIGNATURES, the library exports and binds what it declares, and the workspace query
answers without a GPU.  The eight older headers and their tables stay as they were."""
import ctypes
import os
import re

from gaussreg_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PATH = os.path.join(ROOT, "include", "gaussreg_hip_gicp.h")
NAMES = ["gr_cloud_covariances_from_normals", "gr_cloud_gicp", "gr_cloud_gicp_workspace_bytes", "gr_gs_covariances"]
OLDER = (("gaussreg_hip.h", "SIGNATURES", 105), ("gaussreg_hip_train.h", "TRAIN_SIGNATURES", None),
         ("gaussreg_hip_train_matching.h", "MATCH_TRAIN_SIGNATURES", None),
         ("gaussreg_hip_train_backbone.h", "BACKBONE_TRAIN_SIGNATURES", None), ("gaussreg_hip_cloud.h", "CLOUD_SIGNATURES", 5),
         ("gaussreg_hip_icp.h", "ICP_SIGNATURES", 2), ("gaussreg_hip_feature_nn.h", "FEATURE_NN_SIGNATURES", 2),
         ("gaussreg_hip_icp_plane.h", "ICP_PLANE_SIGNATURES", 4))


def declared_symbols():               # as tests/test_cabi_symbols.py
    text = re.sub(r"/\*.*?\*/", "", open(PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", text)))


def test_parser_covers_the_header():
    sigs, defines = _lib.parse_header(open(PATH).read())
    assert sorted(sigs) == declared_symbols() == NAMES
    assert sigs == _lib.GICP_SIGNATURES and defines == _lib.GICP_DEFINES
    assert defines == {"GR_GS_COV_RAW": 0, "GR_GS_COV_PLANE": 1} and (_lib.GS_COV_RAW, _lib.GS_COV_PLANE) == (0, 1)
    i64, f32, f64, ptr, i, sz = ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert sigs["gr_cloud_gicp_workspace_bytes"] == (sz, [i64, i64, i])
    # gr_cloud_icp_plane's arguments with src_cov after n_src and ref_cov in place of ref_normals
    plane = list(_lib.ICP_PLANE_SIGNATURES["gr_cloud_icp_plane"][1])
    assert sigs["gr_cloud_gicp"] == (i, plane[:2] + [ptr] + plane[2:])
    assert sigs["gr_cloud_gicp"] == (i, [ptr, i64, ptr, ptr, ptr, i64, ptr, f32, i, f64, f64, ptr, ptr, ptr, ptr, ptr, ptr, ptr, sz, ptr])
    assert sigs["gr_cloud_covariances_from_normals"] == (i, [ptr, i64, f64, ptr, ptr, sz, ptr])
    assert sigs["gr_gs_covariances"] == (i, [ptr, ptr, i64, f32, i, f64, ptr, ptr, ptr, ptr, sz, ptr])


def test_the_older_tables_are_untouched():
    new = set(_lib.GICP_SIGNATURES)
    older_defines = {}
    for header, table, count in OLDER:
        text = open(os.path.join(ROOT, "include", header)).read()
        sigs, defines = _lib.parse_header(text)
        assert sigs == getattr(_lib, table) and defines == getattr(_lib, table.replace("SIGNATURES", "DEFINES")), header
        assert not new & set(sigs) and "gicp" not in text and "covariances" not in text, header
        assert count is None or len(sigs) == count, (header, len(sigs))
        older_defines.update(defines)
    assert not [d for d in _lib.GICP_DEFINES if d in older_defines]
    # the status codes are those of the point-to-point header, not redefined here
    assert "GR_CLOUD_ICP_DEGENERATE" in _lib.ICP_DEFINES and "GR_CLOUD_ICP_DEGENERATE" not in _lib.GICP_DEFINES


def test_library_exports_every_declared_symbol_and_binds_it():
    from gaussreg_amd import build
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared_symbols():
        assert hasattr(raw, s), f"libgaussreg_hip.so does not export {s}"
    L = _lib.lib()
    for name, (res, args) in _lib.GICP_SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name


def test_gicp_workspace_query_is_host_only_and_linear():
    ws = _lib.lib().gr_cloud_gicp_workspace_bytes
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
    # linear in both counts: the second difference of steps of 20 to 60 MB stays within 1 MiB -- the alignment of the carved
    # buffers and the cell table of the grid, whose dimension is a step function of n_ref
    for grow in (lambda k: (k * 1_000_000, 1000), lambda k: (1000, k * 1_000_000)):
        assert abs((ws(*grow(3), 1) - ws(*grow(2), 1)) - (ws(*grow(2), 1) - ws(*grow(1), 1))) <= 1 << 20
    # the source covariances are read through the original index, so nothing is carved for them: point-to-plane's layout
    plane = _lib.lib().gr_cloud_icp_plane_workspace_bytes
    for shape in ((1000, 1000, 30), (1_000_000, 1000, 1), (1000, 1_000_000, 1), (4097, 8317, 6)):
        assert ws(*shape) == plane(*shape), shape
