"""CPU: include/gaussreg_hip_cloud.h -- the cross-cloud nearest-neighbour entry points -- is read by the parser that reads
include/gaussreg_hip.h into _lib.CLOUD_SIGNATURES, the library exports and binds what it declares, and the workspace queries
answer without a GPU.  The four older headers and their tables stay as they were."""
import ctypes
import os
import re

from gaussreg_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PATH = os.path.join(ROOT, "include", "gaussreg_hip_cloud.h")
NAMES = ["gr_cloud_knn", "gr_cloud_knn_workspace_bytes", "gr_cloud_radius_count", "gr_cloud_radius_pairs",
         "gr_cloud_radius_workspace_bytes"]
OLDER = (("gaussreg_hip.h", "SIGNATURES", 105), ("gaussreg_hip_train.h", "TRAIN_SIGNATURES", None),
         ("gaussreg_hip_train_matching.h", "MATCH_TRAIN_SIGNATURES", None),
         ("gaussreg_hip_train_backbone.h", "BACKBONE_TRAIN_SIGNATURES", None))


def declared_symbols():               # as tests/test_cabi_symbols.py
    text = re.sub(r"/\*.*?\*/", "", open(PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", text)))


def test_parser_covers_the_header():
    sigs, defines = _lib.parse_header(open(PATH).read())
    assert sorted(sigs) == declared_symbols() == NAMES
    assert sigs == _lib.CLOUD_SIGNATURES and defines == _lib.CLOUD_DEFINES == {"GR_CLOUD_KNN_MAX_K": 8}
    assert _lib.CLOUD_KNN_MAX_K == 8
    i64, f32, ptr, i, sz = ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert sigs["gr_cloud_knn_workspace_bytes"] == (sz, [i64, i64, i])
    assert sigs["gr_cloud_knn"] == (i, [ptr, i64, ptr, i64, i, f32, ptr, ptr, ptr, sz, ptr])
    assert sigs["gr_cloud_radius_workspace_bytes"] == (sz, [i64, i64])
    assert sigs["gr_cloud_radius_count"] == (i, [ptr, i64, ptr, i64, f32, ptr, ptr, ptr, sz, ptr])
    assert sigs["gr_cloud_radius_pairs"] == (i, [ptr, i64, ptr, i64, f32, i64, ptr, ptr, ptr, sz, ptr])


def test_the_older_tables_are_untouched():
    new = set(_lib.CLOUD_SIGNATURES)
    for header, table, count in OLDER:
        text = open(os.path.join(ROOT, "include", header)).read()
        sigs, _ = _lib.parse_header(text)
        assert sigs == getattr(_lib, table), header
        assert not new & set(sigs) and "gr_cloud" not in text, header
        assert count is None or len(sigs) == count, (header, len(sigs))
    assert not [d for d in _lib.CLOUD_DEFINES if d in _lib.DEFINES]


def test_library_exports_every_declared_symbol_and_binds_it():
    from gaussreg_amd import build
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared_symbols():
        assert hasattr(raw, s), f"libgaussreg_hip.so does not export {s}"
    L = _lib.lib()
    for name, (res, args) in _lib.CLOUD_SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name


def test_workspace_queries_are_host_only():
    knn, radius = _lib.lib().gr_cloud_knn_workspace_bytes, _lib.lib().gr_cloud_radius_workspace_bytes
    for args in ((5, 0, 1), (-1, 5, 1), (5, 5, 0), (5, 5, 9), (2 ** 31, 5, 1), (5, 2 ** 31, 1)):   # what the call refuses
        assert knn(*args) == 0, args
    for args in ((5, 0), (-1, 5), (2 ** 31, 5), (5, 2 ** 31)):
        assert radius(*args) == 0, args
    assert knn(0, 1, 1) > 0 and radius(0, 1) > 0                    # no queries is a shape the call accepts
    # the grid over the support, both clouds in cell order (16 B a point), cells and lists: linear in both sizes
    small, big = knn(1000, 1000, 8), knn(1_000_000, 1_000_000, 8)
    assert 16 * 2000 <= small and 16 * 2_000_000 <= big <= 64 * 2_000_000
    assert knn(1000, 1000, 1) == knn(1000, 1000, 8)
    assert knn(1000, 50_000, 1) < knn(50_000, 50_000, 1) and knn(50_000, 1000, 1) < knn(50_000, 50_000, 1)
    assert radius(8192, 8192) >= 16 * 16384
