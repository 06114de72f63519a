"""CPU: gr_node_correspondences and its workspace query are declared in include/gaussreg_hip_train_matching.h -- the two
older headers stay closed --, read by the header parser into _lib.MATCH_TRAIN_SIGNATURES, exported by the library and bound;
the workspace query answers without a GPU, is O(M N + N K) and returns 0 for the shapes the call refuses."""
import ctypes
import os

from gaussreg_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("gr_node_correspondences", "gr_node_correspondences_workspace_bytes")


def test_declared_in_the_matching_training_header_only():
    sigs, _ = _lib.parse_header(open(os.path.join(ROOT, "include", "gaussreg_hip_train_matching.h")).read())
    assert set(NAMES) <= set(sigs) and sigs == _lib.MATCH_TRAIN_SIGNATURES
    i64, f32, ptr, i, sz = ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert sigs["gr_node_correspondences_workspace_bytes"] == (sz, [i64, i64, i64])
    assert sigs["gr_node_correspondences"] == (i, [ptr] * 4 + [i64] * 3 + [ptr, f32] + [ptr] * 6 + [i64, ptr, ptr, ptr, sz, ptr])
    for header in ("gaussreg_hip.h", "gaussreg_hip_train.h"):
        assert "gr_node_correspondences" not in open(os.path.join(ROOT, "include", header)).read()
    assert not set(NAMES) & (set(_lib.SIGNATURES) | set(_lib.TRAIN_SIGNATURES))


def test_library_exports_and_binds_the_symbols():
    from gaussreg_amd import build
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(raw, name), f"libgaussreg_hip.so does not export {name}"
        res, args = _lib.MATCH_TRAIN_SIGNATURES[name]
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name


def test_workspace_query_is_host_only():
    q = _lib.lib().gr_node_correspondences_workspace_bytes
    for args in ((5, 5, 257), (-1, 5, 16), (5, -1, 16), (5, 5, -1), (1 << 16, 1 << 15, 16), (1 << 31, 1, 16)):   # refused shapes
        assert q(*args) == 0, args
    assert q(0, 0, 0) > 0 and q(5, 0, 16) > 0 and q(3, 3, 256) > 0
    # the (M, N) overlap matrix, the transformed source patches and a few words per node: no term in M * N * K or N * K * K
    M, N, K = 767, 767, 128
    floor = 4 * (M * N + 3 * N * K)
    assert floor <= q(M, N, K) <= floor + 64 * (M + N) + 16 * 256
    assert q(2 * M, N, K) - q(M, N, K) <= 4 * M * N + 64 * M + 4096
    assert q(M, N, 2 * K) - q(M, N, K) <= 12 * N * K + 4096
