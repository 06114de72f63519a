"""CPU: include/gaussreg_hip_train_matching.h -- the training entry points of the matching stage -- is read by the parser
that reads include/gaussreg_hip.h into _lib.MATCH_TRAIN_SIGNATURES, the library exports and binds what it declares, and the
workspace query of the Sinkhorn backward answers without a GPU.  The two older headers and their tables stay as they were."""
import ctypes
import os
import re

from gaussreg_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PATH = os.path.join(ROOT, "include", "gaussreg_hip_train_matching.h")


def declared_symbols():               # as tests/test_cabi_symbols.py
    text = re.sub(r"/\*.*?\*/", "", open(PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", text)))


def test_parser_covers_the_header():
    sigs, defines = _lib.parse_header(open(PATH).read())
    assert sorted(sigs) == declared_symbols()
    assert {"gr_sinkhorn_backward", "gr_sinkhorn_backward_workspace_bytes"} <= set(sigs)
    assert sigs == _lib.MATCH_TRAIN_SIGNATURES and defines == _lib.MATCH_TRAIN_DEFINES
    i64, f32, ptr, i = ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_int
    assert sigs["gr_sinkhorn_backward_workspace_bytes"] == (ctypes.c_size_t, [i64, i64, i64, i])
    assert sigs["gr_sinkhorn_backward"] == (i, [ptr, i64, i64, i64, ptr, ptr, ptr, i, f32, i, ptr, ptr, ptr, ptr,
                                                ctypes.c_size_t, ptr])


def test_the_older_tables_are_untouched():
    new = set(_lib.MATCH_TRAIN_SIGNATURES)
    assert not new & set(_lib.SIGNATURES) and not new & set(_lib.TRAIN_SIGNATURES)
    for header in ("gaussreg_hip.h", "gaussreg_hip_train.h"):
        assert "gr_sinkhorn_backward" not in open(os.path.join(ROOT, "include", header)).read()


def test_library_exports_every_declared_symbol_and_binds_it():
    from gaussreg_amd import build
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared_symbols():
        assert hasattr(raw, s), f"libgaussreg_hip.so does not export {s}"
    L = _lib.lib()
    for name, (res, args) in _lib.MATCH_TRAIN_SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name


def test_workspace_query_is_host_only():
    q = _lib.lib().gr_sinkhorn_backward_workspace_bytes
    for args in ((2, 144, 5, 10), (2, 5, 144, 10), (2, 0, 5, 10), (2, 5, 5, -1), (-1, 5, 5, 10)):   # what the call refuses
        assert q(*args) == 0, args
    # a history slot per workgroup, u^t and v^t of every iteration: bounded by the grid, not by the batch
    assert q(1, 128, 128, 100) >= 4 * 100 * 258
    assert q(512, 128, 128, 100) == q(100000, 128, 128, 100) <= 512 * (4 * 100 * 258 + 256) + 256
    assert q(4, 128, 128, 100) < q(8, 128, 128, 100)
    assert q(7, 9, 9, 0) > 0 and q(0, 9, 9, 5) > 0
