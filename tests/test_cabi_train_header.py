"""CPU: include/gaussreg_hip_train.h -- the training entry points added after include/gaussreg_hip.h was closed -- is read
by the same parser into _lib.TRAIN_SIGNATURES, the library exports what it declares, and the host-only queries of the
structure embedding's backward answer without a GPU."""
import ctypes
import os
import re

from gaussreg_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PATH = os.path.join(ROOT, "include", "gaussreg_hip_train.h")


def declared_symbols():               # as tests/test_cabi_symbols.py
    text = re.sub(r"/\*.*?\*/", "", open(PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", text)))


def test_parser_covers_the_train_header():
    sigs, defines = _lib.parse_header(open(PATH).read())
    assert sorted(sigs) == declared_symbols() == ["gr_geo_embedding_backward", "gr_geo_embedding_backward_plan",
                                                  "gr_geo_embedding_backward_workspace_bytes"]
    assert sigs == _lib.TRAIN_SIGNATURES and defines == _lib.TRAIN_DEFINES
    i64, f32, ptr = ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    assert sigs["gr_geo_embedding_backward_workspace_bytes"] == (ctypes.c_size_t, [i64] * 3)
    assert sigs["gr_geo_embedding_backward_plan"] == (ctypes.c_int, [i64] * 3 + [ptr] * 3)
    assert sigs["gr_geo_embedding_backward"] == (ctypes.c_int, [ptr, i64, ptr, ptr, i64, f32, ptr, ptr, ptr, i64, f32, f32, i64,
                                                               ctypes.c_int, ctypes.c_int, ptr, ptr, ptr, ptr, ptr,
                                                               ctypes.c_size_t, ptr])


def test_the_old_header_and_its_tables_are_untouched():
    assert len(_lib.SIGNATURES) == 105 and not set(_lib.SIGNATURES) & set(_lib.TRAIN_SIGNATURES)
    old = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaussreg_hip.h")).read(), flags=re.S)
    assert "gr_geo_embedding_backward" not in old


def test_library_exports_every_declared_symbol_and_binds_it():
    from gaussreg_amd import build
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared_symbols():
        assert hasattr(raw, s), f"libgaussreg_hip.so does not export {s}"
    L = _lib.lib()
    for name, (res, args) in _lib.TRAIN_SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name


def _plan(n, c, k):
    slabs, pairs, tiles = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = _lib.lib().gr_geo_embedding_backward_plan(n, c, k, ctypes.byref(slabs), ctypes.byref(pairs), ctypes.byref(tiles))
    return rc, slabs.value, pairs.value, tiles.value


def test_workspace_and_plan_queries_are_host_only():
    L = _lib.lib()
    assert L.gr_geo_embedding_backward_workspace_bytes(767, 256, 3) > 0
    for n, c, k in ((24, 48, 3), (24, 64, 9), (3, 64, 3), (46341, 64, 3), (24, 64, -1)):      # 0: every shape the call refuses
        assert L.gr_geo_embedding_backward_workspace_bytes(n, c, k) == 0, (n, c, k)
    for n, c, k in ((45, 64, 3), (24, 256, 3), (45, 96, 3), (24, 64, 8), (24, 64, 0), (4, 64, 3), (767, 256, 3)):
        rc, slabs, pairs, tiles = _plan(n, c, k)
        assert rc == 0 and pairs % 32 == 0 and pairs > 0 and tiles == -(-c // 64)
        assert slabs == max(1, -(-n * n // pairs))                                 # the slabs cover the pairs, none is empty
        assert slabs > 1 or n * n <= 64                                            # never one slab for a whole cloud
        # the workspace holds the neighbour lists, two (c, c) partial tiles and c column sums per slab
        assert L.gr_geo_embedding_backward_workspace_bytes(n, c, k) >= n * max(k, 1) * 4 + slabs * (2 * c * c + c) * 4
    rc, slabs, pairs, _ = _plan(45, 64, 3)
    assert slabs >= 2 and (45 * 45) % pairs != 0                                   # several slabs, the last one ragged
    assert _plan(24, 256, 3)[3] > 1                                                # more than one c-tile
    # the multi-chunk case of tests/geo_embedding_grad_cases.py: a slab is more than one 128-pair chunk of indices, the last
    # chunk of a slab and the last slab are ragged
    rc, slabs, pairs, _ = _plan(128, 256, 3)
    assert rc == 0 and pairs > 128 and pairs % 128 != 0 and (128 * 128) % pairs != 0 and slabs > 1
    rc, slabs, pairs, _ = _plan(767, 256, 3)
    assert pairs <= 8192 and 2 * 256 <= slabs * 4 * 2 <= 4 * 256                   # short chains; 2 - 4 workgroups per CU
    # the same answer every time: the cut depends on the shapes only
    assert _plan(767, 256, 3) == _plan(767, 256, 3) and _plan(767, 256, 3)[1:3] == _plan(767, 256, 0)[1:3]


def test_plan_refuses_what_the_call_refuses():
    for n, c, k in ((24, 48, 3), (24, 64, 9), (3, 64, 3), (46341, 64, 3), (24, 0, 0)):
        assert _plan(n, c, k)[0] == _lib.DEFINES["GR_ERR_INVALID"], (n, c, k)
    assert b"angle_k" in _lib.lib().gr_last_error() or b"hidden_dim" in _lib.lib().gr_last_error()
