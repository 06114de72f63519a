"""CPU: include/gaussreg_hip_feature_nn.h -- nearest neighbours in feature space -- is read by the parser that reads
include/gaussreg_hip.h into _lib.FEATURE_NN_SIGNATURES, the library exports and binds what it declares, and the workspace
query answers without a GPU and is linear in n + m.  The six older headers and their tables stay as they were."""
import ctypes
import os
import re

from gaussreg_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PATH = os.path.join(ROOT, "include", "gaussreg_hip_feature_nn.h")
NAMES = ["gr_feature_nn", "gr_feature_nn_workspace_bytes"]
OLDER = (("gaussreg_hip.h", "SIGNATURES", 105), ("gaussreg_hip_train.h", "TRAIN_SIGNATURES", None),
         ("gaussreg_hip_train_matching.h", "MATCH_TRAIN_SIGNATURES", None),
         ("gaussreg_hip_train_backbone.h", "BACKBONE_TRAIN_SIGNATURES", None), ("gaussreg_hip_cloud.h", "CLOUD_SIGNATURES", 5),
         ("gaussreg_hip_icp.h", "ICP_SIGNATURES", 2))


def declared_symbols():               # as tests/test_cabi_symbols.py
    text = re.sub(r"/\*.*?\*/", "", open(PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", text)))


def test_parser_covers_the_header():
    sigs, defines = _lib.parse_header(open(PATH).read())
    assert sorted(sigs) == declared_symbols() == NAMES
    assert sigs == _lib.FEATURE_NN_SIGNATURES and defines == _lib.FEATURE_NN_DEFINES
    assert defines == {"GR_FEATURE_NN_MAX_C": 65536, "GR_FEATURE_NN_WORKSPACE_CAP": 4096}
    assert _lib.FEATURE_NN_MAX_C == 65536
    i64, ptr, i, sz = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert sigs["gr_feature_nn_workspace_bytes"] == (sz, [i64, i64, i64])
    assert sigs["gr_feature_nn"] == (i, [ptr, i64, ptr, i64, i64, i, ptr, ptr, ptr, ptr, ptr, sz, ptr])


def test_the_older_tables_are_untouched():
    new = set(_lib.FEATURE_NN_SIGNATURES)
    for header, table, count in OLDER:
        text = open(os.path.join(ROOT, "include", header)).read()
        sigs, _ = _lib.parse_header(text)
        assert sigs == getattr(_lib, table), header
        assert not new & set(sigs) and "gr_feature_nn" not in text, header
        assert count is None or len(sigs) == count, (header, len(sigs))
    older_defines = [_lib.DEFINES, _lib.TRAIN_DEFINES, _lib.MATCH_TRAIN_DEFINES, _lib.BACKBONE_TRAIN_DEFINES, _lib.CLOUD_DEFINES,
                     _lib.ICP_DEFINES]
    assert not [d for d in _lib.FEATURE_NN_DEFINES if any(d in table for table in older_defines)]


def test_library_exports_every_declared_symbol_and_binds_it():
    from gaussreg_amd import build
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared_symbols():
        assert hasattr(raw, s), f"libgaussreg_hip.so does not export {s}"
    L = _lib.lib()
    for name, (res, args) in _lib.FEATURE_NN_SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name


def test_workspace_query_is_host_only_and_linear():
    ws = _lib.lib().gr_feature_nn_workspace_bytes
    cap = _lib.FEATURE_NN_DEFINES["GR_FEATURE_NN_WORKSPACE_CAP"]
    for args in ((-1, 5, 8), (5, -1, 8), (5, 5, 0), (5, 5, -3), (5, 5, 65537), (2 ** 31, 5, 8), (5, 2 ** 31, 8),
                 (2 ** 31 - 128, 5, 8)):                                        # what the call refuses
        assert ws(*args) == 0, args
    assert ws(0, 0, 1) > 0 and ws(0, 7, 3) > 0 and ws(7, 0, 3) > 0 and ws(2 ** 31 - 129, 5, 65536) > 0
    # keys (8 B) and squared norms (4 B) per row of either input: nothing per pair, per (row, column tile) or per channel
    n = m = 200_000
    assert 12 * (n + m) <= ws(n, m, 256) <= 12 * (n + m) + cap < 16 * (n + m) + cap
    assert ws(n, m, 256) == ws(n, m, 1) == ws(n, m, 65536)
    for a, b in ((1, 1), (1000, 3), (3, 1000), (12345, 54321), (2_000_000, 1_000_000)):
        assert 12 * (a + b) <= ws(a, b, 32) <= 12 * (a + b) + cap, (a, b)
    steps = {ws(2 * k, other, 32) - ws(k, other, 32) for k in (1024, 65536) for other in (0, 1, 1000, 3_000_000)}
    assert steps == {12 * 1024, 12 * 65536}                                    # ws(2n, m) - ws(n, m) does not depend on m
    steps = {ws(other, 2 * k, 32) - ws(other, k, 32) for k in (1024, 65536) for other in (0, 1, 1000, 3_000_000)}
    assert steps == {12 * 1024, 12 * 65536}
