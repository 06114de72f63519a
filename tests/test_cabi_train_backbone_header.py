"""CPU: include/gaussreg_hip_train_backbone.h -- the training entry points of the backbone's GroupNorm -- is read by the parser
that reads include/gaussreg_hip.h into _lib.BACKBONE_TRAIN_SIGNATURES, the library exports and binds what it declares, and the
workspace query of the GroupNorm backward answers without a GPU.  The three older headers and their tables stay as they were."""
import ctypes
import os
import re

from gaussreg_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PATH = os.path.join(ROOT, "include", "gaussreg_hip_train_backbone.h")
NAMES = {"gr_group_norm_train", "gr_group_norm_backward", "gr_group_norm_backward_workspace_bytes"}


def declared_symbols():               # as tests/test_cabi_symbols.py
    text = re.sub(r"/\*.*?\*/", "", open(PATH).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", text)))


def test_parser_covers_the_header():
    sigs, defines = _lib.parse_header(open(PATH).read())
    assert sorted(sigs) == declared_symbols() == sorted(NAMES)
    assert sigs == _lib.BACKBONE_TRAIN_SIGNATURES and defines == _lib.BACKBONE_TRAIN_DEFINES
    i64, f32, ptr, i, sz = ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert sigs["gr_group_norm_backward_workspace_bytes"] == (sz, [i64, i64, i64])
    # gr_group_norm_res's arguments with `stats` after `out`
    assert sigs["gr_group_norm_train"] == (i, [ptr, i64, i64, i64, ptr, ptr, f32, f32, ptr, ptr, ptr, ptr, i64, i64, ptr, sz, ptr])
    res = _lib.SIGNATURES["gr_group_norm_res"][1]
    assert sigs["gr_group_norm_train"][1] == res[:10] + [ptr] + res[10:]
    assert sigs["gr_group_norm_backward"] == (i, [ptr, ptr, ptr, ptr, ptr, i64, i64, i64, f32, ptr, i64, i64, ptr, ptr, ptr,
                                                  ptr, ptr, sz, ptr])


def test_the_older_tables_are_untouched():
    assert len(_lib.SIGNATURES) == 105
    older = set(_lib.SIGNATURES) | set(_lib.TRAIN_SIGNATURES) | set(_lib.MATCH_TRAIN_SIGNATURES)
    assert not set(_lib.BACKBONE_TRAIN_SIGNATURES) & older
    for header in ("gaussreg_hip.h", "gaussreg_hip_train.h", "gaussreg_hip_train_matching.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert "gr_group_norm_train" not in text and "gr_group_norm_backward" not in text


def test_library_exports_every_declared_symbol_and_binds_it():
    from gaussreg_amd import build
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared_symbols():
        assert hasattr(raw, s), f"libgaussreg_hip.so does not export {s}"
    L = _lib.lib()
    for name, (res, args) in _lib.BACKBONE_TRAIN_SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name


def test_workspace_query_is_host_only():
    q = _lib.lib().gr_group_norm_backward_workspace_bytes
    # what the call refuses: channel counts outside the forward's mapping, too many groups, groups that do not divide C,
    # too many segments, none
    for args in ((24, 4, 1), (6, 1, 1), (0, 1, 1), (64, 65, 1), (64, 0, 1), (64, 3, 1), (64, 32, 65536), (64, 32, -1),
                 (64, 32, 0), (5120 + 4, 1, 1)):
        assert q(*args) == 0, args
    # (segment, workgroup, 2, C) fp64 partials + (segment, 2, C) totals + (segment, 2, G) floats: O(blocks * C * nseg),
    # blocks <= 1024 and blocks * C <= 131 072 above 32 blocks -- nothing depends on N (it is not even an argument)
    for c, g in ((4, 1), (8, 8), (64, 32), (128, 32), (1024, 32), (2048, 32)):
        for nseg in (1, 2, 4, 3000, 65535):
            blocks = min(max(131072 // c, 32), 1024, max(1, 2048 // nseg))
            need = nseg * (16 * blocks * c + 16 * c + 8 * g)
            assert need <= q(c, g, nseg) <= need + 768, (c, g, nseg)
    assert q(64, 32, 1) <= (2 << 20) + 4096 and q(2048, 32, 1) <= (2 << 20) + 65536
    assert q(64, 32, 2) > q(64, 32, 1)
