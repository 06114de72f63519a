"""CPU: the ctypes binding is derived from include/gaussreg_hip.h, and _lib.call checks what it passes."""
import ctypes
import os
import re

import pytest
import torch

from gaussreg_amd import _lib, ext, rasterizer

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaussreg_hip.h")).read(), flags=re.S)


def declared_symbols():               # as tests/test_cabi_symbols.py
    return sorted(set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", HEADER)))


def test_parser_covers_the_header():
    sigs, _ = _lib.parse_header(open(os.path.join(ROOT, "include", "gaussreg_hip.h")).read())
    assert sorted(sigs) == declared_symbols() and len(sigs) == 105
    assert sigs == _lib.SIGNATURES
    # one of each kind of type: scalars by width and signedness, the string, a struct pointer, plain pointers, void
    assert sigs["gr_last_error"] == (ctypes.c_char_p, [])
    assert sigs["gr_timing_enable"] == (None, [ctypes.c_int])
    assert sigs["gr_timing_read"] == (ctypes.c_int, [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p])
    assert sigs["gr_ransac_sample_hash"] == (ctypes.c_uint32, [ctypes.c_uint32] * 4)
    assert sigs["gr_rpe_attention_backward_max_keys"] == (ctypes.c_int64, [ctypes.c_int64] * 2)
    assert sigs["gr_gs_knn_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int])
    assert sigs["gr_raster_render"][1][:3] == [ctypes.c_int64, ctypes.POINTER(_lib.RasterView), ctypes.c_int]
    assert sigs["gr_gs_adam_step"][1][:8] == [ctypes.POINTER(_lib.GsAdamGroup), ctypes.c_int, ctypes.c_int64] + \
        [ctypes.c_double] * 5
    assert sigs["gr_radius_count"][1][7:10] == [ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t]
    assert len(sigs["gr_raster_backward_cam"][1]) == 36 and len(sigs["gr_kpconv_backward"][1]) == 24


@pytest.mark.parametrize("text", ["int gr_x(long double a);",           # a type outside the vocabulary
                                  "int gr_x(struct foo* a);", "int gr_x(int** a);", "wchar_t gr_x(int a);",
                                  "int gr_x(int a",                     # malformed: no closing parenthesis
                                  "int gr_x(int, float b);",            # an argument without a name
                                  "int gr_ok(int a); int gr_x(int a) { return a; }"])
def test_parser_refuses_what_it_does_not_know(text):
    with pytest.raises(ValueError, match="gr_x"):
        _lib.parse_header(text)


@pytest.mark.parametrize("cls, name", [(_lib.RasterView, "gr_raster_view"), (_lib.GsAdamGroup, "gr_gs_adam_group"),
                                       (_lib.GsDensifyGroup, "gr_gs_densify_group")])
def test_struct_mirrors_follow_the_header(cls, name):
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), HEADER, flags=re.S).group(1)
    fields = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):      # `int32_t a, b` and `float v[16]` included
        first, *more = stmt.split(",")
        fields += [re.search(r"(\w+)\s*(?:\[\d+\])?$", d.strip()).group(1) for d in [first] + more]
    assert [f[0] for f in cls._fields_] == fields


def test_defines_come_from_the_header():
    for name in ("GR_RASTER_BWD_COLOR_ONLY", "GR_PENDING", "GR_RETRY_FULL", "GR_RETRY_BIN", "GR_GS_KNN_MAX_K",
                 "GR_GS_ADAM_MAX_GROUPS", "GR_GS_DENSIFY_XYZ", "GR_ORDER_CELL", "GR_ERR_WORKSPACE"):
        value = int(re.search(r"#define\s+%s\s+(-?\d+)" % name, HEADER).group(1))
        assert _lib.DEFINES[name] == value
    assert rasterizer.BWD_COLOR_ONLY == _lib.DEFINES["GR_RASTER_BWD_COLOR_ONLY"] == 8
    assert (rasterizer.FAST_EXP, rasterizer.SPLIT, rasterizer.SHARE) == (1, 2, 4)
    assert (_lib.GR_PENDING, _lib.GR_RETRY_FULL, _lib.GR_RETRY_BIN) == (2, 3, 1)
    assert _lib.GR_PENDING == _lib.DEFINES["GR_PENDING"] and _lib.GR_RETRY_FULL == _lib.DEFINES["GR_RETRY_FULL"]
    assert _lib.GS_KNN_MAX_K == _lib.DEFINES["GR_GS_KNN_MAX_K"] == 8
    assert _lib.GS_ADAM_MAX_GROUPS == _lib.DEFINES["GR_GS_ADAM_MAX_GROUPS"] == 8
    assert (_lib.GS_DENSIFY_CARRIED, _lib.GS_DENSIFY_XYZ, _lib.GS_DENSIFY_SCALING) == (0, 1, 2)
    assert ext._ORDER == {"reference": _lib.DEFINES["GR_ORDER_REFERENCE"], "cell": _lib.DEFINES["GR_ORDER_CELL"]}


def test_call_checks_tensors_before_it_touches_the_device(monkeypatch):
    """A tensor that is not on the GPU of the call, or is strided, never reaches C: the error names the entry point and the
    argument, and neither the device nor the library has been entered (no GPU is needed for this test)."""
    entered = []
    monkeypatch.setattr(torch.cuda, "device", lambda dev: entered.append(dev))
    monkeypatch.setattr(_lib, "workspace", lambda dev, nbytes: entered.append(nbytes))
    dev = torch.device("cuda", 0)
    x = torch.zeros(4, 3)
    with pytest.raises(_lib.HipLibraryError, match=r"gr_neighbor_pool: argument 0: the tensor is on cpu"):
        _lib.call(dev, "gr_neighbor_pool", x, 4, 3, None, 0, 0, 0, None)
    with pytest.raises(_lib.HipLibraryError, match=r"gr_gs_knn: argument 3: the tensor is on cpu"):
        _lib.call(dev, "gr_gs_knn", None, 4, 3, x, None, None, ws=1024)
    with pytest.raises(_lib.HipLibraryError, match=r"gr_radius_fill: workspace: the tensor is on cpu"):
        _lib.call(dev, "gr_radius_fill", None, None, 0, 0, 0, 1.0, 0, None, None, ws=torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(_lib.HipLibraryError, match=r"gr_neighbor_pool: argument 7: the tensor is not contiguous"):
        _lib.call(dev, "gr_neighbor_pool", None, 4, 3, None, 0, 0, 0, torch.zeros(4, 6)[:, ::2])
    assert entered == []
