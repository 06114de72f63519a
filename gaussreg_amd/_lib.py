"""ctypes binding of libgaussreg_hip.so.  Fails loudly.

include/gaussreg_hip.h is the only description of the ABI: `parse_header` reads it at import (without loading the library)
into SIGNATURES, name -> (restype, argtypes), and DEFINES, the integer `#define GR_*` constants.  The training entry points
that came after that header was closed are in include/gaussreg_hip_train.h, read the same way into TRAIN_SIGNATURES /
TRAIN_DEFINES, and those of the matching stage in include/gaussreg_hip_train_matching.h into MATCH_TRAIN_SIGNATURES /
MATCH_TRAIN_DEFINES, and those of the backbone's normalisation layers in include/gaussreg_hip_train_backbone.h into
BACKBONE_TRAIN_SIGNATURES / BACKBONE_TRAIN_DEFINES, and the cross-cloud nearest-neighbour entry points of
include/gaussreg_hip_cloud.h into CLOUD_SIGNATURES / CLOUD_DEFINES, and point-to-point ICP of include/gaussreg_hip_icp.h into
ICP_SIGNATURES / ICP_DEFINES, and the feature-space nearest neighbours of include/gaussreg_hip_feature_nn.h into
FEATURE_NN_SIGNATURES / FEATURE_NN_DEFINES, and the PCA normals and point-to-plane ICP of
include/gaussreg_hip_icp_plane.h into ICP_PLANE_SIGNATURES / ICP_PLANE_DEFINES, and generalised ICP with its covariance
kernels of include/gaussreg_hip_gicp.h into GICP_SIGNATURES / GICP_DEFINES; `lib()` binds the nine tables.  Only the three structs
that cross the boundary are mirrored by hand (they hold arrays).  A declaration the parser does not understand raises.

`call` is the one way a wrapper enters the library: it turns tensors into device pointers after checking that they are
contiguous and on the GPU of the call, appends workspace and stream, enters the device and checks the status.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgaussreg_hip.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "gaussreg_hip.h")
TRAIN_HEADER_PATH = os.path.join(_HERE, "..", "include", "gaussreg_hip_train.h")   # the training entry points added since
MATCH_TRAIN_HEADER_PATH = os.path.join(_HERE, "..", "include", "gaussreg_hip_train_matching.h")   # ... of the matching stage
BACKBONE_TRAIN_HEADER_PATH = os.path.join(_HERE, "..", "include", "gaussreg_hip_train_backbone.h")   # ... of the backbone's norms
CLOUD_HEADER_PATH = os.path.join(_HERE, "..", "include", "gaussreg_hip_cloud.h")   # cross-cloud nearest neighbours
ICP_HEADER_PATH = os.path.join(_HERE, "..", "include", "gaussreg_hip_icp.h")   # point-to-point ICP
FEATURE_NN_HEADER_PATH = os.path.join(_HERE, "..", "include", "gaussreg_hip_feature_nn.h")   # feature-space nearest neighbours
ICP_PLANE_HEADER_PATH = os.path.join(_HERE, "..", "include", "gaussreg_hip_icp_plane.h")   # PCA normals, point-to-plane ICP
GICP_HEADER_PATH = os.path.join(_HERE, "..", "include", "gaussreg_hip_gicp.h")   # generalised ICP, covariances

_lib = None

c_void = ctypes.c_void_p
c_f32 = ctypes.c_float


class RasterView(ctypes.Structure):
    """struct gr_raster_view (include/gaussreg_hip.h)."""
    _fields_ = [("image_height", ctypes.c_int32), ("image_width", ctypes.c_int32),
                ("tanfovx", c_f32), ("tanfovy", c_f32), ("bg", c_f32 * 3), ("scale_modifier", c_f32),
                ("viewmatrix", c_f32 * 16), ("projmatrix", c_f32 * 16), ("campos", c_f32 * 3),
                ("sh_degree", ctypes.c_int32), ("prefiltered", ctypes.c_int32), ("debug", ctypes.c_int32)]


class GsAdamGroup(ctypes.Structure):
    """struct gr_gs_adam_group (include/gaussreg_hip.h)."""
    _fields_ = [("param", c_void), ("grad", c_void), ("exp_avg", c_void), ("exp_avg_sq", c_void),
                ("lr", ctypes.c_double), ("K", ctypes.c_int32)]


class GsDensifyGroup(ctypes.Structure):
    """struct gr_gs_densify_group (include/gaussreg_hip.h)."""
    _fields_ = [("src_param", c_void), ("dst_param", c_void), ("src_exp_avg", c_void), ("dst_exp_avg", c_void),
                ("src_exp_avg_sq", c_void), ("dst_exp_avg_sq", c_void), ("K", ctypes.c_int32), ("role", ctypes.c_int32)]


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
            "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}
_POINTEES = set(_SCALARS) | {"void", "uint8_t", "uint64_t"}     # any pointer to these is a c_void_p
_STRUCTS = {"gr_raster_view": RasterView, "gr_gs_adam_group": GsAdamGroup, "gr_gs_densify_group": GsDensifyGroup}
_TYPE = r"(?:const\s+)?(\w+)"


def _ctype(base, star, where):
    if star:
        if base == "char":
            return ctypes.c_char_p
        if base in _STRUCTS:
            return ctypes.POINTER(_STRUCTS[base])
        if base in _POINTEES:
            return ctypes.c_void_p
    elif base in _SCALARS:
        return _SCALARS[base]
    raise ValueError(f"gaussreg_hip.h: type '{base}{star}' in {where} is outside the binding's vocabulary")


def parse_header(text):
    """-> (signatures, defines) of a header in the form of include/gaussreg_hip.h: every statement outside comments,
    preprocessor lines, struct typedefs and enums is `<ret> gr_name(<type> <name>, ...);`.  Anything else raises and
    names the declaration."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(GR_\w+)[ \t]+(-?\d+)[ \t]*$",
                                                                  text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r"\b(?:typedef\s+struct|enum)\b[^{};]*\{[^{}]*\}[^;]*;", "", text)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    signatures = {}
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        m = re.fullmatch(r"(.+?)\b(gr_\w+) ?\((.*)\)", decl)
        if m is None:
            raise ValueError(f"gaussreg_hip.h: cannot parse the declaration '{decl}'")
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        r = re.fullmatch(_TYPE + r"\s*(\*?)", ret)
        if r is None:
            raise ValueError(f"gaussreg_hip.h: cannot parse the return type '{ret}' of {name}")
        restype = None if r.groups() == ("void", "") else _ctype(r.group(1), r.group(2), f"the return type of {name}")
        argtypes = []
        for arg in ([] if args in ("", "void") else args.split(",")):
            a = re.fullmatch(_TYPE + r"(?:\s*(\*)\s*|\s+)\w+", arg.strip())
            if a is None:
                raise ValueError(f"gaussreg_hip.h: cannot parse the argument '{arg.strip()}' of {name}")
            argtypes.append(_ctype(a.group(1), a.group(2) or "", f"argument '{arg.strip()}' of {name}"))
        if name in signatures:
            raise ValueError(f"gaussreg_hip.h: {name} is declared twice")
        signatures[name] = (restype, argtypes)
    return signatures, defines


with open(HEADER_PATH) as _f:
    SIGNATURES, DEFINES = parse_header(_f.read())
with open(TRAIN_HEADER_PATH) as _f:
    TRAIN_SIGNATURES, TRAIN_DEFINES = parse_header(_f.read())
with open(MATCH_TRAIN_HEADER_PATH) as _f:
    MATCH_TRAIN_SIGNATURES, MATCH_TRAIN_DEFINES = parse_header(_f.read())
with open(BACKBONE_TRAIN_HEADER_PATH) as _f:
    BACKBONE_TRAIN_SIGNATURES, BACKBONE_TRAIN_DEFINES = parse_header(_f.read())
with open(CLOUD_HEADER_PATH) as _f:
    CLOUD_SIGNATURES, CLOUD_DEFINES = parse_header(_f.read())
with open(ICP_HEADER_PATH) as _f:
    ICP_SIGNATURES, ICP_DEFINES = parse_header(_f.read())
with open(FEATURE_NN_HEADER_PATH) as _f:
    FEATURE_NN_SIGNATURES, FEATURE_NN_DEFINES = parse_header(_f.read())
with open(ICP_PLANE_HEADER_PATH) as _f:
    ICP_PLANE_SIGNATURES, ICP_PLANE_DEFINES = parse_header(_f.read())
with open(GICP_HEADER_PATH) as _f:
    GICP_SIGNATURES, GICP_DEFINES = parse_header(_f.read())

GR_PENDING = DEFINES["GR_PENDING"]        # gr_raster_forward(GR_RASTER_SPLIT): enqueued, gr_raster_forward_finish collects the counts
GR_RETRY_FULL = DEFINES["GR_RETRY_FULL"]  # gr_raster_forward_finish: repeat the frame with an unsplit gr_raster_forward
GR_RETRY_BIN = DEFINES["GR_RETRY_BIN"]    # gr_raster_forward: bin buffer too small, call gr_raster_render_ex
GS_ADAM_MAX_GROUPS = DEFINES["GR_GS_ADAM_MAX_GROUPS"]
GS_KNN_MAX_K = DEFINES["GR_GS_KNN_MAX_K"]
CLOUD_KNN_MAX_K = CLOUD_DEFINES["GR_CLOUD_KNN_MAX_K"]
CLOUD_ICP_MAX_ITERATIONS = ICP_DEFINES["GR_CLOUD_ICP_MAX_ITERATIONS"]
FEATURE_NN_MAX_C = FEATURE_NN_DEFINES["GR_FEATURE_NN_MAX_C"]
CLOUD_NORMALS_MAX_K = ICP_PLANE_DEFINES["GR_CLOUD_NORMALS_MAX_K"]
GS_COV_RAW, GS_COV_PLANE = GICP_DEFINES["GR_GS_COV_RAW"], GICP_DEFINES["GR_GS_COV_PLANE"]
GS_DENSIFY_CARRIED, GS_DENSIFY_XYZ, GS_DENSIFY_SCALING = (DEFINES["GR_GS_DENSIFY_" + r] for r in ("CARRIED", "XYZ", "SCALING"))


class HipLibraryError(RuntimeError):
    pass


def lib():
    """Load the HIP library; raise (never fall back) if it has not been built."""
    global _lib
    if _lib is None:
        # torch first: libgaussreg_hip.so must bind to the SAME HIP runtime instance torch uses (the
        # wheel bundles its own libamdhip64); loading ours first leaves two runtimes in the process
        # and ours then reports "no ROCm-capable device".
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError(
                f"{LIB_PATH} is missing: build it with `python -m gaussreg_amd.build` "
                "(there is no CPU fallback for the gaussreg_amd ops)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in (list(SIGNATURES.items()) + list(TRAIN_SIGNATURES.items())
                                   + list(MATCH_TRAIN_SIGNATURES.items()) + list(BACKBONE_TRAIN_SIGNATURES.items())
                                   + list(CLOUD_SIGNATURES.items()) + list(ICP_SIGNATURES.items())
                                   + list(FEATURE_NN_SIGNATURES.items()) + list(ICP_PLANE_SIGNATURES.items())
                                   + list(GICP_SIGNATURES.items())):
            fn = getattr(L, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, allow=()):
    """Strict: every status but 0 raises, except the positive codes the call site names in `allow`."""
    if rc != 0 and rc not in allow:
        msg = lib().gr_last_error()
        raise RuntimeError("gaussreg_hip: " + (msg.decode() if msg else f"error {rc}"))
    return rc


def tensor_stamp(tensors):
    """Cache key for objects derived from tensors that may be updated in place: (storage address, version counter) per
    tensor, or None when any of them is an inference tensor (torch.inference_mode(): no version counter exists, reading
    `_version` raises) -- the caller then rebuilds instead of caching."""
    out = []
    for t in tensors:
        if t.is_inference():
            return None
        out.append((t.data_ptr(), t._version))
    return tuple(out)


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise HipLibraryError("gaussreg_amd ops need an MI355X (torch.cuda.is_available() is False); "
                              "there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


_ws_cache = {}


def workspace(device, nbytes):
    """Grow-only scratch buffer per (device, current stream, Python thread): two streams or two threads on one GPU never
    share scratch (the C library is re-entrant across streams only with distinct workspaces)."""
    import threading

    import torch
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream, threading.get_ident())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def stream_ptr(device):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    """Unchecked address of any tensor: the rasterizer's per-frame path, and host tensors handed over on purpose."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def device_ptr(t, dev, what, pos=None):
    """Address of `t` for a kernel that runs on `dev` (None stays NULL): `t` must be contiguous and on that GPU.  The error
    names `what`, and the argument position `pos` when there is one."""
    if t is None:
        return None
    if t.is_cuda and t.device == dev and t.is_contiguous():
        return t.data_ptr()
    where = what if pos is None else f"{what}: argument {pos}"
    if not t.is_contiguous():
        raise HipLibraryError(f"{where}: the tensor is not contiguous")
    raise HipLibraryError(f"{where}: the tensor is on {t.device}, the call runs on {dev}")


def call(dev, name, *args, ws=None, allow=()):
    """Run the entry point `name` on the GPU `dev`, on torch's current stream there, and check its status (`allow`: as
    in `check`); -> the status.  Every tensor among `args` is passed as its device pointer (`device_ptr`: a tensor that
    is elsewhere or strided raises before the device is touched); host memory is passed as ctypes objects, as it is.
    The stream is appended as the last argument; with `ws`, (workspace, its size) go in front of it, where every entry
    point with a workspace takes them: `ws` is a byte count -- the shared grow-only buffer of `workspace` -- or the
    caller's own uint8 tensor, for a buffer that another call reads again."""
    import torch
    Tensor = torch.Tensor
    argv = [device_ptr(a, dev, name, i) if isinstance(a, Tensor) else a for i, a in enumerate(args)]
    if ws is not None:
        if not isinstance(ws, Tensor):
            ws = workspace(dev, ws)
        argv += (device_ptr(ws, dev, name + ": workspace"), ws.numel())
    fn = getattr(lib(), name)
    with torch.cuda.device(dev):
        return check(fn(*argv, torch.cuda.current_stream(dev).cuda_stream), allow)


def to_device(t, dev, dtype=None, name=None, cast=True):
    """`t` contiguous on a GPU: a CPU tensor moves to `dev` (None: the current GPU), a GPU tensor stays where it is.
    `dtype`: cast to it, or with cast=False insist on it ("<name> must be a float tensor": the text of the reference's
    checks)."""
    if dtype is not None and not cast and t.dtype != dtype:
        raise RuntimeError(f"{name} must be a float tensor" if name else "expected a float tensor")
    if dev is None:
        dev = require_gpu()
    t = t if t.is_cuda else t.to(dev)
    return (t if dtype is None else t.to(dtype)).contiguous()


def to_device_bool(t, dev):
    """A mask as contiguous bool on a GPU (moved like `to_device`); any other dtype counts as `t != 0`."""
    import torch
    return to_device(t if t.dtype == torch.bool else t != 0, dev)


def like_input(outs, out_device):
    """A tensor or a tuple of tensors back on the device the caller's input came from (GPU results stay where they are)."""
    if out_device.type == "cuda":
        return outs
    return tuple(o.to(out_device) for o in outs) if isinstance(outs, (tuple, list)) else outs.to(out_device)


def offsets(lengths):
    """[0, l0, l0 + l1, ...]: the offsets of stacked segments from their lengths, as Python ints."""
    off = [0]
    for n in lengths:
        off.append(off[-1] + int(n))
    return off


def host_i64(values):
    arr = (ctypes.c_int64 * max(len(values), 1))(*[int(v) for v in values])
    return arr
