"""Mirror of ``diff_gaussian_rasterization`` (forward and backward) on the HIP rasterizer.

The package is NOT part of the GaussReg tree; the API below is the public
upstream one (graphdeco-inria/diff-gaussian-rasterization, diff_gaussian_rasterization/__init__.py):

    GaussianRasterizationSettings(image_height, image_width, tanfovx, tanfovy, bg, scale_modifier,
                                  viewmatrix, projmatrix, sh_degree, campos, prefiltered, debug)
    GaussianRasterizer(raster_settings).forward(means3D, means2D, opacities, shs=None,
        colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None) -> (color, radii)
    GaussianRasterizer.markVisible(positions) -> BoolTensor
    GaussianRasterizer(raster_settings, render_depth=True).forward(...) -> (color, radii, depth, alpha)   (extension)

plus `rasterize_views(...)`: many cameras over one Gaussian set in one launch sequence (the
throughput path: per-Gaussian inputs are read once per batch).

Differentiable like upstream: when grad mode is on and an input requires grad, the call goes through the autograd
Function (_Rasterize) whose backward is the HIP backward of include/gaussreg_hip.h (gr_raster_backward): gradients
for means3D, means2D (dL/dNDC), shs / colors_precomp, opacities, scales / rotations / cov3D_precomp; radii is not
differentiable.  Otherwise every call takes the forward-only path, unchanged.

Cameras: `viewmatrix`, `projmatrix` and `campos` of every view are differentiable too (gr_raster_backward_cam), as three
INDEPENDENT inputs, exactly as the settings present them: the gradient of `viewmatrix` does not include what reaches the
image through `projmatrix` or `campos`.  A caller that builds the three from one pose in torch (gaussreg_amd/pose.py) gets
the pose gradient by autograd's chain rule.  Element [j][c] of a matrix gradient belongs to element [j][c] of the tensor,
whatever its strides, dtype or device; column 3 of viewmatrix and column 2 of projmatrix are never read by the forward and
get zeros, campos acts through the SH view direction only (zeros with colors_precomp).  tanfovx, tanfovy, scale_modifier
and bg get no gradient.  A camera tensor that requires grad is enough to take the autograd path; with none, every path
and every result is what it is without this feature.
"""
import ctypes
import os
import threading
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


FAST_EXP, SPLIT, SHARE, BWD_COLOR_ONLY = (_lib.DEFINES["GR_RASTER_" + f] for f in ("FAST_EXP", "SPLIT", "SHARE", "BWD_COLOR_ONLY"))
_ENV_FAST = None
_bin_hint = {}  # (device, P, V, W, H) -> (bytes of the binning buffer, largest chunk) the last call of that shape needed


def _flags(fast_exp):
    """fast_exp None: the library default (environment variable GR_RASTER_FAST_EXP=1 switches it on)."""
    global _ENV_FAST
    if fast_exp is None:
        if _ENV_FAST is None:
            _ENV_FAST = os.environ.get("GR_RASTER_FAST_EXP", "0")[:1] == "1"
        fast_exp = _ENV_FAST
    return FAST_EXP if fast_exp else 0


def _view_struct(rs: GaussianRasterizationSettings) -> _lib.RasterView:
    v = _lib.RasterView()
    v.image_height, v.image_width = int(rs.image_height), int(rs.image_width)
    v.tanfovx, v.tanfovy = float(rs.tanfovx), float(rs.tanfovy)
    v.scale_modifier = float(rs.scale_modifier)
    v.sh_degree = int(rs.sh_degree)
    v.prefiltered, v.debug = int(bool(rs.prefiltered)), int(bool(rs.debug))
    bg = rs.bg.detach().to("cpu", torch.float32).reshape(-1).tolist()
    vm = rs.viewmatrix.detach().to("cpu", torch.float32).reshape(-1).tolist()
    pm = rs.projmatrix.detach().to("cpu", torch.float32).reshape(-1).tolist()
    cp = rs.campos.detach().to("cpu", torch.float32).reshape(-1).tolist()
    if len(bg) != 3 or len(vm) != 16 or len(pm) != 16 or len(cp) != 3:
        raise ValueError("bg/campos must have 3 elements, viewmatrix/projmatrix 16")
    v.bg[:] = bg
    v.viewmatrix[:] = vm
    v.projmatrix[:] = pm
    v.campos[:] = cp
    return v


class ViewBatch:
    """Cameras of one batched call, already marshalled into the C struct array (build once, reuse:
    marshalling V settings costs ~40 us of Python each)."""

    def __init__(self, settings: Sequence[GaussianRasterizationSettings]):
        if len(settings) < 1:
            raise ValueError("need at least one view")
        self.count = len(settings)
        self.height, self.width = int(settings[0].image_height), int(settings[0].image_width)
        self.array = (_lib.RasterView * self.count)(*[_view_struct(s) for s in settings])
        # the tensors the cameras were read from: a call under grad mode returns their gradients to them
        self.cameras = tuple((s.viewmatrix, s.projmatrix, s.campos) for s in settings)

    def wants_grad(self):
        return torch.is_grad_enabled() and any(t.requires_grad for cam in self.cameras for t in cam)

    def camera_inputs(self, dev):
        """Stacked (V,4,4), (V,4,4), (V,3) fp32 tensors on `dev`, differentiable functions of the settings' tensors (None
        where no view's tensor requires grad).  Their values are not read: the kernels take the marshalled copy."""
        out = []
        for k, shape in enumerate(((4, 4), (4, 4), (3,))):
            ts = [cam[k] for cam in self.cameras]
            if not any(t.requires_grad for t in ts):
                out.append(None)
                continue
            out.append(torch.stack([t.to(device=dev, dtype=torch.float32).reshape(shape) for t in ts]))
        return out


def _dev_f32(t: Optional[torch.Tensor], dev, name, grad=False):
    """fp32, contiguous, on `dev`.  `grad`: a differentiable conversion (no detach), so gradients reach the caller's tensor
    in its own dtype and device."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if grad:
        return t.to(device=dev, dtype=torch.float32).contiguous()
    if t.device == dev and t.dtype == torch.float32 and t.is_contiguous():
        return t  # only its pointer is read
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


class _FramePipe:
    """Two rasterizer calls in flight (per device and host thread).

    A one-camera frame is a chain of ~15 dependent launches, most of them a few microseconds of work: alone on a stream the
    chip idles through every hand-over.  Consecutive calls therefore run on two internal streams in turn, so the front of
    frame n+1 (preprocess, depth sort, tile counts) fills the gaps of frame n's scatter and blend (+19 % views/s).  Batched
    calls (32 views per call) gain too, for a different reason: the memory-bound sort and binning of call n+1 run next to
    the instruction-bound blend of call n (+5.6 %).  For the caller nothing changes: the outputs are joined into the
    caller's current stream before the call returns.

    Input readiness: a frame may only start when its input tensors are complete on the caller's stream.  In general that
    is `side.wait_stream(current)` -- which, after the previous frame was joined into `current`, also waits for that
    frame and serialises everything.  When the inputs are THE SAME tensors with the same version counters as in the
    previous frame (a static scene rendered from moving cameras), they were already complete at the previous call, and
    the frame waits only for the event recorded on the caller's stream at the FIRST call with these inputs.  The previous
    frame's inputs are kept referenced until the next call so that their addresses cannot be handed to other tensors in
    between (the stamp compares storage address + version).  An in-place update by the caller is ordered behind every frame
    that read the old values: each call joins its frame into the caller's stream before it returns.

    OPT-IN (`static_scene=True` on rasterize_views / GaussianRasterizer, or GR_RASTER_PIPELINE=1): the stamp only sees
    writes that bump a tensor's version counter.  `tensor.data.<op>_()` (`.data` carries its own counter), a custom
    extension kernel or any other library writing through `data_ptr()` change the scene without changing the stamp; the
    next frame would then start on the side stream next to that write and could render stale or torn values.  The
    default therefore is no pipe: every call is ordered on the caller's stream like upstream's.  Callers that opt in and
    do write behind the counter's back call reset_frame_pipe() after the write."""

    def __init__(self, dev):
        self.streams = tuple(torch.cuda.Stream(dev) for _ in range(2))
        self.turn = 0
        self.stamp = None
        self.keep = None
        self.caller = None
        self.ready = None  # recorded on the caller's stream at the first call with this stamp: the inputs were complete there
        self.ptrs = None   # the marshalled input pointers of the scene with this stamp (set by rasterize_views)
        self.overlapping = False

    def begin(self, dev, inputs):
        cur = torch.cuda.current_stream(dev)
        side = self.streams[self.turn]
        stamp = _lib.tensor_stamp(inputs)
        self.overlapping = False
        if stamp is not None and stamp == self.stamp and self.caller == cur.cuda_stream and self.ready is not None:
            side.wait_event(self.ready)
            self.overlapping = True   # this call runs next to the previous one
        else:
            side.wait_stream(cur)
            self.ptrs = None
            self.ready = None
            if stamp is not None:
                self.ready = torch.cuda.Event()
                self.ready.record(cur)
        self.stamp, self.keep, self.caller = stamp, inputs, cur.cuda_stream
        return cur, side

    def abort(self, cur, side):
        self.stamp = self.keep = self.ready = self.ptrs = None
        cur.wait_stream(side)

    def end(self, cur, side, outputs):
        self.turn = (self.turn + 1) % len(self.streams)
        cur.wait_stream(side)
        for t in outputs:
            t.record_stream(cur)


_pipes = threading.local()  # per host thread (the library's split-call state is per thread too) and device


def _frame_pipe(dev, static_scene):
    """The pipe is opt-in (see _FramePipe): `static_scene=True` per call, or GR_RASTER_PIPELINE=1 for the process
    (GR_RASTER_PIPELINE=0 wins over the argument: the switch tests and benches use to get the serial path)."""
    env = os.environ.get("GR_RASTER_PIPELINE")
    if env == "0" or not (static_scene or env == "1"):
        return None
    table = getattr(_pipes, "table", None)
    if table is None:
        table = _pipes.table = {}
    p = table.get(dev.index)
    if p is None:
        p = table[dev.index] = _FramePipe(dev)
    return p


_geom_bytes = {}


def _geom_size(L, P, V, W, H):
    """Bytes of the geometry buffer of a call of this shape (gr_raster_geom_bytes + slack), asked once per shape."""
    gkey = (P, V, W, H)
    gbytes = _geom_bytes.get(gkey)
    if gbytes is None:
        if len(_geom_bytes) > 64:
            _geom_bytes.clear()
        gbytes = _geom_bytes[gkey] = L.gr_raster_geom_bytes(P, V, W, H) + 256
    return gbytes


def reset_frame_pipe():
    """Drop this thread's frame pipes: the references they keep to the last frame's input tensors (see _FramePipe) and the
    readiness events.  The next one-camera call starts with a full wait on the caller's stream."""
    table = getattr(_pipes, "table", None)
    if table:
        for p in table.values():
            p.stamp = p.keep = p.ready = p.ptrs = None


# The per-Gaussian inputs in the order of the C ABI (include/gaussreg_hip.h): every tuple of them below is in this order.
_SCENE = ("means3D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp")
_GRADS = ("means3D", "means2D") + _SCENE[1:]  # the eight gradient outputs, in the order of the C ABI
_CAMERA = ("viewmatrix", "projmatrix", "campos")
_CAMERA_SHAPES = ((4, 4), (4, 4), (3,))
# _Rasterize.forward's arguments after ctx: backward finds needs_input_grad, and places its gradients, by these names
_ARGS = ("vb", "flags", "aux", "one", "box", "means2D") + _SCENE + _CAMERA
# (aux, a camera tensor needs grad) -> the backward entry point; its scratch size comes from <name>_bytes
_BACKWARD = {(False, False): "gr_raster_backward", (True, False): "gr_raster_backward_aux",
             (False, True): "gr_raster_backward_cam", (True, True): "gr_raster_backward_cam"}


def _sh_coeffs(sh, P):
    """M of the C ABI: SH coefficients per Gaussian of a (P, M, 3) or flat `shs` (0 with colors_precomp)."""
    return 0 if sh is None else (sh.shape[1] if sh.dim() == 3 else sh.reshape(max(P, 1), -1, 3).shape[1])


def _render_serial(vb, flags, one, inputs, aux, keep):
    """gr_raster_preprocess + render, serial, on the caller's stream.  `inputs`: _SCENE, fp32, contiguous, on the device.
    `aux`: also the depth and alpha maps (gr_raster_render_aux; otherwise gr_raster_render_keep, which always keeps).
    `keep`: the render also writes final_T and n_contrib for a backward.
    Returns (color, radii[, depth, alpha]), the num_rendered array and (M, geom, bin, state) for the backward; state =
    final_T, n_contrib of all views (None without `keep`).  Every output is a tensor of its own."""
    m = inputs[0]
    dev = m.device
    L = _lib.lib()
    V, views, H, W = vb.count, vb.array, vb.height, vb.width
    P = m.shape[0]
    M = _sh_coeffs(inputs[1], P)
    st = _lib.stream_ptr(dev)
    nr = (ctypes.c_int64 * (V + 1))()
    hw = H * W
    if aux:
        color = torch.empty((3, H, W) if one else (V, 3, H, W), dtype=torch.float32, device=dev)
        depth = torch.empty((1, H, W) if one else (V, 1, H, W), dtype=torch.float32, device=dev)
        alpha = torch.empty_like(depth)
        state = torch.empty(2 * V * hw, dtype=torch.float32, device=dev) if keep else None
    else:
        # colour, final_T, n_contrib (gr_raster_render_keep)
        block = torch.empty(5 * V * hw, dtype=torch.float32, device=dev)
    radii = torch.empty((P,) if one else (V, P), dtype=torch.int32, device=dev)
    gbytes = _geom_size(L, P, V, W, H)
    geom = torch.empty(gbytes, dtype=torch.uint8, device=dev)
    _lib.check(L.gr_raster_preprocess(P, M, *map(_lib.ptr, inputs), views, V, _lib.ptr(radii), _lib.ptr(geom), gbytes, nr,
                                      st))
    binb = torch.empty(L.gr_raster_bin_bytes(sum(nr[:V]), W, H, V) + 256, dtype=torch.uint8, device=dev)
    shared = (P, views, V, nr, _lib.ptr(geom), gbytes, _lib.ptr(binb), binb.numel())
    if aux:
        _lib.check(L.gr_raster_render_aux(*shared, _lib.ptr(color), _lib.ptr(depth), _lib.ptr(alpha), _lib.ptr(state), flags,
                                          st))
        return (color, radii, depth, alpha), nr, (M, geom, binb, state)
    _lib.check(L.gr_raster_render_keep(*shared, _lib.ptr(block), flags, st))
    # a tensor of its own (not a view of the state allocation): callers may modify the image in place, as upstream's
    color = block[:3 * V * hw].view((3, H, W) if one else (V, 3, H, W)).clone()
    return (color, radii), nr, (M, geom, binb, block[3 * V * hw:])


class _Rasterize(torch.autograd.Function):
    """Autograd forward (_render_serial with `keep`) and HIP backward: gr_raster_backward, gr_raster_backward_aux with the
    depth and alpha maps (`aux`), gr_raster_backward_cam when a camera tensor requires grad.  The Gaussian inputs arrive
    as fp32, contiguous, on the device (converted differentiably by the caller); viewmatrix / projmatrix / campos:
    ViewBatch.camera_inputs, or None.  `box` receives num_rendered (not an autograd output)."""

    @staticmethod
    def forward(ctx, vb, flags, aux, one, box, means2D, *scene_and_cameras):
        inputs = scene_and_cameras[:len(_SCENE)]
        outs, nr, (ctx.M, ctx.geom, ctx.binb, ctx.state) = _render_serial(vb, flags, one, inputs, aux, True)
        ctx.vb, ctx.flags, ctx.aux, ctx.nr = vb, flags, aux, nr
        ctx.m2d = None if means2D is None else (means2D.shape, means2D.dtype, means2D.device)
        ctx.save_for_backward(*inputs)
        ctx.mark_non_differentiable(outs[1])
        box.extend(nr[:vb.count])
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_color, grad_radii, grad_depth=None, grad_alpha=None):
        inputs = ctx.saved_tensors
        dev = inputs[0].device
        L = _lib.lib()
        vb, aux = ctx.vb, ctx.aux
        V, H, W = vb.count, vb.height, vb.width
        P = inputs[0].shape[0]
        need = dict(zip(_ARGS, ctx.needs_input_grad))
        # output gradients autograd did not produce: zeros for the colour-only backward, null pointers for the maps
        if grad_color is None and not aux:
            grad_color = torch.zeros((V, 3, H, W), dtype=torch.float32, device=dev)
        gc, gd, ga = (None if g is None else g.to(device=dev, dtype=torch.float32).contiguous()
                      for g in (grad_color, grad_depth, grad_alpha))
        grads = dict.fromkeys(_ARGS)
        for name, t in zip(_SCENE, inputs):
            if t is not None and need[name]:
                grads[name] = torch.empty_like(t)
        if need["means2D"]:
            grads["means2D"] = torch.empty((V, P, 3), dtype=torch.float32, device=dev)
        cam = False
        for name, shape in zip(_CAMERA, _CAMERA_SHAPES):
            if need[name]:
                cam = True
                grads[name] = torch.empty((V,) + shape, dtype=torch.float32, device=dev)
        hw = H * W
        final_T, n_contrib = ctx.state[:V * hw], ctx.state[V * hw:]
        # the three entry points share their argument list up to dL_dcolor and from the flags on; the map gradients
        # (aux, cam) and the camera outputs (cam) are spliced in.  Without the maps, cam gets null map gradients and
        # GR_RASTER_BWD_COLOR_ONLY, in its scratch layout too.
        entry = _BACKWARD[aux, cam]
        color_only = BWD_COLOR_ONLY if cam and not aux else 0
        maps = (_lib.ptr(gd), _lib.ptr(ga)) if aux or cam else ()
        outs = [_lib.ptr(grads[name]) for name in (_GRADS + _CAMERA if cam else _GRADS)]
        with torch.cuda.device(dev):
            sbytes = getattr(L, entry + "_bytes")(P, V, W, H, ctx.nr, *((color_only,) if cam else ())) + 256
            scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)
            _lib.check(getattr(L, entry)(
                P, ctx.M, *map(_lib.ptr, inputs), vb.array, V, _lib.ptr(ctx.geom), ctx.geom.numel(), _lib.ptr(ctx.binb),
                ctx.binb.numel(), ctx.nr, _lib.ptr(final_T), _lib.ptr(n_contrib), _lib.ptr(gc), *maps,
                ctx.flags | color_only, *outs,
                _lib.ptr(scratch), scratch.numel(), _lib.stream_ptr(dev)))
        if grads["means2D"] is not None:
            shape, dtype, device = ctx.m2d
            grads["means2D"] = grads["means2D"].reshape(shape).to(device=device, dtype=dtype)
        return tuple([grads[name] for name in _ARGS])


def _wants_grad(*ts):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def _render_pipelined(vb, flags, one, inputs, static_scene):
    """The forward-only colour path: one gr_raster_forward per frame, on the frame pipe's side streams when the caller
    opted in (_FramePipe).  `inputs`: _SCENE, fp32, contiguous, on the device.  Returns (color, radii, num_rendered)."""
    m, sh, cp, op, sc, rot, cov = inputs
    dev = m.device
    L = _lib.lib()
    V, views, H, W = vb.count, vb.array, vb.height, vb.width
    P = m.shape[0]
    M = _sh_coeffs(sh, P)
    nr = (ctypes.c_int64 * (V + 1))()
    pipe = _frame_pipe(dev, static_scene)
    cur = side = None
    # (explicit set_device / set_stream instead of the context managers: a one-camera frame is ~0.2 ms and every
    # microsecond of Python between two library calls is on the critical path)
    home = torch.cuda.current_device()
    if home != dev.index:
        torch.cuda.set_device(dev)
    try:
        if pipe is not None:
            cur, side = pipe.begin(dev, tuple(t for t in (m, op, sh, cp, sc, rot, cov) if t is not None))
            torch.cuda.set_stream(side)  # allocations below come from the side stream's pool
            st = ctypes.c_void_p(side.cuda_stream)
        else:
            st = _lib.stream_ptr(dev)
        color = torch.empty((3, H, W) if one else (V, 3, H, W), dtype=torch.float32, device=dev)
        radii = torch.empty((P,) if one else (V, P), dtype=torch.int32, device=dev)  # every entry is written by preprocess
        gbytes = _geom_size(L, P, V, W, H)
        geom = torch.empty(gbytes, dtype=torch.uint8, device=dev)
        # the binning buffer is sized from the last call of this shape (+ 25 %): the library is entered once per frame, and
        # only a frame that needs more comes back for a larger buffer
        key = (dev.index, P, V, W, H)
        hint, chunk_hint = _bin_hint.get(key, (0, 0))
        binb = torch.empty(hint + 256, dtype=torch.uint8, device=dev) if hint else None
        nr[V] = chunk_hint  # in: sizes the scatter's staging block of the speculative launch; out: this call's figure

        # (the inputs' pointers are marshalled once per scene: the pipe keeps them while the stamp stays the same)
        if pipe is not None and pipe.ptrs is not None:
            ptrs = pipe.ptrs
        else:
            ptrs = (_lib.ptr(m), _lib.ptr(sh), _lib.ptr(cp), _lib.ptr(op), _lib.ptr(sc), _lib.ptr(rot), _lib.ptr(cov))
            if pipe is not None:
                pipe.ptrs = ptrs

        def forward(fl):
            return L.gr_raster_forward(P, M, *ptrs, views, V, _lib.ptr(radii), _lib.ptr(geom), gbytes, _lib.ptr(binb),
                                       hint + 256 if binb is not None else 0, _lib.ptr(color), fl, nr, st)
        # with the pipe: the library returns as soon as the frame is enqueued, and the stream joins below run while the GPU
        # works through the front of the frame; gr_raster_forward_finish then waits for the instance counts
        rc = forward(flags | ((SPLIT | (SHARE if pipe.overlapping and V == 1 else 0)) if pipe is not None else 0))
        joined = rejoin = False
        if rc == _lib.GR_PENDING:
            try:
                torch.cuda.set_stream(cur)
                pipe.end(cur, side, (color, radii))
                joined = True
            finally:
                rc = L.gr_raster_forward_finish(nr)
            if rc in (_lib.GR_RETRY_BIN, _lib.GR_RETRY_FULL):  # rare: more work for this frame on the side stream
                torch.cuda.set_stream(side)
                rejoin = True
            if rc == _lib.GR_RETRY_FULL:
                rc = forward(flags)
        _lib.check(rc, allow=(_lib.GR_RETRY_BIN,))
        need = L.gr_raster_bin_bytes(sum(nr[:V]), W, H, V)
        if rc == _lib.GR_RETRY_BIN:
            binb = torch.empty(need + 256, dtype=torch.uint8, device=dev)
            _lib.check(L.gr_raster_render_ex(P, views, V, nr, _lib.ptr(geom), geom.numel(), _lib.ptr(binb), binb.numel(),
                                             _lib.ptr(color), flags, st))
        if len(_bin_hint) > 64:
            _bin_hint.clear()
        _bin_hint[key] = (need + need // 4 + 1024, int(nr[V]))
        if pipe is not None:
            torch.cuda.set_stream(cur)
            if not joined:
                pipe.end(cur, side, (color, radii))
            elif rejoin:
                cur.wait_stream(side)
    except BaseException:
        if pipe is not None and cur is not None:
            torch.cuda.set_stream(cur)
            pipe.abort(cur, side)
        raise
    finally:
        if home != dev.index:
            torch.cuda.set_device(home)
    return color, radii, nr[:V]


def rasterize_views(settings, means3D, opacities, shs=None,
                    colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, fast_exp=None, _one=False,
                    static_scene=False, *, means2D=None, render_depth=False):
    """Render the same Gaussians from len(settings) cameras (`settings`: a sequence of
    GaussianRasterizationSettings, or a prebuilt ViewBatch).

    Returns (color (V,3,H,W) f32, radii (V,P) i32, num_rendered list[int]).  num_rendered = (tile, Gaussian)
    instances actually binned per view: at most the reference's count (pairs that cannot reach alpha = 1/255
    anywhere in the tile are dropped before the sort; the image is unaffected).

    `fast_exp=True`: the blend uses the hardware exponential (v_exp_f32) instead of the deterministic polynomial of the
    oracle -- the image is within 1e-5 relative of the bit-exact one (default False: bit-exact).
    `static_scene=True` (extension): consecutive calls over the same, unmodified scene tensors overlap on two internal
    streams (_FramePipe: read its contract first -- only writes that bump the tensors' version counters are seen).
    (`_one`: internal, one camera -- the outputs come back as (3,H,W) and (P,), no view ops on the way out.)

    Autograd: when grad mode is on and any input requires grad, the call is differentiable (see the module docstring);
    the `viewmatrix`, `projmatrix` and `campos` tensors of the settings (or of the settings a ViewBatch was built from)
    count as inputs.  It then runs serially on the caller's stream (`static_scene` is ignored) and keeps its buffers for the backward.
    `means2D` (keyword only, extension): a (V, P, 3) tensor (upstream's (P, 3) screen-space means for one camera) whose
    .grad receives dL/d(NDC position) per view; its values are not read.

    `render_depth=True` (keyword only): returns (color, radii, num_rendered, depth, alpha) with depth and alpha of shape
    (V,1,H,W) fp32: depth = sum_i w_i z_i over the entries the colour blend blends (w_i its weights, z_i the view-space
    depth; the background adds nothing), alpha = 1 - final transmittance.  color and radii are bit-identical to the
    call without it.  Differentiable like the colour.  The call runs serially on the caller's stream with and without
    grad: `static_scene` is ignored on this path."""
    dev = means3D.device if means3D.is_cuda else _lib.require_gpu()
    n_pts = int(means3D.shape[0])

    def given(t):  # upstream passes empty tensors for "not provided"; with zero Gaussians everything is empty
        return t is not None and (t.numel() > 0 or n_pts == 0)

    has_sh, has_cp = given(shs), given(colors_precomp)
    has_sc, has_rot, has_cov = given(scales), given(rotations), given(cov3D_precomp)
    if has_sh == has_cp:
        raise Exception('Please provide excatly one of either SHs or precomputed colors!')
    has_sr = has_sc and has_rot
    if has_sr == has_cov or has_sc != has_rot:
        raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
    vb = settings if isinstance(settings, ViewBatch) else ViewBatch(settings)
    cam_grad = vb.wants_grad()
    grad = cam_grad or _wants_grad(means3D, means2D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp)
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    if grad and means2D is not None:
        ok = (tuple(means2D.shape) == (vb.count, n_pts, 3) or
              (vb.count == 1 and tuple(means2D.shape) == (n_pts, 3)))
        if not ok:
            raise ValueError(f"means2D must have shape ({vb.count}, {n_pts}, 3)" +
                             (f" or ({n_pts}, 3)" if vb.count == 1 else "") + f", got {tuple(means2D.shape)}")
    # under grad the conversion is part of the graph; otherwise only the pointers are read
    inputs = (_dev_f32(means3D, dev, "means3D", grad),
              _dev_f32(shs, dev, "shs", grad) if has_sh else None,
              _dev_f32(colors_precomp, dev, "colors_precomp", grad) if has_cp else None,
              _dev_f32(opacities, dev, "opacities", grad),
              _dev_f32(scales, dev, "scales", grad) if has_sr else None,
              _dev_f32(rotations, dev, "rotations", grad) if has_sr else None,
              _dev_f32(cov3D_precomp, dev, "cov3D_precomp", grad) if has_cov else None)  # (_SCENE)
    flags, one = _flags(fast_exp), _one and vb.count == 1
    if not (grad or render_depth):
        return _render_pipelined(vb, flags, one, inputs, static_scene)
    home = torch.cuda.current_device()
    if home != dev.index:
        torch.cuda.set_device(dev)
    try:
        if grad:
            num_rendered = []
            outs = _Rasterize.apply(vb, flags, render_depth, one, num_rendered, means2D, *inputs,
                                    *(vb.camera_inputs(dev) if cam_grad else (None, None, None)))
        else:
            outs, nr, _ = _render_serial(vb, flags, one, inputs, True, False)
            num_rendered = nr[:vb.count]
    finally:
        if home != dev.index:
            torch.cuda.set_device(home)
    return (outs[0], outs[1], num_rendered) + tuple(outs[2:])


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, fast_exp=None, static_scene=False, render_depth=False):
    """`raster_settings`: GaussianRasterizationSettings, or a one-camera ViewBatch built from it (marshalled once).
    `render_depth=True`: returns (color, radii, depth, alpha), depth and alpha of shape (1, H, W) (see rasterize_views)."""
    vb = raster_settings if isinstance(raster_settings, ViewBatch) else [raster_settings]
    m2d = means2D if isinstance(means2D, torch.Tensor) and means2D.requires_grad else None
    if render_depth:
        color, radii, _, depth, alpha = rasterize_views(vb, means3D, opacities, sh, colors_precomp, scales, rotations,
                                                        cov3Ds_precomp, fast_exp=fast_exp, _one=True, means2D=m2d,
                                                        render_depth=True)
        return color, radii, depth, alpha
    color, radii, _ = rasterize_views(vb, means3D, opacities, sh, colors_precomp, scales, rotations, cov3Ds_precomp,
                                      fast_exp=fast_exp, _one=True, static_scene=static_scene, means2D=m2d)
    return color, radii


class GaussianRasterizer(torch.nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings, fast_exp=None, static_scene=False,
                 render_depth=False):
        """`fast_exp`, `static_scene` (extensions, upstream has no such arguments): see rasterize_views.
        `render_depth=True`: forward returns (color, radii, depth, alpha) with depth and alpha of shape (1, H, W), the
        order and shapes of the common depth forks of upstream; `static_scene` is then ignored."""
        super().__init__()
        self.render_depth = render_depth
        self.raster_settings = raster_settings
        self.fast_exp = fast_exp
        self.static_scene = static_scene
        self._view_batch = None  # (settings object, tensor versions, ViewBatch): the C camera struct is built once

    @staticmethod
    def _stamp(rs):
        # the camera tensors may be updated in place between frames (pose optimisation): their storage and version
        # counters are part of the cache key, so a stale marshalled copy is never rendered
        # (None for inference tensors, which carry no version counter: nothing is cached for them)
        return _lib.tensor_stamp((rs.viewmatrix, rs.projmatrix, rs.campos, rs.bg))

    def _views(self):
        rs = self.raster_settings
        stamp = self._stamp(rs)
        if stamp is None:
            self._view_batch = None
            return ViewBatch([rs])
        if self._view_batch is None or self._view_batch[0] is not rs or self._view_batch[1] != stamp:
            self._view_batch = (rs, stamp, ViewBatch([rs]))
        return self._view_batch[2]

    def markVisible(self, positions):
        with torch.no_grad():
            dev = _lib.require_gpu()
            p = positions.detach().to(device=positions.device if positions.is_cuda else dev,
                                      dtype=torch.float32).contiguous()
            present = torch.zeros((p.shape[0],), dtype=torch.uint8, device=p.device)
            vm = (ctypes.c_float * 16)(*self.raster_settings.viewmatrix.detach().to("cpu", torch.float32)
                                       .reshape(-1).tolist())
            _lib.call(p.device, "gr_raster_mark_visible", p.shape[0], p, vm, present)
            return present.bool()

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        rs = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                   cov3D_precomp, self._views(), fast_exp=self.fast_exp, static_scene=self.static_scene,
                                   render_depth=self.render_depth)
