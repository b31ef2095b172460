"""ctypes binding of libsvbrdf_hip.so (C ABI: include/svbrdf_hip.h).

PyTorch is used here only for device memory, the current HIP stream and (elsewhere)
autograd glue.  No arithmetic of the hot path happens in Python.  If the shared
library is missing or fails to load, every entry point raises NativeLibraryError --
there is deliberately no fallback.
"""
import collections
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SVBRDF_HIP_LIB: load another build of the same ABI (ablation/experiment builds of tools/); default in-tree
_SO = os.environ.get("SVBRDF_HIP_LIB") or os.path.join(_HERE, "lib", "libsvbrdf_hip.so")
ABI_VERSION = 8
# SVBRDF_RECTIFY_GRAD_DEPTH of include/svbrdf_hip.h: the float32 additions a term of svbrdf_rectify_photos_grad_matrices'
# sums passes through at most (the tests' error bound is built on it)
RECTIFY_GRAD_DEPTH = 24

_lock = threading.Lock()
_lib = None
_xrow_cache = {}
_workspace_cache = {}
_launch_hook = None


def set_launch_hook(fn):
    """Measurement aid: ``fn("begin")`` / ``fn("end")`` is called immediately before / after the
    kernel launches of the fused loss are enqueued (bench.py records HIP events there).
    None disables it.  No effect on results."""
    global _launch_hook
    _launch_hook = fn


class NativeLibraryError(RuntimeError):
    """libsvbrdf_hip.so is missing, stale or reported an error."""


def library_path():
    return _SO


_fp, _int, _float, _size, _u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_ulonglong
_DIMS = [_int] * 4 + [_fp]                                            # B, S (or R), H, W, stream
_LOSS = [_fp] * 4 + [_float] + [_fp] * 3 + [_size] + _DIMS            # input, other, scenes, xrow, eps, loss, grad, ws, bytes
_LOSS_W = [_fp] * 3 + [_int] + [_fp] * 2 + [_float] + [_fp] * 3 + [_size] + _DIMS   # input, photos, weights, planes, scenes, ...
# input, photos, weights, planes, exposure, scenes, xrow, eps, loss, grad, grad_exposure, ws, bytes
_LOSS_X = [_fp] * 3 + [_int] + [_fp] * 3 + [_float] + [_fp] * 4 + [_size] + _DIMS
# input, photos, weights, planes, scenes, xrow, eps, loss, grad, grad_scenes, ws, bytes
_LOSS_SG = [_fp] * 3 + [_int] + [_fp] * 2 + [_float] + [_fp] * 4 + [_size] + _DIMS
# maps, exp_avg, exp_avg_sq, photos, weights, planes, scenes, xrow, eps, bounds, lr, beta1, beta2, adam_eps, step, loss, grad, ws, bytes
_LOSS_FIT = [_fp] * 5 + [_int] + [_fp] * 2 + [_float, _fp] + [_float] * 4 + [_int] + [_fp] * 3 + [_size] + _DIMS
# ... step, loss, grad, grad_scenes, ws, bytes: the step's list with grad_scenes behind the gradient
_LOSS_FIT_SG = [_fp] * 5 + [_int] + [_fp] * 2 + [_float, _fp] + [_float] * 4 + [_int] + [_fp] * 4 + [_size] + _DIMS
# ... adam_eps, first_step, n_steps, losses, ws, bytes: the step's list with (first_step, n_steps) for `step` and no gradient
_LOSS_FIT_STEPS = [_fp] * 5 + [_int] + [_fp] * 2 + [_float, _fp] + [_float] * 4 + [_int] * 2 + [_fp] * 2 + [_size] + _DIMS
# maps_in, maps_out, exp_avg, exp_avg_sq, photos, weights, planes, scenes, xrow, eps, smooth, bounds, lr, ...: the step's
# list with maps_out behind the maps and the 12 lambdas in front of the bounds; the same with grad_scenes
_LOSS_FIT_SMOOTH = [_fp] * 6 + [_int] + [_fp] * 2 + [_float, _fp, _fp] + [_float] * 4 + [_int] + [_fp] * 3 + [_size] + _DIMS
_LOSS_FIT_SMOOTH_SG = [_fp] * 6 + [_int] + [_fp] * 2 + [_float, _fp, _fp] + [_float] * 4 + [_int] + [_fp] * 4 + [_size] + _DIMS
_LOSS_L1 = [_fp] * 4 + [_float] * 3 + [_fp] * 3 + [_size] + _DIMS     # ... eps, l1_weight, eps_l1 ...
_INPUTS = [_fp] * 3 + [_u64] * 2 + [_fp] * 2 + _DIMS
# name -> (restype, argtypes) of every SVBRDF_API function of include/svbrdf_hip.h, applied once in _load();
# tests/test_host_logic.py holds the lengths against the header
SIGNATURES = {
    "svbrdf_abi_version": (_int, []),
    "svbrdf_last_error": (ctypes.c_char_p, []),
    "svbrdf_make_xrow": (_int, [_fp, _int]),
    "svbrdf_render_fwd": (_int, [_fp] * 4 + _DIMS),
    "svbrdf_render_bwd": (_int, [_fp] * 5 + _DIMS),
    "svbrdf_render_fwd_host_scenes": (_int, [_fp, _fp, _int, _fp, _fp] + _DIMS),
    "svbrdf_render_bwd_host_scenes": (_int, [_fp, _fp, _int, _fp, _fp, _fp] + _DIMS),
    "svbrdf_render_fwd_ragged": (_int, [_fp] * 5 + _DIMS),
    "svbrdf_render_bwd_ragged": (_int, [_fp] * 6 + _DIMS),
    "svbrdf_rendering_loss_workspace_bytes": (_size, [_int] * 4),
    "svbrdf_rendering_loss_fwd_bwd": (_int, _LOSS),
    "svbrdf_mixed_loss_fwd_bwd": (_int, _LOSS_L1),
    "svbrdf_head_loss_fwd_bwd": (_int, _LOSS_L1),
    "svbrdf_host_scenes_max_rows": (_int, []),
    "svbrdf_mixed_loss_fwd_bwd_host_scenes": (_int, _LOSS_L1),
    "svbrdf_head_loss_fwd_bwd_host_scenes": (_int, _LOSS_L1),
    "svbrdf_photo_loss_fwd_bwd": (_int, _LOSS),
    "svbrdf_photo_loss_fwd_bwd_host_scenes": (_int, _LOSS),
    "svbrdf_head_photo_loss_fwd_bwd": (_int, _LOSS),
    "svbrdf_head_photo_loss_fwd_bwd_host_scenes": (_int, _LOSS),
    "svbrdf_photo_loss_weighted_fwd_bwd": (_int, _LOSS_W),
    "svbrdf_photo_loss_weighted_fwd_bwd_host_scenes": (_int, _LOSS_W),
    "svbrdf_head_photo_loss_weighted_fwd_bwd": (_int, _LOSS_W),
    "svbrdf_head_photo_loss_weighted_fwd_bwd_host_scenes": (_int, _LOSS_W),
    "svbrdf_photo_exposure_workspace_bytes": (_size, [_int] * 4),
    "svbrdf_photo_loss_exposure_fwd_bwd": (_int, _LOSS_X),
    "svbrdf_head_photo_loss_exposure_fwd_bwd": (_int, _LOSS_X),
    "svbrdf_photo_scene_grad_workspace_bytes": (_size, [_int] * 4),
    "svbrdf_photo_loss_scene_grad_fwd_bwd": (_int, _LOSS_SG),
    "svbrdf_head_photo_loss_scene_grad_fwd_bwd": (_int, _LOSS_SG),
    # input, photos, weights, planes, scenes, xrow, eps, loss, grad (or NULL), grad_photos, ws, bytes: _LOSS_SG's list
    "svbrdf_photo_loss_photo_grad_fwd_bwd": (_int, _LOSS_SG),
    "svbrdf_head_photo_loss_photo_grad_fwd_bwd": (_int, _LOSS_SG),
    "svbrdf_photo_fit_adam_scalars": (_int, [_float] * 3 + [_int, _fp]),
    "svbrdf_photo_fit_adam_step": (_int, _LOSS_FIT),
    "svbrdf_photo_fit_adam_step_scene_grad": (_int, _LOSS_FIT_SG),
    "svbrdf_photo_fit_smooth_adam_step": (_int, _LOSS_FIT_SMOOTH),
    "svbrdf_photo_fit_smooth_adam_step_scene_grad": (_int, _LOSS_FIT_SMOOTH_SG),
    "svbrdf_photo_fit_steps_workspace_bytes": (_size, [_int] * 5),
    "svbrdf_photo_fit_adam_steps": (_int, _LOSS_FIT_STEPS),
    # src, format, P, Hs, Ws, matrices, Hd, Wd, k, lut, clip_lo, clip_hi, out, weights_out, stream
    "svbrdf_rectify_photos": (_int, [_fp, _int, _int, _int, _int, _fp, _int, _int, _int, _fp, _float, _float, _fp, _fp, _fp]),
    "svbrdf_rectify_grad_workspace_bytes": (_size, [_int] * 3),
    # src, format, P, Hs, Ws, matrices, Hd, Wd, k, lut, clip_lo, clip_hi, grad_values, grad_matrices, ws, bytes, stream
    "svbrdf_rectify_photos_grad_matrices": (_int, [_fp, _int, _int, _int, _int, _fp, _int, _int, _int, _fp, _float, _float,
                                                   _fp, _fp, _fp, _size, _fp]),
    # src, format, P, Hs, Ws, matrices, lens, Hd, Wd, k, lut, clip_lo, clip_hi, out, weights_out, stream
    "svbrdf_rectify_photos_lens": (_int, [_fp, _int, _int, _int, _int, _fp, _fp, _int, _int, _int, _fp, _float, _float, _fp, _fp,
                                          _fp]),
    "svbrdf_rectify_lens_grad_workspace_bytes": (_size, [_int] * 3),
    # src, format, P, Hs, Ws, matrices, lens, Hd, Wd, k, lut, clip_lo, clip_hi, grad_values, grad_matrices, grad_lens, ws,
    # bytes, stream
    "svbrdf_rectify_photos_lens_grad": (_int, [_fp, _int, _int, _int, _int, _fp, _fp, _int, _int, _int, _fp, _float, _float,
                                               _fp, _fp, _fp, _fp, _size, _fp]),
    "svbrdf_scale_inplace": (_int, [_fp, _fp, _size, _fp]),
    "svbrdf_debug_check_arith": (_int, [_u64, ctypes.c_uint, _float, _float, _fp, _fp]),
    "svbrdf_mix_materials": (_int, [_fp] * 4 + [_int] * 3 + [_fp]),
    "svbrdf_render_inputs": (_int, _INPUTS),
    "svbrdf_render_inputs_host_scenes": (_int, _INPUTS),
    "svbrdf_debug_copy": (_int, [_fp, _fp, _size, _fp]),
    "svbrdf_debug_launch_count": (_u64, []),
    "svbrdf_debug_clock_probe": (_int, [_fp, _u64, _fp]),
    "svbrdf_render_fwd_f64": (_int, [_fp] * 4 + _DIMS),
    "svbrdf_render_bwd_f64": (_int, [_fp] * 5 + _DIMS),
    "svbrdf_render_bwd_jvp_f64": (_int, [_fp] * 7 + _DIMS),
}
# What differs between the modes of a photo entry (photo_loss), keyed by the extra output the entry produces:
#   suffix       between "svbrdf_[head_]photo_loss" and "_fwd_bwd" (without an extra output the weighted entries have a
#                name of their own, "_weighted", and the unweighted ones alone take no (weights, planes))
#   workspace    the library function that sizes its scratch
#   always_grad  the kernel always forms the map gradient, `want_grad` only decides whether it is returned; else
#                `want_grad` picks the forward-only kernel
#   by_value     a *_host_scenes form exists; else a host table is uploaded
_PhotoMode = collections.namedtuple("_PhotoMode", "suffix workspace always_grad by_value")
_PHOTO_MODES = {
    None: _PhotoMode("", "svbrdf_rendering_loss_workspace_bytes", False, True),
    "exposure": _PhotoMode("_exposure", "svbrdf_photo_exposure_workspace_bytes", True, False),
    "scenes": _PhotoMode("_scene_grad", "svbrdf_photo_scene_grad_workspace_bytes", True, False),
    "photos": _PhotoMode("_photo_grad", "svbrdf_rendering_loss_workspace_bytes", False, False),
}


def _load():
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(_SO):
            raise NativeLibraryError(
                "HIP extension not built: %s is missing. Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C svbrdf_estimation_amd/csrc`. There is no CPU fallback." % _SO)
        try:
            # torch is imported first on purpose: its bundled libamdhip64.so.7 is then the
            # one HIP runtime of the process and our NEEDED entry resolves to it by SONAME,
            # so the stream handles torch hands us belong to the runtime that launches.
            lib = ctypes.CDLL(_SO)
        except OSError as e:  # pragma: no cover
            raise NativeLibraryError("cannot load %s: %s" % (_SO, e))
        for name, (restype, argtypes) in SIGNATURES.items():
            if not hasattr(lib, name):
                if "photo_loss" in name or "photo_exposure" in name or "photo_scene_grad" in name or "photo_fit" in name or "rectify" in name:    # joined ABI version 8 without a bump: an older build lacks them
                    raise NativeLibraryError("%s lacks %s (a build of ABI version 8 older than this binding) -- rebuild"
                                             % (_SO, name))
                raise NativeLibraryError("%s does not export %s -- rebuild" % (_SO, name))
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        v = lib.svbrdf_abi_version()
        if v != ABI_VERSION:
            raise NativeLibraryError("ABI mismatch: library %d, binding %d -- rebuild" % (v, ABI_VERSION))
        _lib = lib
    return _lib


def _check(rc, what):
    if rc != 0:
        msg = _load().svbrdf_last_error()
        raise NativeLibraryError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else "?"))


def _call(entry, device, *args, stream=None):
    """THE call into the library.  `entry`, a key of SIGNATURES, is looked up on the loaded library and called with `device`
    selected, `args` and -- as its last argument -- the current raw stream of `device` (or `stream`, a raw handle of the
    caller's own); a non-zero status raises NativeLibraryError under that same name.  device=None: a host-only entry,
    nothing to select and no stream to pass."""
    fn = getattr(_load(), entry)
    if device is None:
        rc = fn(*args)
    else:
        with _on_device(device):
            rc = fn(*args, _stream(device) if stream is None else ctypes.c_void_p(stream))
    _check(rc, entry)


def make_xrow_host(W):
    """torch.linspace(-1, 1, W) bit pattern of the reference's CPU path (renderers.py:73)."""
    buf = (ctypes.c_float * W)()
    _call("svbrdf_make_xrow", None, ctypes.cast(buf, _fp), W)
    return torch.tensor(list(buf), dtype=torch.float32)


def _require_device_f32(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise NativeLibraryError(
            "%s is on %s: the MI355X engine only computes on a ROCm device (no CPU fallback)" % (name, t.device))
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32 (got %s)" % (name, t.dtype))


def xrow(device, W):
    key = (device.index, W)
    t = _xrow_cache.get(key)
    if t is None:
        t = make_xrow_host(W).to(device)
        _xrow_cache[key] = t
    return t


def _workspace(device, nbytes):
    # one scratch buffer per (device, stream): calls on different streams never share it
    key = (device.index, _raw_stream(device))
    t = _workspace_cache.get(key)
    if t is None or t.numel() * 8 < nbytes:
        # zero-initialised once; every completed kernel leaves it zeroed (see svbrdf_hip.h)
        t = torch.zeros((max(nbytes, 64) + 7) // 8, dtype=torch.int64, device=device)
        _workspace_cache[key] = t
    return t


def _raw_stream(device):
    return torch._C._cuda_getCurrentRawStream(device.index if device.index is not None else torch.cuda.current_device())


def _stream(device):
    return ctypes.c_void_p(_raw_stream(device))


class _on_device:
    """`with torch.cuda.device(d)` only when d is not already current (the common case costs ~nothing)"""

    __slots__ = ("ctx",)

    def __init__(self, device):
        self.ctx = None if device.index == torch.cuda.current_device() else torch.cuda.device(device)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


# How one entry family takes its scene table -- the rule of _scene_table as data, with the family's own wording:
#   shared         True: a HOST [S,9] table, the same S scenes for every map, is accepted; else the ValueError that refuses it
#   always_device  the entries take a device table only: a host table is copied over (a plain copy) whatever its size
#   dtype_note     appended to "scenes must be float32 (got ...)"
#   elsewhere      the ValueError for a device table that does not live with the maps ({}: its device, the maps')
#   pair           None, or the two ValueErrors of the second per-row table that travels with the scenes (size or dtype;
#                  not on the scenes' side)
_TableRule = collections.namedtuple("_TableRule", "shared always_device dtype_note elsewhere pair")
_RENDER_TABLE = _TableRule(True, False, "", "scenes are on {}, the maps on {}: a device scene table must live with the maps", None)
_F64_TABLE = _RENDER_TABLE._replace(
    always_device=True, elsewhere="scenes are on {}, the maps on {}",
    dtype_note=": positions and colours are float32 in the reference whatever the maps' dtype (torch.Tensor(...), "
               "renderers.py:79,91,98)")
_INPUTS_TABLE = _TableRule("render_inputs needs one scene row per photo: scenes must be [B,S,9]", False, "",
                           "device scene / noise tables must live with the maps",
                           ("noise_std must be a float32 tensor of B*S = %d levels",
                            "scenes and noise_std must both be on the host or both on the maps' device"))
_LOSS_TABLE = _TableRule("the loss needs one scene table per batch item: scenes must be [B,S,9]", False, "",
                         "input, target and scenes must be on the same device", None)
_PHOTO_TABLE = _LOSS_TABLE._replace(shared="the loss needs one scene row per photo: scenes must be [B,S,9]",
                                    elsewhere="input, photos and scenes must be on the same device")


def _scene_table(rule, maps, scenes, pair=None, channels=12):
    """THE hand-over of a scene table to a launch on the device of `maps` ([B,channels,H,W], H = W), by `rule` (above).
    `scenes` is fp32 [B,S,9], or on the host [S,9] = the same S scenes for every map.  A HOST table of at most
    host_scenes_max_rows() rows rides in the launch's kernel-argument block: no copy.  A larger one is uploaded through
    the pinned ring, shared rows expanded per map first, and `pair` (one fp32 value per row, on the scenes' side) with
    it.  A device table must live with the maps.
    -> (table, B, S, H, W, on_host, shared, pair): contiguous tensors; on_host: `table` goes by value (the *_host_scenes
    entries), with `shared` its rows serve every map."""
    if not isinstance(scenes, torch.Tensor):
        raise TypeError("scenes must be a torch.Tensor")
    if maps.dim() != 4 or maps.shape[1] != channels:
        raise ValueError("maps must be [B,%d,H,W], got %s" % (channels, tuple(maps.shape)))
    B, _, H, W = maps.shape
    if H != W:
        raise ValueError("H must equal W (got %dx%d): the reference transposes the x grid, renderers.py:75" % (H, W))
    on_host = not scenes.is_cuda
    shared = on_host and scenes.dim() == 2 and scenes.shape[1] == 9
    if shared:
        if rule.shared is not True:
            raise ValueError(rule.shared)
    elif scenes.dim() != 3 or scenes.shape[0] != B or scenes.shape[2] != 9:
        raise ValueError("scenes must be [B,S,9], got %s for B=%d" % (tuple(scenes.shape), B))
    S = scenes.shape[-2]
    if scenes.dtype != torch.float32:
        raise TypeError("scenes must be float32 (got %s)%s" % (scenes.dtype, rule.dtype_note))
    if pair is not None:
        if not isinstance(pair, torch.Tensor) or pair.dtype != torch.float32 or pair.numel() != B * S:
            raise ValueError(rule.pair[0] % (B * S))
        if pair.is_cuda == on_host:
            raise ValueError(rule.pair[1])
    device = maps.device
    if on_host and (rule.always_device or (S if shared else B * S) > host_scenes_max_rows()):
        if shared:
            scenes, shared = scenes.unsqueeze(0).expand(B, S, 9), False
        if rule.always_device:
            scenes = scenes.to(device)
        else:
            scenes = upload_scene_table(scenes, device)
            pair = upload_scene_table(pair.reshape(-1), device) if pair is not None else None
        on_host = False
    if not on_host and (scenes.device != device or (pair is not None and pair.device != device)):
        # (the raw pointer would be dereferenced by a kernel running on `device`)
        raise ValueError(rule.elsewhere.format(scenes.device, device))
    if not scenes.is_contiguous():
        scenes = scenes.contiguous()
    if pair is not None and not pair.is_contiguous():
        pair = pair.contiguous()
    return scenes, B, S, H, W, on_host, shared, pair


def loss_scene_table(input, scenes, head=False):
    """The scene table of a rendering_loss call on `input`, handed over ahead of it: the device table a large host table
    was uploaded to, else the table itself.  For a caller that launches more than once on one table
    (losses.RenderingLoss when the target's gradient is wanted too): one upload serves all its launches."""
    return _scene_table(_LOSS_TABLE, input, scenes, channels=9 if head else 12)[0]


def _require_device_float(t, name):
    """float32 (the engine's path) or float64 (the reference's mixed-precision behaviour for double maps)"""
    if isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.is_cuda:
        return True
    _require_device_f32(t, name)
    return False


def _render(maps, scenes, bwd, grad_out=None):
    """the one body of render_fwd and render_bwd (`bwd`: with the cotangent `grad_out`), float32 and float64 maps"""
    f64 = _require_device_float(maps, "maps")
    if not maps.is_contiguous():
        maps = maps.contiguous()
    if bwd:
        if not f64:
            _require_device_f32(grad_out, "grad_out")
        elif grad_out.dtype != torch.float64 or not grad_out.is_cuda:
            raise TypeError("grad_out must be a float64 device tensor for float64 maps")
        if not grad_out.is_contiguous():
            grad_out = grad_out.contiguous()
    table, B, S, H, W, on_host, shared, _ = _scene_table(_F64_TABLE if f64 else _RENDER_TABLE, maps, scenes)
    if bwd:
        if grad_out.numel() != B * S * 3 * H * W or grad_out.shape[-2:] != maps.shape[-2:]:
            raise ValueError("grad_out must be [B,S,3,H,W]")
        out = torch.empty_like(maps)
        results = (grad_out.data_ptr(), out.data_ptr())
    else:
        out = torch.empty((B, S, 3, H, W), dtype=maps.dtype, device=maps.device)
        results = (out.data_ptr(),)
    # svbrdf_render_{fwd,bwd}[_f64 | _host_scenes]; the by-value entries take the shared flag behind the table
    _call("svbrdf_render_" + ("bwd" if bwd else "fwd") + ("_f64" if f64 else "_host_scenes" if on_host else ""), maps.device,
          maps.data_ptr(), table.data_ptr(), *((int(shared),) if on_host else ()), xrow(maps.device, W).data_ptr(), *results,
          B, S, H, W)
    return out


def render_bwd_jvp_f64(maps, tangent, scenes, grad_out):
    """Second order (svbrdf_render_bwd_jvp_f64): for float64 ``maps`` [B,12,H,W], a direction ``tangent`` of the same
    shape and ``grad_out`` [B,S,3,H,W] -> (d/dmaps <J^T grad_out, tangent> [B,12,H,W],  J tangent [B,S,3,H,W]): the two
    products autograd needs to differentiate through the backward of ``render`` (create_graph=True)."""
    for t, name in ((maps, "maps"), (tangent, "tangent"), (grad_out, "grad_out")):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.is_cuda):
            raise TypeError("%s must be a float64 tensor on a ROCm device" % name)
    maps, tangent, grad_out = maps.contiguous(), tangent.contiguous(), grad_out.contiguous()
    table, B, S, H, W = _scene_table(_F64_TABLE, maps, scenes)[:5]
    if tangent.shape != maps.shape or tangent.device != maps.device:
        raise ValueError("tangent must have the maps' shape and device")
    if grad_out.numel() != B * S * 3 * H * W or grad_out.shape[-2:] != maps.shape[-2:] or grad_out.device != maps.device:
        raise ValueError("grad_out must be [B,S,3,H,W] on the maps' device")
    gm_t = torch.empty_like(maps)
    out_t = torch.empty((B, S, 3, H, W), dtype=torch.float64, device=maps.device)
    _call("svbrdf_render_bwd_jvp_f64", maps.device, maps.data_ptr(), tangent.data_ptr(), table.data_ptr(),
          xrow(maps.device, W).data_ptr(), grad_out.data_ptr(), gm_t.data_ptr(), out_t.data_ptr(), B, S, H, W)
    return gm_t, out_t


def render_fwd(maps, scenes):
    """K1: maps [B,12,H,W]; scenes [B,S,9] on the device, or on the HOST as [B,S,9] / [S,9] (the same S scenes for
    every map): a host table of at most host_scenes_max_rows() rows travels with the launch (one dispatch, no copy
    command).  -> renderings [B,S,3,H,W].  float64 maps take the mixed-precision path of the reference (float32
    geometry, double shading: svbrdf_render_fwd_f64) and return float64."""
    return _render(maps, scenes, False)


def device_philox_state(device, generator=None):
    """(seed, offset) for one launch of a counter-based noise kernel, taken from -- and advancing -- torch's generator of
    `device` the way torch's own device random ops do: ``torch.cuda.manual_seed`` therefore controls the sensor noise of
    ``render_inputs`` like it controls ``torch.randn(..., device=...)``.  The kernel uses the offset as the upper counter
    words, so advancing it by one unit (4, the granularity torch requires) gives the next launch a disjoint counter space."""
    gen = generator if generator is not None else torch.cuda.default_generators[
        device.index if device.index is not None else torch.cuda.current_device()]
    seed, offset = int(gen.initial_seed()), int(gen.get_offset())
    gen.set_offset(offset + 4)
    return seed & 0xFFFFFFFFFFFFFFFF, offset & 0xFFFFFFFFFFFFFFFF


def render_inputs(maps, scenes, noise_std=None, seed=0, offset=0):
    """K1 + sensor-noise epilogue (svbrdf_render_inputs*): maps [B,12,H,W] device; scenes [B,S,9] and noise_std [B,S]
    (or None: clamp only) BOTH on the host (at most host_scenes_max_rows() rows: they ride in the launch's argument block)
    or both on the maps' device -> clamp(render + noise_std * N(0,1), 0, 1) [B,S,3,H,W], ONE launch, each photo written
    once.  The normal field is a pure function of (seed, offset, element index): see include/svbrdf_hip.h."""
    _require_device_f32(maps, "maps")
    if not maps.is_contiguous():
        maps = maps.contiguous()
    table, B, S, H, W, on_host, _, sig = _scene_table(_INPUTS_TABLE, maps, scenes, noise_std)
    out = torch.empty((B, S, 3, H, W), dtype=torch.float32, device=maps.device)
    _call("svbrdf_render_inputs_host_scenes" if on_host else "svbrdf_render_inputs", maps.device,
          maps.data_ptr(), table.data_ptr(), sig.data_ptr() if sig is not None else None,
          ctypes.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF), ctypes.c_ulonglong(int(offset) & 0xFFFFFFFFFFFFFFFF),
          xrow(maps.device, W).data_ptr(), out.data_ptr(), B, S, H, W)
    return out


def debug_copy(dst, src):
    """svbrdf_debug_copy: dst[:] = src as a streaming float4 copy kernel on the current stream (measurement aid: the copy
    bandwidth of this box, bench.py / tests/test_gpu_perf_guard.py)"""
    _require_device_f32(dst, "dst")
    _require_device_f32(src, "src")
    if dst.numel() != src.numel() or not dst.is_contiguous() or not src.is_contiguous() or dst.device != src.device:
        raise ValueError("debug_copy needs two contiguous tensors of one size on one device")
    _call("svbrdf_debug_copy", dst.device, dst.data_ptr(), src.data_ptr(), dst.numel())
    return dst


def launch_count():
    """kernels enqueued by libsvbrdf_hip.so in this process so far (svbrdf_debug_launch_count)"""
    return int(_load().svbrdf_debug_launch_count())


def render_bwd(maps, scenes, grad_out):
    """K2: adjoint of render_fwd (same `scenes` forms) -> grad_maps [B,12,H,W]."""
    return _render(maps, scenes, True, grad_out)


def _ragged_offsets(counts, B, R, device):
    counts = [int(c) for c in counts]
    if len(counts) != B or any(c < 0 for c in counts) or sum(counts) != R:
        raise ValueError("counts must hold one non-negative render count per map and sum to the number of scenes")
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    return torch.tensor(off, dtype=torch.int32).to(device)


def _render_ragged(maps, scenes, counts, bwd, grad_out=None):
    """the one body of render_fwd_ragged and render_bwd_ragged (`bwd`: with the cotangent `grad_out` [R,3,H,W])"""
    for t, name in ((maps, "maps"), (scenes, "scenes")) + (((grad_out, "grad_out"),) if bwd else ()):
        _require_device_f32(t, name)
    maps, scenes = maps.contiguous(), scenes.contiguous()
    if maps.dim() != 4 or maps.shape[1] != 12 or maps.shape[2] != maps.shape[3] or scenes.dim() != 2 or scenes.shape[1] != 9:
        raise ValueError("maps must be [B,12,H,H] and scenes [R,9]")
    B, _, H, W = maps.shape
    R = scenes.shape[0]
    if bwd:
        grad_out = grad_out.contiguous()
        if tuple(grad_out.shape) != (R, 3, H, W):
            raise ValueError("grad_out must be [R,3,H,W]")
    off = _ragged_offsets(counts, B, R, maps.device)
    out = torch.empty_like(maps) if bwd else torch.empty((R, 3, H, W), dtype=torch.float32, device=maps.device)
    _call("svbrdf_render_bwd_ragged" if bwd else "svbrdf_render_fwd_ragged", maps.device, maps.data_ptr(), scenes.data_ptr(),
          off.data_ptr(), xrow(maps.device, W).data_ptr(), *((grad_out.data_ptr(),) if bwd else ()), out.data_ptr(), B, R, H, W)
    return out


def render_fwd_ragged(maps, scenes, counts):
    """K1, ragged: maps [B,12,H,W], scenes [R,9] grouped by map, counts[b] renders for map b -> [R,3,H,W]."""
    return _render_ragged(maps, scenes, counts, False)


def render_bwd_ragged(maps, scenes, counts, grad_out):
    """K2, ragged: adjoint of render_fwd_ragged -> grad_maps [B,12,H,W] (zeros for a map without renders)."""
    return _render_ragged(maps, scenes, counts, True, grad_out)


def _fused_loss_call(entry, input, other, scenes, floats, want_grad, B, S, H, W, extra=(), more_grads=(),
                     workspace_bytes="svbrdf_rendering_loss_workspace_bytes", n_losses=1, workspace_lead=()):
    """One launch of the fused-loss entry point `entry`: contiguous device tensors `input` and `other` (target maps or
    photos), the scene table as _scene_table returned it, `floats` = eps (and l1_weight, eps_l1 for the entries that take
    them), `extra` = what the entry takes between `other` and the scene table (the weighted photo entries: weights
    pointer, plane count; the exposure entries: the exposure pointer behind them), `more_grads` = the output pointers it
    takes behind the gradient (the exposure entries: grad_exposure), `workspace_bytes` = the library function that sizes
    its scratch, `workspace_lead` = what that function takes in front of B, S, H, W (the steps entry: n_steps), `n_losses` =
    the length of the loss tensor (the steps entry: one per step).  `want_grad` None: the entry takes no gradient pointer.
    -> (loss [n_losses] device tensor, grad like `input` or None)"""
    ws = _workspace(input.device, getattr(_load(), workspace_bytes)(*workspace_lead, B, S, H, W))
    loss = torch.empty(n_losses, dtype=torch.float32, device=input.device)
    grad = torch.empty_like(input) if want_grad else None
    grad_ptr = () if want_grad is None else (grad.data_ptr() if want_grad else None,)
    xr = xrow(input.device, W)
    hook = _launch_hook
    if hook is not None:
        hook("begin")
    try:
        _call(entry, input.device, input.data_ptr(), other.data_ptr(), *extra, scenes.data_ptr(), xr.data_ptr(), *floats,
              loss.data_ptr(), *grad_ptr, *more_grads, ws.data_ptr(), ws.numel() * 8, B, S, H, W)
    except NativeLibraryError:
        # a failed launch may leave partial sums / arrival counts behind: the scratch contract ("every completed
        # call leaves it zeroed") only covers completed calls, so restore it before reporting the error
        ws.zero_()
        raise
    finally:
        if hook is not None:
            hook("end")
    return loss, grad


def rendering_loss(input, target, scenes, eps=0.1, want_grad=True, l1_weight=0.0, eps_l1=0.01, head=False):
    """K3: fused rendering loss (+ d loss/d input); with l1_weight != 0 the SVBRDF L1 loss is folded
    in (MixedLoss); with head=True `input` is the generator's [B,9,H,W] post-tanh output and the
    network head is decoded in the kernel.  Returns (loss [1] device tensor, grad or None)."""
    _require_device_f32(input, "input")
    _require_device_f32(target, "target")
    if head:
        if input.dim() != 4 or input.shape[1] != 9 or (input.shape[0],) + tuple(input.shape[2:]) != \
                (target.shape[0],) + tuple(target.shape[2:]):
            raise ValueError("head=True needs input [B,9,H,W] and target [B,12,H,W]")
    elif input.shape != target.shape:
        raise ValueError("input and target shapes differ: %s vs %s" % (tuple(input.shape), tuple(target.shape)))
    if target.device != input.device:
        raise ValueError("input, target and scenes must be on the same device")
    scenes, B, S, H, W, on_host = _scene_table(_LOSS_TABLE, target, scenes)[:6]
    if on_host:     # the by-value entries exist with the L1 arguments only
        entry = "svbrdf_head_loss_fwd_bwd_host_scenes" if head else "svbrdf_mixed_loss_fwd_bwd_host_scenes"
    elif head:
        entry = "svbrdf_head_loss_fwd_bwd"
    elif l1_weight != 0.0:
        entry = "svbrdf_mixed_loss_fwd_bwd"
    else:
        entry = "svbrdf_rendering_loss_fwd_bwd"
    floats = (ctypes.c_float(eps),)
    if entry != "svbrdf_rendering_loss_fwd_bwd":
        floats += (ctypes.c_float(l1_weight), ctypes.c_float(eps_l1))
    return _fused_loss_call(entry, input.contiguous(), target.contiguous(), scenes, floats, want_grad, B, S, H, W)


def _checked_weights(weights, device, B, S, H, W):
    """per-pixel weights of a photo entry, float32 [B,S,H,W] or [B,1,H,W] on `device` -> contiguous (the caller keeps the
    result alive until the launch is enqueued, stream-ordered)"""
    _require_device_f32(weights, "weights")
    if weights.device != device:
        raise ValueError("input, photos and weights must be on the same device")
    if tuple(weights.shape) not in ((B, S, H, W), (B, 1, H, W)):
        raise ValueError("weights must be [B,S,H,W] = %s or [B,1,H,W] for these maps and photos, got %s"
                         % ((B, S, H, W), tuple(weights.shape)))
    return weights.contiguous()


def _photo_operands(maps, photos, scenes, weights, channels=12):
    """The operands every photo entry takes beside its maps (float32 device [B,channels,H,W], the caller's check), checked:
    photos float32 [B,S,3,H,W] on the maps' device, the scene table by _PHOTO_TABLE's rule, weights as _checked_weights takes
    them or None.  -> (table, B, S, H, W, on_host: the table is still on the host, small enough to go by value; photos and
    weights contiguous, for the caller's frame to hold until the launch is enqueued; (weights pointer, planes) as the
    weighted entries take them, (None, 0) without weights)"""
    _require_device_f32(photos, "photos")
    if photos.device != maps.device:
        raise ValueError("input, photos and scenes must be on the same device")
    scenes, B, S, H, W, on_host = _scene_table(_PHOTO_TABLE, maps, scenes, channels=channels)[:6]
    if tuple(photos.shape) != (B, S, 3, H, W):
        raise ValueError("photos must be [B,S,3,H,W] = %s for these maps and scenes, got %s"
                         % ((B, S, 3, H, W), tuple(photos.shape)))
    if weights is None:
        return scenes, B, S, H, W, on_host, photos.contiguous(), None, (None, 0)
    weights = _checked_weights(weights, maps.device, B, S, H, W)
    return scenes, B, S, H, W, on_host, photos.contiguous(), weights, (weights.data_ptr(), int(weights.shape[1]))


def photo_loss(input, photos, scenes, eps=0.1, want_grad=True, head=False, weights=None, exposure=None,
               want_exposure_grad=False, want_scene_grad=False, want_photo_grad=False):
    """Fused photo loss (svbrdf_photo_loss_fwd_bwd*): mean |log(render(scenes[b,s], input[b]) + eps) - log(photos[b,s] + eps)|
    and d loss/d input in ONE launch.  input [B,12,H,W] and photos [B,S,3,H,W] device fp32; scenes [B,S,9] fp32 on the
    maps' device, or on the HOST (at most host_scenes_max_rows() rows ride in the launch's argument block, a larger table
    is uploaded).  With head=True `input` is the generator's [B,9,H,W] post-tanh output, the network head is decoded in
    the kernel (svbrdf_head_photo_loss_fwd_bwd*) and the gradient has its 9 channels.  ``weights``: per-pixel confidence
    in [0, 1], float32 [B,S,H,W] (one plane per photo) or [B,1,H,W] (one per item, shared by its photos) on the maps'
    device -- the svbrdf_*photo_loss_weighted_fwd_bwd* entries: sum of w |..| over B S 3 H W, a weight of exactly 0
    excuses the photo value under it (NaN included).  Returns (loss [1] device tensor, grad or None).

    ``exposure``: a positive float32 gain per photo and colour channel, [B,S,3] on the maps' device, that multiplies the
    light colour of its scene row -- the svbrdf_*photo_loss_exposure_fwd_bwd entries, still ONE launch, with or without
    ``weights``.  They are forward + adjoint with the table in device memory: a host table is uploaded, and ``want_grad``
    only decides whether the map gradient is returned.  Returns (loss, grad or None, grad_exposure [B,S,3] or None --
    ``want_exposure_grad``).  A gain that is NaN, infinite or <= 0 gives a NaN loss and an all-NaN grad_exposure.

    ``want_scene_grad=True`` (without ``exposure``: a gain is applied to the table in front of the call): the
    svbrdf_*photo_loss_scene_grad_fwd_bwd entries, still ONE launch, with or without ``weights``, forward + adjoint with the
    table in device memory like the exposure entries.  Returns (loss, grad or None, grad_scenes [B,S,9]): d loss/d scenes,
    camera xyz | light xyz | light rgb.  Loss and map gradient equal the entries' without it bit for bit.  A colour that is
    NaN, infinite or <= 0 gives a NaN loss; a NaN loss comes with an all-NaN grad_scenes.

    ``want_photo_grad=True`` (without ``exposure`` and without ``want_scene_grad``): the
    svbrdf_*photo_loss_photo_grad_fwd_bwd entries, still ONE launch, with or without ``weights``, table in device memory (a
    host table is uploaded).  Returns (loss, grad or None, grad_photos [B,S,3,H,W]): d loss/d photos =
    -(w/N) sign(delta) / (photos + eps) for upstream gradient 1.  Loss and map gradient equal the entries' without it bit for
    bit; ``want_grad=False`` runs the forward-only scene loop (loss and grad_photos: what a registration stage needs)."""
    if want_scene_grad and exposure is not None:
        raise ValueError("want_scene_grad takes no exposure: multiply the table's colour columns by the gains instead")
    if want_photo_grad and (exposure is not None or want_scene_grad):
        raise ValueError("want_photo_grad takes neither an exposure nor want_scene_grad: those combinations are the composed "
                         "definition's (losses.composed_photo_loss); a constant gain multiplies the table's colour columns")
    third = "photos" if want_photo_grad else "scenes" if want_scene_grad else "exposure" if exposure is not None else None
    suffix, workspace, always_grad, by_value = _PHOTO_MODES[third]
    _require_device_f32(input, "input")
    scenes, B, S, H, W, on_host, photos, weights, extra = _photo_operands(input, photos, scenes, weights, 9 if head else 12)
    if third is None:
        if weights is None:
            extra = ()
        else:
            suffix = "_weighted"
    elif third == "exposure":
        _require_device_f32(exposure, "exposure")
        if exposure.device != input.device:
            raise ValueError("input, photos and exposure must be on the same device")
        if tuple(exposure.shape) != (B, S, 3):
            raise ValueError("exposure must be [B,S,3] = %s for these maps and photos, got %s" % ((B, S, 3), tuple(exposure.shape)))
        exposure = exposure.contiguous()
        extra += (exposure.data_ptr(),)
    if on_host and not by_value:
        scenes, on_host = upload_scene_table(scenes, input.device), False
    out, more = None, ()
    if third is not None:       # the mode's own output, like the operand it is the gradient of (the table: the device's)
        like = photos if third == "photos" else scenes if third == "scenes" else exposure if want_exposure_grad else None
        if like is not None:
            out = torch.empty_like(like)
        more = (None if out is None else out.data_ptr(),)
    loss, grad = _fused_loss_call(
        ("svbrdf_head_photo_loss" if head else "svbrdf_photo_loss") + suffix + "_fwd_bwd" + ("_host_scenes" if on_host else ""),
        input.contiguous(), photos, scenes, (ctypes.c_float(eps),), want_grad or always_grad, B, S, H, W, extra, more, workspace)
    return (loss, grad) if third is None else (loss, grad if want_grad else None, out)


def photo_fit_adam_scalars(lr, beta1, beta2, step):
    """(c1, c2, step_size, rsb2) of Adam's step `step` as float32 values (svbrdf_photo_fit_adam_scalars: host only, derived
    in double from the float32 arguments the step entry takes, each rounded once)"""
    out = (ctypes.c_float * 4)()
    _call("svbrdf_photo_fit_adam_scalars", None, ctypes.c_float(lr), ctypes.c_float(beta1), ctypes.c_float(beta2), int(step),
          ctypes.cast(out, _fp))
    return tuple(out)


def _fit_operands(maps, exp_avg, exp_avg_sq, photos, scenes, weights):
    """The operands of a fit entry, checked: maps and state contiguous float32 [B,12,H,W] device tensors (updated in place);
    photos, scenes, weights as photo_loss takes them; a host table is uploaded (the entries take a device table).
    -> (the device table, (B, S, H, W), `extra`: what the entries take between exp_avg and the table, `keep`: the tensors
    behind extra's pointers, for the caller's frame to hold until the launch is enqueued)"""
    for t, name in ((maps, "maps"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _require_device_f32(t, name)
        if not t.is_contiguous() or t.shape != maps.shape or t.device != maps.device:
            raise ValueError("%s is updated in place: a contiguous tensor of the maps' shape on their device" % name)
    scenes, B, S, H, W, on_host, photos, weights, planes = _photo_operands(maps, photos, scenes, weights)
    if on_host:
        scenes = upload_scene_table(scenes, maps.device)
    return scenes, (B, S, H, W), (exp_avg_sq.data_ptr(), photos.data_ptr()) + planes, (photos, weights)


def _adam_floats(eps, bounds, lr, betas, adam_eps, step):
    """what the fit entries take between xrow and the loss pointer, up to Adam's t"""
    return (ctypes.c_float(eps), None if bounds is None else ctypes.cast(bounds, _fp), ctypes.c_float(lr),
            ctypes.c_float(betas[0]), ctypes.c_float(betas[1]), ctypes.c_float(adam_eps), int(step))


def photo_fit_adam_step(maps, exp_avg, exp_avg_sq, photos, scenes, step, lr=1e-2, betas=(0.9, 0.999), adam_eps=1e-8,
                        bounds=None, eps=0.1, weights=None, want_grad=False, want_scene_grad=False):
    """One step of a photo fit (svbrdf_photo_fit_adam_step): the (weighted) photo loss at `maps`, its gradient and the Adam
    update of `maps`, `exp_avg`, `exp_avg_sq` -- contiguous float32 [B,12,H,W] device tensors, updated IN PLACE -- in ONE
    launch.  photos, scenes, eps, weights: as photo_loss (a host table is uploaded: the entry takes a device table).
    `step`: Adam's t, 1 for the first update.  `bounds`: None, or a ctypes array of 24 floats on the host, (lo, hi) per
    channel.  -> (loss at the maps before the update, [1] device tensor; the gradient, or None without `want_grad`: it is
    then never written).

    ``want_scene_grad=True``: svbrdf_photo_fit_adam_step_scene_grad, the same step and still ONE launch
    -> (loss, grad or None, grad_scenes [B,S,9]): d loss / d scenes at the maps before the update, camera xyz | light xyz |
    light rgb, as photo_loss(want_scene_grad=True) returns it bit for bit.  A NaN loss comes with an all-NaN grad_scenes;
    the maps are updated whatever the loss is."""
    scenes, dims, extra, keep = _fit_operands(maps, exp_avg, exp_avg_sq, photos, scenes, weights)
    floats = _adam_floats(eps, bounds, lr, betas, adam_eps, step)
    if want_scene_grad:
        grad_scenes = torch.empty_like(scenes)
        loss, grad = _fused_loss_call("svbrdf_photo_fit_adam_step_scene_grad", maps, exp_avg, scenes, floats, want_grad, *dims,
                                      extra, (grad_scenes.data_ptr(),), "svbrdf_photo_scene_grad_workspace_bytes")
        return loss, grad, grad_scenes
    return _fused_loss_call("svbrdf_photo_fit_adam_step", maps, exp_avg, scenes, floats, want_grad, *dims, extra)


def photo_fit_smooth_adam_step(maps, maps_out, exp_avg, exp_avg_sq, photos, scenes, step, smooth, lr=1e-2, betas=(0.9, 0.999),
                               adam_eps=1e-8, bounds=None, eps=0.1, weights=None, want_grad=False, want_scene_grad=False):
    """One step of a photo fit with the smoothness prior across pixels (svbrdf_photo_fit_smooth_adam_step): the step of
    photo_fit_adam_step with the gradient of sum_ch smooth[ch] TV(maps[:, ch]) / (B H W) added to the photo gradient, in
    ONE launch, OUT OF PLACE for the maps: `maps` is only read, `maps_out` -- a contiguous float32 device tensor of the
    same shape that shares no memory with `maps` -- receives the updated maps; `exp_avg`, `exp_avg_sq` are updated in
    place.  `smooth`: a ctypes array of 12 floats on the host, one lambda per plane, finite and >= 0; a plane with 0
    skips the term.  The other arguments as photo_fit_adam_step.  -> (photo loss at `maps`, [1] device tensor -- the
    prior's own value is not part of it, fitting.smoothness gives it --; the gradient WITH the prior's term, or None).

    ``want_scene_grad=True``: svbrdf_photo_fit_smooth_adam_step_scene_grad -> (loss, grad or None, grad_scenes [B,S,9]),
    grad_scenes bit for bit photo_fit_adam_step's: the prior does not depend on the table."""
    scenes, dims, extra, keep = _fit_operands(maps, exp_avg, exp_avg_sq, photos, scenes, weights)
    _require_device_f32(maps_out, "maps_out")
    if not maps_out.is_contiguous() or maps_out.shape != maps.shape or maps_out.device != maps.device:
        raise ValueError("maps_out receives the updated maps: a contiguous tensor of the maps' shape on their device")
    if smooth is None:
        raise ValueError("smooth must be a ctypes array of 12 floats")
    eps_, *adam = _adam_floats(eps, bounds, lr, betas, adam_eps, step)
    floats = (eps_, ctypes.cast(smooth, _fp), *adam)
    extra = (exp_avg.data_ptr(),) + extra
    if want_scene_grad:
        grad_scenes = torch.empty_like(scenes)
        loss, grad = _fused_loss_call("svbrdf_photo_fit_smooth_adam_step_scene_grad", maps, maps_out, scenes, floats, want_grad,
                                      *dims, extra, (grad_scenes.data_ptr(),), "svbrdf_photo_scene_grad_workspace_bytes")
        return loss, grad, grad_scenes
    return _fused_loss_call("svbrdf_photo_fit_smooth_adam_step", maps, maps_out, scenes, floats, want_grad, *dims, extra)


PHOTO_FIT_MAX_STEPS = 64        # SVBRDF_PHOTO_FIT_MAX_STEPS of include/svbrdf_hip.h


def photo_fit_adam_steps(maps, exp_avg, exp_avg_sq, photos, scenes, first_step, n_steps, lr=1e-2, betas=(0.9, 0.999),
                         adam_eps=1e-8, bounds=None, eps=0.1, weights=None):
    """`n_steps` consecutive steps of a photo fit in ONE launch (svbrdf_photo_fit_adam_steps), 1 <= n_steps <=
    PHOTO_FIT_MAX_STEPS: bit for bit what `n_steps` calls of photo_fit_adam_step with step = first_step, first_step + 1,
    ... leave in `maps`, `exp_avg`, `exp_avg_sq`, the other arguments as there.  -> float32 [n_steps] device tensor: the loss
    before each update.  No gradient is returned."""
    if not 1 <= int(n_steps) <= PHOTO_FIT_MAX_STEPS:
        raise ValueError("n_steps must lie in [1, %d], got %r" % (PHOTO_FIT_MAX_STEPS, n_steps))
    n_steps = int(n_steps)
    scenes, dims, extra, keep = _fit_operands(maps, exp_avg, exp_avg_sq, photos, scenes, weights)
    floats = _adam_floats(eps, bounds, lr, betas, adam_eps, first_step) + (n_steps,)
    return _fused_loss_call("svbrdf_photo_fit_adam_steps", maps, exp_avg, scenes, floats, None, *dims, extra,
                            workspace_bytes="svbrdf_photo_fit_steps_workspace_bytes", n_losses=n_steps,
                            workspace_lead=(n_steps,))[0]


def mix_materials(svbrdf0, svbrdf1, alpha):
    """K4: out[b] = mix(svbrdf0[b], svbrdf1[b], alpha[b]) (dataset.py:142-160) for [B,12,H,W] device tensors and a
    [B] device tensor of blend weights."""
    for t, name in ((svbrdf0, "svbrdf0"), (svbrdf1, "svbrdf1"), (alpha, "alpha")):
        _require_device_f32(t, name)
    if svbrdf0.dim() != 4 or svbrdf0.shape[1] != 12 or svbrdf0.shape != svbrdf1.shape:
        raise ValueError("svbrdf0 and svbrdf1 must both be [B,12,H,W]")
    B, _, H, W = svbrdf0.shape
    if alpha.numel() != B:
        raise ValueError("alpha must hold one weight per batch item")
    if svbrdf1.device != svbrdf0.device or alpha.device != svbrdf0.device:
        raise ValueError("svbrdf0, svbrdf1 and alpha must be on the same device")
    a, b, w = svbrdf0.contiguous(), svbrdf1.contiguous(), alpha.contiguous().view(-1)
    out = torch.empty_like(a)
    _call("svbrdf_mix_materials", a.device, a.data_ptr(), b.data_ptr(), w.data_ptr(), out.data_ptr(), B, H, W)
    return out


def _rectify_grad(entry, query, src, fmt, P, Hs, Ws, matrices, lens, Hd, Wd, k, lut, lo, hi, grad_values):
    """the one launch of a rectify gradient entry, float32 ``[P,9]`` rows out: towards the matrices, and with ``lens`` towards
    the lens rows too.  The scratch is the loss entries' (one buffer per device and stream, zeroed once, left zeroed by every
    call)."""
    _require_device_f32(grad_values, "grad_values")
    if tuple(grad_values.shape) != (P, 3, Hd, Wd) or not grad_values.is_contiguous() or grad_values.device != src.device:
        raise ValueError("grad_values must be contiguous [%d,3,%d,%d] on %s" % (P, Hd, Wd, src.device))
    ws = _workspace(src.device, getattr(_load(), query)(P, Hd, Wd))
    outs = tuple(torch.empty((P, 9), dtype=torch.float32, device=src.device) for _ in range(1 if lens is None else 2))
    _call(entry, src.device, src.data_ptr(), fmt, P, Hs, Ws, matrices.data_ptr(), *(() if lens is None else (lens.data_ptr(),)),
          Hd, Wd, k, None if lut is None else lut.data_ptr(), lo, hi, grad_values.data_ptr(), *(o.data_ptr() for o in outs),
          ws.data_ptr(), ws.numel() * 8)
    return outs


def rectify_grad_matrices(src, fmt, P, Hs, Ws, matrices, Hd, Wd, k, lut, lo, hi, grad_values):
    """svbrdf_rectify_photos_grad_matrices, ONE launch: the gradient of ``capture.rectify``'s values towards its float32
    ``[P,9]`` device matrices, from ``grad_values`` float32 ``[P,3,Hd,Wd]`` contiguous on the device of ``src``; the other
    arguments as ``capture.rectify`` hands them to the forward.  -> float32 ``[P,9]``"""
    return _rectify_grad("svbrdf_rectify_photos_grad_matrices", "svbrdf_rectify_grad_workspace_bytes", src, fmt, P, Hs, Ws,
                         matrices, None, Hd, Wd, k, lut, lo, hi, grad_values)[0]


def rectify_lens_grad(src, fmt, P, Hs, Ws, matrices, lens, Hd, Wd, k, lut, lo, hi, grad_values):
    """svbrdf_rectify_photos_lens_grad, ONE launch: the gradient of ``capture.rectify(..., lens=)``'s values towards its
    float32 ``[P,9]`` device matrices (through the lens's Jacobian) and towards its float32 ``[P,9]`` device lens rows, from
    ``grad_values`` as above.  -> (float32 ``[P,9]``, float32 ``[P,9]``)"""
    return _rectify_grad("svbrdf_rectify_photos_lens_grad", "svbrdf_rectify_lens_grad_workspace_bytes", src, fmt, P, Hs, Ws,
                         matrices, lens, Hd, Wd, k, lut, lo, hi, grad_values)


def clock_probe(out, ticks=300000, stream=None):
    """Measurement aid (svbrdf_debug_clock_probe): one wave spins for `ticks` ticks of the 100 MHz counter on
    `stream` (a torch.cuda.Stream; default: the current one) and writes shader cycles / ticks into `out`
    (device int64[2]).  cycles / ticks * 0.1 = shader clock in GHz under whatever else is running."""
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int64 and out.numel() >= 2):
        raise TypeError("out must be a device int64 tensor of at least 2 elements")
    _call("svbrdf_debug_clock_probe", out.device, out.data_ptr(), int(ticks),
          stream=stream.cuda_stream if stream is not None else None)
    return out


_host_rows = None


def host_scenes_max_rows():
    """largest B*S the *_host_scenes entry points take (the table rides in the launch's kernel-argument block)"""
    global _host_rows
    if _host_rows is None:
        _host_rows = int(_load().svbrdf_host_scenes_max_rows())
    return _host_rows


def scale_inplace_(data, scale):
    """data *= scale (a one-element device tensor) without a host sync; no-op kernel when scale == 1."""
    _require_device_f32(data, "data")
    _require_device_f32(scale, "scale")
    if not data.is_contiguous() or scale.numel() != 1:
        raise ValueError("scale_inplace_ needs a contiguous tensor and a one-element scale")
    _call("svbrdf_scale_inplace", data.device, data.data_ptr(), scale.data_ptr(), data.numel())
    return data


class _PinnedRing:
    """Truly asynchronous upload of the small per-call scene table.

    A pageable-memory ``hipMemcpyAsync`` stages through the runtime and makes the host wait for
    the stream (measured: the step time was host + GPU instead of max(host, GPU)).  The table
    is therefore copied into one of a few pinned slots and uploaded from there; a slot is
    reused only after the event recorded behind its upload has completed."""

    def __init__(self, depth=8):
        self.depth, self.slots, self.events, self.next = depth, [None] * depth, [None] * depth, 0

    def upload(self, host, device):
        i = self.next
        self.next = (i + 1) % self.depth
        if self.events[i] is not None:
            self.events[i].synchronize()            # normally long done: depth steps ago
        slot = self.slots[i]
        if slot is None or slot.numel() < host.numel():
            slot = torch.empty(max(host.numel(), 1024), dtype=torch.float32, pin_memory=True)
            self.slots[i] = slot
        view = slot[:host.numel()].view(host.shape)
        view.copy_(host)
        dev = view.to(device, non_blocking=True)
        ev = self.events[i] or torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self.events[i] = ev
        return dev


_rings = {}


def upload_scene_table(host_table, device):
    """[B,S,9] fp32 host tensor -> device tensor, without stalling the host on the stream."""
    if host_table.dtype != torch.float32:
        raise TypeError("scenes must be float32 (got %s)" % host_table.dtype)
    ring = _rings.get(device.index)
    if ring is None:
        ring = _rings[device.index] = _PinnedRing()
    return ring.upload(host_table.contiguous(), device)
