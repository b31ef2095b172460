"""Losses with the reference's names and semantics (development/multiImage_pytorch/losses.py).

``RenderingLoss(renderer).forward(input, target)`` (losses.py:21-52): per batch item draw
``random_configuration_count`` + ``specular_configuration_count`` scenes from torch's global
CPU generator, render input and target under each, ``log(x + 0.1)``, L1 mean.  When the
injected renderer is this package's ``LocalRenderer`` the whole thing -- both renderings,
the log/L1 and the analytic backward w.r.t. ``input`` -- is ONE fused HIP kernel (K3) that
reads the 24 map planes once and writes the 12 gradient planes once.  Any other object
with a ``.render(scene, svbrdf)`` method (the reference's plugin protocol, e.g. a path
tracer) goes through the generic per-scene loop built from that renderer's own outputs.
"""
import torch
import torch.nn as nn

from . import _hostext, _native, _refcode, environment, renderers, utils


class SVBRDFL1Loss(nn.Module):
    """losses.py:7-19: L1 on normals and roughness, L1 on log(x+0.01) for diffuse/specular."""

    epsilon_l1 = 0.01

    def forward(self, input, target):
        i_n, i_d, i_r, i_s = torch.split(input, (3, 3, 3, 3), dim=-3)
        t_n, t_d, t_r, t_s = torch.split(target, (3, 3, 3, 3), dim=-3)
        l1 = nn.functional.l1_loss
        e = self.epsilon_l1
        return (l1(i_n, t_n) + l1(torch.log(i_d + e), torch.log(t_d + e)) + l1(i_r, t_r)
                + l1(torch.log(i_s + e), torch.log(t_s + e)))


class _FusedRenderingLoss(torch.autograd.Function):
    """K3 behind autograd: the kernel already produces d loss/d input for upstream grad 1."""

    @staticmethod
    def forward(ctx, input, target, scenes, eps, l1_weight=0.0, eps_l1=0.01, head=False):
        need_in = ctx.needs_input_grad[0]
        need_tg = ctx.needs_input_grad[1]
        if head and need_tg:
            raise RuntimeError("the head-fused loss has no gradient w.r.t. the target maps")
        # (kept for backward(create_graph=True) only: references, no copies; a host table is a few hundred floats)
        ctx.save_for_backward(input, target)
        ctx.second_order = (scenes if scenes.is_cuda else scenes.detach().clone(), float(eps), float(l1_weight), float(eps_l1), bool(head))
        loss, grad_in = _native.rendering_loss(input, target, scenes, eps, want_grad=need_in,
                                               l1_weight=l1_weight, eps_l1=eps_l1, head=head)
        grad_tg = None
        if need_tg:
            # every term is |g(a) - g(b)|, symmetric: the target's gradient is the same kernel, roles swapped
            _, grad_tg = _native.rendering_loss(target, input, scenes, eps, want_grad=True,
                                                l1_weight=l1_weight, eps_l1=eps_l1)
        ctx.grads = (grad_in, grad_tg)
        return loss.view(())

    @staticmethod
    def backward(ctx, grad_loss):
        if torch.is_grad_enabled() and ctx.grads is not None:
            # backward(create_graph=True): the kernel's gradient buffers are constants to autograd; recompute the loss
            # from differentiable pieces instead (same scenes) and let autograd derive a gradient it can differentiate
            input, target = ctx.saved_tensors
            return differentiable_loss_backward(input, target, *ctx.second_order, grad_loss,
                                                ctx.needs_input_grad[0], ctx.needs_input_grad[1]) + (None,) * 5
        # This is the FALLBACK host path (the native extension is the default and does the same in csrc/host_ext.cpp)
        grad_in, grad_tg = _hand_over_gradients(ctx, grad_loss, "Trying to backward through the fused rendering loss a "
                                                "second time: its gradient buffers were handed to the first backward.  "
                                                "Specify retain_graph=True for the first one.")
        return grad_in, grad_tg, None, None, None, None, None


def _hand_over_gradients(ctx, grad_loss, second_time):
    """The plain backward of a fused loss whose kernel already produced the gradients ``ctx.grads`` (a tuple, None where
    not wanted) for upstream gradient 1: the chain rule through the scalar loss on the device, no host sync.  A plain
    backward hands the kernel's buffers over and scales them in place -- no copy, no extra pass; under retain_graph=True
    they stay with the graph and every backward receives a scaled copy, so repeated backwards work as through the
    reference's plain-autograd loss (losses.py:29-52), and a second backward without it fails like autograd's own nodes
    do (``second_time``: the message).  The cached 1.0 of ``_UnitGradientLoss`` is recognised (once somebody has asked
    for one): nothing to scale, nothing to launch.  -> the gradients, in ``ctx.grads``' order (that
    tuple itself on the plain unit-gradient step, a list otherwise: callers unpack it)."""
    grads = ctx.grads
    if grads is None:
        raise RuntimeError(second_time)
    keep = _current_backward_keeps_graph()
    if not keep:
        ctx.grads = None
    unit = bool(_unit_gradients) and _is_unit_gradient(grad_loss)
    if unit and not keep:
        return grads        # the plain step: the buffers as they are
    scale = None if unit else grad_loss.detach().to(torch.float32).reshape(1)
    outs = []
    for g in grads:
        if g is not None:
            if keep:
                g = g.clone()
            if scale is not None:
                _native.scale_inplace_(g, scale)
        outs.append(g)
    return outs


# private autograd accessor, looked up once: a torch build without it falls back to "the graph is kept" -- every backward
# then receives a scaled COPY of the kernel's buffers (the behaviour before the hand-over existed), never an AttributeError
_keep_graph_accessor = getattr(getattr(torch._C, "_autograd", None), "_get_current_graph_task_keep_graph", None)


def _current_backward_keeps_graph():
    return True if _keep_graph_accessor is None else bool(_keep_graph_accessor())


def composed_loss(input, target, scenes, eps, l1_weight=0.0, eps_l1=0.01, head=False):
    """The fused kernel's loss -- losses.py:29-52, plus ``l1_weight`` x losses.py:7-19 and the head decode of
    models.py:338-346 when asked for -- from differentiable pieces in float64: S renders per item through the float64
    K1 / K2 (``renderers._RenderFunction``), log / L1 by torch.  What float64 inputs take, and what
    ``backward(create_graph=True)`` of the fused float32 loss differentiates (the fused kernel's own gradient is a constant
    to autograd).  ``scenes`` [B,S,9] float32, host or device."""
    x, t = input.to(torch.float64), target.to(torch.float64)
    maps = decode_head(x) if head else x
    a = torch.log(renderers._RenderFunction.apply(maps, scenes) + eps)
    b = torch.log(renderers._RenderFunction.apply(t, scenes) + eps)
    loss = nn.functional.l1_loss(a, b)
    if float(l1_weight) != 0.0:
        l1 = SVBRDFL1Loss()
        l1.epsilon_l1 = eps_l1
        loss = l1_weight * l1(maps, t) + loss                                  # losses.py:62-63
    return loss


def differentiable_loss_backward(input, target, scenes, eps, l1_weight, eps_l1, head, grad_loss, need_in=True, need_tg=False):
    """(d loss/d input, d loss/d target) x ``grad_loss`` for the fused loss, attached to the autograd graph: the answer
    to ``backward(create_graph=True)`` / ``torch.autograd.grad(..., create_graph=True)``.  Also the entry point the native
    host extension calls back into (csrc/host_ext.cpp)."""
    return _composed_gradients(lambda: composed_loss(input, target, scenes, eps, l1_weight, eps_l1, head), (input, target),
                               (need_in, need_tg), grad_loss)


def _composed_gradients(composed, tensors, needs, grad_loss):
    """What backward(create_graph=True) of a fused loss answers: the gradients of ``composed()`` -- the loss from
    differentiable pieces, a float64 scalar, built here under grad mode -- towards those of ``tensors`` that ``needs``
    marks, times ``grad_loss``, attached to the autograd graph, each in its tensor's dtype; None for the others."""
    with torch.enable_grad():
        wanted = [t for t, need in zip(tensors, needs) if need]
        grads = iter(torch.autograd.grad(composed(), wanted, grad_loss.to(torch.float64).reshape(()), create_graph=True))
    return tuple(next(grads).to(t.dtype) if need else None for t, need in zip(tensors, needs))


class _UnitGradientLoss(torch.Tensor):
    """A 0-dim loss whose PLAIN ``backward()`` hands autograd a cached device-resident 1.0 instead of a fresh ones tensor."""

    __torch_function__ = torch._C._disabled_torch_function_impl      # ops on it return plain tensors, no dispatch cost

    def _plain_backward(self, gradient, create_graph):
        """no explicit gradient, no create_graph, and nobody watches the loss's gradient (a hook, retain_grad): whoever
        does gets the engine's own fresh ones tensor, theirs to edit; the node then sees an ordinary gradient and applies it"""
        return gradient is None and not create_graph and self._backward_hooks is None and not self.retains_grad


class _FusedLossTensor(_UnitGradientLoss):
    """The 0-dim loss the native host path returns when a gradient is wanted: an ordinary tensor, attached to the autograd
    graph as usual, whose PLAIN ``backward()`` (no explicit gradient, no create_graph) costs one kernel launch and no
    Python in front of the engine:

    * PyTorch's autograd engine runs, but is handed the extension's cached device-resident 1.0 as the explicit upstream
      gradient instead of filling a fresh ones tensor, and the loss's autograd node, recognising that tensor by address and
      version, skips its (no-op) scale launch: the step stays ONE kernel launch instead of three (fill, K3, scale).  Same
      values bit for bit: multiplying by 1.0 is what was skipped.
    * the engine is entered from the extension (``torch::autograd::backward``, the public C++ call) rather than through
      ``torch.autograd.backward``'s Python front end (~6 us of interpreter time per step); a loss someone watches (a hook,
      ``retain_grad``) or an ``inputs=`` call takes the ordinary Python route with the engine's own ones tensor.

    (Rounds 2-5 also had an engine-FREE shortcut for leaf inputs that walked autograd internals -- the leaf's gradient
    accumulator and hook lists -- behind a torch-version gate.  With the engine entered from C++ it bought nothing any more
    (224.9 vs 224.7 k patches/s, profiles/HISTORY.md) and it was the fragile part of this file: removed in round 6.)

    Every other use -- an explicit gradient, ``create_graph=True``, a second ``backward()``, arithmetic on the loss (which
    yields a plain tensor), ``torch.autograd.grad`` -- goes through autograd unchanged."""

    def backward(self, gradient=None, retain_graph=None, create_graph=False, inputs=None):
        src = self.__dict__.pop("_svbrdf_src", None)
        if src is not None and _UNIT_GRADIENT and self._plain_backward(gradient, create_graph):
            inner, ext = src
            if inputs is None and _ENGINE_FROM_NATIVE and not _functorch_active():
                # the same engine run, entered through torch::autograd::backward from the extension (no Python
                # argument processing in front of the engine: ~6 us of the ~20 us a step spends on the host)
                # (from `inner`, the extension's own tensor: `self` is an alias of it that nobody watches -- checked
                # above -- so its AliasBackward node would only be one more node for the engine to walk)
                ext.engine_backward(inner, bool(retain_graph))
                return None
            gradient = ext.unit_gradient(inner)
        return torch.Tensor.backward(self, gradient, retain_graph, create_graph, inputs)


# torch.autograd.backward refuses to run inside a functorch transform (vmap / grad): leave that error to it
_functorch_active = getattr(torch._C, "_are_functorch_transforms_active", lambda: False)
_UNIT_GRADIENT = True       # tests switch it off to compare against the engine's own ones tensor
_ENGINE_FROM_NATIVE = True  # ... and this one to compare against torch.Tensor.backward(loss, unit_gradient)


def _check_shapes(input, target):
    if input.dim() != 4 or input.shape != target.shape or input.shape[1] != 12:
        raise ValueError("input and target must both be [B,12,H,W]")


class RenderingLoss(nn.Module):
    epsilon_render = 0.1   # losses.py:45

    def __init__(self, renderer):
        super().__init__()
        self.renderer = renderer
        self.random_configuration_count = 3     # losses.py:26
        self.specular_configuration_count = 6   # losses.py:27

    def sample_scene_table(self, batch_size):
        """[B,S,9] on the host, reference RNG draw order (one item after the other)."""
        key = (int(batch_size), int(self.random_configuration_count), int(self.specular_configuration_count))
        if getattr(self, "_sampler_key", None) != key:
            self._sampler, self._sampler_key = environment.BatchSceneSampler(*key), key
        return self._sampler.sample()

    def forward(self, input, target):
        if self.uses_fused_kernel():
            return self._forward_fused(input, target)
        _check_shapes(input, target)
        return self._forward_plugin(input, target)

    def uses_fused_kernel(self):
        """True for this package's ``LocalRenderer`` -- and for an instance of the REFERENCE's own
        ``renderers.LocalRenderer`` (development/multiImage_pytorch/renderers.py:14), which is exactly what the kernels
        restate: a training script that keeps the reference's renderer class (``install(patch_renderer=False)``) still
        gets the fused path.  "The reference's own" is decided by the class's CODE (``_refcode``: fingerprints of
        ``dot_product``, ``normalize`` and the nine methods, recorded from the reference), never by its name: a fork
        that edits ``renderers.py``, a subclass, an instance with a patched ``render`` -- any other object with
        ``.render`` -- is a plugin and is rendered by calling it (``_forward_plugin``)."""
        r = self.renderer
        if isinstance(r, renderers.LocalRenderer):
            # a subclass (or an instance) that brings its own render() is a plugin like any other
            return type(r).render is renderers.LocalRenderer.render and "render" not in vars(r)
        return _refcode.is_reference_local_renderer(r)

    def _forward_double(self, input, target, l1_weight, eps_l1=0.01):
        """float64 maps: the reference's loss (losses.py:29-52) is dtype-agnostic and, with double maps, mixed precision
        (float32 geometry, double shading -- see svbrdf_render_fwd_f64).  Composed here from the float64 renders through
        autograd: S renders per item in one K1 launch, log / L1 by torch in double, the backward through K2.  The slow
        path of gradient checks and double-precision experiments; same scene draws as the fused path."""
        _check_shapes(input, target)
        if not input.is_cuda:
            raise _native.NativeLibraryError("RenderingLoss needs tensors on a ROCm device (got %s); there is no CPU "
                                             "fallback" % input.device)
        table = self.sample_scene_table(input.shape[0]).to(input.device)
        return composed_loss(input, target, table, self.epsilon_render, l1_weight, eps_l1)

    def _forward_fused(self, input, target, l1_weight=0.0, eps_l1=0.01, head=False):
        if not head and torch.float64 in (input.dtype, target.dtype):
            # either side double: the reference's torch ops promote, so does this (composed_loss computes in double)
            return self._forward_double(input, target, l1_weight, eps_l1)
        if head:
            if input.dim() != 4 or target.dim() != 4 or input.shape[1] != 9 or target.shape[1] != 12:
                raise ValueError("head-fused loss needs input [B,9,H,W] and target [B,12,H,W]")
        else:
            _check_shapes(input, target)
        ext = _hostext.module() if input.is_cuda else None
        if ext is not None and input.dtype == torch.float32 and target.dtype == torch.float32 \
                and input.device.index == torch.cuda.current_device():
            # native host path: same draws, same kernels, no interpreter in the loop
            loss = ext.fused_loss(input, target, int(self.random_configuration_count),
                                  int(self.specular_configuration_count), float(self.epsilon_render),
                                  float(l1_weight), float(eps_l1), _native._raw_stream(input.device), bool(head))
            if loss.requires_grad:
                out = loss.as_subclass(_FusedLossTensor)       # see _FusedLossTensor: a plain backward() is made cheaper
                out.__dict__["_svbrdf_src"] = (loss, ext)
                return out
            return loss
        table = self.sample_scene_table(input.shape[0])
        if not input.is_cuda:
            raise _native.NativeLibraryError(
                "RenderingLoss with the MI355X LocalRenderer needs tensors on a ROCm device "
                "(got %s); there is no CPU fallback" % input.device)
        # handed over here, by the binding's one rule (by value, or uploaded): a call that also wants the target's gradient
        # launches twice on it, and what the node keeps for create_graph=True is the table as it was launched with
        table = _native.loss_scene_table(input, table, head)
        return _FusedRenderingLoss.apply(input, target, table,
                                         self.epsilon_render, float(l1_weight), float(eps_l1), bool(head))

    def _forward_plugin(self, input, target):
        """Generic plugin path for a foreign renderer object (losses.py:29-52 semantics)."""
        rendered_in, rendered_tg = [], []
        for b in range(input.shape[0]):
            scenes = (environment.generate_random_scenes(self.random_configuration_count)
                      + environment.generate_specular_scenes(self.specular_configuration_count))
            rendered_in.append(torch.cat([self.renderer.render(sc, input[b]) for sc in scenes], dim=0))
            rendered_tg.append(torch.cat([self.renderer.render(sc, target[b]) for sc in scenes], dim=0))
        a = torch.log(torch.stack(rendered_in, dim=0) + self.epsilon_render)
        t = torch.log(torch.stack(rendered_tg, dim=0) + self.epsilon_render)
        return nn.functional.l1_loss(a, t)


class _FusedPhotoLoss(torch.autograd.Function):
    """The fused photo-loss kernel behind autograd: it already produces d loss/d input for upstream gradient 1.
    ``head``: ``input`` is the generator's [B,9,H,W] post-tanh output, decoded in the kernel (HeadPhotoLoss)."""

    @staticmethod
    def forward(ctx, input, photos, scenes, eps, head, weights=None, exposure=None):
        needs = ctx.needs_input_grad        # (read once: every access builds the tuple anew)
        # the binding's mode, by the one extra gradient a launch can form: the photos' (no exposure, no table gradient:
        # _forward), else the scene table's (a device table, no exposure: _forward), else the exposure's, else none
        mode = "photos" if needs[1] else "scenes" if needs[2] else "exposure" if exposure is not None else None
        need_s = mode == "scenes"
        # (for backward(create_graph=True) only: references, no copies)
        ctx.save_for_backward(input, photos, *(() if exposure is None else (exposure,)), *((scenes,) if need_s else ()))
        ctx.second_order = (None if need_s else scenes if scenes.is_cuda else scenes.detach().clone(), float(eps), bool(head),
                            weights)
        # ONE launch in every mode: loss, map gradient (a detached input runs the photo-gradient kernels' forward-only
        # scene loop) and the mode's own gradient.  (eps, want_grad, head, weights, exposure, want_exposure_grad,
        # want_scene_grad, want_photo_grad)
        out = _native.photo_loss(input, photos, scenes, eps, needs[0], head, weights, exposure if mode == "exposure" else None,
                                 mode == "exposure" and needs[6], need_s, mode == "photos")
        # always in the order (input, exposure, scenes, photos), None where a gradient was not produced
        third = None if mode is None else out[2]
        ctx.grads = (out[1], third if mode == "exposure" else None, third if need_s else None, third if mode == "photos" else None)
        return out[0].view(())

    @staticmethod
    def backward(ctx, grad_loss):
        if torch.is_grad_enabled():
            # backward(create_graph=True): the kernel's gradient is a constant to autograd; differentiate the composed
            # definition instead (same scenes), in float64 like the other fused losses do
            scenes, eps, head, weights = ctx.second_order
            input, photos, *rest = ctx.saved_tensors
            table = rest.pop() if scenes is None else None
            exposure = rest[0] if rest else None

            def composed():
                x = input.to(torch.float64)
                return composed_photo_loss(decode_head(x) if head else x, photos, scenes if table is None else table, eps,
                                           weights, None if exposure is None else exposure.to(torch.float64))
            g_in, g_e, g_s, g_p = _composed_gradients(
                composed, (input, exposure, table, photos),
                (ctx.needs_input_grad[0], exposure is not None and ctx.needs_input_grad[6], table is not None,
                 ctx.needs_input_grad[1]), grad_loss)
        else:
            g_in, g_e, g_s, g_p = _hand_over_gradients(
                ctx, grad_loss, "Trying to backward through the fused photo loss a second time: its gradient buffer was "
                "handed to the first backward.  Specify retain_graph=True for the first one.")
        return g_in, g_p, g_s, None, None, None, g_e


class _PhotoLossTensor(_UnitGradientLoss):
    """The 0-dim loss PhotoLoss returns when a gradient is wanted: an ordinary tensor whose PLAIN ``backward()`` (no
    explicit gradient, no create_graph, nobody watching the loss's gradient) hands autograd a cached device-resident 1.0
    as the upstream gradient; the loss's node recognises that tensor and skips its (no-op) scale launch, so a step is
    ONE kernel launch.  Same values bit for bit: multiplying by 1.0 is what was skipped.  Every other use goes through
    autograd unchanged (``_FusedLossTensor`` does the same for the native host path of the other losses)."""

    def backward(self, gradient=None, retain_graph=None, create_graph=False, inputs=None):
        if self._plain_backward(gradient, create_graph):
            gradient = _unit_gradient(self.device)
        return torch.Tensor.backward(self, gradient, retain_graph, create_graph, inputs)


_unit_gradients = {}


def _unit_gradient(device):
    t = _unit_gradients.get(device)
    if t is None:
        t = _unit_gradients[device] = torch.ones((), dtype=torch.float32, device=device)
    return t


def _is_unit_gradient(grad):
    t = _unit_gradients.get(grad.device)
    return t is not None and grad.data_ptr() == t.data_ptr() and t._version == 0 and grad.dtype == torch.float32


def weighted_log_l1(rendered, photos, eps, weights):
    """The weighted photo loss of given renderings, literally as specified: with w in [0, 1] broadcast over the colour
    channels, N the number of terms and p' = where(w > 0, photo, 0),

        (1/N) sum w | log(rendered + eps) - log(p' + eps) |

    ``rendered`` and ``photos`` [B,S,3,H,W], ``weights`` [B,S,H,W] or [B,1,H,W].  The photo is REPLACED under a zero
    weight before anything is computed from it, so a NaN there reaches neither the loss nor, through 0 * NaN, autograd."""
    w = weights.to(rendered.dtype).unsqueeze(2)                              # [B,S|1,1,H,W]
    p = photos.to(rendered.dtype)
    p = torch.where((w > 0).expand_as(p), p, torch.zeros((), dtype=p.dtype, device=p.device))
    return (w * (torch.log(rendered + eps) - torch.log(p + eps)).abs()).sum() / rendered.numel()


def composed_photo_loss(input, photos, scenes, eps, weights=None, exposure=None):
    """The photo loss from differentiable pieces -- S renders per item through K1 / K2 (``renderers._RenderFunction``:
    float32 maps through the float32 kernels, float64 maps through the float64 ones), log / L1 mean by torch.  What float64
    maps take and what ``backward(create_graph=True)`` of the fused loss differentiates.  ``scenes`` [B,S,9] float32.
    ``weights`` ([B,S,H,W] or [B,1,H,W], or None): the weighted definition, ``weighted_log_l1``.  ``exposure`` (broadcastable
    to [B,S,3], or None): the per-photo gain, ``rendered * exposure[..., None, None]`` -- the rendering is linear in the
    light colour the fused kernels scale instead.  A table that requires grad takes ``renderers.render_table``, the same
    render in stock torch ops, differentiable in the table as well; any other table takes K1 / K2 as it always did."""
    if scenes.requires_grad and torch.is_grad_enabled():
        rendered = renderers.render_table(input, scenes.to(input.device))
    else:
        rendered = renderers._RenderFunction.apply(input, scenes)
    if exposure is not None:
        rendered = rendered * exposure[..., None, None]       # (a float64 exposure promotes, as torch ops do)
    if weights is not None:
        return weighted_log_l1(rendered, photos, eps, weights)
    return nn.functional.l1_loss(torch.log(rendered + eps), torch.log(photos.to(rendered.dtype) + eps))


def fold_exposure(table, exposure):
    """The scene table ``[B,S,9]`` with the gains ``exposure`` (broadcastable to ``[B,S,3]``) multiplied into its colour
    columns, in the table's float32 when both are: THE expression behind "loss and map gradient equal, bit for bit, those
    of a scene table whose colour columns were multiplied by the gains in float32" (PhotoLoss).  Stock torch ops:
    autograd chains a gradient towards the folded table back to table and gains."""
    return torch.cat((table[..., :6], table[..., 6:] * exposure), dim=-1)


_NORMALIZE = ("count", "weights")
_WEIGHT_SUM_FLOOR = 2.0 ** -126      # the "tiny" of normalize="weights": the smallest normal float32, one weight's worth


def _check_weights(weights, input, photos):
    """``weights`` as the photo losses take them -> float32 [B,S,H,W] or [B,1,H,W] (None passes).  ``photos`` [B,S,3,H,W]"""
    if weights is None:
        return None
    if not isinstance(weights, torch.Tensor):
        raise TypeError("weights must be a tensor")
    B, S, _, H, W = photos.shape
    if weights.dim() == 5 and tuple(weights.shape) == (B, S, 3, H, W):
        raise ValueError("per-channel weights [B,S,3,H,W] are not supported: one weight serves the three channels of a "
                         "pixel -- take the minimum over the channels (weights.amin(dim=2))")
    if weights.dim() == 3:
        weights = weights.unsqueeze(1)              # [B,H,W]: one plane per item, shared by its photos
    if tuple(weights.shape) not in ((B, S, H, W), (B, 1, H, W)):
        raise ValueError("weights must be [B,S,H,W], [B,1,H,W] or [B,H,W] with the photos' B, S, H and W, got %s"
                         % (tuple(weights.shape),))
    if weights.requires_grad:
        raise RuntimeError("the photo losses have no gradient w.r.t. the weights: pass weights.detach()")
    if weights.device != input.device:
        raise ValueError("input and weights must be on the same device")
    if weights.dtype in (torch.bool, torch.uint8):
        weights = weights.to(torch.float32)
    if weights.dtype != torch.float32:
        raise TypeError("weights must be float32, bool or uint8 (got %s)" % weights.dtype)
    return weights


def _check_exposure(exposure, input, photos):
    """``exposure`` as the photo losses take it -> [B,S,3], expanded by torch ops (autograd sums the gradient back over the
    broadcast); None passes.  A positive gain per photo and colour channel: [B,S,3], or [B,S,1] / [B,S] (one per photo,
    grey) or [B,1,1] (one per item).  float32, or float64 (which takes the composed definition); on the input's device;
    it may require grad."""
    if exposure is None:
        return None
    if not isinstance(exposure, torch.Tensor):
        raise TypeError("exposure must be a tensor")
    if not exposure.dtype.is_floating_point:
        raise TypeError("exposure must be float32 or float64 (got %s)" % exposure.dtype)
    B, S = photos.shape[0], photos.shape[1]
    if exposure.dim() == 2:
        exposure = exposure.unsqueeze(-1)           # [B,S]: one gain per photo
    if tuple(exposure.shape) not in ((B, S, 3), (B, S, 1), (B, 1, 1)):
        raise ValueError("exposure must be [B,S,3], [B,S,1], [B,S] or [B,1,1] with the photos' B = %d and S = %d, got %s"
                         % (B, S, tuple(exposure.shape)))
    if exposure.device != input.device:
        raise ValueError("input and exposure must be on the same device")
    if exposure.dtype not in (torch.float32, torch.float64):
        raise TypeError("exposure must be float32 or float64 (got %s)" % exposure.dtype)
    return exposure.expand(B, S, 3)


def _normalized(loss, weights, photos, normalize):
    """normalize="weights": the fused mean over all N terms -> the weighted mean sum w|d| / (3 sum w), sum w over the
    broadcast [B,S,H,W] weights.  Stock torch ops on the device, no host sync; 0 when every weight is 0."""
    if weights is None or normalize == "count":
        return loss
    B, S, _, H, W = photos.shape
    total = weights.sum(dtype=torch.float64) * (3.0 * S / weights.shape[1])       # 3 sum w, shared planes counted S times
    # (the floor only binds when every weight is 0 -- then the loss is exactly 0 and N / floor must stay finite)
    scale = float(B * S * 3 * H * W) / total.clamp_min(_WEIGHT_SUM_FLOOR)
    return (loss.to(torch.float64) * scale).to(loss.dtype)


def _check_fused_photo_inputs(loss_name, input_name, input, photos):
    """The fused photo losses' device and dtype rules, raised as errors: tensors on a ROCm device, float32 or float64.
    -> "promote": double on either side (the reference's torch ops would promote, so the caller takes the composed
    float64 definition)."""
    if not input.is_cuda:
        raise _native.NativeLibraryError("%s with the MI355X LocalRenderer needs tensors on a ROCm device "
                                         "(got %s); there is no CPU fallback" % (loss_name, input.device))
    if input.dtype == torch.float64 or photos.dtype == torch.float64:
        return True
    if input.dtype != torch.float32 or photos.dtype != torch.float32:
        raise TypeError("%s and photos must be float32 or float64 (got %s, %s)" % (input_name, input.dtype, photos.dtype))
    return False


class _PhotoLossModule(nn.Module):
    """What PhotoLoss and HeadPhotoLoss share: the constructor and the routing of a call."""

    def __init__(self, renderer, eps=0.1, normalize="count", differentiable_photos=False):
        super().__init__()
        if normalize not in _NORMALIZE:
            raise ValueError("normalize must be one of %s, got %r" % (_NORMALIZE, normalize))
        self.renderer = renderer
        self.eps = eps
        self.normalize = normalize
        self.differentiable_photos = bool(differentiable_photos)

    def uses_fused_kernel(self):
        return RenderingLoss.uses_fused_kernel(self)     # its rule, on this module's renderer: no module is built per call

    def _forward_decoded(self, encoded9, photos, scenes, weights, exposure=None):
        """the head losses' composed definition: PhotoLoss, which normalises by itself, on the decoded maps"""
        return PhotoLoss(self.renderer, self.eps, self.normalize, self.differentiable_photos)(
            decode_head(encoded9), photos, scenes, weights, exposure)

    def _forward(self, x, photos, scenes, weights, head, exposure=None):
        """The one routing of both modules; ``x``: the 12 maps, or with ``head`` the 9 encoded channels.  A plugin renderer
        and double on any side take the composed definition, everything else is the fused kernel.  ``exposure=None`` is
        the path without exposure, untouched.  With an exposure the fused path is the exposure kernel (loss and both
        gradients in one launch) when the input or the exposure requires grad; a pure evaluation multiplies the table's
        colour columns by the exposure with one torch op and runs the forward-only kernel of the loss without exposure,
        which computes the same loss bit for bit (there is no forward-only exposure kernel: not on the hot path).  A float32
        ``[B,S,9]`` scene table that requires grad takes the scene-gradient kernel (csrc/svbrdf_photo_pose.hip): loss, map
        gradient and d loss/d table in one launch; a table that does not takes exactly the paths above.
        ``differentiable_photos`` with photos that require grad: the photo-gradient kernel
        (csrc/svbrdf_photo_grad_photos.hip), a constant exposure folded into the table's colour columns; together with a table
        or an exposure that requires grad, the composed definition."""
        photos = PhotoLoss._check(x, photos, channels=9 if head else 12, differentiable=self.differentiable_photos)
        need_p = self.differentiable_photos and photos.requires_grad and torch.is_grad_enabled()
        weights = _check_weights(weights, x, photos)
        exposure = _check_exposure(exposure, x, photos)
        B, S = photos.shape[0], photos.shape[1]
        if not self.uses_fused_kernel():
            if head:
                return self._forward_decoded(x, photos, scenes, weights, exposure)
            loss = self._forward_plugin(x, photos, PhotoLoss._scene_objects(scenes, B, S), weights, exposure)
        else:
            table = PhotoLoss._scene_table(scenes, B, S)
            double = _check_fused_photo_inputs(*(("HeadPhotoLoss", "encoded9") if head else ("PhotoLoss", "input")), x, photos)
            if double or (exposure is not None and exposure.dtype == torch.float64):
                if head:
                    return self._forward_decoded(x.to(torch.float64), photos, table, weights, exposure)   # promoted in front of the decode
                loss = composed_photo_loss(x.to(torch.float64), photos, table.to(x.device), self.eps, weights, exposure)  # float64 K1 / K2
            elif need_p and (table.requires_grad or (exposure is not None and exposure.requires_grad)):
                # no kernel forms the photos' gradient beside the table's or the exposure's: the composed definition,
                # differentiable in all of them (float32 K1 / K2, or render_table for the table)
                loss = composed_photo_loss(decode_head(x) if head else x, photos, table.to(x.device), self.eps, weights, exposure)
            else:
                # An exposure goes to its own kernels only when the input's or its own gradient is what is wanted.  The
                # photo-gradient and scene-gradient kernels take none, and there is no forward-only exposure kernel (a
                # pure evaluation is not on the hot path): there the gains multiply the table's colour columns in front
                # of the call -- the exposure kernels' one float32 multiply, the same loss bit for bit -- as constants,
                # unless it is the table's gradient that is wanted: autograd then chains it back to the gains.
                want_table = table.requires_grad and torch.is_grad_enabled()
                fold = exposure is not None and (need_p or want_table or not (
                    torch.is_grad_enabled() and (x.requires_grad or exposure.requires_grad)))
                if want_table or fold:
                    table = table.to(x.device)      # (the kernels behind both take a device table; autograd sees the copy)
                if fold:
                    table, exposure = fold_exposure(table, exposure if want_table else exposure.detach()), None
                loss = _FusedPhotoLoss.apply(x, photos, table, float(self.eps), head, weights, exposure)
                if (weights is None or self.normalize == "count") and loss.requires_grad:
                    return loss.as_subclass(_PhotoLossTensor)
        return _normalized(loss, weights, photos, self.normalize)


class PhotoLoss(_PhotoLossModule):
    """The rendering loss against PHOTOGRAPHS instead of against the renderings of ground-truth maps:

        mean over b,s,c,i,j of | log(render(scenes[b][s], input[b]) + eps) - log(photos[b,s] + eps) |

    -- fitting maps to captured or synthesised photos, self-supervised training on the input photos themselves.
    ``forward(input [B,12,H,W], photos [B,S,3,H,W] or [B,3,H,W] (S = 1), scenes)`` returns a 0-dim tensor, differentiable
    w.r.t. ``input``, w.r.t. ``exposure`` and w.r.t. ``scenes`` when that is a tensor (both below), w.r.t. the photos when
    constructed with ``differentiable_photos=True`` (below); never w.r.t. the weights.  ``scenes``: the light / view of every photo, a ``[B,S,9]`` float32 tensor (host or device;
    camera xyz | light xyz | light rgb) or a nested list ``scenes[b][s]`` of ``environment.Scene``-like objects.

    With this package's ``LocalRenderer`` and float32 maps on a ROCm device it is ONE fused HIP kernel (forward and the
    analytic backward; csrc/svbrdf_photo_loss.hip).  Any other renderer object, float64 maps and
    ``backward(create_graph=True)`` take the composed definition: ``renderer.render`` per scene, ``log``, L1 mean --
    which is also the semantic specification of the fused path.

    ``weights`` (optional): a confidence in [0, 1] per photo pixel, for captured photographs whose clipped highlights,
    pixels outside the patch, noise-floor shadows or invalid (NaN) pixels must not vote -- ``[B,S,H,W]`` (one plane per
    photo), ``[B,1,H,W]`` or ``[B,H,W]`` (one plane per item, shared by its photos); float32, or bool / uint8 masks.  The
    loss becomes ``(1/N) sum w |log(render + eps) - log(p' + eps)|`` with ``p' = where(w > 0, photo, 0)``
    (``weighted_log_l1``): a weight of exactly 0 excuses the photo value under it -- term and gradient exactly 0 even
    where the photo is NaN or infinite -- but never the maps; a weight that is NaN, negative or above 1 gives a NaN loss;
    weights of all ones give the unweighted loss and gradient bit for bit.  Still one launch, one more load per
    pixel-render.  ``normalize="count"`` (default) divides by the number N = B S 3 H W of terms as above;
    ``normalize="weights"`` returns the weighted mean ``sum w|d| / (3 sum w)`` instead (0 when every weight is 0), which
    costs a reduction over the weights and a scale of the loss on the device (two small launches, no host sync).

    ``exposure`` (optional): the unknown radiometric scale of a captured photograph -- flash power, shutter, ISO, white
    balance -- as a positive gain per photo and colour channel that multiplies the light colour of its scene:
    ``[B,S,3]``, ``[B,S,1]`` or ``[B,S]`` (one grey gain per photo) or ``[B,1,1]`` (one per item), float32 on the input's
    device.  It may require grad: with this package's ``LocalRenderer`` the loss, ``d loss/d input`` and
    ``d loss/d exposure`` come out of ONE launch (csrc/svbrdf_photo_exposure.hip), so the gains can be fitted jointly with
    the maps (in log space: they must stay positive -- a gain that is NaN, infinite or <= 0 gives a NaN loss).  Loss and
    map gradient equal, bit for bit, those of a scene table whose colour columns were multiplied by the gains in float32.
    float64 on any side, a plugin renderer and ``backward(create_graph=True)`` take the composed definition,
    ``rendered * exposure[..., None, None]``.

    ``scenes`` as a float32 ``[B,S,9]`` tensor that requires grad: the camera and light positions (and the light colour) of
    every photo are fitted too.  With this package's ``LocalRenderer`` the loss, ``d loss/d input`` and ``d loss/d scenes``
    come out of ONE launch (csrc/svbrdf_photo_pose.hip); loss and map gradient equal, bit for bit, those of the same table
    without the gradient.  The table's gradient follows PyTorch's sub-gradient conventions of the composed definition
    (``renderers.render_table``, which float64, ``backward(create_graph=True)`` and a table on the host side of a double
    input take).  With ``exposure=`` as well the gains multiply the colour columns in front of the kernel and get their
    gradient by the chain rule.  A colour that is NaN, infinite or <= 0 gives a NaN loss and an all-NaN table gradient.
    Scene OBJECTS and a plugin renderer have no gradient towards light or camera positions.

    ``differentiable_photos=True`` (constructor; the default keeps the error for photos that require grad): photos that
    require grad get ``d loss/d photos = -(w/N) sign(delta) / (photos + eps)`` -- what ``capture.rectify``'s gradients
    towards its homographies and its lens take, so ``rectify(...)``, this loss and ``backward()`` are one chain.  With this
    package's ``LocalRenderer`` and float32 tensors the loss, ``d loss/d input`` and ``d loss/d photos`` come out of ONE
    launch (csrc/svbrdf_photo_grad_photos.hip), loss and map gradient bit for bit those without it; a detached input runs
    the cheaper forward-only form (loss and photo gradient: a registration stage).  A constant ``exposure`` is folded into
    the table's colour columns.  These take ``composed_photo_loss`` instead, which is differentiable in the photos
    through ``weighted_log_l1``: float64 on any side, a plugin renderer, ``backward(create_graph=True)``, and photos that
    require grad together with a table or an exposure that requires grad."""

    @staticmethod
    def _check(input, photos, channels=12, differentiable=False):
        if not isinstance(input, torch.Tensor) or not isinstance(photos, torch.Tensor):
            raise TypeError("input and photos must be tensors")
        if input.dim() != 4 or input.shape[1] != channels:
            raise ValueError("input must be [B,%d,H,W]" % channels)
        if photos.dim() == 4:
            photos = photos.unsqueeze(1)                # [B,3,H,W]: one photo per item
        if photos.dim() != 5 or photos.shape[0] != input.shape[0] or photos.shape[2] != 3 \
                or photos.shape[3:] != input.shape[2:]:
            raise ValueError("photos must be [B,S,3,H,W] (or [B,3,H,W]) with the input's B, H and W")
        if photos.requires_grad and not differentiable:
            raise RuntimeError("PhotoLoss has no gradient w.r.t. the photos: pass photos.detach()")
        if photos.device != input.device:
            raise ValueError("input and photos must be on the same device")
        if not photos.dtype.is_floating_point or not input.dtype.is_floating_point:
            raise TypeError("input and photos must be floating point (got %s, %s)" % (input.dtype, photos.dtype))
        return photos

    @staticmethod
    def _scene_objects(scenes, B, S):
        """-> scenes[b][s] as objects with .camera.pos / .light.pos / .light.color (what a plugin renderer takes)"""
        if isinstance(scenes, torch.Tensor):
            if tuple(scenes.shape) != (B, S, 9):
                raise ValueError("scenes must be [B,S,9] = %s, got %s" % ((B, S, 9), tuple(scenes.shape)))
            return [environment.scenes_from_table(t) for t in scenes.detach().to("cpu", torch.float32)]
        rows = [list(r) for r in scenes]
        if len(rows) != B or any(len(r) != S for r in rows):
            raise ValueError("scenes must hold S = %d scenes for each of the B = %d items" % (S, B))
        return rows

    @staticmethod
    def _scene_table(scenes, B, S):
        """-> [B,S,9] float32 tensor (a tensor passes, host or device; Scene objects become a host table)"""
        if isinstance(scenes, torch.Tensor):
            if tuple(scenes.shape) != (B, S, 9):
                raise ValueError("scenes must be [B,S,9] = %s, got %s" % ((B, S, 9), tuple(scenes.shape)))
            if scenes.dtype != torch.float32:
                raise TypeError("scenes must be float32 (got %s)" % scenes.dtype)
            return scenes
        rows = PhotoLoss._scene_objects(scenes, B, S)
        return torch.stack([torch.stack([environment.scene_to_row(sc) for sc in r]) for r in rows])

    def forward(self, input, photos, scenes, weights=None, exposure=None):
        return self._forward(input, photos, scenes, weights, head=False, exposure=exposure)

    def _forward_plugin(self, input, photos, scenes, weights=None, exposure=None):
        """the composed definition with a foreign renderer object: its own render() per scene, log, L1 mean"""
        rendered = torch.stack([torch.cat([self.renderer.render(sc, input[b]) for sc in scenes[b]], dim=0)
                                for b in range(input.shape[0])], dim=0)
        if exposure is not None:
            rendered = rendered * exposure[..., None, None]       # (a float64 exposure promotes, as torch ops do)
        if weights is not None:
            return weighted_log_l1(rendered, photos, self.eps, weights)
        return nn.functional.l1_loss(torch.log(rendered + self.eps), torch.log(photos + self.eps))


class MixedLoss(nn.Module):
    """losses.py:54-63: l1_weight * SVBRDFL1Loss + RenderingLoss.

    With this package's ``LocalRenderer`` the L1 terms are folded into the fused kernel (the 24
    map planes are already in registers: no extra HBM traffic, no extra launches) instead of
    ~45 small elementwise launches of stock ops; any other renderer takes the literal sum."""

    def __init__(self, renderer, l1_weight=0.1):
        super().__init__()
        self.l1_weight = l1_weight
        self.l1_loss = SVBRDFL1Loss()
        self.rendering_loss = RenderingLoss(renderer)

    def forward(self, input, target):
        if self.rendering_loss.uses_fused_kernel() and input.is_cuda and float(self.l1_weight) != 0.0:
            return self.rendering_loss._forward_fused(input, target, l1_weight=float(self.l1_weight),
                                                      eps_l1=self.l1_loss.epsilon_l1)
        return self.l1_weight * self.l1_loss(input, target) + self.rendering_loss(input, target)


def decode_head(encoded9):
    """The network head of the reference's models (models.py:338-346): generator output after tanh,
    [..,9,H,W] in [-1,1] -> [..,12,H,W] maps (unit normals; diffuse, roughness x3, specular in [0,1])."""
    maps = utils.decode_svbrdf(encoded9)
    n, d, r, s = torch.split(maps, (3, 3, 3, 3), dim=-3)
    return utils.pack_svbrdf(n, utils.encode_as_unit_interval(d), utils.encode_as_unit_interval(r),
                             utils.encode_as_unit_interval(s))


class FusedHeadLoss(nn.Module):
    """``MixedLoss(renderer, l1_weight)(decode_head(encoded9), target)`` in one
    kernel -- the head decode (normal-map decode, roughness repeat, range maps), both renderings, the
    L1 and rendering losses and the gradient w.r.t. the NINE encoded channels.  The model returns
    ``tanh(generator(x))`` and skips its own decode; use ``decode_head`` when the maps themselves are
    needed (validation images).  ``l1_weight=0`` gives the pure rendering loss."""

    def __init__(self, renderer, l1_weight=0.1):
        super().__init__()
        self.l1_weight = l1_weight
        self.l1_loss = SVBRDFL1Loss()
        self.rendering_loss = RenderingLoss(renderer)

    def forward(self, encoded9, target):
        if self.rendering_loss.uses_fused_kernel() and encoded9.is_cuda:
            return self.rendering_loss._forward_fused(encoded9, target, l1_weight=float(self.l1_weight),
                                                      eps_l1=self.l1_loss.epsilon_l1, head=True)
        maps = decode_head(encoded9)
        return self.l1_weight * self.l1_loss(maps, target) + self.rendering_loss(maps, target)


class HeadPhotoLoss(_PhotoLossModule):
    """``PhotoLoss(renderer, eps)(decode_head(encoded9), photos, scenes)`` in one kernel: what training or fine-tuning the
    network against photographs needs.  ``forward(encoded9 [B,9,H,W], photos [B,S,3,H,W] or [B,3,H,W] (S = 1), scenes)``
    with ``encoded9`` the generator's output after tanh (any finite value: no clamp of its own) and photos / scenes as
    ``PhotoLoss.forward`` takes them; a 0-dim tensor, differentiable w.r.t. ``encoded9``, w.r.t.
    ``exposure`` and w.r.t. a ``[B,S,9]`` ``scenes`` tensor that requires grad, as ``PhotoLoss`` documents both, w.r.t. the
    photos with ``differentiable_photos=True`` as ``PhotoLoss`` documents it (the same ONE launch, 9 channels); never w.r.t.
    the weights.

    With this package's ``LocalRenderer`` and float32 tensors on a ROCm device the head decode, the renderings, the loss
    and the gradient w.r.t. the NINE encoded channels are ONE fused HIP kernel (csrc/svbrdf_photo_loss.hip: 9 planes in,
    9 out, no 12-channel map tensor, none of the head's elementwise launches).  Any other renderer object, float64 on
    either side and ``backward(create_graph=True)`` take the composed definition above, which is also the specification
    of the fused path.  ``weights`` and ``normalize``: per-pixel confidence, exactly as ``PhotoLoss`` documents them.  A
    float32 ``[B,S,9]`` table that requires grad gets ``d loss/d scenes`` (camera, light, colour) from the same ONE launch
    (csrc/svbrdf_photo_pose.hip), loss and 9-channel gradient unchanged bit for bit; scene OBJECTS and a plugin renderer
    have no gradient towards light or camera positions."""

    def forward(self, encoded9, photos, scenes, weights=None, exposure=None):
        return self._forward(encoded9, photos, scenes, weights, head=True, exposure=exposure)
