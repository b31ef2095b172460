"""Fitting SVBRDF maps to photographs: one Adam step per kernel launch.

The loop a user of ``losses.PhotoLoss`` runs is

    loss = PhotoLoss(x, photos, scenes[, weights]);  loss.backward();  Adam.step();  x[:, 3:].clamp_(0, 1)

Loss and gradient are one launch; ``torch.optim.Adam`` and the clamp then make several more passes over the same
``[B,12,H,W]`` tensors.  A thread of the photo kernels holds its pixel's complete gradient in registers behind the scene
loop, and Adam is element-wise: ``PhotoFit.step`` is the whole line above in ONE launch (csrc/svbrdf_photo_fit.hip), the
gradient never written.

``PhotoFit.steps(n, ...)`` runs n consecutive steps on the same photographs in ceil(n / 64) launches, maps and state kept
on chip between the steps, bit for bit the n single steps.

``PhotoFit.step`` also refines what a real capture leaves unknown: with a scene table that requires grad and / or an
``exposure=`` that does, the same ONE launch returns ``d loss / d (camera, light position, light colour)`` as well
(csrc/svbrdf_photo_fit_pose.hip) and the loss it returns carries it to autograd -- towards the table and the gains only,
never towards the maps, which the launch has already updated.

``PhotoFit(maps, smooth=...)`` couples neighbouring pixels: an anisotropic total-variation prior on the maps
(``smoothness``) whose gradient joins the photo gradient inside the same ONE launch (csrc/svbrdf_photo_fit_smooth.hip).
Without it a pixel that no photograph sees never moves.

``composed_step`` is the same step in stock torch ops and the specification of the fused one.
"""
import ctypes
import math

import torch

from . import _native, losses, renderers


def adam_scalars(lr, beta1, beta2, step, dtype=torch.float32):
    """(c1, c2, step_size, rsb2) of Adam's step ``step``: c1 = 1 - beta1, c2 = 1 - beta2, step_size = lr / (1 - beta1^t),
    rsb2 = 1 / sqrt(1 - beta2^t).  float32: the library's derivation (svbrdf_photo_fit_adam_scalars: in double from the
    float32 arguments, each rounded once to float32).  Any other dtype: Python floats."""
    if dtype == torch.float32:
        return _native.photo_fit_adam_scalars(lr, beta1, beta2, step)
    if step < 1:
        raise ValueError("step must be >= 1")
    return 1.0 - beta1, 1.0 - beta2, lr / (1.0 - beta1 ** step), 1.0 / math.sqrt(1.0 - beta2 ** step)


def _check_hyper(lr, betas, eps):
    if not (math.isfinite(lr) and lr >= 0.0):
        raise ValueError("lr must be finite and >= 0, got %r" % (lr,))
    if not (math.isfinite(eps) and eps >= 0.0):
        raise ValueError("eps must be finite and >= 0, got %r" % (eps,))
    if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
        raise ValueError("betas must be two values in [0, 1), got %r" % (betas,))


def _check_bounds(bounds):
    """``bounds`` -> None or a host float32 [12,2] tensor of (lo, hi) per channel; +-inf = no bound on that side"""
    if bounds is None:
        return None
    b = torch.as_tensor(bounds, dtype=torch.float32, device="cpu").contiguous()
    if tuple(b.shape) != (12, 2):
        raise ValueError("bounds must be None or [12,2] (lo, hi per channel), got %s" % (tuple(b.shape),))
    if torch.isnan(b).any() or (b[:, 0] > b[:, 1]).any():
        raise ValueError("bounds must hold lo <= hi for every channel, and no NaN")
    return b


def _check_smooth(smooth):
    """``smooth`` -> None or a host float64 [12] tensor of lambdas, one per plane: 4 values (one per map group: normal,
    diffuse, roughness, specular) are expanded x3"""
    if smooth is None:
        return None
    lam = torch.as_tensor(smooth, dtype=torch.float64, device="cpu").reshape(-1)
    if lam.numel() == 4:
        lam = lam.repeat_interleave(3)
    if lam.numel() != 12:
        raise ValueError("smooth must be None, 4 values (normal, diffuse, roughness, specular) or 12 (one per plane), got %d"
                         % lam.numel())
    if not torch.isfinite(lam).all() or (lam < 0).any():
        raise ValueError("smooth must hold finite values >= 0")
    return lam.contiguous()


def smoothness(maps, lam):
    """The smoothness prior R(x) of a ``[B,12,H,W]`` map tensor in stock torch ops, differentiable, any dtype and device --
    THE SPECIFICATION of what ``PhotoFit(smooth=lam)`` adds to the photo loss, and what to call to monitor it:

        R(x) = sum_ch lam[ch] / (B H W) sum_b ( sum_{i, j<W-1} |x[b,ch,i,j+1] - x[b,ch,i,j]|
                                              + sum_{i<H-1, j} |x[b,ch,i+1,j] - x[b,ch,i,j]| )

    an anisotropic total variation per plane, no wrap-around, no coupling between items.  ``lam``: 12 finite values >= 0,
    or 4 (one per map group, expanded x3).  lam[ch] / (B H W) is formed in double and rounded once to the maps' dtype.
    -> 0-dim tensor."""
    if maps.dim() != 4 or maps.shape[1] != 12:
        raise ValueError("maps must be [B,12,H,W]")
    lam = _check_smooth(lam)
    if lam is None:
        raise ValueError("lam must be 4 or 12 values")
    B, _, H, W = maps.shape
    scale = (lam / float(B * H * W)).to(device=maps.device, dtype=maps.dtype)
    tv = (maps[:, :, :, 1:] - maps[:, :, :, :-1]).abs().sum(dim=(0, 2, 3)) + (maps[:, :, 1:, :] - maps[:, :, :-1, :]).abs().sum(dim=(0, 2, 3))
    return (tv * scale).sum()


def _wants_grad(scenes, exposure):
    """a step's loss is differentiable: grad mode is on and the scene table (a tensor) or the exposure requires grad"""
    return torch.is_grad_enabled() and ((isinstance(scenes, torch.Tensor) and scenes.requires_grad)
                                        or (exposure is not None and exposure.requires_grad))


class _StepLoss(torch.autograd.Function):
    """The loss of a step that has ALREADY updated the maps, differentiable towards ``inputs`` (the scene table, the
    exposure) and towards nothing else.  ``forward`` makes the step -- ``run()`` -> (0-dim loss, d loss / d input for
    every input, or None) -- so maps and state are updated when it returns, and keeps the gradients; ``backward`` returns
    ``grad_loss * gradient``.  The gradients are those at the maps BEFORE the update: what ``loss.backward();
    opt_maps.step(); opt_pose.step()`` gives in the composed loop.  Once differentiable: a double backward raises."""

    @staticmethod
    def forward(ctx, run, *inputs):
        loss, grads = run()
        ctx.save_for_backward(*grads)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        return (None,) + tuple(None if g is None else (grad_loss * g).to(g.dtype) for g in ctx.saved_tensors)


def composed_step(maps, exp_avg, exp_avg_sq, step, photos, scenes, weights=None, lr=1e-2, betas=(0.9, 0.999), eps=1e-8,
                  bounds=None, loss_eps=0.1, renderer=None, exposure=None, smooth=None):
    """One step of the fit in stock torch ops -- THE SPECIFICATION of ``PhotoFit.step``: the gradient g of
    ``losses.PhotoLoss(renderer, loss_eps)(maps, photos, scenes, weights)``, then per element, each operation rounded in
    the maps' dtype,

        m' = (beta1 m) + (c1 g)
        v' = (beta2 v) + ((c2 g) g)
        den = (sqrt(v') rsb2) + eps
        x' = x - (step_size (m' / den))
        x' = clamp(x', lo[ch], hi[ch])          a NaN stays a NaN; +-inf = no bound

    with ``adam_scalars(lr, *betas, step)``.  ``maps``, ``exp_avg``, ``exp_avg_sq`` are updated in place; ``step`` is
    Adam's t of this update (1 for the first).  Serves float64 maps, CPU tensors and plugin renderers too -- whatever
    ``PhotoLoss`` serves.  ``exposure``: PhotoLoss's per-photo gains.  -> the 0-dim loss at the maps before the update.

    With grad mode on and a ``scenes`` tensor or an ``exposure`` that requires grad, the returned loss carries its graph
    towards them -- ``d loss / d scenes`` and ``d loss / d exposure`` at the maps before the update, as ``PhotoLoss``
    defines them -- and not towards the maps; otherwise it is detached.

    ``smooth``: None, or 4 / 12 lambdas: the gradient is that of the photo loss + ``smoothness(maps, smooth)``, the prior's
    added to the photo gradient on the planes whose lambda is not 0 (the others keep g bit for bit; all zeros is None).
    The loss returned stays the photo term."""
    _check_hyper(lr, betas, eps)
    bounds = _check_bounds(bounds)
    smooth = _check_smooth(smooth)
    if smooth is not None and not smooth.any():
        smooth = None
    fn = losses.PhotoLoss(renderer if renderer is not None else renderers.LocalRenderer(), loss_eps)
    wanted = []
    if _wants_grad(scenes, exposure):
        wanted = [t for t in (scenes, exposure) if isinstance(t, torch.Tensor) and t.requires_grad]
    update = lambda: _composed_update(fn, maps, exp_avg, exp_avg_sq, step, photos, scenes, weights, exposure, lr, betas, eps,
                                      bounds, wanted, smooth)
    return _StepLoss.apply(update, *wanted) if wanted else update()[0]


def _composed_update(fn, maps, exp_avg, exp_avg_sq, step, photos, scenes, weights, exposure, lr, betas, eps, bounds, wanted,
                     smooth=None):
    """composed_step's body -> (the detached loss, d loss / d t for every t of ``wanted``, None where no gradient reaches
    t).  With nothing wanted the table and the gains are constants, whatever requires grad."""
    x = maps.detach().clone().requires_grad_(True)
    if not wanted:
        scenes = scenes.detach() if isinstance(scenes, torch.Tensor) else scenes
        exposure = None if exposure is None else exposure.detach()
    with torch.enable_grad():
        loss = fn(x, photos, scenes, weights, exposure)
        # (a plugin renderer works with scene objects: no gradient reaches the table, as in PhotoLoss)
        g, *grads = torch.autograd.grad(loss, [x] + wanted, allow_unused=True)
        if smooth is not None:
            prior, = torch.autograd.grad(smoothness(x, smooth), [x])
            g = torch.where((smooth != 0).to(g.device).view(1, 12, 1, 1), g + prior, g)
    c1, c2, step_size, rsb2 = adam_scalars(lr, betas[0], betas[1], step, maps.dtype)
    with torch.no_grad():
        m = exp_avg.mul_(betas[0]).add_(g * c1)
        v = exp_avg_sq.mul_(betas[1]).add_((g * c2) * g)
        den = (v.sqrt() * rsb2) + eps
        xn = maps - (m / den) * step_size
        if bounds is not None:
            lo = bounds[:, 0].to(maps.device, maps.dtype).view(1, 12, 1, 1)
            hi = bounds[:, 1].to(maps.device, maps.dtype).view(1, 12, 1, 1)
            xn = torch.where(xn < lo, lo, xn)        # false for NaN: it stays
            xn = torch.where(xn > hi, hi, xn)
        maps.copy_(xn)
    return loss.detach(), tuple(None if t is None else t.detach() for t in grads)


class PhotoFit:
    """Adam on a ``[B,12,H,W]`` map tensor under the photo loss, one launch per step.

        fit = PhotoFit(maps, lr=1e-2, bounds=[[-inf, inf]] * 3 + [[0, 1]] * 9)
        for _ in range(200):
            loss = fit.step(photos, scenes)          # 0-dim device tensor: the loss BEFORE this update; no host sync

    ``maps`` is updated in place (a leaf that requires grad is updated through ``.data``, like an optimiser does).
    ``lr``, ``betas``, ``eps`` are ``torch.optim.Adam``'s (no AMSGrad, no weight decay) and may be reassigned between
    steps; ``bounds``: None, or ``[12,2]`` (lo, hi) per channel applied to the updated maps, +-inf = none on that side;
    ``loss_eps``: PhotoLoss's eps; ``renderer``: None = this package's ``LocalRenderer``.

    ``smooth``: None, or the lambdas of the smoothness prior across pixels -- 4 values (normal, diffuse, roughness,
    specular) or 12 (one per plane), finite and >= 0, reassignable like ``bounds``.  The objective is then the photo loss
    + ``smoothness(maps, smooth)``; the loss ``step`` returns stays the photo term.  On the fused path the step is still
    ONE launch (svbrdf_photo_fit_smooth_adam_step[_scene_grad]), out of place for the maps -- a pixel's neighbours must be
    read as they were before the update -- into a spare buffer this object owns, then copied back: ``maps`` is updated in
    place as ever.  ``steps(n)`` alternates between the two buffers, n launches and one copy only when n is odd.  None or
    all zeros: the entries without the prior.

    The optimiser state has ``torch.optim.Adam``'s names and meaning, readable and assignable: ``fit.exp_avg``,
    ``fit.exp_avg_sq`` (tensors like ``maps``) and the number of updates made so far, ``fit.state["step"]`` -- ``state`` is
    the dict ``Adam.state[p]`` would be (the counter has no attribute of its own: ``step`` is the method).

    float32 maps on a ROCm device with ``LocalRenderer``: ``step`` is ONE fused kernel
    (svbrdf_photo_fit_adam_step; svbrdf_photo_fit_adam_step_scene_grad when the scene table or the exposure wants a
    gradient, see ``step``).  Anything else -- float64 maps, CPU tensors, a plugin renderer -- is ``composed_step``, the
    specification of the fused step."""

    def __init__(self, maps, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, bounds=None, loss_eps=0.1, renderer=None, smooth=None):
        if not isinstance(maps, torch.Tensor) or maps.dim() != 4 or maps.shape[1] != 12 or not maps.dtype.is_floating_point:
            raise ValueError("maps must be a floating-point [B,12,H,W] tensor")
        if not maps.is_contiguous():
            raise ValueError("maps are updated in place: a contiguous tensor")
        _check_hyper(lr, betas, eps)
        self.maps = maps
        self.lr, self.betas, self.eps, self.loss_eps = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(loss_eps)
        self.renderer = renderer if renderer is not None else renderers.LocalRenderer()
        self.bounds = bounds
        self.smooth = smooth
        self._spare = None
        self.state = {"step": 0, "exp_avg": torch.zeros_like(maps.detach()), "exp_avg_sq": torch.zeros_like(maps.detach())}

    exp_avg = property(lambda self: self.state["exp_avg"], lambda self, t: self.state.__setitem__("exp_avg", t))
    exp_avg_sq = property(lambda self: self.state["exp_avg_sq"], lambda self, t: self.state.__setitem__("exp_avg_sq", t))

    @property
    def bounds(self):
        return self._bounds

    @bounds.setter
    def bounds(self, value):
        self._bounds = _check_bounds(value)
        # the fused step takes them from the host, 24 floats in the launch's argument block
        self._bounds_c = None if self._bounds is None else (ctypes.c_float * 24)(*self._bounds.reshape(-1).tolist())

    @property
    def smooth(self):
        return self._smooth

    @smooth.setter
    def smooth(self, value):
        self._smooth = _check_smooth(value)
        # the fused step takes the lambdas from the host, 12 floats in the launch's argument block; None: no prior
        on = self._smooth is not None and bool(self._smooth.any())
        self._smooth_c = (ctypes.c_float * 12)(*self._smooth.tolist()) if on else None

    def _spare_for(self, x):
        """the buffer the out-of-place step writes: like ``x``, owned by this object, never the user's tensor"""
        if self._spare is None or self._spare.shape != x.shape or self._spare.device != x.device or self._spare.dtype != x.dtype:
            self._spare = torch.empty_like(x)
        return self._spare

    def uses_fused_kernel(self):
        return (losses.RenderingLoss.uses_fused_kernel(self) and self.maps.is_cuda     # (its rule, on this renderer)
                and self.maps.dtype == torch.float32)

    def _fused_inputs(self, x, photos, scenes, weights, exposure, constants):
        """What ``step`` and ``steps`` hand the fused entries, or None where the update is ``composed_step``'s (anything but
        float32 maps on a ROCm device with ``LocalRenderer``, and float64 gains) -> (photos, weights, table, want): photos
        and weights checked as PhotoLoss checks them; the scene table with the checked gains multiplied into its colour
        columns; want = the loss is differentiable towards table and gains (never with ``constants``).  Without ``want``
        table and gains are detached, and a table without gains stays where it is: the binding uploads it."""
        if not self.uses_fused_kernel() or (isinstance(exposure, torch.Tensor) and exposure.dtype == torch.float64):
            return None
        photos = losses.PhotoLoss._check(x, photos)
        weights = losses._check_weights(weights, x, photos)
        exposure = losses._check_exposure(exposure, x, photos)
        table = losses.PhotoLoss._scene_table(scenes, photos.shape[0], photos.shape[1])
        want = not constants and _wants_grad(table, exposure)
        if not want:
            table = table.detach()
            exposure = None if exposure is None else exposure.detach()
        if want or exposure is not None:
            # the kernels take a device table and no exposure: the gains multiply the colour columns in front of them
            # (_PhotoLossModule._forward), and autograd chains the table's gradient back through both
            table = table.to(x.device)
            if exposure is not None:
                table = losses.fold_exposure(table, exposure)
        return photos, weights, table, want

    def step(self, photos, scenes, weights=None, exposure=None):
        """One update from ``photos`` [B,S,3,H,W] (or [B,3,H,W]), ``scenes``, optional ``weights`` and optional ``exposure``
        (a positive gain per photo and colour channel) as ``losses.PhotoLoss`` takes them -> the 0-dim loss at the maps
        before the update.

        The light, the camera and the gains are refined WITH the maps: with grad mode on and ``scenes`` a float32
        ``[B,S,9]`` tensor that requires grad (PhotoLoss's signal) and / or an ``exposure`` that requires grad, the returned
        loss is attached to autograd towards ``scenes`` and ``exposure`` -- never towards the maps, which are already
        updated when ``step`` returns -- and ``loss.backward()`` deposits ``d loss / d scenes`` (camera xyz | light xyz |
        light rgb) at the maps BEFORE the update, once differentiable.  Still ONE launch on the fused path
        (svbrdf_photo_fit_adam_step_scene_grad); the gains multiply the table's colour columns with torch ops in front of
        it, and autograd chains the colour gradient back to them, through ``log_e.exp()`` too.  The update of the table and
        of the gains is the caller's: a stock ``torch.optim`` over a few hundred floats.

        With nothing that requires grad, or under ``torch.no_grad()``, it is the step without a table gradient: one launch
        of svbrdf_photo_fit_adam_step, a loss that does not require grad, a given ``exposure`` multiplied in as a
        constant."""
        x = self.maps.detach()
        t = int(self.state["step"]) + 1
        fused = self._fused_inputs(x, photos, scenes, weights, exposure, constants=False)
        if fused is None:
            loss = composed_step(x, self.exp_avg, self.exp_avg_sq, t, photos, scenes, weights, self.lr, self.betas, self.eps,
                                 self._bounds, self.loss_eps, self.renderer, exposure, self._smooth)
        else:
            photos, weights, table, want = fused
            rest = (self.lr, self.betas, self.eps, self._bounds_c, self.loss_eps, weights)

            def launch(table, **kw):
                if self._smooth_c is None:
                    return _native.photo_fit_adam_step(x, self.exp_avg, self.exp_avg_sq, photos, table, t, *rest, **kw)
                # out of place with the prior: into the spare buffer, then back -- ``maps`` is updated in place
                spare = self._spare_for(x)
                out = _native.photo_fit_smooth_adam_step(x, spare, self.exp_avg, self.exp_avg_sq, photos, table, t,
                                                         self._smooth_c, *rest, **kw)
                x.copy_(spare)
                return out

            def joint():
                loss, _, grad_scenes = launch(table.detach(), want_scene_grad=True)
                return loss.view(()), (grad_scenes,)

            if want:
                loss = _StepLoss.apply(joint, table)
            else:
                loss = launch(table)[0].view(())
        self.state["step"] = t
        return loss

    def steps(self, n, photos, scenes, weights=None, exposure=None):
        """``n`` consecutive updates from the same ``photos``, ``scenes`` and ``weights`` -> a ``[n]`` device tensor of the
        losses at the maps before each update; no host synchronisation.  Maps, state and losses are those of ``n`` calls
        of ``step`` -- on the fused path bit for bit, in ceil(n / 64) launches (svbrdf_photo_fit_adam_steps: the thread
        that owns a pixel runs the steps on it with maps and state kept on chip; csrc/svbrdf_photo_fit.hip).  ``lr``,
        ``betas``, ``eps`` and ``bounds`` are read once per call; ``state["step"]`` advances by ``n``.  Anything but float32
        maps on a ROCm device with ``LocalRenderer`` is ``n`` times ``composed_step``.

        With ``smooth`` the fused path is ``n`` LAUNCHES of the single step, alternating between ``maps`` and the spare
        buffer, and one copy back only when n is odd: a second step needs the neighbours' updated values, which inside one
        launch would take a grid barrier.

        Maps only: the table and the ``exposure`` gains are CONSTANTS of the n steps, whatever requires grad, and the losses
        returned are never differentiable.  The table's gradient is a sum over all pixels of an item; applying it between
        two steps of one launch would need a grid barrier (csrc/svbrdf_photo_fit_pose.hip).  To refine the table, call
        ``step`` in a loop."""
        n = int(n)
        if n < 1:
            raise ValueError("n must be >= 1, got %r" % (n,))
        x = self.maps.detach()
        lr, betas, eps, bounds, bounds_c = self.lr, self.betas, self.eps, self._bounds, self._bounds_c
        t = int(self.state["step"]) + 1
        fused = self._fused_inputs(x, photos, scenes, weights, exposure, constants=True)
        if fused is None:
            seen = []
            with torch.no_grad():
                for k in range(n):
                    seen.append(composed_step(x, self.exp_avg, self.exp_avg_sq, t + k, photos, scenes, weights, lr, betas,
                                              eps, bounds, self.loss_eps, self.renderer, exposure, self._smooth))
                    self.state["step"] = t + k
            return torch.stack(seen)
        photos, weights, table, _ = fused
        out = []
        if self._smooth_c is not None:
            src, dst = x, self._spare_for(x)
            for k in range(n):
                out.append(_native.photo_fit_smooth_adam_step(src, dst, self.exp_avg, self.exp_avg_sq, photos, table, t + k,
                                                              self._smooth_c, lr, betas, eps, bounds_c, self.loss_eps,
                                                              weights)[0])
                src, dst = dst, src
                self.state["step"] = t + k
            if src is not x:        # n is odd: the result stands in the spare buffer
                x.copy_(src)
            return torch.cat(out)
        for first in range(0, n, _native.PHOTO_FIT_MAX_STEPS):
            k = min(_native.PHOTO_FIT_MAX_STEPS, n - first)
            out.append(_native.photo_fit_adam_steps(x, self.exp_avg, self.exp_avg_sq, photos, table, t + first, k, lr, betas,
                                                    eps, bounds_c, self.loss_eps, weights))
            self.state["step"] = t + first + k - 1
        return out[0] if len(out) == 1 else torch.cat(out)
