"""Fit SVBRDF maps to photographs with the fused photo loss (losses.PhotoLoss): the inverse-rendering use of the engine.

    python tools/fit_photos.py [--size 256] [--batch 2] [--photos 9] [--steps 200] [--lr 0.01] [--noise] [--seed 1]
                               [--fit-exposure] [--fit-pose [--pose-lr 0.002]] [--fused-step [--steps-per-launch K]]
                               [--captured [--sensor 640x480] [--clip 250] [--fit-registration [--corner-noise PX]]]
                               [--smooth LAMBDA]

Ground-truth maps come from the tests' deterministic generator (tests/synth.py); their photographs and the light / view of
each from ``synthesis.render_inputs`` (the scene table is what that call draws from torch's global generator: the same seed
gives it again).  A perturbed copy of the maps is then a leaf tensor that Adam fits to the photographs through
``PhotoLoss`` -- one kernel launch per step for loss and gradient.  Prints the loss per step and the time per step.

``--fit-exposure``: every photograph is taken with a HIDDEN gain per colour channel in [0.5, 2] (an unknown flash power and
white balance: the light colour of its scene row times the gain, noise-free, clamped to [0, 1]).  The fit starts from a gain
of 1 and fits the gains jointly with the maps, the parameter in log space (``exposure=log_e.exp()``), still one launch per
step for the loss and both gradients; the mean |log e - log e*| is printed beside the maps' error.

``--fit-pose``: the fit is GIVEN camera and light positions that are a few per cent off (a camera from a homography, a flash
"somewhere next to the lens") and fits the six position columns of the scene table jointly with the maps -- and with the
gains under ``--fit-exposure`` -- through the table's gradient, which comes out of the same one launch per step; the mean
|position - truth| is printed beside the maps' error.  The positions take their own learning rate, ``--pose-lr``.

``--fused-step``: the whole step -- loss, gradient, Adam update of the maps and the clamp of diffuse, roughness and specular
to [0, 1] -- is ONE launch (``fitting.PhotoFit``: the gradient is never written, ``torch.optim.Adam`` is not used for the
maps).  With ``--fit-pose`` and / or ``--fit-exposure`` the same one launch also returns the gradient towards the scene
table (``fit.step(photos, cat(pos, colour), None, exposure=log_e.exp())``): ``loss.backward()`` hands it to the positions and,
through the colour columns, to ``log e``, and a small Adam over those few hundred floats follows (``--pose-lr`` as above).

``--steps-per-launch K`` (only with ``--fused-step``): K consecutive steps per launch (``fitting.PhotoFit.steps``: the thread
that owns a pixel runs them with maps and state kept on chip, read from memory once and written once per launch; ceil(K / 64)
launches).  Maps and losses are bit for bit those of K single-step launches.  The losses of every ``--print-every``-th step
are printed from the returned tensor -- the maps' error only where a launch ends, the maps in between never reach memory --
and the time per step is the time of a launch divided by its steps.  Maps only: refused with ``--fit-pose`` or
``--fit-exposure`` -- the table's gradient sums over all pixels, and applying it between two steps of one launch would need a
grid barrier.

``--captured``: the fit is run twice, once on the photographs as synthesised on the patch grid (as without the option) and
once on what a camera would deliver.  Every synthesised photograph is pushed through ``capture.to_perspective`` from its own
camera position onto a ``--sensor`` of WIDTHxHEIGHT pixels, encoded with gamma 2.2 to 8 bits on the host, and ingested again
with ``capture.rectify``: the homography of the patch corners the camera sees (``camera_corners`` / ``patch_homography``),
``gamma_lut()``, 2 x 2 sub-samples, codes of 0 (the border around the patch) and of ``--clip`` or more (clipped highlights)
refused.  The material of this mode is band limited (the generator's maps at an eighth of the size, enlarged): photographs
of per-pixel white noise survive no resampling.  The second fit runs on the rectified photographs WITH their weights through the same path as the first
(``--fused-step`` included); with ``--fit-pose`` its camera positions start from ``capture.camera_from_corners`` instead of
from the perturbed truth.  The share of zero weights and both final map errors are printed at the end.

``--fit-registration`` (only with ``--captured``): two more fits, on photographs whose four patch corners are GIVEN off by up
to ``--corner-noise`` source pixels per coordinate (somebody clicked them).  The first leaves them as given: every
photograph sits shifted against the others on the grid, and the fit averages that into its maps.  The second refines them:
every ``--registration-every`` map steps it renders the current maps under the scene table (K1, detached), takes
``--registration-steps`` Adam steps on the eight corner coordinates of every photograph with
``sum w |log(R + eps) - log(rect + eps)| / sum w`` in stock torch ops through the differentiable ``capture.rectify``
(``capture.corner_matrices``; forward and backward one launch each; dividing by ``sum w`` keeps a rectangle that shrinks out
of the image from looking like progress), and rectifies again.  The mean corner error is printed at every stage and both
final map errors at the end.  Whether alternating with maps that are still wrong converges is not known in general: the
tool records what it does.  Not with ``--steps-per-launch``.

``--smooth LAMBDA``: a smoothness prior across pixels on diffuse, roughness and specular (``fitting.smoothness`` with LAMBDA on
those nine planes, 0 on the normals): the objective is the photo loss + the prior, the loss printed stays the photo term.
Without it a pixel that no photograph sees -- every weight 0, as under ``--captured`` -- has an all-zero gradient and stays at
its start value.  On the unfused path the prior is added to the loss with torch ops; with ``--fused-step`` its gradient is
formed inside the one launch (``fitting.PhotoFit(smooth=...)``), with ``--fit-pose`` / ``--fit-exposure`` too.  With
``--steps-per-launch K`` it is K LAUNCHES per call of ``steps`` (a second step needs the neighbours' updated values).  The
map error on the never-seen pixels is printed beside the overall one.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import synth  # noqa: E402
from svbrdf_estimation_amd import _native, capture, fitting, losses, renderers, synthesis  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--photos", type=int, default=9, help="photographs per material")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--noise", action="store_true", help="sensor noise on the photographs (dataset.py:215-217)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--print-every", type=int, default=10)
    ap.add_argument("--fit-exposure", action="store_true", help="photographs with hidden per-photo gains, fitted with the maps")
    ap.add_argument("--fit-pose", action="store_true", help="camera and light positions given a few per cent off, fitted with the maps")
    ap.add_argument("--pose-lr", type=float, default=0.002)
    ap.add_argument("--fused-step", action="store_true", help="loss, gradient, Adam update and clamp of the maps in one launch")
    ap.add_argument("--steps-per-launch", type=int, default=None, help="with --fused-step: this many consecutive steps per launch")
    ap.add_argument("--captured", action="store_true", help="fit a second time, on 8-bit perspective photographs rectified onto the grid")
    ap.add_argument("--sensor", default="640x480", help="with --captured: the camera's sensor, WIDTHxHEIGHT pixels")
    ap.add_argument("--clip", type=int, default=250, help="with --captured: codes of this value or more are clipped highlights")
    ap.add_argument("--fit-registration", action="store_true",
                    help="with --captured: the patch corners are given a few pixels off and refined against renderings of the maps")
    ap.add_argument("--corner-noise", type=float, default=2.0, metavar="PX", help="with --fit-registration: source pixels per coordinate")
    ap.add_argument("--registration-every", type=int, default=20, help="map steps between two registration stages")
    ap.add_argument("--registration-steps", type=int, default=5, help="Adam steps on the corners per stage")
    ap.add_argument("--registration-lr", type=float, default=0.1, help="Adam learning rate of the corners, source pixels")
    ap.add_argument("--smooth", type=float, default=None, metavar="LAMBDA",
                    help="smoothness prior across pixels on diffuse, roughness and specular (normals stay at 0); with "
                         "--steps-per-launch K it is K launches, not one")
    args = ap.parse_args()
    if args.smooth is not None and not (args.smooth >= 0.0 and args.smooth < float("inf")):
        ap.error("--smooth must be finite and >= 0")
    if args.steps_per_launch is not None and not args.fused_step:
        ap.error("--steps-per-launch needs --fused-step: only the fused step runs several steps in a launch")
    if args.steps_per_launch is not None and args.steps_per_launch < 1:
        ap.error("--steps-per-launch must be >= 1")
    if args.steps_per_launch is not None and (args.fit_exposure or args.fit_pose):
        ap.error("--steps-per-launch updates the maps only: positions and gains would have to be updated between the steps of "
                 "a launch, from a gradient summed over all pixels (a grid barrier) -- use --fused-step without it")
    if args.fit_registration and (not args.captured or args.steps_per_launch is not None):
        ap.error("--fit-registration refines the corners of --captured photographs between single map steps")
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    B, H, S = args.batch, args.size, args.photos
    truth = torch.from_numpy(synth.make_maps(args.seed, B, H)).to(dev)
    if args.captured:
        truth = band_limited_maps(args.seed, B, H).to(dev)
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed(args.seed)
    photos = synthesis.render_inputs(truth, S, use_augmentation=True, noise="device" if args.noise else None)
    torch.manual_seed(args.seed)
    table = torch.stack([synthesis.input_scene_table(S, True) for _ in range(B)], dim=0).to(dev)
    hidden = None
    if args.fit_exposure:
        if args.noise:
            ap.error("--fit-exposure renders its photographs noise-free: not combined with --noise")
        hidden = 0.5 + 1.5 * torch.from_numpy(synth.uniform01(args.seed + 2000, (B, S, 3))).to(dev)
        scaled = torch.cat((table[..., :6], table[..., 6:] * hidden), dim=-1)
        photos = _native.render_fwd(truth, scaled).clamp_(0.0, 1.0)
    if not args.captured:
        return fit(args, dev, truth, photos, table, hidden)
    on_grid = fit(args, dev, truth, photos, table, hidden)
    rectified, weights, cameras, images, corners = ingest(args, dev, photos, table)
    seen = weights.unsqueeze(2).expand_as(photos) > 0
    print("--- the same fit on the captured photographs: %s sensor, gamma 2.2, 8 bits, rectified with 2 x 2 sub-samples; "
          "%.2f %% of the weights are zero, %.2f %% of the pixels are seen by no photograph; mean |rectified - on the grid| %.5f "
          "where the weight is 1" % (args.sensor, 100.0 * (weights == 0).float().mean().item(),
                                     100.0 * (weights.amax(dim=1) == 0).float().mean().item(),
                                     (rectified - photos)[seen].abs().mean().item()))
    captured = fit(args, dev, truth, rectified, table, hidden, weights, cameras)
    print("final mean |d,r,s - truth|: on the grid %.5f, captured %.5f (zero weights: %.2f %%)" % (
        on_grid, captured, 100.0 * (weights == 0).float().mean().item()))
    if not args.fit_registration:
        return
    noise = args.corner_noise * (2.0 * synth.uniform01(args.seed + 4000, corners.shape) - 1.0)
    results = []
    for refine in (False, True):
        reg = Registration(args, images, corners, corners + noise, H)
        print("--- the captured fit with every corner coordinate given up to %g source pixels off (mean corner error %.3f px), %s"
              % (args.corner_noise, reg.error(), "refined every %d map steps (%d Adam steps, lr %g)" % (
                  args.registration_every, args.registration_steps, args.registration_lr) if refine else "left as given"))
        shifted, w = reg.rectify()
        results.append((fit(args, dev, truth, shifted, table, hidden, w, cameras, reg if refine else None), reg.error()))
    print("final mean |d,r,s - truth|: true corners %.5f; corners %g px off, as given %.5f (corner error %.3f px), refined %.5f "
          "(corner error %.3f px)" % (captured, args.corner_noise, results[0][0], results[0][1], results[1][0], results[1][1]))


class Registration:
    """--fit-registration: the corners of every captured photograph as an Adam parameter, float64 [B,S,4,2] on the host"""

    EPS = 0.01

    def __init__(self, args, images, true_corners, start_corners, H):
        self.args, self.images, self.H = args, images, H
        self.true = torch.from_numpy(true_corners)
        self.corners = torch.from_numpy(start_corners).clone().requires_grad_(True)
        self.opt = torch.optim.Adam([self.corners], lr=args.registration_lr)
        self.lut = capture.gamma_lut()

    def error(self):
        return (self.corners.detach() - self.true).norm(dim=-1).mean().item()

    def rectify(self, grad=False):
        M = capture.corner_matrices(self.corners, self.H)
        return capture.rectify(self.images, M if grad else M.detach(), self.H, lut=self.lut, clip=(0, self.args.clip), samples=2)

    def refine(self, maps, scenes):
        """one stage: a few Adam steps on the corners against the rendering of `maps` under `scenes` -> (photos, weights)"""
        with torch.no_grad():
            log_r = (_native.render_fwd(maps.detach().contiguous(), scenes.detach().contiguous()).clamp_(0.0, 1.0) + self.EPS).log()
        for _ in range(self.args.registration_steps):
            self.opt.zero_grad(set_to_none=True)
            rect, w = self.rectify(grad=True)
            loss = (w.unsqueeze(2) * (log_r - (rect + self.EPS).log()).abs()).sum() / (3.0 * w.sum())
            loss.backward()
            self.opt.step()
        return self.rectify()


def band_limited_maps(seed, B, H, cell=8):
    """--captured: the generator's maps at 1 / `cell` of the size, enlarged bilinearly, normals renormalised.  The generator
    draws every pixel independently; photographs of white noise survive no resampling at all (rectifying them gives the mean
    of unrelated neighbours), so the captured mode -- both of its fits -- uses a material whose features span a few pixels."""
    small = torch.from_numpy(synth.make_maps(seed, B, max(H // cell, 2)))
    maps = torch.nn.functional.interpolate(small, size=(H, H), mode="bilinear", align_corners=True)
    maps[:, :3] = maps[:, :3] / maps[:, :3].norm(dim=1, keepdim=True)
    return maps.contiguous()


def ingest(args, dev, photos, table):
    """--captured: the photographs as a camera at each photo's position delivers them -- perspective, gamma 2.2, 8 bits --
    and back onto the grid -> (photos [B,S,3,H,W], weights [B,S,H,W], the camera positions recovered from the corners, the
    8-bit images [B,S,h,w,3], the corners [B,S,4,2] in their pixels)"""
    sensor = tuple(int(v) for v in args.sensor.lower().split("x"))
    B, S, H = photos.shape[0], photos.shape[1], photos.shape[-1]
    cams = table[..., :3].cpu().numpy().astype(np.float64)
    seen = capture.to_perspective(photos, cams, sensor)                                  # [B,S,3,sensor h,sensor w]
    codes = (seen.clamp(0.0, 1.0).cpu().double().pow(1.0 / 2.2) * 255.0).round().to(torch.uint8)
    images = codes.permute(0, 1, 3, 4, 2).contiguous().to(dev)                           # what an image decoder returns: HWC
    corners = [capture.camera_corners(c, sensor) for c in cams.reshape(-1, 3)]
    matrices = np.stack([capture.patch_homography(c, (H, H)) for c in corners]).reshape(B, S, 3, 3)
    rectified, weights = capture.rectify(images, matrices, H, lut=capture.gamma_lut(), clip=(0, args.clip), samples=2)
    recovered = np.stack([capture.camera_from_corners(c, sensor) for c in corners]).reshape(B, S, 3)
    return rectified, weights, torch.from_numpy(recovered).float().to(dev), images, np.stack(corners).reshape(B, S, 4, 2)


def map_error(x, truth, unseen):
    """-> (mean |d,r,s - truth| over all pixels, the text that reports it -- with the never-seen pixels' own beside it)"""
    diff = (x.detach()[:, 3:] - truth[:, 3:]).abs()
    err = diff.mean().item()
    text = "mean |d,r,s - truth| %.5f" % err
    if unseen is not None and unseen.any():
        text += " (never seen: %.5f)" % diff[unseen.expand_as(diff)].mean().item()
    return err, text


def fit(args, dev, truth, photos, table, hidden, weights=None, cameras=None, registration=None):
    """one fit of perturbed maps to `photos` (with `weights`, if given) -> the final mean |d,r,s - truth|.  `registration`: a
    Registration whose stage replaces `photos` and `weights` every --registration-every steps."""
    B, H, S = args.batch, args.size, args.photos
    unseen = None if weights is None else weights.amax(dim=1, keepdim=True) == 0      # [B,1,H,W]: no photograph sees it
    lam = None if args.smooth is None else [0.0, args.smooth, args.smooth, args.smooth]
    log_e = torch.zeros((B, S, 3), device=dev, requires_grad=True) if args.fit_exposure else None
    pos, true_pos, colour = None, table[..., :6], table[..., 6:]
    if args.fit_pose:
        off = 1.0 + 0.06 * (torch.from_numpy(synth.uniform01(args.seed + 3000, (B, S, 6))).to(dev) - 0.5)
        pos = true_pos * off                                                 # every coordinate up to 3 % off
        if cameras is not None:                                              # --captured: the camera from the corners it saw
            pos = torch.cat((cameras, pos[..., 3:]), dim=-1)
        pos = pos.requires_grad_(True)
    start = truth.clone()
    jitter = torch.from_numpy(synth.uniform01(args.seed + 1000, (B, 9, H, H))).to(dev) - 0.5
    start[:, 3:] = (start[:, 3:] + 0.3 * jitter).clamp_(0.02, 0.98)        # diffuse, roughness, specular off by up to 0.15
    x = start.clone().requires_grad_(True)
    fn = losses.PhotoLoss(renderers.LocalRenderer())
    groups = [{"params": [x] if log_e is None else [x, log_e]}] + ([] if pos is None else [{"params": [pos], "lr": args.pose_lr}])
    opt = torch.optim.Adam(groups, lr=args.lr)
    fit = None
    if args.fused_step:
        inf = float("inf")
        fit = fitting.PhotoFit(x.detach(), lr=args.lr, bounds=[[-inf, inf]] * 3 + [[0.0, 1.0]] * 9, smooth=lam)
        # the maps are the fused step's; what is left for torch.optim is the few hundred floats of gains and positions
        groups = ([] if log_e is None else [{"params": [log_e]}]) + ([] if pos is None else [{"params": [pos], "lr": args.pose_lr}])
        opt = torch.optim.Adam(groups, lr=args.lr) if groups else None
    print("fitting %d x [12,%d,%d] maps to %d photographs each (%s%s%s), Adam lr %g%s" % (
        B, H, H, S, "sensor noise" if args.noise else "noise-free", ", hidden gains fitted too" if args.fit_exposure else "",
        ", positions fitted too (lr %g)" % args.pose_lr if args.fit_pose else "", args.lr,
        ", the whole step in one launch" if fit is not None else "")
        + ("" if lam is None else ", smoothness prior %g on d, r, s" % args.smooth))
    if args.steps_per_launch is not None:
        return run_in_launches(args, fit, photos, table, x, truth, weights, unseen)
    t_last, step_ms = None, []
    for step in range(args.steps):
        if step % args.print_every == 0:
            torch.cuda.synchronize()
            now = time.perf_counter()
            if t_last is not None:
                step_ms.append(1e3 * (now - t_last) / args.print_every)
            t_last = now
        if registration is not None and step and step % args.registration_every == 0:
            with torch.no_grad():
                scenes = table if pos is None else torch.cat((pos, colour), dim=-1)
                if log_e is not None:
                    scenes = torch.cat((scenes[..., :6], scenes[..., 6:] * log_e.exp()), dim=-1)
            photos, weights = registration.refine(x, scenes)
            unseen = weights.amax(dim=1, keepdim=True) == 0
            print("step %4d  registration stage: mean corner error %.3f px" % (step, registration.error()))
        if fit is not None and opt is None:
            loss = fit.step(photos, table, weights)
        elif fit is not None:
            opt.zero_grad(set_to_none=True)
            scenes = table if pos is None else torch.cat((pos, colour), dim=-1)
            loss = fit.step(photos, scenes, weights, exposure=None if log_e is None else log_e.exp())
            loss.backward()
            opt.step()
        else:
            opt.zero_grad(set_to_none=True)
            scenes = table if pos is None else torch.cat((pos, colour), dim=-1)
            loss = fn(x, photos, scenes, weights) if log_e is None else fn(x, photos, scenes, weights, log_e.exp())
            (loss if lam is None else loss + fitting.smoothness(x, lam)).backward()
            opt.step()
            with torch.no_grad():
                x[:, 3:].clamp_(0.0, 1.0)
        if step % args.print_every == 0 or step == args.steps - 1:
            err = map_error(x, truth, unseen)[1]
            gains = "" if log_e is None else "  mean |log e - log e*| %.5f" % (log_e.detach() - hidden.log()).abs().mean().item()
            if pos is not None:
                gains += "  mean |position - truth| %.5f" % (pos.detach() - true_pos).abs().mean().item()
            print("step %4d  loss %.6f  %s%s%s" % (
                step, loss.item(), err, gains, "  %.3f ms/step" % step_ms[-1] if step_ms else ""))
    if step_ms:
        print("median %.3f ms per step (loss + backward + Adam + clamp, host included)" % float(np.median(step_ms)))
    return map_error(x, truth, unseen)[0]


def run_in_launches(args, fit, photos, table, x, truth, weights=None, unseen=None):
    """--steps-per-launch: the fit in launches of K steps, the losses read from the tensors the launches return"""
    K, launch_ms = args.steps_per_launch, []
    print("%d steps per launch" % K)
    for first in range(0, args.steps, K):
        n = min(K, args.steps - first)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses_dev = fit.steps(n, photos, table, weights)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / n
        if first:                               # (the first launch loads the code object)
            launch_ms.append(ms)
        seen = losses_dev.cpu().tolist()
        for k, loss in enumerate(seen):
            step = first + k
            if step % args.print_every == 0 or step == args.steps - 1:
                err = ""
                if k == n - 1:
                    err = "  %s behind it" % map_error(x, truth, unseen)[1]
                print("step %4d  loss %.6f%s  %.3f ms/step" % (step, loss, err, ms))
    if launch_ms:
        print("median %.3f ms per step (%d steps per launch, host included)" % (float(np.median(launch_ms)), K))
    return map_error(x, truth, unseen)[0]


if __name__ == "__main__":
    main()
