"""Fit SVBRDF maps to photographs with the fused photo loss (losses.PhotoLoss): the inverse-rendering use of the engine.

    python tools/fit_photos.py [--size 256] [--batch 2] [--photos 9] [--steps 200] [--lr 0.01] [--noise] [--seed 1]
                               [--fit-exposure] [--fit-pose [--pose-lr 0.002]] [--fused-step [--steps-per-launch K]]
                               [--captured [--sensor 640x480] [--clip 250] [--fit-registration [--corner-noise PX]
                                [--fused-registration]]
                                [--lens K1[,K2] [--fit-lens [--lens-lr 0.01]]]]
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

``--fused-registration`` (with ``--fit-registration``): a third fit whose registration stage takes the FUSED loss instead of
the composition above: ``PhotoLoss(renderer, eps=Registration.EPS, normalize="weights", differentiable_photos=True)(
maps.detach(), rect, scenes, w)`` -- loss and d loss / d rect from ONE launch of the forward-only photo-gradient kernel
(the maps are constants of the stage: no K1, no torch ops of the definition), handed to ``capture.rectify``'s backward by
autograd.  It is the loss the maps are fitted with; unlike the composition it has NO clamp of the rendering at 1.  Its
corner error and map error are printed beside the composed stage's; nothing about the alternation's convergence is
asserted.  Without the flag the tool's output is unchanged.

``--lens K1[,K2]`` (only with ``--captured``): the camera has a lens.  ``ingest`` bends every camera image with the lens
``capture.pinhole_lens(sensor)`` + (k1, k2) on the host before quantisation -- a float64 ``capture.undistort_points`` grid per
sensor pixel feeds a ``grid_sample`` of the pinhole image; a demo's synthesis, no hot path -- and the corner positions it
hands on are ``capture.distort_points`` of the true ones: what somebody would click.  Two more fits: one rectified IGNORING
the lens (the clicked corners into ``patch_homography``, no ``lens=``), one with the true lens (``undistort_points`` of the
clicked corners, ``capture.rectify(..., lens=)``).  The map error is reported three ways: ignoring the lens, with the true
lens, and with the pinhole image as before.

A negative K1 may be written ``--lens -0.18,0.04`` or ``--lens=-0.18,0.04``.  A camera at a grazing angle sees a patch
corner thousands of pixels outside its sensor; the polynomial throws such a point further than Newton comes back from (it
describes the lens inside the frame only) and nobody clicks there: those corners keep the ideal position this synthesis
knows, and how many did is printed beside the figure they enter.
With ``--fit-registration`` the registration fits then run on the bent images with the lens known: the corners given off
are the ideal ones, and every stage's rectification and its gradient go through ``lens=``.

``--fit-lens`` (with ``--lens`` and ``--fit-registration``): the lens's k1 is NOT known.  The registration fits hold the
CLICKED corners -- distorted coordinates, given off by ``--corner-noise`` -- as their parameter; the ideal corners that
``corner_matrices`` needs are ``undistort_points`` of them under the current lens, recomputed at every step, with the
gradient carried through the implicit inverse (one Newton step in torch ops around the host's solution: d ideal / d clicked
is the inverse of the polynomial's 2x2 Jacobian, d ideal / d k1 that inverse times -d distorted / d k1).  k1 starts at 0
and is refined in the registration stage alongside the corners: ONE coefficient shared by all photographs of the camera,
in its own Adam group (``--lens-lr``); k2 stays as given (k1 and k2 trade off against each other on a patch that covers the
middle of the frame: one coefficient per stage).  The fit "as given" keeps k1 = 0.  k1 is printed at every stage and the
three map errors at the end.  Nothing about the alternation's convergence is asserted: the tool records what it does.

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
    ap.add_argument("--fused-registration", action="store_true",
                    help="with --fit-registration: one more fit whose registration stage takes the fused photo loss and its "
                         "gradient towards the photographs (no clamp of the rendering at 1)")
    ap.add_argument("--corner-noise", type=float, default=2.0, metavar="PX", help="with --fit-registration: source pixels per coordinate")
    ap.add_argument("--registration-every", type=int, default=20, help="map steps between two registration stages")
    ap.add_argument("--registration-steps", type=int, default=5, help="Adam steps on the corners per stage")
    ap.add_argument("--registration-lr", type=float, default=0.1, help="Adam learning rate of the corners, source pixels")
    ap.add_argument("--lens", default=None, metavar="K1[,K2]",
                    help="with --captured: the camera's radial distortion coefficients (a negative K1: --lens -0.18,0.04 or --lens=-0.18,0.04)")
    ap.add_argument("--fit-lens", action="store_true", help="with --lens and --fit-registration: k1 from 0, refined beside the corners")
    ap.add_argument("--lens-lr", type=float, default=0.01, help="with --fit-lens: Adam learning rate of k1")
    ap.add_argument("--smooth", type=float, default=None, metavar="LAMBDA",
                    help="smoothness prior across pixels on diffuse, roughness and specular (normals stay at 0); with "
                         "--steps-per-launch K it is K launches, not one")
    argv = sys.argv[1:]
    for n in range(len(argv) - 1):          # argparse takes "-0.18,0.04" for an option: hand it over as --lens=-0.18,0.04
        if argv[n] == "--lens" and argv[n + 1][:1] == "-" and argv[n + 1][1:2].isdigit():
            argv[n:n + 2] = ["--lens=" + argv[n + 1]]
            break
    args = ap.parse_args(argv)
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
    if args.fused_registration and not args.fit_registration:
        ap.error("--fused-registration is a form of the registration stage: it needs --fit-registration")
    if args.lens is not None and not args.captured:
        ap.error("--lens bends the camera images of --captured")
    if args.fit_lens and (args.lens is None or not args.fit_registration):
        ap.error("--fit-lens refines k1 in the registration stage: it needs --lens and --fit-registration")
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
        scaled = losses.fold_exposure(table, hidden)
        photos = _native.render_fwd(truth, scaled).clamp_(0.0, 1.0)
    if not args.captured:
        return fit(args, dev, truth, photos, table, hidden)
    on_grid = fit(args, dev, truth, photos, table, hidden)
    rectified, weights, cameras, images, corners, ideal, _ = ingest(args, dev, photos, table)
    seen = weights.unsqueeze(2).expand_as(photos) > 0
    print("--- the same fit on the captured photographs: %s sensor, gamma 2.2, 8 bits, rectified with 2 x 2 sub-samples; "
          "%.2f %% of the weights are zero, %.2f %% of the pixels are seen by no photograph; mean |rectified - on the grid| %.5f "
          "where the weight is 1" % (args.sensor, 100.0 * (weights == 0).float().mean().item(),
                                     100.0 * (weights.amax(dim=1) == 0).float().mean().item(),
                                     (rectified - photos)[seen].abs().mean().item()))
    captured = fit(args, dev, truth, rectified, table, hidden, weights, cameras)
    print("final mean |d,r,s - truth|: on the grid %.5f, captured %.5f (zero weights: %.2f %%)" % (
        on_grid, captured, 100.0 * (weights == 0).float().mean().item()))
    lens, beyond = None, None
    if args.lens is not None:
        sensor = tuple(int(v) for v in args.sensor.lower().split("x"))
        coeff = [float(v) for v in args.lens.split(",")] + [0.0]
        lens = capture.pinhole_lens(sensor).double().numpy()
        lens[4], lens[5] = coeff[0], coeff[1]
        errors = []
        for use in (False, True):
            bent, w, _, images, corners, _, beyond = ingest(args, dev, photos, table, lens, use)
            how = "IGNORING the lens"
            if use:
                how = "with the true lens (%d of %d clicked corners lie beyond Newton's reach and keep their known ideal position)" % (
                    int(beyond.sum()), beyond.size)
            print("--- the captured fit through a lens k1 = %g, k2 = %g, rectified %s; %.2f %% of the weights are zero; mean "
                  "|rectified - on the grid| %.5f where the weight is 1" % (
                      lens[4], lens[5], how, 100.0 * (w == 0).float().mean().item(),
                      (bent - photos)[w.unsqueeze(2).expand_as(photos) > 0].abs().mean().item()))
            errors.append(fit(args, dev, truth, bent, table, hidden, w, cameras))
        print("final mean |d,r,s - truth|: ignoring the lens %.5f, with the true lens %.5f, the pinhole image %.5f" % (
            errors[0], errors[1], captured))
        captured = errors[1]
    if not args.fit_registration:
        return
    if lens is not None and not args.fit_lens:
        corners = ideal                                        # the registration fits know the lens: ideal corners
    noise = args.corner_noise * (2.0 * synth.uniform01(args.seed + 4000, corners.shape) - 1.0)
    results = []
    for refine in (False, True):
        reg = Registration(args, images, corners, corners + noise, H, lens, (ideal, beyond) if args.fit_lens else None)
        print("--- the captured fit with every corner coordinate given up to %g source pixels off (mean corner error %.3f px), %s"
              % (args.corner_noise, reg.error(), "refined every %d map steps (%d Adam steps, lr %g)" % (
                  args.registration_every, args.registration_steps, args.registration_lr) if refine else "left as given"))
        shifted, w = reg.rectify()
        results.append((fit(args, dev, truth, shifted, table, hidden, w, cameras, reg if refine else None), reg.error()))
    print("final mean |d,r,s - truth|: true corners %.5f; corners %g px off, as given %.5f (corner error %.3f px), refined %.5f "
          "(corner error %.3f px)%s" % (captured, args.corner_noise, results[0][0], results[0][1], results[1][0], results[1][1],
                                        reg.lens_text()))
    if args.fused_registration:
        reg = Registration(args, images, corners, corners + noise, H, lens, (ideal, beyond) if args.fit_lens else None, fused=True)
        print("--- the same refined fit with the registration stage on the FUSED photo loss (one launch: loss and its gradient "
              "towards the rectified photographs; eps %g, weighted mean, no clamp of the rendering at 1)" % Registration.EPS)
        shifted, w = reg.rectify()
        error = fit(args, dev, truth, shifted, table, hidden, w, cameras, reg)
        print("final mean |d,r,s - truth|: refined with the composed stage %.5f (corner error %.3f px), with the fused stage %.5f "
              "(corner error %.3f px)%s" % (results[1][0], results[1][1], error, reg.error(), reg.lens_text()))


class Registration:
    """--fit-registration: the corners of every captured photograph as an Adam parameter, float64 [B,S,4,2] on the host"""

    EPS = 0.01

    def __init__(self, args, images, true_corners, start_corners, H, lens=None, unknown=None, fused=False):
        """`lens`: float64 [9] of the camera, or None.  `unknown` None: the lens is known and the corners are ideal
        coordinates.  `unknown` = (ideal, beyond), --fit-lens: the corners are the CLICKED, distorted ones, k1 starts at 0 as a
        parameter of its own Adam group, and the ideal corners follow from both at every step (`ideal_of`); `ideal` [B,S,4,2]
        are the true corners' ideal positions, which the corners marked in `beyond` (no Newton from where the polynomial
        throws them) keep, moved by what their parameter has moved.  `fused`: --fused-registration, the stage's loss is the
        fused photo loss with its gradient towards the photographs."""
        self.args, self.images, self.H = args, images, H
        self.fused_loss = None
        if fused:
            self.fused_loss = losses.PhotoLoss(renderers.LocalRenderer(), eps=self.EPS, normalize="weights",
                                               differentiable_photos=True)
        self.lens = None if lens is None else torch.from_numpy(np.array(lens, np.float64))
        self.true = torch.from_numpy(true_corners)
        self.corners = torch.from_numpy(start_corners).clone().requires_grad_(True)
        groups = [{"params": [self.corners]}]
        self.k1 = None
        if unknown is not None:
            self.true_k1 = float(lens[4])
            self.lens[4] = 0.0
            self.k1 = torch.zeros((), dtype=torch.float64, requires_grad=True)
            self.known, self.beyond = torch.from_numpy(unknown[0]), torch.from_numpy(unknown[1])
            groups.append({"params": [self.k1], "lr": args.lens_lr})
        self.opt = torch.optim.Adam(groups, lr=args.registration_lr)
        self.lut = capture.gamma_lut()

    def error(self):
        return (self.corners.detach() - self.true).norm(dim=-1).mean().item()

    def lens_text(self):
        return "" if self.k1 is None else "; k1 %.5f (truth %g)" % (self.k1.item(), self.true_k1)

    def ideal_of(self, lens):
        """--fit-lens: the ideal corners of the clicked ones under `lens` (a tensor [9] that may require grad), differentiable
        towards both.  The host solves x0 = undistort_points(clicked, lens); one Newton step around it in torch ops,
        x0 - J^-1 (distort(x0, lens) - clicked) with J the polynomial's Jacobian at x0 as a constant, has x0's value and the
        implicit inverse's gradients."""
        moved = self.corners - self.true                            # what the parameter has moved, with its gradient
        kept = self.known + moved
        x0, failed = ideal_corners(self.corners.detach().numpy(), lens.detach().numpy(), kept.detach().numpy())
        failed = torch.from_numpy(failed) | self.beyond
        l = lens.detach().numpy()
        xn, yn = (x0[..., 0] - l[2]) / l[0], (x0[..., 1] - l[3]) / l[1]
        _, _, _, jxx, jxy, jyy = capture._distort_normalised(xn, yn, l)
        a, b, c, d = jxx, jxy * l[0] / l[1], jxy * l[1] / l[0], jyy  # d (ud, vd) / d (u, v) in pixels
        det = a * d - b * c
        inv = torch.from_numpy(np.stack((np.stack((d, -b), -1), np.stack((-c, a), -1)), -2) / det[..., None, None])
        r = distort_torch(torch.from_numpy(x0), lens) - self.corners
        step = (inv * r[..., None, :]).sum(dim=-1)
        return torch.where(failed[..., None], kept, torch.from_numpy(x0) - step)

    def rectify(self, grad=False):
        lens, corners = self.lens, self.corners
        if self.k1 is not None:
            pick = torch.zeros(9, dtype=torch.float64)
            pick[4] = 1.0
            lens = lens + pick * self.k1
            corners = self.ideal_of(lens)
        M = capture.corner_matrices(corners, self.H)
        if not grad:
            M, lens = M.detach(), None if lens is None else lens.detach()
        return capture.rectify(self.images, M, self.H, lut=self.lut, clip=(0, self.args.clip), samples=2, lens=lens)

    def refine(self, maps, scenes):
        """one stage: a few Adam steps on the corners against the rendering of `maps` under `scenes` -> (photos, weights)"""
        if self.fused_loss is not None:
            # ONE launch per step for the loss and d loss / d rect (the forward-only photo-gradient kernel: the maps are
            # constants here); no clamp of the rendering at 1
            maps, scenes = maps.detach().contiguous(), scenes.detach().contiguous()
            for _ in range(self.args.registration_steps):
                self.opt.zero_grad(set_to_none=True)
                rect, w = self.rectify(grad=True)
                self.fused_loss(maps, rect, scenes, w).backward()
                self.opt.step()
            return self.rectify()
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


def ideal_corners(clicked, lens, fallback):
    """capture.undistort_points per corner -> (ideal [...,2], failed [...] bool).  A camera at a grazing angle sees a patch
    corner thousands of pixels outside its sensor; the polynomial throws such a point further than Newton comes back from (it
    describes the lens inside the frame only), and nobody clicks there: those corners take `fallback`'s position."""
    clicked, fallback = np.asarray(clicked, np.float64), np.asarray(fallback, np.float64)
    out = fallback.copy().reshape(-1, 2)
    failed = np.zeros(len(out), bool)
    for n, point in enumerate(clicked.reshape(-1, 2)):
        try:
            out[n] = capture.undistort_points(point, lens)
        except ValueError:
            failed[n] = True
    return out.reshape(clicked.shape), failed.reshape(clicked.shape[:-1])


def distort_torch(points, lens):
    """capture.distort_points in torch ops, differentiable towards `points` [...,2] and `lens` [9]"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = lens.unbind()
    xn, yn = (points[..., 0] - cx) / fx, (points[..., 1] - cy) / fy
    xx, yy, xy = xn * xn, yn * yn, xn * yn
    r2 = xx + yy
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = xn * rad + (p1 * 2.0 * xy + p2 * (r2 + 2.0 * xx))
    yd = yn * rad + (p1 * (r2 + 2.0 * yy) + p2 * 2.0 * xy)
    return torch.stack((xd * fx + cx, yd * fy + cy), dim=-1)


def bend(seen, lens):
    """--lens: the pinhole images [B,S,3,h,w] as the lens delivers them.  Every sensor pixel is a DISTORTED position; its ideal
    position (capture.undistort_points, float64 on the host) is where the pinhole image is read, bilinearly, zeros outside."""
    h, w = seen.shape[-2:]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ideal = capture.undistort_points(np.stack((xx, yy), axis=-1), lens)
    grid = torch.from_numpy(np.stack((2.0 * ideal[..., 0] / (w - 1) - 1.0, 2.0 * ideal[..., 1] / (h - 1) - 1.0), axis=-1)).float()
    flat = seen.reshape((-1,) + tuple(seen.shape[-3:]))
    out = torch.nn.functional.grid_sample(flat, grid.to(seen.device)[None].expand(flat.shape[0], h, w, 2), mode="bilinear",
                                          padding_mode="zeros", align_corners=True)
    return out.reshape(seen.shape)


def ingest(args, dev, photos, table, lens=None, use_lens=True):
    """--captured: the photographs as a camera at each photo's position delivers them -- perspective, gamma 2.2, 8 bits --
    and back onto the grid -> (photos [B,S,3,H,W], weights [B,S,H,W], the camera positions recovered from the corners, the
    8-bit images [B,S,h,w,3], the corners [B,S,4,2] in their pixels as handed on, their ideal positions, and which of them
    lie beyond Newton's reach [B,S,4]).  `lens` (float64 [9]): the images are bent with it before
    quantisation and the corners handed on are where the lens puts them; the rectification then either ignores the lens
    (those corners into patch_homography) or, `use_lens`, undoes it (their ideal positions, and lens= in the one launch)."""
    sensor = tuple(int(v) for v in args.sensor.lower().split("x"))
    B, S, H = photos.shape[0], photos.shape[1], photos.shape[-1]
    cams = table[..., :3].cpu().numpy().astype(np.float64)
    seen = capture.to_perspective(photos, cams, sensor)                                  # [B,S,3,sensor h,sensor w]
    if lens is not None:
        seen = bend(seen, lens)
    codes = (seen.clamp(0.0, 1.0).cpu().double().pow(1.0 / 2.2) * 255.0).round().to(torch.uint8)
    images = codes.permute(0, 1, 3, 4, 2).contiguous().to(dev)                           # what an image decoder returns: HWC
    corners = [capture.camera_corners(c, sensor) for c in cams.reshape(-1, 3)]
    recovered = np.stack([capture.camera_from_corners(c, sensor) for c in corners]).reshape(B, S, 3)
    shown = corners if lens is None else [capture.distort_points(c, lens) for c in corners]
    beyond = np.zeros((len(corners), 4), bool)
    used = shown
    if lens is not None:
        solved = [ideal_corners(d, lens, c) for d, c in zip(shown, corners)]
        beyond = np.stack([f for _, f in solved])
        used = [c for c, _ in solved] if use_lens else shown
    matrices = np.stack([capture.patch_homography(c, (H, H)) for c in used]).reshape(B, S, 3, 3)
    rectified, weights = capture.rectify(images, matrices, H, lut=capture.gamma_lut(), clip=(0, args.clip), samples=2,
                                         lens=lens if use_lens else None)
    return (rectified, weights, torch.from_numpy(recovered).float().to(dev), images, np.stack(shown).reshape(B, S, 4, 2),
            np.stack(corners).reshape(B, S, 4, 2), beyond.reshape(B, S, 4))


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
                    scenes = losses.fold_exposure(scenes, log_e.exp())
            photos, weights = registration.refine(x, scenes)
            unseen = weights.amax(dim=1, keepdim=True) == 0
            print("step %4d  registration stage: mean corner error %.3f px%s" % (step, registration.error(), registration.lens_text()))
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
