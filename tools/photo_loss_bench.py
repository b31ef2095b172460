"""The fused photo loss against K3 and against the composed form, one process, one box (profiles/r09_photo_loss.txt).

    python tools/photo_loss_bench.py [--out FILE] [--variants TAG=LIB ...] [--head] [--weights {none,shared,per-photo}] [--pose] [--exposure] [--fit]

At the configuration-2 shape (B = 8, 256 x 256, S = 9, scene table by value, six batches rotating beyond the 256 MB
Infinity Cache, as bench.py does) it prints the event-timed median per launch of
  * the photo loss (svbrdf_photo_loss_fwd_bwd_host_scenes),
  * K3, the rendering loss on the same maps (svbrdf_mixed_loss_fwd_bwd_host_scenes, l1_weight 0),
  * the composed form: K1, log / L1 mean by torch, the backward of those ops, K2 (what PhotoLoss takes for float64 maps,
    here on float32 maps),
the fraction of 8 TB/s at the algorithmic bytes (12 + 3 S + 12) * 4 * H * W * B, and the VALU instructions per
pixel-render of the scene loops from tools/isa_stats.py (where hipcc is present).  The method is that of
tests/test_gpu_photo_loss.py::test_photo_loss_is_no_slower_than_k3 (tests/photo_checks.py::measure_photo_loss_against_k3, the
tests' helper module, which this tool imports): launches enqueued behind a spinning wave so that the stream runs them back
to back, an event between every two, medians of interleaved rounds.

--head: the head leg instead -- the head-fused photo loss (svbrdf_head_photo_loss_fwd_bwd_host_scenes: the generator's
[B,9,H,W] output in, its gradient out), the 12-channel photo kernel on the decoded maps and the unfused composition
PhotoLoss(decode_head(x)) forward + backward through autograd, same shape, one process
(tests/head_photo_checks.py::measure_head_photo_loss, the method of tests/test_gpu_head_photo_loss.py's speed test).

--weights shared | per-photo: the weighted leg instead -- the photo loss with per-pixel confidence weights
(svbrdf_photo_loss_weighted_fwd_bwd_host_scenes; one [B,1,H,W] plane per item or one [B,S,H,W] plane per photo), the
unweighted kernel on the same maps and photos and the unfused weighted composition (K1, the torch ops of the definition and
their backward, K2), same shape, one process (tests/weighted_photo_checks.py::measure_weighted_photo_loss, the method of
tests/test_gpu_weighted_photo_loss.py's speed test).  `none` (default) is the unweighted report.

--pose: the scene-gradient leg instead -- the photo loss with the gradient towards the scene table
(svbrdf_photo_loss_scene_grad_fwd_bwd, per-photo weights, device table), the weighted kernel on the same table and the
composed torch-op definition with the table as a leaf, forward + backward (tests/pose_photo_checks.py::
measure_pose_photo_loss, the method of tests/test_gpu_pose_photo_loss.py's speed test).

--exposure: the exposure leg instead -- the photo loss with a per-photo exposure and its gradient
(svbrdf_photo_loss_exposure_fwd_bwd, per-photo weights, device table), the weighted kernel on the pre-scaled table and the
composed definition with an exposure leaf (tests/exposure_photo_checks.py::measure_exposure_photo_loss, the method of
tests/test_gpu_exposure_photo_loss.py's speed test).

--fit: the fit-step leg instead -- the fused step (svbrdf_photo_fit_adam_step through fitting.PhotoFit: loss, gradient, Adam
update and clamp of the maps in ONE launch, per-photo weights, device table), the weighted loss kernel's launch on the same
data, and the composed step -- PhotoLoss forward + backward, torch.optim.Adam.step(), clamp_ -- with the stock default and
with fused=True (tests/photo_fit_checks.py::measure_photo_fit, the method of tests/test_gpu_photo_fit.py's speed test).

--variants: other builds of the library (tools/build_variant.sh, e.g. the photo-loss unit compiled with another of the
Makefile's scheduler sets), each measured in a child process of its own on this box, interleaved with the shipped build.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def isa_lines():
    hipcc, csrc = "/opt/rocm/bin/hipcc", os.path.join(ROOT, "svbrdf_estimation_amd", "csrc")
    if not os.path.exists(hipcc):
        return ["VALU per pixel-render: not counted here (no hipcc on this box); tests/test_photo_loss_cpu.py holds the budget"]
    import tempfile
    import isa_stats
    var = lambda n: subprocess.check_output(["make", "-s", "-C", csrc, "print-" + n], text=True).split()
    out = os.path.join(tempfile.mkdtemp(prefix="photo_isa_"), "photo.s")
    cmd = var("HIPCC") + var("HIPFLAGS") + var("SCHED_PHOTO") + ["-S", "--cuda-device-only", "-o", out, "svbrdf_photo_loss.hip"]
    subprocess.check_call(cmd, cwd=csrc, stderr=subprocess.DEVNULL)
    text, lines = open(out).read(), []
    for k in sorted(isa_stats.kernels(text)):
        if "k_photo_loss" not in k and "k_head_photo" not in k and "wphoto" not in k:
            continue
        _, meta, _, loops, _, _ = isa_stats.analyse(text, k)
        per = 2 if "ILb1E" in k else 1
        for c in sorted((c for c in loops if c["trans"]), key=lambda c: c["valu"]):
            lines.append("%-33s %s loop: %5.1f VALU, %4.1f transcendentals per pixel-render; %s VGPRs, scratch %s" % (
                ("weighted " if "wphoto" in k else "") + ("head " if "k_head_" in k else "") + ("by-value" if "_inl" in k else "device")
                + (" fwd+bwd" if per == 2 else " fwd only"),
                "tied  " if c["trans"] / per < 14 else "untied", c["valu"] / per, c["trans"] / per, meta.get("NumVgprs"),
                meta.get("ScratchSize")))
    return lines


def measure_composed(dev, native, sets=6, n=30, rounds=3):
    import torch
    from bench import synthetic_maps
    from svbrdf_estimation_amd import environment, losses
    import photo_checks
    B, H = 8, 256
    gen = torch.Generator().manual_seed(5)
    torch.manual_seed(11)
    table = environment.BatchSceneSampler(B, 3, 6).sample().contiguous()
    ins = [synthetic_maps(gen, B, H, tied=True).to(dev).requires_grad_(True) for _ in range(sets)]
    photos = [native.render_fwd(synthetic_maps(gen, B, H, tied=True).to(dev), table).clamp_(0.0, 1.0) for _ in range(sets)]

    def step(i):
        k = i % sets
        ins[k].grad = None
        losses.composed_photo_loss(ins[k], photos[k], table, 0.1).backward()

    medians, _ = photo_checks.timed_legs((("composed_us", step),), n, rounds, photo_checks.spinning_wave(native, dev), dev)
    return medians["composed_us"]


def child(head=False, weights="none", pose=False, exposure=False, fit=False):
    import torch
    from svbrdf_estimation_amd import _native
    import photo_checks
    dev = torch.device("cuda:0")
    if fit:
        import photo_fit_checks
        res = photo_fit_checks.measure_photo_fit(dev, _native)
    elif pose:
        import pose_photo_checks
        res = pose_photo_checks.measure_pose_photo_loss(dev, _native)
    elif exposure:
        import exposure_photo_checks
        res = exposure_photo_checks.measure_exposure_photo_loss(dev, _native)
    elif weights != "none":
        import weighted_photo_checks
        res = weighted_photo_checks.measure_weighted_photo_loss(dev, _native, weights)
    elif head:
        import head_photo_checks
        res = head_photo_checks.measure_head_photo_loss(dev, _native)
    else:
        res = photo_checks.measure_photo_loss_against_k3(dev, _native)
        res["composed_us"] = measure_composed(dev, _native)
    res["library"] = _native.library_path()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--variants", nargs="*", default=[], metavar="TAG=LIB")
    ap.add_argument("--passes", type=int, default=1, help="how often the builds are measured in turn")
    ap.add_argument("--head", action="store_true", help="the head leg: fused head photo loss, 12-channel kernel, unfused composition")
    ap.add_argument("--weights", choices=("none", "shared", "per-photo"), default="none",
                    help="the weighted leg: weighted photo loss, unweighted kernel, unfused weighted composition")
    ap.add_argument("--pose", action="store_true",
                    help="the scene-gradient leg: photo loss with grad_scenes, weighted kernel, composed torch-op definition")
    ap.add_argument("--exposure", action="store_true",
                    help="the exposure leg: photo loss with grad_exposure, weighted kernel, composed definition with an exposure leaf")
    ap.add_argument("--fit", action="store_true",
                    help="the fit-step leg: fused loss + Adam step, weighted kernel, PhotoLoss + torch.optim.Adam + clamp_")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.head + (args.weights != "none") + args.pose + args.exposure + args.fit > 1:
        ap.error("--head, --weights, --pose, --exposure and --fit measure different legs: give one of them")
    if args.child:
        return child(args.head, args.weights, args.pose, args.exposure, args.fit)
    builds = [("shipped", None)] + [tuple(v.split("=", 1)) for v in args.variants]
    rows = []
    for p in range(args.passes):
        for tag, lib in builds:
            env = dict(os.environ)
            if lib:
                env["SVBRDF_HIP_LIB"] = os.path.abspath(lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--weights", args.weights]
                                 + (["--head"] if args.head else []) + (["--pose"] if args.pose else [])
                                 + (["--exposure"] if args.exposure else []) + (["--fit"] if args.fit else []), env=env, text=True, timeout=300,
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not line:
                print(out.stdout[-2000:])
                raise SystemExit("measurement of build %r failed (exit status %s): nothing more is started" % (tag, out.returncode))
            rows.append((tag, p, json.loads(line[0][7:])))
    B, H, S = 8, 256, 9
    if args.fit:
        lines = ["# tools/photo_loss_bench.py --fit on %s; B = %d, %d x %d, S = %d, per-photo weights, device table, %d rotating batches" % (
            rows[0][2]["device"], B, H, H, S, rows[0][2]["sets"]),
            "# medians of event-timed steps (us per step); algorithmic bytes of the fused step (72 + 3 S + P) * 4 * H * W * B = %.1f MB, "
            "of the weighted loss (24 + 3 S + P): byte ratio %.3f" % ((72 + 3 * S + S) * 4 * H * H * B / 1e6, rows[0][2]["byte_ratio"])]
        for tag, p, r in rows:
            lines.append("%-16s pass %d: fused step %7.2f  weighted loss launch %7.2f (ratio %.3f)  composed step PhotoLoss fwd + bwd, "
                         "Adam, clamp_: stock %8.2f, fused=True %8.2f  fused step / faster composed %.3f   fused step = %.3f of 8 TB/s"
                         "   rounds %s" % (tag, p, r["fit_us"], r["weighted_us"], r["fit_over_weighted"], r["composed_us"],
                                           r["composed_fused_us"], r["fit_over_composed"], r["fit_frac_of_8TBps"], r["rounds"]))
    elif args.pose or args.exposure:
        key, what, leaf = ("pose_us", "grad_scenes", "a table") if args.pose else ("exposure_us", "grad_exposure", "an exposure")
        lines = ["# tools/photo_loss_bench.py --%s on %s; B = %d, %d x %d, S = %d, per-photo weights, device table, %d rotating batches" % (
            "pose" if args.pose else "exposure", rows[0][2]["device"], B, H, H, S, rows[0][2]["sets"]),
            "# medians of event-timed steps (us per step)"]
        for tag, p, r in rows:
            lines.append("%-16s pass %d: photo loss with %s %7.2f  weighted photo loss on the same table %7.2f (ratio %.3f)  "
                         "composed torch-op definition with %s leaf fwd + bwd %8.2f (%.1fx)   rounds %s" % (
                             tag, p, what, r[key], r["weighted_us"], r[key] / r["weighted_us"], leaf, r["composition_us"],
                             r["composition_us"] / r[key], r["rounds"]))
    elif args.weights != "none":
        P = rows[0][2]["planes"]
        lines = ["# tools/photo_loss_bench.py --weights %s on %s; B = %d, %d x %d, S = %d, scene table by value, %d rotating batches" % (
            args.weights, rows[0][2]["device"], B, H, H, S, rows[0][2]["sets"]),
            "# medians of event-timed steps (us per step); algorithmic bytes of the weighted photo loss (12 + 3 S + P + 12) * 4 * H * W * B "
            "= %.1f MB with P = %d weight planes per item" % ((12 + 3 * S + P + 12) * 4 * H * H * B / 1e6, P)]
        for tag, p, r in rows:
            lines.append("%-16s pass %d: weighted photo loss %7.2f  unweighted %7.2f (ratio %.3f; byte ratio %.3f)  unfused weighted "
                         "composition fwd + bwd %8.2f   weighted = %.3f of 8 TB/s, %.1fx the composition   rounds %s" % (
                             tag, p, r["weighted_us"], r["unweighted_us"], r["weighted_us"] / r["unweighted_us"],
                             (12 + 3 * S + P + 12) / (12 + 3 * S + 12.0), r["composition_us"], r["weighted_frac_of_8TBps"],
                             r["composition_us"] / r["weighted_us"], r["rounds"]))
    elif args.head:
        lines = ["# tools/photo_loss_bench.py --head on %s; B = %d, %d x %d, S = %d, scene table by value, %d rotating batches" % (
            rows[0][2]["device"], B, H, H, S, rows[0][2]["sets"]),
            "# medians of event-timed steps (us per step); algorithmic bytes of the head photo loss (9 + 3 S + 9) * 4 * H * W * B = %.1f MB"
            % ((9 + 3 * S + 9) * 4 * H * H * B / 1e6)]
        for tag, p, r in rows:
            lines.append("%-16s pass %d: head photo loss %7.2f  12-channel photo loss %7.2f  unfused PhotoLoss(decode_head(x)) fwd + bwd "
                         "%8.2f   head photo loss = %.3f of 8 TB/s, %.1fx the composition   rounds %s" % (
                             tag, p, r["head_photo_us"], r["photo12_us"], r["composition_us"], r["head_photo_frac_of_8TBps"],
                             r["composition_us"] / r["head_photo_us"], r["rounds"]))
    else:
        lines = ["# tools/photo_loss_bench.py on %s; B = %d, %d x %d, S = %d, scene table by value, %d rotating batches" % (
            rows[0][2]["device"], B, H, H, S, rows[0][2]["sets"]),
            "# medians of event-timed launches (us per launch); algorithmic bytes of the photo loss (12 + 3 S + 12) * 4 * H * W * B = %.1f MB"
            % ((12 + 3 * S + 12) * 4 * H * H * B / 1e6)]
        for tag, p, r in rows:
            lines.append("%-16s pass %d: photo loss %7.2f  K3 %7.2f  composed K1 + torch + K2 %8.2f   photo loss = %.3f of 8 TB/s, "
                         "%.2fx K3, %.1fx composed   rounds %s" % (tag, p, r["photo_loss_us"], r["k3_us"], r["composed_us"],
                                                                 r["photo_loss_frac_of_8TBps"], r["k3_us"] / r["photo_loss_us"],
                                                                 r["composed_us"] / r["photo_loss_us"], r["rounds"]))
    lines += ["# scene loops of the shipped source (hipcc -S with the Makefile's flags, tools/isa_stats.py); K3's tied loop: 301 VALU per pixel-render"]
    lines += isa_lines()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
