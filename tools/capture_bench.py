#!/usr/bin/env python3
"""Time capture.rectify (svbrdf_rectify_photos: one launch) against the same work composed from torch ops.

    python tools/capture_bench.py [--out profiles/r21_capture.txt] [--rounds 3] [--steps 12]

Shapes: the configuration-2-like batch B = 8, S = 9 (P = 72 photographs) of 1200 x 1600 onto 256 x 256 --
uint8 sources at k = 1 (with the composition: to float, table gather, permute, grid_sample, validity and clip masks, where),
the same at k = 2 (2 x 2 sub-samples; the composition has no counterpart), and float32 planar sources at k = 1 -- and the
speed test's P = 8 of 480 x 640.  One process, the legs alternating round by round behind a spinning wave, medians of the
event-timed launches (tests/capture_checks.measure_capture, the method of tools/photo_loss_bench.py).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import capture_checks as cc  # noqa: E402
from svbrdf_estimation_amd import _native  # noqa: E402

CASES = (
    ("P=72 (B=8,S=9) uint8 1200x1600 -> 256x256, k=1, lut + clip", dict(P=72, src_size=(1200, 1600), k=1, u8=True, sets=2)),
    ("P=72 (B=8,S=9) uint8 1200x1600 -> 256x256, k=2, lut + clip", dict(P=72, src_size=(1200, 1600), k=2, u8=True, sets=2)),
    ("P=72 (B=8,S=9) float32 1200x1600 -> 256x256, k=1, clip", dict(P=72, src_size=(1200, 1600), k=1, u8=False, sets=2)),
    ("P=8 uint8 480x640 -> 256x256, k=1, lut + clip (the speed test's shape)", dict(P=8, src_size=(480, 640), k=1, u8=True, sets=4)),
)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=12, help="timed calls per leg and round")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    lines = ["# tools/capture_bench.py on %s: us per call, median of %d rounds x %d event-timed calls, legs alternating" % (
        torch.cuda.get_device_name(dev), args.rounds, args.steps)]
    for title, kw in CASES:
        r = cc.measure_capture(dev, _native, dst_size=(256, 256), n=args.steps, rounds=args.rounds, **kw)
        moved = r["source_bytes"] + r["output_bytes"]
        line = "%s\n    one launch %.2f us" % (title, r["fused_us"])
        if "composed_us" in r:
            line += "; torch composition %.2f us; ratio %.4f (%.1f x)" % (r["composed_us"], r["fused_over_composed"],
                                                                        1.0 / r["fused_over_composed"])
        line += "\n    zero-weight share %.3f; whole sources %.1f MB + outputs %.1f MB = %.3f TB/s if every source byte were fetched " \
                "(it is not: UNMEASURED how many are)" % (r["zero_weight_share"], r["source_bytes"] / 1e6, r["output_bytes"] / 1e6,
                                                          moved / (r["fused_us"] * 1e-6) / 1e12)
        line += "\n    rounds: %s" % {k: [round(v, 2) for v in vs] for k, vs in r["rounds"].items()}
        print(line)
        lines.append(line)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
