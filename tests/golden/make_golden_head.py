#!/usr/bin/env python3
"""Generate tests/golden/g19_head_loss_edges.npz FROM THE REFERENCE ITSELF (the head-fused loss at its edges).

Run in the build container only (needs the reference checkout, never on the GPU box):

    python tests/golden/make_golden_head.py

The reference (mworchel/svbrdf-estimation, development/multiImage_pytorch) is imported read-only exactly as
make_golden.py imports it: byte-code writing disabled, empty placeholder modules for `cv2` and `pyredner`.

What g11_head_loss.npz (make_golden.py) leaves out:

    shape    B = 3, H = 13: the plane has 169 elements, so the 9 encoded planes and the 9 gradient planes of items 1 and 2
             start 4 bytes off 16-byte alignment
    input    tests/head_checks.py `tanh_case`: tanh(4 z) of tests/synth.py's approximate normals, rounded to float32 -- the
             distribution a trained generator's tanh produces, with a few per cent of the values at exactly -1.0 / +1.0 --
             plus image rows 0..7 in which ONE channel group (normal xy 0:2, diffuse 2:5, roughness 5, specular 6:9) is forced
             to -1 (even row) or +1 (odd row): diffuse / specular decode to exactly 0 or 1, roughness to exactly 0 (below the
             renderer's 1e-3 clamp: its gradient mask) or 1, the normal to (+-3, +-3, 1)/sqrt(19)
    loss     the reference's own head (models.py:338-346: utils.decode_svbrdf, then encode_as_unit_interval of diffuse,
             roughness and specular), MixedLoss(l1_weight = 0.1) and RenderingLoss under torch.manual_seed(RNG_SEED), autograd
             back to the 9 encoded channels, on the CPU in float32

DATA ONLY: the encoded input and its sha256 and seed, the target maps (tests/synth.py) and their seed, the scenes the
reference drew, the two losses, the two 9-channel gradients, the decoded maps and the RNG seed.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
# make_golden.py imports the reference (placeholder modules for cv2 / pyredner, no byte-code) when it is imported itself
import make_golden  # noqa: E402
from make_golden import _Recorder, ref_losses, ref_renderers, ref_utils, synth  # noqa: E402

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root: head_checks imports the C oracle
import head_checks  # noqa: E402   (tests/ is on the path through make_golden)

NAME = "g19_head_loss_edges.npz"
B, H = 3, 13
ENC_SEED, TARGET_SEED, RNG_SEED = 1901, 1902, 19


def head(t):
    sv = ref_utils.decode_svbrdf(t)
    n, d, r, s = ref_utils.unpack_svbrdf(sv)
    return ref_utils.pack_svbrdf(n, ref_utils.encode_as_unit_interval(d), ref_utils.encode_as_unit_interval(r),
                                 ref_utils.encode_as_unit_interval(s))


def main():
    enc = head_checks.fixture_input(ENC_SEED, B, H)
    tgt = synth.make_maps(TARGET_SEED, B, H, tiled_roughness=True)
    out = {}
    for tag, w in (("mixed", 0.1), ("render", 0.0)):
        x = torch.from_numpy(enc).clone().requires_grad_(True)
        maps = head(x)
        torch.manual_seed(RNG_SEED)
        with _Recorder() as rec:
            if w:
                loss = ref_losses.MixedLoss(ref_renderers.LocalRenderer(), l1_weight=w)(maps, torch.from_numpy(tgt))
            else:
                loss = ref_losses.RenderingLoss(ref_renderers.LocalRenderer())(maps, torch.from_numpy(tgt))
        loss.backward()
        out[tag + "_loss"] = np.float32(loss.item())
        out[tag + "_grad9"] = x.grad.numpy()
        if "scenes" in out:
            assert np.array_equal(out["scenes"], rec.table()), "the two losses drew different scenes"
        out["scenes"] = rec.table()
        out["decoded12"] = maps.detach().numpy()
    path = os.path.join(HERE, NAME)
    np.savez_compressed(path, B=np.int64(B), H=np.int64(H), enc9=enc, enc_seed=np.int64(ENC_SEED),
                        enc_sha256=np.array(synth.checksum(enc)), target=tgt, target_seed=np.int64(TARGET_SEED),
                        target_sha256=np.array(synth.checksum(tgt)), rng_seed=np.int64(RNG_SEED), **out)
    print("wrote %s %8.1f KiB  mixed %.9g  render %.9g  max|g9| %.4e" % (
        NAME, os.path.getsize(path) / 1024.0, float(out["mixed_loss"]), float(out["render_loss"]),
        float(np.abs(out["mixed_grad9"]).max())))
    # MANIFEST.json: the environment make_golden.py recorded stays; fixtures written by a generator of their own are listed
    man_path = os.path.join(HERE, "MANIFEST.json")
    with open(man_path) as f:
        manifest = json.load(f)
    manifest.setdefault("fixtures", {})[NAME] = {
        "generator": "tests/golden/make_golden_head.py", "torch": torch.__version__, "numpy": np.__version__,
        "cpu_capability": torch.backends.cpu.get_cpu_capability(), "sha256": synth.checksum(np.fromfile(path, np.uint8)),
    }
    with open(man_path, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
