#!/usr/bin/env python3
"""Generate tests/golden/g20_head_photo_loss.npz FROM THE REFERENCE ITSELF (the head-fused photo loss: HeadPhotoLoss,
svbrdf_head_photo_loss_*).

Run in the build container only (needs the reference checkout, never on the GPU box):

    python tests/golden/make_golden_head_photo.py

The reference (mworchel/svbrdf-estimation, development/multiImage_pytorch) is imported read-only exactly as
make_golden.py imports it: byte-code writing disabled, empty placeholder modules for `cv2` and `pyredner`.

The reference has no photo loss of its own; the fixture composes it from the reference's parts, op for op:

    shape    B = 3, H = 13: the plane has 169 elements, so the 9 encoded planes, the 9 gradient planes and the photos of
             items 1 and 2 start 4 bytes off 16-byte alignment
    input    tests/head_checks.py `fixture_input`: tanh(4 z), and image rows 0..7 with one channel group at a time at exactly
             -1 or +1 (make_golden_head.py)
    scenes   S = 3 + 6 per item from environment.generate_random_scenes / generate_specular_scenes under
             torch.manual_seed(RNG_SEED)
    photos   LocalRenderer.render of OTHER synthetic maps under those scenes, with the sensor noise and the clamp to [0, 1]
             of make_golden_photo.py (dataset.py:215-217)
    loss     the reference's own head (models.py:338-346: utils.decode_svbrdf, then encode_as_unit_interval of diffuse,
             roughness and specular: make_golden_head.py::head), LocalRenderer.render per scene, log(x + 0.1), l1_loss
             against log(photo + 0.1), autograd back to the 9 encoded channels

once in float32 (the reference as it runs) and once in float64 on the same float32-valued inputs (make_golden_photo.py:
double input and photos, scene vectors as python floats, default dtype float64, torch.linspace wrapped so that the pixel
grid keeps its float32 values).

The saturated input makes exact ties likelier than the sweeps' inputs do (a photo value of exactly 0 meets a rendering of
~1e-8 from near-zero decoded roughness and diffuse): the seeds below were chosen with the C oracle alone so that the tie
pixels stay within tests/tolerances.py's MAX_TIE_PIXELS; the count is printed.

The manifest entry of the fixture (generator, torch / numpy versions, sha256 of the file) goes to
tests/golden/MANIFEST_g20_head_photo_loss.json, under "fixtures" as in MANIFEST.json, which is left untouched.

DATA ONLY: seeds + sha256 of the input and of the photographed maps, scenes, photos, the two losses and 9-channel gradients.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
# make_golden.py imports the reference (placeholder modules for cv2 / pyredner, no byte-code) when it is imported itself
import make_golden  # noqa: E402,F401
from make_golden import ref_env, ref_renderers, scene_row, synth  # noqa: E402
from make_golden_head import head  # noqa: E402
from make_golden_photo import as_float_scene  # noqa: E402

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository root: the helpers import the C oracle
import head_checks  # noqa: E402   (tests/ is on the path through make_golden)
import photo_checks  # noqa: E402
import tolerances  # noqa: E402

NAME = "g20_head_photo_loss.npz"
MANIFEST_NAME = "MANIFEST_g20_head_photo_loss.json"
B, H, N_RANDOM, N_SPECULAR = 3, 13, 3, 6
ENC_SEED, PHOTO_MAPS_SEED, RNG_SEED, NOISE_SEED = 2003, 2004, 21, 31
EPS = 0.1


def head_photo_loss(enc_t, photos_t, scenes):
    R = ref_renderers.LocalRenderer()
    maps = head(enc_t)
    rendered = torch.stack([torch.cat([R.render(sc, maps[b]) for sc in scenes[b]], dim=0) for b in range(enc_t.shape[0])], dim=0)
    return torch.nn.functional.l1_loss(torch.log(rendered + EPS), torch.log(photos_t + EPS))


def make(enc_seed=ENC_SEED, photo_maps_seed=PHOTO_MAPS_SEED, rng_seed=RNG_SEED, noise_seed=NOISE_SEED):
    enc = head_checks.fixture_input(enc_seed, B, H)
    other = synth.make_maps(photo_maps_seed, B, H)
    torch.manual_seed(rng_seed)
    scenes = [ref_env.generate_random_scenes(N_RANDOM) + ref_env.generate_specular_scenes(N_SPECULAR) for _ in range(B)]
    torch.manual_seed(noise_seed)
    R = ref_renderers.LocalRenderer()
    photos = []
    for b in range(B):
        per_item = []
        for sc in scenes[b]:
            rendering = R.render(sc, torch.from_numpy(other[b]).unsqueeze(0))
            std = torch.exp(torch.Tensor(1).normal_(mean=np.log(0.005), std=0.3)).numpy()[0]
            noise = torch.zeros_like(rendering).normal_(mean=0.0, std=std)
            per_item.append(torch.clamp(rendering + noise, min=0.0, max=1.0))
        photos.append(torch.cat(per_item, dim=0))
    photos = torch.stack(photos, dim=0).contiguous()            # [B,S,3,H,W] float32
    x = torch.from_numpy(enc).clone().requires_grad_(True)
    loss = head_photo_loss(x, photos, scenes)
    loss.backward()
    linspace = torch.linspace
    torch.set_default_dtype(torch.float64)
    torch.linspace = lambda *a, **k: linspace(*a, dtype=torch.float32, **k).to(torch.float64)
    try:
        x64 = torch.from_numpy(enc.astype(np.float64)).requires_grad_(True)
        loss64 = head_photo_loss(x64, photos.to(torch.float64), [[as_float_scene(sc) for sc in row] for row in scenes])
        loss64.backward()
    finally:
        torch.linspace = linspace
        torch.set_default_dtype(torch.float32)
    assert x64.grad.dtype == torch.float64 and loss64.dtype == torch.float64
    table = np.stack([np.stack([scene_row(sc) for sc in row]) for row in scenes]).astype(np.float32)
    ties = photo_checks.Reference(enc, photos.numpy(), table, EPS, head=True).n_ties()
    arrays = dict(
        B=np.int64(B), H=np.int64(H), eps=np.float32(EPS), enc_seed=np.int64(enc_seed),
        photo_maps_seed=np.int64(photo_maps_seed), rng_seed=np.int64(rng_seed), noise_seed=np.int64(noise_seed),
        enc_sha256=np.array(synth.checksum(enc)), photo_maps_sha256=np.array(synth.checksum(other)), scenes=table,
        photos=photos.numpy(), loss=np.float32(loss.item()), grad9=x.grad.numpy(), loss_f64=np.float64(loss64.item()),
        grad9_f64=x64.grad.numpy())
    return arrays, ties


def main():
    arrays, ties = make()
    print("tie pixels by the oracle's composition: %d of %d (cap %d)" % (ties, B * H * H, tolerances.MAX_TIE_PIXELS))
    assert ties <= tolerances.MAX_TIE_PIXELS, "choose other seeds"
    path = os.path.join(HERE, NAME)
    np.savez_compressed(path, **arrays)
    print("wrote %s %8.1f KiB  loss %.9g  f64 %.12g  max|g9| %.4e" % (
        NAME, os.path.getsize(path) / 1024.0, float(arrays["loss"]), float(arrays["loss_f64"]),
        float(np.abs(arrays["grad9"]).max())))
    # the entry MANIFEST.json's "fixtures" holds for a fixture with a generator of its own (make_golden_head.py), in a file
    # of this fixture's: MANIFEST.json is written by make_golden.py and stays as that left it
    entry = {
        "generator": "tests/golden/make_golden_head_photo.py", "torch": torch.__version__, "numpy": np.__version__,
        "cpu_capability": torch.backends.cpu.get_cpu_capability(), "sha256": synth.checksum(np.fromfile(path, np.uint8)),
    }
    with open(os.path.join(HERE, MANIFEST_NAME), "w") as f:
        json.dump({"fixtures": {NAME: entry}}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
