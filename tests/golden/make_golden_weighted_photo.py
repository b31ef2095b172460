#!/usr/bin/env python3
"""Generate tests/golden/g21_weighted_photo_loss.npz FROM THE REFERENCE ITSELF (the photo losses with per-pixel confidence
weights: PhotoLoss / HeadPhotoLoss with `weights`, svbrdf_*photo_loss_weighted_*).

Run in the build container only (needs the reference checkout, never on the GPU box):

    python tests/golden/make_golden_weighted_photo.py

The reference is imported read-only exactly as make_golden.py imports it.  It has no photo loss, weighted or not; the
fixture composes the definition from the reference's parts, op for op, following make_golden_head_photo.py:

    shape    B = 3, H = 13 (odd: planes of items 1 and 2 start 4 bytes off 16-byte alignment), S = 3 + 6
    scenes   environment.generate_random_scenes(3) + generate_specular_scenes(6) per item under torch.manual_seed(RNG_SEED)
    photos   LocalRenderer.render of OTHER synthetic maps under those scenes with the sensor noise and the clamp to [0, 1]
             of make_golden_photo.py (dataset.py:215-217)
    weights  [B,S,H,W], one plane per photo (tests/weighted_photo_checks.py weight_field): values in (0, 1), about a
             quarter exact 0, a quarter exact 1, image row MASKED_ROW zero in every plane; NaN is then WRITTEN INTO THE
             PHOTOS under about half of the zero weights (all three channels), the whole masked row included
    loss     with p' = where(w > 0, photo, 0):  sum(w |log(render + 0.1) - log(p' + 0.1)|) / N, LocalRenderer.render per
             scene, torch autograd back to the 12 maps; and the same through the reference's head (make_golden_head.py)
             back to the 9 encoded channels of a second input

each once in float32 (the reference as it runs) and once in float64 on the same float32-valued inputs
(make_golden_photo.py: double input and photos, scene vectors as python floats, default dtype float64, torch.linspace
wrapped so that the pixel grid keeps its float32 values).

The seeds were chosen with the C oracle alone so that the tie pixels of both inputs stay within tests/tolerances.py's
MAX_TIE_PIXELS; the counts are printed.  The manifest entry goes to tests/golden/MANIFEST_g21_weighted_photo_loss.json;
MANIFEST.json is left untouched.

DATA ONLY: seeds + sha256 of the synthetic inputs, scenes, photos, weights, the losses and gradients.
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
import weighted_photo_checks  # noqa: E402

NAME = "g21_weighted_photo_loss.npz"
MANIFEST_NAME = "MANIFEST_g21_weighted_photo_loss.json"
B, H, N_RANDOM, N_SPECULAR = 3, 13, 3, 6
INPUT_SEED, ENC_SEED, PHOTO_MAPS_SEED, RNG_SEED, NOISE_SEED, WEIGHT_SEED, NAN_SEED = 2101, 2102, 2103, 41, 43, 2104, 2105
MASKED_ROW = 5
EPS = 0.1


def weighted_loss(maps_t, photos_t, weights_t, scenes):
    R = ref_renderers.LocalRenderer()
    rendered = torch.stack([torch.cat([R.render(sc, maps_t[b]) for sc in scenes[b]], dim=0) for b in range(maps_t.shape[0])], dim=0)
    w = weights_t.to(rendered.dtype).unsqueeze(2)
    p = torch.where((w > 0).expand_as(photos_t), photos_t, torch.zeros((), dtype=photos_t.dtype))
    return (w * (torch.log(rendered + EPS) - torch.log(p + EPS)).abs()).sum() / rendered.numel()


def both_precisions(x_np, photos, weights, scenes, through_head):
    """-> (loss32, grad32, loss64, grad64) of the definition w.r.t. x (12 maps, or 9 encoded channels through the head)"""
    def fn(t, ph, w, sc):
        return weighted_loss(head(t) if through_head else t, ph, w, sc)

    x = torch.from_numpy(x_np).clone().requires_grad_(True)
    loss = fn(x, photos, weights, scenes)
    loss.backward()
    linspace = torch.linspace
    torch.set_default_dtype(torch.float64)
    torch.linspace = lambda *a, **k: linspace(*a, dtype=torch.float32, **k).to(torch.float64)
    try:
        x64 = torch.from_numpy(x_np.astype(np.float64)).requires_grad_(True)
        loss64 = fn(x64, photos.to(torch.float64), weights.to(torch.float64),
                    [[as_float_scene(sc) for sc in row] for row in scenes])
        loss64.backward()
    finally:
        torch.linspace = linspace
        torch.set_default_dtype(torch.float32)
    assert x64.grad.dtype == torch.float64 and loss64.dtype == torch.float64
    assert torch.isfinite(x.grad).all() and torch.isfinite(x64.grad).all() and torch.isfinite(loss) and torch.isfinite(loss64)
    return np.float32(loss.item()), x.grad.numpy(), np.float64(loss64.item()), x64.grad.numpy()


def make():
    inp = synth.make_maps(INPUT_SEED, B, H)
    enc = head_checks.fixture_input(ENC_SEED, B, H)
    other = synth.make_maps(PHOTO_MAPS_SEED, B, H)
    torch.manual_seed(RNG_SEED)
    scenes = [ref_env.generate_random_scenes(N_RANDOM) + ref_env.generate_specular_scenes(N_SPECULAR) for _ in range(B)]
    torch.manual_seed(NOISE_SEED)
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
    photos = torch.stack(photos, dim=0).contiguous().numpy()                # [B,S,3,H,W] float32
    S = photos.shape[1]
    weights = weighted_photo_checks.weight_field(WEIGHT_SEED, B, S, H, masked_rows=False)
    weights[:, :, MASKED_ROW, :] = 0.0
    spoil = (weights == 0.0) & (synth.uniform01(NAN_SEED, weights.shape) < 0.5)
    spoil[:, :, MASKED_ROW, :] = True
    photos[np.broadcast_to(spoil[:, :, None], photos.shape)] = np.nan
    photos_t, weights_t = torch.from_numpy(photos), torch.from_numpy(weights)
    loss, grad, loss64, grad64 = both_precisions(inp, photos_t, weights_t, scenes, False)
    hloss, hgrad, hloss64, hgrad64 = both_precisions(enc, photos_t, weights_t, scenes, True)
    table = np.stack([np.stack([scene_row(sc) for sc in row]) for row in scenes]).astype(np.float32)
    ties = (photo_checks.Reference(inp, photos, table, EPS, weights=weights).n_ties(),
            photo_checks.Reference(enc, photos, table, EPS, head=True, weights=weights).n_ties())
    arrays = dict(
        B=np.int64(B), H=np.int64(H), eps=np.float32(EPS), masked_row=np.int64(MASKED_ROW),
        input_seed=np.int64(INPUT_SEED), enc_seed=np.int64(ENC_SEED), photo_maps_seed=np.int64(PHOTO_MAPS_SEED),
        rng_seed=np.int64(RNG_SEED), noise_seed=np.int64(NOISE_SEED), weight_seed=np.int64(WEIGHT_SEED),
        nan_seed=np.int64(NAN_SEED), input_sha256=np.array(synth.checksum(inp)), enc_sha256=np.array(synth.checksum(enc)),
        photo_maps_sha256=np.array(synth.checksum(other)), scenes=table, photos=photos, weights=weights,
        loss=loss, grad_input=grad, loss_f64=loss64, grad_input_f64=grad64,
        head_loss=hloss, grad9=hgrad, head_loss_f64=hloss64, grad9_f64=hgrad64)
    return arrays, ties


def main():
    arrays, ties = make()
    print("tie pixels by the oracle's composition: maps %d, head %d of %d (cap %d)" % (
        ties[0], ties[1], B * H * H, tolerances.MAX_TIE_PIXELS))
    assert max(ties) <= tolerances.MAX_TIE_PIXELS, "choose other seeds"
    w, ph = arrays["weights"], arrays["photos"]
    print("weights: %d exact 0, %d exact 1, %d inside (0, 1) of %d; NaN photo values %d, all under zero weights: %s" % (
        (w == 0).sum(), (w == 1).sum(), ((w > 0) & (w < 1)).sum(), w.size, np.isnan(ph).sum(),
        bool(np.broadcast_to(w[:, :, None] == 0, ph.shape)[np.isnan(ph)].all())))
    path = os.path.join(HERE, NAME)
    np.savez_compressed(path, **arrays)
    print("wrote %s %8.1f KiB  loss %.9g (f64 %.12g) max|g| %.4e  head loss %.9g (f64 %.12g) max|g9| %.4e" % (
        NAME, os.path.getsize(path) / 1024.0, float(arrays["loss"]), float(arrays["loss_f64"]),
        float(np.abs(arrays["grad_input"]).max()), float(arrays["head_loss"]), float(arrays["head_loss_f64"]),
        float(np.abs(arrays["grad9"]).max())))
    entry = {
        "generator": "tests/golden/make_golden_weighted_photo.py", "torch": torch.__version__, "numpy": np.__version__,
        "cpu_capability": torch.backends.cpu.get_cpu_capability(), "sha256": synth.checksum(np.fromfile(path, np.uint8)),
    }
    with open(os.path.join(HERE, MANIFEST_NAME), "w") as f:
        json.dump({"fixtures": {NAME: entry}}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
