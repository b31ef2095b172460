#!/usr/bin/env python3
"""Generate tests/golden/g18_photo_loss.npz FROM THE REFERENCE ITSELF (the photo loss: PhotoLoss, svbrdf_photo_loss_*).

Run in the build container only (needs the reference checkout, never on the GPU box):

    python tests/golden/make_golden_photo.py

The reference (mworchel/svbrdf-estimation, development/multiImage_pytorch) is imported read-only exactly as
make_golden.py imports it: byte-code writing disabled, empty placeholder modules for `cv2` and `pyredner`.

The reference has no photo loss of its own; the fixture composes it from the reference's parts, op for op:

    scenes   S = 9 per item from environment.generate_random_scenes(3) + generate_specular_scenes(6), as
             RenderingLoss.forward draws them (losses.py:35), under torch.manual_seed(RNG_SEED)
    photos   LocalRenderer.render (renderers.py:67-104) of OTHER maps under those scenes, with the sensor noise of
             dataset.py:215-217: std = exp(N(log 0.005, 0.3)), + N(0, std), clamp to [0, 1]
    loss     mean | log(render(scene, input) + 0.1) - log(photo + 0.1) |  -- losses.py:46-50 with the photo in the target's
             place -- and its autograd gradient w.r.t. the input maps

once in float32 (the reference as it runs) and once in float64 on the same float32-valued inputs: double maps and photos,
scene vectors as python floats, torch's default dtype float64, and torch.linspace wrapped so that the pixel grid keeps
the float32 values of renderers.py:73 (the "f64" of tests/tolerances.py: the reference's formulas evaluated in double on
the same fp32 inputs).  DATA ONLY: seeds + sha256 of the synthetic maps, scenes, photos, the two losses and gradients.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
# make_golden.py imports the reference (placeholder modules for cv2 / pyredner, no byte-code) when it is imported itself
import make_golden  # noqa: E402
from make_golden import ref_env, ref_renderers, scene_row, synth  # noqa: E402

import torch  # noqa: E402

B, H, N_RANDOM, N_SPECULAR = 2, 32, 3, 6
INPUT_SEED, PHOTO_MAPS_SEED, RNG_SEED, NOISE_SEED = 181, 182, 23, 29
EPS = 0.1


def as_float_scene(sc):
    """the same scene with python-float vectors: torch.Tensor(list) then takes the default dtype (renderers.py:79,91,98)"""
    row = scene_row(sc).astype(np.float64).tolist()
    return ref_env.Scene(ref_env.Camera(row[0:3]), ref_env.Light(row[3:6], row[6:9]))


def photo_loss(maps_t, photos_t, scenes):
    R = ref_renderers.LocalRenderer()
    rendered = torch.stack([torch.cat([R.render(sc, maps_t[b]) for sc in scenes[b]], dim=0) for b in range(maps_t.shape[0])], dim=0)
    return torch.nn.functional.l1_loss(torch.log(rendered + EPS), torch.log(photos_t + EPS))


def main():
    inp = synth.make_maps(INPUT_SEED, B, H)
    other = synth.make_maps(PHOTO_MAPS_SEED, B, H)
    torch.manual_seed(RNG_SEED)
    scenes = [ref_env.generate_random_scenes(N_RANDOM) + ref_env.generate_specular_scenes(N_SPECULAR) for _ in range(B)]
    # photos: dataset.py:206-219 on the other maps
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
    photos = torch.stack(photos, dim=0).contiguous()            # [B,S,3,H,W] float32
    # float32: the reference as it runs
    x = torch.from_numpy(inp).clone().requires_grad_(True)
    loss = photo_loss(x, photos, scenes)
    loss.backward()
    # float64 on the same float32-valued inputs
    linspace = torch.linspace
    torch.set_default_dtype(torch.float64)
    torch.linspace = lambda *a, **k: linspace(*a, dtype=torch.float32, **k).to(torch.float64)
    try:
        x64 = torch.from_numpy(inp.astype(np.float64)).requires_grad_(True)
        loss64 = photo_loss(x64, photos.to(torch.float64), [[as_float_scene(sc) for sc in row] for row in scenes])
        loss64.backward()
    finally:
        torch.linspace = linspace
        torch.set_default_dtype(torch.float32)
    assert x64.grad.dtype == torch.float64 and loss64.dtype == torch.float64
    path = os.path.join(HERE, "g18_photo_loss.npz")
    np.savez_compressed(
        path, B=np.int64(B), H=np.int64(H), eps=np.float32(EPS), input_seed=np.int64(INPUT_SEED),
        photo_maps_seed=np.int64(PHOTO_MAPS_SEED), rng_seed=np.int64(RNG_SEED), noise_seed=np.int64(NOISE_SEED),
        input_sha256=np.array(synth.checksum(inp)), photo_maps_sha256=np.array(synth.checksum(other)),
        scenes=np.stack([np.stack([scene_row(sc) for sc in row]) for row in scenes]).astype(np.float32),
        photos=photos.numpy(), loss=np.float32(loss.item()), grad_input=x.grad.numpy(),
        loss_f64=np.float64(loss64.item()), grad_input_f64=x64.grad.numpy())
    print("wrote g18_photo_loss.npz %8.1f KiB  loss %.9g  f64 %.12g  max|g| %.4e" % (
        os.path.getsize(path) / 1024.0, loss.item(), loss64.item(), float(x.grad.abs().max())))


if __name__ == "__main__":
    main()
