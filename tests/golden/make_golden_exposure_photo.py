#!/usr/bin/env python3
"""Generate tests/golden/g22_photo_exposure.npz FROM THE REFERENCE ITSELF (the photo losses with a per-photo exposure:
PhotoLoss / HeadPhotoLoss with `exposure`, svbrdf_*photo_loss_exposure_fwd_bwd).

Run in the build container only (needs the reference checkout, never on the GPU box):

    python tests/golden/make_golden_exposure_photo.py

The reference is imported read-only exactly as make_golden.py imports it.  Its renderer has no exposure
(renderers.py:102 ends in a TODO for it) and wraps `light.color` in torch.Tensor(...), which cuts autograd there, so the gain
is a LEAF [B,S,3,1,1] that multiplies the reference's own LocalRenderer.render output -- the rendering is linear in the light
colour the kernels scale instead.  Everything else follows make_golden_weighted_photo.py, op for op:

    shape     B = 3, H = 13, S = 3 + 6
    scenes    environment.generate_random_scenes(3) + generate_specular_scenes(6) per item under torch.manual_seed(RNG_SEED)
    photos    LocalRenderer.render of OTHER synthetic maps under those scenes with sensor noise and the clamp to [0, 1]
    weights   [B,S,H,W], one plane per photo (weighted_photo_checks.weight_field), image row MASKED_ROW zero in every
              plane; NaN WRITTEN INTO THE PHOTOS under about half of the zero weights
    exposure  uniform in [0.5, 2) per photo and colour channel (synth.uniform01)
    loss      with p' = where(w > 0, photo, 0):  sum(w |log(e render + 0.1) - log(p' + 0.1)|) / N, torch autograd back to
              the 12 maps AND to e; the same through the reference's head back to the 9 encoded channels of a second input

each once in float32 and once in float64 on the same float32-valued inputs.  The seeds were chosen with the C oracle alone
(tests/exposure_photo_checks.py) so that tie pixels and tied terms stay within tests/tolerances.py's MAX_TIE_PIXELS; the
counts are printed.  The manifest entry goes to tests/golden/MANIFEST_g22_photo_exposure.json.

DATA ONLY: seeds + sha256 of the synthetic inputs, scenes, photos, weights, gains, the losses and gradients.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401
from make_golden import ref_env, ref_renderers, scene_row, synth  # noqa: E402
from make_golden_head import head  # noqa: E402
from make_golden_photo import as_float_scene  # noqa: E402

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import exposure_photo_checks  # noqa: E402   (tests/ is on the path through make_golden)
import head_checks  # noqa: E402
import tolerances  # noqa: E402
import weighted_photo_checks  # noqa: E402

NAME = "g22_photo_exposure.npz"
MANIFEST_NAME = "MANIFEST_g22_photo_exposure.json"
B, H, N_RANDOM, N_SPECULAR = 3, 13, 3, 6
INPUT_SEED, ENC_SEED, PHOTO_MAPS_SEED, RNG_SEED, NOISE_SEED, WEIGHT_SEED, NAN_SEED, GAIN_SEED = 2201, 2202, 2203, 47, 53, 2204, 2205, 2206
MASKED_ROW = 5
EPS = 0.1


def exposure_loss(maps_t, photos_t, weights_t, gain_t, scenes):
    R = ref_renderers.LocalRenderer()
    rendered = torch.stack([torch.cat([R.render(sc, maps_t[b]) for sc in scenes[b]], dim=0) for b in range(maps_t.shape[0])], dim=0)
    rendered = rendered * gain_t                                             # [B,S,3,1,1] leaf
    w = weights_t.to(rendered.dtype).unsqueeze(2)
    p = torch.where((w > 0).expand_as(photos_t), photos_t, torch.zeros((), dtype=photos_t.dtype))
    return (w * (torch.log(rendered + EPS) - torch.log(p + EPS)).abs()).sum() / rendered.numel()


def both_precisions(x_np, photos, weights, gain_np, scenes, through_head):
    """-> (loss32, grad32, ge32, loss64, grad64, ge64) w.r.t. x (12 maps, or 9 encoded channels through the head) and the gains"""
    def fn(t, ph, w, e, sc):
        return exposure_loss(head(t) if through_head else t, ph, w, e, sc)

    x = torch.from_numpy(x_np).clone().requires_grad_(True)
    e = torch.from_numpy(gain_np).clone().reshape(B, -1, 3, 1, 1).requires_grad_(True)
    loss = fn(x, photos, weights, e, scenes)
    loss.backward()
    linspace = torch.linspace
    torch.set_default_dtype(torch.float64)
    torch.linspace = lambda *a, **k: linspace(*a, dtype=torch.float32, **k).to(torch.float64)
    try:
        x64 = torch.from_numpy(x_np.astype(np.float64)).requires_grad_(True)
        e64 = torch.from_numpy(gain_np.astype(np.float64)).reshape(B, -1, 3, 1, 1).requires_grad_(True)
        loss64 = fn(x64, photos.to(torch.float64), weights.to(torch.float64), e64,
                    [[as_float_scene(sc) for sc in row] for row in scenes])
        loss64.backward()
    finally:
        torch.linspace = linspace
        torch.set_default_dtype(torch.float32)
    assert x64.grad.dtype == torch.float64 and e64.grad.dtype == torch.float64 and loss64.dtype == torch.float64
    for t in (x.grad, x64.grad, e.grad, e64.grad, loss, loss64):
        assert torch.isfinite(t).all()
    return (np.float32(loss.item()), x.grad.numpy(), e.grad.numpy().reshape(B, -1, 3),
            np.float64(loss64.item()), x64.grad.numpy(), e64.grad.numpy().reshape(B, -1, 3))


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
    gain = (np.float32(0.5) + np.float32(1.5) * synth.uniform01(GAIN_SEED, (B, S, 3))).astype(np.float32)
    photos_t, weights_t = torch.from_numpy(photos), torch.from_numpy(weights)
    loss, grad, ge, loss64, grad64, ge64 = both_precisions(inp, photos_t, weights_t, gain, scenes, False)
    hloss, hgrad, hge, hloss64, hgrad64, hge64 = both_precisions(enc, photos_t, weights_t, gain, scenes, True)
    table = np.stack([np.stack([scene_row(sc) for sc in row]) for row in scenes]).astype(np.float32)
    refs = (exposure_photo_checks.ExposureReference(inp, photos, table, gain, EPS, False, weights),
            exposure_photo_checks.ExposureReference(enc, photos, table, gain, EPS, True, weights))
    arrays = dict(
        B=np.int64(B), H=np.int64(H), eps=np.float32(EPS), masked_row=np.int64(MASKED_ROW),
        input_seed=np.int64(INPUT_SEED), enc_seed=np.int64(ENC_SEED), photo_maps_seed=np.int64(PHOTO_MAPS_SEED),
        rng_seed=np.int64(RNG_SEED), noise_seed=np.int64(NOISE_SEED), weight_seed=np.int64(WEIGHT_SEED),
        nan_seed=np.int64(NAN_SEED), gain_seed=np.int64(GAIN_SEED), input_sha256=np.array(synth.checksum(inp)),
        enc_sha256=np.array(synth.checksum(enc)), photo_maps_sha256=np.array(synth.checksum(other)), scenes=table,
        photos=photos, weights=weights, exposure=gain,
        loss=loss, grad_input=grad, grad_exposure=ge, loss_f64=loss64, grad_input_f64=grad64, grad_exposure_f64=ge64,
        head_loss=hloss, grad9=hgrad, head_grad_exposure=hge, head_loss_f64=hloss64, grad9_f64=hgrad64,
        head_grad_exposure_f64=hge64)
    return arrays, refs


def main():
    arrays, refs = make()
    for what, r in zip(("maps", "head"), refs):
        print("%s by the oracle's composition: %d tie pixels, %d tied terms of the exposure gradient, %d sign flips outside them "
              "(cap %d)" % (what, r.ref.n_ties(), r.tied_terms, r.sign_flips, tolerances.MAX_TIE_PIXELS))
        assert r.ref.n_ties() <= tolerances.MAX_TIE_PIXELS and r.tied_terms <= tolerances.MAX_TIE_PIXELS and r.sign_flips == 0, \
            "choose other seeds"
    path = os.path.join(HERE, NAME)
    np.savez_compressed(path, **arrays)
    print("wrote %s %8.1f KiB  loss %.9g (f64 %.12g) max|g| %.4e max|ge| %.4e  head loss %.9g (f64 %.12g) max|g9| %.4e" % (
        NAME, os.path.getsize(path) / 1024.0, float(arrays["loss"]), float(arrays["loss_f64"]),
        float(np.abs(arrays["grad_input"]).max()), float(np.abs(arrays["grad_exposure"]).max()), float(arrays["head_loss"]),
        float(arrays["head_loss_f64"]), float(np.abs(arrays["grad9"]).max())))
    entry = {
        "generator": "tests/golden/make_golden_exposure_photo.py", "torch": torch.__version__, "numpy": np.__version__,
        "cpu_capability": torch.backends.cpu.get_cpu_capability(), "sha256": synth.checksum(np.fromfile(path, np.uint8)),
    }
    with open(os.path.join(HERE, MANIFEST_NAME), "w") as f:
        json.dump({"fixtures": {NAME: entry}}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
