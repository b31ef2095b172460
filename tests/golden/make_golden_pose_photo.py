#!/usr/bin/env python3
"""Generate tests/golden/g23_photo_pose.npz FROM THE REFERENCE ITSELF (the photo losses with the gradient towards the scene
table: PhotoLoss / HeadPhotoLoss with a table that requires grad, svbrdf_*photo_loss_scene_grad_fwd_bwd).

Run in the build container only (needs the reference checkout, never on the GPU box):

    python tests/golden/make_golden_pose_photo.py

The reference is imported read-only exactly as make_golden.py imports it.  Its renderer wraps `camera.pos`, `light.pos` and
`light.color` in torch.Tensor(...) (renderers.py:79,91,98), which cuts autograd there, so the table gradient is taken from
the reference's own float64 RENDERINGS by central differences, per scene and column:

    d rad / d row_k  ~  (render(row + h e_k) - render(row - h e_k)) / 2h          at steps h = H_STEP and h / 2
    t = w sign(delta) (d rad / d row_k) / (N (rad + 0.1))                         chained analytically, delta in float64
    G = sum t,  A = sum |t|,  T = sum |t| over the tied terms (tests/pose_photo_checks.py's rule)

The two steps must agree to 1e-7 A (asserted: a clamp or a sign change inside +-h would show here); the h / 2 value is
stored, with A and T.  Everything else follows make_golden_weighted_photo.py, op for op:

    shape     B = 3, H = 13, S = 3 + 6
    scenes    environment.generate_random_scenes(3) + generate_specular_scenes(6) per item under torch.manual_seed(RNG_SEED)
    photos    LocalRenderer.render of OTHER synthetic maps under those scenes with sensor noise and the clamp to [0, 1]
    weights   [B,S,H,W], one plane per photo (weighted_photo_checks.weight_field), image row MASKED_ROW zero in every
              plane; NaN WRITTEN INTO THE PHOTOS under about half of the zero weights
    loss      with p' = where(w > 0, photo, 0):  sum(w |log(render + 0.1) - log(p' + 0.1)|) / N, torch autograd back to the
              12 maps; the same through the reference's head back to the 9 encoded channels of a second input

each once in float32 and once in float64 on the same float32-valued inputs.  The seeds were chosen with the helper
(tests/pose_photo_checks.py) so that tie pixels and tied terms stay within tests/tolerances.py's MAX_TIE_PIXELS and no sign
flips outside them; the counts are printed.  The manifest entry goes to tests/golden/MANIFEST_g23_photo_pose.json.

DATA ONLY: seeds + sha256 of the synthetic inputs, scenes, photos, weights, the losses and gradients.
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
from make_golden_weighted_photo import both_precisions  # noqa: E402

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import head_checks  # noqa: E402   (tests/ is on the path through make_golden)
import photo_checks  # noqa: E402
import pose_photo_checks  # noqa: E402
import tolerances  # noqa: E402
import weighted_photo_checks  # noqa: E402

NAME = "g23_photo_pose.npz"
MANIFEST_NAME = "MANIFEST_g23_photo_pose.json"
B, H, N_RANDOM, N_SPECULAR = 3, 13, 3, 6
INPUT_SEED, ENC_SEED, PHOTO_MAPS_SEED, RNG_SEED, NOISE_SEED, WEIGHT_SEED, NAN_SEED = 2301, 2302, 2303, 59, 61, 2304, 2305
MASKED_ROW = 5
EPS = 0.1
H_STEP = 5e-6


def scene_gradient(x_np, photos, weights, table, through_head):
    """-> (G [B,S,9] at h / 2, A, T, worst |G(h) - G(h/2)| / A, tied terms): central differences of the reference's float64
    renderings, chained through the loss analytically"""
    linspace = torch.linspace
    torch.set_default_dtype(torch.float64)
    torch.linspace = lambda *a, **k: linspace(*a, dtype=torch.float32, **k).to(torch.float64)
    try:
        R = ref_renderers.LocalRenderer()
        x64 = torch.from_numpy(x_np.astype(np.float64))
        maps = head(x64) if through_head else x64
        rows = table.astype(np.float64)
        S = rows.shape[1]

        def render(b, row):
            sc = ref_env.Scene(ref_env.Camera(row[0:3].tolist()), ref_env.Light(row[3:6].tolist(), row[6:9].tolist()))
            return R.render(sc, maps[b])[0].numpy()

        rad = np.stack([np.stack([render(b, rows[b, s]) for s in range(S)]) for b in range(B)])
        drad = {}
        for h in (H_STEP, H_STEP / 2):
            d = np.empty((B, S, 9) + rad.shape[2:], np.float64)
            for b, s, k in np.ndindex(B, S, 9):
                up, dn = rows[b, s].copy(), rows[b, s].copy()
                up[k] += h
                dn[k] -= h
                d[b, s, k] = (render(b, up) - render(b, dn)) / (2 * h)
            drad[h] = d
    finally:
        torch.linspace = linspace
        torch.set_default_dtype(torch.float32)
    assert rad.dtype == np.float64
    ph = photo_checks.excused_photos(photos, weights).astype(np.float64)
    w = weights.astype(np.float64)[:, :, None]
    delta = np.log(rad + EPS) - np.log(ph + EPS)
    g = w * np.sign(delta) / (delta.size * (rad + EPS))
    t = {h: g[:, :, None] * d for h, d in drad.items()}
    G = {h: v.sum(axis=(3, 4, 5)) for h, v in t.items()}
    fine = t[H_STEP / 2]
    A = np.abs(fine).sum(axis=(3, 4, 5))
    maps32 = maps.numpy().astype(np.float32)
    structural = ((ph == 0.0) & (photo_checks.unclamped_n_dot_wi(maps32, table) < -1e-6)[:, :, None]) | (weights == 0.0)[:, :, None]
    tied = (np.abs(delta) < tolerances.TIE_LEVEL) & ~structural
    T = np.where(tied[:, :, None], np.abs(fine), 0.0).sum(axis=(3, 4, 5))
    return G[H_STEP / 2], A, T, float((np.abs(G[H_STEP] - G[H_STEP / 2]) / A).max()), int(tied.sum())


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
    G, A, T, step_gap, tied = scene_gradient(inp, photos, weights, table, False)
    hG, hA, hT, hstep_gap, htied = scene_gradient(enc, photos, weights, table, True)
    print("central differences at h = %g and h / 2: worst |G(h) - G(h/2)| / A  maps %.3g  head %.3g" % (H_STEP, step_gap, hstep_gap))
    assert step_gap <= 1e-7 and hstep_gap <= 1e-7, "a clamp or a sign change inside +-h: choose other seeds"
    refs = (pose_photo_checks.PoseReference(inp, photos, table, EPS, False, weights),
            pose_photo_checks.PoseReference(enc, photos, table, EPS, True, weights))
    arrays = dict(
        B=np.int64(B), H=np.int64(H), eps=np.float32(EPS), masked_row=np.int64(MASKED_ROW), h_step=np.float64(H_STEP),
        input_seed=np.int64(INPUT_SEED), enc_seed=np.int64(ENC_SEED), photo_maps_seed=np.int64(PHOTO_MAPS_SEED),
        rng_seed=np.int64(RNG_SEED), noise_seed=np.int64(NOISE_SEED), weight_seed=np.int64(WEIGHT_SEED),
        nan_seed=np.int64(NAN_SEED), input_sha256=np.array(synth.checksum(inp)),
        enc_sha256=np.array(synth.checksum(enc)), photo_maps_sha256=np.array(synth.checksum(other)), scenes=table,
        photos=photos, weights=weights,
        loss=loss, grad_input=grad, loss_f64=loss64, grad_input_f64=grad64, grad_scenes_f64=G, scene_A=A, scene_T=T,
        head_loss=hloss, grad9=hgrad, head_loss_f64=hloss64, grad9_f64=hgrad64, head_grad_scenes_f64=hG, head_scene_A=hA,
        head_scene_T=hT)
    return arrays, refs, (tied, htied)


def main():
    arrays, refs, tied = make()
    for what, r, n_tied, key in zip(("maps", "head"), refs, tied, ("grad_scenes_f64", "head_grad_scenes_f64")):
        print("%s by the helper: %d tie pixels, %d tied terms of the scene gradient (%d by the reference's renderings), %d sign "
              "flips outside them (cap %d); the reference's central differences against the helper's duals: err/bound %.3g, "
              "err/A %.3g" % ((what, r.ref.n_ties(), r.tied_terms, n_tied, r.sign_flips, tolerances.MAX_TIE_PIXELS) + r.worst(arrays[key])))
        assert r.ref.n_ties() <= tolerances.MAX_TIE_PIXELS and r.tied_terms <= tolerances.MAX_TIE_PIXELS and r.sign_flips == 0 \
            and n_tied <= tolerances.MAX_TIE_PIXELS, "choose other seeds"
    path = os.path.join(HERE, NAME)
    np.savez_compressed(path, **arrays)
    print("wrote %s %8.1f KiB  loss %.9g (f64 %.12g) max|g| %.4e max|gs| %.4e  head loss %.9g (f64 %.12g) max|g9| %.4e" % (
        NAME, os.path.getsize(path) / 1024.0, float(arrays["loss"]), float(arrays["loss_f64"]),
        float(np.abs(arrays["grad_input"]).max()), float(np.abs(arrays["grad_scenes_f64"]).max()), float(arrays["head_loss"]),
        float(arrays["head_loss_f64"]), float(np.abs(arrays["grad9"]).max())))
    entry = {
        "generator": "tests/golden/make_golden_pose_photo.py", "torch": torch.__version__, "numpy": np.__version__,
        "cpu_capability": torch.backends.cpu.get_cpu_capability(), "sha256": synth.checksum(np.fromfile(path, np.uint8)),
    }
    with open(os.path.join(HERE, MANIFEST_NAME), "w") as f:
        json.dump({"fixtures": {NAME: entry}}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
