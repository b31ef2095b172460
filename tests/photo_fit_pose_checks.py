"""Shared by tests/test_photo_fit_pose_cpu.py and tests/test_gpu_photo_fit_pose.py: the direct C ABI calls of the joint fit
step (csrc/svbrdf_photo_fit_pose.hip, svbrdf_photo_fit_adam_step_scene_grad) and of its reference value, the scene-gradient
entry svbrdf_photo_loss_scene_grad_fwd_bwd, on the cases of photo_fit_checks -- every buffer between canaries -- and the
speed measurement.  No golden fixture of its own: the scene-gradient entry is pinned to the reference by g23, the loss and
the map gradient by g18 / g21, Adam by the restatement that tests/test_photo_fit_cpu.py holds against float64
torch.optim.Adam.
"""
import ctypes

import numpy as np

import photo_checks
import photo_fit_checks as fc

EPS = fc.EPS
JOINT_ENTRY, SCENE_GRAD_ENTRY, WORKSPACE_BYTES = ("svbrdf_photo_fit_adam_step_scene_grad", "svbrdf_photo_loss_scene_grad_fwd_bwd",
                                                  "svbrdf_photo_scene_grad_workspace_bytes")
PARTIAL_WAVE_CASES = ("b1_7_s1", "b3_17_s1_shared", "b1_17_s5", "b3_7_s2_shared_untied")      # H W is no multiple of 64


def scratch(lib, dev, c):
    import torch
    need = getattr(lib, WORKSPACE_BYTES)(c["B"], c["S"], c["H"], c["H"])
    assert need == (65 + 9 * c["B"] * c["S"]) * 8
    return torch.zeros(need // 8, dtype=torch.int64, device=dev)


def _weights(c, dev, shift):
    if c["weights"] is None:
        return None, None, 0
    w = fc.Guarded(c["weights"], dev, shift)
    return w, w.ptr(), int(c["weights"].shape[1])


def abi_scene_grad(native, dev, c, shift=0):
    """svbrdf_photo_loss_scene_grad_fwd_bwd on the case's inputs through its own ctypes call
    -> (loss float32 [1], grad_input [B,12,H,W], grad_scenes [B,S,9])"""
    import torch
    lib = native._load()
    B, S, H = c["B"], c["S"], c["H"]
    x, ph, sc = fc.Guarded(c["maps"], dev, shift), fc.Guarded(c["photos"], dev, shift), fc.Guarded(c["scenes"], dev, shift)
    g, gs = fc.Guarded(np.zeros_like(c["maps"]), dev, shift), fc.Guarded(np.full_like(c["scenes"], 7.0), dev, shift)
    _, wptr, planes = _weights(c, dev, shift)
    loss = torch.full((1,), -1.0, device=dev)
    ws = scratch(lib, dev, c)
    xr = native.xrow(dev, H)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = getattr(lib, SCENE_GRAD_ENTRY)(x.ptr(), ph.ptr(), wptr, planes, sc.ptr(), xr.data_ptr(), ctypes.c_float(EPS),
                                        loss.data_ptr(), g.ptr(), gs.ptr(), ws.data_ptr(), ws.numel() * 8, B, S, H, H, st)
    assert rc == 0, lib.svbrdf_last_error()
    torch.cuda.synchronize(dev)
    assert not ws.any().item()
    return loss.cpu().numpy(), g.get()[0], gs.get()[0]


def abi_joint(native, dev, c, t=None, bounds=None, want_grad=True, shift=0, lr=fc.LR, beta1=fc.BETA1, beta2=fc.BETA2,
              adam_eps=fc.ADAM_EPS, ws=None):
    """svbrdf_photo_fit_adam_step_scene_grad on the case (fc.call_fit_entry), grad_scenes between canaries too -> dict: loss
    [1], grad (or None), grad_scenes, x, m, v after the step, `inputs_intact`, `canaries_intact`, `launches`, `scratch_zero`"""
    outs = (("loss", np.full(1, -1.0, np.float32)), ("grad", np.full_like(c["maps"], 7.0) if want_grad else None),
            ("grad_scenes", np.full_like(c["scenes"], 7.0)))
    ws = scratch(native._load(), dev, c) if ws is None else ws
    return fc.call_fit_entry(native, dev, c, JOINT_ENTRY, (c["t"] if t is None else t,), outs, ws, bounds, shift, lr, beta1,
                             beta2, adam_eps)


# ------------------------------------------------------------------------------------------------ the speed measurement

def measure_joint_fit(dev, native, sets=6, n=40, rounds=3, pose_lr=2e-3):
    """-> dict of medians (us per step) at the configuration-2 shape, B = 8, 256 x 256, S = 9, per-photo weights, device
    table, `sets` rotating batches, one process, the legs alternating round by round (photo_checks.timed_legs):

        joint_us          PhotoFit.step with a table leaf (ONE launch of svbrdf_photo_fit_adam_step_scene_grad), its
                          backward() and the small Adam on the table
        scene_grad_us     the scene-gradient loss launch alone on the same data (svbrdf_photo_loss_scene_grad_fwd_bwd)
        composed_us       PhotoLoss with the table leaf forward + backward, one torch.optim.Adam over maps and table (the
                          stock default), clamp_
        composed_fused_us the same with torch.optim.Adam(fused=True)
    """
    import torch
    from svbrdf_estimation_amd import fitting
    lib = native._load()
    B, H, S, table, starts, photos, weights = fc.fit_workload(dev, native, sets)
    bounds = torch.from_numpy(fc.BOUNDS_FIT)
    fits = [fitting.PhotoFit(a.clone(), lr=fc.LR, bounds=bounds) for a in starts]
    leaves = [table.clone().requires_grad_(True) for _ in range(sets)]
    pose_opts = [torch.optim.Adam([t], lr=pose_lr) for t in leaves]
    grads = [torch.empty_like(a) for a in starts]
    grad_s = torch.empty_like(table)
    xr = native.xrow(dev, H)
    ws = torch.zeros(getattr(lib, WORKSPACE_BYTES)(B, S, H, H) // 8, dtype=torch.int64, device=dev)
    loss = torch.empty(1, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def joint(i):
        k = i % sets
        pose_opts[k].zero_grad(set_to_none=True)
        fits[k].step(photos[k], leaves[k], weights[k]).backward()
        pose_opts[k].step()

    def scene_grad(i):
        k = i % sets
        rc = getattr(lib, SCENE_GRAD_ENTRY)(starts[k].data_ptr(), photos[k].data_ptr(), weights[k].data_ptr(), S, table.data_ptr(),
                                            xr.data_ptr(), ctypes.c_float(EPS), loss.data_ptr(), grads[k].data_ptr(),
                                            grad_s.data_ptr(), ws.data_ptr(), ws.numel() * 8, B, S, H, H, st)
        assert rc == 0, lib.svbrdf_last_error()

    legs = (("joint_us", joint), ("scene_grad_us", scene_grad),
            ("composed_us", fc.composed_fit_leg(starts, photos, table, weights, pose_lr)),
            ("composed_fused_us", fc.composed_fit_leg(starts, photos, table, weights, pose_lr, fused=True)))
    out, res = photo_checks.timed_legs(legs, n, rounds, photo_checks.spinning_wave(native, dev), dev)
    out.update(rounds=res, device=torch.cuda.get_device_name(dev), steps_per_round=n, sets=sets)
    out["joint_over_scene_grad"] = out["joint_us"] / out["scene_grad_us"]
    out["joint_over_composed"] = out["joint_us"] / min(out["composed_us"], out["composed_fused_us"])
    return out
