"""Shared by tests/test_photo_fit_steps_cpu.py and tests/test_gpu_photo_fit_steps.py: several steps of a photo fit in one
launch (csrc/svbrdf_photo_fit.hip: k_fit_run*; svbrdf_photo_fit_adam_steps).  The oracle everywhere is THE SEQUENTIAL RUN:
n calls of svbrdf_photo_fit_adam_step (photo_fit_checks.abi_fit) with t = first_step + k, each fed with the result of the one
before; that step is itself pinned to the restatement and to float64 Adam by tests/test_gpu_photo_fit.py.  Every comparison
is bit for bit (photo_fit_checks.same_bits: a NaN compares as "both NaN").
"""
import ctypes

import numpy as np

import photo_fit_checks as fc
from photo_fit_checks import (BOUNDS_FIT, CASES, Guarded, abi_fit, bounds_array, case_inputs, library_scalars,  # noqa: F401
                              same_bits)

STEPS_ENTRY, STEPS_BYTES = "svbrdf_photo_fit_adam_steps", "svbrdf_photo_fit_steps_workspace_bytes"
MAX_STEPS = 64


def abi_steps(native, dev, c, n, first_step=None, bounds=None, shift=0, ws=None, lr=fc.LR, beta1=fc.BETA1, beta2=fc.BETA2,
              adam_eps=fc.ADAM_EPS):
    """svbrdf_photo_fit_adam_steps on the case `c` (maps, m, v, photos, scenes, weights; fc.call_fit_entry) -> dict: losses
    [n], x, m, v after the launch, `inputs_intact`, `canaries_intact`, `launches`, `scratch_zero` (all 65 n words)"""
    import torch
    lib = native._load()
    need = getattr(lib, STEPS_BYTES)(n, c["B"], c["S"], c["H"], c["H"])
    assert need == n * lib.svbrdf_rendering_loss_workspace_bytes(c["B"], c["S"], c["H"], c["H"]) == n * 65 * 8
    ws = torch.zeros(need // 8, dtype=torch.int64, device=dev) if ws is None else ws
    assert ws.numel() * 8 >= need
    return fc.call_fit_entry(native, dev, c, STEPS_ENTRY, (c["t"] if first_step is None else first_step, n),
                             (("losses", np.full(n, -1.0, np.float32)),), ws, bounds, shift, lr, beta1, beta2, adam_eps)


def sequential(native, dev, c, n, first_step=None, bounds=None, **hyper):
    """THE ORACLE: n single-step launches, each on the result of the one before.  -> list of n + 1 states
    dict(x, m, v, loss): entry k is the state BEFORE step k with the loss step k reported (entry n: loss None)"""
    first_step = c["t"] if first_step is None else first_step
    states, d = [], dict(c)
    for k in range(n):
        out = abi_fit(native, dev, d, t=first_step + k, bounds=bounds, want_grad=False, **hyper)
        assert out["launches"] == 1 and out["scratch_zero"] and out["canaries_intact"] and out["inputs_intact"]
        states.append(dict(x=d["maps"], m=d["m"], v=d["v"], loss=out["loss"]))
        d = dict(d, maps=out["x"], m=out["m"], v=out["v"])
    states.append(dict(x=d["maps"], m=d["m"], v=d["v"], loss=None))
    return states


def assert_same_run(out, states, n, what):
    """the launch's maps, state and n losses against the first n steps of a sequential run"""
    want = states[n]
    for key in ("x", "m", "v"):
        assert same_bits(out[key], want[key]), "%s: %s differs from the sequential run in %d values" % (
            what, key, fc.count_differing(out[key], want[key]))
    seq = np.concatenate([states[k]["loss"] for k in range(n)])
    assert same_bits(out["losses"], seq), "%s: losses %s, sequential %s" % (what, out["losses"], seq)


def assert_clean(out, what, launches=1):
    assert out["launches"] == launches, (what, out["launches"])
    assert out["scratch_zero"] and out["canaries_intact"] and out["inputs_intact"], (what, out["scratch_zero"],
                                                                                   out["canaries_intact"], out["inputs_intact"])


# ------------------------------------------------------------------------------------------------ the speed measurement

def measure_steps_against_single(dev, native, steps=16, sets=6, n=10, rounds=3):
    """-> dict of medians (us) at the configuration-2 shape of photo_fit_checks.measure_photo_fit -- B = 8, 256 x 256, S = 9,
    per-photo weights, device table, `sets` rotating data sets so that maps and state come from HBM -- one process, the two
    legs alternating round by round (photo_checks.timed_legs), each timed unit being `steps` Adam steps of one data set:

        run_us       ONE launch of svbrdf_photo_fit_adam_steps with n_steps = `steps`
        single_us    `steps` launches of svbrdf_photo_fit_adam_step, back to back on the stream
    """
    import torch
    import photo_checks
    lib = native._load()
    B, H, S, table, starts, photos, weights = fc.fit_workload(dev, native, sets)
    state = {leg: [(a.clone(), torch.zeros_like(a), torch.zeros_like(a)) for a in starts] for leg in ("run", "single")}
    keep, bptr = bounds_array(BOUNDS_FIT)
    xr = native.xrow(dev, H)
    ws = torch.zeros(65 * steps, dtype=torch.int64, device=dev)
    losses = torch.empty(steps, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    f = ctypes.c_float
    hyper = (f(fc.LR), f(fc.BETA1), f(fc.BETA2), f(fc.ADAM_EPS))
    run_fn, step_fn = getattr(lib, STEPS_ENTRY), getattr(lib, fc.STEP_ENTRY)

    def run(i):
        k = i % sets
        x, m, v = state["run"][k]
        rc = run_fn(x.data_ptr(), m.data_ptr(), v.data_ptr(), photos[k].data_ptr(), weights[k].data_ptr(), S, table.data_ptr(),
                    xr.data_ptr(), f(fc.EPS), bptr, *hyper, 1, steps, losses.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                    B, S, H, H, st)
        assert rc == 0, lib.svbrdf_last_error()

    def single(i):
        k = i % sets
        x, m, v = state["single"][k]
        for t in range(1, steps + 1):
            rc = step_fn(x.data_ptr(), m.data_ptr(), v.data_ptr(), photos[k].data_ptr(), weights[k].data_ptr(), S,
                         table.data_ptr(), xr.data_ptr(), f(fc.EPS), bptr, *hyper, t, losses.data_ptr(), None, ws.data_ptr(),
                         65 * 8, B, S, H, H, st)
            assert rc == 0, lib.svbrdf_last_error()

    out, res = photo_checks.timed_legs((("run_us", run), ("single_us", single)), n, rounds,
                                       photo_checks.spinning_wave(native, dev), dev)
    del keep
    assert not ws.any().item()
    out.update(rounds=res, device=torch.cuda.get_device_name(dev), steps=steps, units_per_round=n, sets=sets,
               ratio=out["run_us"] / out["single_us"], run_us_per_step=out["run_us"] / steps,
               single_us_per_step=out["single_us"] / steps)
    return out
