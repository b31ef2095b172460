"""The straight-line code at the two ends of a fused-loss wave, on the GPU, at small shapes.

The by-value-table kernels fetch the launch's scalars once at wave entry, request render 0's scene row in front of the
plane loads, and every fused-loss kernel sums a wave's partial loss with lane swaps and DPP rotations instead of
ds_bpermute (rendering_loss_body, wave_sum_k3 in svbrdf_device.h).  The device-table kernels keep the ordinary
prologue, so the two forms check each other: same inputs, same bits.  Against the oracle and the reference fixture the
bounds are the suite's own (tests/tolerances.py).

Shapes: 7x7 with S = 5 (a ragged last workgroup, no power-of-two width, the reference fixture), 16x16 with S = 1 (the
hoisted row is the only row of the launch), 16x16 with S = 2 (the second row is the loop's first own fetch), 65 batch
items of 16x16 (65 workgroups on 64 slots: slot 0 is completed by its second arrival), and a NaN normal with S = 1 (the
poison travels in the pixel's x coordinate and has to reach render 0, whose row no longer comes from the loop's load).
"""
import numpy as np
import pytest
import torch

import synth
from tolerances import assert_grad_close, assert_loss_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X (select CPU tests with -m 'not gpu')"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def native():
    from svbrdf_estimation_amd import _native
    _native._load()
    return _native


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _both_forms(native, dev, inp, tgt, table, **kw):
    """the loss by-value (host table) and through the device table; -> (loss, grad) of the by-value form after checking
    that the device-table form returned the same bits"""
    assert table.shape[0] * table.shape[1] <= native.host_scenes_max_rows()
    d_in, d_tg = _t(inp, dev), _t(tgt, dev)
    host_table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32))
    l_val, g_val = native.rendering_loss(d_in, d_tg, host_table, **kw)
    l_dev, g_dev = native.rendering_loss(d_in, d_tg, host_table.to(dev), **kw)
    assert np.array_equal(_bits(l_val), _bits(l_dev)), (l_val.item(), l_dev.item())
    assert np.array_equal(_bits(g_val), _bits(g_dev))
    # forward only (LDS-staged rows, the same wave sum): the same loss bits
    l_fwd, none = native.rendering_loss(d_in, d_tg, host_table, want_grad=False, **kw)
    assert none is None and np.array_equal(_bits(l_fwd), _bits(l_val)), (l_fwd.item(), l_val.item())
    return l_val, g_val


def _table(seed, B, n_random, n_specular):
    from svbrdf_estimation_amd import environment
    torch.manual_seed(seed)
    return torch.stack([environment.scene_table(n_random, n_specular) for _ in range(B)]).numpy()


def test_reference_fixture_7x7_five_scenes(dev, native, oracle, golden):
    g = golden("g3_loss_7_s5.npz")
    loss, grad = _both_forms(native, dev, g["input"], g["target"], g["scenes"])
    ref_l, ref_g = oracle.rendering_loss(g["input"], g["target"], g["scenes"])
    _, g64 = oracle.rendering_loss(g["input"], g["target"], g["scenes"], f64=True)
    assert_loss_close(loss.item(), ref_l, "7x7 s5 vs oracle")
    assert_loss_close(loss.item(), g["loss"], "7x7 s5 vs reference", rtol=2e-6)
    assert_grad_close(grad.cpu().numpy(), ref_g, "7x7 s5 grad vs oracle", f64=g64)
    assert_grad_close(grad.cpu().numpy(), g["grad_input"], "7x7 s5 grad vs reference", f64=g64)
    # the mixed loss of the same fixture (the L1 kernels share the prologue and the wave sum)
    mixed, mgrad = _both_forms(native, dev, g["input"], g["target"], g["scenes"], l1_weight=0.1, eps_l1=0.01)
    _, m64 = oracle.mixed_loss(g["input"], g["target"], g["scenes"], 0.1, f64=True)
    assert_loss_close(mixed.item(), g["mixed_loss"], "7x7 s5 mixed vs reference", rtol=2e-6)
    assert_grad_close(mgrad.cpu().numpy(), g["mixed_grad"], "7x7 s5 mixed grad vs reference", f64=m64)


@pytest.mark.parametrize("B,n_random,n_specular", [(2, 0, 1), (2, 1, 1), (65, 1, 1)],
                         ids=["16x16-S1", "16x16-S2", "65-workgroups"])
@pytest.mark.parametrize("tied", [True, False], ids=["tied", "untied"])
def test_small_shapes_both_forms_and_oracle(dev, native, oracle, B, n_random, n_specular, tied):
    H = 16
    inp = synth.make_maps(700 + B, B, H, tiled_roughness=tied)
    tgt = synth.make_maps(800 + B, B, H, tiled_roughness=tied)
    table = _table(30 + B + n_random, B, n_random, n_specular)
    what = "B=%d S=%d tied=%d" % (B, n_random + n_specular, tied)
    loss, grad = _both_forms(native, dev, inp, tgt, table)
    ref_l, ref_g = oracle.rendering_loss(inp, tgt, table)
    _, g64 = oracle.rendering_loss(inp, tgt, table, f64=True)
    assert_loss_close(loss.item(), ref_l, what)
    assert_grad_close(grad.cpu().numpy(), ref_g, what + " grad", f64=g64, tie_map=oracle.loss_tie_map(inp, tgt, table),
                      tie_allowance=oracle.loss_tie_allowance(inp, tgt, table))
    # run to run: the same bits, and the scratch words were left zeroed by the finisher
    again, grad2 = _both_forms(native, dev, inp, tgt, table)
    assert np.array_equal(_bits(again), _bits(loss)) and np.array_equal(_bits(grad2), _bits(grad))


def test_nan_normal_reaches_the_only_render(dev, native):
    B, H = 2, 16
    inp, tgt = synth.make_maps(901, B, H), synth.make_maps(902, B, H)
    table = _table(77, B, 0, 1)
    clean, clean_grad = _both_forms(native, dev, inp, tgt, table)
    assert np.isfinite(clean.item())
    bad = inp.copy()
    bad[1, 0, 9, 5] = np.nan       # normal x of one pixel in the second workgroup
    loss, grad = _both_forms(native, dev, bad, tgt, table)
    assert np.isnan(loss.item())
    assert torch.isnan(grad[1, :, 9, 5]).any().item()
    assert torch.isfinite(grad[0]).all().item()     # the other workgroup's pixels are untouched
    after, after_grad = _both_forms(native, dev, inp, tgt, table)       # nothing sticks
    assert np.array_equal(_bits(after), _bits(clean)) and np.array_equal(_bits(after_grad), _bits(clean_grad))
