"""GPU: K3, the fused rendering loss, against the REFERENCE's own loss and gradient at the BASELINE sizes.

tests/golden/g3_loss_256_b8.npz is config 2 (B=8, 256x256, 3 + 6 scenes: the shape bench.py times) with RenderingLoss
and MixedLoss; g3_loss_512_s32.npz is config 5's per-item shape (512x512, 11 + 21 scenes, B=2) with MixedLoss.  Both
hold the reference's loss, its gradient on a stride lattice, per-plane sums of g and |g| and the plane's max|g|.  Each
is checked through the module path bench.py times (loss module under the fixture's torch seed, then backward through the
autograd engine) and through the C ABI with the recorded scene table, under the bounds of tests/tolerances.py: the fp64
widening and the exact tie allowance of the C oracle.  The whole batch is compared with the oracle as well."""
import numpy as np
import pytest
import torch

import synth
from tolerances import MAX_WIDENED_GRAD, assert_grad_close, assert_loss_at_size, assert_loss_close

pytestmark = pytest.mark.gpu

FIXTURES = ["g3_loss_256_b8.npz", "g3_loss_512_s32.npz"]
REFERENCE_LOSS_RTOL = 2e-6      # as for every other comparison of a K3 loss with the reference's float32 loss


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X (select CPU tests with -m 'not gpu')"
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _tags(g):
    return [(t, w) for t, w in (("render", 0.0), ("mixed", 0.1)) if t + "_loss" in g.files]


def _oracle_side(oracle, inp, tgt, table, w):
    oracle.set_threads(oracle.max_threads())
    _, g32 = oracle.mixed_loss(inp, tgt, table, w)
    _, g64 = oracle.mixed_loss(inp, tgt, table, w, f64=True)
    return g32, g64


def _whole_batch_vs_oracle(grad, g32, g64, tie, allow, table, what):
    B, _, H, W = grad.shape
    assert_grad_close(grad, g32, what + " vs oracle, whole batch", f64=g64, tie_map=tie, tie_allowance=allow,
                      max_ties=max(8, int(2e-6 * B * H * W * table.shape[1] * 3)),
                      max_widened=max(MAX_WIDENED_GRAD, int(2e-6 * grad.size)))


def _module_run(g, tag, inp, tgt, dev, table=None):
    """the loss module under the fixture's torch seed, backward through the engine.  Returns loss, gradient and the
    scene tables the Python sampler handed to the forward (none where the native host path draws them itself);
    `table` replaces what the sampler draws."""
    from svbrdf_estimation_amd import losses, renderers
    if tag == "render":
        fn = rl = losses.RenderingLoss(renderers.LocalRenderer())
    else:
        fn = losses.MixedLoss(renderers.LocalRenderer())
        rl = fn.rendering_loss
    rl.random_configuration_count, rl.specular_configuration_count = int(g["n_random"]), int(g["n_specular"])
    assert rl.uses_fused_kernel()
    drawn, sample = [], rl.sample_scene_table

    def recording(batch_size):
        t = sample(batch_size) if table is None else torch.from_numpy(table.copy())
        drawn.append(t.detach().cpu().numpy().copy())
        return t
    rl.sample_scene_table = recording
    x = _t(inp, dev).requires_grad_(True)
    torch.manual_seed(int(g["rng_seed"]))
    loss = fn(x, _t(tgt, dev))
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), x.grad.detach().cpu().numpy(), drawn


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", FIXTURES)
def test_loss_module_path_against_the_reference_at_size(dev, oracle, golden, name):
    """The module path: native host extension (as bench.py runs it) and Python + ctypes, bitwise equal.  The scene table
    it draws is bit for bit the reference's draw order (per-item environment.scene_table) on this machine, and the
    fixture's table up to the last bit of the CPU math library (torch's CPU trigonometry / sqrt take a code path that
    depends on the host CPU; the fixture comes from the build machine, cf. g5_scene_sampler).  Loss and gradient
    against the reference with the fixture's table given to the module bit for bit, and against the oracle with both
    tables."""
    from svbrdf_estimation_amd import _hostext, _native, environment
    g = golden(name)
    inp, tgt = synth.loss_fixture_maps(g)
    table = g["scenes"]
    B = inp.shape[0]
    torch.manual_seed(int(g["rng_seed"]))
    per_item = torch.stack([environment.scene_table(int(g["n_random"]), int(g["n_specular"])) for _ in range(B)]).numpy()
    ulps = np.abs(per_item.view(np.int32).astype(np.int64) - table.view(np.int32).astype(np.int64))
    print("[at size] %s: scene table drawn here differs from the fixture's in %d of %d entries, by at most %d ULP" % (
        name, int((ulps > 0).sum()), table.size, int(ulps.max())))
    np.testing.assert_allclose(per_item, table, rtol=1e-6, atol=1e-7)      # a few ULP through exp / trigonometry
    tie, allow = oracle.loss_tie_map(inp, tgt, table), oracle.loss_tie_allowance(inp, tgt, table)
    for tag, w in _tags(g):
        try:
            _hostext.set_enabled(True)
            loss, grad, _ = _module_run(g, tag, inp, tgt, dev)
            _hostext.set_enabled(False)
            loss_py, grad_py, drawn = _module_run(g, tag, inp, tgt, dev)
            loss_fx, grad_fx, given = _module_run(g, tag, inp, tgt, dev, table=table)
        finally:
            _hostext.set_enabled(True)
        what = "%s %s module" % (name, tag)
        assert len(drawn) == 1 and _same_bits(drawn[0], per_item), what + ": not the reference's draw order"
        assert loss == loss_py and np.array_equal(grad, grad_py), what + ": the two host paths differ"
        assert len(given) == 1 and _same_bits(given[0], table)
        if _same_bits(per_item, table):
            assert loss_fx == loss and np.array_equal(grad_fx, grad)
        # as drawn: the loss against the reference, everything against the oracle with the same scenes
        assert_loss_close(loss, g[tag + "_loss"], what + " as drawn vs reference", rtol=REFERENCE_LOSS_RTOL)
        l_nat, g_nat = _native.rendering_loss(_t(inp, dev), _t(tgt, dev), torch.from_numpy(per_item), l1_weight=w)
        assert l_nat.item() == loss and np.array_equal(g_nat.cpu().numpy(), grad), what + ": module != C ABI"
        if not _same_bits(per_item, table):
            d32, d64 = _oracle_side(oracle, inp, tgt, per_item, w)
            _whole_batch_vs_oracle(grad, d32, d64, oracle.loss_tie_map(inp, tgt, per_item),
                                   oracle.loss_tie_allowance(inp, tgt, per_item), per_item, what + " as drawn")
        # the fixture's scenes: against the reference's loss, gradient lattice and plane sums, and the oracle
        g32, g64 = _oracle_side(oracle, inp, tgt, table, w)
        assert_loss_at_size(g, tag, loss_fx, grad_fx, g64, tie, allow, what, loss_rtol=REFERENCE_LOSS_RTOL)
        _whole_batch_vs_oracle(grad_fx, g32, g64, tie, allow, table, what)


@pytest.mark.parametrize("name", FIXTURES)
def test_native_rendering_loss_against_the_reference_at_size(dev, oracle, golden, name):
    from svbrdf_estimation_amd import _native
    g = golden(name)
    inp, tgt = synth.loss_fixture_maps(g)
    table = g["scenes"]
    d_in, d_tg, d_sc = _t(inp, dev), _t(tgt, dev), _t(table, dev)
    tie, allow = oracle.loss_tie_map(inp, tgt, table), oracle.loss_tie_allowance(inp, tgt, table)
    for tag, w in _tags(g):
        loss, grad = _native.rendering_loss(d_in, d_tg, d_sc, l1_weight=w)
        loss_fwd, none = _native.rendering_loss(d_in, d_tg, d_sc, l1_weight=w, want_grad=False)
        assert none is None and loss_fwd.item() == loss.item(), "%s %s: forward-only loss differs" % (name, tag)
        grad = grad.cpu().numpy()
        g32, g64 = _oracle_side(oracle, inp, tgt, table, w)
        what = "%s %s native" % (name, tag)
        assert_loss_at_size(g, tag, loss.item(), grad, g64, tie, allow, what, loss_rtol=REFERENCE_LOSS_RTOL)
        ref_l, _ = oracle.mixed_loss(inp, tgt, table, w, want_grad=False)
        assert_loss_close(loss.item(), ref_l, what + " vs oracle")
        _whole_batch_vs_oracle(grad, g32, g64, tie, allow, table, what)
