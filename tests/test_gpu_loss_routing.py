"""Which C entry point the ctypes binding reaches for each form of a fused-loss call, and what every such call must leave
behind: one launch, a finite loss, zeroed scratch, one begin/end pair for the launch hook.  4 x 4 pixels and one scene are
the smallest shapes at which a wrong route, a lost hook or a missing ``zero_`` shows; 289 rows is one more than a table
that rides in the launch's argument block, so a host table of that size is uploaded and reaches the device entry.  The
weighted photo rows ({"weights": P}: P weight planes per item, uniform in (0, 1) from a fixed seed) repeat the unweighted
ones: a wrong kernel pick for (gradient, head, weighted) shows as a wrong entry, a non-finite loss or a wrong gradient shape.
The exposure, scene-gradient and photo-gradient rows ({"exposure": S}: [1,S,3] gains in (0.5, 2) from a fixed seed, asked for
their gradient too) have no by-value form: a host table, however small, is uploaded and reaches the same entry as a device
table, with or without weights, and the third result has its documented shape."""
import numpy as np
import pytest
import torch

import head_checks
import synth

pytestmark = pytest.mark.gpu

H = 4
# (call, input channels, scenes on the host, S, options) -> entry
ROUTES = [
    ("rendering_loss", 12, True, 1, {"l1_weight": 0.0}, "svbrdf_mixed_loss_fwd_bwd_host_scenes"),
    ("rendering_loss", 12, True, 1, {"l1_weight": 0.1}, "svbrdf_mixed_loss_fwd_bwd_host_scenes"),
    ("rendering_loss", 9, True, 1, {"head": True}, "svbrdf_head_loss_fwd_bwd_host_scenes"),
    ("rendering_loss", 12, False, 1, {"l1_weight": 0.0}, "svbrdf_rendering_loss_fwd_bwd"),
    ("rendering_loss", 12, False, 1, {"l1_weight": 0.1}, "svbrdf_mixed_loss_fwd_bwd"),
    ("rendering_loss", 9, True, 289, {"head": True}, "svbrdf_head_loss_fwd_bwd"),
    ("photo_loss", 12, True, 1, {}, "svbrdf_photo_loss_fwd_bwd_host_scenes"),
    ("photo_loss", 12, False, 1, {}, "svbrdf_photo_loss_fwd_bwd"),
    ("photo_loss", 9, True, 1, {"head": True}, "svbrdf_head_photo_loss_fwd_bwd_host_scenes"),
    ("photo_loss", 9, False, 1, {"head": True}, "svbrdf_head_photo_loss_fwd_bwd"),
    ("photo_loss", 12, True, 289, {}, "svbrdf_photo_loss_fwd_bwd"),
    ("photo_loss", 12, True, 1, {"weights": 1}, "svbrdf_photo_loss_weighted_fwd_bwd_host_scenes"),
    ("photo_loss", 12, False, 1, {"weights": 1}, "svbrdf_photo_loss_weighted_fwd_bwd"),
    ("photo_loss", 9, True, 1, {"head": True, "weights": 1}, "svbrdf_head_photo_loss_weighted_fwd_bwd_host_scenes"),
    ("photo_loss", 9, False, 1, {"head": True, "weights": 1}, "svbrdf_head_photo_loss_weighted_fwd_bwd"),
    ("photo_loss", 12, True, 289, {"weights": 289}, "svbrdf_photo_loss_weighted_fwd_bwd"),
]
# the modes with a third result, (options, entry suffix): each for maps and head, on a device table unweighted and weighted
# and on a host table of S = 1
for _options, _suffix in (({"exposure": 1}, "exposure"), ({"want_scene_grad": True}, "scene_grad"),
                          ({"want_photo_grad": True}, "photo_grad")):
    for _channels, _head, _stem in ((12, {}, "svbrdf_photo_loss_"), (9, {"head": True}, "svbrdf_head_photo_loss_")):
        for _on_host, _weights in ((False, {}), (False, {"weights": 1}), (True, {})):
            ROUTES.append(("photo_loss", _channels, _on_host, 1, dict(_options, **_head, **_weights), _stem + _suffix + "_fwd_bwd"))


class _Recorder:
    """stands in for the loaded library: every svbrdf_* function looked up on it is called through, its name noted"""

    def __init__(self, lib):
        self._lib, self.called = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("svbrdf_"):
            return fn

        def call(*args):
            self.called.append(name)
            return fn(*args)
        return call


@pytest.fixture(scope="module")
def inputs():
    """device tensors shared by every case (never written): maps, encoded head output, target maps, scene tables and
    clamped photos of other maps for S = 1 and S = 289, weights [1,P,4,4] for P = 1 and P = 289, exposure [1,S,3] for S = 1"""
    from svbrdf_estimation_amd import _native, environment
    assert torch.cuda.is_available(), "GPU tests need an MI355X (select CPU tests with -m 'not gpu')"
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    out = {12: torch.from_numpy(synth.make_maps(1, 1, H)).to(dev),
           9: torch.from_numpy(head_checks.interior(2, 1, H)).to(dev),
           "target": torch.from_numpy(synth.make_maps(3, 1, H)).to(dev)}
    other = torch.from_numpy(synth.make_maps(4, 1, H)).to(dev)
    for S in (1, 289):
        table = environment.scene_table(S // 2, S - S // 2).unsqueeze(0).contiguous()
        assert tuple(table.shape) == (1, S, 9) and table.dtype == torch.float32
        out["scenes", S] = table
        out["photos", S] = _native.render_fwd(other, table).clamp(0.0, 1.0)
        out["weights", S] = torch.from_numpy(synth.uniform01(5 + S, (1, S, H, H))).to(dev)
        assert 0.0 < out["weights", S].min() and out["weights", S].max() < 1.0
    out["exposure", 1] = (0.5 + 1.5 * torch.from_numpy(synth.uniform01(11, (1, 1, 3)))).to(dev)
    assert 0.5 < out["exposure", 1].min() and out["exposure", 1].max() < 2.0
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("want_grad", [True, False], ids=["grad", "forward_only"])
@pytest.mark.parametrize("route", ROUTES, ids=["%02d_%s%s" % (i + 1, r[-1][len("svbrdf_"):], "_from_host" * (i >= 16 and r[2]))
                                                for i, r in enumerate(ROUTES)])
def test_fused_loss_call_reaches_its_entry(route, want_grad, inputs, monkeypatch):
    from svbrdf_estimation_amd import _native
    call, channels, on_host, S, options, entry = route
    assert 288 == _native.host_scenes_max_rows()
    x = inputs[channels]
    other = inputs["photos", S] if call == "photo_loss" else inputs["target"]
    scenes = inputs["scenes", S] if on_host else inputs["scenes", S].to(x.device)
    if "weights" in options:
        options = dict(options, weights=inputs["weights", options["weights"]])
    if "exposure" in options:
        options = dict(options, exposure=inputs["exposure", options["exposure"]], want_exposure_grad=True)
    _native.xrow(x.device, H)           # (the cached x row: its first use is no part of the call under test)
    rec = _Recorder(_native._load())
    monkeypatch.setattr(_native, "_load", lambda: rec)
    uploads = []
    upload = _native.upload_scene_table
    monkeypatch.setattr(_native, "upload_scene_table", lambda *a: (uploads.append(1), upload(*a))[1])
    seen = []
    _native.set_launch_hook(seen.append)
    try:
        before = _native.launch_count()
        loss, grad, *rest = getattr(_native, call)(x, other, scenes, want_grad=want_grad, **options)
        after = _native.launch_count()
    finally:
        _native.set_launch_hook(None)
    torch.cuda.synchronize()
    reached = [n for n in rec.called if "_fwd_bwd" in n]
    print("%s -> %s, launches %d, loss %r, hook %r" % (route[:5], reached, after - before, loss.item(), seen))
    assert reached == [entry]
    # a host table goes by value where the entry has that form, else it is uploaded: once
    assert len(uploads) == (1 if on_host and not entry.endswith("_host_scenes") else 0)
    assert after - before == 1
    assert np.isfinite(loss.item())
    if want_grad:
        assert grad.shape == x.shape and torch.isfinite(grad).all()
    else:
        assert grad is None
    third = {"exposure": (1, S, 3), "want_scene_grad": (1, S, 9), "want_photo_grad": tuple(other.shape)}
    shapes = [third[k] for k in third if k in options]
    assert [tuple(t.shape) for t in rest] == shapes and all(torch.isfinite(t).all() for t in rest)
    assert seen == ["begin", "end"]
    assert _native._workspace_cache and all(not ws.any().item() for ws in _native._workspace_cache.values())
