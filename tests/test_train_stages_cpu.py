"""train.py's stage helpers on their own: the convolution-flag calibration schedule, the DDP probe's schedule and report,
the per-rank record.  No GPU, no process group and no training run: timings, the MAX over ranks and the gather are
injected."""
import pytest
import torch

import train

cudnn = torch.backends.cudnn


@pytest.fixture
def reference_flags():
    """the flags as utils.enable_deterministic_random_engine leaves them; whatever the test does to them is undone"""
    saved = cudnn.deterministic, cudnn.benchmark
    cudnn.deterministic, cudnn.benchmark = True, False
    yield
    cudnn.deterministic, cudnn.benchmark = saved


def _drive(mode, timings=(), max_over_ranks=None, on_gpu=True, steps=6):
    """ConvFlags over `steps` steps as train_steps calls it -> the chooser, per step cudnn.deterministic (during the forward,
    during the backward, after the optimizer), and the steps at which a stopwatch was started"""
    queue, timed, now = list(timings), [], [None]

    def stopwatch():
        timed.append(now[0])
        return lambda: queue.pop(0)
    conv = train.ConvFlags(mode, on_gpu, max_over_ranks, stopwatch)
    seen = []
    for step in range(steps):
        now[0] = step
        conv.before_forward(step)
        forward = cudnn.deterministic
        conv.after_forward()
        backward = cudnn.deterministic
        conv.after_optimizer()
        seen.append((forward, backward, cudnn.deterministic))
    return conv, seen, timed


@pytest.mark.parametrize("mode,flag,benchmark", [("reference", True, False), ("fast", False, False), ("autotune", False, True)])
def test_fixed_conv_modes_set_the_flags_once_and_never_toggle(reference_flags, mode, flag, benchmark):
    conv, seen, timed = _drive(mode)
    assert seen == [(flag, flag, flag)] * 6 and cudnn.benchmark is benchmark
    assert timed == [] and conv.calib_steps == 0 and conv.report() is None and conv.mode == mode


def test_hybrid_runs_forward_under_reference_flags_and_backward_under_immediate_mode(reference_flags):
    conv, seen, timed = _drive("hybrid")
    assert seen == [(True, False, True)] * 6 and cudnn.benchmark is False
    assert timed == [] and conv.calib_steps == 0 and conv.report() is None


@pytest.mark.parametrize("mode", ["hybrid", "auto"])
def test_hybrid_and_auto_leave_the_flags_alone_without_a_gpu(reference_flags, mode):
    conv, seen, timed = _drive(mode, on_gpu=False)
    assert seen == [(True, True, True)] * 6 and timed == [] and conv.calib_steps == 0 and conv.report() is None


@pytest.mark.parametrize("t_ref,t_imm,keeps_reference", [(5.0, 7.0, True), (7.0, 5.0, False), (5.0, 5.0, True)])
def test_auto_calibration_schedule_and_choice(reference_flags, t_ref, t_imm, keeps_reference):
    conv, seen, timed = _drive("auto", [t_ref, t_imm])
    assert conv.calib_steps == 4 and timed == [1, 3]                  # the second step of each pair is the timed one
    assert [f for f, _, _ in seen[:4]] == [True, True, False, False]    # steps 0-1 reference flags, 2-3 immediate mode
    assert [f for f, _, _ in seen[4:]] == [keeps_reference] * 2         # from step 4 on: reference exactly when t_ref <= t_imm
    assert all((b, after) == (False, True) for _, b, after in seen)     # backward immediate; reference again after the optimizer
    assert conv.report() == {"chosen": "reference flags" if keeps_reference else "immediate mode",
                             "calibration_ms": {"reference flags": t_ref, "immediate mode": t_imm}}


def test_auto_choice_follows_the_max_over_ranks(reference_flags):
    """this rank alone would keep the reference's flags (5 <= 7); the other rank's 9 ms under them decides for the job"""
    other, calls = [9.0, 6.0], []

    def max_over_ranks(values):
        calls.append(list(values))
        return [max(a, b) for a, b in zip(values, other)]
    conv, seen, _ = _drive("auto", [5.0, 7.0], max_over_ranks)
    assert calls == [[5.0, 7.0]]                                        # one reduce, at step 4: reference first
    assert [f for f, _, _ in seen] == [True, True, False, False, False, False]
    assert conv.report() == {"chosen": "immediate mode", "calibration_ms": {"reference flags": 9.0, "immediate mode": 7.0}}


def test_probe_schedule():
    k = 5
    probe = train.DdpProbe(True, k)
    assert probe.steps == 8 and [s for s in range(k + 12) if probe.probing(s)] == list(range(k, k + 8))
    assert all(probe.synced(s) for s in range(k))                         # training steps always synchronise
    assert [probe.synced(k + o) for o in range(8)] == [True, False] * 4   # odd offsets run under no_sync
    off = train.DdpProbe(False, k)
    assert off.steps == 0 and not any(off.probing(s) for s in range(k + 12)) and all(off.synced(s) for s in range(k + 12))
    assert off.start(k) is None and off.backward_ms() == {"with_allreduce": None, "no_sync": None}


def test_probe_discards_the_first_pair_and_reports_three_samples_of_each_kind():
    k = 3
    probe = train.DdpProbe(True, k)
    for o in range(8):
        if o < 2:
            probe.record(k + o, 1000.0, [1.0, 100.0])                     # offsets 0 and 1: warm-up, must leave no trace
        else:
            probe.record(k + o, 10.0 + o, [2.0, 2.0] if o % 2 == 0 else [2.0, 3.0])
    rep = probe.report(world=2, on_gpu=False)
    assert rep["samples_each"] == 3 and len(probe.ms[False]) == 3
    assert rep["backward_ms_with_allreduce"] == 14.0 and rep["backward_ms_no_sync"] == 15.0
    assert probe.backward_ms() == {"with_allreduce": 14.0, "no_sync": 15.0}
    assert rep["grad_checksum_spread_over_ranks_synced"] == 0.0
    assert rep["grad_checksum_spread_over_ranks_no_sync"] == pytest.approx(1.0 / 3.0, rel=1e-15)
    assert rep["no_sync_left_gradients_rank_local"] is True and "the host clock around loss.backward()" in rep["note"]
    assert list(rep) == ["backward_ms_with_allreduce", "backward_ms_no_sync", "samples_each",
                         "grad_checksum_spread_over_ranks_synced", "grad_checksum_spread_over_ranks_no_sync",
                         "no_sync_left_gradients_rank_local", "note"]
    assert probe.report(world=1, on_gpu=True)["no_sync_left_gradients_rank_local"] is None
    assert "HIP events around loss.backward()" in probe.report(world=1, on_gpu=True)["note"]


def test_probe_checksum_spread_and_the_1e_9_rule():
    spread = train.DdpProbe.spread
    assert spread([]) is None and spread([[1.0, 1.0]]) == 0.0
    assert spread([[1.0, 1.0], [4.0, 5.0], [10.0, 9.0]]) == pytest.approx(0.2, rel=1e-15)     # the largest of 0, 0.2, 0.1

    def verdict(synced, no_sync):
        probe = train.DdpProbe(True, 0)
        for o in range(2, 8):
            probe.record(o, 1.0, [1.0, 1.0 + (synced if o % 2 == 0 else no_sync)])
        return probe.report(world=2, on_gpu=False)["no_sync_left_gradients_rank_local"]
    assert verdict(0.0, 1e-6) is True
    assert verdict(1e-8, 1e-6) is False               # a synchronised step whose ranks disagree
    assert verdict(0.0, 1e-10) is False               # a no_sync step whose ranks agree: the all-reduce ran after all


def test_probe_times_the_backward_and_gathers_the_first_gradient_checksum():
    k = 4
    net = torch.nn.Linear(2, 1)
    net.weight.grad = torch.tensor([[1.5, -2.5]])
    probe = train.DdpProbe(True, k, gather=lambda mine: [mine, 2 * mine], stopwatch=lambda: (lambda: 42.0))
    assert probe.start(k - 1) is None
    probe.finish(k + 2, probe.start(k + 2), net)
    assert probe.ms == {True: [42.0], False: []} and probe.sums == {True: [[4.0, 8.0]], False: []}


def test_per_rank_record_single_and_gathered_forms():
    place = {"cpus": "0-3", "n_cpus": 4, "numa_node": None, "source": "unbound: --device cpu", "bound": False}
    single = train.per_rank_table([train.rank_record(place, 2.0)], batch=4, steps=10)
    assert single == {"elapsed_s": [2.0], "cpus": ["0-3"], "numa_node": [None], "cpu_binding": ["unbound: --device cpu"],
                      "pci_crosscheck": [None], "ms_per_step": [200.0], "patches_per_s": [20.0]}
    assert list(single) == ["elapsed_s", "cpus", "numa_node", "cpu_binding", "pci_crosscheck", "ms_per_step", "patches_per_s"]
    bound = dict(place, cpus="8-15", numa_node=1, source="sysfs", pci_crosscheck="match")
    ms = {"with_allreduce": 14.0, "no_sync": None}
    gathered = train.per_rank_table([train.rank_record(place, 2.0, ms), train.rank_record(bound, 4.0, ms)], batch=4, steps=10)
    assert list(gathered) == ["elapsed_s", "cpus", "numa_node", "cpu_binding", "pci_crosscheck", "backward_ms",
                              "ms_per_step", "patches_per_s"]
    assert gathered["elapsed_s"] == [2.0, 4.0] and gathered["patches_per_s"] == [20.0, 10.0] and gathered["numa_node"] == [None, 1]
    assert gathered["pci_crosscheck"] == [None, "match"] and gathered["backward_ms"] == [ms, ms]
