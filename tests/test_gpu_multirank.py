"""Rows (e) / (f4) on the ONE GPU a test box has: the code an N-GPU run executes, executed.

The reference is single-device (development/multiImage_pytorch/main.py:33-36); the multi-GPU layout here is one
process per GPU, batch sharded by rank, no data-path collective.  An 8-GPU node is the
driver's to run, so these tests make every branch of that layout run on one MI355X:

  * RCCL itself at world size 1 (``--force-dist``): ``init_process_group("nccl", device_id=...)``,
    ``barrier(device_ids=...)``, the MAX all-reduce of the elapsed time on a device tensor, the global-mean
    all-reduce, DDP's bucketed gradient all-reduce -- the branches ``bench.py`` / ``train.py`` take for N > 1;
  * two self-spawned ranks sharing the device (``--gpus 2 --backend gloo --share-device``): rank launch, rendezvous,
    barriers, per-rank scene streams, MAX over ranks, one JSON line -- with the HIP kernels running in both ranks;
  * DDP over two ranks with the fused MixedLoss: the averaged gradient of a fixed global batch equals the
    single-process gradient of the same batch.

Every script is started as a FRESH child process (never a re-exec of the pytest process, which has initialised the
GPU runtime).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.update(extra)
    return env


def _run(script, *argv, timeout=900, **extra_env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + [str(a) for a in argv], env=_clean_env(**extra_env),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "%s %s failed (%d):\n%s" % (script, argv, r.returncode, r.stderr[-3000:])
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.strip().startswith("{") and l.strip().endswith("}")]
    assert len(lines) == 1, "expected ONE JSON line, got %d:\n%s" % (len(lines), r.stdout[-2000:])
    return lines[0], r.stderr


def test_bench_rccl_process_group_of_one():
    """bench.py's N > 1 branches over RCCL (backend "nccl"), world size 1: bench.py:init_process_group(device_id),
    barrier(device_ids), all_reduce(MAX) of a device tensor, distributed.global_mean, all_gather, destroy"""
    line, _ = _run("bench.py", "--gpus", 1, "--force-dist", "--steps", 40, "--warmup", 10, "--settle-ms", 20,
                   "--no-cpu-baseline", "--no-secondary")
    assert line["process_group"].startswith("nccl") and line["ranks_seen"] == 1 and line["n_gpus"] == 1
    assert line["value"] > 1e4 and np.isfinite(line["loss"])
    assert line["per_rank"]["scene_seed"] == [313] and len(line["per_rank"]["elapsed_s"]) == 1
    assert abs(line["per_rank"]["last_loss"][0] - line["loss"]) <= 1e-6 * abs(line["loss"])
    print("bench.py over RCCL, world 1: %.0f patches/s" % line["value"])


def test_bench_two_self_spawned_ranks_share_the_device():
    """`python bench.py --gpus 2` as ONE plain process (how the driver calls it): it spawns its own two ranks; with
    --backend gloo --share-device both drive cuda:0, so the whole N-rank control flow runs with the kernels in it"""
    line, err = _run("bench.py", "--gpus", 2, "--backend", "gloo", "--share-device", "--steps", 50, "--warmup", 10,
                     "--settle-ms", 20, "--no-cpu-baseline", "--no-secondary")
    assert line["launch"] == "self-spawned" and line["ranks_seen"] == 2 and line["n_gpus"] == 2
    assert line["process_group"].startswith("gloo")
    assert line["value"] > 1e4 and line["config"]["global_batch"] == 16
    pr = line["per_rank"]
    assert pr["scene_seed"] == [313, 314]                                   # per-rank scene streams
    assert pr["last_loss"][0] != pr["last_loss"][1]                         # ... and per-rank batches
    assert all(np.isfinite(v) for v in pr["last_loss"])
    assert abs(0.5 * sum(pr["last_loss"]) - line["loss"]) <= 1e-6 * abs(line["loss"])     # global mean of the shard means
    assert line["ms_per_step"] * line["steps"] * 1e-3 >= max(pr["elapsed_s"]) * (1 - 1e-9)  # MAX over ranks
    # what the scaling judge reads on every N: aggregate and per-GPU value, each rank's own step time, and where each
    # rank runs -- pinned to the CPUs of its GPU's NUMA node before its first GPU call, the two ranks that share this
    # GPU's socket on disjoint halves of it (or both left unbound where the topology cannot be read)
    from svbrdf_estimation_amd import launch
    assert abs(line["per_gpu_value"] * 2 - line["value"]) <= 1e-9 * line["value"] and len(pr["ms_per_step"]) == 2
    assert all(abs(p - 8 * 50 / e) <= 1e-6 * p for p, e in zip(pr["patches_per_s"], pr["elapsed_s"]))
    cpus = [set(launch.parse_cpulist(c)) for c in pr["cpus"]]
    assert len(cpus) == 2 and all(cpus) and (cpus[0].isdisjoint(cpus[1]) or cpus[0] == cpus[1]), pr["cpus"]
    if pr["numa_node"][0] is not None:
        assert pr["numa_node"][0] == pr["numa_node"][1] and cpus[0].isdisjoint(cpus[1]), (pr["numa_node"], pr["cpus"])
    print("rank placement: %s" % list(zip(pr["cpus"], pr["cpu_binding"])))
    print("bench.py, two ranks on one device: %.0f patches/s aggregate; per-rank seconds %s" % (line["value"], pr["elapsed_s"]))
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "multirank_bench_share_device.json"), "w") as f:
        json.dump(line, f, indent=1)


def test_bench_eight_self_spawned_ranks_as_the_scaling_run_starts_it():
    """`python bench.py --gpus 8 --steps 20 --warmup 5` as ONE plain process -- the last command of the driver's scaling
    run -- on the one GPU a box has (gloo, every rank on cuda:0): eight fresh rank processes, eight scene streams, eight
    CPU slices of the GPU's socket (disjoint where the topology is readable), MAX over ranks, one JSON line."""
    line, _ = _run("bench.py", "--gpus", 8, "--backend", "gloo", "--share-device", "--steps", 20, "--warmup", 5,
                   "--settle-ms", 20, "--no-cpu-baseline", "--no-secondary", timeout=1500)
    assert line["launch"] == "self-spawned" and line["ranks_seen"] == 8 and line["n_gpus"] == 8
    pr = line["per_rank"]
    assert pr["scene_seed"] == list(range(313, 321)) and len(set(pr["last_loss"])) == 8
    assert len(pr["ms_per_step"]) == 8 and abs(line["per_gpu_value"] * 8 - line["value"]) <= 1e-9 * line["value"]
    assert line["ms_per_step"] * line["steps"] * 1e-3 >= max(pr["elapsed_s"]) * (1 - 1e-9)
    from svbrdf_estimation_amd import launch
    cpus = [set(launch.parse_cpulist(c)) for c in pr["cpus"]]
    if pr["numa_node"][0] is not None:
        assert len(set(pr["numa_node"])) == 1 and all(a.isdisjoint(b) for i, a in enumerate(cpus) for b in cpus[i + 1:]), pr["cpus"]
    print("bench.py, eight ranks on one device: %.0f patches/s aggregate; slices %s" % (line["value"], pr["cpus"]))


def test_bench_under_torch_distributed_run_with_the_kernels_in_it():
    """the driver's N > 1 command, word for word -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node 2
    --master-addr 127.0.0.1 --master-port P bench.py --gpus 2 --steps 20 --warmup 5` -- on the one GPU a box has (plus the
    two flags that needs: gloo, every rank on cuda:0): the ranks come from the launcher's environment (no self-spawn),
    LOCAL_RANK picks the device, the timed regions (--full) are the median of the job's (MAX over ranks), rank 0 alone prints"""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20",
                        "--warmup", "5", "--backend", "gloo", "--share-device", "--full", "--no-cpu-baseline", "--no-secondary"],
                       env=_clean_env(), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.strip().startswith("{") and l.strip().endswith("}")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = lines[0]
    assert line["launch"] == "external launcher" and line["n_gpus"] == 2 and line["ranks_seen"] == 2
    assert line["steps"] == 20 and line["warmup"] == 5 and line["timed_regions"]["count"] >= 9
    assert line["config"]["global_batch"] == 16 and line["scaling"] == "weak" and line["value"] > 1e4
    assert abs(line["value"] - 16 * 1e3 / line["ms_per_step"]) <= 1e-6 * line["value"]
    alg = 144.0 * 256 * 256 * 8
    assert abs(line["roofline"]["frac"] * 8e12 * line["ms_per_step"] * 1e-3 / alg - 1.0) < 1e-9      # per launch, one clock
    assert line["per_rank"]["scene_seed"] == [313, 314] and len(line["per_rank"]["ms_per_step"]) == 2
    print("bench.py under torch.distributed.run, two ranks on one device: %.0f patches/s aggregate" % line["value"])


def test_bench_refuses_to_time_ranks_that_share_a_gpu_unannounced():
    """a scaling number measured with two ranks on one device is not a scaling number: two ranks whose launcher maps both to
    cuda:0 (LOCAL_RANK = 0 twice) without --share-device are found out before anything is timed -- the runtime's PCI
    addresses, gathered, are not `world` distinct ones -- and the job exits with code 3 and the reason"""
    from svbrdf_estimation_amd import launch
    port = launch.free_port()
    procs = []
    for r in range(2):
        env = _clean_env(RANK=str(r), LOCAL_RANK="0", WORLD_SIZE="2", LOCAL_WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                         MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo",
                                       "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-secondary"],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=600) for p in procs]
    assert [p.returncode for p in procs] == [3, 3], ([p.returncode for p in procs], outs[0][1][-1500:])
    assert "2 ranks sit on 1 distinct GPUs" in outs[0][1] and not any(o[0].strip().startswith("{") for o in outs)


def _check_selftest_line(line, world, transport):
    assert line["selftest"] is True and line["ok"] is True and line["ranks_seen"] == world == line["n_gpus"]
    assert line["distinct_devices"] == line["distinct_devices_expected"] and len(line["pci_bus_ids"]) == world
    assert line["transport"].startswith(transport) and line["allreduce_sums_correct"] is True
    for size in ("8MB", "320MB"):
        assert len(line["allreduce_GBps"][size]) == world and all(v > 0 for v in line["allreduce_GBps"][size])
    assert len(line["parity"]) == world
    for p in line["parity"]:
        assert p["ok"] and p["loss_rel_err"] <= 2e-6 and p["grad_outside_tolerance"] <= 8, p


def test_selftest_first_contact_over_rccl_world_of_one():
    """tools/scale_first_contact.md step 1 on the one GPU a box has: `bench.py --gpus 1 --force-dist --selftest` -- RCCL
    bring-up, PCI all-gather, the 8 MB and 320 MB all-reduces on device tensors, the fused loss against the committed
    reference fixture; one JSON line with ranks_seen / distinct_devices / allreduce_GBps"""
    line, _ = _run("bench.py", "--gpus", 1, "--force-dist", "--selftest")
    _check_selftest_line(line, 1, "RCCL")
    assert line["distinct_devices"] == 1 and line["process_group"].startswith("nccl")
    print("selftest over RCCL, world 1: device %s, 320 MB all-reduce call %.2f ms, parity %s" % (
        line["pci_bus_ids"], 1e3 * line["allreduce_seconds"]["320MB"][0], line["parity"][0]))
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "selftest_rccl_world1.json"), "w") as f:
        json.dump(line, f, indent=1)


@pytest.mark.parametrize("world", [2, 8])
def test_selftest_first_contact_self_spawned_ranks_share_the_device(world):
    """the same self-test as the driver's node would start it (`python bench.py --gpus N --selftest`, self-spawned), N ranks
    on this box's one GPU over gloo: every rank gathers, reduces and checks parity on the device"""
    line, _ = _run("bench.py", "--gpus", world, "--backend", "gloo", "--share-device", "--selftest", timeout=1500)
    _check_selftest_line(line, world, "gloo")
    assert line["launch"] == "self-spawned" and line["distinct_devices"] == 1 and len(set(line["pci_bus_ids"])) == 1
    print("selftest, %d ranks on one device (gloo): 320 MB all-reduce %s GB/s" % (
        world, ["%.1f" % v for v in line["allreduce_GBps"]["320MB"]]))


def test_selftest_that_finds_ranks_sharing_a_gpu_exits_with_code_3():
    """the failure the self-test exists for: N ranks, fewer than N distinct GPUs (here: two ranks told to expect their own
    device each while sharing cuda:0) -> exit code 3 and the reason on stderr, no hang, no JSON verdict of success"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-device",
                        "--selftest", "--selftest-expect-distinct"], env=_clean_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 3, (r.returncode, r.stderr[-2000:])
    assert "[selftest] FAILED" in r.stderr and "distinct GPUs" in r.stderr, r.stderr[-2000:]
    assert not any(l.strip().startswith("{") and '"ok": true' in l for l in r.stdout.splitlines())


def test_train_rccl_ddp_world_of_one():
    """train.py's N > 1 branches over RCCL at world size 1: process group with device_id, DistributedDataParallel
    around the U-Net (bucketed all-reduce of its 320 MB of gradients through RCCL), fused MixedLoss, barriers, the
    MAX and global-mean all-reduces"""
    line, _ = _run("train.py", "--gpus", 1, "--force-dist", "--steps", 2, "--warmup", 1, "--batch", 2, "--workers", 0,
                   "--loss", "mixed", timeout=1500)
    assert line["process_group"].startswith("nccl") and "DistributedDataParallel" in line["process_group"]
    assert line["ranks_seen"] == 1 and np.isfinite(line["loss_first_quarter"]) and np.isfinite(line["loss_last_quarter"])
    # bucket-overlap evidence the scaling run will carry: the backward with DDP's all-reduce and under no_sync()
    probe = line["ddp_backward_probe"]
    assert probe["samples_each"] >= 3 and probe["backward_ms_with_allreduce"] > 0 and probe["backward_ms_no_sync"] > 0
    assert len(line["per_rank"]["cpus"]) == 1 and line["per_rank"]["backward_ms"][0]["no_sync"] > 0
    assert probe["no_sync_left_gradients_rank_local"] is None              # one rank: nothing to compare (two: next test)
    assert line["config"]["miopen_cache"]["in_tree"] in (True, False) and abs(line["per_gpu_value"] - line["value"]) < 1e-9
    print("train.py over RCCL, world 1: backward %.1f ms with the all-reduce, %.1f ms under no_sync; miopen cache %s" % (
        probe["backward_ms_with_allreduce"], probe["backward_ms_no_sync"], line["config"]["miopen_cache"]))


def test_train_two_ranks_ddp_probe_checks_what_it_times():
    """train.py on two ranks sharing the device (gloo carries DDP's all-reduce): the probe steps after the timed region
    time a step with DDP's all-reduce and a step under model.no_sync() -- and check it: after a no_sync step (forward AND
    backward inside the context; DDP reads require_backward_grad_sync at the forward) the ranks' gradients differ, after
    a synchronised step they are equal.  Round 4's probe entered no_sync around the backward only and timed the
    all-reduce twice."""
    line, _ = _run("train.py", "--gpus", 2, "--backend", "gloo", "--share-device", "--steps", 2, "--warmup", 1, "--batch", 2,
                   "--workers", 0, "--loss", "mixed", timeout=1500)
    probe = line["ddp_backward_probe"]
    assert line["ranks_seen"] == 2 and probe["samples_each"] == 3
    assert probe["grad_checksum_spread_over_ranks_synced"] <= 1e-9 < probe["grad_checksum_spread_over_ranks_no_sync"], probe
    assert probe["no_sync_left_gradients_rank_local"] is True
    print("train.py, two ranks on one device (gloo): backward %.1f ms with the all-reduce, %.1f ms under no_sync; checksum "
          "spread over ranks %.1e synced / %.1e no_sync" % (probe["backward_ms_with_allreduce"], probe["backward_ms_no_sync"],
                                                            probe["grad_checksum_spread_over_ranks_synced"],
                                                            probe["grad_checksum_spread_over_ranks_no_sync"]))


def test_ddp_fused_loss_two_ranks_equal_the_global_batch(tmp_path):
    """DDP-wrapped U-Net + fused MixedLoss on two ranks sharing the device (gloo carries the gradient all-reduce)
    against ONE process with the whole batch: same items, same scenes per item (--verify-global-batch), so DDP's
    average of the two shard gradients must be the global-batch gradient, and the mean of the shard losses the
    global loss."""
    one, two = str(tmp_path / "one.npz"), str(tmp_path / "two.npz")
    common = ("--steps", 1, "--warmup", 0, "--workers", 0, "--loss", "mixed", "--samples", 4)
    l1, _ = _run("train.py", "--gpus", 1, "--batch", 4, "--verify-global-batch", one, *common, timeout=1500)
    l2, _ = _run("train.py", "--gpus", 2, "--backend", "gloo", "--share-device", "--batch", 2,
                 "--verify-global-batch", two, *common, timeout=1500)
    assert l2["ranks_seen"] == 2 and "gloo" in l2["process_group"] and l1["process_group"] is None
    a, b = np.load(one), np.load(two)
    assert int(a["world"]) == 1 and int(b["world"]) == 2 and a["grad"].shape == b["grad"].shape
    assert a["grad"].size > 79_000_000                                      # every trainable parameter of the U-Net
    assert abs(float(a["loss"]) - float(b["loss"])) <= 2e-6 * abs(float(a["loss"])), (a["loss"], b["loss"])
    gmax = np.abs(a["grad"]).max()
    err = np.abs(a["grad"] - b["grad"]).max()
    print("DDP (2 ranks) vs global batch: loss %.7f / %.7f, gradient max err / max = %.2e" % (a["loss"], b["loss"], err / gmax))
    # the convolutions' weight gradients sum over the batch in a different order (2 + 2 averaged vs 4) and MIOpen picks its
    # algorithms per batch shape; nothing else differs.  Measured 6.0e-5 ... 6.8e-5 of max over the boxes and conv modes of
    # round 3 (fp32 convolutions over 65,536 pixels); a sharding or scene-stream mistake is O(1) of max
    assert np.isfinite(a["grad"]).all() and gmax > 0 and err <= 3e-4 * gmax
