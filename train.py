#!/usr/bin/env python3
"""train.py -- data-parallel training harness around the rendering-loss engine.

One process per GPU (started by torchrun, or by this script itself: ``--gpus N`` without a rank environment
spawns N fresh rank processes before anything touches a GPU, svbrdf_estimation_amd/launch.py), batch sharded by rank with a DistributedSampler, stock
DistributedDataParallel for the U-Net: its ~320 MB of fp32 gradients per step are all-reduced by
RCCL over xGMI in buckets overlapped with the backward pass (backend "nccl" is RCCL on ROCm).  The
rendering / mixed loss itself needs no collective: each rank evaluates it on its shard with its own
scene RNG stream (seed + rank) and DDP's gradient averaging makes the result the global-batch
gradient.  What the reference's main.py:56-150 does on one GPU, in the reference's order:
batch -> (synthesise missing photos) -> model -> MixedLoss -> backward -> Adam(lr 1e-5).

  python train.py --steps 20                                   # 1 GPU, synthetic SVBRDFs, single-view
  python train.py --gpus 8 --batch 8 --steps 100               # 8 GPUs: spawns its own 8 ranks (config 3: global batch 64)
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train.py --gpus 8 --batch 8 --steps 100
  python train.py --model multi --views 5 --batch 16           # BASELINE config 4
  python train.py --size 512 --random-scenes 11 --specular-scenes 21   # BASELINE config 5 (per GPU)
  python train.py --data /path/to/tiled_pngs --image-count 10  # Deschaintre tiled-PNG samples

  python train.py --gpus 1 --force-dist                        # one GPU, but every multi-rank branch (RCCL process group, DDP)
  python train.py --gpus 2 --backend gloo --share-device       # two ranks on one GPU (control flow of an N-GPU run)

Convolutions: the U-Net runs on stock PyTorch-ROCm (MIOpen).  ``--conv-mode auto`` (default) picks, per direction, between
the reference's cudnn flags and MIOpen's immediate-mode choice (a four-step calibration of the forward; backward always
immediate: the reference's ``deterministic=True`` pins MIOpen to a backward 5-20x slower) -- DESIGN.md section 10.

``run(args)`` reads top to bottom: setup_rank -> build_model -> build_data -> train_steps -> assemble_result.  The modes
that reach into the step loop each have one home, called unconditionally and a no-op when off: ConvFlags (--conv-mode),
PhaseTimer (--phase-times), DdpProbe (the untimed DDP / no_sync steps behind the timed region).

Prints one JSON line per run on rank 0 (end-to-end patches/s, mean loss of the first/last steps).
"""
import argparse
import contextlib
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from svbrdf_estimation_amd import distributed, launch, losses, renderers, training, utils  # noqa: E402
from svbrdf_estimation_amd.training import data, models  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=0,
                    help="ranks (one per GPU).  0: whatever the launcher's WORLD_SIZE says (1 without a launcher)")
    ap.add_argument("--data", default="synthetic",
                    help="'synthetic': random SVBRDF maps drawn ON THE DEVICE, one batch per step, per-rank generator (no "
                         "dataloader: one CPU worker produces ~60 synthetic samples/s, less than a training step consumes); "
                         "'synthetic-cpu': the same statistics from a torch Dataset through the DataLoader / "
                         "DistributedSampler (what --device cpu and --verify-global-batch use); or a directory of tiled "
                         "PNG samples (the reference's SvbrdfDataset format)")
    ap.add_argument("--image-count", type=int, default=10, help="photos stored per tiled PNG")
    ap.add_argument("--scale-mode", choices=("crop", "resize"), default="crop")      # cli.py scale mode, dataset.py:58-89
    ap.add_argument("--random-crop", action="store_true")
    ap.add_argument("--mix-materials", action="store_true",
                    help="material-mixing augmentation (dataset.py:52-56, 142-160; main.py:49 enables it for training): "
                         "partner and weight drawn in the dataloader, blend on the GPU (kernel K4); needs --image-count 0")
    ap.add_argument("--linear-input", action="store_true")
    ap.add_argument("--model", choices=("single", "multi"), default="single")
    ap.add_argument("--views", type=int, default=1, help="input photos per sample (multi-view: N)")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=8, help="per-GPU batch")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lr", type=float, default=1e-5)                    # main.py:74
    ap.add_argument("--l1-weight", type=float, default=0.1)              # losses.py:55
    ap.add_argument("--random-scenes", type=int, default=3)              # losses.py:26
    ap.add_argument("--specular-scenes", type=int, default=6)            # losses.py:27
    ap.add_argument("--loss", choices=("mixed", "rendering", "l1"), default="mixed")
    ap.add_argument("--fused-head", action="store_true", help="model returns 9 channels, head decoded in the loss kernel")
    ap.add_argument("--no-coords", action="store_true")
    ap.add_argument("--samples", type=int, default=0, help="synthetic dataset length (default: enough for --steps)")
    ap.add_argument("--workers", type=int, default=-1,
                    help="DataLoader worker processes per rank; -1 = from the host: (cpus / ranks on this node) - 1, at "
                         "least 2, at most 16 -- the tiled-PNG reader delivers ~45-60 samples/s per worker "
                         "(profiles/r03_loader_rate.json), a training step consumes hundreds per GPU")
    ap.add_argument("--float-transport", action="store_true",
                    help="tiled-PNG samples: decode to float32 in the DataLoader workers (the reference's way) instead of "
                         "shipping the cropped 8-bit pixels and decoding them on the device with lookup tables (same bits, a "
                         "quarter of the bytes; 'crop' scale mode only)")
    ap.add_argument("--no-pin", action="store_true", help="DataLoader without the pinned-memory staging thread")
    ap.add_argument("--prefetch", type=int, default=4, help="batches each DataLoader worker keeps ready (prefetch_factor)")
    ap.add_argument("--seed", type=int, default=313)                     # utils.py:7
    ap.add_argument("--device", default="cuda", choices=("cuda", "cpu"))
    ap.add_argument("--backend", default=None, help="torch.distributed backend (default nccl on cuda, gloo on cpu)")
    ap.add_argument("--save", default=None, help="write a checkpoint (model + optimizer state) here at the end")
    ap.add_argument("--resume", default=None,
                    help="checkpoint to start from: one written by --save, or a checkpoint.tar of the reference "
                         "(persistence.py:52-69; model weights only)")
    ap.add_argument("--conv-mode", choices=("auto", "hybrid", "reference", "fast", "autotune"), default="auto",
                    help="how stock PyTorch-ROCm picks the U-Net's MIOpen convolution algorithms (DESIGN.md section 10).  "
                         "reference: cudnn.deterministic=True, benchmark=False as utils.py:11-12 sets them -- on ROCm a fine "
                         "forward and a pathological backward (2.7 s per step at configs[3]); fast: deterministic=False, "
                         "benchmark=False -- MIOpen's immediate-mode choice, no search: good backward; its forward is 5x "
                         "slower than the reference-flag forward on a box without stored find results and 30 %% faster with "
                         "them; hybrid: the reference's flags while the network runs forward, the immediate-mode choice while "
                         "autograd runs backward (the flags are read when a convolution executes); auto (default): hybrid, "
                         "plus a calibration during the first four steps that times the forward under both settings and "
                         "keeps the faster one -- no search, right on a fresh box and on one with a tuned cache; autotune: "
                         "benchmark=True -- MIOpen's find step compiles and times every candidate at the first call of "
                         "each shape (7 min at config 2; > 44 min at configs[3]); its results land in MIOpen's user cache")
    ap.add_argument("--autotune", action="store_true", help="same as --conv-mode autotune")
    ap.add_argument("--channels-last", action="store_true", help="NHWC activations/weights for the U-Net")
    ap.add_argument("--share-device", action="store_true",
                    help="every rank uses cuda:0 (with --backend gloo: the N-rank control flow, DDP included, on a box with "
                         "fewer GPUs than ranks; tests/test_gpu_multirank.py)")
    ap.add_argument("--force-dist", action="store_true",
                    help="with one rank: still create the process group (world size 1), wrap the network in DDP and take "
                         "every multi-rank branch, so that the RCCL code an N-GPU run executes runs on a one-GPU box")
    ap.add_argument("--verify-global-batch", default=None, metavar="NPZ",
                    help="verification run: makes an N-rank run and a one-rank run of the same GLOBAL batch comparable -- "
                         "contiguous unshuffled shards, dropout off, the network's input photo taken from the diffuse map, "
                         "and ONE scene stream (every rank seeds alike and skips the draws that belong to the other ranks' "
                         "items) -- and writes rank 0's gradient after the first backward (DDP-averaged) and the global "
                         "loss to this file")
    ap.add_argument("--bringup-timeout", type=float, default=60.0,
                    help="multi-rank: seconds the rendezvous + communicator set-up + first all-reduce may take before the "
                         "rank prints a diagnosis and exits with code 3 (the limit covers the rendezvous: raise it for multi-node "
                         "jobs and slow cold starts)")
    ap.add_argument("--no-ddp-probe", action="store_true",
                    help="skip the eight untimed steps after the timed region that time a whole step's forward + backward "
                         "with DDP's all-reduce and under model.no_sync() (multi-rank GPU runs; CPU runs with --ddp-probe)")
    ap.add_argument("--ddp-probe", action="store_true",
                    help="run the DDP probe steps on --device cpu too (host clock instead of HIP events): the gloo tests of "
                         "the probe's control flow")
    ap.add_argument("--phase-times", action="store_true",
                    help="bracket the phases of every timed step (dataloader wait on the host clock; upload + input "
                         "synthesis, network forward, loss, backward, optimizer with HIP events) and report their means: "
                         "costs one device synchronisation per step, so `value` of such a run is not a throughput figure")
    return ap.parse_args(argv)


def mark():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def stopwatch(device):
    """starts now; the call it returns ends it and gives the milliseconds (HIP events and one device synchronisation, or
    the host clock on the CPU)"""
    start = mark() if device.type == "cuda" else time.perf_counter()

    def stop():
        if device.type != "cuda":
            return 1e3 * (time.perf_counter() - start)
        end = mark()
        torch.cuda.synchronize(device)
        return start.elapsed_time(end)
    return stop


class ConvFlags:
    """--conv-mode in one place: what cudnn.deterministic / benchmark are around forward, backward and optimizer.
    reference / fast / autotune set them once and never toggle; hybrid: the reference's flags while the network runs
    forward, MIOpen's immediate-mode choice while autograd runs backward (only on a GPU).
    auto: hybrid, with the forward under the reference's flags at steps 0-1, under the immediate-mode choice at steps 2-3
    (the first of each pair compiles, the second is timed by `stopwatch`); from step 4 on the faster of the two.  The four
    calibration steps are EXTRA untimed steps in front of the warm-up (they carry two device synchronisations and two
    steps under the slower setting: never part of `value`, whatever --warmup says), and the ranks agree on the choice:
    the timings go through `max_over_ranks` (None with one rank) before they are compared."""

    def __init__(self, mode, on_gpu, max_over_ranks=None, stopwatch=None):
        self.mode, self.max_over_ranks, self.stopwatch = mode, max_over_ranks, stopwatch
        self.hybrid = mode in ("hybrid", "auto") and on_gpu
        self.auto = mode == "auto" and on_gpu
        self.calib_steps = 4 if self.auto else 0
        self.forward_flag, self.calib, self.stop = True, {}, None
        if mode in ("fast", "autotune"):       # enable_deterministic_random_engine set the reference's flags before this
            torch.backends.cudnn.deterministic = False
            torch.backends.cudnn.benchmark = mode == "autotune"

    def before_forward(self, step):
        if self.auto:
            if step < 4:
                self.forward_flag = step < 2
            elif step == 4 and len(self.calib) == 2:
                if self.max_over_ranks:     # one choice for the whole job: the slowest rank's timing of each setting decides
                    self.calib = dict(zip((True, False), self.max_over_ranks([self.calib[True], self.calib[False]])))
                self.forward_flag = self.calib[True] <= self.calib[False]
            if step in (1, 3):
                self.stop = self.stopwatch()
        if self.hybrid:
            torch.backends.cudnn.deterministic = self.forward_flag

    def after_forward(self):
        if self.stop is not None:
            self.calib[self.forward_flag] = self.stop()
            self.stop = None
        if self.hybrid:      # backward always takes MIOpen's immediate-mode choice
            torch.backends.cudnn.deterministic = False

    def after_optimizer(self):
        if self.hybrid:
            torch.backends.cudnn.deterministic = True

    def report(self):       # result["config"]["conv_forward"]; None outside auto
        name = {True: "reference flags", False: "immediate mode"}
        return {"chosen": name[self.forward_flag], "calibration_ms": {name[k]: v for k, v in self.calib.items()}} if self.auto else None


class PhaseTimer:
    """--phase-times: HIP events between the phases of a step and one device synchronisation at its end; off, every
    call returns at once."""
    phases = ("data_wait", "upload_synthesis", "forward", "loss", "backward", "optimizer")

    def __init__(self, on, device):
        self.on, self.device, self.ms = on, device, {k: [] for k in self.phases}

    def start(self, wait_s):
        if self.on:
            self.wait_s, self.marks = wait_s, [mark()]

    def mark(self):
        if self.on:
            self.marks.append(mark())

    def commit(self, timed):
        if self.on:
            self.marks.append(mark())
            torch.cuda.synchronize(self.device)
            if timed:
                self.ms["data_wait"].append(1e3 * self.wait_s)
                for name, a, b in zip(self.phases[1:], self.marks[:-1], self.marks[1:]):
                    self.ms[name].append(a.elapsed_time(b))

    def report(self):
        return {"phase_ms_mean": {k: sum(v) / max(1, len(v)) for k, v in self.ms.items()},
                "phase_note": "per-step means over the timed steps; one device synchronisation per step (not a throughput run)"}


class DdpProbe:
    """After the timed region, DDP runs only: the same step WITH the bucketed all-reduce (DDP's hooks launch a bucket's
    all-reduce on RCCL's stream as soon as its gradients exist, overlapping the rest of the backward) and WITHOUT it,
    alternating, a `stopwatch` around loss.backward() -- what the all-reduce of ~320 MB costs a step beyond the backward it
    hides behind.  DDP decides whether a backward synchronises when the FORWARD runs (require_backward_grad_sync is read
    in DistributedDataParallel.forward), so a no_sync probe step has its forward, its loss and its backward inside
    model.no_sync() (round 4 entered it around the backward only and measured the all-reduce twice).  Each probe step
    also checks what it claims: a checksum of the first parameter's gradient goes through `gather` to every rank -- equal
    on all ranks after a synchronised step, rank-local after a no_sync step.  No optimizer step in these.
    The probe steps are `first` .. `first + 7` (none when off); odd offsets run under no_sync."""

    def __init__(self, on, first, gather=None, stopwatch=None):
        self.steps, self.first, self.gather, self.stopwatch = 8 if on else 0, first, gather, stopwatch
        self.ms = {True: [], False: []}
        self.sums = {True: [], False: []}          # per probe step: the gradient checksum of every rank

    def probing(self, step):
        return self.first <= step < self.first + self.steps

    def synced(self, step):
        return not (self.probing(step) and (step - self.first) % 2 == 1)

    def start(self, step):
        return self.stopwatch() if self.probing(step) else None

    def finish(self, step, stop, net):
        ms = stop()
        g0 = next(p.grad for p in net.parameters() if p.grad is not None)
        self.record(step, ms, self.gather(g0.detach().double().abs().sum().reshape(1)))

    def record(self, step, ms, sums):
        if step - self.first >= 2:                    # the first pair warms the no_sync path up
            self.ms[self.synced(step)].append(ms)
            self.sums[self.synced(step)].append([float(e) for e in sums])

    def backward_ms(self):
        return {("with_allreduce" if k else "no_sync"): (sum(v) / len(v) if v else None) for k, v in self.ms.items()}

    @staticmethod
    def spread(sums):       # largest relative difference between the ranks' gradient checksums of one step
        return max((max(v) - min(v)) / max(abs(max(v)), 1e-300) for v in sums) if sums else None

    def report(self, world, on_gpu):
        """result["ddp_backward_probe"]"""
        w, n = self.ms[True], self.ms[False]
        synced, no_sync = self.spread(self.sums[True]), self.spread(self.sums[False])
        return {"backward_ms_with_allreduce": sum(w) / len(w), "backward_ms_no_sync": sum(n) / len(n), "samples_each": len(w),
                "grad_checksum_spread_over_ranks_synced": synced, "grad_checksum_spread_over_ranks_no_sync": no_sync,
                "no_sync_left_gradients_rank_local": (no_sync > 1e-9 and synced <= 1e-9) if world > 1 else None,
                "note": "rank 0, untimed steps after the timed region, %s around loss.backward(): DDP's bucketed "
                        "all-reduce (gradient_as_bucket_view, 25 MB buckets) against a step whose forward and backward both ran "
                        "inside model.no_sync(); the difference is what the all-reduce of the U-Net's gradients costs a step "
                        "beyond the backward it overlaps with.  grad_checksum_spread_*: sum |grad| of the first parameter, "
                        "gathered from every rank per probe step -- 0 after a synchronised step, > 0 after a no_sync step (the "
                        "ranks hold different shards), which is the evidence that the second figure is a backward WITHOUT the "
                        "all-reduce (with one rank there is nothing to compare)" % ("HIP events" if on_gpu else "the host clock")}


def setup_rank(args):
    """Rank bring-up: the rank environment, the CPU binding before the first GPU call, the device, the process group.
    May set args.backend (--share-device)."""
    # this pool's host driver only supports dmabuf IPC: RCCL between rank processes needs it (read when the HSA runtime
    # starts, i.e. at the first GPU call; the self-spawning parent sets it for its children too)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", world))      # ranks on THIS node (multi-node: world > local_world)
    if args.gpus and args.gpus != world:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: start one rank per GPU (or run train.py without a rank "
                         "environment and let it spawn them)" % (args.gpus, world))
    on_gpu = args.device == "cuda"
    host_cpus = os.sched_getaffinity(0)
    if on_gpu:
        # first thing in a rank, before any GPU call: pin it (and the DataLoader workers it will fork) to the CPUs next to
        # its GPU, ranks on one socket splitting that socket's cores (launch.py)
        placement = launch.bind_rank_to_gpu_numa(local_rank, local_world, args.share_device)
        assert torch.cuda.is_available(), "no ROCm device visible"
        if args.share_device:
            local_rank = 0
            if world > 1 and (args.backend or "nccl") == "nccl":
                # RCCL refuses two ranks on one device (and would hang in init or the first collective before saying so)
                if args.backend == "nccl":
                    raise SystemExit("--share-device puts every rank on cuda:0, which RCCL does not support: use --backend gloo")
                args.backend = "gloo"
        elif torch.cuda.device_count() <= local_rank:
            raise SystemExit("local rank %d but only %d device(s) visible on this node" % (local_rank, torch.cuda.device_count()))
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        placement = launch.crosscheck_placement(placement, local_rank, host_cpus)   # PCI address: sysfs vs the runtime
    else:
        placement = {"cpus": launch.format_cpulist(host_cpus), "n_cpus": len(host_cpus), "numa_node": None,
                     "source": "unbound: --device cpu", "bound": False}
        if args.loss != "l1":
            raise SystemExit("the rendering loss has no CPU path; --device cpu only supports --loss l1 (plumbing tests)")
        if args.mix_materials:
            raise SystemExit("--mix-materials blends on the GPU (kernel K4); there is no CPU path for it")
        dev = torch.device("cpu")
    ranks_seen = 1
    grouped = world > 1 or args.force_dist
    backend = (args.backend or ("nccl" if on_gpu else "gloo")) if grouped else None
    nccl = backend == "nccl"
    if grouped:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:                          # --force-dist without a launcher: a rendezvous of one
            os.environ.setdefault("MASTER_PORT", str(launch.free_port()))
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        # rendezvous + communicator + one all-reduce under a watchdog (distributed.init_process_group_checked): exit code 3
        # and a diagnosis after --bringup-timeout seconds instead of the launcher's limit
        ranks_seen = distributed.init_process_group_checked(backend, dev if nccl else None, args.bringup_timeout)
        if on_gpu:      # one rank per GPU, or the job stops here with the reason (--share-device: the plumbing tests' exception)
            distributed.require_distinct_devices(dev, args.share_device, rank)

    def fence():    # what opens and closes the timed region: one device synchronisation, one barrier when grouped, the clock
        if on_gpu:
            torch.cuda.synchronize(dev)
        if nccl:
            dist.barrier(device_ids=[local_rank])
        elif grouped:
            dist.barrier()
        return time.perf_counter()
    return types.SimpleNamespace(rank=rank, local_rank=local_rank, world=world, local_world=local_world, on_gpu=on_gpu,
                                 device=dev, placement=placement, grouped=grouped, backend=backend, nccl=nccl,
                                 ranks_seen=ranks_seen, fence=fence)


def max_over_ranks(r, values):
    t = torch.tensor(values, dtype=torch.float64, device=r.device if r.nccl else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return t.tolist()


def gather_over_ranks(r, mine):
    if r.on_gpu and not r.nccl:                      # gloo moves host tensors
        mine = mine.cpu()
    every = [torch.zeros_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(every, mine)
    return every


def build_model(args, r):
    """Seed, network (+ --resume), DDP, optimizer, loss and the convolution flags, in the order the RNG and cudnn need."""
    verify = args.verify_global_batch
    # per-rank scene RNG -- or, for --verify-global-batch, one stream shared by all ranks (each skips the others' draws)
    utils.enable_deterministic_random_engine(args.seed if verify else distributed.rank_seed(args.seed, r.rank))
    if r.on_gpu:    # the rank's own CPU work is tiny (scene sampler, collation): a big intra-op pool only spins (bench.py main)
        torch.set_num_threads(max(1, min(8, r.placement["n_cpus"])))
    decode = not args.fused_head
    if args.model == "multi":
        net = models.MultiViewModel(use_coords=not args.no_coords, decode=decode)
    else:
        net = models.SingleViewModel(use_coords=not args.no_coords, decode=decode)
    conv = ConvFlags("autotune" if args.autotune else args.conv_mode, r.on_gpu,
                     (lambda values: max_over_ranks(r, values)) if r.grouped else None, lambda: stopwatch(r.device))
    steps_done = 0
    if args.resume:
        ck = torch.load(args.resume, map_location="cpu", weights_only=False)
        state = ck["model_state_dict"]
        own = set(net.state_dict().keys())
        # a checkpoint in the reference's parameter names (what --save writes, and what the reference writes), or one in
        # this package's own names (written by --save before it switched to the reference's layout)
        net.load_state_dict(state if set(state.keys()) <= own else models.convert_reference_state_dict(state))
        steps_done = int(ck.get("steps", 0))
    net = net.to(r.device).train()
    if verify:
        for m in net.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
    if args.channels_last:
        net = net.to(memory_format=torch.channels_last)
    # identical initial weights on every rank: DDP broadcasts rank 0's parameters at construction.
    # gradient_as_bucket_view: the parameters' .grad ARE views of the all-reduce buckets (no 320 MB copy per step)
    model = torch.nn.parallel.DistributedDataParallel(net, device_ids=[r.local_rank] if r.on_gpu else None,
                                                      gradient_as_bucket_view=True) if r.grouped else net
    optimizer = torch.optim.Adam(model.parameters(), lr=args.lr)
    if args.resume and "optimizer_state_dict_amd" in ck:
        optimizer.load_state_dict(ck["optimizer_state_dict_amd"])

    if args.loss == "l1":
        loss_fn = losses.SVBRDFL1Loss()
        if args.fused_head:
            raise SystemExit("--fused-head needs the rendering or mixed loss")
    else:
        weight = args.l1_weight if args.loss == "mixed" else 0.0
        loss_fn = (losses.FusedHeadLoss if args.fused_head else losses.MixedLoss)(renderers.LocalRenderer(), weight)
        loss_fn.rendering_loss.random_configuration_count = args.random_scenes
        loss_fn.rendering_loss.specular_configuration_count = args.specular_scenes
    return types.SimpleNamespace(net=net, model=model, optimizer=optimizer, loss_fn=loss_fn, conv=conv, steps_done=steps_done)


def build_data(args, r, n_steps):
    """The batch source for `n_steps` steps: an endless iterator, and whether it draws on the device.  Sets args.workers."""
    verify = args.verify_global_batch
    if args.workers < 0:        # the rank's CPU set is its share of the node already (placement), else split the host
        mine = r.placement["n_cpus"] if r.placement.get("bound") else (os.cpu_count() or 2) // max(1, r.local_world)
        args.workers = max(2, min(16, mine - 1))
    if args.data == "synthetic" and r.on_gpu and not verify:
        args.workers = 0

        def device_batches():
            gen = torch.Generator(device=r.device).manual_seed(distributed.rank_seed(args.seed * 7919, r.rank))
            empty = torch.zeros(args.batch, 0, 3, args.size, args.size)
            while True:
                yield {"inputs": empty, "svbrdf": data.synthetic_svbrdf_batch(args.batch, args.size, r.device, gen)}
        return device_batches(), True
    if args.data in ("synthetic", "synthetic-cpu"):
        n = args.samples or n_steps * args.batch * r.world
        dataset = data.SyntheticSvbrdfDataset(n, image_size=args.size, seed=args.seed)
    else:
        dataset = data.TiledPngDataset(args.data, image_size=args.size, image_count=args.image_count,
                                       used_image_count=args.views, is_linear=args.linear_input,
                                       scale_mode=args.scale_mode, random_crop=args.random_crop,
                                       mix_materials=args.mix_materials, uint8_transport=r.on_gpu and not args.float_transport)
    if verify:
        sampler = distributed.ContiguousShardSampler(len(dataset), args.batch, r.rank, r.world)
    else:
        sampler = torch.utils.data.distributed.DistributedSampler(dataset, num_replicas=r.world, rank=r.rank, shuffle=True,
                                                                  seed=args.seed, drop_last=True) if r.world > 1 else None
    loader = torch.utils.data.DataLoader(dataset, batch_size=args.batch, sampler=sampler, shuffle=sampler is None,
                                         num_workers=args.workers, pin_memory=r.on_gpu and not args.no_pin, drop_last=True,
                                         persistent_workers=args.workers > 0,
                                         **({"prefetch_factor": args.prefetch} if args.workers > 0 else {}))

    def epochs():
        epoch = 0
        while True:
            if sampler is not None and hasattr(sampler, "set_epoch"):
                sampler.set_epoch(epoch)
            for b in loader:
                yield b
            epoch += 1
    return epochs(), False


def prepare_inputs(args, r, batch):
    """a batch as the source delivers it -> the network's input and the target maps, on the device"""
    batch = data.decode_uint8_batch(batch, r.device, is_linear=args.linear_input)    # 8-bit transport: decoded on the device
    svbrdf = batch["svbrdf"].to(r.device, non_blocking=True)
    stored = batch["inputs"].to(r.device, non_blocking=True)
    if r.on_gpu and not args.verify_global_batch:
        svbrdf = data.apply_mixing(svbrdf, batch)                            # K4: material mixing, whole batch
        photos = data.complete_inputs(stored, svbrdf, args.views)           # K1: missing photos, whole batch
    else:                                                                    # CPU plumbing runs: constant photos
        photos = torch.cat((stored, svbrdf[:, None, 3:6].expand(-1, max(args.views - stored.shape[1], 0), -1, -1, -1)), 1)
    return (photos if args.model == "multi" else photos[:, 0]), svbrdf


def save_global_gradient(path, args, r, net, loss):
    """--verify-global-batch: rank 0's gradient after the first backward (DDP-averaged) and the global loss"""
    g_loss = distributed.global_mean(loss.detach() if (r.nccl or not r.grouped) else loss.detach().cpu()).item()
    if r.rank == 0:
        flat = torch.cat([p.grad.reshape(-1) for p in net.parameters() if p.grad is not None])
        np.savez(path, grad=flat.cpu().numpy(), loss=np.float64(g_loss), world=r.world, per_rank_batch=args.batch)


def train_steps(args, r, m, batches, timer, probe, first_timed, end_timed):
    """The step loop: untimed steps up to `first_timed`, the timed region up to `end_timed` (outside the helpers' modes no
    device synchronisation inside it; one fence opens it, one closes it), then the probe's steps.  Returns the loss of every
    step that updated the weights and the seconds this rank spent in the timed region."""
    verify, conv, model, optimizer = args.verify_global_batch, m.conv, m.model, m.optimizer

    def skip_scenes(items_of_ranks):     # --verify-global-batch: ONE scene stream, the other ranks' draws skipped
        if verify and args.loss != "l1" and items_of_ranks > 0:
            m.loss_fn.rendering_loss.sample_scene_table(items_of_ranks * args.batch)
    losses_seen, t0, elapsed = [], None, None
    for step in range(end_timed + probe.steps):
        if step == first_timed:
            t0 = r.fence()
        if step == end_timed:
            elapsed = r.fence() - t0
        t_wait = time.perf_counter()
        batch = next(batches)
        timer.start(time.perf_counter() - t_wait)
        net_in, svbrdf = prepare_inputs(args, r, batch)
        optimizer.zero_grad(set_to_none=True)
        timer.mark()
        conv.before_forward(step)
        with (contextlib.nullcontext() if probe.synced(step) else model.no_sync()):     # forward AND backward: see DdpProbe
            out = model(net_in)
            conv.after_forward()
            timer.mark()
            skip_scenes(r.rank)                                                         # the scenes of the lower ranks' items
            loss = m.loss_fn(out, svbrdf)
            skip_scenes(r.world - 1 - r.rank)                                           # ... and of the higher ranks' items
            timer.mark()
            stop = probe.start(step)
            loss.backward()
        if stop is not None:
            probe.finish(step, stop, m.net)
            optimizer.zero_grad(set_to_none=True)
            continue
        if verify and step == 0:
            save_global_gradient(verify, args, r, m.net, loss)
        timer.mark()
        optimizer.step()
        conv.after_optimizer()
        losses_seen.append(loss.detach())
        timer.commit(step >= first_timed)
    t1 = r.fence()
    return losses_seen, (t1 - t0 if elapsed is None else elapsed)


def rank_record(placement, elapsed, backward_ms=None):
    """what one rank reports about itself; `backward_ms` (the probe's means) only in a process group"""
    rec = {"elapsed_s": elapsed, "cpus": placement["cpus"], "numa_node": placement["numa_node"],
           "cpu_binding": placement["source"], "pci_crosscheck": placement.get("pci_crosscheck")}
    return rec if backward_ms is None else dict(rec, backward_ms=backward_ms)


def per_rank_table(records, batch, steps):
    """result["per_rank"]: the ranks' records column by column, with the rates that follow from elapsed_s"""
    per_rank = {k: [e[k] for e in records] for k in records[0]}
    per_rank["ms_per_step"] = [1e3 * e / steps for e in per_rank["elapsed_s"]]
    per_rank["patches_per_s"] = [batch * steps / e for e in per_rank["elapsed_s"]]
    return per_rank


def assemble_result(args, r, m, device_source, miopen_cache, losses_seen, own_elapsed, timer, probe):
    own = rank_record(r.placement, own_elapsed, probe.backward_ms() if r.grouped else None)
    records, elapsed = [own], own_elapsed
    if r.grouped:
        elapsed, = max_over_ranks(r, [own_elapsed])
        records = [None] * dist.get_world_size()
        dist.all_gather_object(records, own)
    vals = torch.stack(losses_seen).float()
    if r.grouped and not r.nccl:
        vals = vals.cpu()
    first, last = vals[: max(1, len(vals) // 4)].mean(), vals[-max(1, len(vals) // 4):].mean()
    first, last = distributed.global_mean(first).item(), distributed.global_mean(last).item()
    result = {"metric": "end-to-end training patches/s (U-Net + %s loss)" % args.loss,
              "value": r.world * args.batch * args.steps / elapsed, "unit": "patches/s", "n_gpus": r.world,
              "per_gpu_value": args.batch * args.steps / elapsed,
              "ranks_seen": r.ranks_seen, "per_rank": per_rank_table(records, args.batch, args.steps),
              "process_group": ("%s, world size %d, DistributedDataParallel" % (r.backend, dist.get_world_size())) if r.grouped else None,
              "ms_per_step": 1e3 * elapsed / args.steps, "steps": args.steps, "warmup": args.warmup,
              "loss_first_quarter": first, "loss_last_quarter": last,
              "config": {"model": args.model, "views": args.views, "size": args.size, "per_gpu_batch": args.batch,
                         "scenes": args.random_scenes + args.specular_scenes, "fused_head": bool(args.fused_head),
                         "data": ("synthetic (device)" if device_source else args.data) if args.data.startswith("synthetic") else "tiled-png",
                         "workers": args.workers, "conv_mode": m.conv.mode, "channels_last": bool(args.channels_last),
                         "miopen_cache": training.miopen_cache_identity(miopen_cache)}}
    if len(vals) <= 64:         # short runs (tests): every step's own loss, calibration and warm-up steps included
        result["loss_per_step"] = [float(v) for v in vals.tolist()]
        result["untimed_leading_steps"] = m.conv.calib_steps + args.warmup
    if probe.steps:
        result["ddp_backward_probe"] = probe.report(r.world, r.on_gpu)
    if m.conv.auto:
        result["config"]["conv_forward"] = m.conv.report()
    if timer.on:
        result.update(timer.report())
    return result


def save_checkpoint(path, args, m, steps):
    # the reference's checkpoint.tar layout (persistence.py:52-69) with the REFERENCE's parameter names, so that
    # its Checkpoint.restore_model_state loads the weights into its own SingleViewModel / MultiViewModel.  The
    # optimizer state indexes parameters by position, which differs between the two module trees: it is kept
    # under its own key instead of one the reference would load into the wrong slots.
    torch.save({"model_type": args.model, "use_coords": not args.no_coords, "epoch": 0,
                "model_state_dict": models.convert_to_reference_state_dict(m.net.state_dict()),
                "optimizer_state_dict_amd": m.optimizer.state_dict(), "steps": steps}, path)


def run(args):
    miopen_cache = training.use_in_tree_miopen_cache()      # before the first convolution of the process
    r = setup_rank(args)
    m = build_model(args, r)
    first_timed = m.conv.calib_steps + args.warmup
    end_timed = first_timed + args.steps
    batches, device_source = build_data(args, r, end_timed)
    timer = PhaseTimer(args.phase_times and r.on_gpu, r.device)
    probe = DdpProbe(r.grouped and (r.on_gpu or args.ddp_probe) and not args.verify_global_batch and not args.no_ddp_probe,
                     end_timed, lambda mine: gather_over_ranks(r, mine), lambda: stopwatch(r.device))
    losses_seen, elapsed = train_steps(args, r, m, batches, timer, probe, first_timed, end_timed)
    result = assemble_result(args, r, m, device_source, miopen_cache, losses_seen, elapsed, timer, probe)
    if r.rank == 0:
        if args.save:       # total steps: calibration, warm-up and probe steps included
            save_checkpoint(args.save, args, m, m.steps_done + end_timed + probe.steps)
        print(json.dumps(result), flush=True)
    if r.grouped:
        dist.destroy_process_group()
    return result


def main(argv=None):
    args = parse_args(argv)
    if args.gpus > 1 and not launch.launched_as_rank():
        # one plain process asked for N GPUs: become the parent of N fresh rank processes (no GPU call has
        # happened in this process and none will)
        sys.exit(launch.spawn_ranks(os.path.abspath(__file__), sys.argv[1:] if argv is None else argv, args.gpus))
    return run(args)


if __name__ == "__main__":
    main()
