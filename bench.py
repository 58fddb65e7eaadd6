#!/usr/bin/env python
"""bench.py -- TrackFormer-Deformable per-frame inference throughput on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config cfg1|cfg2|cfg3|cfg4|cfg5]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
    (`python bench.py --gpus N` with N > 1 outside a launcher re-executes itself under
    torch.distributed.run on 127.0.0.1: one rank per GPU.)

--config selects a BASELINE.json configuration (cfg2 -- the one the metric is quoted on -- is the
default and the headline; the others print their own metric in the same JSON layout):
  cfg1  plain DETR R50, one 480x640 frame, 100 object queries: forward + post-processing
  cfg2  Deformable TrackFormer inference, 800x1333, 300 object + 100 track queries: Tracker.step
  cfg3  Deformable TrackFormer training step, bs 2 per GPU, 800x1333 (fwd prev frame + match + fwd +
        loss + bwd incl. the MSDeformAttn backward + gradient all-reduce over RCCL + AdamW)
  cfg4  MOT20 crowded-scene model (multi_frame: hidden 288, 8 decoder levels), 500 + 300 queries
  cfg5  MOTS20 mask head on the tracking detector (the buildable configuration: hidden 256, see
        DESIGN.md section 2), Tracker.step incl. per-track masks

Workload (BASELINE.json configs[1], SURVEY.md section 8d "cfg 2"): DeformableDETRTracking
(ResNet-50, 4 feature levels, hidden 256, 6+6 layers), synthetic 800x1333 frames already resident in
HBM, 300 object queries + exactly 100 track queries per frame, batch 1, fp32, weights = seeded default
initialisation (no checkpoints / datasets exist offline).  One step = one `Tracker.step(blob)`:
detector forward, post-processing, the single packed device->host copy and the host-side association
(thresholds, NMS, id bookkeeping).  Before every step the tracker is re-seeded with the same 100
tracks so that each step has exactly 300+100 queries.  Since round 3 the association leg has work to do: the "person"
output of the last class head is rescaled / shifted on frame 0 (calibrate_association) so that about half of the 400 queries
pass the 0.4 thresholds and the seeded tracks are that frame's top-100 outputs -- ~98 seeded tracks survive a step, ~150
detections go through NMS and add_tracks (`association` in the line; --no-calibration: the default-initialised head, no
query passes, the leg idles as in rounds 1-2).  Several sequences per GPU are interleaved in ONE host thread
(Tracker.step_async / step_finish): `multi_sequence_fps`; `value` is the ONE-sequence figure (BASELINE cfg 2: bs = 1).

Multi-GPU: the path shards by video sequence (engine.py:289-303 of the reference); every rank tracks
its own sequence on its own GPU, there is no collective in the data path ("scaling": "weak").  RCCL is
used only for the barriers around the timed region and the max-over-ranks of the elapsed time.

Timing: W untimed warm-up steps, then EXACTLY K steps between barrier + synchronize on both sides,
max over ranks; `value` is K / that time, `ms_per_step` the time of one step.  A plain run does only that; every other
figure below needs --full (null otherwise), whose side legs repeat their K-step set for at least --min-seconds (2 s).
--dump-outputs DIR: what the timed leg computed in its last step, as DIR/<name>.npy (bench.write_outputs).

The JSON line also carries
  roofline      -- the dominant custom kernel, MSDeformAttn forward at the encoder call shape
                   (N=1, S=Lq=22223, M=8, D=32, L=4, P=4) THROUGH THE FUSED ENTRY the model calls:
                   algorithmic bytes (79.65 MB) / average launch duration measured here with
                   HIP events on the launch stream (launches replayed from one HIP graph, rotating over
                   4 input sets so that the Infinity Cache is cold), on the perturbed-weight sampling
                   pattern; the default-initialised and the wide pattern are reported beside it.
  cpu_baseline  -- the same workload on the host CPU: identical nn.Modules on CPU with the reference's
                   pure-CPU MSDeformAttn path (grid_sample, oracle/msda_grid_sample.py: "kind":
                   "reference-restated"); the C port of the kernels' arithmetic (oracle/msda_ref.c)
                   timed beside it; rank 0, N=1 only, a bounded sample.
  step_only_fps / host_frames_fps / plain_step_fps -- one sequence: (1) step_finish(step_async(blob)) per frame, no look-ahead
                   (= Tracker.step with tracker.deferred = False; HBM frames); (2) the pipelined loop with the frames in pinned
                   host memory, the upload inside the timed step; (3) the reference's own loop, `for blob in frames:
                   tracker.step(blob)` (src/track.py:130-134) on host frames -- what an UNMODIFIED caller gets: with the deferred
                   association of Tracker.step (round 6, default) and with tracker.deferred = False.  `value` is the pipelined
                   loop on HBM-resident frames.
  single_sequence_fps / multi_sequence_fps -- cfg2/4/5: the same steps with ONE sequence per GPU (no overlap of one
                   sequence's host-side association with another's forward) / with --sequences interleaved.
  precision     -- `value` is measured with the DEFAULT arithmetic of the package (fused.split_terms(); `dtype` and
                   `precision.value_measured_with` name it): every dense layer as a split product on the matrix cores with fp32
                   accumulation (include/tf_fused.h) -- the fp16 product (two / three fp16 pieces per operand, three MFMAs, fp32-class
                   accuracy) or the six-term bf16 product (all 24 significand bits).  Beside it: fp32_exact_fps /
                   single_sequence_fp32_exact_fps (every matrix product in the fp32 LIBRARIES: hipBLASLt linears, MIOpen
                   convolutions; 3 sequences / one sequence) and the other fp32-class product (split6_fps / split_f16_fps).
                   (The three-term bf16 fast mode of rounds 2-4 and its split3_fps leg were removed in round 5.)
  association   -- what the association leg did in four untimed steps (survivors, initialised, alive).
  parity        -- cfg2: in-run check against the committed reference goldens (max |d boxes|, max |d logits|, ids equal).
  mfma_utilisation -- "live": the dense kernels of the frame timed HERE with HIP events at their cfg-2 shapes, as fp32-equivalent
                   TFLOP/s and as matrix-pipe utilisation = flops x terms / (2.5 PFLOP/s x time); "pmc": the committed counter
                   pass (rocprofv3 --pmc needs its own run), with the commit it was taken at.
  ranks         -- N > 1: what every rank runs on, gathered over the job's own backend.
"""
import argparse
import json
import math
import os
import sys
import time

# RCCL / cross-process device memory on this stack need dmabuf IPC (see the environment notes)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

IMG_H, IMG_W = 800, 1333
HBM_PEAK_GBS = 8000.0   # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s

# BASELINE.json configs: (config overlays, overrides, (H, W), track queries, what a step is)
CONFIGS = {
    "cfg1": dict(overlays=(), overrides=dict(dataset="coco"), size=(480, 640), tracks=0, kind="detect",
                 name="BASELINE cfg 1: plain DETR R50, one 480x640 frame, 100 object queries, forward + PostProcess",
                 metric="frames/sec, plain DETR (ResNet-50, 640x480, 100 queries) forward + post-processing",
                 unit="frames/s"),
    "cfg2": dict(overlays=("deformable", "tracking", "mot17"), overrides={}, size=(IMG_H, IMG_W), tracks=100,
                 kind="track",
                 name="BASELINE cfg 2: Tracker.step on 800x1333 synthetic frames, DeformableDETRTracking R50 4 "
                      "levels, 300 obj + 100 track queries",
                 metric="frames/sec, TrackFormer-Deformable inference (ResNet-50, 1333x800, 300 object + 100 "
                        "track queries, bs 1 per GPU); roofline = ms_deform_attn HBM GB/s", unit="frames/s"),
    "cfg3": dict(overlays=("deformable", "tracking", "mot17"), overrides={}, size=(IMG_H, IMG_W), tracks=0,
                 kind="train",
                 name="BASELINE cfg 3: training step (fwd prev frame + match + fwd + loss + bwd + all-reduce + "
                      "AdamW), bs 2 per GPU, 800x1333, 30 boxes per image",
                 metric="images/sec, Deformable TrackFormer training step, bs 2 per GPU, 1333x800", unit="images/s"),
    "cfg4": dict(overlays=("deformable", "tracking", "multi_frame", "mot17"), overrides={}, size=(IMG_H, IMG_W),
                 tracks=300, kind="track",
                 name="BASELINE cfg 4: Tracker.step, multi-frame model (hidden 288, 8 decoder levels), 500 obj + "
                      "300 track queries, 800x1333",
                 metric="frames/sec, TrackFormer multi-frame (MOT20 config) inference, 1333x800, 500 + 300 queries",
                 unit="frames/s"),
    "cfg5": dict(overlays=("deformable", "tracking", "mots20"), overrides={}, size=(IMG_H, IMG_W), tracks=100,
                 kind="track",
                 name="BASELINE cfg 5: Tracker.step with the mask head (MOTS20: deformable + tracking + masks, "
                      "hidden 256 -- the buildable configuration), 300 obj + 100 track queries, 800x1333",
                 metric="frames/sec, TrackFormer MOTS20 (mask head) inference, 1333x800, 300 + 100 queries",
                 unit="frames/s"),
}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="default: 120 (cfg 1/2/4), 24 (cfg 5), 6 (cfg 3)")
    ap.add_argument("--warmup", type=int, default=None, help="default: 8 (cfg 1/2/4), 4 (cfg 3, cfg 5)")
    ap.add_argument("--config", choices=sorted(CONFIGS), default="cfg2")
    ap.add_argument("--min-seconds", type=float, default=2.0,
                    help="--full side legs: repeat the K-step set until this much timed work has accumulated")
    ap.add_argument("--full", action="store_true",
                    help="also the side legs, association, parity, roofline, matrix-core and CPU figures")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the headline leg computed in its last timed step as DIR/<name>.npy")
    ap.add_argument("--no-graph", action="store_true", help="run the detector eagerly (no HIP graph)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline-only", action="store_true",
                    help="(internal) time the CPU leg of --config and print its JSON object: the main run starts this in a "
                         "fresh process so that the leg gets torch's default one-thread-per-core set-up")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-single-sequence", action="store_true")
    ap.add_argument("--no-prepare", action="store_true",
                    help="do not run the next frame's image-only half ahead of the association (Tracker.step_prepare)")
    ap.add_argument("--look-ahead", type=int, default=2,
                    help="frames whose image-only half may be enqueued ahead of the frame being associated (capped by Tracker.look_ahead)")
    ap.add_argument("--no-fp32-exact", action="store_true",
                    help="skip the second measurement with every matrix product in fp32 (hipBLASLt / library convolutions)")
    ap.add_argument("--no-parity", action="store_true",
                    help="skip the in-run parity check against the committed reference goldens (cfg 2 only)")
    ap.add_argument("--no-calibration", action="store_true",
                    help="keep the default-initialised class bias (-4.6: no query passes a score threshold, the association leg idles)")
    ap.add_argument("--roofline-only", action="store_true",
                    help="measure only the roofline kernel (headline pattern) and print its JSON object: the command "
                         "profiles/r02_bench_roofline_kernel_stats.csv was collected with under rocprofv3 --stats")
    ap.add_argument("--cpu-frames", type=int, default=2)
    ap.add_argument("--host-frames", action="store_true",
                    help="keep the frames in pinned host memory (PCIe copy inside the timed region); "
                         "the reported headline value always uses HBM-resident frames")
    ap.add_argument("--split-linear", dest="split_linear", action="store_true", default=None,
                    help="encoder / decoder linears as bf16 split products on the matrix cores "
                         "(tf_linear_split_f32; same as TF_SPLIT_LINEAR=1)")
    ap.add_argument("--no-split-linear", dest="split_linear", action="store_false")
    ap.add_argument("--split-terms", type=int, choices=(6, 16), default=None,
                    help="the split product (include/tf_fused.h): 6 bf16 terms or 16 = fp16 pieces (three terms, fp32-class accuracy); "
                         "default: the package's (fused.split_terms())")
    ap.add_argument("--no-split3", action="store_true",
                    help="skip the extra measurement with the other split product (the flag's name is from the rounds that had three)")
    ap.add_argument("--conv1x1-split", dest="conv1x1_split", action="store_true", default=None,
                    help="the backbone's stride-1 1x1 convolutions through the split-product GEMM with the "
                         "FrozenBN / identity / ReLU epilogue (the default; --no-conv1x1-split = TF_CONV1X1_SPLIT=0)")
    ap.add_argument("--no-conv1x1-split", dest="conv1x1_split", action="store_false")
    ap.add_argument("--conv3x3-split", dest="conv3x3_split", action="store_true", default=None,
                    help="the bottlenecks' 3x3 convolutions through the split-product implicit GEMM (the default)")
    ap.add_argument("--no-conv3x3-split", dest="conv3x3_split", action="store_false")
    ap.add_argument("--input-proj-fused", dest="input_proj_fused", action="store_true", default=None,
                    help="input_proj (1x1 convolution + GroupNorm) as split GEMM + own GroupNorm (the default)")
    ap.add_argument("--no-input-proj-fused", dest="input_proj_fused", action="store_false")
    ap.add_argument("--sequences", type=int, default=3,
                    help="independent video sequences interleaved per GPU (one HIP stream each, one host thread in all: "
                         "Tracker.step_async / step_finish); frames of one sequence stay strictly sequential")
    args = ap.parse_args()
    train = CONFIGS[args.config]["kind"] == "train"
    heavy = args.config == "cfg5"   # ~100 full-size masks per frame reach the host: tens of ms per step
    if args.steps is None:
        args.steps = 6 if train else 24 if heavy else 120
    if args.warmup is None:
        args.warmup = 4 if train else 4 if heavy else 8   # (training: 2 steps left a one-off ~0.6 s stall of the first process on a fresh box inside the timed region, profiles/r06_train_step_breakdown.txt)
    return args


def relaunch_under_torchrun(args):
    """`python bench.py --gpus N` (N > 1) outside a launcher: re-execute under torch.distributed.run,
    one rank per GPU, rendezvous on 127.0.0.1 (engine.py:289-303 shards sequences over ranks)."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    os.execv(sys.executable, cmd)


def init_distributed(args):
    from trackformer_amd import dist_utils as du
    rank, local_rank, world = du.env_world()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch_under_torchrun(args)
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if world > 1:
        per_rank_caches(local_rank)
        if os.environ.get("TF_BENCH_ONE_DEVICE") == "1":
            # debugging aid for boxes with a single GPU: every rank uses cuda:0, the barriers go over gloo.
            # Exercises the launcher / rank-0 reporting path; the numbers it prints mean nothing.
            du.init_from_env(backend="gloo")
            return rank, 0, world
        torch.cuda.set_device(local_rank)
        du.pin_rank_to_cpus(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
        from trackformer_amd import runtime
        runtime.bind_streams(torch.device("cuda", local_rank))   # (before RCCL creates its own streams: see main())
        du.init_from_env(backend="nccl", device=torch.device("cuda", local_rank))  # nccl == RCCL
        verify_ranks(world, torch.device("cuda", local_rank))
    return rank, local_rank, world


def per_rank_caches(local_rank):
    """Every rank gets its own MIOpen user database / kernel cache directory and its own TunableOp output file.  Eight ranks
    of a first run writing ONE find-db under ~/.config/miopen serialise on its file lock (and can corrupt it): the classic
    first-run stall of an N = 8 job.  Must run before the first convolution (MIOpen reads the variables when it initialises)."""
    base = os.path.join(os.environ.get("TMPDIR", "/tmp"), "tf_bench_rank%d" % local_rank)
    for var, sub in (("MIOPEN_USER_DB_PATH", "miopen_db"), ("MIOPEN_CUSTOM_CACHE_DIR", "miopen_cache")):
        if var not in os.environ:
            os.makedirs(os.path.join(base, sub), exist_ok=True)
            os.environ[var] = os.path.join(base, sub)
    os.environ.setdefault("PYTORCH_TUNABLEOP_FILENAME", os.path.join(base, "tunableop_results.csv"))
    return base


def verify_ranks(world, device):
    """Before anything is timed: the job really is `world` processes on `world` DISTINCT devices talking over RCCL.  A
    mis-launched job (two ranks on one GPU, a gloo fall-back, a rank that did not start) would otherwise print a plausible
    line; here it stops with what it found (VERDICT r04 task 8; reference util/misc.py:421-444 init_distributed_mode)."""
    from trackformer_amd import dist_utils as du
    seen = du.ranks_seen(device)
    devices = {(r.get("uuid"), r.get("pci_bus_id"), r.get("device")) for r in seen}
    problems = []
    if len(seen) != world or len({r["pid"] for r in seen}) != world:
        problems.append("%d processes answered, %d expected" % (len({r["pid"] for r in seen}), world))
    if len(devices) != world:
        problems.append("%d distinct devices for %d ranks: %s" % (len(devices), world, sorted(str(d) for d in devices)))
    if any(r.get("backend") != "nccl" for r in seen):
        problems.append("backend %s, not nccl (RCCL)" % sorted({str(r.get("backend")) for r in seen}))
    if problems:
        raise SystemExit("bench.py --gpus %d: the job is not what the scaling run needs -- %s" % (world, "; ".join(problems)))


def _active_optins(backbone, fused):
    """Names of the fused routes (defaults since round 3) that are switched on in this process, plus any
    off-switch set in the environment: recorded in the JSON line."""
    flags = [("conv1x1_split", backbone._conv1x1_split), ("conv3x3_split", backbone._conv3x3_split),
             ("input_proj_fused", fused._input_proj_fused), ("box_refine_fused", fused._box_refine_fused),
             ("ffn_fused", fused.ffn_fused_enabled()), ("linln_fused", fused.linear_ln_fused_enabled()),
             ("stem_pool_fused", fused.stem_pool_fused_enabled()), ("stem_conv_split", fused.stem_conv_split_enabled()),
             ("pos_add_fused", fused.pos_add_fused_enabled()), ("heads_split", fused.heads_split_enabled())]
    names = [n for n, on in flags if on]
    for env in ("TF_SPLIT_TERMS", "TF_MSDA_PQUAD", "TF_MSDA_DIRECT9", "TF_MSDA_BWD_SORTED2",
                "TF_CONV_SPLIT_SKIP", "TF_CONV_SPLITK", "TF_CONV1X1_SPLITK", "TF_CONV_KSPLIT_POLICY", "TF_LAZY_MASKS"):
        if os.environ.get(env):
            names.append("%s=%s" % (env, os.environ[env]))
    return names


def build_model(cfg, device):
    from trackformer_amd import config, factory
    margs = config.make_args(*cfg["overlays"], device=str(device), **cfg["overrides"])
    torch.manual_seed(42)   # cfgs/train.yaml:112
    model, criterion, post = factory.build_model(margs)
    model.to(device)
    return model, criterion, post, margs


def sequence_stream(device, lanes=1, lane=0, narrow=False):
    """The stream a sequence's tracker runs on (dist_utils.sequence_stream, what track_sequences uses: high priority for a single
    sequence -- the decoder half and the post-processing, ~150 small launches the host waits for, are dispatched ahead of the
    image-only halves GraphedDetector runs on its side streams --, normal priority for interleaved sequences)."""
    from trackformer_amd.dist_utils import sequence_stream as make
    return make(device, lanes, lane, narrow)


def build_tracker(model, post, use_graph, lanes=1, lane=0):
    from trackformer_amd import config
    from trackformer_amd.tracker import Tracker
    detector = model
    if use_graph:
        from trackformer_amd.graphed import GraphedDetector
        detector = GraphedDetector(model, bucket=1, lanes=lanes, lane=lane)   # the benchmark's track-query count is fixed: no filler queries
    tracker = Tracker(detector, post, config.tracker_cfg(), False)
    tracker.reset()
    return tracker


class TrackSeeder:
    """Re-seeds the tracker with the same synthetic tracks before every step (exactly `n` track queries)."""

    def __init__(self, device, hidden_dim, n, size, seed=0, seeds=None):
        from trackformer_amd.box_ops import box_cxcywh_to_xyxy
        g = torch.Generator().manual_seed(seed)
        h, w = size
        self.n = n
        self.obj_ind = torch.arange(n).view(n, 1)
        if seeds is not None:   # calibrate_association: the detector's own top-n outputs on frame 0
            self.pos, self.scores, self.hs = seeds["pos"], seeds["scores"], seeds["hs"]
            return
        centres = torch.rand(n, 2, generator=g) * 0.8 + 0.1
        sizes = torch.rand(n, 2, generator=g) * 0.18 + 0.02
        self.pos = box_cxcywh_to_xyxy(torch.cat([centres, sizes], 1)) * torch.tensor(
            [w, h, w, h], dtype=torch.float32)
        self.scores = torch.full((n,), 0.9)
        self.hs = torch.randn(n, hidden_dim, generator=g).to(device)

    def seed(self, tracker):
        from trackformer_amd.tracker import Track
        # positions, scores and embeddings as (frame array, row) references, which is how the tracker itself files them: in a
        # running sequence every live track points into the previous frame's arrays (tracker._HsHistory, Track.pos)
        pos, scores, hs = self.pos, self.scores, self.hs
        tracker.tracks = [Track((pos, i), (scores, i), i, (hs, i), i) for i in range(self.n)]
        tracker.inactive_tracks = []
        tracker.track_num = self.n


def calibrate_association(model, frame, n_tracks, size, device, spread=1.5):
    """Give the association leg real work on random-init weights.  A default-initialised class head has bias
    -4.6 (deformable_detr.py:60-61 of the reference) and a random-init decoder spreads the logits of its queries over a few
    hundredths: no query reaches detection_obj_score_thresh / track_obj_score_thresh = 0.4, nothing is detected, every
    seeded track goes inactive.  Here the "person" output (class 0, the only label the tracker keeps: tracker.py:340 of the
    reference) of the LAST class head is rescaled and shifted by two constants, logit' = a * logit + b,
    chosen on frame 0 IN THE TRACKING CONTEXT (n seeded track queries + the object queries) so that the scores' logits
    have a standard deviation of `spread` and the n-th best object query sits at 0.4: about n detections per frame go
    through NMS against the tracks and through add_tracks, and (measured, `association` in the line) nearly all of the n
    seeded tracks survive each step.  The n seeded tracks are frame 0's top-n outputs (boxes, scores, decoder embeddings), so they
    come back as track queries with realistic content.  Only two constants of one Linear change: same kernels, same
    shapes, same arithmetic."""
    from trackformer_amd.box_ops import box_cxcywh_to_xyxy, box_xyxy_to_cxcywh
    h, w = size
    wh = torch.tensor([w, h, w, h], dtype=torch.float32, device=device)
    head = model.class_embed[-1]

    def seeds_from(out):
        scores = out['pred_logits'][0].sigmoid().max(-1).values
        top = scores.topk(n_tracks).indices
        return {"pos": (box_cxcywh_to_xyxy(out['pred_boxes'][0][top]) * wh).cpu(), "scores": scores[top].cpu(),
                "hs": out['hs_embed'][0][top].clone()}
    with torch.no_grad():
        img = frame['img'].to(device)
        out, *_ = model(img, None, None)
        seeds = seeds_from(out)
        target = [{'track_query_boxes': box_xyxy_to_cxcywh(seeds["pos"].to(device)) / wh, 'image_id': torch.ones(1, dtype=torch.int64, device=device),
                   'track_query_hs_embeds': seeds["hs"]}]
        out, *_ = model(img, [dict(t) for t in target], None)
        logit = out['pred_logits'][0][:, 0]
        a = spread / max(float(logit.std()), 1e-6)
        head.weight[0].mul_(a)
        head.bias[0].mul_(a)
        # the threshold sits at the n-th best OBJECT query (the last num_queries rows): ~n detections per frame (VERDICT r02:
        # "~100 object queries pass 0.4 and ~100 tracks survive"); the track queries are frame 0's best outputs and score
        # above it with few exceptions
        obj = logit[n_tracks:] * a
        k = max(1, min(int(obj.numel()) - 1, n_tracks))
        kth = float(obj.topk(k).values[-1])
        b = math.log(0.4 / 0.6) - kth + 1e-3
        head.bias[0].add_(b)
        out, *_ = model(img, None, None)     # the seeds' scores under the calibrated head
        seeds = seeds_from(out)
        out, *_ = model(img, [dict(t, track_query_hs_embeds=seeds["hs"]) for t in target], None)
        scores = out['pred_logits'][0].sigmoid().max(-1).values
    seeds.update(scale=round(a, 3), shift=round(b, 4), queries_above_0p4_frame0=int((scores > 0.4).sum()),
                 track_queries_above_0p4_frame0=int((scores[:n_tracks] > 0.4).sum()))
    return seeds


def association_stats(model, post, seeder, frames, steps=4):
    """What the association leg did in `steps` untimed steps of one (eager) tracker, per step: seeded tracks that survived
    (score threshold + track NMS), tracks newly initialised by add_tracks, tracks alive after the NMS of new against
    existing."""
    tracker = build_tracker(model, post, use_graph=False)
    survived, created, alive = [], [], []
    with torch.no_grad():
        for i in range(steps):
            seeder.seed(tracker)
            tracker.step(frames[i % len(frames)])
            survived.append(sum(1 for t in tracker.tracks if t.id < seeder.n))
            created.append(tracker.track_num - seeder.n)
            alive.append(len(tracker.tracks))
    return {"seeded_tracks": seeder.n, "seeded_tracks_surviving": survived, "new_tracks_initialised": created,
            "tracks_alive_after_step": alive}


def measure_parity(device, pipelined=True):
    """In-run parity of the product path against the committed goldens of the reference's own classes (tests/golden/
    full_cfg2_full.npz, full_tracker_cfg2.npz; generated by tests/golden/make_golden_full.py from /root/reference on CPU): the
    800 x 1333 cfg-2 model with the parity tests' perturbed weights in the bench set-up (tuned runtime, HIP graph, every
    default route), one detector call and the 3-frame tracker sequence.  Same code as tests/test_full_size_gpu.py."""
    import numpy as np
    from tests import test_full_size_gpu as T, util_models as um
    from trackformer_amd import config, factory
    cache = {}

    def models(case):
        if case not in cache:
            model, post, margs = um.build(case, factory.build_model, config.make_args, device=device)
            model.to(device).tracking()
            cache[case] = (model, post, margs)
        return cache[case]
    from trackformer_amd import fused
    case = "cfg2_full"
    # the set-up of tests/test_full_size_gpu.py that matches the arithmetic `value` is measured with
    setup = {16: "graph_split_linear", 6: "graph_split6"}[fused.split_terms()] if fused.split_linear_enabled() else "graph_tuned"
    model, out, res, feats, memory = T._forward(case, models, device, setup)
    z = np.load(os.path.join(T.GOLDEN, "full_%s.npz" % case))
    dbox = float(np.abs(out['pred_boxes'].cpu().numpy() - z['pred_boxes']).max())
    dlogit = float(np.abs(out['pred_logits'].cpu().numpy() - z['pred_logits']).max())
    tracker, rows, active = T._run_tracker(models, device, setup)
    zt = np.load(os.path.join(T.GOLDEN, "full_tracker_cfg2.npz"))
    ids_equal = bool(rows.shape == zt["rows"].shape and np.array_equal(rows[:, [0, 1, 7]], zt["rows"][:, [0, 1, 7]])
                     and int(zt["num_tracks"]) == tracker.track_num and zt["active_per_frame"].tolist() == active)
    line = {"against": "reference CPU path goldens (tests/golden/full_cfg2_full.npz, full_tracker_cfg2.npz), perturbed weights, 800x1333",
            "setup": setup, "max_abs_boxes": dbox, "max_abs_logits": dlogit, "tolerance": 1e-3,
            "ids_equal": ids_equal, "tracker_frames": int(len(active)), "track_rows": int(rows.shape[0])}
    if pipelined and setup in T._SPLIT_SETUPS:
        # THE PATH `value` IS TIMED ON (VERDICT r05 task 1b): step_async / step_prepare / step_finish with the image-only half of
        # the next frame on the side stream, two graphs, over the 64-frame well-conditioned 800x1333 sequence against the
        # reference's own Tracker (full_tracker_cfg2_wc64.npz): ids of every frame, and that the frames really were prepared
        zw = np.load(os.path.join(T.GOLDEN, "full_tracker_cfg2_wc64.npz"))
        n = len(zw["active_per_frame"])
        with torch.cuda.stream(sequence_stream(device)):   # (the high-priority stream the timed loop runs on)
            tr, rw, act, prepared = T._run_wc_tracker_pipelined(case, device, setup, n, host_frames=False)
        same_shape = rw.shape == zw["rows"].shape
        line["path"] = "pipelined"
        line["pipelined"] = {
            "against": "tests/golden/full_tracker_cfg2_wc64.npz (the reference's Tracker on CPU, well-conditioned 64-frame sequence, 800x1333)",
            "loop": "step_async(t) -> step_prepare(t+1, t+2) -> step_finish(t), frames resident in HBM, on a high-priority stream: "
                    "the loop run_tracking times",
            "look_ahead": int(tr.look_ahead),
            "frames": int(n), "frames_prepared": int(prepared), "track_rows": int(rw.shape[0]),
            "ids_equal": bool(same_shape and np.array_equal(rw[:, [0, 1, 7]], zw["rows"][:, [0, 1, 7]])
                              and int(zw["num_tracks"]) == tr.track_num and zw["active_per_frame"].tolist() == act),
            "max_abs_boxes_px": float(np.abs(rw[:, 2:6] - zw["rows"][:, 2:6]).max()) if same_shape else None,
            "max_abs_scores": float(np.abs(rw[:, 6] - zw["rows"][:, 6]).max()) if same_shape else None}
        line["ids_equal"] = bool(line["ids_equal"] and line["pipelined"]["ids_equal"])
    else:
        line["path"] = "step"
    return line


def make_frames(device, size, n=4, host=False):
    h, w = size
    frames = []
    for i in range(n):
        g = torch.Generator().manual_seed(i)
        img = torch.randn(1, 3, h, w, generator=g)
        img = img.pin_memory() if host else img.to(device)
        frames.append({'img': img, 'orig_size': torch.tensor([[h, w]]),
                       'size': torch.tensor([[h, w]]), 'dets': torch.zeros(1, 0, 4)})
    return frames


def _encoder_call_inputs(pattern, sets, device, seed=0, D=32):
    """Inputs of the FUSED operator entry at the cfg-2 encoder call shape, `sets` independent copies:
    value [1,S,8,32], qproj [1,S,384] (raw sampling offsets | attention logits, what the model's
    concatenated projection GEMM hands to the kernel), encoder reference points [1,S,4,2].
    pattern  init   the default-initialised module: zero offset weights, 8-direction bias grid
             pert   the bias grid + N(0, 0.8) raw offsets: what the perturbed-weight model of the parity
                    tests (tests/util_weights.py: sampling_offsets.weight ~ 0.05 * N(0,1), 256 inputs) produces
             local  reference point + N(0, 2 px) in the sampled level (SURVEY 8d "realistic")"""
    from tools.bench_msda import CFG2_SHAPES
    M, L, P = 8, 4, 4
    S = sum(h * w for h, w in CFG2_SHAPES)
    g = torch.Generator(device=device).manual_seed(seed)
    refs = []
    for (h, w) in CFG2_SHAPES:
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=device) + 0.5,
                                torch.arange(w, dtype=torch.float32, device=device) + 0.5, indexing="ij")
        refs.append(torch.stack([xs.reshape(-1) / w, ys.reshape(-1) / h], -1))
    ref = torch.cat(refs, 0).view(1, S, 1, 2).expand(1, S, L, 2).contiguous()
    dirs = torch.tensor([(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1) if (a, b) != (0, 0)],
                        dtype=torch.float32, device=device).view(1, 1, M, 1, 1, 2)
    k = torch.arange(1, P + 1, dtype=torch.float32, device=device).view(1, 1, 1, 1, P, 1)
    hw = torch.tensor(CFG2_SHAPES, dtype=torch.float32, device=device).view(1, 1, 1, L, 1, 2)   # (H, W)
    out = []
    for _ in range(sets):
        value = torch.randn(1, S, M, D, generator=g, device=device)
        noise = torch.randn(1, S, M, L, P, 2, generator=g, device=device)
        if pattern == "init":
            off = (dirs * k).expand(1, S, M, L, P, 2)
        elif pattern == "pert":
            off = dirs * k + 0.8 * noise
        elif pattern == "local":   # N(0, 2 px) of the sampled level; the module divides x by H_l and y by W_l
            off = noise * 2.0 * hw / hw.flip(-1)
        else:
            raise ValueError(pattern)
        logits = torch.randn(1, S, M * L * P, generator=g, device=device)
        qproj = torch.cat([off.reshape(1, S, M * L * P * 2), logits], -1).contiguous()
        out.append((value, qproj))
    return out, ref, S


def measure_roofline_backward(device, launches=10):
    """cfg 3: the MSDeformAttn backward at the encoder call shape of a bs-2 training step (N = 2), wide
    sampling pattern; 273 MB algorithmic bytes per launch (> the Infinity Cache with its outputs)."""
    from tools.bench_msda import CFG2_SHAPES, algorithmic_bytes, make_inputs, time_launches
    from trackformer_amd import msda
    S = sum(h * w for h, w in CFG2_SHAPES)
    value, shapes, loc, attn, grad_out = make_inputs(2, 8, 32, S, 4, CFG2_SHAPES, "local", device,
                                                     encoder_refs=True)
    ms = time_launches(lambda: msda.ms_deform_attn_backward(value, shapes, loc, attn, grad_out, 64), launches)
    alg = algorithmic_bytes(N=2, S=S, M=8, D=32, L=4, Lq=S, P=4, backward=True)
    gbs = alg / ms / 1e6
    kernel = msda.last_kernel()
    traffic = traffic_src = None   # the committed counter pass of the same kernel / shape / pattern (rocprofv3 --pmc needs its own runs)
    try:
        import glob
        newest = sorted(glob.glob(os.path.join(REPO, "profiles", "r[0-9][0-9]_msda_bwd_sorted2_traffic.json")))[-1]
        with open(newest) as f:
            tj = json.load(f)
        traffic = tj[kernel]["hbm_traffic_bytes_per_launch"]
        traffic_src = "profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, own passes; taken at commit %s)" % (os.path.basename(newest), tj.get("_commit"))
    except (OSError, KeyError, ValueError, IndexError):
        pass
    return {"bound": "hbm", "kernel": kernel + " (encoder call of a bs-2 training step, N=2, Lq=S=22223)",
            "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
            "traffic": traffic, "traffic_source": traffic_src, "algorithmic_bytes": alg, "avg_launch_us": round(ms * 1e3, 2), "launches": launches,
            "pattern": "local (reference point + N(0, 2 px))"}


def measure_roofline(device, launches=48, sets=4, train=False, head_dim=32, patterns=("pert", "init", "local"),
                     warm_replays=3, timed_replays=8):
    """HIP-event timing of the MSDeformAttn forward kernel at the cfg-2 encoder call shape, THROUGH THE
    FUSED ENTRY the model calls (tf_msda_forward_fused_f32), on the sampling pattern of the
    perturbed-weight parity model, rotating over `sets` input sets (4 x 80 MB > the 256 MiB Infinity
    Cache, so every launch reads HBM).  `launches` launches are captured in one HIP graph on the launch
    stream.  The default-initialised (`init`) and the wide (`local`) pattern are reported next to it."""
    if train:
        return measure_roofline_backward(device)
    from tools.bench_msda import CFG2_SHAPES, algorithmic_bytes
    from trackformer_amd import msda
    M, L, P, D = 8, 4, 4, head_dim
    stream = torch.cuda.Stream(device)
    per_pattern = {}
    alg = None
    for pattern in patterns:
        inputs, ref, S = _encoder_call_inputs(pattern, sets, device, D=D)
        alg = algorithmic_bytes(N=1, S=S, M=M, D=D, L=L, Lq=S, P=P)
        shapes = msda.attach_host_shapes(torch.tensor(CFG2_SHAPES, dtype=torch.long, device=device),
                                         CFG2_SHAPES)
        torch.cuda.synchronize(device)
        stream.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(stream):
            for value, qproj in inputs:
                msda.ms_deform_attn_forward_fused(value, shapes, ref, qproj, M, L, P)
            graph = torch.cuda.CUDAGraph()
            stream.synchronize()
            with torch.cuda.graph(graph, stream=stream):
                for i in range(launches):
                    value, qproj = inputs[i % sets]
                    msda.ms_deform_attn_forward_fused(value, shapes, ref, qproj, M, L, P)
            for _ in range(warm_replays):   # (clocks and caches in their steady state: one 2 ms replay alone read 41-44 us on
                graph.replay()              # boxes where ten of them read 38)
            stream.synchronize()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            for _ in range(timed_replays):
                graph.replay()
            end.record(stream)
            end.synchronize()
        us = start.elapsed_time(end) * 1e3 / (launches * timed_replays)
        per_pattern[pattern] = {"avg_launch_us": round(us, 2), "GBps": round(alg / (us * 1e-6) / 1e9, 1),
                                "frac": round(alg / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                                "kernel": msda.last_kernel()}   # what the library dispatched for this thread's last call
        del graph, inputs
    head = per_pattern["pert"]
    # HBM traffic of the same kernel / shape / pattern from the PMC counters: collected offline (rocprofv3
    # --pmc needs its own passes) and committed together with the method; see the file's "_how"
    # the kernel the LIBRARY dispatched for these calls (tf_msda_last_kernel), not what the options suggest
    kernel = head["kernel"]
    family = kernel.split("<")[0]   # the key of the committed counter passes
    if D != 32 and family == "msda_fwd_f32_pquad":
        family = "msda_fwd_f32_pquad<D=36>"
    traffic = traffic_src = None
    try:
        import glob
        newest = sorted(glob.glob(os.path.join(REPO, "profiles", "r[0-9][0-9]_msda_fwd_pquad_traffic.json")))[-1]
        with open(newest) as f:
            tj = json.load(f)
        traffic = tj[family]["hbm_traffic_bytes_per_launch"]
        traffic_src = "profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, own passes; taken at commit %s)" % (
            os.path.basename(newest), tj.get("_commit", "of round 3"))
    except (OSError, KeyError, ValueError, IndexError):
        pass
    return {"bound": "hbm", "kernel": kernel + " via tf_msda_forward_fused_f32 (encoder call, Lq=S=22223)",
            "achieved": head["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": head["frac"],
            "traffic": traffic, "traffic_source": traffic_src, "algorithmic_bytes": alg, "avg_launch_us": head["avg_launch_us"],
            "launches": launches * timed_replays, "launches_per_graph": launches, "warm_replays": warm_replays, "input_sets": sets,
            "pattern": "pert (perturbed-weight model sampling), Infinity-Cache-cold",
            "other_patterns": {k: v for k, v in per_pattern.items() if k != "pert"}}


MFMA_PEAK_BF16 = 2.5e15   # dense bf16 flop/s of the matrix cores (MI355X_MICROARCH.md)


# split product (fused.split_terms()) -> (short name, key of its side leg in the line, `dtype` text)
_ARITH = {
    6: ("six-term bf16 split product", "split6_fps",
        "f32 (dense layers as the six-term bf16 split product on MFMA: hi / mid / lo pieces carry all 24 significand bits, dropped terms "
        "< 2^-24 of a product, f32 accumulate -- fp32 arithmetic in another summation order)"),
    16: ("fp16 split product (three terms)", "split_f16_fps",
         "f32 (dense layers as the fp16 split product on MFMA: two fp16 pieces per activation, three per weight scaled per output "
         "channel -- 22 + 1 significand bits per operand, the one dropped product < 2^-22 --, three terms, f32 accumulate)"),
}


def measure_dense_kernels(device, hidden=256):
    """The dense kernels of a cfg-2 frame, timed HERE (HIP events around 20 launches replayed from one HIP graph on the launch
    stream) at the shapes the frame runs them: fp32-equivalent TFLOP/s and matrix-pipe utilisation = 2 M K N x terms /
    (2.5 PFLOP/s x time) -- the share of the run the matrix cores spend on this kernel's MFMAs if nothing else ran on them.
    Live, unlike the PMC figures next to it (which need their own rocprofv3 pass and are committed with their commit)."""
    import torch.nn as nn
    from trackformer_amd import fused
    terms = 3 if fused.split_terms() == 16 else fused.split_terms()   # MFMAs per product
    g = torch.Generator().manual_seed(0)
    rows = 22223
    out = {}

    def timed(fn, flop):
        stream = torch.cuda.Stream(device)
        with torch.cuda.stream(stream):
            fn()                                   # weight images built outside the capture
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                for _ in range(20):
                    fn()
            graph.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            graph.replay()
            e1.record(stream)
            e1.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / 20
        return {"us": round(us, 2), "tflops_fp32_equivalent": round(flop / us * 1e-6, 1),
                "mfma_util": round(flop * terms / MFMA_PEAK_BF16 / (us * 1e-6), 3)}
    with torch.no_grad():
        x = torch.randn(rows, hidden, generator=g).to(device)
        lin1, lin2, norm = nn.Linear(hidden, 1024).to(device), nn.Linear(1024, hidden).to(device), nn.LayerNorm(hidden).to(device)
        if fused.ffn(x, lin1, lin2, norm, x) is not None:
            out["ffn_fused 22223 x %d x 1024" % hidden] = timed(lambda: fused.ffn(x, lin1, lin2, norm, x), 4.0 * rows * hidden * 1024)
        proj = nn.Linear(hidden, hidden).to(device)
        if fused.linear(x, proj.weight, proj.bias) is not None:
            out["linear 22223 x %d -> %d" % (hidden, hidden)] = timed(lambda: fused.linear(x, proj.weight, proj.bias), 2.0 * rows * hidden * hidden)
        if fused.linear_residual_norm(x, proj, x, norm) is not None:
            out["linear + residual + LayerNorm 22223 x %d" % hidden] = timed(lambda: fused.linear_residual_norm(x, proj, x, norm),
                                                                             2.0 * rows * hidden * hidden)
        # ResNet-50 at 800 x 1333: layer2's 3 x 3 convolution (128 -> 128 at 100 x 167) and layer1's closing 1 x 1 (64 -> 256 at 200 x 334)
        xc = torch.randn(1, 128, 100, 167, generator=g).to(device).contiguous(memory_format=torch.channels_last)
        taps = (torch.randn(128, 9 * 128, generator=g) / 34).to(device)
        bias = torch.zeros(128, device=device)
        if fused.conv3x3(xc, taps, bias, True, 1) is not None:
            out["conv 3x3 128 -> 128 at 100 x 167"] = timed(lambda: fused.conv3x3(xc, taps, bias, True, 1), 2.0 * 16700 * 1152 * 128)
        x1 = torch.randn(66800, 64, generator=g).to(device)
        w1 = (torch.randn(256, 64, generator=g) / 8).to(device)
        r1 = torch.randn(66800, 256, generator=g).to(device)
        if fused.linear(x1, w1, None, relu=True, residual=r1) is not None:
            out["conv 1x1 64 -> 256 + identity + ReLU at 200 x 334"] = timed(lambda: fused.linear(x1, w1, None, relu=True, residual=r1),
                                                                             2.0 * 66800 * 64 * 256)
    return {"terms": terms, "split_product": _ARITH[fused.split_terms()][0], "peak": "2.5 PFLOP/s dense bf16 / fp16", "kernels": out}


def committed_mfma_utilisation():
    """Matrix-core utilisation of the dense kernels from a committed counter pass: PMC counters need their own
    rocprofv3 run.  Utilisation = SQ_VALU_MFMA_BUSY_CYCLES (summed over all SIMDs) / (dispatch duration x 2.4 GHz x 1024 SIMDs):
    it cannot exceed 1.  The newest profiles/r*_mfma_utilisation.json is used; `source_commit` / `terms` say what it describes."""
    import glob
    files = sorted(glob.glob(os.path.join(REPO, "profiles", "r[0-9][0-9]_mfma_utilisation.json")))
    if not files:
        return None
    try:
        with open(files[-1]) as f:
            d = json.load(f)
    except (OSError, ValueError):
        return None
    frame = {k: round(v["mfma_util"], 3) for k, v in d.get("mfma_frame", {}).items() if "mfma_util" in v}
    harness = {}
    for key, kern, label in (("mfma_ffn", "ffn_fused_kernel", "tf_ffn_fused_f32 22223x256x1024"),
                             ("mfma_lin1", "stream_gemm_kernel", "tf_linear_packed_f32 22223x256->1024"),
                             ("mfma_lin2", "gemm_kernel", "tf_linear_packed_f32 / tf_linear_split_f32 22223x256->256")):
        try:   # the kernel of that harness run that spent the most time (its name carries the template arguments)
            hits = [v for k, v in d[key].items() if kern in k and isinstance(v, dict) and "mfma_util" in v]
            if hits:
                harness[label] = round(max(hits, key=lambda v: v.get("dispatch_ns_total", 0))["mfma_util"], 3)
        except (KeyError, TypeError, AttributeError):
            pass
    return {"source": "profiles/%s (rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES, own pass)" % os.path.basename(files[-1]),
            "source_commit": d.get("_commit", "before round 4 (three-term kernels of round 3)"), "terms": d.get("_terms", 3),
            "per_kernel_in_an_eager_cfg2_frame": frame, "harness": harness}


def cpu_operator(kind):
    """MSDeformAttnFunction stand-ins for the CPU leg -- checkers used as the timed baseline, never shipped."""
    if kind == "reference-restated":
        from oracle import msda_grid_sample
        return msda_grid_sample.make_torch_function()
    from oracle import msda_oracle
    msda_oracle.build()
    cores = torch.get_num_threads()

    class HostOp(torch.autograd.Function):
        @staticmethod
        def forward(ctx, value, shapes, loc, attn, step):
            out = msda_oracle.msda_forward(value.numpy(), shapes.numpy(), loc.numpy(),
                                           attn.numpy(), nthreads=cores)
            return torch.from_numpy(out)
    return HostOp


def cpu_baseline_in_fresh_process(args):
    """The CPU leg in its own interpreter: this process has capped torch's intra-op threads for the association leg, holds a
    HIP context and pinned buffers; re-raising the thread count here left the leg ~10x slower on the MI355X box than in
    a process that never touched it (round 3, gpu_r03_16.sh).  A fresh process is what a CPU-only user would run."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["HIP_VISIBLE_DEVICES"] = ""     # the leg must not touch the GPU
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", "--config", args.config, "--cpu-frames", str(args.cpu_frames)]
    try:
        out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240, check=True, text=True).stdout
        return json.loads(out.strip().splitlines()[-1])
    except (subprocess.SubprocessError, ValueError, IndexError) as exc:
        return {"error": "%s: %s" % (type(exc).__name__, str(exc)[:200])}


def measure_cpu_baseline(cfg, frames):
    """The same workload on the host: identical modules on CPU; MSDeformAttn = the reference's pure-CPU
    path restated (grid_sample), and, as a second figure, the C port of the kernels' arithmetic."""
    from trackformer_amd import msda
    cores = torch.get_num_threads()   # a fresh process (cpu_baseline_in_fresh_process): torch's default, one thread per core
    cpu = torch.device("cpu")
    model, criterion, post, margs = build_model(cfg, cpu)
    saved = msda.MSDeformAttnFunction
    results = {}
    kinds = ("reference-restated", "port") if margs.deformable else ("port",)
    try:
        for kind in kinds:
            msda.MSDeformAttnFunction = cpu_operator(kind)
            if cfg["kind"] == "train":
                from tools.bench_train import synthetic_batch
                from trackformer_amd import engine
                if kind == "port":
                    continue   # the C port has no autograd
                model.train()
                criterion.train()
                optimizer, _ = engine.build_optimizer(model, margs)
                samples, targets = synthetic_batch(cpu, 1, *cfg["size"], seed=0)
                t0 = time.perf_counter()
                engine.train_step(model, criterion, optimizer, samples, targets,
                                  clip_max_norm=margs.clip_max_norm)
                dt = time.perf_counter() - t0
                results[kind] = (1 / dt, "1 training step on 1 image (bs 1 instead of 2), %.1f s" % dt)
                continue
            if hasattr(model, "tracking"):
                model.tracking()
            else:
                model.eval()
            t0 = time.perf_counter()
            with torch.no_grad():
                if cfg["kind"] == "detect":
                    for i in range(frames):
                        g = torch.Generator().manual_seed(i)
                        out, *_ = model(torch.randn(1, 3, *cfg["size"], generator=g), None, None)
                        post['bbox'](out, torch.tensor([list(cfg["size"])]))
                else:
                    tracker = build_tracker(model, post, use_graph=False)
                    seeder = TrackSeeder(cpu, margs.hidden_dim, cfg["tracks"], cfg["size"])
                    blobs = make_frames(cpu, cfg["size"], n=frames)
                    seeder.seed(tracker)
                    tracker.step(blobs[0])          # untimed: thread pools, oneDNN primitives, allocator
                    t0 = time.perf_counter()
                    for blob in blobs:
                        seeder.seed(tracker)
                        tracker.step(blob)
            dt = time.perf_counter() - t0
            results[kind] = (frames / dt, "%d frame(s) after one untimed frame, %.1f s" % (frames, dt))
    finally:
        msda.MSDeformAttnFunction = saved
    head = kinds[0]
    line = {"value": round(results[head][0], 4), "unit": cfg["unit"], "cores": cores, "kind": head,
            "sample": "%s of the same workload through the same nn.Modules on CPU (torch CPU kernels, %d "
                      "threads) with %s as the MSDeformAttn operator" % (
                          results[head][1], cores,
                          "the reference's pure-CPU path restated (grid_sample, oracle/msda_grid_sample.py)"
                          if head == "reference-restated" else "no deformable attention in this model"
                          if not margs.deformable else "oracle/msda_ref.c")}
    if "port" in results and head != "port":
        line["c_port"] = {"value": round(results["port"][0], 4), "kind": "port",
                          "sample": results["port"][1] + ", oracle/msda_ref.c (OpenMP, %d threads) as the "
                                                         "operator" % cores}
    return line


def _reduce_device(device):
    import torch.distributed as dist
    return "cpu" if dist.is_initialized() and dist.get_backend() == "gloo" else device


def timed_repeats(run_set, steps, world, device, min_seconds):
    """EXACTLY `steps` steps per repetition, each bracketed by barrier + synchronize; repeated until
    `min_seconds` of timed work; per-repetition time = max over ranks."""
    from trackformer_amd import dist_utils as du
    global _last_local_seconds
    total, reps, local = 0.0, 0, 0.0
    while True:
        torch.cuda.synchronize()
        du.barrier()
        t0 = time.perf_counter()
        run_set(steps)
        torch.cuda.synchronize()
        mine = time.perf_counter() - t0          # this rank's own time for the K steps (before it waits for the others)
        du.barrier()
        total += du.max_over_ranks(time.perf_counter() - t0, _reduce_device(device))
        local += mine
        reps += 1
        if total >= min_seconds or reps >= 200:
            _last_local_seconds = (local, reps)
            return total, reps


_last_local_seconds = None   # (this rank's own seconds, repetitions) of the last timed_repeats call
_last_outputs = None         # () -> {name: array}: what the last run_* leg computed in its last step (--dump-outputs)
DUMP_LIMIT_BYTES = 64 << 20
MASK_SAMPLE_PIXELS = 1 << 14
PARAM_SAMPLE = 1 << 20


def tracker_outputs(tracker, prefix=""):
    """What a caller of Tracker.step gets for the tracker's last frame (the rows `results` files for it): track ids, boxes (xyxy px),
    scores and object-query indices in track-id order; per-track masks at MASK_SAMPLE_PIXELS fixed, seeded pixel positions."""
    import numpy as np
    tracker._flush_deferred()
    last = tracker._pending_results[-1] if tracker._pending_results else None
    if last is None or last[0] != tracker.frame_index - 1:   # (no live track after the last frame: no row was filed for it)
        last = (tracker.frame_index - 1, [], np.zeros((0, 4)), [], [], None)
    frame, ids, pos, scores, obj_inds, extras = last
    order = np.argsort(np.asarray(ids, dtype=np.int64), kind="stable")
    out = {prefix + "track_ids": np.asarray(ids, dtype=np.float64)[order],
           prefix + "track_boxes": np.asarray(pos, dtype=np.float32).reshape(-1, 4)[order],
           prefix + "track_scores": np.asarray(scores, dtype=np.float32).reshape(-1)[order],
           prefix + "track_query_index": np.asarray(obj_inds, dtype=np.float64)[order]}
    masks = [None if extras is None else extras[i][0] for i in order]
    if any(m is not None for m in masks):
        rows = []
        pick = None
        for m in masks:
            m = m.materialise() if hasattr(m, "materialise") else m
            m = np.asarray(m.cpu() if torch.is_tensor(m) else m).reshape(-1)
            if pick is None:
                pick = np.sort(np.random.default_rng(0).choice(m.size, size=min(m.size, MASK_SAMPLE_PIXELS), replace=False))
            rows.append(m[pick].astype(np.float32))
        out[prefix + "track_masks_sampled"] = np.stack(rows)
        out[prefix + "track_masks_sample_index"] = pick.astype(np.float64)
    return out


def write_outputs(directory, arrays):
    """--dump-outputs: DIR/<name>.npy per array, float64 kept, everything else as float32; at most DUMP_LIMIT_BYTES in all."""
    import numpy as np
    conv = {}
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        conv[name] = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
    total = sum(a.nbytes for a in conv.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit("--dump-outputs: %d bytes, more than the %d allowed" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(directory, exist_ok=True)
    for name, a in conv.items():
        np.save(os.path.join(directory, name + ".npy"), a)
    return sorted(conv)


def _local_rate(steps, units=1):
    """This rank's own units per second over the last timed_repeats call (its K steps before it waited at the barrier)."""
    if _last_local_seconds is None or _last_local_seconds[0] <= 0:
        return None
    seconds, reps = _last_local_seconds
    return steps * reps * units / seconds


def run_tracking(cfg, args, device, world, model, post, margs, n_seq, seeds=None):
    """cfg 2 / 4 / 5: `n_seq` trackers (own HIP stream + graph buffers each, shared weights) step through synthetic frames;
    returns (elapsed, repeats).  Several sequences are interleaved in ONE thread (Tracker.step_async / step_finish): while
    one sequence's forward runs on the GPU the host does another one's association; frames of one sequence stay strictly
    sequential.  (Round 2 used one thread per sequence: with the association leg at work they serialise on the GIL and
    four threads are slower than one, profiles/r03_sequences_sweep.txt.)"""
    trackers = [build_tracker(model, post, use_graph=not args.no_graph, lanes=n_seq, lane=k) for k in range(n_seq)]
    # (the look-ahead policy of dist_utils.track_sequences: not for multi-frame models with several sequences in flight)
    look_ahead = not args.no_prepare and (n_seq == 1 or not getattr(model, "multi_frame_attention", False))
    depth = min(trackers[0].look_ahead, args.look_ahead) if look_ahead else 0
    seeder = TrackSeeder(device, margs.hidden_dim, cfg["tracks"], cfg["size"], seeds=seeds)
    frames = make_frames(device, cfg["size"], host=args.host_frames)
    narrow = bool(getattr(model, "multi_frame_attention", False))   # (the lanes' streams: dist_utils.LANE_MAINS_NARROW)
    streams = [sequence_stream(device, n_seq, k, narrow) for k in range(n_seq)]

    def run_set(steps):
        per_seq = [steps // n_seq + (1 if i < steps % n_seq else 0) for i in range(n_seq)]
        handles, issued, done, ahead = [None] * n_seq, [0] * n_seq, [0] * n_seq, [0] * n_seq
        torch.cuda.set_device(device)
        with torch.no_grad():
            while any(done[s] < per_seq[s] for s in range(n_seq)):
                for s in range(n_seq):
                    with torch.cuda.stream(streams[s]):
                        nxt = frames[(s + issued[s]) % len(frames)] if issued[s] < per_seq[s] else None
                        if handles[s] is not None:
                            # the image-only halves of the next frames (backbone, encoder) go to the GPU BEFORE the host associates
                            # this one: Tracker.step_prepare -- a single sequence no longer leaves the GPU idle; up to
                            # `depth` frames ahead (Tracker.look_ahead: 2 with graphs -- the halves of t + 1 and t + 2 share the chip)
                            while ahead[s] < depth and issued[s] + ahead[s] < per_seq[s]:
                                blob = frames[(s + issued[s] + ahead[s]) % len(frames)]
                                if not trackers[s].step_prepare(blob, image_ready=not args.host_frames):   # (device frames: resident since before the run)
                                    break
                                ahead[s] += 1
                            trackers[s].step_finish(handles[s])
                            handles[s] = None
                            done[s] += 1
                        if nxt is not None:
                            seeder.seed(trackers[s])
                            handles[s] = trackers[s].step_async(nxt)
                            issued[s] += 1
                            ahead[s] = max(0, ahead[s] - 1)
        for st in streams:
            st.synchronize()

    # warm-up (MIOpen find mode and the host-side caches are filled here; >= 4 steps per sequence: both HIP graphs of a
    # multi-frame model), then time
    run_set(n_seq * max(10, (args.warmup + n_seq - 1) // n_seq))   # (>= 10: every slot's pair of graphs exists before the timed region)
    torch.cuda.synchronize()
    from trackformer_amd import runtime
    runtime.settle_heap()   # model, trackers and graphs exist: the cyclic collector need not walk them again
    global _last_outputs
    _last_outputs = lambda: {k: v for s, tr in enumerate(trackers)   # noqa: E731
                             for k, v in tracker_outputs(tr, "seq%d_" % s if n_seq > 1 else "").items()}
    return timed_repeats(run_set, args.steps, world, device, args.min_seconds)


def run_plain_step(cfg, args, device, world, model, post, margs, seeds=None, deferred=True):
    """The reference's own loop, src/track.py:130-134: `for frame_data in seq_loader: tracker.step(frame_data)` -- ONE call per
    frame, frames arriving in (pinned) host memory as a DataLoader hands them over, nothing else touches the tracker.  With the
    deferred association of Tracker.step (round 6) this loop runs the pipelined schedule by itself.  The benchmark's re-seeding
    (exactly cfg["tracks"] track queries in every step) happens where it does in run_tracking: inside the step, after the previous
    frame's association and before this frame's track queries are built (a subclass hook; the call per frame stays step())."""
    from trackformer_amd import config, runtime
    from trackformer_amd.graphed import GraphedDetector
    from trackformer_amd.tracker import Tracker
    seeder = TrackSeeder(device, margs.hidden_dim, cfg["tracks"], cfg["size"], seeds=seeds)

    class SeededTracker(Tracker):
        def step_async(self, blob):
            seeder.seed(self)
            return super().step_async(blob)
    detector = model if args.no_graph else GraphedDetector(model, bucket=1)
    tracker = SeededTracker(detector, post, config.tracker_cfg(), False)
    tracker.reset()
    tracker.deferred = bool(deferred)
    frames = make_frames(device, cfg["size"], host=True)
    stream = sequence_stream(device)
    count = [0]

    def run_set(steps):
        torch.cuda.set_device(device)
        with torch.no_grad(), torch.cuda.stream(stream):
            for _ in range(steps):
                tracker.step(frames[count[0] % len(frames)])
                count[0] += 1
            tracker._flush_deferred()   # the last frame's association belongs to the timed region
        stream.synchronize()
    run_set(max(4, args.warmup))
    torch.cuda.synchronize()
    runtime.settle_heap()
    global _last_outputs
    _last_outputs = lambda: tracker_outputs(tracker)   # noqa: E731
    return timed_repeats(run_set, args.steps, world, device, args.min_seconds)


def run_detect(cfg, args, device, world, model, post):
    """cfg 1: forward + PostProcess of the plain DETR on one frame per step."""
    detector = model
    if not args.no_graph:
        from trackformer_amd.graphed import GraphedDetector
        detector = GraphedDetector(model)
    frames = make_frames(device, cfg["size"])
    sizes = torch.tensor([list(cfg["size"])], device=device)
    last = [None]

    def run_set(steps):
        with torch.no_grad():
            for i in range(steps):
                out, *_ = detector(frames[i % len(frames)]['img'], None, None)
                res = post['bbox'](out, sizes)
            res[0]['scores'].cpu()   # the frame's result reaches the host
        last[0] = res
    run_set(max(3, args.warmup))
    global _last_outputs
    _last_outputs = lambda: {"det_" + k: last[0][0][k] for k in ("scores", "labels", "boxes")}   # noqa: E731
    return timed_repeats(run_set, args.steps, world, device, args.min_seconds)


def run_training(cfg, args, device, world, rank, model, criterion, margs):
    """cfg 3: engine.train_step on a fixed synthetic batch of 2 images per GPU (DDP over RCCL when world > 1)."""
    from tools.bench_train import synthetic_batch
    from trackformer_amd import engine
    model.train()
    criterion.train()
    optimizer, _ = engine.build_optimizer(model, margs)
    ddp = engine.wrap_ddp(model, device)
    samples, targets = synthetic_batch(device, 2, *cfg["size"], seed=rank)
    last = [None]

    def run_set(steps):
        for _ in range(steps):
            tg = [dict(t, prev_target=dict(t['prev_target'])) for t in targets]   # forward mutates targets
            last[0] = engine.train_step(ddp, criterion, optimizer, samples, tg, clip_max_norm=margs.clip_max_norm)
    run_set(args.warmup)
    engine.settle_heap()   # (as engine.train_one_epoch does after its first steps: no oldest-generation collector pass inside a step)

    def outputs():
        """The step's weighted loss and loss dict, and PARAM_SAMPLE fixed, seeded entries of the updated parameters."""
        losses, loss_dict = last[0]
        out = {"loss": losses.double()}
        out.update(("loss_dict_" + k, torch.as_tensor(v).detach().double()) for k, v in sorted(loss_dict.items()))
        with torch.no_grad():
            flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
            pick = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(0))[:PARAM_SAMPLE].sort().values
            out["params_sampled"] = flat[pick.to(flat.device)]
            out["params_sample_index"] = pick.double()
        return out
    global _last_outputs
    _last_outputs = outputs
    return timed_repeats(run_set, args.steps, world, device, args.min_seconds)


def main():
    if os.environ.get("TF_BENCH_WATCHDOG"):   # debugging aid: dump every thread's stack after that many seconds
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["TF_BENCH_WATCHDOG"]), repeat=True, file=sys.stderr)
    args = parse_args()
    if args.cpu_baseline_only:   # no GPU, no process group: the host leg alone
        print(json.dumps(measure_cpu_baseline(CONFIGS[args.config], args.cpu_frames)))
        return
    rank, local_rank, world = init_distributed(args)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback for the product path)")
    cfg = CONFIGS[args.config]
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    from trackformer_amd import _cabi, fused, runtime
    _cabi.lib()   # fail loudly if the HIP library is missing
    # PyTorch's pool streams get their hardware queues here, in a fixed order, before anything else of this process (the tracker
    # loops, RCCL's own streams at the first collective) uses a stream: the rate of the pipelined loop depends on it
    runtime.bind_streams(device)
    train = cfg["kind"] == "train"
    if train:
        runtime.configure_training()
    else:
        runtime.configure_inference(tune=os.environ.get("TF_TUNE", "0") == "1",
                                    miopen_find=os.environ.get("TF_MIOPEN_FIND", "1") == "1",
                                    verbose=(rank == 0))
    if args.split_linear is not None:
        fused.set_split_linear(args.split_linear)
    if args.split_terms is not None:
        fused.set_split_terms(args.split_terms)
    from trackformer_amd import backbone as _backbone
    if args.conv1x1_split is not None:
        _backbone.set_conv1x1_split(args.conv1x1_split)
    if args.conv3x3_split is not None:
        _backbone.set_conv3x3_split(args.conv3x3_split)
    if args.input_proj_fused is not None:
        fused.set_input_proj_fused(args.input_proj_fused)
    if os.environ.get("TF_ROUND2_ROUTES") == "1":   # every round-3 route off at once (A/B aid: the round-2 defaults)
        _backbone.set_conv1x1_split(False)
        _backbone.set_conv3x3_split(False)
        fused.set_input_proj_fused(False)
        fused.set_box_refine_fused(False)
        fused.set_ffn_fused(False)
        fused.set_linear_ln_fused(False)
        fused.set_stem_pool_fused(False)
        fused.set_pos_add_fused(False)
        fused.set_stem_conv_split(False)
        fused.set_heads_split(False)

    if args.roofline_only:
        if rank == 0:
            hd = 36 if "multi_frame" in cfg["overlays"] else 32   # hidden 288 / 8 heads
            print(json.dumps(measure_roofline(device, head_dim=hd, patterns=("pert", "init", "local"))))
        return
    model, criterion, post, margs = build_model(cfg, device)
    single = fp32_exact = fp32_exact_single = association = multi = step_only = host_frames_fps = plain_step = None
    other_arith = {}
    n_seq = 1
    import copy
    head_args = copy.copy(args)
    head_args.min_seconds = 0.0   # the headline leg: ONE set of exactly --steps timed steps

    def headline_done():
        """Right after the headline leg: its rate on this rank, and (--dump-outputs, rank 0) what its last step computed."""
        if args.dump_outputs and rank == 0:
            names = write_outputs(args.dump_outputs, _last_outputs())
            print("bench: %d arrays of the last timed step in %s" % (len(names), args.dump_outputs), file=sys.stderr)
        return _local_rate(args.steps, units=2 if train else 1)
    if cfg["kind"] == "track":
        model.tracking()
        n_seq = max(1, args.sequences)
        seeds = None
        if not args.no_calibration and cfg["tracks"] > 0:
            seeds = calibrate_association(model, make_frames(device, cfg["size"], n=1)[0], cfg["tracks"], cfg["size"], device)
        if args.no_single_sequence:     # (A/B aid: only the interleaved set-up; then THAT is what the line reports)
            elapsed, reps = run_tracking(cfg, head_args, device, world, model, post, margs, n_seq, seeds)
            headline_local = headline_done()
        else:
            # THE HEADLINE: one sequence per GPU -- BASELINE.json's "bs = 1 on 1 x MI355X" (VERDICT r04 task 4).  The
            # throughput with --sequences interleaved (one sequence's host-side association under another's forward) is
            # reported beside it as multi_sequence_fps (--full), never as `value`.
            elapsed, reps = run_tracking(cfg, head_args, device, world, model, post, margs, 1, seeds)
            headline_local = headline_done()
            single = args.steps * reps * world / elapsed
            if n_seq > 1 and args.full:
                em, rm = run_tracking(cfg, args, device, world, model, post, margs, n_seq, seeds)
                multi = args.steps * rm * world / em
            n_seq = 1
        if args.full and not args.no_prepare and not args.no_single_sequence and not args.host_frames:
            # ... and the two figures a caller of the reference's own loop gets (VERDICT r05 task 1c): (1) plain Tracker.step()
            # per frame, no step_prepare -- what an unmodified src/track.py:130-134 drives; (2) the pipelined loop with the frames
            # in pinned HOST memory, the 12.8 MB upload inside the timed step (tracker.py:283-284 of the reference uploads too)
            a_step = copy.copy(args)
            a_step.no_prepare = True
            es, rs = run_tracking(cfg, a_step, device, world, model, post, margs, 1, seeds)
            step_only = args.steps * rs * world / es
            a_host = copy.copy(args)
            a_host.host_frames = True
            eh, rh = run_tracking(cfg, a_host, device, world, model, post, margs, 1, seeds)
            host_frames_fps = args.steps * rh * world / eh
            # (3) the reference's own loop itself: tracker.step(blob) per frame on host frames, association deferred into the next
            # step (the default) and not (tracker.deferred = False: step() returns after its association, as in round 5)
            ep, rp = run_plain_step(cfg, args, device, world, model, post, margs, seeds, deferred=True)
            es2, rs2 = run_plain_step(cfg, args, device, world, model, post, margs, seeds, deferred=False)
            plain_step = {"deferred_association": round(args.steps * rp * world / ep, 3),
                          "association_before_return": round(args.steps * rs2 * world / es2, 3),
                          "loop": "for blob in frames: tracker.step(blob) -- src/track.py:130-134 of the reference; frames in pinned host memory"}
        if args.full and seeds is not None and rank == 0:
            association = association_stats(model, post, TrackSeeder(device, margs.hidden_dim, cfg["tracks"], cfg["size"], seeds=seeds),
                                            make_frames(device, cfg["size"]))
            association.update(class_head_scale=seeds["scale"], class_head_shift=seeds["shift"],
                               queries_above_thresh_frame0=seeds["queries_above_0p4_frame0"],
                               track_queries_above_thresh_frame0=seeds["track_queries_above_0p4_frame0"])
        if args.full and fused.split_linear_enabled() and not args.no_fp32_exact:
            # the same measurement with every matrix product in the fp32 libraries (hipBLASLt linears, MIOpen convolutions), with
            # --sequences and with one sequence
            prev_split = fused.set_split_linear(False)
            try:
                ef, rf = run_tracking(cfg, args, device, world, model, post, margs, max(1, args.sequences), seeds)
                fp32_exact = args.steps * rf * world / ef
                if args.sequences > 1 and not args.no_single_sequence:
                    ef, rf = run_tracking(cfg, args, device, world, model, post, margs, 1, seeds)
                    fp32_exact_single = args.steps * rf * world / ef
            finally:
                fused.set_split_linear(prev_split)
        if args.full and fused.split_linear_enabled() and not args.no_split3:
            # ... and with the other split products (reported beside the headline, never as the headline)
            for alt in (6, 16):
                if alt == fused.split_terms():
                    continue
                prev_terms = fused.set_split_terms(alt)
                try:
                    e3, r3 = run_tracking(cfg, args, device, world, model, post, margs, max(1, args.sequences), seeds)
                    leg = {"sequences_per_gpu": max(1, args.sequences), "value": round(args.steps * r3 * world / e3, 3)}
                    if args.sequences > 1 and not args.no_single_sequence:
                        e3, r3 = run_tracking(cfg, args, device, world, model, post, margs, 1, seeds)
                        leg["single_sequence"] = round(args.steps * r3 * world / e3, 3)
                    other_arith[_ARITH[alt][1]] = leg
                finally:
                    fused.set_split_terms(prev_terms)
    elif cfg["kind"] == "detect":
        model.eval()
        elapsed, reps = run_detect(cfg, head_args, device, world, model, post)
        headline_local = headline_done()
    else:
        elapsed, reps = run_training(cfg, head_args, device, world, rank, model, criterion, margs)
        headline_local = headline_done()

    roofline = cpu_baseline = parity = mfma = None
    if rank == 0 and args.full:
        if not args.no_roofline and margs.deformable:
            roofline = measure_roofline(device, train=train, head_dim=margs.hidden_dim // margs.nheads)
        if args.config == "cfg2" and not args.no_parity and not args.no_graph:
            parity = measure_parity(device, pipelined=not args.no_prepare)
        if not train and margs.deformable:
            mfma = {"live": measure_dense_kernels(device, margs.hidden_dim) if fused.split_linear_enabled() else None,
                    "pmc": committed_mfma_utilisation()}
        if world == 1 and not args.no_cpu_baseline:
            del model
            torch.cuda.empty_cache()
            cpu_baseline = cpu_baseline_in_fresh_process(args)

    ranks = None
    if world > 1:
        from trackformer_amd import dist_utils as du
        seen = du.ranks_seen(device)   # over the job's backend (RCCL): one entry per process
        per_rank = du.gather_results(headline_local)   # each rank's OWN rate over the headline leg: a straggler is visible
        cache_dirs = du.gather_results(os.environ.get("MIOPEN_USER_DB_PATH"))
        ranks = {"world": world, "per_rank_fps": [None if v is None else round(v, 3) for v in per_rank],
                 "cache_dirs": len(set(cache_dirs)), "backend": seen[0].get("backend"), "distinct_devices": len({(r.get("uuid"), r.get("pci_bus_id"), r.get("device")) for r in seen}),
                 "distinct_processes": len({r["pid"] for r in seen}), "cpus_per_rank": [r.get("cpus") for r in seen],
                 "devices": [r.get("name") for r in seen]}
        du.barrier()
        import torch.distributed as dist
        dist.destroy_process_group()

    if rank == 0:
        units_per_step = 2 if train else 1   # cfg 3: 2 images per step and GPU
        steps_timed = args.steps * reps
        value = steps_timed * units_per_step * world / elapsed
        line = {
            "metric": cfg["metric"], "value": round(value, 3), "unit": cfg["unit"], "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / steps_timed, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32" if not fused.split_linear_enabled() or train else _ARITH[fused.split_terms()][2],
            "data": "synthetic", "per_gpu": round(value / world, 3),
            "timed_repeats": reps, "steps_timed": steps_timed, "timed_seconds": round(elapsed, 3),
            "config": {"workload": cfg["name"] + ", seeded random-init weights, frames "
                                   + ("in pinned host memory (PCIe copy timed)" if args.host_frames
                                      else "resident in HBM"),
                       "global_batch": world * (2 if train else 1),
                       "parallelism": ("DDP x%d (RCCL all-reduce)" if train else "sequence-sharded x%d") % world,
                       "sequences_per_gpu": n_seq, "hip_graph": not args.no_graph and not train,
                       **({"pipelined": "the backbone + encoder of the next frames (Tracker.look_ahead: two for a single-frame model "
                                        "without a mask head, else one) are enqueued before the host associates the current frame, "
                                        "on side streams next to the current frame's decoder half (Tracker.step_prepare; results "
                                        "those of step()); the sequence runs on a high-priority stream (dist_utils.sequence_stream)"}
                          if cfg["kind"] == "track" and not args.no_prepare else {}),
                       "linears": (_ARITH[fused.split_terms()][0] + ", f32 accumulate (own kernels)")
                                  if fused.split_linear_enabled() and not train else "f32 (hipBLASLt)",
                       **({"routes": _active_optins(_backbone, fused)} if not train and _active_optins(_backbone, fused) else {}),
                       **({"ffn": "one launch per feed-forward block (tf_ffn_fused_f32)"} if fused.ffn_fused_enabled() and not train else {}),
                       **({"projection_norm": "output projection + residual + LayerNorm in one launch (tf_linear_res_ln_f32)"}
                          if fused.linear_ln_fused_enabled() and not train else {}),
                       **({"mask_head": "lazy: evaluated for the surviving tracks' queries only (Tracker default)"}
                          if "segm" in post and os.environ.get("TF_LAZY_MASKS", "1") != "0" and not train else {})},
            "single_sequence_fps": None if single is None else round(single, 3),
            "multi_sequence_fps": None if multi is None else {"sequences_per_gpu": max(1, args.sequences), "value": round(multi, 3)},
            "step_only_fps": None if step_only is None else round(step_only, 3),
            "host_frames_fps": None if host_frames_fps is None else round(host_frames_fps, 3),
            "plain_step_fps": plain_step,
            "fp32_exact_fps": None if fp32_exact is None else round(fp32_exact, 3),
            "single_sequence_fp32_exact_fps": None if fp32_exact_single is None else round(fp32_exact_single, 3),
            **{_ARITH[a][1]: other_arith.get(_ARITH[a][1]) for a in (6, 16) if a != fused.split_terms() or not fused.split_linear_enabled()},
            "precision": None if train else {
                "value_measured_with": (_ARITH[fused.split_terms()][0] + ", own kernels") if fused.split_linear_enabled()
                                       else "fp32 libraries (hipBLASLt, MIOpen)",
                "fp32_exact_fps": "fp32 libraries (hipBLASLt linears, MIOpen convolutions), --sequences per GPU",
                "single_sequence_fp32_exact_fps": "the same with one sequence per GPU",
                "split6_fps": "six-term bf16 split product: all 24 significand bits of both operands",
                "split_f16_fps": "fp16 split product: three MFMAs per product, 22 + 1 significand bits per operand (include/tf_fused.h)"},
            "association": association, "parity": parity, "ranks": ranks, "mfma_utilisation": mfma,
            "roofline": roofline, "cpu_baseline": cpu_baseline,
        }
        print(json.dumps(line))


if __name__ == "__main__":
    main()
