#!/usr/bin/env python3
"""Headline benchmark: fused frames/s on synthetic 1920x1080 frames + 120k-point clouds.

One step = one pass of the hot path over one frame, inputs already resident in HBM:
    segmentation forward (DeepLabV3+/ResNeXt-50 OS8)  ->  uint8 label map (stays in HBM)
    -> LiDAR projection + label gather + BEV vote + grid update (avl_fused_frame)
Default precision is "mixed" (f16 MFMA on hi+lo split operands, the correction products as MX-FP4 passes on the block-scaled
matrix cores, fp32 accumulate): the mode whose logits stay within north_star's 1e-3 of the reference's fp32 forward on every
weights draw measured (the `parity` block reports the WORST of two weight seeds); `--precision bf16|f16` time the
single-rounding 16-bit modes (faster, 2e-3 .. 2e-2).

N > 1: one process per GPU (torch.distributed, backend nccl = RCCL), one camera stream and one private grid per
rank, no data-path collective per frame; the shared global grid is formed by ONE all-reduce (sum) of the private
grids (float32 payload: 80 MB for the 2000 x 2000 x 5 grid), inside the timed region and also timed on its own
with HIP events (`exchange_ms`, `exchange_bytes`) ("weak" scaling: per-GPU work fixed).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR]
`--dump-outputs DIR` writes what the timed path computed in its last step (rank 0) as DIR/<name>.npy: the label map and
the logits of the network, and the grid after that step as a seeded sample of cells plus its row and column sums (all in
float32 / float64, ~35 MB; `bench_outputs/` is ignored by git).  The inputs are seeded: the same arguments give the same inputs
on every run, so two builds can be compared output for output.
`python bench.py --gpus N` (N > 1, no WORLD_SIZE in the environment) starts its N ranks itself: a child
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...` started BEFORE anything
touches the GPU; its exit code is this process's.  Launched under torch.distributed.run it just runs its rank.

Rank 0 prints ONE JSON line (contract in the task statement) with
  roofline      dominant kernel = the 1x1-conv MFMA GEMM, HIP-event time per launch on the launch stream
  parity        this very workload against the oracle, for two weight seeds (the bench's own and one more): logits / arg-max of
                the network at the benchmarked precision, the grid with the oracle fed ITS OWN labels (end to end: the headline
                field `max_abs_dlogodds_vs_oracle`) and fed the GPU's labels (mapping only: `grid_same_labels_*`); `worst` = the
                worse of the two seeds, field by field
  mapping       the projection / vote / grid-update kernels alone: config C (120k points, 0.2 m) and config E (1M
                points, 0.05 m): GPU microseconds per frame, algorithmic bytes, GB/s and fraction of the 8 TB/s HBM peak
  fps_incl_h2d  the same loop with the frame and the cloud uploaded from pinned host memory every frame (copy stream,
                double-buffered, overlapped with the previous frame)
  cpu_baseline  the NumPy / torch-CPU oracle timed on this box's host cores on the same frame (full size, once).
  robust_plan   the complete hi + lo plan the load-time self-check falls back to (never `value`): its frames/s on this workload and, for two
                checkpoint-LIKE weight draws (heavy-tailed, calibrated BatchNorm statistics), the logits error of the mixed plan and of this one
  roofline.kernels   per kernel family: launches, ms, TFLOP/s, GB/s, bound, fraction of that bound's peak, PMC bytes over algorithmic, MFMA busy
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

H, W, NPTS = 1080, 1920, 120000
GRID_RES, GRID_HALF = 0.2, 200.0          # 2000 x 2000 cells (BASELINE config C / D)
PEAK_MFMA16_TFLOPS = 2500.0               # MI355X dense bf16 / f16 MFMA peak (MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3
PEAK_HBM_GBS = 8000.0
SURVEY_FLOP_PER_FRAME = 1.7768e12          # 888.4 GMAC per 1080 x 1920 forward (whole_frame_frac = this x frames/s/GPU / the f16 MFMA peak)


def self_launch(args):
    """--gpus N without a launcher: start the N ranks as a CHILD process tree (never exec: nothing here has touched the
    GPU yet, and nothing will in this process) and pass their exit code on."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), "--gpus", str(args.gpus), "--steps", str(args.steps), "--warmup",
           str(args.warmup), "--precision", args.precision, "--mixed-opts", args.mixed_opts]
    if args.dump_outputs:
        cmd += ["--dump-outputs", os.path.abspath(args.dump_outputs)]
    if args.no_cpu_baseline:
        cmd.append("--no-cpu-baseline")
    if args.no_other_precisions:
        cmd.append("--no-other-precisions")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--precision", default="mixed", choices=["mixed", "bf16", "f16", "f32"])
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the oracle runs (no parity block, no cpu_baseline)")
    ap.add_argument("--no-other-precisions", action="store_true", help="skip the bf16 / f16 context runs (other_precisions block)")
    ap.add_argument("--mixed-opts", default="", help="comma list of key=0|1 overrides for the mixed mode (conv2_split, mx, trunk_fp4, conv1_split)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the outputs of the last timed step as DIR/<name>.npy (rank 0)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    # the device check, before any other GPU call: a rank without a GPU of its own stops here
    ndev = torch.cuda.device_count()
    if ndev <= local_rank:
        raise SystemExit("bench.py rank %d/%d: needs GPU %d, this box exposes %d GPU(s)" % (rank, world, local_rank, ndev))

    from vision_semantic_segmentation_amd import SemanticMapping, get_cfg_defaults, synthetic as syn
    from vision_semantic_segmentation_amd.camera import camera_setup_1
    from vision_semantic_segmentation_amd.mapping import PCD_ORIGIN_OFFSET
    from vision_semantic_segmentation_amd.network import SegNet, random_state_dict
    from vision_semantic_segmentation_amd.utils.logger import MyLogger

    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    # ---- workload, resident in HBM (each rank its own camera stream: different seed)
    rng = np.random.default_rng(1 + rank)
    cam = camera_setup_1().scaled(1.0, H / 1440.0, imSize=[W, H])
    image_host = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    image = torch.from_numpy(image_host).to(dev)
    cloud = syn.make_cloud(rng, NPTS, cam.K, cam.R, cam.t, W, H)
    points_host = np.ascontiguousarray(cloud.T.astype(np.float32))                            # [N,4] f32 (PointCloud2 layout)
    points = torch.from_numpy(points_host).to(dev)
    cfg = get_cfg_defaults()
    cfg.MAPPING.BOUNDARY = syn.centred_boundary(PCD_ORIGIN_OFFSET[:2], GRID_HALF)
    cfg.MAPPING.RESOLUTION = GRID_RES
    sm = SemanticMapping(cfg, device=dev, logger=MyLogger("bench", quiet=True))
    sm.confusion_matrix = syn.log_confusion(5)
    state = random_state_dict(0)
    mixed_opts = {kv.split("=")[0]: bool(int(kv.split("=")[1])) for kv in args.mixed_opts.split(",") if kv}
    net = SegNet(state, H, W, precision=args.precision, device=dev, **mixed_opts)
    net.image.copy_(image)                 # the frame is resident in the plan's input buffer (HBM)
    net.capture_graph()                    # the plan's ~90 launches replay as one hipGraph launch per frame

    def step():
        labels = net.forward()
        sm.frame_device(points, "velodyne", labels, None, cam, src_kind="classmap", image_size=(H, W))

    def sync():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize(dev)

    ex0, ex1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def exchange():
        """the one exchange step: private grids -> shared grid, ONE RCCL all-reduce of a float32 copy (80 MB)"""
        ex0.record()
        total = sm.global_map(exchange_dtype=torch.float32)
        ex1.record()
        return total

    for _ in range(args.warmup):
        step()
    if world > 1:
        exchange()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    if world > 1:
        shared = exchange()
    sync()
    elapsed = time.perf_counter() - t0
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, net, sm)           # before anything else runs the path again
    exchange_ms, exchange_bytes, per_rank_fps, exchange_sparse = None, None, None, None
    if world > 1:
        own_elapsed = elapsed
        exchange_ms = ex0.elapsed_time(ex1)                 # cast + all-reduce on this rank's stream (the frames before it are queued ahead)
        exchange_bytes = int(shared.numel() * shared.element_size())
        t = torch.tensor([elapsed, exchange_ms], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, exchange_ms = float(t[0].item()), float(t[1].item())
        # outside the timed region: every rank's own frames/s, and the RECORD exchange (all-gather of (cell, delta[C])
        # records, distributed.reduce_grids_sparse) timed beside the dense all-reduce, so one N-GPU run yields the curve and the comparison
        fps_all = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(world)]
        dist.all_gather(fps_all, torch.tensor([args.steps / own_elapsed], dtype=torch.float64, device=dev))
        per_rank_fps = [round(float(f.item()), 2) for f in fps_all]
        sm.global_map(mode="sparse")                        # warm-up (allocations, RCCL channels for the all-gather)
        sync()
        sx0, sx1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sx0.record()
        shared_sparse = sm.global_map(mode="sparse")
        sx1.record()
        sync()
        t2 = torch.tensor([sx0.elapsed_time(sx1)], dtype=torch.float64, device=dev)
        dist.all_reduce(t2, op=dist.ReduceOp.MAX)
        exchange_sparse = {"ms": round(float(t2[0].item()), 3), "bytes_sent_per_rank": sm.last_exchange[1],
                           "max_abs_diff_vs_dense": float((shared_sparse - shared.to(shared_sparse.dtype)).abs().max().item())}

    result = None
    if rank == 0:
        fps = world * args.steps / elapsed
        roofline = gemm_roofline(net, args.precision)
        fps_h2d = fps_with_uploads(net, sm, cam, image_host, points_host, dev, min(args.steps, 60), max(3, min(args.warmup, 10)))
        mapping = mapping_block(dev, rng)
        parity, cpu_baseline, other, robust = None, None, None, None
        if not args.no_cpu_baseline:
            parity, cpu_baseline, logits_ref = parity_and_cpu_baseline(net, state, cfg, sm.confusion_matrix, cam, image, image_host, points,
                                                                       dev, want_baseline=(world == 1))
            # a second weights draw (the logits error follows the weights): same frame, same cloud.  That draw's
            # arg-max map is almost never one of the reference's five map classes (3 cells touched: a vacuous grid check), so ITS five
            # most frequent classes play the five map classes, on both sides
            parity = {"weight_seed_0": parity}
            for seed2 in PARITY_EXTRA_SEEDS:
                st2 = random_state_dict(seed2)
                net2 = SegNet(st2, H, W, precision=args.precision, device=dev, **mixed_opts)
                parity["weight_seed_%d" % seed2] = parity_and_cpu_baseline(net2, st2, cfg, sm.confusion_matrix, cam, image, image_host, points,
                                                                           dev, want_baseline=False, remap_votes=True)[0]
                del net2
                torch.cuda.empty_cache()
            parity["worst"] = worst_parity([v for k, v in parity.items() if k.startswith("weight_seed_")])
            if world == 1 and not args.no_other_precisions:
                other = other_precisions(args.precision, state, cfg, sm.confusion_matrix, cam, image, points, dev, logits_ref)
                robust = robust_plan(state, cfg, sm.confusion_matrix, cam, image, points, dev, logits_ref)
        result = {
            "metric": "fused frames/sec/GPU (1920x1080 + 120k pts) + max|dlog-odds| vs ref",
            "value": round(fps, 2), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": {"mixed": "f16 hi+lo split, MX-FP4 correction passes, fp32 accumulate"}.get(args.precision, args.precision),
            "data": "synthetic", "per_gpu": round(fps / world, 2), "fps_incl_h2d": fps_h2d,
            # end to end: HIP network -> HIP mapping against oracle network -> oracle mapping, worst of the weight seeds checked
            "max_abs_dlogodds_vs_oracle": None if parity is None else parity["worst"]["grid_e2e_max_abs_dlogodds"],
            "grid_e2e_cells_differing_frac": None if parity is None else parity["worst"]["grid_e2e_cells_differing_frac"],
            "grid_same_labels_max_abs_dlogodds": None if parity is None else parity["worst"]["grid_same_labels_max_abs_dlogodds"],
            "logits_max_rel_err_vs_oracle": None if parity is None else parity["worst"]["logits_max_rel_err"],
            # every label pixel whose arg-max differs from the oracle's is a near-tie of the ORACLE's logits: its winner beats the class
            # the GPU picked by at most this much (relative to max|logit|; bounded by 2 x the logits tolerance)
            "flip_margin_max_rel": None if parity is None else parity["worst"]["flip_margin_max_rel"],
            "exchange_ms": None if exchange_ms is None else round(exchange_ms, 3), "exchange_bytes": exchange_bytes,
            "exchange_sparse": exchange_sparse, "per_rank_fps": per_rank_fps,
            "config": {"workload": "configs[2] full fuse: seg 1920x1080 + projection + 0.2 m BEV log-odds update, 120k pts, "
                                   "2000x2000x5 f64 grid; weights random-init ResNeXt50-OS8 DeepLabV3+",
                       "precision": args.precision, "frame": [H, W], "points": NPTS, "grid": [sm.map_height, sm.map_width, sm.map_depth],
                       "parallelism": "frame-parallel x%d, 1 grid all-reduce" % world},
            "roofline": dict(roofline, whole_frame_frac=round(SURVEY_FLOP_PER_FRAME * fps / world / (PEAK_MFMA16_TFLOPS * 1e12), 4)),
            "parity": parity, "mapping": mapping, "cpu_baseline": cpu_baseline,
            "other_precisions": other, "robust_plan": robust,
        }
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return result


DUMP_GRID_CELLS = 500000          # grid cells sampled by --dump-outputs (of 2000 x 2000; x 5 classes x 8 bytes = 20 MB)


def dump_outputs(out_dir, net, sm):
    """--dump-outputs: what a caller of the timed path receives after its last step -- the network's label map and logits,
    and the log-odds grid (float64, 160 MB in full: a fixed seeded sample of cells, and its row / column sums over every cell)."""
    os.makedirs(out_dir, exist_ok=True)
    grid = sm.map
    cells = np.sort(np.random.default_rng(12345).choice(grid.shape[0] * grid.shape[1], size=min(DUMP_GRID_CELLS, grid.shape[0] * grid.shape[1]),
                                                          replace=False))
    outs = {"labels": net.labels.cpu().numpy().astype(np.float32),
            "logits": net.logits.cpu().numpy().astype(np.float32),
            "grid_sample": np.ascontiguousarray(grid.reshape(-1, grid.shape[2])[cells], dtype=np.float64),
            "grid_sample_cells": cells.astype(np.float64),
            "grid_row_sums": grid.sum(axis=1, dtype=np.float64),
            "grid_col_sums": grid.sum(axis=0, dtype=np.float64)}
    for name, a in outs.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return outs


PARITY_EXTRA_SEEDS = (2,)          # weight seed 2 is the worst draw of tools/seed_sweep.py


def worst_parity(blocks):
    """field-by-field worst of several parity blocks (max of the errors and counts, min of the agreement)"""
    out = {}
    for key in ("logits_max_rel_err", "label_pixels_differing", "grid_same_labels_max_abs_dlogodds", "grid_e2e_max_abs_dlogodds",
                "grid_e2e_cells_differing", "grid_e2e_cells_differing_frac", "flip_margin_max_rel", "flip_top2_margin_max_rel"):
        out[key] = max(b[key] for b in blocks)
    out["argmax_agreement"] = min(b["argmax_agreement"] for b in blocks)
    out["grid_cells_touched"] = min(b["grid_cells_touched"] for b in blocks)
    return out


def gemm_roofline(net, precision):
    """Roofline of the dominant kernel (the 1x1-conv GEMM) from per-launch HIP events on the launch stream.  `achieved`
    counts ALGORITHMIC flops (2 M N K per launch); in the mixed mode the matrix cores execute 2 or 3 f16 passes per
    product (MX GEMMs: one f16 pass + one or two FP4 passes of a quarter of the MFMAs each), reported next to it as
    `executed_tflops` in f16-pass equivalents."""
    prof = net.profile()
    for _ in range(2):
        for a, b in zip(prof, net.profile()):
            a["ms"] = min(a["ms"], b["ms"])
    gemm = [(p, op) for p, op in zip(prof, net.ops) if p["kind"] == "gemm"]
    g_ms, g_fl = sum(p["ms"] for p, _ in gemm), sum(p["flops"] for p, _ in gemm)
    def passes(op):          # matrix-pipe work in f16-pass equivalents: an FP4 correction pass issues a quarter of the MFMAs of an f16 one
        if op.w_split == 2:
            return 1.0 + 0.25 * (2 if (op.in_lo or (op.mx_flags & 1)) else 1)
        return (3 if op.in_lo else 2) if op.w_split else 1

    g_exec = sum(p["flops"] * passes(op) for p, op in gemm)
    seg_ms, seg_fl = sum(p["ms"] for p in prof), sum(p["flops"] for p in prof)
    peak = PEAK_F32_TFLOPS if precision == "f32" else PEAK_MFMA16_TFLOPS
    achieved = g_fl / g_ms / 1e9
    traffic, traffic_note = pmc_traffic(len(gemm), precision)
    kernels = kernel_families(prof, net.ops, precision)
    return {"bound": "mfma", "kernel": "k_gemm_mx_pipe (MX GEMMs) / k_gemm_ring / k_gemm: the 1x1 convs, %d launches/frame" % len(gemm), "achieved": round(achieved, 1),
            "kernels": kernels,
            "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_note": traffic_note,
            "executed_tflops": round(g_exec / g_ms / 1e9, 1), "executed_frac": round(g_exec / g_ms / 1e9 / peak, 4),
            "algorithmic_bytes_per_frame": sum(p["bytes"] for p, _ in gemm),
            "flops_per_frame": g_fl, "ms_per_frame": round(g_ms, 4),
            "whole_net": {"gflop_per_frame": round(seg_fl / 1e9, 1), "ms_sum_of_ops": round(seg_ms, 3),
                          "tflops": round(seg_fl / seg_ms / 1e9, 1)}}


PMC_SUMMARIES = [os.path.join("profiles", r, "pmc_seg_summary_%s.json") for r in ("r05", "r04", "r03", "r02")]
OP_FAMILY = {"gconv": ("gconv", "hbm"), "dwpw": ("dwpw", "mfma"), "dwconv": ("dwconv", "hbm"), "bottleneck": ("bottleneck", "mfma")}
KERNEL_FAMILY = (("k_gemm_mx_pipe", "gemm_mx"), ("k_gemm_ring_mx", "gemm_mx"), ("k_gemm", "gemm_ring"), ("k_gconv", "gconv"), ("k_dwpw", "dwpw"),
                 ("k_dwconv", "dwconv"), ("k_bottleneck", "bottleneck"))


def kernel_families(prof, ops, precision):
    """per kernel family of one frame -- launches, HIP-event milliseconds, algorithmic TFLOP/s and GB/s, the
    roofline that bounds the family and the fraction of ITS peak reached; from the committed PMC summary (tools/pmc_seg.sh: separate
    --pmc passes) the HBM traffic over the algorithmic bytes and the matrix cores' busy fraction (SQ_VALU_MFMA_BUSY_CYCLES over kernel
    cycles x 1024 SIMDs).  gemm_mx = 1x1 convs on the MX kernels (f16 + FP4 passes), gemm_ring = the other 1x1 convs, glue = stem,
    pooling, bilinear, sub-sampling, GEMVs, arg-max."""
    fam = {}
    for p, op in zip(prof, ops):
        if p["kind"] == "gemm":
            name, bound = ("gemm_mx" if op.w_split == 2 else "gemm_ring"), "mfma"
        else:
            name, bound = OP_FAMILY.get(p["kind"], ("glue", "hbm"))
        f = fam.setdefault(name, {"family": name, "launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0, "bound": bound})
        f["launches"] += 1
        f["ms"] += p["ms"]
        f["flops"] += p["flops"]
        f["bytes"] += p["bytes"]
    pmc, pmc_file = {}, None
    for rel in PMC_SUMMARIES:
        path = os.path.join(ROOT, rel % precision)
        if os.path.exists(path):
            pmc_file = rel % precision
            for r in json.load(open(path)):
                name = next((f for k, f in KERNEL_FAMILY if r["kernel"].startswith(k)), "glue")
                a = pmc.setdefault(name, {"bytes": 0.0, "launches": 0, "busy": 0.0, "busy_w": 0.0})
                a["bytes"] += (r["fetch_MB_per_launch"] + r["write_MB_per_launch"]) * 1048576.0 * r["launches_profiled"]
                a["launches"] += r["launches_profiled"]
                if r.get("mfma_busy") is not None:          # weighted by the family's matrix instructions
                    w = r.get("mfma_insts_per_launch", 0.0) * r["launches_profiled"] + 1e-9
                    a["busy"] += r["mfma_busy"] * w
                    a["busy_w"] += w
            break
    out = []
    peak_tf = PEAK_F32_TFLOPS if precision == "f32" else PEAK_MFMA16_TFLOPS
    for f in sorted(fam.values(), key=lambda f: -f["ms"]):
        tf, gb = f["flops"] / f["ms"] / 1e9, f["bytes"] / f["ms"] / 1e6
        row = {"family": f["family"], "launches": f["launches"], "ms": round(f["ms"], 4), "tflops": round(tf, 1), "GBps": round(gb, 1), "bound": f["bound"],
               "frac_of_bound_peak": round(tf / peak_tf if f["bound"] == "mfma" else gb / PEAK_HBM_GBS, 4),
               "pmc_over_algorithmic": None, "mfma_busy": None}
        a = pmc.get(f["family"])
        if a and a["launches"]:
            per_frame = a["bytes"] / (a["launches"] / float(f["launches"]))
            row["pmc_over_algorithmic"] = round(per_frame / f["bytes"], 3) if f["bytes"] else None
            row["mfma_busy"] = round(a["busy"] / a["busy_w"], 3) if a["busy_w"] > 1e-6 else None
        out.append(row)
    return {"families": out, "pmc_summary": pmc_file}


def pmc_traffic(n_gemm_launches, precision):
    """HBM bytes per frame moved by the GEMM kernels, from the committed rocprofv3 PMC summary (separate
    --pmc passes for FETCH_SIZE and WRITE_SIZE; FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for
    16-B/lane reads on gfx950).  PMC cannot be collected inside the timed run, so this is read from
    profiles/ (tools/pmc_seg.sh regenerates it); None if no summary for this precision is committed."""
    for rel in (os.path.join("profiles", "r05", "pmc_seg_summary_%s.json" % precision),
                os.path.join("profiles", "r04", "pmc_seg_summary_%s.json" % precision),
                os.path.join("profiles", "r03", "pmc_seg_summary_%s.json" % precision),
                os.path.join("profiles", "r02", "pmc_seg_summary_%s.json" % precision),
                os.path.join("profiles", "r01", "pmc_seg_summary.json") if precision == "bf16" else None):
        if rel and os.path.exists(os.path.join(ROOT, rel)):
            rows = [r for r in json.load(open(os.path.join(ROOT, rel))) if r["kernel"].startswith("k_gemm")]
            forwards = sum(r["launches_profiled"] for r in rows) / float(n_gemm_launches)
            total = sum((r["fetch_MB_per_launch"] + r["write_MB_per_launch"]) * r["launches_profiled"] for r in rows) / forwards
            return round(total * 1048576.0), "bytes per frame over all GEMM launches, " + rel
    return None, "no PMC summary committed for precision %s" % precision


def fps_with_uploads(net, sm, cam, image_host, points_host, dev, steps, warmup):
    """The bench loop with the boundary's host buffers in it: every frame's image (6.2 MB) and cloud (1.9 MB) come from
    pinned host memory on a copy stream into one of two staging buffers while the previous frame computes; the compute
    stream waits for the upload's event, moves the image into the plan's input buffer (device to device) and runs."""
    import torch
    img_pin = torch.from_numpy(image_host).pin_memory()
    pts_pin = torch.from_numpy(points_host).pin_memory()
    stage_img = [torch.empty_like(net.image) for _ in range(2)]
    stage_pts = [torch.empty((points_host.shape[0], 4), dtype=torch.float32, device=dev) for _ in range(2)]
    copy_stream = torch.cuda.Stream(device=dev)
    main = torch.cuda.current_stream(dev)
    up = [torch.cuda.Event() for _ in range(2)]
    done = [torch.cuda.Event() for _ in range(2)]

    def upload(i):
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(done[i % 2])              # the frame that last used this staging pair has finished
            stage_img[i % 2].copy_(img_pin, non_blocking=True)
            stage_pts[i % 2].copy_(pts_pin, non_blocking=True)
            up[i % 2].record(copy_stream)

    def run(n):
        for b in range(2):
            done[b].record(main)
        upload(0)
        for i in range(n):
            if i + 1 < n:
                upload(i + 1)
            main.wait_event(up[i % 2])
            net.image.copy_(stage_img[i % 2], non_blocking=True)
            labels = net.forward()
            sm.frame_device(stage_pts[i % 2], "velodyne", labels, None, cam, src_kind="classmap", image_size=(H, W))
            done[i % 2].record(main)
        torch.cuda.synchronize(dev)

    run(warmup)
    t0 = time.perf_counter()
    run(steps)
    return round(steps / (time.perf_counter() - t0), 2)


def _gpu_us_per_frame(fn, dev, reps=100):
    """GPU time of fn()'s kernels, back to back: the stream is first held busy (a few ms of large fills) so that the host
    runs ahead and the launches queue up; HIP events bracket the reps on the launch stream (torch's current stream).  The fills
    evict the grid from L2 / Infinity Cache, so a few untimed frames run between them and the first event (steady state, as in
    the frame loop)."""
    import torch
    a = torch.empty(1 << 28, device=dev, dtype=torch.float32)          # 1 GiB: one fill ~0.3 ms
    fn()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(30):
        a.fill_(1.0)
    for _ in range(10):
        fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return 1e3 * e0.elapsed_time(e1) / reps


def mapping_block(dev, rng):
    """The mapping kernels alone (projection/gather/grid roofline): config C = this bench's cloud and grid,
    config E = BASELINE configs[4] (1M points, 0.05 m cells, 4000 x 4000 grid)."""
    import torch
    from vision_semantic_segmentation_amd import SemanticMapping, get_cfg_defaults, synthetic as syn
    from vision_semantic_segmentation_amd.camera import camera_setup_1
    from vision_semantic_segmentation_amd.mapping import PCD_ORIGIN_OFFSET
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    cam = camera_setup_1().scaled(1.0, H / 1440.0, imSize=[W, H])
    labels = torch.from_numpy(syn.make_label_map(rng, H // 4 - 4, W // 4 - 4)).to(dev)
    out = {}
    for name, n, res, half in (("C", NPTS, 0.2, 200.0), ("E", 1000000, 0.05, 100.0)):
        cfg = get_cfg_defaults()
        cfg.MAPPING.BOUNDARY = syn.centred_boundary(PCD_ORIGIN_OFFSET[:2], half)
        cfg.MAPPING.RESOLUTION = res
        sm = SemanticMapping(cfg, device=dev, logger=MyLogger("bench", quiet=True))
        sm.confusion_matrix = syn.log_confusion(5)
        cloud = syn.make_cloud(rng, n, cam.K, cam.R, cam.t, W, H)
        pts = torch.from_numpy(np.ascontiguousarray(cloud.T.astype(np.float32))).to(dev)
        fn = lambda: sm.frame_device(pts, "velodyne", labels, None, cam, src_kind="classmap", image_size=(H, W))      # noqa: E731
        us = _gpu_us_per_frame(fn, dev)
        sm.map_dev.zero_()
        fn()
        touched = int((sm.map_dev != 0).any(dim=2).sum().item())
        # 16 B per point (x, y, z, i as f32) + 1 B label gather + U cells x (read + write C doubles) + 8 B of
        # vote-mask set and clear per touched cell
        alg = n * 16 + n * 1 + touched * (2 * sm.map_depth * 8) + touched * 8
        out[name] = {"points": n, "resolution_m": res, "grid": [sm.map_height, sm.map_width, sm.map_depth], "touched_cells": touched,
                     "gpu_us_per_frame": round(us, 2), "algorithmic_bytes": alg, "GBps": round(alg / us / 1e3, 1),
                     "frac_of_hbm_peak": round(alg / us / 1e3 / PEAK_HBM_GBS, 4)}
        del sm
        torch.cuda.empty_cache()
    return out


def other_precisions(default_precision, state, cfg, cm, cam, image, points, dev, logits_ref, steps=30):
    """The same workload in the other MODEL.PRECISION settings, for context next to the headline mode (never `value`):
    fused frames/s over `steps` frames, logits error against the same oracle output, GEMM roofline of that mode."""
    import torch
    from vision_semantic_segmentation_amd import SemanticMapping
    from vision_semantic_segmentation_amd.network import SegNet
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    out = {}
    for prec in ("bf16", "f16"):
        if prec == default_precision:
            continue
        net2 = SegNet(state, H, W, precision=prec, device=dev)
        net2.image.copy_(image)
        net2.capture_graph()
        sm2 = SemanticMapping(cfg, device=dev, logger=MyLogger("bench", quiet=True))
        sm2.confusion_matrix = cm

        def step():
            labels = net2.forward()
            sm2.frame_device(points, "velodyne", labels, None, cam, src_kind="classmap", image_size=(H, W))

        for _ in range(5):
            step()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize(dev)
        fps = steps / (time.perf_counter() - t0)
        logits = net2.logits.permute(2, 0, 1).float().cpu()
        rel = float((logits - logits_ref).abs().max() / logits_ref.abs().max())
        roof = gemm_roofline(net2, prec)
        out[prec] = {"fps": round(fps, 2), "logits_max_rel_err": rel, "gemm_tflops": roof["achieved"], "gemm_frac_of_peak": roof["frac"]}
        del net2, sm2
        torch.cuda.empty_cache()
    return out


def robust_plan(state, cfg, cm, cam, image, points, dev, logits_ref, steps=20):
    """The plan MODEL.MIXED_SELF_CHECK falls back to for a checkpoint the mixed plan cannot hold within 1e-3: the COMPLETE
    hi + lo pipeline, SegNet(full_split=True) = the ladder's "split16" rung.  Same workload: fused frames/s and logits error on the seeded
    weights; then two checkpoint-LIKE weight draws (oracle/checkpoint_like.py: heavy-tailed BatchNorm scales, calibrated running
    statistics) at 320 x 416 through the mixed plan and through this one, against the torch-CPU oracle.  Never `value`."""
    import torch
    from oracle import network_oracle as no
    from oracle.checkpoint_like import heavy_tailed_state_dict
    from vision_semantic_segmentation_amd import SemanticMapping
    from vision_semantic_segmentation_amd.network import SegNet
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    net2 = SegNet(state, H, W, precision="mixed", device=dev, full_split=True)
    net2.image.copy_(image)
    net2.capture_graph()
    sm2 = SemanticMapping(cfg, device=dev, logger=MyLogger("bench", quiet=True))
    sm2.confusion_matrix = cm

    def step():
        labels = net2.forward()
        sm2.frame_device(points, "velodyne", labels, None, cam, src_kind="classmap", image_size=(H, W))

    for _ in range(5):
        step()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize(dev)
    fps = steps / (time.perf_counter() - t0)
    logits = net2.logits.permute(2, 0, 1).float().cpu()
    out = {"plan": "split16 (SegNet(full_split=True)): every tensor two f16 planes, every product three f16 passes, no FP4", "fps": round(fps, 2),
           "logits_max_rel_err_seeded_weights": float((logits - logits_ref).abs().max() / logits_ref.abs().max()), "checkpoint_like": []}
    del net2, sm2
    torch.cuda.empty_cache()
    h, w = 320, 416
    for ws in (0, 1):
        st = heavy_tailed_state_dict(ws)
        img = np.random.default_rng(50 + ws).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        ref = no.forward_logits(st, img)[0]
        row = {"weights": "heavy_tailed_state_dict(%d)" % ws, "frame": [h, w]}
        for name, opts in (("mixed", {}), ("split16", {"full_split": True})):
            net3 = SegNet(st, h, w, precision="mixed", device=dev, **opts)
            net3.forward(torch.from_numpy(img).to(dev))
            got = net3.logits.permute(2, 0, 1).float().cpu()
            row[name + "_logits_max_rel_err"] = float((got - ref).abs().max() / ref.abs().max())
            row[name + "_argmax_agreement"] = float((got.argmax(0) == ref.argmax(0)).float().mean())
            del net3
            torch.cuda.empty_cache()
        out["checkpoint_like"].append(row)
    return out


def flip_margins(logits_ref, labels_ref, labels_gpu):
    """Where the GPU's arg-max differs from the oracle's: by how much does the ORACLE's winner beat (a) the class the GPU picked,
    (b) its own runner-up, relative to max|logit| (vision_semantic_segmentation_node.py:101-102 commits to a label there).  With
    logits within eps of the oracle's, (b) <= (a) <= 2 eps: a flip can only be a near-tie.  Returns (a, b) maxima; (0, 0) without flips."""
    lr = logits_ref.numpy() if hasattr(logits_ref, "numpy") else np.asarray(logits_ref)
    flip = labels_ref != labels_gpu
    if not flip.any():
        return 0.0, 0.0
    scale = float(np.abs(lr).max())
    cols = lr[:, flip]                                        # [19, flips]
    top = np.sort(cols, axis=0)
    picked = cols[labels_gpu[flip].astype(np.int64), np.arange(cols.shape[1])]
    return float((top[-1] - picked).max() / scale), float((top[-1] - top[-2]).max() / scale)


def host_threads():
    """(os.cpu_count(), BLAS threads of NumPy's backend) for the cpu_baseline block"""
    blas = None
    try:
        from threadpoolctl import threadpool_info
        blas = max([int(i.get("num_threads", 0)) for i in threadpool_info() if i.get("user_api") == "blas"] or [0]) or None
    except Exception:
        pass
    return os.cpu_count(), blas


def parity_and_cpu_baseline(net, state, cfg, cm, cam, image, image_host, points, dev, want_baseline, remap_votes=False):
    """Parity of this very workload.  The oracle network (torch CPU fp32) runs ONCE on the full 1080 x 1920 frame: its
    logits check the GPU's, its own arg-max feeds the oracle mapping, and its wall time is the network half of the CPU
    baseline.  remap_votes: the five most frequent classes of the oracle's label map take the roles of the reference's five map
    classes (LABEL_COLORS = their palette colours, on both sides), so that a weights draw whose arg-max never hits
    LABELS = [2, 1, 8, 10, 3] still votes into > 10 000 cells."""
    import torch
    from oracle import mapping_oracle as mo
    from oracle import network_oracle as no
    from vision_semantic_segmentation_amd import SemanticMapping
    from vision_semantic_segmentation_amd.utils.logger import MyLogger
    labels_gpu = net.forward(image).clone()
    logits_gpu = net.logits.permute(2, 0, 1).float().cpu()
    no.forward_logits(state, image_host[:96, :128])          # warm-up (thread pool, allocator)
    t0 = time.perf_counter()
    logits_ref = no.forward_logits(state, image_host)[0]
    t_net = time.perf_counter() - t0
    labels_ref = logits_ref.argmax(0).numpy().astype(np.uint8)
    label_colors, vote_classes = mo.LABEL_COLORS, list(mo.LABELS)
    if remap_votes:
        counts = np.bincount(labels_ref.ravel(), minlength=19)
        vote_classes = [int(c) for c in np.argsort(-counts, kind="stable")[:5]]
        label_colors = [list(mo.PALETTE_19[c]) for c in vote_classes]
    sm2 = SemanticMapping(cfg, device=dev, logger=MyLogger("bench", quiet=True))
    sm2.confusion_matrix = cm
    sm2.label_colors = np.array(label_colors)
    sm2.frame_device(points, "velodyne", labels_gpu, None, cam, src_kind="classmap", image_size=(H, W))
    grid_gpu = sm2.map
    rel = float((logits_gpu - logits_ref).abs().max() / logits_ref.abs().max())
    labels_gpu_h = labels_gpu.cpu().numpy()
    agree = float((labels_ref == labels_gpu_h).mean())
    margin_picked, margin_top2 = flip_margins(logits_ref, labels_ref, labels_gpu_h)
    ocfg = dict(range_max=100.0, boundary=cfg.MAPPING.BOUNDARY, resolution=GRID_RES, label_names=mo.LABELS_NAMES,
                label_colors=label_colors, confusion_matrix=cm, use_pcd_intensity=True)
    pcd64 = points.cpu().numpy().T.astype(np.float64)

    def oracle_grid(lab):
        sem = mo.semantic_image_from_labels(lab, H, W)
        grid = np.zeros(grid_gpu.shape)
        mo.mapping_frame(grid, pcd64, "velodyne", sem, None, cam.P, ocfg)
        return grid, sem

    grid_own, sem_own = oracle_grid(labels_ref)                # oracle network -> oracle mapping (end to end)
    grid_same, _ = oracle_grid(labels_gpu_h)                   # oracle mapping fed the GPU's label map (mapping only)
    d_e2e = np.abs(grid_gpu - grid_own)
    parity = {
        "precision": net.precision, "logits_max_rel_err": rel, "argmax_agreement": agree,
        "label_pixels_differing": int((labels_ref != labels_gpu_h).sum()),
        "flip_margin_max_rel": margin_picked, "flip_top2_margin_max_rel": margin_top2,
        "grid_same_labels_max_abs_dlogodds": float(np.max(np.abs(grid_gpu - grid_same))),
        "grid_e2e_max_abs_dlogodds": float(d_e2e.max()), "grid_e2e_cells_differing": int((d_e2e.max(axis=2) > 0).sum()),
        "grid_cells_touched": int((grid_own != 0).any(axis=2).sum()), "vote_classes": vote_classes,
        "grid_e2e_cells_differing_frac": float((d_e2e.max(axis=2) > 0).sum()) / max(1, int((grid_own != 0).any(axis=2).sum())),
        "note": "e2e = HIP network -> HIP mapping against oracle network -> oracle mapping; a grid cell differs only where a LiDAR "
                "point lands on one of the label pixels whose arg-max flipped; every such pixel is a near-tie of the oracle's own "
                "logits (flip_margin_max_rel <= 2 x the logits tolerance)",
    }
    baseline = None
    if want_baseline:
        # NumPy restatement of a7 + a8 on the same inputs, 1 process, min of >= 5 repetitions after 3 warm-ups
        times = []
        for rep in range(8):
            grid = np.zeros(grid_gpu.shape)
            t = time.perf_counter()
            mo.mapping_frame(grid, pcd64, "velodyne", sem_own, None, cam.P, ocfg)
            if rep >= 3:
                times.append(time.perf_counter() - t)
        t_map = min(times)
        ncpu, blas = host_threads()
        baseline = {"value": round(1.0 / (t_net + t_map), 4), "unit": "frames/s", "cores": torch.get_num_threads(), "kind": "port",
                    "host_cpu_count": ncpu, "blas_threads": blas, "network_s": round(t_net, 3), "mapping_ms": round(1e3 * t_map, 2),
                    "sample": "one full 1080x1920 frame + 120k points: oracle network (torch CPU fp32, %d threads, once after a small warm-up "
                              "frame) %.2f s, oracle mapping (NumPy, 1 process, BLAS threads %s, min of %d after 3 warm-ups) %.1f ms; "
                              "os.cpu_count() = %s" % (torch.get_num_threads(), t_net, blas, len(times), 1e3 * t_map, ncpu)}
    return parity, baseline, logits_ref


if __name__ == "__main__":
    main()
