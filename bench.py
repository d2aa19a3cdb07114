#!/usr/bin/env python3
"""bench.py -- S2ANet-R50-FPN training throughput (1024x1024 tiles/s) on MI355X.

Contract (driver):  python bench.py --gpus N --steps K --warmup W
  N>1 is launched by the driver through torch.distributed.run (one rank per GPU, RCCL).
  Prints ONE JSON line from rank 0.
  --dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step returned (total loss + loss terms)
  and a seeded sample of the parameters it left as DIR/<name>.npy; the inputs are seeded, so two builds can be compared.

A "step" = one full training step of BASELINE.json configs[1]: S2ANet-R50-FPN, 4 synthetic
1024x1024 DOTA-shaped tiles per GPU, fp32: backbone+FPN (MIOpen), S2ANetHead with the
hand-written HIP hot path (fused refine+offset, deformable im2col/col2im, ARF, batched rotated
IoU + MaxIoU assignment), focal/smooth-L1 losses, backward, RCCL gradient all-reduce (DDP),
grad-clip 35, SGD update.  Inputs (tiles and targets) are resident in HBM before the timed
region.  Weak scaling: 4 tiles per GPU at every N.

Extra objects on the same JSON line (kept under 8 KB: the driver's record truncates longer lines):
  roofline      the oriented-box call the timed step makes (fused anchor targets), HIP-event timed in
                this process; roofline_dense_iou / roofline_dense_iou_two_tier / roofline_nms beside it
  kernels_top12 {us, frac, bound} of 12 hand-written kernels (the conv3x3 MFMA rows, then by time per call); the full table
                goes to kernels_file (gpurun_out/bench_kernels.json or ./bench_kernels.json) and stderr
  bf16, bf16_*  the second timed leg (bf16 autocast, channels_last) and its flat scalars
  fresh_k*      a short leg on never-seen gt-count tuples (what --fresh-k times in full)
  host_enqueue_ms_per_step   host time to enqueue a step (== ms_per_step: the host paces the GPU)
  cpu_baseline  the reference's own CPU rotated-IoU source (oracle/_ref, kind "reference";
                falls back to the oracle restatement, kind "port") on this box's host cores
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
# MIOpen find mode (honoured if already set).  With the packaged solver records (rs_detection_amd/miopen_db, see
# utils/miopen_db.py) FAST answers from those records for every shipped config in seconds.  Without them
# (RSDET_NO_MIOPEN_DB=1 or another MIOpen build) FAST equals NORMAL for the S2ANet line (64.5 vs 64.4 ms/step) but
# lands on im2col+GEMM convolutions for the VAN backbone of --model orcnn_van3 (347 vs 157 ms/step): NORMAL there.
_no_db = os.environ.get("RSDET_NO_MIOPEN_DB", "0") == "1"
os.environ.setdefault("MIOPEN_FIND_MODE", "NORMAL" if ("orcnn_van3" in sys.argv and _no_db) else "FAST")

import numpy as np  # noqa: E402
import torch  # noqa: E402

# tuned MIOpen solver records for the shipped configs (rs_detection_amd/miopen_db, 140 KB of text): see the module
from rs_detection_amd.utils.miopen_db import use_packaged_miopen_db  # noqa: E402
MIOPEN_DB_DIR = use_packaged_miopen_db()

torch.backends.cudnn.benchmark = os.environ.get("RSDET_CUDNN_BENCHMARK", "0") == "1"
if os.environ.get("RSDET_BLAS_LIB"):  # A/B switch: "hipblas" (rocBLAS) or "hipblaslt"
    torch.backends.cuda.preferred_blas_library(os.environ["RSDET_BLAS_LIB"])

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md: 8.0 TB/s; ~6.3 TB/s achievable)
TILE = int(os.environ.get("RSDET_BENCH_TILE", "1024"))  # 1024 = the metric; smaller only for the self-launch test (named in config.workload)
BATCH_PER_GPU = 4


def s2anet_cfg():
    """configs/s2anet/s2anet_r50_fpn_1x_dota.py of the reference, model + optimiser part
    (kept in-repo as data so the GPU box needs no /root/reference)."""
    from rs_detection_amd.config import Config
    return Config(os.path.join(ROOT, "configs", "s2anet", "s2anet_r50_fpn_1x_dota.py"))


FP32_VALU_PEAK_TFLOPS = 157.3  # MI355X fp32 vector peak (MI355X_MICROARCH.md)
WORKLOADS = {
    "s2anet_r50": "S2ANet-R50-FPN train step, %d x %dx%d DOTA-shaped tiles per GPU, %s, K gts/tile cycle "
                  "[16,100,400,40], one anchor per cell over strides 8..128 (A=21824 per 1024^2 tile)",
    "s2anet_r101": "S2ANet-R101-FPN (s2anet_r101_fpn_1x_dota_rotate_balance_ms) train step, %d x %dx%d DOTA-shaped "
                   "tiles per GPU, %s, K gts/tile cycle [16,100,400,40], A=21824 per 1024^2 tile",
    "orcnn_van3": "Oriented R-CNN + VAN-B3 (orcnn_van3_7_anchor) train step, %d x %dx%d tiles per GPU, %s, K gts/tile "
                  "cycle [16,100,400,40], 10 classes, 2000 proposals/tile -> 512 sampled RoIs",
}
METRICS = {"s2anet_r50": "1024x1024 tiles/sec S2ANet-R50-FPN train", "s2anet_r101": "1024x1024 tiles/sec S2ANet-R101-FPN train",
           "orcnn_van3": "1024x1024 tiles/sec Oriented-RCNN VAN-B3 train"}


def event_time(fn, iters, warmup=3, graph=True):
    """Average device time of fn() in seconds: HIP events on torch's current stream (the stream every
    rsdet_* launch goes to) around a replayed hipGraph of `iters` calls, so that the host-side cost of the
    ctypes call / torch.empty (10-25 us, comparable to these kernels) is not billed to the kernel."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if graph:
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(iters):
                    fn()
            g.replay()
            torch.cuda.synchronize()
            s.record()
            g.replay()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) * 1e-3 / iters
        except Exception:  # capture not possible (e.g. an op syncs): fall back to eager timing
            torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e-3 / iters


ROOFLINE_FILE = next((f for f in (os.path.join(ROOT, "profiles", "r%02d_roofline.json" % r) for r in (6, 5, 4, 3, 2))
                      if os.path.exists(f)), os.path.join(ROOT, "profiles", "r05_roofline.json"))
# `traffic` (PMC bytes) and `issue` (SQ counters) of the roofline objects are NOT measured by this process (rocprofv3
# counter passes cannot run inside it): they are read from the committed counter table and labelled so in the line
COUNTER_SOURCE = "committed profile: profiles/%s (rocprofv3 --pmc passes of profiles/scripts/roofline.sh)" % \
    os.path.basename(ROOFLINE_FILE)
FAST_ROW = "box_iou_rotated_fast(two-tier clipper, 1 launch; prepared anchors cached, gts prepared in the tile)"
AT_ROW = "anchor_target_rotated(fused: IoU + assign + encode + weights; 2 launches)"
BN_ROW = "bn_act_forward_kernel<f32>(bn + residual + relu; 4x256x256x256, NCHW)"
BN_ROW_CL = "bn_act_forward_nhwc_kernel<f32>(bn + residual + relu; 4x256x256x256, layer1 of the channels_last step)"
NMS_ROW = "nms_rotated(3 kernels; label-major order, as ml_nms_rotated calls it)"


def issue_side():
    """VALU / latency side of the calls whose HBM fraction says nothing (anchor targets, NMS, the dense two-tier IoU):
    VALU instructions issued / issue slots of the launch, waiting share, from the SQ-counter passes committed in
    profiles/ (`issue` object of the roofline file, written by profiles/scripts/roofline.py) -- never a literal here."""
    if not os.path.exists(ROOFLINE_FILE):
        return {}
    with open(ROOFLINE_FILE) as f:
        return json.load(f).get("issue", {})


def pmc_traffic(call, shape_ok):
    """HBM bytes per launch of a C-ABI call from the committed counter table (profiles/r02_roofline.json, produced by
    profiles/scripts/roofline.sh: rocprofv3 --pmc WRITE_SIZE / FETCH_SIZE passes + kernel trace + code-object notes of
    the same kernels at the same shapes) -- never a literal in this file.  None when the table is absent or the shape
    differs from the one it was measured at."""
    if not shape_ok or not os.path.exists(ROOFLINE_FILE):
        return None
    with open(ROOFLINE_FILE) as f:
        c = json.load(f).get("calls", {}).get(call)
    return c["traffic_bytes"] if c else None


def kernel_rooflines(device, targets):
    """HIP-event timing of each hand-written kernel at the shapes of this very step."""
    from rs_detection_amd import ops
    from rs_detection_amd.utils import synthetic as syn
    out = {}
    anchors = torch.from_numpy(syn.s2anet_anchor_grid()).to(device)
    A = anchors.shape[0]
    ks = [int(t["rboxes"].shape[0]) for t in targets]
    gt = torch.cat([t["rboxes"] for t in targets]).to(device)
    lab = torch.cat([t["labels"] for t in targets]).to(device).int()
    ro = torch.tensor(np.concatenate([[0], np.cumsum(ks)]), dtype=torch.int32, device=device)
    n1 = sum(ks)
    ov = torch.empty((n1, A), device=device)

    # -- batched rotated IoU (a1): bytes = 20*(N1+N2) + 4*N1*N2
    t = event_time(lambda: ops.box_iou_rotated_grouped(gt, ro, max(ks), anchors, out=ov), 50)
    by = 20 * (n1 + A) + 4 * n1 * A
    # SURVEY 8d also asks for the VALU view: the reference's algorithm costs ~0.3 kFLOP for a disjoint pair and
    # ~0.8 kFLOP for an overlapping one; "valu_frac" prices THOSE flops (not the ones the early-outs leave) against
    # the fp32 vector peak, i.e. how far the call is beyond a kernel that ran the clipper on every pair.
    nz = int((ov != 0).sum())
    alg_flops = 300.0 * (n1 * A - nz) + 800.0 * nz
    out["box_iou_rotated(prepare+filter+clip)"] = dict(bound="hbm", achieved=by / t / 1e9, peak=HBM_PEAK_GBS, unit="GB/s",
                                         frac=by / t / 1e9 / HBM_PEAK_GBS,
                                         traffic=pmc_traffic("box_iou_rotated (3 launches)", (n1, A) == (556, 21824)),
                                         us=t * 1e6,
                                         mpairs_per_s=n1 * A / t / 1e6, shape="sumK=%d x A=%d (B=%d)" % (n1, A, len(ks)),
                                         overlapping_pairs=nz, alg_gflop=alg_flops / 1e9,
                                         valu_frac=alg_flops / t / 1e12 / FP32_VALU_PEAK_TFLOPS)
    # -- the same matrix in ONE launch (csrc/anchor_target.hip: each 16 x 256 tile detected, zero-filled and clipped by
    #    the workgroup that owns it), prepared anchors cached as the FAM grid's are
    prep = ops.prepare_boxes(anchors, cache=True)
    pgt = ops.prepare_boxes(gt, heavy_from=n1)
    t1 = event_time(lambda: ops.box_iou_rotated_tiled(gt, anchors, ro, ks=ks, out=ov, prepared=prep, prepared1=pgt), 50)
    out["box_iou_rotated_tiled(1 launch; prepared anchors cached)"] = dict(
        bound="hbm", achieved=by / t1 / 1e9, peak=HBM_PEAK_GBS, unit="GB/s", frac=by / t1 / 1e9 / HBM_PEAK_GBS,
        traffic=pmc_traffic("box_iou_rotated_tiled (1 launch)", (n1, A) == (556, 21824)), us=t1 * 1e6)
    # -- the same matrix with the two-tier clipper (csrc/iou_fast.hip): Green integral on every overlapping pair, the
    #    reference-order clipper only where the reference itself is fragile / for exact zeros; |value - exact| < 3e-6
    t3 = event_time(lambda: ops.box_iou_rotated_fast(gt, anchors, ro, ks=ks, out=ov, prepared=prep), 50)
    out[FAST_ROW] = dict(
        bound="hbm", achieved=by / t3 / 1e9, peak=HBM_PEAK_GBS, unit="GB/s", frac=by / t3 / 1e9 / HBM_PEAK_GBS,
        traffic=pmc_traffic("box_iou_rotated_fast (1 launch)", (n1, A) == (556, 21824)), us=t3 * 1e6,
        mpairs_per_s=n1 * A / t3 / 1e6)
    # -- what the train step runs since round 2: fused sparse anchor targets (IoU of the overlapping pairs only ->
    #    assignment -> encode -> weights / counts, no matrix): bytes = boxes in + 56 B of targets per anchor out
    t2 = event_time(lambda: ops.anchor_target_rotated(anchors, gt, lab, ro, ks, 0.5, 0.4, 0.0, prepared=prep,
                                                      prepared_gt=pgt), 50)
    by2 = 20 * (n1 + A) + 56 * len(ks) * A
    out[AT_ROW] = dict(
        bound="latency/alu", achieved=by2 / t2 / 1e9, peak=HBM_PEAK_GBS, unit="GB/s", frac=by2 / t2 / 1e9 / HBM_PEAK_GBS,
        traffic=pmc_traffic("anchor_target_rotated (2 launches)", (n1, A) == (556, 21824)), us=t2 * 1e6,
        replaces="box_iou_rotated_grouped + assign_wrt_overlaps + ~15 torch kernels of anchor_target_batched")
    # -- assignment (a4): two passes over the matrix + outputs
    t = event_time(lambda: ops.assign_wrt_overlaps(ov, ro, max(ks), 0.5, 0.4, 0.0, True, True, lab, 0), 50)
    by = 2 * 4 * n1 * A + 12 * len(ks) * A
    out["assign_row+col_kernel"] = dict(bound="hbm", achieved=by / t / 1e9, peak=HBM_PEAK_GBS, unit="GB/s",
                                        frac=by / t / 1e9 / HBM_PEAK_GBS, us=t * 1e6,
                                        traffic=pmc_traffic("assign_wrt_overlaps", (n1, A) == (556, 21824)))
    # -- deformable im2col / col2im at pyramid level 0 (a11): bytes = 4*(C*HW*B + 18*HW*B + 9*C*HW*B)
    B, C, H = len(ks), 256, TILE // 8
    x = torch.randn(B, C, H, H, device=device)
    off = torch.randn(B, 18, H, H, device=device)
    t = event_time(lambda: ops.deformable_im2col(x, off, (3, 3), (1, 1), (1, 1), (1, 1)), 10, 2)
    by = 4 * (C * H * H * B + 18 * H * H * B + 9 * C * H * H * B)
    out["deform_im2col_kernel"] = dict(bound="hbm", achieved=by / t / 1e9, peak=HBM_PEAK_GBS, unit="GB/s",
                                       frac=by / t / 1e9 / HBM_PEAK_GBS, us=t * 1e6,
                                       traffic=pmc_traffic("deform_im2col", (B, C, H) == (4, 256, 128)))
    # AlignConv as an implicit GEMM on the matrix cores (csrc/alignconv_mfma.hip): 2*B*HW*O*9*C flops; SURVEY 8(d)'s
    # fused-variant bytes (no 9*C column term) for the HBM view.  bf16: gather-bound; fp32: bound by the fp32 MFMA rate
    from rs_detection_amd import _lib as _L
    lib_ = _L.load()
    O_ = 256
    geom = _L.DcnGeom(C, H, H, 3, 3, 1, 1, 1, 1, 1, 1, B, 1)
    fl = 2.0 * B * H * H * O_ * 9 * C
    for name, dt, entry, peak in (("bf16", torch.bfloat16, lib_.rsdet_alignconv_fwd_mfma_bf16, 2500.0),
                                  ("f32", torch.float32, lib_.rsdet_alignconv_fwd_mfma_f32, 157.3)):
        xq = x.permute(0, 2, 3, 1).contiguous().to(dt)
        wq = (torch.randn(O_, 9 * C, device=device) / 48).to(dt)
        oq = torch.empty((B, H, H, O_), dtype=dt, device=device)
        t = event_time(lambda: entry(_L.ptr(xq), _L.ptr(off), _L.ptr(wq), geom, O_, 1, _L.ptr(oq), None,
                                     _L.stream_ptr()), 10, 2)
        es = xq.element_size()
        by_f = es * (C * H * H * B + O_ * H * H * B + O_ * 9 * C) + 4 * 18 * H * H * B
        out["alignconv_fwd_mfma_kernel<%s>(implicit GEMM, level 0, no columns in HBM)" % name] = dict(
            bound="mfma", achieved=fl / t / 1e12, peak=peak, unit="TFLOP/s", frac=fl / t / 1e12 / peak, us=t * 1e6,
            hbm_alg_bytes=by_f, traffic=pmc_traffic("alignconv_mfma_" + name, (B, C, H) == (4, 256, 128)))
    # the bf16 3x3 implicit GEMM of the head's tower convolutions on the pyramid canvas of this tile size
    # (csrc/conv3x3_mfma.hip): plain, and with bias + ReLU + gap mask in the epilogue (what the step launches)
    from rs_detection_amd.ops.pyramid import canvas_layout
    lay = canvas_layout([(TILE // s_, TILE // s_) for s_ in (8, 16, 32, 64, 128)], device)
    xc = torch.randn(B, C, lay.Hc, lay.Wc, device=device).bfloat16().contiguous(memory_format=torch.channels_last)
    wc = (torch.randn(O_, C, 3, 3, device=device) * 0.05).bfloat16().contiguous(memory_format=torch.channels_last)
    bc = torch.randn(O_, device=device)
    oc = torch.empty((B, O_, lay.Hc, lay.Wc), dtype=torch.bfloat16, device=device, memory_format=torch.channels_last)
    xcs = [xc] + [torch.randn_like(xc) for _ in range(3)]
    ocs = [oc] + [torch.empty_like(oc) for _ in range(3)]
    turn = [0]
    if lib_.rsdet_conv3x3_mfma_supported(B, lay.Hc, lay.Wc, C, O_):
        flc = 2.0 * B * lay.Hc * lay.Wc * O_ * 9 * C
        byc = 2 * (B * lay.Hc * lay.Wc * (C + O_) + 9 * C * O_)
        # operands rotated over four buffer sets (4 x 100 MB > the 256 MB Infinity Cache): ten back-to-back launches on ONE
        # set keep it cache-resident and read 10-20 % faster than the kernel does in the step or under rocprofv3 -- the gap
        # between this table and profiles/r05_roofline.json that VERDICT round 5 pointed at
        for tag, args in (("plain", (None, None, 0)), ("bias+ReLU+gap mask fused", (_L.ptr(bc), _L.ptr(lay.live), 1))):
            def conv_once():
                i = turn[0] & 3
                turn[0] += 1
                return lib_.rsdet_conv3x3_fwd_mfma_bf16(_L.ptr(xcs[i]), _L.ptr(wc), args[0], args[1], B, lay.Hc, lay.Wc, C, O_,
                                                        args[2], _L.ptr(ocs[i]), _L.stream_ptr())
            t = event_time(conv_once, 12, 4)
            out["conv3x3_fwd_mfma_bf16_kernel(head canvas %dx%dx%dx%d, %s)" % (B, lay.Hc, lay.Wc, C, tag)] = dict(
                bound="mfma", achieved=flc / t / 1e12, peak=2500.0, unit="TFLOP/s", frac=flc / t / 1e12 / 2500.0,
                us=t * 1e6, hbm_alg_bytes=byc, traffic=pmc_traffic("conv3x3_mfma bf16 (head canvas 4x128x196x256)", (B, C, lay.Wc) == (4, 256, 196)))
    # ... and its weight gradient (csrc/conv3x3_wrw_mfma.hip: split-K main launch + fold), same canvas
    if lib_.rsdet_conv3x3_wrw_mfma_supported(B, lay.Hc, lay.Wc, C, O_):
        gc = torch.randn(B, O_, lay.Hc, lay.Wc, device=device).bfloat16().contiguous(memory_format=torch.channels_last)
        gwc = torch.empty((O_, C, 3, 3), dtype=torch.bfloat16, device=device, memory_format=torch.channels_last)
        nbw = lib_.rsdet_conv3x3_wrw_mfma_ws_size(B, lay.Hc, lay.Wc, C, O_)
        wsw = torch.empty((nbw,), dtype=torch.uint8, device=device)
        gcs = [gc] + [torch.randn_like(gc) for _ in range(3)]

        def wrw_once():
            i = turn[0] & 3
            turn[0] += 1
            return lib_.rsdet_conv3x3_wrw_mfma_bf16(_L.ptr(gcs[i]), _L.ptr(xcs[i]), B, lay.Hc, lay.Wc, C, O_, _L.ptr(gwc), 1,
                                                    _L.ptr(wsw), nbw, _L.stream_ptr())
        t = event_time(wrw_once, 12, 4)
        out["conv3x3_wrw_mfma_bf16_kernel+fold(head canvas %dx%dx%dx%d, 2 launches)" % (B, lay.Hc, lay.Wc, C)] = dict(
            bound="mfma", achieved=flc / t / 1e12, peak=2500.0, unit="TFLOP/s", frac=flc / t / 1e12 / 2500.0, us=t * 1e6,
            hbm_alg_bytes=2 * (B * lay.Hc * lay.Wc * (C + O_) + 9 * C * O_),
            traffic=pmc_traffic("conv3x3_wrw_mfma bf16 (head canvas 4x128x196x256, 2 launches)", (B, C, lay.Wc) == (4, 256, 196)))
        del gc, gcs, gwc, wsw
    del xc, wc, oc
    xcs = ocs = None
    # (the reference-layout col2im -- one lane per column row, 13.2 ms here -- is kept for API parity only; the step
    #  uses the channels-last pair below, so it is not timed: it would dominate the rocprof summary of this command)
    xn = x.permute(0, 2, 3, 1).contiguous()
    t = event_time(lambda: ops.deformable_im2col_nhwc(xn, off, (3, 3), (1, 1), (1, 1), (1, 1)), 10, 2)
    out["deform_im2col_nhwc_kernel"] = dict(bound="hbm", achieved=by / t / 1e9, peak=HBM_PEAK_GBS, unit="GB/s",
                                            frac=by / t / 1e9 / HBM_PEAK_GBS, traffic=None, us=t * 1e6)
    colT = ops.deformable_im2col_nhwc(xn, off, (3, 3), (1, 1), (1, 1), (1, 1))
    t = event_time(lambda: ops.deformable_col2im_nhwc(colT, off, xn.shape, (3, 3), (1, 1), (1, 1), (1, 1)), 10, 2)
    out["deform_col2im_nhwc_kernel(atomics; several deformable groups only)"] = dict(
        bound="hbm(atomics)", achieved=by / t / 1e9, peak=HBM_PEAK_GBS, unit="GB/s", frac=by / t / 1e9 / HBM_PEAK_GBS,
        traffic=None, us=t * 1e6)
    from rs_detection_amd.ops.dcn_v1 import deformable_col2im_gather_nhwc
    t = event_time(lambda: deformable_col2im_gather_nhwc(colT, off, xn.shape, (3, 3), (1, 1), (1, 1), (1, 1)), 10, 2)
    out["dcn_idx_count+scan+fill+dcn_gather(col2im of the step)"] = dict(
        bound="hbm", achieved=by / t / 1e9, peak=HBM_PEAK_GBS, unit="GB/s", frac=by / t / 1e9 / HBM_PEAK_GBS,
        us=t * 1e6,
        traffic=pmc_traffic("deform_col2im (gather form, 5 launches)", (B, C, H) == (4, 256, 128)))
    del colT, xn, x, off
    # -- rotated NMS (a16), SURVEY 8d micro-bench shape M=5344, 6 columns (15 classes), thr 0.1.  Timed the way the
    #    class-aware entry points call it (ops.ml_nms_rotated: label-major order, one concurrent sweep per label run)
    #    and, for reference, in plain score order through one sweep.
    d, s, l = syn.nms_cluster_boxes(5344)
    d6 = torch.from_numpy(np.concatenate([d, l[:, None].astype(np.float32)], 1)).to(device)
    sc, lab = torch.from_numpy(s).to(device), torch.from_numpy(l).to(device)
    from rs_detection_amd.ops.nms_rotated import _label_major_order
    lorder = _label_major_order(sc, lab).int()
    order = torch.argsort(sc, descending=True, stable=True).int()
    M = 5344
    by = 4 * 6 * M + 2 * 8 * M * ((M + 63) // 64) + M
    cnt = np.bincount(l.astype(np.int64))
    same_cls = int((cnt * (cnt - 1) // 2).sum())
    for name, fn in (("nms_rotated(3 kernels; label-major order, as ml_nms_rotated calls it)",
                      lambda: ops.nms_rotated_keep_mask(d6, lorder, 0.1, 6, label_major=True)),
                     ("nms_rotated(3 kernels; plain score order, one sweep)",
                      lambda: ops.nms_rotated_keep_mask(d6, order, 0.1, 6))):
        t = event_time(fn, 10, 2)
        # the ALU-side figure: candidate pairs the greedy rule is defined over (ordered pairs i < j of the same class:
        # nms_rotated.py:73-120 tests exactly those) per second; the mask kernel culls most of them on centre distance
        out[name] = dict(bound="latency/alu", achieved=by / t / 1e9, peak=HBM_PEAK_GBS, unit="GB/s",
                         frac=by / t / 1e9 / HBM_PEAK_GBS, traffic=None, us=t * 1e6, mboxes_per_s=M / t / 1e6,
                         same_class_pairs=same_cls, mpairs_per_s=same_cls / t / 1e6)
    out.update(bn_act_rows(device, len(ks)))
    out.update(gemm1x1_rows(device, len(ks)))
    out.update(next_row_kernels(device))
    out.update(van_rows(device))
    out.update(survey_8d_rows(device))
    return out


def survey_8d_rows(device):
    """SURVEY 8(d)'s micro-bench sweeps in the driver-visible table: dense rotated IoU at K in {16, 100, 400}
    gts of ONE tile against the 21 824-anchor grid -- exact grid and refined anchors (seed 7) -- through the two-tier kernel
    (csrc/iou_fast.hip) and the bit-exact one; rotated NMS at M in {2 000, 5 344, 20 000} boxes in label-major order (as
    ml_nms_rotated calls it) and plain score order.  frac = SURVEY 8(d)'s algorithmic bytes / time / 8 TB/s."""
    from rs_detection_amd import ops
    from rs_detection_amd.utils import synthetic as syn
    from rs_detection_amd.ops.nms_rotated import _label_major_order
    out = {}
    rng = np.random.default_rng(3)
    grids = (("exact grid", syn.s2anet_anchor_grid()), ("refined anchors (seed 7)", syn.refined_anchor_grid(7)))
    for gname, grid in grids:
        anchors = torch.from_numpy(np.ascontiguousarray(grid, dtype=np.float32)).to(device)
        A = anchors.shape[0]
        prep = ops.prepare_boxes(anchors, cache=False)
        for K in (16, 100, 400):
            gt = torch.from_numpy(syn.dota_gt_boxes(rng, K)).to(device)
            ro = torch.tensor([0, K], dtype=torch.int32, device=device)
            ov = torch.empty((K, A), device=device)
            by = 20 * (K + A) + 4 * K * A
            for kname, fn in (("two-tier", lambda: ops.box_iou_rotated_fast(gt, anchors, ro, ks=[K], out=ov, prepared=prep)),
                              ("bit-exact", lambda: ops.box_iou_rotated_grouped(gt, ro, K, anchors, out=ov))):
                t = event_time(fn, 30)
                out["iou_sweep[%s, K=%d, %s]" % (kname, K, gname)] = dict(
                    bound="hbm", achieved=by / t / 1e9, peak=HBM_PEAK_GBS, unit="GB/s", frac=by / t / 1e9 / HBM_PEAK_GBS,
                    traffic=None, us=t * 1e6, mpairs_per_s=K * A / t / 1e6, overlapping_pairs=int((ov != 0).sum()))
    for M in (2000, 5344, 20000):
        d, sc_, l = syn.nms_cluster_boxes(M)
        d6 = torch.from_numpy(np.concatenate([d, l[:, None].astype(np.float32)], 1)).to(device)
        sc, lab = torch.from_numpy(sc_).to(device), torch.from_numpy(l).to(device)
        lorder = _label_major_order(sc, lab).int()
        order = torch.argsort(sc, descending=True, stable=True).int()
        by = 4 * 6 * M + 2 * 8 * M * ((M + 63) // 64) + M
        for oname, fn in (("label-major", lambda: ops.nms_rotated_keep_mask(d6, lorder, 0.1, 6, label_major=True)),
                          ("score order", lambda: ops.nms_rotated_keep_mask(d6, order, 0.1, 6))):
            t = event_time(fn, 10, 2)
            out["nms_sweep[M=%d, %s]" % (M, oname)] = dict(
                bound="latency/alu", achieved=by / t / 1e9, peak=HBM_PEAK_GBS, unit="GB/s", frac=by / t / 1e9 / HBM_PEAK_GBS,
                traffic=None, us=t * 1e6, mboxes_per_s=M / t / 1e6)
    return out


def eval_leg(device, steps=10):
    """The S2ANet TEST path (/root/reference/python/jdet/runner/runner.py:214-245 -> s2anet_head.py:510-601 get_bboxes ->
    ops/nms_rotated.py:540-596 multiclass_nms_rotated) through Runner.predict on resident synthetic 1024^2 tiles: tiles/s
    at B = 1 and B = 4, fp32 and bf16 autocast (channels_last), the detections left on the device as in the eval loop."""
    from rs_detection_amd.config import Config
    from rs_detection_amd.runner.runner import Runner
    from rs_detection_amd.utils.synthetic import synthetic_targets
    out = {}
    for tag, amp in (("f32", None), ("bf16", torch.bfloat16)):
        torch.manual_seed(0)
        r = Runner(s2anet_cfg(), device=device, memory_format=torch.channels_last, amp_dtype=amp)
        for B in (1, 4):
            im = torch.randn(B, 3, TILE, TILE, device=device)
            tg = synthetic_targets(B, img=TILE)
            with torch.no_grad():
                for _ in range(3):
                    r.predict(im, tg)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    r.predict(im, tg)
                t_enq = time.perf_counter() - t0
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out["%s_b%d" % (tag, B)] = {"tiles_per_s": B * steps / dt, "ms_per_call": dt / steps * 1e3,
                                        "host_enqueue_ms_per_call": t_enq / steps * 1e3}
        del r
        torch.cuda.empty_cache()
    return out


def van_rows(device):
    """Round 6: the fp32 MFMA GEMM and weight gradient of the VAN block (csrc/van_gemm.hip) at the stage-3 shapes of the
    Oriented R-CNN step (2 images, 64 x 64 positions, C = 320, R = 1280), and the kernels of the heads' control path
    (csrc/orpn.hip): the radix-select sampler over the RPN's 611 072 anchors and the proposals of a batch.  GEMM rows are
    MFMA-bound (fp32 dense peak); the control-path rows are latency-bound -- their `frac` is of HBM, for the record."""
    from rs_detection_amd import _lib as _L
    from rs_detection_amd.ops import orpn
    lib = _L.load()
    out = {}
    P = _L.ptr
    N, C, R, HW = 2, 320, 1280, 64 * 64
    x = torch.randn(N, C, HW, device=device)
    h = torch.randn(N, R, HW, device=device)
    w_rc, w_cr, w_cc = (torch.randn(a, b, device=device) * 0.05 for a, b in ((R, C), (C, R), (C, C)))
    v = [torch.rand(R, device=device) for _ in range(3)]
    o_r, o_c, o_c1 = torch.empty(N, R, HW, device=device), torch.empty(N, C, HW, device=device), torch.empty(N, C, HW, device=device)

    def mfma_row(name, flops, t):
        out[name] = dict(bound="mfma", achieved=flops / t / 1e12, peak=FP32_VALU_PEAK_TFLOPS, unit="TFLOP/s",
                         frac=flops / t / 1e12 / FP32_VALU_PEAK_TFLOPS, traffic=None, us=t * 1e6)
    f_cr, f_cc = 2.0 * N * HW * C * R, 2.0 * N * HW * C * C
    calls = (
        ("van_gemm_f32 fc1 1280x320x8192 (+ bias)", f_cr,
         lambda: lib.rsdet_van_gemm_f32(P(w_rc), P(x), R, C, HW, N, 1, P(v[0]), None, None, None, None, None, P(o_r), None, _L.stream_ptr())),
        ("van_gemm_f32 fc2 320x1280x8192 (+ layer scale + shortcut)", f_cr,
         lambda: lib.rsdet_van_gemm_f32(P(w_cr), P(h), C, R, HW, N, 4, None, P(v[1]), P(v[2]), None, P(x), None, P(o_c), None, _L.stream_ptr())),
        ("van_gemm_f32 proj_1 320x320x8192 (+ bias + GELU, two outputs)", f_cc,
         lambda: lib.rsdet_van_gemm_f32(P(w_cc), P(x), C, C, HW, N, 2, P(v[0]), None, None, None, None, None, P(o_c), P(o_c1), _L.stream_ptr())),
        ("van_gemm_f32 fc2 backward-data 1280x320x8192 (x GELU')", f_cr,
         lambda: lib.rsdet_van_gemm_f32(P(w_rc), P(x), R, C, HW, N, 6, None, None, None, None, P(h), None, P(o_r), None, _L.stream_ptr())),
    )
    for name, fl, fn in calls:
        mfma_row(name, fl, event_time(fn, 10, 2))
    S = max(lib.rsdet_van_wgrad_f32_splits(C, R, HW, N) * C * R, lib.rsdet_van_wgrad_f32_splits(C, C, HW, N) * C * C)
    part = torch.empty(S, device=device)
    mfma_row("van_wgrad_f32 320x1280 over 8192 pixels (split-K partials)", f_cr,
             event_time(lambda: lib.rsdet_van_wgrad_f32(P(x), P(h), C, R, HW, N, P(part), _L.stream_ptr()), 10, 2))
    mfma_row("van_wgrad_f32 320x320 over 8192 pixels (split-K partials)", f_cc,
             event_time(lambda: lib.rsdet_van_wgrad_f32(P(x), P(o_c), C, C, HW, N, P(part), _L.stream_ptr()), 10, 2))
    del x, h, o_r, o_c, o_c1, part
    # -- the heads' control path
    rng = np.random.default_rng(3)
    n_a = 611072
    gti = torch.from_numpy(np.where(rng.random(n_a) < 0.002, 1, np.where(rng.random(n_a) < 0.9, 0, -1)).astype(np.int32)).to(device)
    pri = torch.rand(n_a, device=device)
    t = event_time(lambda: orpn.sample_masked(gti, None, 0, pri, 256, 128, -1.0), 10, 2)
    out["sample_masked(radix select: 256 of 611 072 anchors; memset + 3 counting passes + emit + final)"] = dict(
        bound="latency", achieved=8 * n_a / t / 1e9, peak=HBM_PEAK_GBS, unit="GB/s", frac=8 * n_a / t / 1e9 / HBM_PEAK_GBS,
        traffic=None, us=t * 1e6)
    A, sizes = 7, [(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)]
    sc = [torch.rand(2, hh, ww, A, device=device) for hh, ww in sizes]
    rg = [torch.randn(2, 6 * A, hh, ww, device=device) * 0.3 for hh, ww in sizes]
    an = []
    for (hh, ww), st in zip(sizes, (4, 8, 16, 32, 64)):
        cy, cx = torch.meshgrid(torch.arange(hh, device=device) * st + st / 2, torch.arange(ww, device=device) * st + st / 2, indexing="ij")
        c = torch.stack([cx, cy, cx, cy], -1).reshape(-1, 1, 4).float()
        half = torch.tensor([[-4., -4., 4., 4.]], device=device) * st * torch.linspace(0.5, 2.0, A, device=device)[:, None]
        an.append((c + half[None]).reshape(-1, 4).contiguous())
    # MaxIoUAssigner on horizontal boxes without the (K, A) matrix: the level-major anchors above against K = 100 hulls
    anc_all = torch.cat(an)
    ctr = torch.rand(100, 2, device=device) * 1024
    gwh = torch.exp(torch.rand(100, 2, device=device) * (math.log(200.) - math.log(10.)) + math.log(10.))
    hulls = torch.cat([ctr - gwh / 2, ctr + gwh / 2], 1).contiguous()
    t = event_time(lambda: orpn.hbb_assign(anc_all, hulls, 0.7, 0.3, 0.3, True, True), 10, 2)
    by = (16 + 8) * anc_all.shape[0]
    out["hbb_assign(611 072 anchors x K = 100; prep + row maxima + columns, no matrix)"] = dict(
        bound="latency/alu", achieved=by / t / 1e9, peak=HBM_PEAK_GBS, unit="GB/s", frac=by / t / 1e9 / HBM_PEAK_GBS,
        traffic=None, us=t * 1e6)
    t = event_time(lambda: orpn.proposals(sc, rg, an, 2000, 2000, 0.8, 0, None, (1., 1., 1., 1., .5, .5), 4.135), 5, 2)
    by = sum(4 * 2 * A * hh * ww * 7 for hh, ww in sizes)
    out["orpn_proposals(2 images x 5 levels, 611 072 anchors each -> 2 x 2000 rows; 12 launches)"] = dict(
        bound="latency", achieved=by / t / 1e9, peak=HBM_PEAK_GBS, unit="GB/s", frac=by / t / 1e9 / HBM_PEAK_GBS, traffic=None,
        us=t * 1e6)
    return out


def gemm1x1_rows(device, B):
    """The streaming 1x1 GEMM of the bf16 trunk (csrc/gemm1x1_mfma.hip) at the layer2 shapes of the step (B x 128 x 128
    maps, 512 <-> 128 channels): forward with the BatchNorm + identity + ReLU epilogue, backward-data with the next
    BatchNorm's backward in the epilogue (mode 2) and with the identity branch's gradient added (mode 3).  HBM-bound:
    bytes = every operand once (bf16): M K + N K + M N out (+ M N side)."""
    from rs_detection_amd import _lib as _L
    lib = _L.load()
    out = {}
    M, C0, C1 = B * 128 * 128, 512, 128
    if not (lib.rsdet_gemm1x1_mfma_supported(M, C0, C1) and lib.rsdet_gemm1x1_mfma_supported(M, C1, C0)):
        return out
    bf = dict(dtype=torch.bfloat16, device=device)
    y2, x = torch.randn(M, C1, **bf), torch.randn(M, C0, **bf)
    w3 = (torch.randn(C0, C1, device=device) / C1 ** 0.5).bfloat16()
    wt3, wt1 = w3.t().contiguous(), (torch.randn(C0, C1, device=device) / C1 ** 0.5).bfloat16()
    st = [torch.rand(C0, device=device) + 0.5 for _ in range(4)]
    st1 = [torch.rand(C1, device=device) + 0.5 for _ in range(3)]
    y3, gz, gc2, gx = torch.empty(M, C0, **bf), torch.randn(M, C0, **bf), torch.empty(M, C1, **bf), torch.empty(M, C0, **bf)
    gc1 = torch.randn(M, C1, **bf)
    nb = lib.rsdet_conv1x1_dgrad_ws_size(M, C1, C0)
    ws = torch.empty((nb,), dtype=torch.uint8, device=device)
    gg, gb = torch.empty(C1, device=device), torch.empty(C1, device=device)

    def row(name, by, fn):
        t = event_time(fn, 20, 3)
        out[name] = dict(bound="hbm", achieved=by / t / 1e9, peak=HBM_PEAK_GBS, unit="GB/s", frac=by / t / 1e9 / HBM_PEAK_GBS,
                         traffic=None, us=t * 1e6, tflops=2.0 * M * C0 * C1 / t / 1e12)
    row("gemm1x1_bn_act_mfma_bf16_kernel<4,1>(conv3 + bn + identity + relu forward, %dx128 -> 512)" % M,
        2 * (M * C1 + C0 * C1 + 2 * M * C0),
        lambda: lib.rsdet_conv1x1_bn_act_fwd_bf16(_L.ptr(y2), _L.ptr(w3), M, C0, C1, _L.ptr(st[0]), _L.ptr(st[1]),
                                                  _L.ptr(st[2]), _L.ptr(st[3]), 1e-5, _L.ptr(x), 1, _L.ptr(y3), _L.stream_ptr()))
    row("gemm1x1_bn_act_mfma_bf16_kernel<2,2>+finish(conv3 backward-data + bn2's gate and sums in the epilogue, %dx512 -> 128)" % M,
        2 * (M * C0 + C0 * C1 + 2 * M * C1),
        lambda: lib.rsdet_conv1x1_dgrad_bf16(_L.ptr(gz), _L.ptr(wt3), M, C1, C0, 2, _L.ptr(y2), _L.ptr(gb), _L.ptr(ws), nb,
                                             _L.ptr(gc2), _L.stream_ptr()))
    row("gemm1x1_bn_act_mfma_bf16_kernel<4,3>(conv1 backward-data + identity gradient, %dx128 -> 512)" % M,
        2 * (M * C1 + C0 * C1 + 2 * M * C0),
        lambda: lib.rsdet_conv1x1_dgrad_bf16(_L.ptr(gc1), _L.ptr(wt1), M, C0, C1, 3, _L.ptr(gz), None, None, 0,
                                             _L.ptr(gx), _L.stream_ptr()))
    return out


def bn_act_rows(device, B):
    """The fused eval-mode BatchNorm tails of the trunk (csrc/bn_act.hip), the hand-written kernels with the most time
    in the step.  Shapes: the layer1 block output of the step (B x 256 x 256 x 256 with the identity added) in fp32 NCHW
    and in bf16 channels_last.  bytes: forward = x + residual in, y out; backward = gy + y in, gx + gres out (the
    per-channel parameter sums ride on the same pass)."""
    from rs_detection_amd.ops.bn_act import bn_act
    out = {}
    C, H = 256, TILE // 4
    bn = torch.nn.BatchNorm2d(C).to(device).eval()
    for tag, dt, cl in (("f32", torch.float32, False), ("f32 nhwc", torch.float32, True), ("bf16 nhwc", torch.bfloat16, True)):
        x = torch.randn(B, C, H, H, device=device, dtype=dt)
        r = torch.randn(B, C, H, H, device=device, dtype=dt)
        if cl:
            x, r = x.contiguous(memory_format=torch.channels_last), r.contiguous(memory_format=torch.channels_last)
        es = x.element_size()
        t = event_time(lambda: bn_act(x, bn, r, True), 10, 2)
        name = BN_ROW if tag == "f32" else (BN_ROW_CL if tag == "f32 nhwc" else
                                            "bn_act_forward_nhwc_kernel<bf16>(bn + residual + relu; %dx256x%dx%d)" % (B, H, H))
        by = 3 * es * x.numel()
        out[name] = dict(bound="hbm", achieved=by / t / 1e9, peak=HBM_PEAK_GBS, unit="GB/s", frac=by / t / 1e9 / HBM_PEAK_GBS,
                         traffic=pmc_traffic("bn_act_forward_" + tag.split()[0], (B, H) == (4, 256)) if tag != "f32 nhwc" else None,
                         us=t * 1e6)
        xg, rg = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
        y = bn_act(xg, bn, rg, True)
        gy = torch.randn_like(y)
        t = event_time(lambda: torch.autograd.grad(y, (xg, rg, bn.weight, bn.bias), gy, retain_graph=True), 10, 2, graph=False)
        by = 4 * es * x.numel()
        out["bn_act_backward%s<%s>(gx + gres + parameter sums; same shape; eager launches)" % ("_nhwc" if cl else "", tag.split()[0])] = dict(
            bound="hbm", achieved=by / t / 1e9, peak=HBM_PEAK_GBS, unit="GB/s", frac=by / t / 1e9 / HBM_PEAK_GBS,
            traffic=pmc_traffic("bn_act_backward_" + tag.split()[0], (B, H) == (4, 256)) if tag != "f32 nhwc" else None,
            us=t * 1e6)
        del x, r, xg, rg, y, gy
    return out


def next_row_kernels(device):
    """SURVEY 8(f) rows (RROIAlign of the Oriented R-CNN head, and the rank-4 ops): same HIP-event timing."""
    from rs_detection_amd import _lib, ops
    from rs_detection_amd.utils import synthetic as syn
    lib = _lib.load()
    out = {}

    def row(name, by, t, bound="hbm", **kw):
        out[name] = dict(bound=bound, achieved=by / t / 1e9, peak=HBM_PEAK_GBS, unit="GB/s",
                         frac=by / t / 1e9 / HBM_PEAK_GBS, traffic=None, us=t * 1e6, **kw)

    rng = np.random.default_rng(3)
    # -- ROIAlignRotated_v1 / v0 (a18, f4): 512 RoIs on the stride-4 level of two 1024^2 tiles, 7x7 bins, 2x2 samples;
    #    bytes = 4*R*C*49*(1 out + 16 gathered in)
    N, C, H, R = 2, 256, TILE // 4, 512
    feat = torch.randn(N, C, H, H, device=device, requires_grad=True)
    b = syn.dota_gt_boxes(rng, R).astype(np.float32)
    rois = torch.from_numpy(np.concatenate([rng.integers(0, N, (R, 1)).astype(np.float32), b], 1)).to(device)
    by = 4 * R * C * 49 * 17
    for tag, fn in (("v1", ops.roi_align_rotated_v1), ("v0", ops.roi_align_rotated.roi_align)):
        t = event_time(lambda: fn(feat.detach(), rois, (7, 7), 0.25, 2), 10, 2)
        row("rroi_forward_kernel(%s; 512 RoIs x 256 ch)" % tag, by, t)
    from rs_detection_amd.ops.roi_align_rotated_v1 import rroi_align_backward
    go = torch.randn(R, C, 7, 7, device=device)
    t = event_time(lambda: rroi_align_backward(go, rois, (N, C, H, H), (7, 7), 0.25, 2, "v1"), 10, 2)
    row("rroi_idx_count+scan+fill+rroi_gather(backward, default route; a %d MB output)"
        % (N * C * H * H * 4 // 2 ** 20), 4 * (R * C * 49 + N * C * H * H), t)
    import importlib
    rmod = importlib.import_module("rs_detection_amd.ops.roi_align_rotated_v1")
    was = rmod._NCHW_GATHER
    for flag in (False, True):
        rmod._NCHW_GATHER = flag
        t = event_time(lambda: rroi_align_backward(go, rois, (N, C, H, H), (7, 7), 0.25, 2, "v1"), 10, 2)
        row("rroi backward, %s" % ("NCHW written by the gather (one layout turn: grad_out)" if flag else
                                   "channels-last gather + two layout turns"), 4 * (R * C * 49 + N * C * H * H), t)
    rmod._NCHW_GATHER = was
    del feat, go
    # -- depthwise convolutions of the VAN backbone (a20): stage-1 shapes of VAN-B3 on two 1024^2 tiles;
    #    bytes = one read + one write of the tensor (forward / backward-data), two reads (backward-weight)
    from rs_detection_amd.ops.dwconv import dwconv2d
    for (Cd, Hd, K, D) in ((512, 256, 3, 1), (64, 256, 5, 1), (64, 256, 7, 3)):
        xd = torch.randn(2, Cd, Hd, Hd, device=device, requires_grad=True)
        wd = torch.randn(Cd, 1, K, K, device=device, requires_grad=True)
        bd = torch.zeros(Cd, device=device, requires_grad=True)
        t = event_time(lambda: dwconv2d(xd.detach(), wd.detach(), bd.detach(), D), 10, 2)
        row("dwconv_stencil_kernel<%d,%d>(forward; 2x%dx%dx%d)" % (K, D, Cd, Hd, Hd), 8 * xd.numel(), t)
        # backward: the two C-ABI calls of ops/dwconv.py's node on preallocated buffers, replayed from a graph (device
        # time: the autograd call of these 30-MB shapes is host-bound, which is what rounds 4-5 reported for <5,1> / <7,3>)
        god = torch.randn_like(xd)
        gxd, gwd, gbd = torch.empty_like(xd), torch.empty_like(wd), torch.empty_like(bd)
        wsb = lib.rsdet_dwconv2d_backward_weight_ws_size(2, Cd, Hd, Hd, K)
        wsd = torch.empty((max(wsb, 4),), dtype=torch.uint8, device=device)
        xdd, wdd = xd.detach(), wd.detach()

        def dw_bwd():
            _lib.check(lib.rsdet_dwconv2d_backward_data_f32(_lib.ptr(god), _lib.ptr(wdd), 2, Cd, Hd, Hd, K, D, _lib.ptr(gxd),
                                                            None, None, 0, _lib.stream_ptr()), "dwconv backward-data")
            _lib.check(lib.rsdet_dwconv2d_backward_weight_f32(_lib.ptr(god), _lib.ptr(xdd), None, 2, Cd, Hd, Hd, K, D,
                                                              _lib.ptr(gwd), _lib.ptr(gbd), _lib.ptr(wsd), wsb,
                                                              _lib.stream_ptr()), "dwconv backward-weight")
        t = event_time(dw_bwd, 10, 2)
        row("dwconv backward-data + backward-weight<%d,%d>" % (K, D), 16 * xd.numel(), t)
        del xd, god, gxd
    # -- FeatureRefine (f4): R3Det level 0 of two tiles, 256 channels; bytes = read + write every element once
    N, C, H = 2, 256, TILE // 8
    f = torch.randn(N, C, H, H, device=device, requires_grad=True)
    yc, xc = np.meshgrid(8.0 * np.arange(H), 8.0 * np.arange(H), indexing="ij")
    bx = np.stack([xc[None] + 32 * rng.standard_normal((N, H, H)), yc[None] + 32 * rng.standard_normal((N, H, H)),
                   32 * np.exp(rng.standard_normal((N, H, H))), 32 * np.exp(rng.standard_normal((N, H, H))),
                   -np.pi / 2 * rng.random((N, H, H))], -1).astype(np.float32)
    bx = torch.from_numpy(bx).to(device)
    by = 4 * (2 * N * C * H * H + 5 * N * H * H)
    for pts in (1, 5):
        t = event_time(lambda: ops.feature_refine(f.detach(), bx, 0.125, pts), 10, 2)
        row("fr_forward_kernel<%d>" % pts, by, t)
        from rs_detection_amd.ops.fr import feature_refine_backward
        go = torch.randn(N, C, H, H, device=device)
        t = event_time(lambda: feature_refine_backward(go, bx, 0.125, pts), 10, 2)
        row("fr_idx_count+scan+fill+gather<%d>(backward; incl. the two layout permutes)" % pts, by, t)
        # the same op on a channels_last map (what a channels_last step hands over): NHWC forward, no permutes backward
        fcl = f.detach().contiguous(memory_format=torch.channels_last)
        t = event_time(lambda: ops.feature_refine(fcl, bx, 0.125, pts), 10, 2)
        row("fr_forward_nhwc_kernel<%d>(channels_last map)" % pts, by, t)
        gocl = go.contiguous(memory_format=torch.channels_last)
        t = event_time(lambda: feature_refine_backward(gocl, bx, 0.125, pts), 10, 2)
        row("fr_idx_count+scan+fill+gather<%d>(backward; channels_last gradient, no permutes)" % pts, by, t)
        del fcl, gocl
    del f, go
    # -- convex_sort (f4): the poly_iou_loss shape, 24 candidate points per pair, 20 000 pairs
    nbs, npts = 20000, 24
    p = torch.randn(nbs, npts, 2, device=device) * 20
    m = torch.rand(nbs, npts, device=device) > 0.6
    t = event_time(lambda: ops.convex_sort(p, m), 10, 2)
    row("convex_sort_kernel(20000 sets x 24 points)", nbs * (npts * 12 + (npts + 1) * 4), t, bound="latency/alu",
        msets_per_s=nbs / t / 1e6)
    # -- poly_nms (f4): 2000 quadrilaterals of the NMS micro-bench clusters, fp32 reference arithmetic on every pair
    d, sc, _ = syn.nms_cluster_boxes(2000)
    from rs_detection_amd.ops.box_coder import rotated_box_to_poly
    q = rotated_box_to_poly(torch.from_numpy(d).to(device))
    dets = torch.cat([q, torch.from_numpy(sc).to(device)[:, None]], 1).contiguous()
    t = event_time(lambda: ops.poly_nms(dets, 0.1), 5, 1, graph=False)
    row("poly_nms(iota + mask + sweep; 2000 quads, all pairs)", 36 * 2000, t, bound="alu",
        mpairs_per_s=2000 * 1999 / 2 / t / 1e6)
    return out


def cpu_baseline(budget_s=12.0):
    """Reference CPU rotated IoU (single thread, as box_iou_rotated.py:495-499) on a bounded sample."""
    import oracle
    from rs_detection_amd.utils import synthetic as syn
    ref = oracle.ref()
    kind, impl = ("reference", ref) if ref.available else ("port", oracle.c())
    anchors = syn.s2anet_anchor_grid()
    gts = syn.dota_gt_boxes(np.random.default_rng(1234), 100)
    pairs, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < budget_s:
        impl.box_iou_rotated(gts, anchors, 0)
        pairs += gts.shape[0] * anchors.shape[0]
    dt = time.perf_counter() - t0
    single = pairs / dt / 1e6
    # the same source with its outer (gt) loop split over all host cores: ctypes releases the GIL during the call
    from concurrent.futures import ThreadPoolExecutor
    ncores = os.cpu_count() or 1
    big = syn.dota_gt_boxes(np.random.default_rng(4321), 64 * ncores)
    chunks = np.array_split(big, ncores)
    calls, t0 = 0, time.perf_counter()
    with ThreadPoolExecutor(ncores) as pool:
        while time.perf_counter() - t0 < budget_s / 2:
            list(pool.map(lambda g: impl.box_iou_rotated(g, anchors, 0), chunks))
            calls += 1
    dt2 = time.perf_counter() - t0
    return dict(value=single, unit="Mpairs/s (rotated IoU; the reference has no CPU path for the full "
                "S2ANet step: DeformConv is CUDA-only, dcn_v1.py:588-589)", cores=1, kind=kind,
                sample="K=100 gt x A=21824 S2ANet anchors, repeated for %.0f s (%d calls)" % (dt, pairs // (100 * 21824)),
                all_cores=dict(value=calls * big.shape[0] * anchors.shape[0] / dt2 / 1e6, cores=ncores,
                               sample="K=%d gt split over %d threads, %.0f s" % (big.shape[0], ncores, dt2)))


N_BATCHES = 4  # resident batches rotated through the timed loop


def make_batches(n, batch, rank, ncls, device, mf, orcnn):
    from rs_detection_amd.utils import synthetic as syn
    out = []
    for it in range(n):
        g = torch.Generator(device="cpu").manual_seed(1000 * it + rank)
        images = torch.randn(batch, 3, TILE, TILE, generator=g).to(device)
        if mf is torch.channels_last:
            images = images.contiguous(memory_format=mf)
        targets = []
        for t in syn.synthetic_targets(batch, rank=rank, it=it, num_classes=ncls, img=TILE, k_shift=it):
            t = dict(t)
            t["rboxes"] = torch.from_numpy(t["rboxes"]).to(device)
            t["labels"] = torch.from_numpy(t["labels"]).to(device)
            if orcnn:
                t["hboxes"] = None
            targets.append(t)
        out.append((images, targets))
    return out


def timed_region(runner, batches, steps, rdist, device):
    """EXACTLY `steps` train steps between barrier + synchronize on both sides; max over ranks.  Also returns the host
    time the loop took to ENQUEUE the steps (before the closing synchronize): enqueue ~ total means the host, not the
    GPU, paces the step -- the number that explains a flat multi-GPU curve with one Python process per GPU -- and the
    loss terms of the last step."""
    rdist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        loss, parsed = runner.train_step(*batches[i % len(batches)])
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    rdist.barrier()
    dt = time.perf_counter() - t0
    dt = rdist.all_reduce_max(dt, device)
    loss_v = float(loss.detach())
    assert np.isfinite(loss_v), "non-finite loss"
    return dt, loss_v, t_enq, parsed


DUMP_PARAM_SAMPLE = 1 << 20  # parameters written by --dump-outputs: a fixed seeded sample of 1 Mi values (4 MB)


def dump_outputs(out_dir, runner, loss_v, parsed):
    """--dump-outputs DIR: what the last timed step handed its caller -- the total loss (``total_loss.npy``) and every
    loss term (``<name>.npy``), float64 -- and the model it left behind: ``params_sample.npy``, float32, the values of
    DUMP_PARAM_SAMPLE positions drawn with seed 0 from all parameters flattened in ``named_parameters()`` order."""
    import re
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "total_loss.npy"), np.array(loss_v, np.float64))
    for name, v in parsed.items():
        np.save(os.path.join(out_dir, re.sub(r"[^A-Za-z0-9_.-]", "_", name) + ".npy"),
                np.asarray(v.detach().double().cpu().numpy(), np.float64))
    flat = torch.cat([p.detach().reshape(-1).float() for _, p in runner.model.named_parameters()])
    idx = np.sort(np.random.default_rng(0).choice(flat.numel(), min(flat.numel(), DUMP_PARAM_SAMPLE), replace=False))
    np.save(os.path.join(out_dir, "params_sample.npy"), flat[torch.from_numpy(idx).to(flat.device)].cpu().numpy())


def extra_leg(model, amp, mf, steps, rank, device, rdist, bf16_params):
    """A short timed leg of ANOTHER BASELINE config on this GPU (own Runner, own resident batches, torn down after):
    {value tiles/s, ms_per_step, host_enqueue_ms_per_step, steps}.  Same timed_region as the headline."""
    from rs_detection_amd.config import Config
    from rs_detection_amd.runner.runner import Runner
    if model == "orcnn_van3":
        cfg, batch, ncls = Config(os.path.join(ROOT, "configs", "orcnn", "orcnn_van3_7_anchor.py")), 2, 10
    else:
        cfg = Config(os.path.join(ROOT, "configs", "s2anet", "s2anet_r101_fpn_1x_dota_rotate_balance_ms.py"))
        batch, ncls = BATCH_PER_GPU, 15
    torch.manual_seed(0)
    r = Runner(cfg, device=device, memory_format=mf, amp_dtype=amp, bf16_params=bf16_params)
    bs = make_batches(N_BATCHES, batch, rank, ncls, device, mf, model == "orcnn_van3")
    for i in range(2 * N_BATCHES):
        r.train_step(*bs[i % N_BATCHES])
    dt, loss, enq, _ = timed_region(r, bs, steps, rdist, device)
    out = {"value": batch * steps / dt, "unit": "tiles/s", "ms_per_step": dt / steps * 1e3, "steps": steps,
           "host_enqueue_ms_per_step": enq / steps * 1e3, "final_loss": loss, "tiles_per_step": batch,
           "dtype": "bf16" if amp is not None else "f32"}
    del r, bs
    torch.cuda.empty_cache()
    return out


def ddp_overhead_leg(cfg, device, b16, steps, warm, bf16_params, rdist, enq_plain_ms, ms_plain):
    """The bf16 S2ANet leg again with the data-parallel gradient reduction FORCED ON in a one-rank ``nccl`` (= RCCL)
    process group: the buckets, their multi-tensor copies and one all-reduce per bucket through RCCL run on this single
    GPU.  Reported: the host time it adds to the enqueue of a step (the bf16 step is host-paced: this, not xGMI, is the
    first scaling risk of one Python process per GPU) for the product's reducer (utils/reducer.GradReducer) and, beside
    it, for torch's DistributedDataParallel (bucket views + bf16 compress hook).  A failure to bring RCCL up is
    reported in the object, not raised."""
    import torch.distributed as dist
    from rs_detection_amd.runner.runner import Runner
    made = False
    try:
        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(rdist.free_port()))
            dist.init_process_group(backend="nccl", rank=0, world_size=1)
            made = True
        out = {"backend": dist.get_backend(), "world": 1}
        for tag, mode in (("reducer", "force"), ("torch_ddp", "ddp-force")):
            torch.manual_seed(0)
            r = Runner(cfg, device=device, memory_format=torch.channels_last, amp_dtype=torch.bfloat16,
                       bf16_params=bf16_params, distributed=mode)
            assert (r.reducer is not None) if tag == "reducer" else (r.ddp is not r.model)
            for i in range(warm):
                r.train_step(*b16[i % N_BATCHES])
            dt, loss, enq, _ = timed_region(r, b16, steps, rdist, device)
            leg = {"ms_per_step": dt / steps * 1e3, "host_enqueue_ms_per_step": enq / steps * 1e3,
                   "host_overhead_ms": enq / steps * 1e3 - enq_plain_ms, "step_overhead_ms": dt / steps * 1e3 - ms_plain,
                   "final_loss": loss}
            if tag == "reducer":
                leg["wire"], leg["buckets"] = r.reducer.wire_dtypes, len(r.reducer.buckets)
                out.update(leg)              # the product's numbers at the top level of the object
            else:
                out["torch_ddp"] = leg
            del r
            torch.cuda.empty_cache()
    except Exception as e:  # noqa: BLE001
        out = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
    finally:
        if made:
            try:
                dist.destroy_process_group()
            except Exception:  # noqa: BLE001
                pass
    torch.cuda.empty_cache()
    return out


def fresh_k_batches(batches, n, rank, ncls, device, orcnn):
    """`n` target sets with a K tuple never seen before (a real DOTA stream brings new gt counts every step),
    on the images of the resident batches: every step then misses the per-K-tuple tile table of the anchor-target path
    (ops/anchor_target.row_tile_table: built on the host, one pinned upload) and meets new allocation sizes."""
    from rs_detection_amd.utils import synthetic as syn
    rng = np.random.default_rng(99 + rank)
    out = []
    for it in range(n):
        images, tg0 = batches[it % len(batches)]
        ks = [int(k) for k in rng.integers(8, 420, len(tg0))]
        targets = []
        for j, k in enumerate(ks):
            t = dict(syn.synthetic_targets(1, rank=rank, it=1000 + it * 16 + j, num_classes=ncls, img=TILE, ks=[k])[0])
            t["rboxes"] = torch.from_numpy(t["rboxes"]).to(device)
            t["labels"] = torch.from_numpy(t["labels"]).to(device)
            if orcnn:
                t["hboxes"] = None
            targets.append(t)
        out.append((images, targets))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-bf16-leg", action="store_true", help="skip the second (bf16) timed leg of the default line")
    ap.add_argument("--fresh-k", action="store_true",
                    help="the timed steps see a NEW gt-count tuple every step (the per-iteration stream of real DOTA "
                         "batches) instead of the four rotating resident batches; without the flag the default line "
                         "reports that mode as a short extra leg (fresh_k_ms_per_step)")
    ap.add_argument("--kernels-out", default=None, help="where the full per-kernel table goes (default: "
                    "gpurun_out/bench_kernels.json when that directory exists, else ./bench_kernels.json); the JSON "
                    "line itself carries the 12 rows with the most time")
    ap.add_argument("--no-extra-legs", action="store_true",
                    help="skip the short Oriented R-CNN VAN-B3 (configs[3]) / S2ANet-R101 bf16 (configs[4]) / DDP-overhead "
                         "legs the default single-GPU line carries as flat scalars")
    ap.add_argument("--bf16-params", choices=["0", "1"], default="1",
                    help="bf16 legs: conv / linear weights held in bf16 with fp32 masters in the fused optimizer "
                         "(csrc/optim.hip; 1, default) or fp32 parameters under autocast + foreach SGD (0)")
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32",
                    help="f32 = BASELINE config[1] (the metric); bf16 = torch.autocast over the MIOpen/rocBLAS part "
                         "(configs[2]/[4]); the oriented-box kernels always compute in fp32")
    ap.add_argument("--model", choices=["s2anet_r50", "s2anet_r101", "orcnn_van3"], default="s2anet_r50",
                    help="s2anet_r50 = BASELINE configs[1] (the metric, default); orcnn_van3 = the Oriented R-CNN + VAN-B3 "
                         "model of configs[3] (RROIAlign + rotated NMS in the train step), 2 tiles per GPU as in the "
                         "reference config; reported under its own workload name, no kernel table")
    ap.add_argument("--memory-format", choices=["channels_last", "contiguous", "trunk_channels_last"], default=None,
                    help="activation layout of the torch/MIOpen part.  Default: channels_last for the S2ANet models in "
                         "both dtypes.  bf16: MIOpen's bf16 kernels are NHWC-native (round 2: 26.8 vs 28.3 ms/step).  f32: "
                         "with find records for the NHWC shapes MIOpen runs its fp32 MFMA implicit-GEMM kernels without "
                         "layout transposes, 52.5 vs 55.3 ms/step (round 3; on heuristics the same layout was 494 ms in "
                         "round 1 -- the packaged records are what makes it the faster one).  contiguous for the others")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (total loss and every loss "
                         "term, float64) and a fixed seeded sample of the parameters it left (float32) as DIR/<name>.npy; "
                         "rank 0 only.  The inputs are seeded: two builds run with the same arguments can be compared")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.memory_format is None:
        # (the R101 trunk has fp32 NHWC records for none of its layer3 shapes: it stays NCHW in f32)
        from rs_detection_amd.utils.miopen_db import packaged_records_match
        f32_cl = args.model == "s2anet_r50" and packaged_records_match()     # without the records: 7 x slower, NCHW then
        args.memory_format = "channels_last" if (f32_cl or (
            args.dtype == "bf16" and args.model.startswith("s2anet"))) else "contiguous"

    from rs_detection_amd.utils import dist as rdist
    from rs_detection_amd.utils import synthetic as syn
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: this process becomes the launcher (the reference's `mpirun -np N`,
        # README_competition.md:79-80).  It has not touched the GPU (device_count() does not initialise HIP) and
        # never will: the N ranks are child processes, rank 0's JSON line is relayed, the exit code is theirs.
        if torch.cuda.device_count() < args.gpus:
            # fewer GPUs than ranks (the 1-GPU test box): ranks share devices, which RCCL refuses -> gloo
            os.environ.setdefault("RSDET_DIST_BACKEND", "gloo")
        rc, out = rdist.launch_ranks(args.gpus, [os.path.abspath(__file__)] + sys.argv[1:])
        for ln in out.splitlines():     # ONE JSON line on stdout; anything else a rank printed (gloo's banner) -> stderr
            print(ln, file=sys.stdout if ln.startswith("{") else sys.stderr, flush=True)
        raise SystemExit(rc)
    rank, local_rank, world = rdist.init_distributed()
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X; there is no CPU fallback for the HIP hot path")
    device = torch.device("cuda", local_rank % torch.cuda.device_count())  # (% only matters for the 1-GPU gloo smoke test)
    torch.cuda.set_device(device)
    rdist.require_rccl(world)            # a GPU per rank and yet not RCCL: refuse (non-zero exit of every rank)
    facts = rdist.gather_objects(rdist.rank_facts(device))
    from rs_detection_amd import _lib
    _lib.load()

    from rs_detection_amd.runner.runner import Runner
    torch.manual_seed(0)  # same initial weights on every rank (DDP also broadcasts)
    mf = {"channels_last": torch.channels_last, "trunk_channels_last": "trunk_channels_last"}.get(args.memory_format)
    if args.model == "orcnn_van3":
        from rs_detection_amd.config import Config
        cfg, batch, ncls = Config(os.path.join(ROOT, "configs", "orcnn", "orcnn_van3_7_anchor.py")), 2, 10
        args.no_kernels = True
    elif args.model == "s2anet_r101":
        # BASELINE configs[4]: same head, Resnet101 trunk; reported under its own workload name, no kernel table
        from rs_detection_amd.config import Config
        cfg = Config(os.path.join(ROOT, "configs", "s2anet", "s2anet_r101_fpn_1x_dota_rotate_balance_ms.py"))
        batch, ncls = BATCH_PER_GPU, 15
        args.no_kernels = True
    else:
        cfg, batch, ncls = s2anet_cfg(), BATCH_PER_GPU, 15
    amp = torch.bfloat16 if args.dtype == "bf16" else None
    runner = Runner(cfg, device=device, memory_format=mf, amp_dtype=amp, bf16_params=args.bf16_params == "1")
    mg_buckets = len(runner.reducer.buckets) if runner.reducer is not None else None
    mg_wire = runner.reducer.wire_dtypes if runner.reducer is not None else None
    # synthetic DOTA-shaped batches, resident in HBM before the timed region.  N_BATCHES different batches
    # rotate through the timed loop (step i runs batch i % N_BATCHES, the K cycle shifted by one slot per batch), so the
    # per-K-tuple tile tables and the prepared-box caches of the anchor-target path see new gts every step.
    batches = make_batches(N_BATCHES, batch, rank, ncls, device, mf, args.model == "orcnn_van3")
    images, targets = batches[0]

    # untimed set-up before the W warm-up steps: every resident batch once (kernel loads, MIOpen handles, the caching
    # allocator's steady state for each K layout), then the flop-counting step; the W warm-up steps and the K timed steps
    # follow back to back
    for b_ in batches:
        runner.train_step(*b_)
    step_flops = None
    if not args.no_kernels:
        # one extra UNTIMED step under torch's flop counter (convs + GEMMs, fwd + bwd).  On EVERY rank: the step
        # contains DDP's gradient all-reduce, a rank that skipped it would leave the others hanging.
        # Counted on the reference's level-by-level head (``bbox_head.packed = False`` for this one step): the canvas of
        # the timed step convolves 13-15 % gap pixels too, and those are not algorithmic flops.
        # ... and on the library routes (torch's counter sees aten convolutions and GEMMs, not the launches of our own
        # C ABI: the fused 1x1 GEMMs, the one-node Bottleneck, the 3x3 MFMA kernels and AlignConv's implicit GEMM are
        # switched to their aten equivalents for this one step -- same algorithmic flops).
        from torch.utils.flop_counter import FlopCounterMode
        import importlib
        head = runner.model.bbox_head
        head.packed = False
        routes = [("rs_detection_amd.ops.conv_bn", "_ON"), ("rs_detection_amd.ops.bottleneck", "_ON"),
                  ("rs_detection_amd.ops.conv1x1", "_ON"), ("rs_detection_amd.ops.conv3x3", "_ON"),
                  ("rs_detection_amd.ops.conv3x3", "_MFMA"), ("rs_detection_amd.ops.conv3x3", "_TOWER"),
                  ("rs_detection_amd.ops.dcn_v1", "_MFMA_ALIGNCONV")]
        saved = [(importlib.import_module(m), a, getattr(importlib.import_module(m), a)) for m, a in routes]
        for mod, a, _ in saved:
            setattr(mod, a, False)
        try:
            with FlopCounterMode(display=False) as fc:
                runner.train_step(images, targets)
        finally:
            head.packed = True
            for mod, a, v in saved:
                setattr(mod, a, v)
        step_flops = float(fc.get_total_flops())
    orcnn = args.model == "orcnn_van3"
    timed_batches = batches
    if args.fresh_k:
        timed_batches = fresh_k_batches(batches, args.warmup + args.steps, rank, ncls, device, orcnn)
    for i in range(args.warmup):
        runner.train_step(*timed_batches[i % len(timed_batches)])
    if args.fresh_k:
        timed_batches = timed_batches[args.warmup:]
    dt, loss_v, t_enq, parsed = timed_region(runner, timed_batches, args.steps, rdist, device)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, runner, loss_v, parsed)
    del parsed
    # short extra leg of the default line: the same runner on never-seen K tuples (what --fresh-k times in full)
    fresh = None
    if not args.fresh_k and args.model == "s2anet_r50":
        nf = min(max(args.steps, 8), 16)
        fb = fresh_k_batches(batches, nf + 2, rank, ncls, device, orcnn)
        for b_ in fb[:2]:
            runner.train_step(*b_)
        dtf, _, enqf, _ = timed_region(runner, fb[2:], nf, rdist, device)
        fresh = dict(ms_per_step=dtf / nf * 1e3, steps=nf, host_enqueue_ms_per_step=enqf / nf * 1e3)
        del fb
    BN_DOM = BN_ROW_CL if args.memory_format == "channels_last" else BN_ROW     # the form the timed fp32 step ran

    # second, separately timed leg: the SAME model and batches in bf16 autocast + channels_last (BASELINE configs[2]'s
    # arithmetic), its own Runner, its own warm-up; reported as a nested object, never as `value`
    bf16_leg = None
    if args.dtype == "f32" and args.model == "s2anet_r50" and not args.no_bf16_leg:
        del runner
        torch.cuda.empty_cache()
        torch.manual_seed(0)
        r16 = Runner(cfg, device=device, memory_format=torch.channels_last, amp_dtype=torch.bfloat16,
                     bf16_params=args.bf16_params == "1")
        b16 = [(im.contiguous(memory_format=torch.channels_last), tg) for im, tg in batches]
        # two rounds over the resident batches before the clock starts: with fewer, the last batch (its own K layout)
        # first appears inside the timed region and the caching allocator's hipMallocs land there (16.5-18.8 ms run to run)
        warm16 = max(args.warmup, 2 * N_BATCHES)
        for i in range(warm16):
            r16.train_step(*b16[i % N_BATCHES])
        steps16 = max(args.steps, 20)
        dt16, loss16, enq16, _ = timed_region(r16, b16, steps16, rdist, device)
        bf16_leg = {"value": batch * world * steps16 / dt16, "unit": "tiles/s", "ms_per_step": dt16 / steps16 * 1e3,
                    "steps": steps16, "warmup": warm16, "dtype": "bf16", "memory_format": "channels_last",
                    "bf16_params": bool(r16.bf16_params), "host_enqueue_ms_per_step": enq16 / steps16 * 1e3,
                    "final_loss": loss16,
                    "flop_roofline": None if step_flops is None else {
                        "bound": "mfma", "achieved": step_flops / (dt16 / steps16) / 1e12, "unit": "TFLOP/s",
                        "peak": 2500.0, "frac": step_flops / (dt16 / steps16) / 1e12 / 2500.0}}
        del r16
        torch.cuda.empty_cache()
        # what DDP adds to the HOST side of that (host-paced) step: the same leg under an `nccl` (= RCCL) process group of
        # one rank with DDP forced on -- bucket views, bf16 compress hook, one all-reduce per bucket through RCCL
        ddp_leg = None
        if world == 1 and not args.no_extra_legs:
            ddp_leg = ddp_overhead_leg(cfg, device, b16, steps16, warm16, args.bf16_params == "1", rdist,
                                       enq16 / steps16 * 1e3, dt16 / steps16 * 1e3)
        del b16
        torch.cuda.empty_cache()
    else:
        ddp_leg = None

    # the other BASELINE configs' single-GPU numbers, as short legs with their own Runner (flat scalars in the line)
    extra = {}
    if args.dtype == "f32" and args.model == "s2anet_r50" and world == 1 and not args.no_extra_legs:
        try:
            del runner
        except NameError:
            pass
        del batches
        torch.cuda.empty_cache()
        extra["r101_bf16"] = extra_leg("s2anet_r101", torch.bfloat16, torch.channels_last, 12, rank, device, rdist,
                                       args.bf16_params == "1")
        extra["orcnn"] = extra_leg("orcnn_van3", None, None, 8, rank, device, rdist, False)
        if rank == 0:
            extra["eval"] = eval_leg(device)

    if rank != 0:
        rdist.barrier()          # rank 0 is still timing its kernel table: leave the group together
        rdist.shutdown()
        return
    kernels = {} if args.no_kernels else kernel_rooflines(device, targets)
    dense = kernels.get("box_iou_rotated(prepare+filter+clip)")
    roof = kernels.get(AT_ROW)
    tiles = batch * world * args.steps
    keys = ("bound", "achieved", "peak", "unit", "frac", "traffic")
    issue = issue_side()     # VALU / latency side of the latency-bound calls, from the committed SQ-counter table
    # The full per-kernel table goes to a file (and stderr); the line keeps the 12 rows with the most time, as
    # {us, frac of the bound's peak, bound} -- the driver's record holds ~8 KB of this line, the table alone was 12.
    kfile = None
    if kernels:
        kfile = args.kernels_out or os.path.join("gpurun_out" if os.path.isdir("gpurun_out") else ".", "bench_kernels.json")
        try:
            with open(kfile, "w") as fh:
                json.dump(kernels, fh, indent=1)
        except OSError:
            kfile = None
        print("bench.py kernels " + json.dumps(kernels), file=sys.stderr, flush=True)
    # 12 headline rows: the matrix-core kernels of the step first (round 4: the 3x3 implicit GEMMs of the head), then the
    # rest by time per call
    first = [kv for kv in kernels.items() if kv[0].startswith("conv3x3_")]
    rest = sorted((kv for kv in kernels.items() if not kv[0].startswith("conv3x3_")), key=lambda kv: -kv[1].get("us", 0.0))
    top = (first + rest)[:12]
    r3 = lambda x: None if x is None else float("%.4g" % x)
    ev = lambda k: (extra["eval"][k]["tiles_per_s"] if extra.get("eval") else None)
    kf = lambda row, key: (kernels[row][key] if row in kernels else None)
    peak_f = FP32_VALU_PEAK_TFLOPS if args.dtype == "f32" else 2500.0
    line = {
        "metric": METRICS[args.model],
        "value": tiles / dt,
        "unit": "tiles/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": args.dtype,
        "data": "synthetic",
        "config": {"workload": (WORKLOADS[args.model] % (batch, TILE, TILE, "fp32" if args.dtype == "f32" else
                                                             "bf16 autocast (fp32 box kernels)")
                                + ("; a NEW K tuple every step (--fresh-k)" if args.fresh_k else
                                   "; %d resident batches per rank, step i runs batch i %% %d" % (N_BATCHES, N_BATCHES))),
                   "global_batch": batch * world, "parallelism": "dp%d" % world,
                   "memory_format": args.memory_format,
                   "miopen_records": "packaged" if MIOPEN_DB_DIR else "none / user-provided"},
        "final_loss": loss_v,
        "host_enqueue_ms_per_step": t_enq / args.steps * 1e3,
        "fresh_k_ms_per_step": fresh["ms_per_step"] if fresh else None,
        "fresh_k_delta_ms": (fresh["ms_per_step"] - dt / args.steps * 1e3) if fresh else None,
        "bf16_tiles_per_s": bf16_leg["value"] if bf16_leg else None,
        "bf16_ms_per_step": bf16_leg["ms_per_step"] if bf16_leg else None,
        "bf16_flop_frac": bf16_leg["flop_roofline"]["frac"] if bf16_leg and bf16_leg["flop_roofline"] else None,
        "bf16_host_enqueue_ms_per_step": bf16_leg["host_enqueue_ms_per_step"] if bf16_leg else None,
        # configs[4]'s model (S2ANet-R101-FPN, bf16 autocast, channels_last, 4 tiles) and configs[3]'s (Oriented R-CNN +
        # VAN-B3, fp32, 2 tiles) on this one GPU: short legs, own Runner each (`--model s2anet_r101 --dtype bf16` /
        # `--model orcnn_van3` time them in full)
        "r101_bf16_tiles_per_s": extra["r101_bf16"]["value"] if extra.get("r101_bf16") else None,
        "r101_bf16_ms_per_step": extra["r101_bf16"]["ms_per_step"] if extra.get("r101_bf16") else None,
        "r101_bf16_host_enqueue_ms_per_step": extra["r101_bf16"]["host_enqueue_ms_per_step"] if extra.get("r101_bf16") else None,
        "orcnn_tiles_per_s": extra["orcnn"]["value"] if extra.get("orcnn") else None,
        "orcnn_ms_per_step": extra["orcnn"]["ms_per_step"] if extra.get("orcnn") else None,
        "orcnn_host_enqueue_ms_per_step": extra["orcnn"]["host_enqueue_ms_per_step"] if extra.get("orcnn") else None,
        # the TEST path (Runner.predict incl. multiclass_nms_rotated) of configs[1]'s model on resident 1024^2 tiles
        "eval_tiles_per_s_f32_b1": ev("f32_b1"), "eval_tiles_per_s_f32_b4": ev("f32_b4"),
        "eval_tiles_per_s_bf16_b1": ev("bf16_b1"), "eval_tiles_per_s_bf16_b4": ev("bf16_b4"),
        "eval_host_ms_per_call_bf16_b1": (extra["eval"]["bf16_b1"]["host_enqueue_ms_per_call"] if extra.get("eval") else None),
        # SURVEY 8(d) sweeps (all rows: kernels_file): dense IoU at the largest single-tile K on refined anchors, NMS at 20 000
        "iou_k400_refined_two_tier_frac": kf("iou_sweep[two-tier, K=400, refined anchors (seed 7)]", "frac"),
        "iou_k400_refined_bit_exact_frac": kf("iou_sweep[bit-exact, K=400, refined anchors (seed 7)]", "frac"),
        "nms_m20000_label_major_mboxes_per_s": kf("nms_sweep[M=20000, label-major]", "mboxes_per_s"),
        "nms_m20000_score_order_mboxes_per_s": kf("nms_sweep[M=20000, score order]", "mboxes_per_s"),
        # what the run itself saw of the node: one record per rank (device opened, its PCI address and NUMA node, cores
        # pinned), the collective backend and the group size as torch.distributed reports them, the gradient buckets
        "multi_gpu": {"visible_gpus": torch.cuda.device_count(), "backend": facts[0]["backend"],
                      "group_world": facts[0]["group_world"], "ranks": facts,
                      "grad_buckets": mg_buckets, "wire_dtypes": mg_wire},
        "ddp_host_overhead_ms": ddp_leg.get("host_overhead_ms") if ddp_leg else None,
        "ddp": ddp_leg,
        "rotated_iou_mpairs_per_s": dense["mpairs_per_s"] if dense else None,
        # the oriented-box call the timed step itself makes (twice per step: FAM and ODM targets).  Priced against HBM as
        # the contract asks; its algorithmic bytes are tiny (no K x A matrix is written), so the HBM fraction only says
        # "not bandwidth-bound": `issue` is the side that binds (VALU instructions issued / issue slots, SQ counters)
        "roofline": ({k: roof[k] for k in keys} | {
            "bound": "hbm", "bound_note": "latency / VALU-issue bound (5.3 MB algorithmic per call)",
            "kernel": "rsdet_anchor_target_rotated_f32 (tile + finish launches)",
            "source": {"us_per_launch / achieved / frac": "measured in this run (HIP events)",
                       "traffic / issue": COUNTER_SOURCE},
            "us_per_launch": roof["us"], "shape": dense["shape"] if dense else None,
            "issue": issue.get("anchor_target")}) if roof else None,
        "counter_source": COUNTER_SOURCE,
        # the standalone north-star kernel (dense K x A rotated IoU, the matrix written to HBM), not on the step's path
        "roofline_dense_iou": ({k: dense[k] for k in keys} | {
            "kernel": "rsdet_box_iou_rotated_grouped_f32 (bit-exact, 3 launches)",
            "us_per_launch": dense["us"], "shape": dense["shape"], "valu_frac": dense["valu_frac"],
            "overlapping_pairs": dense["overlapping_pairs"]}) if dense else None,
        "roofline_dense_iou_two_tier": ({k: kernels[FAST_ROW][k] for k in keys} | {
            "kernel": "rsdet_box_iou_rotated_fast_f32 (1 launch, two-tier clipper; |d| < 3e-6 of the reference)",
            "us_per_launch": kernels[FAST_ROW]["us"], "mpairs_per_s": kernels[FAST_ROW]["mpairs_per_s"],
            "issue": issue.get("dense_iou_two_tier")})
        if FAST_ROW in kernels else None,
        "roofline_nms": ({k: kernels[NMS_ROW][k] for k in keys} | {
            "kernel": "rsdet_nms_rotated (prepare + mask + sweep), M=5344, 15 classes, label-major",
            "us_per_launch": kernels[NMS_ROW]["us"], "mpairs_per_s": kernels[NMS_ROW]["mpairs_per_s"],
            "issue": issue.get("nms_rotated")}) if NMS_ROW in kernels else None,
        # the hand-written kernel with the most time in the timed step
        "roofline_dominant_handwritten": ({k: kernels[BN_DOM][k] for k in keys} | {
            "kernel": BN_DOM, "us_per_launch": kernels[BN_DOM]["us"]}) if BN_DOM in kernels else None,
        "bf16": bf16_leg,
        "fresh_k": fresh,
        # the conv / GEMM side of the step against the MFMA roofline: flops of one rank's step as counted
        # by torch.utils.flop_counter, over the measured step time, over the dense peak of the compute dtype
        "flop_roofline": None if step_flops is None else {
            "bound": "mfma", "tflop_per_step_per_gpu": step_flops / 1e12,
            "achieved": step_flops / (dt / args.steps) / 1e12, "unit": "TFLOP/s", "peak": peak_f,
            "frac": step_flops / (dt / args.steps) / 1e12 / peak_f},
        "kernels_top12": {k: {"us": r3(v.get("us")), "frac": r3(v.get("frac")), "bound": v.get("bound")} for k, v in top},
        "kernels_file": kfile,
        # the CPU baseline is timed on rank 0 of a single-GPU run only (SURVEY 8d / bench contract)
        "cpu_baseline": None if (args.no_cpu_baseline or world > 1) else cpu_baseline(),
    }
    print(json.dumps(line), flush=True)
    rdist.barrier()
    rdist.shutdown()


if __name__ == "__main__":
    main()
