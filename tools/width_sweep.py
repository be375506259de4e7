#!/usr/bin/env python3
"""Training-step time of width-scaled MobileNet backbones (MobileNet(widen_factor=w)) on one MI355X, measured the way bench.py measures
its headline (which builds width 1.0 only): the WHOLE step (forward + losses + backward + clip + Adam) at B = 512 with default flags,
replayed as one captured hipGraph, every width built and warmed up first, then timed in windows of at least one second of GPU work.  The
widths alternate inside one process, in two passes, so the run-to-run spread is visible next to the differences.

Per width it prints crops/s and ms/step of both passes, the ALGORITHMIC HBM bytes and FLOPs of one step (from the layer shapes, below:
every activation-sized tensor counted once per kernel that reads or writes it, 2 FLOPs per multiply-add) and the fraction of the peak that
the faster bound allows: 8 TB/s of HBM, or the 155 TFLOP/s of the exact-fp32 matrix instruction for the any-channel-count GEMMs
(fp16-split layers: three products on the 16-bit pipe, counted against 3 x their FLOPs at 2.5 PFLOP/s - never the bound).

  python tools/width_sweep.py [--out profiles/width_sweep] [--widths 0.25,0.5,...] [--batch 512] [--commit <sha>]
A per-kernel table of one width comes from a separate run under the profiler:
  rocprofv3 --kernel-trace --stats -- python tools/width_sweep.py --widths 0.75 --passes 1 --window 0.2 --out /tmp/x"""
from __future__ import annotations

import argparse
import json
import os
import socket
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (REPO, os.path.join(REPO, "neuralnet-tracker-traincode_amd"), os.path.join(REPO, "tools")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

HBM_BYTES_PER_S = 8.0e12
FP32_MFMA_FLOPS = 155.0e12
FP16_MFMA_FLOPS = 2.5e15


def step_model(net, B, H=129):
    """Algorithmic traffic and arithmetic of one training step of the backbone, from the block table and the kernel plan.
    Tensors (fp32): x = block input [M_in, Cin], d = depthwise output [M, Cin], y = pointwise output [M, Cout].
      forward : depthwise reads x (+ the residual input of the producer), writes d (+ the materialised input of a residual block);
                pointwise reads d, writes y
      backward: pointwise weight gradient reads g_y, y, d; data gradient reads g_y, y, d, writes g_d; depthwise reads g_d, d, x
                (+ residual operands), writes g_x
    The stem, the pool, the heads and the optimiser are a few per cent and are left out of the bound (they are in the measured time)."""
    from trackertraincode.backbones.mobilenet_v1 import _tuned_c

    h = (H + 1) // 2
    c0 = net.conv1.out_channels
    by = 4 * B * (H * H + 2 * h * h * c0)  # stem forward: x, y; backward re-reads g, y, x
    by += 4 * B * (H * H + 2 * h * h * c0)
    fl_valu = 2 * 2.0 * 25 * B * h * h * c0  # stem: forward + weight gradient
    fl_fp32 = fl_fp16 = 0.0
    for _, cin, cout, stride in net._blocks:
        ho = (h - 1) // stride + 1
        Mi, M = B * h * h, B * ho * ho
        skip = stride == 1 and cin == cout
        fwd = Mi * cin + M * cin + (Mi * cin if skip else 0) + M * cin + M * cout
        bwd = (2 * M * cout + M * cin) + (2 * M * cout + 2 * M * cin) + (2 * M * cin + 2 * Mi * cin + (2 * Mi * cin if skip else 0))
        by += 4 * (fwd + bwd)
        gemm = 3 * 2.0 * M * cin * cout  # forward, data gradient, weight gradient
        if _tuned_c(cin) and _tuned_c(cout) and cin >= 64:
            fl_fp16 += gemm
        else:
            fl_fp32 += gemm
        fl_valu += 3 * 2.0 * 9 * M * cin
        h = ho
    t_hbm = by / HBM_BYTES_PER_S
    t_mm = fl_fp32 / FP32_MFMA_FLOPS + 3 * fl_fp16 / FP16_MFMA_FLOPS
    return {"hbm_bytes": by, "flops_fp32_mfma": fl_fp32, "flops_fp16_split": fl_fp16, "flops_depthwise_valu": fl_valu,
            "floor_ms_hbm": t_hbm * 1e3, "floor_ms_matrix": t_mm * 1e3, "bound": "HBM 8 TB/s" if t_hbm >= t_mm else "fp32 MFMA 155 TF"}


def build(width, batch, device):
    import argparse as _ap

    import bench

    a = _ap.Namespace(backbone="mobilenetv1", blurpool=False, precision="fp32", batch=batch, seed=0)
    if width == 1.0:
        return bench.build_step(a, device)  # exactly bench.py's network
    import torch
    import trackertraincode.train as train
    from trackertraincode.neuralnets.models import NetworkWithPointHead
    from trackertraincode.pipelines import SyntheticPoseLoader, Tag

    import importlib.util

    spec = importlib.util.spec_from_file_location("amd_train_script", os.path.join(REPO, "neuralnet-tracker-traincode_amd", "scripts", "train_poseestimator.py"))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    ns = S.make_parser().parse_args(["--widen-factor", str(width)])
    torch.manual_seed(0)
    net = S.create_net(ns)
    g = torch.Generator().manual_seed(7)
    net.landmarks.deformablekeypoints.set_basis(torch.randn(68, 3, generator=g) * 0.5, torch.randn(50, 68, 3, generator=g) * 0.05)
    net = net.to(device).train()
    crit, _ = S.setup_losses(ns, net)
    opt, _ = S.create_optimizer(net, ns)
    loader = SyntheticPoseLoader(batch, [(Tag.POSE_WITH_LANDMARKS, 110.0), (Tag.POSE_WITH_LMKS_NO_SHAPE_PARAMS, 10.0)], device=device, seed=1234)
    return net, crit, opt, next(iter(loader)), train


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="0.25,0.5,0.75,1.0,1.5,2.0")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of GPU work per timed window (at least)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "width_sweep"))
    ap.add_argument("--commit", default=None, help="git commit the tree was taken from (a GPU box's snapshot has no .git)")
    args = ap.parse_args()
    import torch

    import build_id

    device = torch.device("cuda", 0)
    widths = [float(w) for w in args.widths.split(",")]
    steps, models = {}, {}
    for w in widths:  # build, capture and warm up every width first
        net, crit, opt, batches, train = build(w, args.batch, device)
        graphed = train.GraphedTrainStep(net, crit, opt)
        run = (lambda gr, bs: (lambda: gr.run(bs, 0)["loss"]))(graphed, batches)
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        est = (time.perf_counter() - t0) / 5
        steps[w] = (run, max(10, int(args.window / est) + 1), net)
        models[w] = step_model(net.convnet, args.batch)
        models[w]["anyc_layers"] = sum(f == "anyc" for _, f in net.convnet.kernel_plan())
    res = {w: [] for w in widths}
    for _ in range(args.passes):
        for w in widths:
            run, n, _net = steps[w]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                loss = run()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert torch.isfinite(loss), (w, loss)
            res[w].append({"ms_per_step": dt / n * 1e3, "crops_per_s": args.batch * n / dt, "steps": n})
    head = (f"width sweep: whole training step, B = {args.batch}, fp32, hipGraph replay, {args.passes} alternating passes, >= {args.window} s per window\n"
            f"host {socket.gethostname()}  device {torch.cuda.get_device_name(0)}  commit {args.commit or 'unknown'}  csrc_sha256 {build_id.csrc_sha256()}\n")
    lines = [head, f"{'width':>6} {'anyc':>5} " + " ".join(f"{'ms/step p%d' % (i + 1):>12} {'crops/s p%d' % (i + 1):>12}" for i in range(args.passes))
             + f" {'HBM GB':>8} {'GFLOP f32mm':>12} {'GFLOP f16x3':>12} {'floor ms':>9} {'of peak':>8}  bound"]
    for w in widths:
        m = models[w]
        best = min(r["ms_per_step"] for r in res[w])
        floor = max(m["floor_ms_hbm"], m["floor_ms_matrix"])
        m["fraction_of_bound"] = floor / best
        lines.append(f"{w:>6} {m['anyc_layers']:>5} " + " ".join(f"{r['ms_per_step']:>12.3f} {r['crops_per_s']:>12.0f}" for r in res[w])
                     + f" {m['hbm_bytes'] / 1e9:>8.2f} {m['flops_fp32_mfma'] / 1e9:>12.1f} {m['flops_fp16_split'] / 1e9:>12.1f} {floor:>9.3f} {floor / best:>8.2f}  {m['bound']}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out + ".txt", "w").write(text)
    json.dump({"batch": args.batch, "host": socket.gethostname(), "device": torch.cuda.get_device_name(0), "commit": args.commit,
               "csrc_sha256": build_id.csrc_sha256(), "widths": {str(w): {"passes": res[w], **models[w]} for w in widths}}, open(args.out + ".json", "w"), indent=1)


if __name__ == "__main__":
    main()
