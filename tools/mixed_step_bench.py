"""Step time of a training step whose per-Tag split changes every step (the Tag mix of BASELINE config 5, POSE_WITH_LANDMARKS :
POSE_WITH_LMKS_NO_SHAPE_PARAMS = 110 000 : 10 000, drawn per step), network and losses of bench.py's headline:

  a  eager per-Tag steps            - what --graph-steps degrades to on such a loader (GraphedTrainStep's fallback)
  b  ONE flat graph                 - GraphedTrainStep(layout="flat"), --graph-steps --graph-layout flat
  c  per-Tag graph of a FIXED split - the existing replay, as the ceiling (it cannot follow a varying split)

over precision x batch size.  The step's batches come from a pool drawn before the clock starts (the loaders' own launches are not
part of the step); per leg 5 warm-up steps, then windows of at least --steps steps and --seconds seconds, host clock around a device
synchronise; --reps rounds with the legs alternating.  `host_ms` is the host time to enqueue a window's steps (before the final
synchronise): where it equals the step time the leg is host-bound.  One JSON line per (precision, batch), then a table.

--pkg DIR runs against another checkout's package (DIR/trackertraincode, DIR/libttk_hip.so) - leg a of the parent commit beside
this tree's, to show the default path did not move (the tool draws the splits itself, so it needs nothing of the feature for leg a).

  python tools/mixed_step_bench.py                              # the whole sweep
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/mixed_step_bench.py --legs b --precision fp32 --batch 512 --reps 1
"""
import argparse
import importlib.util
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX = (("POSE_WITH_LANDMARKS", 110000.0), ("POSE_WITH_LMKS_NO_SHAPE_PARAMS", 10000.0))


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--precision", nargs="+", default=["fp32", "bf16-compute"])
    ap.add_argument("--batch", nargs="+", type=int, default=[64, 256, 512])
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--steps", type=int, default=100, help="timed steps per window at least")
    ap.add_argument("--seconds", type=float, default=0.5, help="window length at least")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pool", type=int, default=8, help="distinct splits the step cycles through")
    ap.add_argument("--pkg", default=os.path.join(REPO, "neuralnet-tracker-traincode_amd"))
    ap.add_argument("--label", default="this tree")
    return ap.parse_args()


def main():
    args = parse()
    sys.path.insert(0, args.pkg)
    import torch

    import trackertraincode.train as train
    from trackertraincode import pipelines as P
    from trackertraincode.neuralnets.models import NetworkWithPointHead

    spec = importlib.util.spec_from_file_location("amd_train_script", os.path.join(args.pkg, "scripts", "train_poseestimator.py"))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    tags = [(getattr(P.Tag, n), w) for n, w in MIX]

    def script_args(flags):
        ns = S.make_parser().parse_args([])
        for k, v in flags.items():
            setattr(ns, k, v)
        return ns

    def build(precision):  # bench.py build_step
        torch.manual_seed(0)
        net = NetworkWithPointHead(enable_point_head=True, enable_uncertainty=False, config="mobilenetv1", backbone_args={"use_blurpool": False})
        g = torch.Generator().manual_seed(7)
        net.landmarks.deformablekeypoints.set_basis(torch.randn(68, 3, generator=g) * 0.5, torch.randn(50, 68, 3, generator=g) * 0.05)
        net = net.to(device).train()
        net.convnet.set_precision(precision)
        flags = dict(with_pointhead=True, with_nll_loss=False, rampup_nll_losses=False)
        crit, _ = S.setup_losses(script_args(flags), net)
        opt, _ = S.create_optimizer(net, script_args(flags))
        return net, crit, opt

    def pools(B):
        gen = torch.Generator().manual_seed(1234)
        draw = torch.Generator().manual_seed(4321)
        probs = torch.tensor([w for _, w in tags], dtype=torch.float64)
        probs /= probs.sum()
        varying = []
        while len(varying) < args.pool:
            counts = torch.bincount(torch.multinomial(probs, B, replacement=True, generator=draw), minlength=len(tags)).tolist()
            if all(counts):  # (every step of the pool holds both Tags: the per-Tag step then always has two sub-batches)
                varying.append([P.synthetic_subbatch(t, c, device, gen) for (t, _), c in zip(tags, counts)])
        fixed = next(iter(P.SyntheticPoseLoader(B, tags, device=device, seed=1234)))
        return varying, fixed, [[b.meta.batchsize for b in bs] for bs in varying]

    def make_leg(leg, precision, varying, fixed):
        net, crit, opt = build(precision)
        if leg == "a":
            def step(i):
                opt.zero_grad(set_to_none=True)
                out = train.training_step(net, varying[i % len(varying)], 0, crit)
                out["loss"].backward()
                opt.step()
                return out
            return step, None
        g = train.GraphedTrainStep(net, crit, opt, layout="flat") if leg == "b" else train.GraphedTrainStep(net, crit, opt)
        return (lambda i: g.run(varying[i % len(varying)] if leg == "b" else fixed, 0)), g

    def window(step, n, start):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            out = step(start + i)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t2 - t0) / n * 1e3, (t1 - t0) / n * 1e3, float(out["loss"].item())

    rows = []
    for precision in args.precision:
        for B in args.batch:
            varying, fixed, sizes = pools(B)
            legs, res = {}, {}
            for leg in args.legs:
                step, g = make_leg(leg, precision, varying, fixed)
                for i in range(args.warmup):
                    step(i)
                est, _, _ = window(step, 20, args.warmup)
                legs[leg] = (step, g, max(args.steps, int(math.ceil(1.2 * args.seconds * 1e3 / est))))
                res[leg] = {"step_ms": [], "host_ms": []}
            for rep in range(args.reps):  # the legs alternate
                for leg, (step, g, n) in legs.items():
                    ms, host, loss = window(step, n, args.warmup + 20 + rep * n)
                    if not math.isfinite(loss):
                        raise RuntimeError(f"leg {leg} {precision} B={B}: loss {loss}")
                    res[leg]["step_ms"].append(round(ms, 4))
                    res[leg]["host_ms"].append(round(host, 4))
            for leg, (step, g, n) in legs.items():
                res[leg]["steps_per_window"] = n
                if g is not None:
                    res[leg]["captures"], res[leg]["eager_only"] = g.captures, g.eager_only
            row = {"tree": args.label, "precision": precision, "batch": B, "splits": sizes, "legs": res}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del legs, varying, fixed
            torch.cuda.empty_cache()
    names = {"a": "eager per-Tag", "b": "flat graph", "c": "fixed-split graph"}
    print(f"\n{args.label}: ms per step, median of {args.reps} windows (min - max); host = enqueue time per step")
    for row in rows:
        for leg, r in row["legs"].items():
            s, h = r["step_ms"], r["host_ms"]
            print(f"  {row['precision']:<13} B={row['batch']:<4} {leg} {names[leg]:<18} {statistics.median(s):7.3f} ({min(s):.3f} - {max(s):.3f})   host {statistics.median(h):6.3f}"
                  f"   {row['batch'] / statistics.median(s):6.1f} k crops/s" + (f"   captures {r['captures']}" if "captures" in r else ""))


if __name__ == "__main__":
    main()
