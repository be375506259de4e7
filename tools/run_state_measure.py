#!/usr/bin/env python
"""The two measurements behind profiles/run_state.txt (needs the MI355X).

  guard   HIP-event time of the fused clip + Adam call on the default network's parameter set, guarded (ttk_clip_adam_guarded) and unguarded
          (ttk_clip_adam) passes alternating in one process; a pass is one replay of a graph of 200 calls.
  save    wall time of one train.save_run_state of the default network (weights + two moments + SWA copy) and the time of an eager training
          epoch (10 * 1024 samples) at B = 64 and B = 512, from which the interval follows at which saving costs under 1 % of the run.

Prints one JSON line per measurement.  usage: python tools/run_state_measure.py guard|save [--out DIR]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "neuralnet-tracker-traincode_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import trackertraincode.train as train  # noqa: E402


def _script():
    import importlib.util

    spec = importlib.util.spec_from_file_location("ttk_train_script", os.path.join(REPO, "neuralnet-tracker-traincode_amd", "scripts", "train_poseestimator.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _default_run(S, extra=()):
    args = S.make_parser().parse_args(list(extra))
    args.input_size = 129
    net = S.create_net(args).to("cuda")
    crit, test_crit = S.setup_losses(args, net)
    opt, sch = S.create_optimizer(net, args)
    return args, net, crit, test_crit, opt, sch


def measure_guard(passes=12, calls=200):
    S = _script()
    _, net, _, _, _, _ = _default_run(S)
    params = [p for p in net.parameters()]
    g = torch.Generator().manual_seed(0)
    for p in params:
        p.grad = (torch.randn(p.shape, generator=g) * 1e-3).to("cuda")
    opts = {name: train.ClipAdam(params, lr=1e-6, max_norm=1.0, skip_nonfinite=name == "guarded") for name in ("unguarded", "guarded")}
    graphs = {}
    for name, o in opts.items():
        for _ in range(5):
            o.step()
        torch.cuda.synchronize()
        # `calls` optimiser calls in ONE captured graph: the events then bracket device time, not the Python loop that enqueues 2 launches per call
        o.sync_hyper_to_device()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(calls):
                o.step()
        graphs[name].replay()
    torch.cuda.synchronize()
    times = {name: [] for name in opts}
    for _ in range(passes):
        for name in opts:  # alternating passes: drift of the box lands on both
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graphs[name].replay()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / calls)
    assert opts["guarded"].health()["skipped"] == 0
    out = {"measurement": "guard", "tensors": len(params), "elements": sum(p.numel() for p in params), "calls_per_pass": calls,
           "us_per_call": {k: [round(v, 2) for v in vs] for k, vs in times.items()},
           "median_us": {k: round(statistics.median(vs), 2) for k, vs in times.items()},
           "min_max_us": {k: [round(min(vs), 2), round(max(vs), 2)] for k, vs in times.items()}}
    return out


def measure_save(out_dir, steps=30, warmup=8):
    S = _script()
    res = {"measurement": "save", "epoch_samples": 10 * 1024}
    for B in (64, 512):
        args, net, crit, test_crit, opt, sch = _default_run(S, ["--batchsize", str(B)])
        tr, te, _ = S.setup_datasets(args, torch.device("cuda", 0))
        it = (b for _ in iter(int, 1) for b in tr)  # epoch after epoch
        swa = train.SwaCallback(start_epoch=-1)
        swa.on_train_start(net)
        dts = []
        for i in range(warmup + steps):
            batches = next(it)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            opt.zero_grad(set_to_none=True)
            out = train.training_step(net, batches, 0, crit)
            out["loss"].backward()
            opt.step()
            torch.cuda.synchronize()
            if i >= warmup:
                dts.append(time.perf_counter() - t0)
        step_ms = statistics.median(dts) * 1e3
        epoch_s = step_ms * 1e-3 * (10 * 1024 // B)
        res[f"B{B}"] = {"eager_step_ms_median": round(step_ms, 3), "steps_per_epoch": 10 * 1024 // B, "epoch_s": round(epoch_s, 3)}
        if B == 64:  # the state does not depend on the batch size
            swa.on_train_epoch_end(0, net)
            ck = train.CheckpointCallback(out_dir)
            saves = []
            path = os.path.join(out_dir, "train_state.pt")
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                train.save_run_state(path, net, opt, sch, next_epoch=1, callbacks=[ck, swa], train_loader=tr, val_loader=te)
                saves.append(time.perf_counter() - t0)
            res["save_s"] = [round(v, 4) for v in saves]
            res["save_s_median"] = round(statistics.median(saves), 4)
            res["state_file_MiB"] = round(os.path.getsize(path) / 2 ** 20, 2)
        del net, opt, tr, te, it
        torch.cuda.empty_cache()
    for B in (64, 512):
        # saving every n epochs costs save / (n * epoch): under 1 % from n = ceil(100 * save / epoch)
        res[f"B{B}"]["interval_epochs_under_1_percent"] = max(1, int(-(-100.0 * res["save_s_median"] // res[f"B{B}"]["epoch_s"])))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["guard", "save"])
    ap.add_argument("--out", default=None, help="save: directory of the state file (default: a temporary one)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("run_state_measure.py measures on the GPU: none found")
    if a.what == "guard":
        print(json.dumps(measure_guard()))
    else:
        with tempfile.TemporaryDirectory() as tmp:
            print(json.dumps(measure_save(a.out or tmp)))


if __name__ == "__main__":
    main()
