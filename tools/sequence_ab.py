"""Python against native launch sequence of the MobileNet backbone (MobileNet.set_sequence): host enqueue time of the EAGER step.  (GPU box)

One process, one network per (batch, precision), the two sequences ALTERNATING pass by pass on it: a pass is `--steps` steps (default 20), each
timed on the host clock from an idle GPU (synchronise, start, enqueue, stop - no synchronise inside the window: what is measured is the enqueue,
not the kernels), reported as the median over `--passes` passes (default 7, >= 5) after one untimed pass, with the passes' minimum and maximum as the spread
and the pass-by-pass difference beside it (a drift of the host's clocks moves both sequences of a pass together).
  backbone    forward_features + backward of the backbone alone (what the native sequence replaces)
  step        training_step + backward of the whole pose estimator (heads and losses still enqueue from Python)
  wall        the same steps back to back with one synchronise at the end: what a step costs when nothing overlaps it
and torch.cuda.max_memory_allocated of one B = 512 step per sequence: the native workspaces cannot release tensors progressively as the Python
backward does (its g / g_prev pairs and the autograd context die layer by layer), so the peak differs.  No profiler is attached.

    python tools/sequence_ab.py [--out profiles/native_sequence.txt] [--batches 64,512] [--passes 7] [--steps 20]
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "neuralnet-tracker-traincode_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "native_sequence.txt"))
ap.add_argument("--batches", default="64,512")
ap.add_argument("--passes", type=int, default=7)
ap.add_argument("--steps", type=int, default=20)
opts = ap.parse_args()
assert opts.passes >= 5
sys.argv = sys.argv[:1]

import torch  # noqa: E402

import bench  # noqa: E402

dev = torch.device("cuda", 0)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed_pass(fn, steps):
    """Host ms per step of `steps` steps, each enqueued on an idle GPU."""
    total = 0.0
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        total += time.perf_counter() - t0
    torch.cuda.synchronize()
    return 1e3 * total / steps


def wall_pass(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def fmt(v):
    return f"{statistics.median(v):6.3f} [{min(v):6.3f} .. {max(v):6.3f}]"


say(f"# tools/sequence_ab.py: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; ms per step, median [min .. max] of {opts.passes} passes of "
    f"{opts.steps} steps, sequences alternating pass by pass")
verdicts = []
for B in [int(b) for b in opts.batches.split(",")]:
    for precision in ("fp32", "bf16-compute"):
        args = bench.parse()
        args.batch, args.precision = B, precision
        net, crit, opt, batches, train = bench.build_step(args, dev)
        params = list(net.parameters())
        x = torch.concat([b["image"] for b in batches]) if len(batches) > 1 else batches[0]["image"]
        ones = torch.ones(x.shape[0], net.convnet.num_features, device=dev)

        def backbone():
            for q in params:
                q.grad = None
            net.convnet.forward_features(x).backward(ones)

        def step():
            for q in params:
                q.grad = None
            train.training_step(net, batches, 0, crit)["loss"].backward()

        res = {(seq, what): [] for seq in ("python", "native") for what in ("backbone", "step", "wall")}
        for seq in ("python", "native"):  # warm-up: code objects, plans, the allocator's blocks
            net.convnet.set_sequence(seq)
            for _ in range(5):
                backbone()
                step()
        for seq in ("python", "native"):  # ... and one untimed pass of each: the host's clocks settle over the first few hundred steps
            net.convnet.set_sequence(seq)
            timed_pass(backbone, opts.steps), timed_pass(step, opts.steps), wall_pass(step, opts.steps)
        for _ in range(opts.passes):
            for seq in ("python", "native"):
                net.convnet.set_sequence(seq)
                res[seq, "backbone"].append(timed_pass(backbone, opts.steps))
                res[seq, "step"].append(timed_pass(step, opts.steps))
                res[seq, "wall"].append(wall_pass(step, opts.steps))
        say(f"\nB = {B}, {precision} (backbone batch {x.shape[0]})")
        for what, label in (("backbone", "host enqueue, backbone only"), ("step", "host enqueue, whole step   "), ("wall", "wall time, whole step     ")):
            say(f"  {label}   python {fmt(res['python', what])}   native {fmt(res['native', what])}")
        py, nat = res["python", "backbone"], res["native", "backbone"]
        gain = statistics.median(py) - statistics.median(nat)
        spread = max(max(py) - min(py), max(nat) - min(nat))
        clear = min(py) > max(nat)
        paired = [a - b for a, b in zip(py, nat)]  # (pass i of one sequence ran right before pass i of the other)
        say(f"  backbone enqueue: native lower by {gain:.3f} ms (median); spread of the passes {spread:.3f} ms; every native pass below every python pass: {clear}; "
            f"pass by pass (python - native) {fmt(paired)}")
        verdicts.append(gain > spread and clear)
        if B == 512:
            for seq in ("python", "native"):
                net.convnet.set_sequence(seq)
                step()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                step()
                torch.cuda.synchronize()
                say(f"  peak memory of one step, {seq:6s}: max_memory_allocated {torch.cuda.max_memory_allocated() / 2**20:8.1f} MiB "
                    f"({(torch.cuda.max_memory_allocated() - base) / 2**20:8.1f} MiB above the {base / 2**20:.1f} MiB held before it)")
        del net, crit, opt, batches, params, x, ones
        torch.cuda.empty_cache()
say(f"\nnative backbone enqueue lower than python by more than the spread of the passes in {sum(verdicts)} of {len(verdicts)} configurations")
os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
with open(opts.out, "w") as f:
    f.write("\n".join(lines) + "\n")
