"""What train.GraphedTrainStep does step by step, as text that two checkouts can be compared by: per step the loss as a hex float, `captures`,
`eager_only`, the ttk_multi_copy launches that wrote static inputs with the fields they carried, and the fields that fell back to `copy_`.

Four runs of twelve steps at B = 8 on the golden batches (tests/golden/model_full.npz): layout per_tag | flat x a fixed split | a split
that changes every step.  The scheduler steps and the ramped loss weights change (epoch 0 -> 150) after the sixth step.  The batches carry
what the copy-in has to route: int64 convention ids, float32 labels, on odd steps a non-contiguous `roi`, on every fourth step of the
fixed per-Tag run a `pose` that already is the static tensor; in the flat runs the first sub-batch's `dataset_weight` is float64 and the
second sub-batch has none.  A field is named `<static batch>.<field>[<first row>:<last row + 1>]` after the rows of the static input it
was written to.

--pkg DIR runs another checkout's package (DIR/trackertraincode, DIR/libttk_hip.so, DIR/scripts), as tools/mixed_step_bench.py does.  The
losses are only comparable bit for bit with the reductions in their fixed order:

  TTK_DETERMINISTIC=1 python tools/graphed_step_trace.py [--pkg DIR]
"""
import argparse
import importlib.util
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARYING = [5, 2, 8, 5, 0, 7, 3, 6, 5, 1, 4, 5]  # rows of the first Tag, step by step
STEPS, CHANGE = 12, 6


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pkg", default=os.path.join(REPO, "neuralnet-tracker-traincode_amd"))
    args = ap.parse_args()
    if os.environ.get("TTK_DETERMINISTIC", "0") == "0":
        sys.exit("graphed_step_trace.py: set TTK_DETERMINISTIC=1 (the losses are compared bit for bit)")
    sys.path[:0] = [args.pkg, REPO, os.path.join(REPO, "tests")]
    import numpy as np
    import torch
    import warnings

    import trackertraincode.train as train
    from oracle.synth import make_inputs, make_labels
    from trackertraincode import _hip
    from trackertraincode.datasets.batch import Batch, Metadata
    from trackertraincode.pipelines import Tag
    from util import build_net, load_golden, script_args

    spec = importlib.util.spec_from_file_location("amd_train_script", os.path.join(args.pkg, "scripts", "train_poseestimator.py"))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    dev = torch.device("cuda", 0)
    _, meta = load_golden("model_full.npz")
    B = meta["B"]
    image, ids = make_inputs(B, seed=meta["input_seed"])
    lab = make_labels(B, seed=meta["input_seed"])

    def batches(k, step, flat):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        out = []
        for j, (tag, rows, fields) in enumerate(((Tag.POSE_WITH_LANDMARKS, slice(0, k), ("pose", "coord", "roi", "pt3d_68", "shapeparam")),
                                                 (Tag.ONLY_POSE, slice(k, B), ("pose", "coord", "roi")))):
            if len(range(B)[rows]) == 0:
                continue
            d = dict(image=t(image[rows][..., ::-1] if step % 2 else image[rows]), coord_convention_id=t(ids[rows]).long(), **{f: t(lab[f][rows]) for f in fields})
            if step % 2:
                d["roi"] = d["roi"].t().contiguous().t()
            if not flat:
                d["dataset_weight"] = t(lab["dataset_weight"][rows])
            elif j == 0:
                d["dataset_weight"] = t(lab["dataset_weight"][rows]).double()
            out.append(Batch(Metadata(129, batchsize=len(range(B)[rows]), tag=tag), d))
        return out

    lib = _hip.lib()
    lib_copy, tensor_copy, device_sync = lib.multi_copy, torch.Tensor.copy_, torch.cuda.synchronize
    for layout in ("per_tag", "flat"):
        for split in ("fixed", "varying"):
            net = build_net(meta, dev).train()
            crit, _ = S.setup_losses(script_args(meta["flags"]), net)
            opt, sch = S.create_optimizer(net, script_args(meta["flags"], epochs=20))
            g = train.GraphedTrainStep(net, crit, opt, layout=layout)
            for i in range(STEPS):
                if i == CHANGE:
                    sch.step()
                bs = batches(meta["split"] if split == "fixed" else VARYING[i], i, layout == "flat")
                if layout == "per_tag" and split == "fixed" and i % 4 == 3:
                    bs[1]["pose"] = g._static[1]["pose"]
                launches, fallbacks, synced = [], [], []

                def spy_multi(srcs, dsts):
                    launches.append([(d.data_ptr(), d.numel() * d.element_size()) for d in dsts])
                    return lib_copy(srcs, dsts)

                def spy_copy(self, *a, **kw):
                    if self.is_cuda:
                        fallbacks.append((self.data_ptr(), self.numel() * self.element_size()))
                    return tensor_copy(self, *a, **kw)

                def spy_sync(*a, **kw):
                    # run() synchronises between the eager first step and building the static inputs (the first synchronise of such a step;
                    # opening the capture is another): what the eager step copied went to memory that is free again, and the static inputs
                    # may be allocated right there
                    if not synced:
                        launches.clear(), fallbacks.clear()
                    synced.append(1)
                    return device_sync(*a, **kw)

                lib.multi_copy, torch.Tensor.copy_, torch.cuda.synchronize = spy_multi, spy_copy, spy_sync
                try:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore", RuntimeWarning)
                        loss = g.run(bs, 0 if i < CHANGE else 150)["loss"].item()
                finally:
                    lib.multi_copy, torch.Tensor.copy_, torch.cuda.synchronize = lib_copy, tensor_copy, device_sync
                # the static inputs as they are after the step (`_flat`: where checkouts before the single driver kept the flat buffers)
                static = [(f"{j}.{k}", v) for j, b in enumerate(list(g._static) or [getattr(g, "_flat", {})]) for k, v in b.items() if v.dim() and v.numel()]

                def name(ptr, nbytes):
                    for label, v in static:
                        row = v.numel() * v.element_size() // int(v.shape[0])
                        if v.data_ptr() <= ptr < v.data_ptr() + v.numel() * v.element_size():
                            return f"{label}[{(ptr - v.data_ptr()) // row}:{(ptr - v.data_ptr() + nbytes) // row}]"
                    return None

                words = [sorted(n for n in (name(*d) for d in dsts) if n) for dsts in launches]
                words = [w for w in words if w]
                print(f"{layout} {split} step {i:2d} loss {float(loss).hex()} captures {g.captures} eager_only {g.eager_only} multi_copy {len(words)} "
                      f"words {words} copy_ {sorted(n for n in (name(*d) for d in fallbacks) if n)}", flush=True)


if __name__ == "__main__":
    main()
