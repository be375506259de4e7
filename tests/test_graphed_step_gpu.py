"""train.GraphedTrainStep as ONE protocol under both layouts: how new batches reach the graph's static inputs, that the owner of the object can
free a live capture, and that capture and replay happen where they should and nowhere else.  B = 8, the rows of the golden step
(tests/golden/model_full.npz) as 5 POSE_WITH_LANDMARKS + 3 ONLY_POSE rows.  The expected routing and the capture / replay counts are those of
the class as it was before it had a single driver, read off tools/graphed_step_trace.py (profiles/graphed_step_refactor.txt).  What a replayed
step computes is held by test_model_gpu, test_flat_step_gpu and test_landmark_step_gpu."""
import gc
import weakref

import numpy as np
import pytest
import torch

from oracle.synth import make_inputs, make_labels
from util import build_net, load_golden, script_args, train_script

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAYOUTS = ["per_tag", "flat"]


def _run(layout):
    import trackertraincode.train as train

    _, meta = load_golden("model_full.npz")
    S = train_script()
    net = build_net(meta, DEV).train()
    crit, _ = S.setup_losses(script_args(meta["flags"]), net)
    opt, sch = S.create_optimizer(net, script_args(meta["flags"], epochs=20))
    return meta, train.GraphedTrainStep(net, crit, opt, layout=layout), sch


def _batches(meta, step, flat):
    """The batches of tools/graphed_step_trace.py's fixed split: int64 convention ids, float32 labels, on odd steps mirrored images and a
    non-contiguous `roi`; per-Tag a float32 `dataset_weight` in both sub-batches, flat a float64 one in the first and none in the second."""
    from trackertraincode.datasets.batch import Batch, Metadata
    from trackertraincode.pipelines import Tag

    B, k = meta["B"], meta["split"]
    image, ids = make_inputs(B, seed=meta["input_seed"])
    lab = make_labels(B, seed=meta["input_seed"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    out = []
    for j, (tag, rows, fields) in enumerate(((Tag.POSE_WITH_LANDMARKS, slice(0, k), ("pose", "coord", "roi", "pt3d_68", "shapeparam")),
                                             (Tag.ONLY_POSE, slice(k, B), ("pose", "coord", "roi")))):
        d = dict(image=t(image[rows][..., ::-1] if step % 2 else image[rows]), coord_convention_id=t(ids[rows]).long(), **{f: t(lab[f][rows]) for f in fields})
        if step % 2:
            d["roi"] = d["roi"].t().contiguous().t()
            assert not d["roi"].is_contiguous()
        if not flat:
            d["dataset_weight"] = t(lab["dataset_weight"][rows])
        elif j == 0:
            d["dataset_weight"] = t(lab["dataset_weight"][rows]).double()
        out.append(Batch(Metadata(129, batchsize=len(range(B)[rows]), tag=tag), d))
    return out


def _static_name(g, ptr, nbytes):
    """`<static batch>.<field>[<rows>]` of the static input that holds the bytes at `ptr`, None when none does."""
    for j, b in enumerate(g._static):
        for k, v in b.items():
            size = v.numel() * v.element_size()
            if v.data_ptr() <= ptr < v.data_ptr() + size:
                row = size // int(v.shape[0])
                return f"{j}.{k}[{(ptr - v.data_ptr()) // row}:{(ptr - v.data_ptr() + nbytes) // row}]"
    return None


# per replay: the fields of the ONE ttk_multi_copy launch, the fields that fell back to copy_ (profiles/graphed_step_refactor.txt)
PER_TAG_ALL = {f"0.{f}[0:5]" for f in ("image", "coord_convention_id", "pose", "coord", "roi", "pt3d_68", "shapeparam", "dataset_weight")} | \
              {f"1.{f}[0:3]" for f in ("image", "coord_convention_id", "pose", "coord", "roi", "dataset_weight")}
FLAT_ALL = {f"0.{f}[0:5]" for f in ("tag_code", "image", "coord_convention_id", "pose", "coord", "roi", "pt3d_68", "shapeparam", "dataset_weight")} | \
           {f"0.{f}[5:8]" for f in ("tag_code", "image", "coord_convention_id", "pose", "coord", "roi", "dataset_weight")}
ROUTING = {  # layout -> step -> (words, fallbacks)
    "per_tag": {1: (PER_TAG_ALL - {"0.roi[0:5]", "1.roi[0:3]"}, {"0.roi[0:5]", "1.roi[0:3]"}),
                2: (PER_TAG_ALL, set()),
                3: (PER_TAG_ALL - {"0.roi[0:5]", "1.roi[0:3]", "1.pose[0:3]"}, {"0.roi[0:5]", "1.roi[0:3]"})},  # (1.pose is the static tensor)
    "flat": {1: (FLAT_ALL - {"0.roi[0:5]", "0.roi[5:8]"}, {"0.roi[0:5]", "0.roi[5:8]"}),
             2: (FLAT_ALL, set()),
             3: (FLAT_ALL - {"0.roi[0:5]", "0.roi[5:8]"}, {"0.roi[0:5]", "0.roi[5:8]"})},
}


@pytest.mark.parametrize("layout", LAYOUTS)
def test_copy_in_routing(layout, monkeypatch):
    """Every replay moves its batches into the static inputs with ONE ttk_multi_copy launch for whatever can travel as 32-bit words (int64
    ids, float32 labels, the flat layout's Tag codes and float32 weights - the float64 ones converted, ones where a sub-batch has none) and
    copy_ for the rest (a non-contiguous field); a field that already is the static tensor is left alone.  Afterwards the static inputs
    hold the sources bit for bit."""
    from trackertraincode import _hip
    from trackertraincode.train import _tag_code

    meta, g, _ = _run(layout)
    lib = _hip.lib()
    lib_copy, tensor_copy = lib.multi_copy, torch.Tensor.copy_
    launches, fallbacks = [], []
    monkeypatch.setattr(lib, "multi_copy", lambda s, d: (launches.append([(x.data_ptr(), x.numel() * x.element_size()) for x in d]), lib_copy(s, d))[1])
    monkeypatch.setattr(torch.Tensor, "copy_", lambda self, *a, **kw: (fallbacks.append((self.data_ptr(), self.numel() * self.element_size())),
                                                                      tensor_copy(self, *a, **kw))[1])
    for step in range(4):
        bs = _batches(meta, step, layout == "flat")
        if layout == "per_tag" and step == 3:
            g._static[1]["pose"].copy_(bs[1]["pose"].flip(0))  # what a loader that writes into the static tensor does
            bs[1]["pose"] = g._static[1]["pose"]
        launches.clear(), fallbacks.clear()
        g.run(bs, 0)
        if step == 0:
            assert g.captures == 1
            continue
        words = [{n for n in (_static_name(g, *x) for x in d) if n} for d in launches]
        copied = {n for n in (_static_name(g, *x) for x in fallbacks) if n}
        print(f"ROUTING {layout} step {step}: {len(launches)} launch(es), words {sorted(map(sorted, words))}, copy_ {sorted(copied)}")
        assert len(launches) == 1, "a replay runs no eager forward: every ttk_multi_copy launch is the copy-in"
        assert (words[0], copied) == ROUTING[layout][step]
        off = 0
        for j, b in enumerate(bs):
            n = b.meta.batchsize
            held = g._static[j] if layout == "per_tag" else {k: v[off:off + n] for k, v in g._static[0].items()}
            for k, v in b.items():
                assert torch.equal(held[k], v.to(held[k].dtype) if k == "dataset_weight" else v), (step, j, k)
                assert k == "dataset_weight" or held[k].dtype == v.dtype
            if layout == "flat":
                assert held["tag_code"].tolist() == [_tag_code(b.meta.tag)] * n
                assert "dataset_weight" in b or held["dataset_weight"].tolist() == [1.0] * n
            off += n
    assert g.captures == 1 and not g.eager_only


@pytest.mark.parametrize("layout", LAYOUTS)
def test_three_assignments_release_a_live_capture(layout):
    """bench.py drops a capture it will not use with `graph = _out = None; _static = []`: after exactly that nothing in the object may keep
    the graph, its outputs or its static inputs (and with them the graph's private memory pool) alive."""
    meta, g, _ = _run(layout)
    for step in range(2):
        g.run(_batches(meta, step, layout == "flat"), 0)
    torch.cuda.synchronize()
    assert g.captures == 1 and len(g._static) == (2 if layout == "per_tag" else 1)
    tensors = [v for b in g._static for v in b.values()] + [g._out["loss"]] + [v for k in g._out if k != "loss" for v in g._out[k].values()]
    assert all(torch.is_tensor(v) for v in tensors)
    refs = {"graph": weakref.ref(g.graph), **{f"tensor {i}": weakref.ref(v) for i, v in enumerate(tensors)}}
    del tensors
    g.graph = g._out = None
    g._static = []
    gc.collect()
    assert [n for n, r in refs.items() if r() is not None] == []


@pytest.mark.parametrize("layout, captures, replays", [("per_tag", 2, 4), ("flat", 1, 5)])
def test_one_capture_and_one_replay_path(layout, captures, replays, monkeypatch):
    """Six steps, the scheduler stepping and the ramped loss weights changing after the third.  The weights are launch constants of the per-Tag
    step (one re-capture) and a device table of the flat one (none); every other step is a replay - counted at torch.cuda.graph and
    CUDAGraph.replay themselves, so a second path to either would show."""
    meta, g, sch = _run(layout)
    opened, replayed = [], []
    graph_cm, replay = torch.cuda.graph, torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda, "graph", lambda *a, **kw: (opened.append(1), graph_cm(*a, **kw))[1])
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replayed.append(1), replay(self))[1])
    losses = []
    for step in range(6):
        if step == 3:
            sch.step()
        losses.append(g.run(_batches(meta, step, layout == "flat"), 0 if step < 3 else 150)["loss"].item())
    torch.cuda.synchronize()
    print(f"PATHS {layout}: captures {g.captures}, torch.cuda.graph opened {len(opened)}, replays {len(replayed)}, losses {losses}")
    assert (g.captures, len(opened), len(replayed)) == (captures, captures, replays)
    assert not g.eager_only and g.optimizer._t == 6 and all(np.isfinite(losses))
