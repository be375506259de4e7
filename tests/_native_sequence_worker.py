"""Worker of tests/test_native_sequence_gpu.py, started with TTK_DETERMINISTIC=1 (the mode is read once per process): the Python and the native
launch sequence on identical weights, buffers and inputs.  Prints one line "RESULT <json>":
  grads[<case>]  names of the gradient tensors (and "feat") that differ bitwise between the two sequences - expected empty;
  step           three ClipAdam steps of the pose estimator (model_default.npz, B = 8) per sequence: the losses as hex floats and a hash of every
                 parameter and buffer afterwards;
  graph          four native steps eager, and four through train.GraphedTrainStep (one eager, three replays): the losses as hex floats."""
import copy
import hashlib
import json
import sys

REPO = sys.argv[1]
sys.path.insert(0, REPO)
sys.path.insert(0, REPO + "/neuralnet-tracker-traincode_amd")
sys.path.insert(0, REPO + "/tests")

import torch  # noqa: E402

import trackertraincode.backbones.mobilenet_v1 as MB  # noqa: E402
import trackertraincode.train as train  # noqa: E402
from test_native_sequence_gpu import make_backbone, one_pass  # noqa: E402
from util import build_net, load_golden, make_batches, script_args, train_script  # noqa: E402

assert MB._DETERMINISTIC
result = {"grads": {}, "step": {}}
for name, precision, wf, blur, B, H in (("fp32_w100", "fp32", 1.0, False, 3, 129), ("fp32_w050", "fp32", 0.5, False, 3, 129), ("fp32_blur", "fp32", 1.0, True, 2, 65),
                                        ("bc_w100", "bf16-compute", 1.0, False, 3, 129), ("bc_blur", "bf16-compute", 1.0, True, 2, 65)):
    net = make_backbone(wf, blur, precision)
    x = torch.randn(B, 1, H, H, generator=torch.Generator().manual_seed(7)).cuda()
    G = torch.randn(B, net.num_features, generator=torch.Generator().manual_seed(8)).cuda()
    start = copy.deepcopy(net.state_dict())
    outs = {}
    for seq in ("python", "native"):
        net.load_state_dict(start)
        outs[seq] = one_pass(net.set_sequence(seq), x, G)
    bad = [k for k in outs["python"] if not torch.equal(outs["python"][k], outs["native"][k])]
    result["grads"][name] = bad

S = train_script()
_, meta = load_golden("model_default.npz")
meta = dict(meta, B=8, split=5)
for seq in ("python", "native"):
    net = build_net(meta, "cuda").train()
    net.convnet.set_sequence(seq)
    crit, _ = S.setup_losses(script_args(meta["flags"]), net)
    opt, _ = S.create_optimizer(net, script_args(meta["flags"], epochs=20))
    batches = make_batches(meta, "cuda")
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        out = train.training_step(net, batches, 150, crit)
        out["loss"].backward()
        opt.step()
        losses.append(float(out["loss"].item()).hex())
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for k, v in net.state_dict().items():
        h.update(v.detach().cpu().numpy().tobytes())
    result["step"][seq] = {"losses": losses, "state": h.hexdigest(), "optimizer": type(opt).__name__}

# the native step eager against captured and replayed (train.GraphedTrainStep runs its first step eagerly, captures, and replays from the second on)
runs = {}
for how in ("eager", "graphed"):
    net = build_net(meta, "cuda").train()
    net.convnet.set_sequence("native")
    crit, _ = S.setup_losses(script_args(meta["flags"]), net)
    opt, _ = S.create_optimizer(net, script_args(meta["flags"], epochs=20))
    batches = make_batches(meta, "cuda")
    g = train.GraphedTrainStep(net, crit, opt) if how == "graphed" else None
    losses = []
    for _ in range(4):
        if g is not None:
            out = g.run(batches, 150)
        else:
            opt.zero_grad(set_to_none=True)
            out = train.training_step(net, batches, 150, crit)
            out["loss"].backward()
            opt.step()
        losses.append(float(out["loss"].item()).hex())
    torch.cuda.synchronize()
    runs[how] = {"losses": losses}
    if g is not None:
        runs[how].update(captures=g.captures, eager_only=g.eager_only, has_graph=g.graph is not None)
result["graph"] = runs
print("RESULT " + json.dumps(result))
