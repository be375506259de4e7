"""Worker of tests/test_resume_gpu.py (its own process: TTK_DETERMINISTIC is read when the package is imported).

Per configuration: run A = four epochs straight (B = 8, 3 steps per epoch, learning-rate schedule over 4 epochs, a validation epoch after
each); run B = two epochs, the run state saved, EVERY object rebuilt from scratch with other seeds (network, optimiser, scheduler, callbacks,
loaders, global generators), the state loaded, two more epochs.  Reported: the names of all tensors that differ bitwise between A and B
(parameters, BatchNorm buffers, Adam moments, step counts, the SWA average, best.ckpt) and both validation histories.
"guard": nine steps with one poisoned gradient (step 4), guarded and unguarded, against a run that leaves that optimiser step out; and ten
poisoned steps in a row.

Prints one line "RESULT <json>" with one entry per configuration.
usage: _resume_worker.py <repo> <work dir> <configuration> [<configuration> ...]
"""
import json
import os
import sys
import traceback
import warnings

repo, work = sys.argv[1], sys.argv[2]
for p_ in (repo, repo + "/neuralnet-tracker-traincode_amd", repo + "/tests"):
    sys.path.insert(0, p_)
import torch  # noqa: E402

import landmark_shards as LS  # noqa: E402
from util import gpu_section, script_args, train_script  # noqa: E402
import trackertraincode.backbones.mobilenet_v1 as MB  # noqa: E402
import trackertraincode.pipelines as P  # noqa: E402
import trackertraincode.train as train  # noqa: E402

assert MB._DETERMINISTIC, "run with TTK_DETERMINISTIC=1"
S = train_script()
B, STEPS, EPOCHS, HALF = 8, 3, 4, 2
PLAIN = dict(with_pointhead=True, with_nll_loss=False, rampup_nll_losses=False)
FULL = dict(with_pointhead=True, with_nll_loss=True, rampup_nll_losses=True)
MIX = [(P.Tag.POSE_WITH_LANDMARKS, 5.0), (P.Tag.POSE_WITH_LMKS_NO_SHAPE_PARAMS, 3.0)]
CONFIGS = {
    # flags, precision, graphed, vary_split, shards placement, first epoch that SWA does not average
    "default": (PLAIN, None, False, False, None, 1),          # eager fp32, intensity augmentation, SWA starts at epoch 2
    "full": (FULL, None, "flat", True, None, 0),              # NLL ramp (epoch-dependent weights), one flat graph captured after the load
    "bf16-compute": (PLAIN, "bf16-compute", False, False, None, 1),
    "shards-device": (PLAIN, None, False, False, "device", 1),
    "shards-host": (PLAIN, None, False, False, "host", 1),    # the prefetch thread
}


def build(cfg, outdir, seed_shift, skip_nonfinite=False):
    """Everything a run consists of, from scratch.  `seed_shift` moves every seed: what a resumed run continues with must come out of the
    run state, not out of the constructors."""
    flags, precision, graphed, vary, placement, swa_start = CONFIGS[cfg]
    torch.manual_seed(5 + seed_shift)
    args = script_args(dict(flags, skip_nonfinite=skip_nonfinite), epochs=EPOCHS)
    net = S.create_net(args).to("cuda")
    if precision:
        net.convnet.set_precision(precision)
    crit, test_crit = S.setup_losses(args, net)
    opt, sch = S.create_optimizer(net, args)
    if placement is None:
        augs = P.make_image_augmentations(torch.Generator().manual_seed(100 + seed_shift))
        tr = P.SyntheticPoseLoader(B, MIX, device="cuda", seed=1 + seed_shift, steps_per_epoch=STEPS, image_augmentations=augs, vary_split=vary)
        te = P.SyntheticPoseLoader(B, [(P.Tag.POSE_WITH_LANDMARKS, 1.0)], device="cuda", seed=4321 + seed_shift, steps_per_epoch=1, single_batch=True)
    else:
        P._TEST_SHARD = ("aflw2k", P.Tag.POSE_WITH_LANDMARKS, (0, 8))  # (the generated stand-in has 16 frames)
        tr, te, _ = P.make_pose_estimation_loaders(129, B, [P.Id.REPO_300WLP, P.Id.SYNFACE], datadir=os.path.join(work, "shards"), device="cuda",
                                                   seed=3 + seed_shift, steps_per_epoch=STEPS, frames_on=placement)
        assert all(d.on_host == (placement == "host") for d in tr.datasets)
    cbs = [train.CheckpointCallback(outdir), train.SwaCallback(start_epoch=swa_start)]
    return dict(net=net, crit=crit, test_crit=test_crit, opt=opt, sch=sch, tr=tr, te=te, cbs=cbs, graphed=graphed)


def fit(r, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        train.fit(r["net"], r["tr"], r["crit"], r["opt"], r["sch"], epochs=EPOCHS, callbacks=r["cbs"], val_loader=r["te"], val_criterions=r["test_crit"],
                  graphed=r["graphed"], **kw)
    torch.cuda.synchronize()


def tensors_of(r, outdir):
    out = {"model/" + k: v for k, v in r["net"].state_dict().items()}
    names = [n for n, _ in r["net"].named_parameters()]
    by_param = {id(p): n for n, p in r["net"].named_parameters()}
    for p, st in r["opt"].state.items():
        for k, v in st.items():
            out[f"adam/{by_param[id(p)]}/{k}"] = v
    assert len([k for k in out if k.startswith("adam/") and k.endswith("/step")]) == len(names)
    out.update({"swa/" + k: v for k, v in r["cbs"][1].swa_model.state_dict().items()})
    out.update({"best/" + k: v for k, v in torch.load(os.path.join(outdir, "best.ckpt"), weights_only=True)["state_dict"].items()})
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def differing(a, b):
    assert list(a) == list(b)
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    return [k for k in a if not torch.equal(bits(a[k]), bits(b[k]))]


def run_resume(cfg):
    da, db = os.path.join(work, cfg, "a"), os.path.join(work, cfg, "b")
    a = build(cfg, da, 0)
    fit(a)
    ta, hist_a, swa_a = tensors_of(a, da), list(a["cbs"][0].history), a["cbs"][1].n_averaged
    del a
    torch.cuda.empty_cache()
    path = os.path.join(db, "train_state.pt")
    b1 = build(cfg, db, 0)
    fit(b1, run_state=train.RunState(path, every=0, stop_after_epoch=HALF))
    assert len(b1["cbs"][0].history) == HALF
    del b1
    torch.cuda.empty_cache()
    b2 = build(cfg, db, 1000)
    state = train.load_run_state(path)
    assert state["next_epoch"] == HALF
    fit(b2, run_state=train.RunState(path, every=0, resume=state))
    tb = tensors_of(b2, db)
    steps = sorted({float(v) for k, v in tb.items() if k.startswith("adam/") and k.endswith("/step")})
    return dict(differing=differing(ta, tb), tensors=len(ta), history_a=hist_a, history_b=list(b2["cbs"][0].history), best_epoch=b2["cbs"][0].best_epoch,
                swa_averaged=[swa_a, b2["cbs"][1].n_averaged], steps=steps)


CULPRIT = "posnet.linear_xy.weight"


def guard_run(skip_nonfinite, poisoned, leave_out=None, epochs=3):
    """`epochs` x 3 steps of the default configuration without validation; the gradient of CULPRIT is NaN in the steps `poisoned`; the
    optimiser step `leave_out` is not taken at all (its forward and backward run)."""
    r = build("default", os.path.join(work, "guard"), 0, skip_nonfinite=skip_nonfinite)
    count = {"backward": 0, "step": 0}

    def hook(g):
        k = count["backward"]
        count["backward"] += 1
        return torch.full_like(g, float("nan")) if k in poisoned else g

    dict(r["net"].named_parameters())[CULPRIT].register_hook(hook)
    if leave_out is not None:
        real = r["opt"].step

        def step():
            k = count["step"]
            count["step"] += 1
            return None if k == leave_out else real()

        r["opt"].step = step
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        train.fit(r["net"], r["tr"], r["crit"], r["opt"], r["sch"], epochs=epochs)
    torch.cuda.synchronize()
    assert count["backward"] == 3 * epochs
    state = {k: v.detach().cpu().clone() for k, v in r["net"].state_dict().items()}
    state.update({f"adam{i}/{k}": v.detach().cpu().clone() for i, st in enumerate(r["opt"].state.values()) for k, v in st.items()})
    return state, (r["opt"].health() if skip_nonfinite else None), [str(w.message) for w in caught if "skipped" in str(w.message)]


def run_guard():
    guarded, health, reports = guard_run(True, {4})
    without_step, _, _ = guard_run(False, set(), leave_out=4)
    unguarded, _, _ = guard_run(False, {4})
    finite = lambda st: all(bool(torch.isfinite(v).all()) for v in st.values() if v.is_floating_point())
    out = dict(health=health, reports=reports, guarded_finite=finite(guarded), unguarded_finite=finite(unguarded), differing=differing(guarded, without_step),
               tensors=len(guarded))
    try:
        guard_run(True, set(range(2, 12)), epochs=4)
        out["ten_in_a_row"] = "no error"
    except train.NonFiniteGradientError as e:
        out["ten_in_a_row"] = str(e)
    return out


results = {}
with gpu_section():
    if any(c.startswith("shards") for c in sys.argv[3:]):
        os.makedirs(os.path.join(work, "shards"), exist_ok=True)
        LS.write_training_mix(os.path.join(work, "shards"))
    for cfg in sys.argv[3:]:
        try:
            results[cfg] = run_guard() if cfg == "guard" else run_resume(cfg)
        except Exception:  # noqa: BLE001  (reported to the test of this configuration)
            results[cfg] = dict(error=traceback.format_exc()[-3000:])
            # nothing more is started on the GPU after a failure, whatever its kind: the remaining configurations are reported as not run
            results.update({c: dict(error=f"not run: configuration {cfg!r} failed before it") for c in sys.argv[3:] if c not in results})
            break
print("RESULT " + json.dumps(results))
