"""A run stopped after an epoch and resumed from its run state is bitwise the uninterrupted run (train.fit(run_state=...), TTK_DETERMINISTIC=1), and
the non-finite guard end to end.  The runs happen in ONE worker process (tests/_resume_worker.py: the deterministic mode is read at import), started
once for all tests of this file; every comparison is bitwise, so there is no tolerance to choose."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from util import REPO

pytestmark = pytest.mark.gpu
CONFIGS = ["default", "full", "bf16-compute", "shards-device", "shards-host"]


@pytest.fixture(scope="module")
def worker(tmp_path_factory):
    work = tmp_path_factory.mktemp("resume")
    env = dict(os.environ, TTK_DETERMINISTIC="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(REPO, "tests", "_resume_worker.py"), REPO, str(work), *CONFIGS, "guard"], env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    print(json.dumps({k: {n: v for n, v in r.items() if n != "error"} for k, r in res.items()}))
    return res


@pytest.mark.parametrize("cfg", CONFIGS)
def test_resumed_run_is_bitwise_the_uninterrupted_one(worker, cfg):
    r = worker[cfg]
    assert "error" not in r, r["error"]
    print(cfg, r)
    assert r["tensors"] > 400  # parameters, buffers, two moments and a step count per parameter, the SWA average, best.ckpt
    assert r["differing"] == []
    assert r["history_a"] == r["history_b"] and len(r["history_a"]) == 4 and all(math.isfinite(v) for v in r["history_a"])
    assert r["swa_averaged"][0] == r["swa_averaged"][1] == (3 if cfg == "full" else 2)
    # 4 epochs x 3 steps, as in the uninterrupted run (0: a parameter none of the configuration's loss terms reaches is never stepped)
    assert max(r["steps"]) == 12.0 and set(r["steps"]) <= {0.0, 12.0}


def test_guard_end_to_end(worker):
    r = worker["guard"]
    assert "error" not in r, r["error"]
    print(r)
    assert r["health"] == {"skipped": 1, "consecutive": 0, "culprit_index": r["health"]["culprit_index"]} and r["health"]["culprit_index"] >= 0
    assert len(r["reports"]) == 1 and "posnet.linear_xy.weight" in r["reports"][0] and "epoch 1" in r["reports"][0]
    assert r["guarded_finite"] and not r["unguarded_finite"]
    assert r["tensors"] > 400 and r["differing"] == []  # weights, buffers and optimiser state of a run over the other 8 steps' updates
    assert "posnet.linear_xy.weight" in r["ten_in_a_row"] and "epoch 3" in r["ten_in_a_row"] and "10" in r["ten_in_a_row"]


def _build(seed, outdir):
    import trackertraincode.pipelines as P
    import trackertraincode.train as train
    from util import script_args, train_script

    S = train_script()
    torch.manual_seed(seed)
    args = script_args(dict(with_pointhead=True, with_nll_loss=False, rampup_nll_losses=False, skip_nonfinite=True), epochs=2)
    net = S.create_net(args).to("cuda")
    crit, test_crit = S.setup_losses(args, net)
    opt, sch = S.create_optimizer(net, args)
    augs = P.make_image_augmentations(torch.Generator().manual_seed(seed))
    tr = P.SyntheticPoseLoader(8, [(P.Tag.POSE_WITH_LANDMARKS, 1.0)], device="cuda", seed=seed, steps_per_epoch=2, image_augmentations=augs)
    te = P.SyntheticPoseLoader(8, [(P.Tag.POSE_WITH_LANDMARKS, 1.0)], device="cuda", seed=seed + 1, steps_per_epoch=1, single_batch=True)
    cbs = [train.CheckpointCallback(outdir), train.SwaCallback(start_epoch=-1)]
    kw = dict(callbacks=cbs, val_loader=te, val_criterions=test_crit)
    return net, tr, te, crit, opt, sch, cbs, kw


def _everything(net, tr, te, opt, sch, cbs):
    out = {"model/" + k: v for k, v in net.state_dict().items()}
    for i, st in enumerate(opt.state_dict()["state"].values()):
        out.update({f"adam{i}/{k}": v for k, v in st.items()})
    out.update({"swa/" + k: v for k, v in cbs[1].swa_model.state_dict().items()})
    for name, loader in (("train", tr), ("val", te)):
        sd = loader.state_dict()
        out.update({f"{name}/gen": sd["gen"], **{f"{name}/aug{i}": a for i, a in enumerate(sd["augs"])}})
    out["rng/cpu"], out["rng/cuda"] = torch.get_rng_state(), torch.cuda.get_rng_state(torch.device("cuda", torch.cuda.current_device()))
    out = {k: v.detach().cpu().clone() for k, v in out.items()}
    plain = dict(lrs=[g["lr"] for g in opt.param_groups], last_epoch=sch.last_epoch, best=(cbs[0].best_value, cbs[0].best_epoch, list(cbs[0].history)),
                 n_averaged=cbs[1].n_averaged, health=opt.health())
    return out, plain


def test_every_restored_tensor_equals_what_was_saved_and_the_run_finishes(tmp_path):
    """Without the deterministic mode: directly after a load everything holds what was saved, and the resumed run goes on to its end."""
    import trackertraincode.train as train

    path = str(tmp_path / "out" / "train_state.pt")
    net, tr, te, crit, opt, sch, cbs, kw = _build(3, str(tmp_path / "out"))
    train.fit(net, tr, crit, opt, sch, epochs=2, run_state=train.RunState(path, every=1, stop_after_epoch=1), **kw)
    torch.cuda.synchronize()
    saved, saved_plain = _everything(net, tr, te, opt, sch, cbs)
    assert saved_plain["n_averaged"] == 1 and saved_plain["last_epoch"] == 1 and len(saved_plain["best"][2]) == 1
    state = train.load_run_state(path)
    net2, tr2, te2, crit2, opt2, sch2, cbs2, kw2 = _build(77, str(tmp_path / "out"))
    # epochs == the saved epoch: fit() restores and has nothing left to run
    train.fit(net2, tr2, crit2, opt2, sch2, epochs=1, run_state=train.RunState(path, every=0, resume=state), **kw2)
    assert opt2._tables is None  # resumed before any step: nothing cached from before the load
    got, got_plain = _everything(net2, tr2, te2, opt2, sch2, cbs2)
    assert list(got) == list(saved) and len(got) > 400
    assert [k for k in got if not torch.equal(got[k], saved[k])] == []
    assert got_plain == saved_plain
    with pytest.raises(ValueError, match="start_epoch"):
        train.fit(net2, tr2, crit2, opt2, sch2, epochs=2, start_epoch=2, run_state=train.RunState(path, every=0, resume=state), **kw2)
    train.fit(net2, tr2, crit2, opt2, sch2, epochs=2, run_state=train.RunState(path, every=1, resume=state), **kw2)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in net2.parameters()) and len(cbs2[0].history) == 2 and cbs2[1].n_averaged == 2
    assert float(next(iter(opt2.state.values()))["step"]) == 4.0 and train.load_run_state(path)["next_epoch"] == 2
