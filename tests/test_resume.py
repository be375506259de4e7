"""Run state on the CPU: every random stream of the data path, the scheduler and the two callbacks survive a state round trip, the state file is
replaced atomically, and the training script refuses a resume with arguments that change what the run computes (train.save_run_state /
load_run_state / RunState, the loaders' and callbacks' state_dict(), scripts/train_poseestimator.py --resume)."""
import copy
import io
import os

import numpy as np
import pytest
import torch

from util import train_script


def _through_file(state):
    """The state as a run-state file hands it back: torch.save -> torch.load(weights_only=True)."""
    buf = io.BytesIO()
    torch.save(state, buf)
    buf.seek(0)
    return torch.load(buf, map_location="cpu", weights_only=True)


def _same_batches(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        xs, ys = (x if isinstance(x, list) else [x]), (y if isinstance(y, list) else [y])
        assert [s.meta.tag for s in xs] == [s.meta.tag for s in ys] and [s.meta.batchsize for s in xs] == [s.meta.batchsize for s in ys]
        for s, t in zip(xs, ys):
            assert list(s.keys()) == list(t.keys())
            for k in s.keys():
                assert torch.equal(s[k], t[k]), k


@pytest.mark.parametrize("vary_split", [False, True])
def test_synthetic_loader_state_round_trip(vary_split):
    from trackertraincode.pipelines import SyntheticPoseLoader, Tag

    mix = [(Tag.POSE_WITH_LANDMARKS, 5.0), (Tag.ONLY_POSE, 2.0), (Tag.POSE_WITH_LMKS_NO_SHAPE_PARAMS, 1.0)]
    make = lambda: SyntheticPoseLoader(8, mix, device="cpu", seed=7, inputsize=9, steps_per_epoch=3, vary_split=vary_split)
    a = make()
    first = list(a)
    state = _through_file(a.state_dict())
    second = list(a)
    b = make()
    b.load_state_dict(state)
    _same_batches(list(b), second)
    with pytest.raises(AssertionError):  # (the second epoch is not the first: the comparison above compares something)
        _same_batches(first, second)
    if vary_split:
        assert len({tuple(s.meta.batchsize for s in step) for step in first + second}) > 1
    other = SyntheticPoseLoader(8, mix, device="cpu", seed=7, inputsize=9, steps_per_epoch=3, vary_split=not vary_split)
    with pytest.raises(ValueError, match="built differently"):
        other.load_state_dict(state)


def test_synthetic_test_loader_state_round_trip():
    """The synthetic TEST loader draws new crops at every validation epoch: it has a stream too."""
    from trackertraincode.pipelines import SyntheticPoseLoader, Tag

    make = lambda: SyntheticPoseLoader(4, [(Tag.POSE_WITH_LANDMARKS, 1.0)], device="cpu", seed=4321, inputsize=9, steps_per_epoch=2, single_batch=True)
    a = make()
    list(a)
    state = _through_file(a.state_dict())
    second = list(a)
    b = make()
    b.load_state_dict(state)
    _same_batches(list(b), second)


def test_resident_loader_draws_continue_after_a_state_round_trip():
    from trackertraincode.datasets.resident import ResidentFrames, ResidentLoader

    def frames(n, tag):
        return ResidentFrames(tag, {"image": torch.zeros(n, 1, 4, 4, dtype=torch.uint8), "roi": torch.zeros(n, 4)})

    # 7 frames, about 10 of 16 draws per step: the small set's permutation wraps in every step, also between the saved state and the end
    make = lambda: ResidentLoader([frames(7, "a"), frames(300, "b")], [3.0, 2.0], batchsize=16, steps_per_epoch=3, seed=5)
    a = make()
    before = [a.draw() for _ in range(4)]
    pos_then = list(a._pos)
    state = _through_file(a.state_dict())
    after = [a.draw() for _ in range(6)]
    assert sum(len(idx) for step in after for d, idx in step if d == 0) > 7  # wrapped after the state was taken
    b = make()
    b.load_state_dict(state)
    assert b._pos == pos_then
    resumed = [b.draw() for _ in range(6)]
    for s, t in zip(after, resumed):
        assert [d for d, _ in s] == [d for d, _ in t]
        for (_, i), (_, j) in zip(s, t):
            np.testing.assert_array_equal(i, j)
    fresh = [make().draw()]
    assert not all(np.array_equal(i, j) for (_, i), (_, j) in zip(fresh[0], after[0]))
    # the torch generator of the crop and the intensity parameters travels with it
    u = torch.rand(5, generator=a._gen)
    c = make()
    c.load_state_dict(_through_file(a.state_dict()))
    assert torch.equal(torch.rand(5, generator=a._gen), torch.rand(5, generator=c._gen)) and not torch.equal(u, torch.rand(5, generator=c._gen))
    with pytest.raises(ValueError, match="other datasets"):
        ResidentLoader([frames(8, "a"), frames(300, "b")], [3.0, 2.0], batchsize=16, steps_per_epoch=3, seed=5).load_state_dict(state)


def test_scheduler_state_round_trip():
    import trackertraincode.train as train

    def make():
        lin = torch.nn.Linear(1, 1)
        opt = torch.optim.SGD([{"params": [lin.weight], "lr": 1.0}, {"params": [lin.bias], "lr": 0.1}], lr=1.0)
        return opt, train.ExponentialUpThenSteps(opt, 3, 0.1, [6])

    def run(opt, sch, n):
        out = []
        for _ in range(n):
            out.append([g["lr"] for g in opt.param_groups])
            opt.step()
            sch.step()
        return out

    opt, sch = make()
    straight = run(opt, sch, 10)
    opt, sch = make()
    head = run(opt, sch, 4)
    so, ss = _through_file(opt.state_dict()), _through_file(sch.state_dict())
    opt2, sch2 = make()
    opt2.load_state_dict(so)
    sch2.load_state_dict(ss)
    assert head + run(opt2, sch2, 6) == straight and len({tuple(v) for v in straight}) > 4


def test_callback_state_round_trips(tmp_path):
    import trackertraincode.train as train

    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3, bias=False), torch.nn.BatchNorm2d(4))

    def move(model, i):
        g = torch.Generator().manual_seed(50 + i)
        with torch.no_grad():
            for v in model.state_dict().values():
                v.copy_(torch.randn(v.shape, generator=g) if v.is_floating_point() else torch.tensor(i + 1))

    straight = train.SwaCallback(start_epoch=0)
    straight.on_train_start(m)
    halted = train.SwaCallback(start_epoch=0)
    halted.on_train_start(m)
    for i in range(3):
        move(m, i)
        straight.on_train_epoch_end(i, m)
        halted.on_train_epoch_end(i, m)
    state = _through_file(halted.state_dict())
    assert state["n_averaged"] == 2
    resumed = train.SwaCallback(start_epoch=0)
    with pytest.raises(RuntimeError, match="on_train_start"):
        resumed.load_state_dict(state)
    move(m, 77)  # the live model a resumed run starts from is not the average
    resumed.on_train_start(m)
    resumed.load_state_dict(state)
    for i in range(3, 5):
        move(m, i)
        straight.on_train_epoch_end(i, m)
        resumed.on_train_epoch_end(i, m)
    assert resumed.n_averaged == straight.n_averaged == 4
    for (k, a), (_, b) in zip(straight.swa_model.state_dict().items(), resumed.swa_model.state_dict().items()):
        assert torch.equal(a, b), k

    from trackertraincode.neuralnets.models import NetworkWithPointHead

    m = NetworkWithPointHead(enable_point_head=False, enable_uncertainty=False)  # (save_model stores the constructor arguments)
    cb = train.CheckpointCallback(str(tmp_path / "a"))
    for e, v in enumerate([3.0, 1.5, 2.0]):
        cb.on_validation_end(e, m, v)
    cb2 = train.CheckpointCallback(str(tmp_path / "b"))
    cb2.load_state_dict(_through_file(cb.state_dict()))
    assert (cb2.best_value, cb2.best_epoch, cb2.history) == (1.5, 1, [3.0, 1.5, 2.0])
    cb2.on_validation_end(3, m, 1.7)  # not a new best: nothing but last.ckpt is written
    assert not os.path.exists(cb2.best_model_path) and os.path.exists(cb2.last_model_path) and cb2.best_epoch == 1


def _tiny_run(tmp_path):
    import trackertraincode.train as train

    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    model(torch.randn(4, 3)).sum().backward()
    opt.step()
    sch = train.ExponentialUpThenSteps(opt, 2, 0.1, [3])
    return train, model, opt, sch, str(tmp_path / "train_state.pt")


def test_run_state_file_round_trip(tmp_path):
    train, model, opt, sch, path = _tiny_run(tmp_path)
    cb = train.CheckpointCallback(str(tmp_path))
    cb.best_value, cb.best_epoch, cb.history = 0.25, 0, [0.25]
    train.save_run_state(path, model, opt, sch, next_epoch=1, callbacks=[cb], meta={"args": {"lr": 1e-3}})
    expected_cpu_rng = torch.get_rng_state()
    state = train.load_run_state(path)
    assert state["next_epoch"] == 1 and state["meta"] == {"args": {"lr": 1e-3}} and state["world"] == 1
    for k, v in model.state_dict().items():
        assert torch.equal(state["model"][k], v), k
    assert torch.equal(state["rng"]["cpu"], expected_cpu_rng)
    assert state["callbacks"] == [("CheckpointCallback", {"best_value": 0.25, "best_epoch": 0, "history": [0.25]})]
    assert sorted(os.listdir(tmp_path)) == ["train_state.pt"]  # no temporary file stays behind
    with pytest.raises(ValueError, match="WORLD_SIZE"):
        train.load_run_state(path, rank=0, world=2)


def test_failed_write_leaves_the_previous_state_intact(tmp_path, monkeypatch):
    train, model, opt, sch, path = _tiny_run(tmp_path)
    train.save_run_state(path, model, opt, sch, next_epoch=1)
    before = open(path, "rb").read()
    with torch.no_grad():
        model[0].weight.add_(1.0)
    real_save = torch.save

    def failing_save(obj, f, *a, **kw):
        f.write(b"half a file")  # the temporary file is open and partly written when the write fails
        raise OSError(28, "No space left on device")

    monkeypatch.setattr(torch, "save", failing_save)
    with pytest.raises(OSError, match="No space left"):
        train.save_run_state(path, model, opt, sch, next_epoch=2)
    monkeypatch.setattr(torch, "save", real_save)
    assert open(path, "rb").read() == before and sorted(os.listdir(tmp_path)) == ["train_state.pt"]
    state = train.load_run_state(path)
    assert state["next_epoch"] == 1 and not torch.equal(state["model"]["0.weight"], model[0].weight)
    train.save_run_state(path, model, opt, sch, next_epoch=2)
    assert train.load_run_state(path)["next_epoch"] == 2


def test_per_rank_files_and_world_size(tmp_path):
    train, model, opt, sch, path = _tiny_run(tmp_path)
    replica = copy.deepcopy(model)
    with torch.no_grad():
        replica[1].running_mean.add_(0.5)  # BatchNorm statistics are per replica
    train.save_run_state(path, model, opt, sch, next_epoch=2, rank=0, world=2)
    torch.manual_seed(11)
    train.save_run_state(path, replica, opt, sch, next_epoch=2, rank=1, world=2)
    rng1 = torch.get_rng_state()
    assert sorted(os.listdir(tmp_path)) == ["train_state.pt", "train_state.pt.rank0", "train_state.pt.rank1"]
    s0, s1 = train.load_run_state(path, rank=0, world=2), train.load_run_state(path, rank=1, world=2)
    assert torch.equal(s0["model"]["0.weight"], s1["model"]["0.weight"])
    assert torch.equal(s0["buffers"]["1.running_mean"] + 0.5, s1["buffers"]["1.running_mean"]) and torch.equal(s1["rng"]["cpu"], rng1)
    fresh = copy.deepcopy(model)
    with torch.no_grad():
        for v in fresh.state_dict().values():
            v.zero_()
    fopt = torch.optim.Adam(fresh.parameters(), lr=1e-2)
    fsch = train.ExponentialUpThenSteps(fopt, 2, 0.1, [3])
    # fit() restores before the first step; at epochs == the saved epoch it does nothing else.  Rank 1: the shared part, then its own buffers
    train.fit(fresh, [], None, fopt, fsch, epochs=2, run_state=train.RunState(path, every=0, resume=s1, rank=1, world=2))
    for (k, a), (_, b) in zip(fresh.state_dict().items(), replica.state_dict().items()):
        assert torch.equal(a, b), k
    assert torch.equal(torch.get_rng_state(), rng1) and fsch.last_epoch == sch.last_epoch
    for a, b in zip(fopt.state_dict()["state"].values(), opt.state_dict()["state"].values()):
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"]) and float(a["step"]) == float(b["step"])
    with pytest.raises(ValueError, match="WORLD_SIZE"):
        train.load_run_state(path, rank=0, world=1)
    with pytest.raises(ValueError, match="WORLD_SIZE"):
        train.load_run_state(path, rank=0, world=4)
    train.save_run_state(path, model, opt, sch, next_epoch=3, rank=0, world=2)  # rank 1 died before writing epoch 3
    with pytest.raises(ValueError, match="does not belong"):
        train.load_run_state(path, rank=1, world=2)


def test_fit_start_epoch_and_default_signature():
    """The loop runs range(start_epoch, epochs); the new arguments default to the behaviour so far."""
    import inspect

    import trackertraincode.train as train

    sig = inspect.signature(train.fit)
    assert (sig.parameters["start_epoch"].default, sig.parameters["run_state"].default, sig.parameters["max_consecutive_skips"].default) == (0, None, 10)
    seen = []

    class Cb:
        def on_train_epoch_end(self, epoch, model):
            seen.append(epoch)

    train.fit(torch.nn.Linear(1, 1), [], None, None, epochs=5, callbacks=[Cb()], start_epoch=3)
    assert seen == [3, 4]


def test_resume_argument_check_names_the_flag():
    S = train_script()
    p = S.make_parser()
    saved = S.recorded_args(p.parse_args(["--epochs", "4"]))
    assert "lr" in saved and "epochs" in saved and "batchsize" in saved and "ds" in saved and "precision" in saved and "widen_factor" in saved
    for free in ("outdir", "sequence", "graph_steps", "graph_layout", "stop_after_epoch", "save_state_every", "resume"):
        assert free not in saved
    S.check_resume_args(saved, S.recorded_args(p.parse_args(["--epochs", "4"])))
    S.check_resume_args(saved, S.recorded_args(p.parse_args(["--epochs", "4", "--sequence", "native", "--outdir", "/elsewhere", "--resume", "auto",
                                                             "--stop-after-epoch", "3", "--save-state-every", "2", "--graph-steps", "--graph-layout", "flat"])))
    with pytest.raises(ValueError, match=r"--lr is 0\.002 here.*0\.001"):
        S.check_resume_args(saved, S.recorded_args(p.parse_args(["--epochs", "4", "--lr", "2e-3"])))
    with pytest.raises(ValueError, match="--epochs"):
        S.check_resume_args(saved, S.recorded_args(p.parse_args(["--epochs", "5"])))
    with pytest.raises(ValueError, match="--with-swa"):
        S.check_resume_args(saved, S.recorded_args(p.parse_args(["--epochs", "4", "--with-swa"])))
    with pytest.raises(ValueError, match="--skip-nonfinite"):
        S.check_resume_args(saved, S.recorded_args(p.parse_args(["--epochs", "4", "--skip-nonfinite"])))
    # what the file hands back compares equal to what was recorded
    S.check_resume_args(_through_file({"args": saved})["args"], saved)
    d = p.parse_args([])  # all four flags are off by default
    assert (d.save_state_every, d.resume, d.stop_after_epoch, d.skip_nonfinite) == (0, None, None, False)
