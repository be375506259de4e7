"""scripts/train_poseestimator.py as a program: --save-state-every / --stop-after-epoch / --resume auto.  A run of four epochs stopped after two and
resumed writes bitwise the last.ckpt of the uninterrupted run (TTK_DETERMINISTIC=1 in the children) - on one GPU, and with two ranks sharing the
GPU over gloo (TTK_DRYRUN_SHARE_GPU=1, launched like tests/test_train_script_dp_dryrun_gpu.py), where every rank's parameters and every rank's own
BatchNorm buffers are compared.  The epoch is cut to six steps and the global generators are seeded, in every child alike."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(REPO, "neuralnet-tracker-traincode_amd", "scripts", "train_poseestimator.py")
NET = "NetworkWithPointHead_mobilenetv1"
WRAP = r"""
import sys, os, runpy, hashlib, torch
sys.argv = [sys.argv[1]] + sys.argv[2:]
import trackertraincode.pipelines as P
_orig = P.make_pose_estimation_loaders
def short(*a, **k):  # 6 steps per epoch instead of 10 * 1024 / batchsize
    tr, te, n = _orig(*a, **k)
    tr._steps = 6
    return tr, te, n
P.make_pose_estimation_loaders = short
import trackertraincode.train as T
_fit = T.fit
def digest(tensors):
    h = hashlib.sha256()
    for v in tensors:
        h.update(v.detach().cpu().numpy().tobytes())
    return h.hexdigest()
def fit(model, *a, **k):
    out = _fit(model, *a, **k)
    r = os.environ.get("RANK", "0")
    print(f"RANK {r} PARAMS {digest(model.parameters())}", flush=True)
    print(f"RANK {r} BUFFERS {digest(model.buffers())}", flush=True)
    return out
T.fit = fit
torch.manual_seed(20)  # the script does not seed the global generators (weight initialisation, the augmentation's Gaussian noise): runs compare only from one seed
runpy.run_path(sys.argv[0], run_name="__main__")
"""
FLAGS = ["--ds", "synthetic", "--batchsize", "64", "--epochs", "4"]


def _env():
    env = dict(os.environ, TTK_DETERMINISTIC="1", PYTHONPATH=os.path.join(REPO, "neuralnet-tracker-traincode_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    return env


def _run(cmd, env):
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, "\n".join(l for l in out.stderr.splitlines() if "Error" in l or "error" in l or "File" in l or "raise" in l)[-3000:]
    return {tuple(l.split()[1:3]): l.split()[3] for l in out.stdout.splitlines() if l.startswith("RANK ")}


def _ckpt(outdir, name="last.ckpt"):
    return torch.load(os.path.join(outdir, NET, name), weights_only=True)["state_dict"]


def test_stopped_and_resumed_script_run_writes_the_uninterrupted_checkpoint(tmp_path):
    wrap = tmp_path / "wrap.py"
    wrap.write_text(WRAP)
    base = [sys.executable, str(wrap), SCRIPT, *FLAGS]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    straight = _run(base + ["--outdir", a], _env())
    assert not os.path.exists(os.path.join(a, NET, "train_state.pt"))  # off by default
    _run(base + ["--outdir", b, "--save-state-every", "1", "--stop-after-epoch", "2"], _env())
    import trackertraincode.train as train

    state = train.load_run_state(os.path.join(b, NET, "train_state.pt"))
    assert state["next_epoch"] == 2 and state["meta"]["args"]["lr"] == 1e-3 and "outdir" not in state["meta"]["args"]
    assert len(state["callbacks"][0][1]["history"]) == 2
    resumed = _run(base + ["--outdir", b, "--save-state-every", "1", "--resume", "auto"], _env())
    assert resumed == straight and len(straight) == 2
    sa, sb = _ckpt(a), _ckpt(b)
    assert list(sa) == list(sb) and [k for k in sa if not torch.equal(sa[k], sb[k])] == []
    ba, bb = _ckpt(a, "best.ckpt"), _ckpt(b, "best.ckpt")
    assert [k for k in ba if not torch.equal(ba[k], bb[k])] == []
    assert train.load_run_state(os.path.join(b, NET, "train_state.pt"))["next_epoch"] == 4
    # a resume that changes what the run computes is refused, naming the flag; --resume auto without a state is a fresh start (checked above: run a)
    out = subprocess.run(base + ["--outdir", b, "--resume", "auto", "--lr", "2e-3"], env=_env(), capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "--lr is 0.002 here" in out.stderr


def test_two_ranks_stopped_and_resumed_equal_the_uninterrupted_two_rank_run(tmp_path):
    wrap = tmp_path / "wrap.py"
    wrap.write_text(WRAP)
    env = dict(_env(), HSA_ENABLE_IPC_MODE_LEGACY="0", TTK_DRYRUN_SHARE_GPU="1")

    def launch(port, *flags):
        return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                str(wrap), SCRIPT, *FLAGS, *flags]

    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    straight = _run(launch(29584, "--outdir", a), env)
    _run(launch(29585, "--outdir", b, "--save-state-every", "1", "--stop-after-epoch", "2"), env)
    assert sorted(os.listdir(os.path.join(b, NET)))[-3:] == ["train_state.pt", "train_state.pt.rank0", "train_state.pt.rank1"]
    resumed = _run(launch(29586, "--outdir", b, "--save-state-every", "1", "--resume", "auto"), env)
    assert set(straight) == {("0", "PARAMS"), ("0", "BUFFERS"), ("1", "PARAMS"), ("1", "BUFFERS")}
    assert straight[("0", "PARAMS")] == straight[("1", "PARAMS")]        # every parameter bitwise equal on both ranks
    assert straight[("0", "BUFFERS")] != straight[("1", "BUFFERS")]      # BatchNorm running statistics are per replica
    assert resumed == straight                                            # and both equal the uninterrupted run, rank by rank
    sa, sb = _ckpt(a), _ckpt(b)
    assert [k for k in sa if not torch.equal(sa[k], sb[k])] == []
    import trackertraincode.train as train

    with pytest.raises(ValueError, match="WORLD_SIZE"):
        train.load_run_state(os.path.join(b, NET, "train_state.pt"), rank=0, world=1)
