#!/usr/bin/env python3
"""Golden vectors of the face localizer: the reference's own LocalizerNet (neuralnets/models.py:30-93) on torch-CPU.

Build container only (it imports the reference through oracle/tools/ref_shims.py).  The reference builds its blocks from torchvision's
`mnasnet._InvertedResidual`; torchvision is not installed and the shim's placeholder is not an nn.Module, so a real inverted-residual
block (conv 1x1, BN, ReLU, depthwise k x k, BN, ReLU, conv 1x1, BN, the input added when shapes allow) is put into the stub module BEFORE
the reference's `models` is imported.  The network gets a seeded initialisation; every BatchNorm's running statistics are first set from
the inputs (so that activations stay of order one through 14 layers), after its weight and bias were drawn at random, and then perturbed - the
defaults (mean 0, variance 1, weight 1, bias 0) would make BatchNorm a no-op and the test degenerate.

Writes tests/golden/localizer.npz (data only): the key list with shapes and the state dict, three uint8 inputs of 224 x 288, out32, out64,
attention64, the float64 outputs of convnet[1], [2], [8], [14] for the first input - [1] and [2] at the rows / columns
tests/localizer_ref.sample_grid gives, which keeps the file below the largest fixture - and fp32_dev = max |out32 - out64|.
    python tools/gen_golden_localizer.py"""
from __future__ import annotations

import copy
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle", "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

import ref_shims  # noqa: E402

torch = ref_shims.install()
import torch.nn as nn  # noqa: E402

from localizer_ref import ADD, MUL, TAPS, sample_grid  # noqa: E402


class InvertedResidual(nn.Module):
    def __init__(self, in_ch, out_ch, kernel_size, stride, expansion_factor, bn_momentum=0.1):
        super().__init__()
        mid = in_ch * expansion_factor
        self.apply_residual = in_ch == out_ch and stride == 1
        self.layers = nn.Sequential(
            nn.Conv2d(in_ch, mid, 1, bias=False), nn.BatchNorm2d(mid, momentum=bn_momentum), nn.ReLU(inplace=True),
            nn.Conv2d(mid, mid, kernel_size, padding=kernel_size // 2, stride=stride, groups=mid, bias=False),
            nn.BatchNorm2d(mid, momentum=bn_momentum), nn.ReLU(inplace=True),
            nn.Conv2d(mid, out_ch, 1, bias=False), nn.BatchNorm2d(out_ch, momentum=bn_momentum))

    def forward(self, x):
        return self.layers(x) + x if self.apply_residual else self.layers(x)


sys.modules["torchvision.models.mnasnet"]._InvertedResidual = InvertedResidual
import trackertraincode.neuralnets.models as models  # noqa: E402  (the reference's)

SEED = 20240611


def make_inputs(rng):
    """Three frames with structure at several scales: smooth blobs, an edge, noise."""
    yy, xx = np.mgrid[0:224, 0:288].astype(np.float64)
    frames = []
    for i in range(3):
        f = 110 + 60 * np.sin(xx / (9.0 + 5 * i) + i) * np.cos(yy / (7.0 + 3 * i))
        cx, cy, r = rng.uniform(60, 220), rng.uniform(50, 170), rng.uniform(25, 60)
        f += 80 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * r * r))
        f[:, int(rng.uniform(40, 250)):] -= 35
        f += rng.normal(0, 12, f.shape)
        frames.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
    return np.stack(frames)


def main():
    rng = np.random.default_rng(SEED)
    torch.manual_seed(SEED)
    assert models.__file__.startswith(ref_shims.REFERENCE_ROOT), models.__file__
    net = models.LocalizerNet()
    frames = make_inputs(rng)
    x32 = (torch.from_numpy(frames).to(torch.float32) * MUL + ADD)[:, None]
    bns = [m for m in net.modules() if isinstance(m, nn.BatchNorm2d)]
    g = torch.Generator().manual_seed(SEED)
    with torch.no_grad():
        for m in bns:
            n = m.num_features
            m.weight.copy_(torch.empty(n).uniform_(0.6, 1.5, generator=g) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1))
            m.bias.copy_(0.3 * torch.randn(n, generator=g))
    # running statistics from the inputs themselves: one training-mode pass with momentum 1 (the momenta are no part of the state dict)
    saved = [m.momentum for m in bns]
    for m in bns:
        m.momentum = 1.0
    net.train()
    with torch.no_grad():
        net(x32)
    for m, mom in zip(bns, saved):
        m.momentum = mom
    with torch.no_grad():
        for m in bns:
            n = m.num_features
            m.running_mean += 0.2 * torch.sqrt(m.running_var) * torch.randn(n, generator=g)
            m.running_var *= torch.empty(n).uniform_(0.8, 1.25, generator=g)
    net.eval()
    state = net.state_dict()
    with torch.no_grad():
        out32 = net(x32).numpy()
        net64 = copy.deepcopy(net).double()
        x64 = x32.double()
        out64 = net64(x64).numpy()
        attention64 = net64.attentionmap.numpy()
        taps, z = {}, x64[:1]
        for i, layer in enumerate(net64.convnet):
            z = layer(z)
            if i in TAPS:
                taps[i] = z[0].numpy()
    for i in (1, 2):  # the two large ones: at sample_grid's rows and columns
        t = taps[i]
        taps[i] = t[np.ix_(np.arange(t.shape[0]), sample_grid(t.shape[1]), sample_grid(t.shape[2]))]
    fp32_dev = float(np.abs(out32.astype(np.float64) - out64).max())
    keys = list(state.keys())
    meta = {"keys": keys, "shapes": [list(state[k].shape) for k in keys], "seed": SEED, "mul": MUL, "add": ADD}
    arrays = {"meta": np.array(json.dumps(meta)), "frames": frames, "out32": out32, "out64": out64, "attention64": attention64,
              "fp32_dev": np.array(fp32_dev)}
    arrays.update({f"tap{i}": v for i, v in taps.items()})
    arrays.update({"sd/" + k: v.numpy() for k, v in state.items()})
    path = os.path.join(REPO, "tests", "golden", "localizer.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size <= 820 * 1024, size
    print(path, size, "bytes; fp32_dev", fp32_dev)
    print("out64", out64)
    print("attention max", attention64.reshape(3, -1).max(1), "min", attention64.reshape(3, -1).min(1))


if __name__ == "__main__":
    main()
