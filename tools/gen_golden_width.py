#!/usr/bin/env python3
"""Golden vectors of WIDTH-SCALED pose networks: the reference's own NetworkWithPointHead(backbone_args={"widen_factor": w}) on torch-CPU,
through the machinery of oracle/tools/gen_golden.py (same inputs' recipes, same entries, same file format as tests/golden/model_default.npz:
meta with config / shapes / seeds / flags, per-loss values at epochs 0 / 20 / 150, train and eval predictions, gradient and
running-statistics digests).  No weights are stored: they come from oracle.synth.make_state(shapes of the reference's state_dict, seed).

Build container only (it imports the reference through oracle/tools/ref_shims.py).  Re-run with
    python tools/gen_golden_width.py [w050 w075 w025 w150]
Writes tests/golden/model_w050.npz, model_w075.npz (default) - each well under 1 MB."""
from __future__ import annotations

import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle", "tools"))
sys.path.insert(0, REPO)

import gen_golden as G  # noqa: E402  (installs the reference shims on import)

WIDTHS = {"w025": 0.25, "w050": 0.5, "w075": 0.75, "w150": 1.5}


def config(w):
    """The script's default flags (point head on, NLL off) at width w; widen_factor is not a flag of the reference's script, so `flags`
    carries it under the name this package's --widen-factor uses."""
    return (dict(enable_point_head=True, enable_uncertainty=False, config="mobilenetv1", backbone_args={"widen_factor": w, "use_blurpool": False}),
            dict(with_pointhead=True, with_nll_loss=False, rampup_nll_losses=False, widen_factor=w))


if __name__ == "__main__":
    for name in sys.argv[1:] or ["w050", "w075"]:
        G.CONFIGS[name] = config(WIDTHS[name])
        G.gen_model(name)
        path = os.path.join(G.GOLD, f"model_{name}.npz")
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
        print(path, os.path.getsize(path), "bytes")
