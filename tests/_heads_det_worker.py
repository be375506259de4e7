"""Worker of tests/test_heads_rows_gpu.py::test_deterministic_mode_weight_gradients_repeat: started with TTK_DETERMINISTIC=1 (the library
reads it once when it loads).  ttk_heads_bwd at B = 300 (five 64-sample chunks in the default mode, one here), F = 260 and 1024: the
reductions within their float64 bounds, and dW / db - like everything else - bitwise equal across two runs."""
import os
import sys

repo = sys.argv[1]
for p_ in (repo, os.path.join(repo, "neuralnet-tracker-traincode_amd"), os.path.join(repo, "tests")):
    sys.path.insert(0, p_)

import torch  # noqa: E402

from head_loss_cases import HeadsProblem  # noqa: E402
from util import gpu_section  # noqa: E402

assert os.environ.get("TTK_DETERMINISTIC") == "1"
with gpu_section():
    for F in (260, 1024):
        p = HeadsProblem((1, 1, 0, 1), 300, F, seed=F)
        fwd = p.forward()
        b1, b2 = p.backward(fwd.get("z")), p.backward(fwd.get("z"))
        torch.cuda.synchronize()
        for o in (fwd, b1, b2):
            o.check(f"F={F}")
        p.check_linear(fwd.np("z", 300, p.NZ))
        p.check_reductions(b1)
        for k in b1.bufs:
            assert torch.equal(b1.get(k), b2.get(k)), f"F={F}: {k} differs between two runs in deterministic mode"
print("RESULT ok")
