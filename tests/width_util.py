"""Helpers of the width-scaled backbone tests (tests/test_width_host.py, tests/test_width_gpu.py): the scaled block table, the oracle with
its table swapped (oracle.refmodel reads MOBILENET_BLOCKS at call time and then reproduces the reference's MobileNet(widen_factor=w) bit for
bit; tests/test_width_host.py pins that against the reference's fixtures), and state recipes whose shapes come from the product's own
state_dict (R.state_shapes hard-codes width 1.0)."""
from oracle import refmodel as R
from oracle.synth import make_state

WIDTHS = [0.25, 0.5, 0.75, 1.5]
FIXTURES = {0.5: "model_w050.npz", 0.75: "model_w075.npz"}  # tools/gen_golden_width.py: the reference's NetworkWithPointHead at these widths
_BASE = list(R.MOBILENET_BLOCKS)


def scaled_channels(w, c=32):
    return int(c * w)  # the reference's truncation (backbones/mobilenet_v1.py:113-146)


def scaled_blocks(w):
    return [(name, int(cin * w), int(cout * w), stride) for name, cin, cout, stride in _BASE]


def oracle_width(monkeypatch, w):
    monkeypatch.setattr(R, "MOBILENET_BLOCKS", scaled_blocks(w))


def backbone_state(w, seed=0, blur=False):
    """make_state over the `convnet.`-prefixed shapes of MobileNet(widen_factor=w).state_dict()."""
    from trackertraincode.backbones.mobilenet_v1 import MobileNet

    net = MobileNet(num_classes=None, widen_factor=w, use_blurpool=blur)
    shapes = {"convnet." + k: tuple(v.shape) for k, v in net.state_dict().items()}
    return make_state(shapes, seed), shapes
