"""Host side of the native launch sequence (MobileNet.set_sequence("native"): one C call per direction, include/ttk.h
"The MobileNet backbone as ONE call per direction").  GPU side: tests/test_native_sequence_gpu.py.

The plan's size arithmetic asks the pointwise kernels for their row tilings, which read the device's compute-unit count
(csrc/pwconv_r.hip), so the layout invariants live in the GPU file; what is refused BEFORE any such query is checked here."""
import pytest
import torch

from util import train_script


def _mb():
    import trackertraincode.backbones.mobilenet_v1 as MB

    return MB


def test_set_sequence_accepts_the_two_names_and_rejects_others():
    MB = _mb()
    net = MB.MobileNet(num_classes=0)
    assert net.sequence is None and net.effective_sequence() == "python" and MB.get_sequence() == "python"  # the default stays "python"
    assert net.set_sequence("native") is net and net.effective_sequence() == "native"
    assert net.set_sequence("python").effective_sequence() == "python"
    for bad in ("c", "Native", "", 1, torch.float32):
        with pytest.raises(ValueError, match="sequence"):
            net.set_sequence(bad)
        with pytest.raises(ValueError, match="sequence"):
            MB.set_sequence(bad)
    assert net.effective_sequence() == "python"
    try:  # the module-wide default, shaped like set_activation_dtype: instances without a value of their own follow it
        MB.set_sequence("native")
        other = MB.MobileNet(num_classes=0, widen_factor=0.5)
        assert other.effective_sequence() == "native" and net.effective_sequence() == "python"
        assert net.set_sequence(None).effective_sequence() == "native"
    finally:
        MB.set_sequence("python")
    assert MB.get_sequence() == "python" and net.effective_sequence() == "python"


def test_the_setting_is_neither_in_the_config_nor_in_the_state_dict():
    from trackertraincode.neuralnets.models import NetworkWithPointHead

    net = NetworkWithPointHead(enable_point_head=False, enable_uncertainty=False)
    before, keys = net.get_config(), list(net.state_dict())
    net.convnet.set_sequence("native")
    assert net.get_config() == before and list(net.state_dict()) == keys
    assert "sequence" not in str(before) and not any("sequence" in k for k in keys)
    sd = net.state_dict()
    fresh = NetworkWithPointHead(**before)
    fresh.load_state_dict(sd, strict=True)
    assert fresh.convnet.effective_sequence() == "python"


def test_train_script_flag_parses_and_defaults_to_python():
    S = train_script()
    p = S.make_parser()
    assert p.parse_args([]).sequence == "python"
    assert p.parse_args(["--sequence", "native"]).sequence == "native"
    assert p.parse_args(["--sequence", "python"]).sequence == "python"
    with pytest.raises(SystemExit):
        p.parse_args(["--sequence", "c"])


@pytest.mark.parametrize("module,attr,value", [
    ("mobilenet_v1", "_ELIDE_HEAD_INPUT", True), ("mobilenet_v1", "_ELIDE_HEAD_INPUT", False), ("mobilenet_v1", "_EXP_TENSOR_HOOK", print)])
def test_native_refuses_a_non_product_switch_and_names_it(monkeypatch, module, attr, value):
    MB = _mb()
    import trackertraincode._hip as H
    from trackertraincode.backbones import _mobilenet_bc

    mod = {"mobilenet_v1": MB, "_mobilenet_bc": _mobilenet_bc, "_hip": H}[module]
    net = MB.MobileNet(num_classes=0)
    net.set_sequence("native")  # product values: accepted
    monkeypatch.setattr(mod, attr, value)
    with pytest.raises(ValueError, match=attr):
        MB.MobileNet(num_classes=0).set_sequence("native")
    with pytest.raises(ValueError, match=attr):
        MB.set_sequence("native")
    assert MB.get_sequence() == "python"
    # an instance that was switched before the experiment attribute changed refuses when it is asked to run, not silently
    with pytest.raises(ValueError, match=attr):
        MB._native_forward(torch.zeros(1, 1, 129, 129), [], [], 0.1, 1e-5, "train", None, "fp32", net._blocks)
    MB.MobileNet(num_classes=0).set_sequence("python")  # the Python sequence takes every value


def test_the_settled_switches_are_gone_and_the_one_bench_reads_is_inert():
    """bench.py saves and restores `_USE_WGRAD_STREAM` (an AttributeError otherwise); the removed names must not come back as attributes that
    a tool sets and nobody reads."""
    MB = _mb()
    import trackertraincode._hip as H
    from trackertraincode.backbones import _mobilenet_bc

    assert MB._USE_WGRAD_STREAM is False
    assert not hasattr(H, "BN_PIVOT")
    for mod in (MB, _mobilenet_bc):
        for name in ("_FOLD_WITH_FINALIZE", "_FUSED_PW_BWD", "_DW_WGRAD_ROWS"):
            assert not hasattr(mod, name), (mod.__name__, name)


def test_plan_refuses_bf16_compute_at_another_width_and_bad_tables():
    """ttk_mobilenet_plan_init validates before it sizes anything: these refusals need no device."""
    MB = _mb()
    import trackertraincode._hip as H

    L = H.lib()
    c0, blocks = MB._scaled_blocks(0.5)
    table = tuple((cin, cout, s) for _, cin, cout, s in blocks)
    with pytest.raises(ValueError, match="bf16-compute"):
        L.mobilenet_plan(3, 129, 129, c0, table, (False,) * 13, "train", "bf16-compute", False)
    ref = tuple((cin, cout, s) for _, cin, cout, s in MB._BLOCKS)
    with pytest.raises(ValueError, match=r"cin\[3\]"):  # a table whose channel counts do not chain
        L.mobilenet_plan(3, 129, 129, 32, ref[:3] + ((64, 256, 2),) + ref[4:], (False,) * 13, "train", "fp32", False)
    with pytest.raises(ValueError, match="block 0"):  # a channel count outside every kernel family's domain
        L.mobilenet_plan(3, 129, 129, 32, ((32, 36, 1), (36, 64, 1)), (False,) * 2, "train", "fp32", False)
    with pytest.raises(ValueError, match=r"blur\[0\]"):
        L.mobilenet_plan(3, 129, 129, 32, ref, (True,) + (False,) * 12, "train", "fp32", False)
    with pytest.raises(ValueError, match="32-bit"):
        L.mobilenet_plan(1 << 20, 129, 129, 32, ref, (False,) * 13, "train", "fp32", False)
    with pytest.raises(ValueError, match="blocks"):
        L.mobilenet_plan(3, 129, 129, 32, ref + ref[-1:] * 4, (False,) * 17, "train", "fp32", False)
    assert L.cdll.ttk_mobilenet_plan_bytes() == __import__("ctypes").sizeof(H.MobileNetPlan)  # the ctypes mirror and the header agree
    # a zeroed (refused) plan is refused by every later call
    plan = H.MobileNetPlan()
    assert L.cdll.ttk_mobilenet_forward_workspace_bytes(plan) == 0 and L.cdll.ttk_mobilenet_backward_workspace_bytes(plan) == 0
    assert L.cdll.ttk_mobilenet_describe(plan, 0, None, 0, None) != 0
