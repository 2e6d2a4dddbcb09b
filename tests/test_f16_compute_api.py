"""The fp16 compute mode's surface without a GPU: the C ABI additions are declared and exported, and `compute_precision` is plumbed
and validated through the modules without touching state_dict keys (tests/test_gpu_f16_compute.py covers the arithmetic)."""
import os
import re
from argparse import Namespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = dict(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=100, move_metrics_to_cpu=False)
NEW_SYMBOLS = ("rnnt_hip_lstm_fwd_ex", "rnnt_hip_lstm_bwd_ex", "rnnt_hip_lstm_takes_f16")


def test_header_declares_and_library_exports_the_precision_entries():
    from rnntransducer_amd import _lib
    header = open(os.path.join(ROOT, "include", "rnnt_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SYMBOLS, name
        assert getattr(_lib.lib(), name) is not None
    defines = dict(re.findall(r"#define\s+(RNNT_\w+)\s+(\w+)", header))
    assert defines["RNNT_GEMM_HP_F16"] == "32u" and _lib.GEMM_HP_F16 == 32
    assert (defines["RNNT_PRECISION_FP32"], defines["RNNT_PRECISION_F16"]) == ("0", "1")
    assert (_lib.PRECISION_FP32, _lib.PRECISION_F16) == (0, 1)
    # the new flag bit is not one of the existing RNNT_GEMM_* bits
    others = [int(v.rstrip("u")) for k, v in defines.items() if k.startswith("RNNT_GEMM_") and k != "RNNT_GEMM_HP_F16"]
    assert all(o & 32 == 0 for o in others)


def test_takes_f16_answers_without_a_device():
    """A sizing-style query (assumes the MI355X's 256 CUs without a device): config-2 layers take the one-product forms, lstm.hip's v3 /
    v4 shapes (H = 1024) and the ReLU cell do not; shapes outside the library's range answer 0."""
    from rnntransducer_amd import _lib
    L = _lib.lib()
    assert L.rnnt_hip_lstm_takes_f16(1000, 32, 80, 512, 2, 0) == 1
    assert L.rnnt_hip_lstm_takes_f16(1000, 16, 1024, 1024, 2, 1) == 0
    assert L.rnnt_hip_lstm_takes_f16(1000, 32, 80, 512, 2, 3) == 0
    assert L.rnnt_hip_lstm_takes_f16(0, 32, 80, 512, 2, 0) == 0


def _model(compute_precision="fp32", **kw):
    from rnntransducer_amd import RNNTransducer
    torch.manual_seed(0)
    tn = dict(input_size=80, hidden_size=128, output_size=64, num_layers=2, dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=30, hidden_size=64, output_size=64, num_layers=1, dropout=0.0, rnn_type="gru")
    args = Namespace(**ARGS, **({} if compute_precision is None else {"compute_precision": compute_precision}), **kw)
    return RNNTransducer(pn, tn, dict(num_classes=30), args)


def _stacks(model):
    from rnntransducer_amd.networks.rnn import HipLSTM
    return [m for m in model.modules() if isinstance(m, HipLSTM)]


def test_compute_precision_plumbing_on_a_cpu_module():
    m = _model(None)                       # no compute_precision in args: fp32
    assert [s.compute_precision for s in _stacks(m)] == ["fp32", "fp32"]
    m16 = _model("fp16", precision=16)     # args.precision (the reference's --precision 16) does not select anything by itself
    assert [s.compute_precision for s in _stacks(m16)] == ["fp16", "fp16"]
    assert _model(None, precision=16).jointnet.encoder.rnn.compute_precision == "fp32"
    j = m.jointnet
    assert j.set_compute_precision("fp16") is j
    assert [s.compute_precision for s in _stacks(m)] == ["fp16", "fp16"]
    assert j.encoder.set_compute_precision("fp32") is j.encoder
    assert (j.encoder.rnn.compute_precision, j.decoder.rnn.compute_precision) == ("fp32", "fp16")
    assert j.decoder.set_compute_precision("fp32") is j.decoder
    assert j.decoder.rnn.compute_precision == "fp32"
    # what a stack really runs: fp32 while asked for fp32; c2-sized batches of the encoder in fp16 mode take the one-product forms
    assert j.encoder.rnn.effective_precision(1000, 32) == "fp32"
    j.encoder.rnn.compute_precision = "fp16"
    assert j.encoder.rnn.effective_precision(1000, 32) == "fp16"
    assert j.encoder.rnn.effective_precision(4, 2) == "fp32"   # 8 frames: below the half-pair products' limits


@pytest.mark.parametrize("bad", ["fp64", "bf16", "FP16", 16])
def test_invalid_compute_precision_raises_value_error(bad):
    from rnntransducer_amd.networks.rnn import HipLSTM
    with pytest.raises(ValueError):
        _model(bad)
    hip = HipLSTM(8, 16, 1)
    with pytest.raises(ValueError):
        hip.compute_precision = bad
    assert hip.compute_precision == "fp32"
    m = _model("fp32")
    with pytest.raises(ValueError):
        m.jointnet.set_compute_precision(bad)


def test_state_dict_keys_and_values_are_the_same_in_both_modes():
    a, b = _model("fp32"), _model("fp16")
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert not any("precision" in k for k in sa)
