"""CPU-side checks of the CTC branch (csrc/ctc.hip, JointNet(aux_ctc=True)): the C ABI's argument validation, which happens
on the host before any launch (the pointers below are stand-ins that are never dereferenced), the rule that a model without the
head is exactly the model of before, and the checkpoint rules.  No device work."""
from argparse import Namespace

import pytest
import torch

P, Q, R = 0x10000, 0x20000, 0x30000   # stand-ins for device pointers

ENTRIES = ("rnnt_hip_ctc_loss_workspace_bytes", "rnnt_hip_ctc_loss_fwd", "rnnt_hip_ctc_loss_bwd", "rnnt_hip_ctc_greedy")


def _args(**kw):
    a = dict(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=10)
    a.update(kw)
    return Namespace(**a)


CFG = (dict(embedding_size=10, hidden_size=8, output_size=8, num_layers=2), dict(input_size=12, hidden_size=8, output_size=12, num_layers=2))
HEAD_KEYS = {"jointnet.ctc_head.weight", "jointnet.ctc_head.bias"}


def _model(aux, seed=0, **args):
    from rnntransducer_amd import RNNTransducer
    torch.manual_seed(seed)
    jp = dict(num_classes=10, aux_ctc=True) if aux else dict(num_classes=10)
    return RNNTransducer(*CFG, jp, _args(**args))


def test_entries_are_declared_and_exported():
    import os
    from rnntransducer_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rnnt_hip.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and name + "(" in header and hasattr(L, name)
    assert L.rnnt_hip_version() == 4


def test_workspace_query():
    from rnntransducer_amd import _lib
    L = _lib.lib()
    assert L.rnnt_hip_ctc_loss_workspace_bytes(0, 1, 1, 2) == 0
    assert L.rnnt_hip_ctc_loss_workspace_bytes(1, 0, 1, 2) == 0 and L.rnnt_hip_ctc_loss_workspace_bytes(1, 1, 1, 0) == 0
    assert L.rnnt_hip_ctc_loss_workspace_bytes(1, 1, -1, 2) == 0
    assert L.rnnt_hip_ctc_loss_workspace_bytes(2, 10, 3, 5) > 0
    assert L.rnnt_hip_ctc_loss_workspace_bytes(2, 10, 0, 5) > 0        # no labels at all: the all-blank lattice
    assert L.rnnt_hip_ctc_loss_workspace_bytes(2, 10, 4, 5) > L.rnnt_hip_ctc_loss_workspace_bytes(2, 10, 3, 5)


def test_arguments_are_refused_before_any_launch():
    from rnntransducer_amd import _lib
    L = _lib.lib()
    B, T, U, V = 2, 10, 3, 5
    need = L.rnnt_hip_ctc_loss_workspace_bytes(B, T, U, V)

    def fwd(logits=P, labels=Q, t_lens=Q, u_lens=Q, U=U, V=V, blank=0, nll=R, ws=R, nws=need, z_sb=T * V, z_st=V, T=T):
        return L.rnnt_hip_ctc_loss_fwd(logits, z_sb, z_st, labels, t_lens, u_lens, B, T, U, V, blank, nll, ws, nws, None)

    def bwd(logits=P, labels=Q, t_lens=Q, u_lens=Q, U=U, V=V, blank=0, gvec=Q, stride=1, dz=R, ws=R, nws=need):
        return L.rnnt_hip_ctc_loss_bwd(logits, T * V, V, labels, t_lens, u_lens, B, T, U, V, blank, 1.0, gvec, stride, dz, ws, nws, None)

    def greedy(logits=P, t_lens=Q, V=V, blank=0, tokens=R, counts=R, T=T):
        return L.rnnt_hip_ctc_greedy(logits, T * V, V, t_lens, B, T, V, blank, tokens, counts, None, None)

    err = L.rnnt_hip_last_error
    for call in (fwd, bwd):
        assert call(logits=None) == -1 and b"null" in err()
        assert call(labels=None) == -1 and b"null" in err()
        assert call(t_lens=None) == -1 and call(u_lens=None) == -1
        assert call(ws=None) == -1 and b"workspace" in err()
        assert call(blank=-1) == -1 and b"blank" in err()
        assert call(blank=V) == -1 and b"blank" in err()
        assert call(U=512, nws=1 << 40) == -1 and b"511" in err()
        assert call(nws=need - 1) == -1 and b"workspace too small" in err()
    assert fwd(nll=None) == -1 and b"null" in err()
    assert fwd(z_st=V - 1) == -1 and b"stride" in err()
    assert fwd(T=1 << 20, U=511, nws=1 << 50) == -1 and b"buffer resource" in err()
    assert bwd(dz=None) == -1 and b"null" in err()
    for stride in (-1, 2):
        assert bwd(stride=stride) == -1 and b"gvec_stride" in err()
    assert greedy(logits=None) == -1 and greedy(t_lens=None) == -1 and greedy(tokens=None) == -1 and greedy(counts=None) == -1
    assert b"null" in err()
    assert greedy(blank=V) == -1 and b"blank" in err()
    assert greedy(T=0) == -1 and greedy(V=0) == -1


def test_default_model_is_unchanged_and_the_head_comes_last():
    """Without aux_ctc the state_dict keys are those of the model before the feature (the reference's: SURVEY.md §8b); under one
    seed every tensor equals that of a model with the head, which has exactly two more keys."""
    from rnntransducer_amd import JointNet
    plain, aux = _model(False), _model(True)
    sd, sda = plain.state_dict(), aux.state_dict()
    names = {f"{n}_l{l}{r}" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh") for l in (0, 1) for r in ("", "_reverse")}
    today = ({"jointnet.encoder.rnn." + n for n in names} | {"jointnet.decoder.rnn." + n for n in names if "reverse" not in n}
             | {"jointnet.encoder.out_proj.weight", "jointnet.encoder.out_proj.bias", "jointnet.decoder.embedding.weight",
                "jointnet.decoder.out_proj.weight", "jointnet.decoder.out_proj.bias", "jointnet.fc.weight", "jointnet.fc.bias"})
    assert set(sd) == today
    assert set(sda) - set(sd) == HEAD_KEYS and set(sd) <= set(sda)
    for k, v in sd.items():
        assert torch.equal(v, sda[k]), k
    assert sda["jointnet.ctc_head.weight"].shape == (10, 12) and sda["jointnet.ctc_head.bias"].shape == (10,)
    assert not plain.jointnet.aux_ctc and aux.jointnet.aux_ctc and not hasattr(plain.jointnet, "ctc_head")
    torch.manual_seed(3)
    a = JointNet(dict(CFG[1]), dict(CFG[0], pad_token_id=0), 10)
    torch.manual_seed(3)
    b = JointNet(dict(CFG[1]), dict(CFG[0], pad_token_id=0), 10, aux_ctc=True)
    assert set(b.state_dict()) - set(a.state_dict()) == {"ctc_head.weight", "ctc_head.bias"}
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())


def test_misuse_raises():
    from rnntransducer_amd import CTCLoss, JointNet
    from rnntransducer_amd._lib import RnntHipError
    with pytest.raises(ValueError):
        _model(False, ctc_weight=0.3)
    assert _model(True, ctc_weight=0.3).ctc_weight == pytest.approx(0.3) and _model(True).ctc_weight == 0.0
    with pytest.raises(ValueError):
        CTCLoss(reduction="avg")
    z, y = torch.zeros(2, 5, 10), torch.ones(2, 2, dtype=torch.int32)
    tl, ul = torch.tensor([5, 4], dtype=torch.int32), torch.tensor([2, 1], dtype=torch.int32)
    with pytest.raises(RnntHipError):                                    # no CPU / eager fallback
        CTCLoss()(z, y, tl, ul)
    from rnntransducer_amd.ops import ctc_greedy
    with pytest.raises(RnntHipError):
        ctc_greedy(z, tl, 0)
    net = JointNet(dict(CFG[1]), dict(CFG[0], pad_token_id=0), 10).eval()
    x, txt = torch.zeros(2, 5, 12), torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(ValueError):
        net.loss(x, tl, txt, y, ul, 0, ctc_weight=0.3)
    with pytest.raises(ValueError):
        net.loss(x, tl, txt, y, ul, 0, return_parts=True)
    with pytest.raises(ValueError):
        net.ctc_loss(x, tl, y, ul, 0)
    with pytest.raises(ValueError):
        net.recognize_ctc_greedy(x, tl, 0)
    with pytest.raises(ValueError):
        _model(False).recognize_ctc_greedy(x, tl)


def test_checkpoint_rules(tmp_path):
    from rnntransducer_amd import RNNTransducer
    plain, aux = _model(False, seed=1), _model(True, seed=2, ctc_weight=0.3)
    ref = {k: torch.randn_like(v) for k, v in plain.state_dict().items()}
    path = tmp_path / "ref.ckpt"
    torch.save({"epoch": 1, "global_step": 5, "pytorch-lightning_version": "1.8.0", "state_dict": ref,
                "hyper_parameters": {"prednet_params": CFG[0], "transnet_params": CFG[1], "jointnet_params": dict(num_classes=10),
                                     "args": _args()}}, path)
    # a reference-style file into a model with the head: exactly the two head keys may be missing, the head keeps its values
    head = {k: aux.state_dict()[k].clone() for k in HEAD_KEYS}
    aux.load_reference_checkpoint(str(path))
    for k, v in aux.state_dict().items():
        assert torch.equal(v, head[k] if k in HEAD_KEYS else ref[k]), k
    short = dict(ref)
    del short["jointnet.fc.bias"]
    torch.save({"state_dict": short}, tmp_path / "short.ckpt")
    with pytest.raises(RuntimeError):
        aux.load_reference_checkpoint(str(tmp_path / "short.ckpt"))
    torch.save({"state_dict": dict(ref, **{"jointnet.extra": torch.zeros(1)})}, tmp_path / "extra.ckpt")
    with pytest.raises(RuntimeError):
        aux.load_reference_checkpoint(str(tmp_path / "extra.ckpt"))
    # include_aux=False (the default): no head tensors, no aux_ctc entry; loads strictly into a model without the head
    out = tmp_path / "noaux.ckpt"
    aux.save_reference_checkpoint(str(out), epoch=2, global_step=9)
    blob = RNNTransducer.read_reference_checkpoint(str(out))
    assert set(blob["state_dict"]) == set(ref) and "aux_ctc" not in blob["hyper_parameters"]["jointnet_params"]
    plain.load_reference_checkpoint(str(out), strict=True)
    assert all(torch.equal(v, ref[k]) for k, v in plain.state_dict().items())
    m = RNNTransducer.from_reference_checkpoint(str(out))
    assert not m.jointnet.aux_ctc and all(torch.equal(v, ref[k]) for k, v in m.state_dict().items())
    # include_aux=True keeps both and round-trips the head
    out2 = tmp_path / "aux.ckpt"
    aux.save_reference_checkpoint(str(out2), include_aux=True)
    blob2 = RNNTransducer.read_reference_checkpoint(str(out2))
    assert set(blob2["state_dict"]) == set(ref) | HEAD_KEYS and blob2["hyper_parameters"]["jointnet_params"]["aux_ctc"] is True
    m2 = RNNTransducer.from_reference_checkpoint(str(out2))
    assert m2.jointnet.aux_ctc and m2.ctc_weight == pytest.approx(0.3)
    assert all(torch.equal(v, aux.state_dict()[k]) for k, v in m2.state_dict().items())
    with pytest.raises(RuntimeError):                                    # a model without the head refuses the head's tensors
        plain.load_reference_checkpoint(str(out2))
