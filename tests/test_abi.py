"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads and exports every symbol that
include/rnnt_hip.h declares; the python surface mirrors the reference's names; no compute calls here."""
import ctypes
import os
import re
from argparse import Namespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from rnntransducer_amd import _lib
    from rnntransducer_amd.csrc import build
    build.build()
    header = open(os.path.join(ROOT, "include", "rnnt_hip.h")).read()
    declared = set(re.findall(r"\b(rnnt_hip_\w+)\s*\(", header))
    assert declared, "no declarations parsed"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in rnnt_hip.h but not exported"
    assert declared == set(_lib.SYMBOLS), (declared ^ set(_lib.SYMBOLS))
    assert _lib.lib().rnnt_hip_version() == _lib.ABI_VERSION == 4


def test_argument_validation_happens_before_any_device_work():
    from rnntransducer_amd import _lib
    L = _lib.lib()
    assert L.rnnt_hip_gemm_f32(None, None) == -1 and b"null" in L.rnnt_hip_last_error()
    assert L.rnnt_hip_joint_loss_workspace_bytes(0, 1, 1, 1) == 0
    assert L.rnnt_hip_joint_loss_workspace_bytes(2, 10, 3, 5) > 0
    assert L.rnnt_hip_lstm_workspace_bytes(10, 2, 80, 6, 2) == 0       # H % 4 != 0 -> unsupported
    assert L.rnnt_hip_lstm_workspace_bytes(10, 2, 80, 128, 2) > 0
    rc = L.rnnt_hip_loss_from_logits_fwd_bwd(None, None, None, None, 1, 1, 600, 3, 0, 1.0, None, None, None, 0, None)
    assert rc == -1
    # half-pair entry points that take index tables and a C map: refused on the host, with addresses that are never dereferenced
    import ctypes as C
    P, Q = 0x10000, 0x20000                                            # 128-byte aligned stand-ins for device pointers

    def hp_desc(**kw):
        d = _lib.HpGemmDesc()
        d.A, d.a_amax, d.B, d.b_amax, d.C = P, Q, P, Q, Q
        d.M, d.N, d.K, d.c_div, d.c_so, d.c_si = 8, 8, 32, 1, 8, 0
        for k, v in kw.items():
            setattr(d, k, v)
        return C.byref(d)
    assert L.rnnt_hip_gemm_hp_ex(None, None) == -1 and b"null" in L.rnnt_hip_last_error()
    assert L.rnnt_hip_gemm_hp_ex(hp_desc(a_rowidx=P, a_plane_rows=7), None) == -1 and b"row count" in L.rnnt_hip_last_error()
    assert L.rnnt_hip_gemm_hp_ex(hp_desc(a_rowidx=P), None) == -1                      # a_plane_rows left at 0
    assert L.rnnt_hip_gemm_hp_ex(hp_desc(a_plane_rows=8), None) == -1 and b"without a_rowidx" in L.rnnt_hip_last_error()
    assert L.rnnt_hip_gemm_hp_ex(hp_desc(c_div=0), None) == -1 and b"c_div" in L.rnnt_hip_last_error()
    assert L.rnnt_hip_gemm_hp_ex(hp_desc(workspace_bytes=4096), None) == -1 and b"workspace" in L.rnnt_hip_last_error()
    assert L.rnnt_hip_gemm_hp_ex(hp_desc(a_amax=None), None) == -1
    assert L.rnnt_hip_gemm_hp_ex(hp_desc(A=P + 64), None) == -1 and b"aligned" in L.rnnt_hip_last_error()
    assert L.rnnt_hip_gemm_hp_ex(hp_desc(M=0), None) == -1
    plan = _lib.HpGemmPlan()
    assert L.rnnt_hip_gemm_hp_plan(8, 8, 32, 0, None) == -1
    assert L.rnnt_hip_gemm_hp_plan(0, 8, 32, 0, C.byref(plan)) == -1 and L.rnnt_hip_gemm_hp_plan(8, 8, 1 << 31, 0, C.byref(plan)) == -1
    assert L.rnnt_hip_hp_split_ex(P, 8, 32, 32, 0, 0, 0, P, Q, 1, Q, None) == -1       # row-major: the maxima are computed, never given
    assert L.rnnt_hip_hp_split_ex(P, 8, 32, 31, 0, 0, 0, P, Q, 0, Q, None) == -1       # ld < K
    assert L.rnnt_hip_hp_split_ex(P, 8, 32, 7, 1, 40, 0, P, Q, 1, Q, None) == -1       # transposed: ld < rows
    assert L.rnnt_hip_hp_split_ex(P, 8, 32, 8, 1, 0, 0, P, Q, 1, Q, None) == -1        # no source rows
    assert L.rnnt_hip_hp_split_ex(P, 8, 32, 32, 0, 0, 0, P + 64, Q, 0, None, None) == -1
    assert L.rnnt_hip_hp_split_ex(None, 8, 32, 32, 0, 0, 0, P, Q, 0, None, None) == -1
    assert L.rnnt_hip_hp_split_both_ex(P, 8, 32, 31, Q, Q, P, P, Q, None) == -1
    assert L.rnnt_hip_hp_split_both_ex(P, 8, 32, 32, None, Q, P, P, Q, None) == -1
    assert L.rnnt_hip_hp_split_both_ex(P, 8, 32, 32, Q, Q, P, P + 64, None, None) == -1
    assert L.rnnt_hip_hp_colmax(None, 8, 32, 32, Q, None) == -1 and L.rnnt_hip_hp_colmax(P, 8, 32, 32, None, None) == -1
    assert L.rnnt_hip_hp_colmax(P, 8, 32, 31, Q, None) == -1 and L.rnnt_hip_hp_colmax(P, -1, 32, 32, Q, None) == -1


# The loss / alignment entries of csrc/loss.hip: (name, argument names in ABI order).  SEP / DENSE: the operand block they share.
_SEP = ("A", "a_sb", "a_st", "C", "c_sb", "c_su", "bias", "labels", "t_lens", "u_lens", "B", "T", "U1", "V", "blank")
_DENSE = ("logits", "dtype", "labels", "t_lens", "u_lens", "B", "T", "U1", "V", "blank")
_WS = ("workspace", "workspace_bytes", "stream")
_WIN = ("emit_lo", "emit_hi", "win_stride")
_BWD = ("gvec", "gvec_stride", "dA", "dC")
_LOSS_ENTRIES = {
    "joint_loss_fwd_bwd": _SEP + ("gscale", "nll", "dA", "dC") + _WS,
    "joint_loss_fwd_bwd_fastemit": _SEP + ("gscale", "lam", "nll", "dA", "dC") + _WS,
    "joint_loss_fwd_bwd_window": _SEP + ("gscale", "lam") + _WIN + ("nll", "dA", "dC") + _WS,
    "joint_loss_bwd": _SEP + ("gscale",) + _BWD + _WS,
    "joint_loss_bwd_fastemit": _SEP + ("gscale", "lam") + _BWD + _WS,
    "joint_loss_bwd_window": _SEP + ("gscale", "lam") + _BWD + _WS,
    "loss_from_logits_fwd_bwd": tuple(n for n in _DENSE if n != "dtype") + ("gscale", "nll", "grad") + _WS,
    "loss_from_logits_fwd_bwd_ex": _DENSE + ("gscale", "nll", "grad") + _WS,
    "loss_from_logits_fwd_bwd_fastemit": _DENSE + ("gscale", "lam", "nll", "grad") + _WS,
    "loss_from_logits_fwd_bwd_window": _DENSE + ("gscale", "lam") + _WIN + ("nll", "grad") + _WS,
    "joint_align": _SEP + ("frames", "score") + _WS,
    "align_from_logits_ex": _DENSE + ("frames", "score") + _WS,
}


def _loss_refusals(name, fields):
    """(why, overrides) for every argument set `name` must refuse; each changes ONE thing in an otherwise acceptable call."""
    bwd_only, align, windowed = "_bwd" in name and "fwd" not in name, "align" in name, name.endswith("_window")
    required = {"A", "C", "bias", "logits", "labels", "t_lens", "u_lens", "nll", "frames", "score", "workspace"}
    if bwd_only:
        required |= {"dA", "dC"}                     # "given singly" is "one of them missing" there
    if windowed and not bwd_only:
        required |= {"emit_lo", "emit_hi"}
    rows = [(f"null {f}", {f: None}) for f in fields if f in required]
    rows += [(f"{d} = {v}", {d: v}) for d in ("B", "T", "U1", "V") for v in (0, -1)]
    rows += [("blank = -1", {"blank": -1}), ("blank = V", {"blank": 5}), ("U1 = 513", {"U1": 513, "workspace_bytes": 1 << 62})]
    if not bwd_only:                                 # the backward-only entries took any lattice the forward had accepted
        rows += [("T x U1 x 8 = 2^31", {"T": 1 << 20, "U1": 256, "workspace_bytes": 1 << 62}),
                 ("T x U1 x 8 > 2^31", {"T": (1 << 28) + 1, "U1": 1, "labels": None, "frames": None, "workspace_bytes": 1 << 62})]
    rows += [("workspace one byte short", {"workspace_bytes": "short"}), ("no workspace bytes", {"workspace_bytes": 0})]
    if "dA" in fields and not bwd_only:
        rows += [("dA alone", {"dC": None}), ("dC alone", {"dA": None})]
    if bwd_only:
        rows += [("gvec_stride = 2", {"gvec_stride": 2}), ("gvec_stride = -1", {"gvec_stride": -1}), ("V = 1", {"V": 1})]
    if "lam" in fields:
        rows += [(f"lambda = {v}", {"lam": v}) for v in (-0.5, float("inf"), -float("inf"), float("nan"))]
    if "win_stride" in fields:
        rows += [(f"win_stride = {v}", {"win_stride": v}) for v in (1, 0, -3)]          # U = 2
    if "dtype" in fields:
        rows += [(f"dtype code {v}", {"dtype": v}) for v in (7, -1, 3)]
    return [(why, {k: v for k, v in over.items() if k in fields}) for why, over in rows]


def test_loss_entries_refuse_bad_arguments_before_any_device_work():
    """Every loss / alignment entry of csrc/loss.hip against one table of argument sets it must refuse: each returns -1 and leaves
    a message, on the host.  The addresses are stand-ins that are never dereferenced; every call in here is a refused one, so nothing
    reaches a launch.  Then the workspace queries at a grid of shapes, against the byte counts of the layout as it has always been."""
    from rnntransducer_amd import _lib
    L = _lib.lib()
    P = 0x10000
    B, T, U1, V = 2, 4, 3, 5
    good = dict(A=P, a_sb=T * V, a_st=V, C=P, c_sb=U1 * V, c_su=V, bias=P, logits=P, dtype=0, labels=P, t_lens=P, u_lens=P,
                B=B, T=T, U1=U1, V=V, blank=0, gscale=1.0, lam=0.0, emit_lo=P, emit_hi=P, win_stride=U1 - 1, gvec=P, gvec_stride=1,
                nll=P, dA=P, dC=P, grad=P, frames=P, score=P, workspace=P, stream=None)
    calls = 0
    for name, fields in _LOSS_ENTRIES.items():
        entry = getattr(L, "rnnt_hip_" + name)
        query = (L.rnnt_hip_joint_align_workspace_bytes if "align" in name else
                 L.rnnt_hip_joint_loss_window_workspace_bytes if name.endswith("_window") else L.rnnt_hip_joint_loss_workspace_bytes)
        need = query(B, T, U1, V)
        assert need > 0
        for why, over in _loss_refusals(name, fields):
            args = {**good, "workspace_bytes": need, **over}
            if args["workspace_bytes"] == "short":
                args["workspace_bytes"] = need - 1
            rc = entry(*(args[f] for f in fields))
            assert rc == -1, f"{name}: {why}: returned {rc}"
            assert L.rnnt_hip_last_error(), f"{name}: {why}: no message"
            calls += 1
    assert calls > 11 * 20
    # window tables of a wider row stride and of U = 0 are refused for their stride alone (labels may be null at U = 0)
    n0 = L.rnnt_hip_joint_loss_window_workspace_bytes(B, T, 1, V)
    for name in ("joint_loss_fwd_bwd_window", "loss_from_logits_fwd_bwd_window"):
        fields = _LOSS_ENTRIES[name]
        args = dict(good, U1=1, labels=None, win_stride=0, workspace_bytes=n0)
        assert getattr(L, "rnnt_hip_" + name)(*(args[f] for f in fields)) == -1 and L.rnnt_hip_last_error()
    # the queries: plain, windowed, align -- T on both sides of a 32-frame tile and word, U1 on both sides of 64, V = 1
    recorded = _LOSS_WORKSPACE_BYTES
    for (b, t, u1, v), want in recorded.items():
        got = (L.rnnt_hip_joint_loss_workspace_bytes(b, t, u1, v), L.rnnt_hip_joint_loss_window_workspace_bytes(b, t, u1, v),
               L.rnnt_hip_joint_align_workspace_bytes(b, t, u1, v))
        assert got == want, ((b, t, u1, v), got, want)
    for query in (L.rnnt_hip_joint_loss_workspace_bytes, L.rnnt_hip_joint_loss_window_workspace_bytes, L.rnnt_hip_joint_align_workspace_bytes):
        for bad in ((0, 4, 3, 5), (2, 0, 3, 5), (2, 4, 0, 5), (2, 4, 3, 0), (-1, 4, 3, 5)):
            assert query(*bad) == 0


_LOSS_WORKSPACE_BYTES = {   # (B, T, U1, V): (loss, windowed loss, alignment), as the library has always answered
    (1, 1, 1, 1): (1536, 2304, 768),
    (2, 4, 3, 5): (1536, 2304, 768),
    (3, 31, 63, 29): (163584, 165376, 47872),
    (3, 32, 64, 29): (169984, 171776, 49920),
    (3, 33, 65, 29): (200704, 203008, 53504),
    (2, 100, 1, 260): (14336, 15104, 2304),
    (1, 64, 512, 8): (819456, 823808, 266240),
    (5, 97, 130, 3): (1545472, 1551360, 515328),
    (2, 33, 5, 256): (29440, 30208, 3328),
    (4, 2560, 20, 72): (6758656, 6759936, 1664000),
}


def test_gemm_hp_plan_is_the_workspace_query():
    """rnnt_hip_gemm_hp_plan (host only): the split rule at the shapes the GPU tests name, and its agreement with
    rnnt_hip_gemm_hp_workspace_bytes — both read the one function the launch takes its decisions from."""
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import gemm_hp_plan
    L = _lib.lib()
    slab = 70 * 40 * 4
    assert gemm_hp_plan(70, 40, 2061)[:5] == (1, 1, 4, 2, 33)                          # 65 K-tiles: 33 + 32
    assert gemm_hp_plan(70, 40, 4100)[:5] == (1, 1, 4, 4, 33)                          # 129 K-tiles: 33 + 33 + 33 + 30
    assert gemm_hp_plan(70, 40, 4100, 2 * slab)[:5] == (1, 1, 4, 2, 65)
    assert gemm_hp_plan(70, 40, 4100, 2 * slab - 1).splits == 1 and gemm_hp_plan(70, 40, 4100, 0)[:5] == (1, 1, 4, 1, 129)
    assert gemm_hp_plan(1300, 300, 40)[:5] == (6, 2, 4, 1, 2) and gemm_hp_plan(1, 1, 1)[:5] == (1, 1, 4, 1, 1)
    assert gemm_hp_plan(70, 40, 2016).splits == 1 and gemm_hp_plan(49000, 768, 2048).splits == 1   # 63 K-tiles; >= 192 tiles
    assert gemm_hp_plan(5381, 3328, 40).group_m == 8                                   # 22 x 13 tiles
    for M, N, K in [(70, 40, 2061), (70, 40, 4100), (512, 260, 5000), (4096, 1024, 20000), (300, 257, 96), (1, 1, 1 << 20)]:
        p = gemm_hp_plan(M, N, K, 1 << 40)
        want = L.rnnt_hip_gemm_hp_workspace_bytes(M, N, K)
        assert p.workspace_bytes_wanted == want and gemm_hp_plan(M, N, K, 0).workspace_bytes_wanted == want
        assert gemm_hp_plan(M, N, K, want) == p                                        # what the query asks for is enough for the full split
        assert (p.splits > 1) == (want > 0) and p.splits * M * N * 4 <= max(want, M * N * 4)
        nkt = -(-K // 32)
        assert (p.splits - 1) * p.kt_per_split < nkt <= p.splits * p.kt_per_split      # every slab has work, the last takes the rest


def test_module_surface_mirrors_reference_and_fails_loudly_on_cpu():
    from rnntransducer_amd import RNNTransducer
    from rnntransducer_amd._lib import RnntHipError
    args = Namespace(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=10)
    m = RNNTransducer(dict(embedding_size=72, hidden_size=128, output_size=128, num_layers=1),
                      dict(input_size=80, hidden_size=128, output_size=128, num_layers=1), dict(num_classes=72), args)
    keys = set(m.state_dict())
    for k in ("jointnet.encoder.rnn.weight_ih_l0", "jointnet.encoder.rnn.weight_hh_l0_reverse", "jointnet.encoder.out_proj.bias",
              "jointnet.decoder.embedding.weight", "jointnet.decoder.rnn.bias_hh_l0", "jointnet.decoder.out_proj.weight",
              "jointnet.fc.weight", "jointnet.fc.bias"):
        assert k in keys, k
    assert m.jointnet.fc.weight.shape == (72, 256)
    assert torch.all(m.jointnet.decoder.embedding.weight[0] == 0)       # padding_idx row (decoder.py:69)
    with pytest.raises(RnntHipError):                                     # no CPU / eager fallback
        m(torch.zeros(2, 5, 80), [5, 4], torch.zeros(2, 3, dtype=torch.long), [3, 2])
    with pytest.raises(NotImplementedError):
        RNNTransducer(dict(embedding_size=72, hidden_size=128, output_size=128, num_layers=1),
                      dict(input_size=80, hidden_size=128, output_size=128, num_layers=1, rnn_type="transformer"), dict(num_classes=72), args)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "rnntransducer_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp")):
                src = open(os.path.join(dirpath, f)).read()
                hit = re.search(r"^\s*(from|import)\s+oracle|oracle[/.]\w|librnnt_oracle", src, re.M)
                assert hit is None, f"{f} reaches into oracle/: {hit.group(0)!r}"


def test_reference_style_checkpoint_round_trip(tmp_path):
    """f-4: a Lightning .ckpt as the REFERENCE writes it — `state_dict` with its key names plus `hyper_parameters` holding what
    `save_hyperparameters(prednet_params, transnet_params, jointnet_params, args)` stores at model.py:22 (three dicts and an
    argparse.Namespace), epoch / global_step / optimizer_states — loads with a weights-only (no code execution) loader; and
    what save_reference_checkpoint writes round-trips through the same loader and through from_reference_checkpoint
    (inference.py:19-25)."""
    from rnntransducer_amd import RNNTransducer
    args = Namespace(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=10, precision=32,
                     val_on_cpu=False, vocab_path="config/vocab.json", move_metrics_to_cpu=False)
    cfg = (dict(embedding_size=10, hidden_size=8, output_size=8, num_layers=2), dict(input_size=12, hidden_size=8, output_size=8, num_layers=2),
           dict(num_classes=10))
    torch.manual_seed(1)
    ref_like = torch.nn.ModuleDict({"encoder_rnn": torch.nn.LSTM(12, 8, 2, bidirectional=True), "decoder_rnn": torch.nn.LSTM(8, 8, 2)})
    a = RNNTransducer(*cfg, args)
    sd = {k: torch.randn_like(v) for k, v in a.state_dict().items()}
    # torch.nn.LSTM (what the reference instantiates) uses exactly these names/shapes for the recurrent weights
    for k, v in ref_like["encoder_rnn"].state_dict().items():
        assert sd["jointnet.encoder.rnn." + k].shape == v.shape
    for k, v in ref_like["decoder_rnn"].state_dict().items():
        assert sd["jointnet.decoder.rnn." + k].shape == v.shape
    path = tmp_path / "ref.ckpt"
    opt_ref = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(3))])
    torch.save({"epoch": 3, "global_step": 1234, "pytorch-lightning_version": "1.8.0", "state_dict": sd,
                "hyper_parameters": {"prednet_params": cfg[0], "transnet_params": cfg[1], "jointnet_params": cfg[2], "args": args},
                "optimizer_states": [opt_ref.state_dict()], "lr_schedulers": [{"last_epoch": 1234}],
                "callbacks": {}, "loops": {}}, path)
    with pytest.raises(Exception):   # the plain weights-only loader refuses the Namespace: that was round 1's bug
        torch.load(str(path), weights_only=True)
    b = RNNTransducer(*cfg, args)
    b.load_reference_checkpoint(str(path))
    for k, v in b.state_dict().items():
        assert torch.equal(v, sd[k]), k
    blob = RNNTransducer.read_reference_checkpoint(str(path))
    assert blob["hyper_parameters"]["args"].learning_rate == 1e-3 and blob["global_step"] == 1234
    c = RNNTransducer.from_reference_checkpoint(str(path))          # ctor args from hyper_parameters
    assert all(torch.equal(v, sd[k]) for k, v in c.state_dict().items())
    # save side
    out = tmp_path / "ours.ckpt"
    b.save_reference_checkpoint(str(out), epoch=4, global_step=77)
    blob2 = RNNTransducer.read_reference_checkpoint(str(out))
    assert set(blob2["hyper_parameters"]) == {"prednet_params", "transnet_params", "jointnet_params", "args"}
    assert isinstance(blob2["hyper_parameters"]["args"], Namespace) and blob2["epoch"] == 4 and blob2["global_step"] == 77
    assert set(blob2["state_dict"]) == set(sd) and all(torch.equal(blob2["state_dict"][k], sd[k]) for k in sd)
    d = RNNTransducer.from_reference_checkpoint(str(out))
    assert all(torch.equal(v, sd[k]) for k, v in d.state_dict().items())


def test_ragged_plan_lists_the_valid_time_major_rows():
    """ops.RaggedPlan (rnnt_lstm_desc.row_idx): rows t*B + b with t < lens[b], ascending — the frames pack_padded_sequence keeps
    (networks/encoder.py:99), in the same time-major order, built on the host from the collate's python list."""
    import torch
    from torch.nn.utils.rnn import pack_padded_sequence
    from rnntransducer_amd.ops import RaggedPlan
    lens, T = [7, 3, 5, 7, 1], 7
    plan = RaggedPlan(lens, T, "cpu")
    assert plan.n_rows == sum(lens) and not plan.dense and plan.lens.dtype == torch.int32 and plan.row_idx.dtype == torch.int32
    x = torch.arange(T * len(lens), dtype=torch.float32).reshape(T, len(lens), 1)   # value = its own time-major row index
    packed = pack_padded_sequence(x, torch.tensor(lens), enforce_sorted=False)      # rows sorted by length inside every time slab
    assert sorted(packed.data.reshape(-1).to(torch.int32).tolist()) == plan.row_idx.tolist()
    assert plan.row_idx.tolist() == sorted(plan.row_idx.tolist())
    assert RaggedPlan([4, 4], 4, "cpu").dense and RaggedPlan([4, 4], 4, "cpu").row_idx is None
    with pytest.raises(ValueError):
        RaggedPlan([5, 2], 4, "cpu")


def test_lstm_launch_record_entry_points():
    """rnnt_hip_lstm_launch_log_enable / rnnt_hip_lstm_launch_log: host-only state, usable without a device.  enable(1) starts an
    empty record, the query reports the full length and truncates to the buffer it is given; nothing is recorded here (no launch)."""
    import ctypes as C
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import lstm_launch_record
    L = _lib.lib()
    assert L.rnnt_hip_lstm_launch_log_enable(1) == 0
    assert L.rnnt_hip_lstm_launch_log(None, 0) == 0
    buf = C.create_string_buffer(b"x" * 8)
    assert L.rnnt_hip_lstm_launch_log(buf, 8) == 0 and buf.value == b""
    assert L.rnnt_hip_lstm_launch_log_enable(0) == 0
    with lstm_launch_record() as rec:
        pass
    assert rec.symbols == [] and rec.instances == []


def test_gemm_plan_entry_point():
    """rnnt_hip_gemm_plan: host-only, reads the descriptor and the operand addresses' alignment, launches nothing.  The rules it shares
    with the launch (csrc/gemm.hip, make_gemm_plan): 128x128 tiles unless N is a multiple of 256 with >= 64 tiles of 128x256; 256x256
    tiles from 64 (tiles x split-K slabs) on; scalar loads for a stride or an address off 16 bytes; split-K only with a workspace;
    the launch's own argument checks."""
    import ctypes as C
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import gemm_plan
    L = _lib.lib()
    plan = _lib.GemmPlan()
    assert L.rnnt_hip_gemm_plan(None, C.byref(plan)) == -1 and b"null" in L.rnnt_hip_last_error()
    a = torch.zeros(64)
    kw = dict(split_k=False)
    p = gemm_plan(130, 70, 33, a, a, a, a_si=36, b_sn=36, **kw)
    assert (p.mode, p.tile, p.a_kc, p.b_kc, p.vec, p.tiles, p.splits, p.kchunk) == (6, (128, 128), True, True, True, 2, 1, 33)
    assert not gemm_plan(130, 70, 33, a, a, a, **kw).vec                               # row stride 33
    assert not gemm_plan(130, 70, 33, a, a, a, a_si=36, b_sn=36, b_off=7, **kw).vec    # address off 16 bytes
    p = gemm_plan(130, 70, 33, a, a, a, a_mc=True, a_sk=132, b_sn=1, b_sk=72, flags=_lib.GEMM_EXACT_F32, **kw)
    assert (p.mode, p.a_kc, p.b_kc, p.vec) == (0, False, False, True)
    assert gemm_plan(3970, 512, 40, a, a, a, **kw).tile == (128, 256) and gemm_plan(3970, 520, 40, a, a, a, **kw).tile == (128, 128)
    assert gemm_plan(2100, 1800, 40, a, a, a, **kw).tile == (256, 256) and gemm_plan(2100, 1500, 40, a, a, a, **kw).tile == (128, 128)
    p = gemm_plan(515, 515, 1030, a, a, a, split_k=True)
    assert (p.tile, p.tiles, p.splits, p.kchunk) == ((256, 256), 9, 8, 144)
    assert gemm_plan(515, 515, 1030, a, a, a, **kw).splits == 1
    p = gemm_plan(0, 70, 33, a, a, a, **kw)
    assert p.tiles == 0 and p.tile == (0, 0)
    with pytest.raises(ValueError):
        gemm_plan(4, 4, 4, a, a, a, b_sn=2, b_sk=2)
