"""BASELINE.json configs at their FULL lattice / layer sizes on the HIP path.

  * the FUSED joint + RNN-T loss entry (`JointLossFn`: lse_sep / alphabeta / grad_sep kernels — what `training_step`
    runs, networks/transducer.py:58-69 + model.py:56-57) at T=1000/U=40/V=72, T=2000/U=120/V=72, T=1500/U=80/V=2048
    on two utterances, against the float64 C oracle (oracle/rnnt_loss_ref.c) + float64 torch autograd;
  * a full-model step at config-2 layer sizes (4x512 bi-LSTM, 1x512 prediction net, T=1000, U=40) against
    `OracleJointNet(...).double()`: loss and every parameter gradient — at B=2 AND on the launch that bench.py times (B=32: 8 sync
    groups x 32 workgroups), where the 30 other rows get upstream weight 0 so the same 2-utterance oracle applies;
  * the same at config-3 geometry (T=2000, U=120, B=8: the 4-row-group kernels) and at config-5 layer sizes (6x640, V=2048, T=1500:
    at B=2 and on the B=16 launch bench.py times);
  * the reference's shipped config.json (8x1024 bi-GRU encoder, 2x1024 LSTM prediction net, O=512, V=72, T=1000, U=40): every
    parameter gradient at B=2 and on the B=16 launch bench.py times — the v3 / v4 register-form recurrences, which no other config runs;
  * one bi-LSTM layer at the timed geometry (B=32, T=1000, H=512) against torch.nn.LSTM in float64, fixed and ragged lengths;
  * one bi-GRU / bi-LSTM layer at H = 1024 / 768 and T = 1000 against torch float64: the shipped encoder's inner and first layer,
    scattered length classes (dense and with the valid-frame table these shapes ignore), a batch the module splits along B, and the
    opt-in v5 forms (RNNT_LSTM_V5_WIDE=1);
  * config 3 at full size: the joint + loss segment never allocates anything near a (B,T,U+1,V) tensor.

Tolerances (fp32 path vs float64 oracle): NLL 1e-5 relative (north_star: 1e-4); input/weight gradients of the fused
entry 5e-5 of max(1, |ref|max); parameter gradients of the whole model 2e-4 of the tensor's max; single layers: outputs 2e-5
absolute, dx 2e-4 of its max, weight and bias gradients 2e-4 of the max of each gate's block, padded outputs and padded dx exact
zeros on NaN-poisoned memory.
"""
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import usable_cores
from test_gpu_lstm import _poison_free_memory
from oracle.rnnt_oracle import OracleJointNet, make_batch, rnnt_loss_c, training_loss

pytestmark = pytest.mark.gpu
ARGS = Namespace(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=100,
                 move_metrics_to_cpu=False)
SHAPES = {  # name: (T, U, V, O) of BASELINE.json configs[1], [2], [4]
    "c2": (1000, 40, 72, 512),
    "c3": (2000, 120, 72, 512),
    "c5": (1500, 80, 2048, 640),
}


def _gelu64(x):
    return torch.nn.functional.gelu(x, approximate="tanh")


@pytest.mark.parametrize("cfg", list(SHAPES))
def test_fused_joint_loss_at_baseline_lattice_shapes(cfg):
    """Two utterances (one full length, one ragged) at the config's T, U, V and joint width O."""
    from rnntransducer_amd.ops import JointLossFn
    T, U, V, O = SHAPES[cfg]
    B = 2
    g = torch.Generator().manual_seed(1000 + T + U + V)
    enc = torch.randn(B, T, O, generator=g, dtype=torch.float64)
    dec = torch.randn(B, U + 1, O, generator=g, dtype=torch.float64)
    W = torch.randn(V, 2 * O, generator=g, dtype=torch.float64) * (1.0 / O ** 0.5)
    bias = torch.randn(V, generator=g, dtype=torch.float64) * 0.1
    y = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
    t_lens, u_lens = [T, (2 * T) // 3 + 1], [U, (2 * U) // 3]
    # float64 oracle.  c2: the MATERIALISING joint of networks/transducer.py:58-69; c3 / c5: its separable equal
    # (A[b,t] + C[b,u] + bias — equality pinned at small sizes by test_gpu_loss.py and tests/test_oracle_networks.py),
    # because the (B,T,U+1,2*O) float64 concat of c3/c5 is 8-10 GB per copy
    e, d, w, bb = (x.clone().requires_grad_(True) for x in (enc, dec, W, bias))
    if cfg == "c2":
        cat = torch.cat((e[:, :, None, :].expand(-1, -1, U + 1, -1), d[:, None, :, :].expand(-1, T, -1, -1)), -1)
        logits = _gelu64(cat) @ w.T + bb
    else:
        A = _gelu64(e) @ w[:, :O].T
        Cm = _gelu64(d) @ w[:, O:].T
        logits = A[:, :, None, :] + Cm[:, None, :, :] + bb
    ref_nll, dlog = rnnt_loss_c(logits.detach().numpy(), y.numpy(), t_lens, u_lens, 0)
    gw = torch.tensor([1.0, 0.5], dtype=torch.float64)
    logits.backward(torch.from_numpy(dlog) * gw.view(-1, 1, 1, 1))
    del dlog, logits
    dev = "cuda"
    te = enc.float().transpose(0, 1).contiguous().to(dev).requires_grad_(True)
    td = dec.float().transpose(0, 1).contiguous().to(dev).requires_grad_(True)
    tw = W.float().to(dev).requires_grad_(True)
    tb = bias.float().to(dev).requires_grad_(True)
    nll = JointLossFn.apply(te, td, tw, tb, y.to(dev), torch.tensor(t_lens, dtype=torch.int32, device=dev),
                            torch.tensor(u_lens, dtype=torch.int32, device=dev), 0)
    (nll * gw.float().to(dev)).sum().backward()
    np.testing.assert_allclose(nll.detach().cpu().numpy(), ref_nll, rtol=1e-5)
    for name, got, ref in (("d_enc", te.grad.transpose(0, 1), e.grad), ("d_dec", td.grad.transpose(0, 1), d.grad),
                           ("d_fc.weight", tw.grad, w.grad), ("d_fc.bias", tb.grad, bb.grad)):
        err = (got.double().cpu() - ref).abs().max().item()
        assert err < 5e-5 * max(1.0, ref.abs().max().item()), f"{cfg} {name}: {err} (ref max {ref.abs().max().item()})"
    # padded frames / label positions get no gradient (warp-transducer convention)
    assert te.grad[t_lens[1]:, 1].abs().max().item() == 0.0
    assert td.grad[u_lens[1] + 1:, 1].abs().max().item() == 0.0


def _two_utterances_equal_frames_ragged_labels(T, U, V, seed):
    """Two utterances of T frames each, the second with 2U/3 labels.  Equal frame counts let the float64 oracle run its LSTMs as one
    plain batch (its autograd costs ~60 us per timestep node: config 3 / 5 sizes with per-utterance calls took 2-3 minutes on the GPU
    box); ragged FRAME counts at these sizes are covered by the LSTM-level tests and by config 2 above."""
    a, a_list, a_len, texts, t_list, targets, u_len = make_batch(2, T, U, V, ragged=False, seed=seed)
    u1 = (2 * U) // 3
    targets[1, u1:] = 0
    texts[1, u1 + 1:] = 0
    u_len[1] = u1
    return (a, a_list, a_len, texts, [U + 1, u1 + 1], targets, u_len)


def _embed_rows(small, big):
    """The 7-tuple `big` with its first rows replaced by the rows of `small` (same T, U): the batch the HIP path runs while the
    float64 oracle runs `small` alone."""
    n = small[0].shape[0]
    out = []
    for a, b in zip(small, big):
        if isinstance(a, torch.Tensor):
            c = b.clone()
            c[:n] = a
            out.append(c)
        else:
            out.append(list(a) + list(b[n:]))
    return tuple(out)


def _oracle_step(tn, pn, V, model, small, per_utterance, separable):
    """float64 oracle on the batch `small` with the model's weights -> (loss, {name: grad})."""
    from oracle import rnnt_oracle as ro
    oracle = OracleJointNet(dict(tn), dict(pn, pad_token_id=0), V).double()
    oracle.load_state_dict({k[len("jointnet."):]: v.double() for k, v in model.state_dict().items()})
    torch.set_num_threads(usable_cores())
    ro.PER_UTTERANCE = per_utterance   # config 3 / 5 sizes: autograd through a PackedSequence is O(T^2) on the CPU (equality pinned
    try:                               # by tests/test_oracle_networks.py::test_per_utterance_lstm_equals_the_packed_one)
        ref = training_loss(oracle, (small[0].double(),) + small[1:], separable=separable)
        ref.backward()
    finally:
        ro.PER_UTTERANCE = False
    return ref.item(), {k: p.grad for k, p in oracle.named_parameters()}


def _hip_step_on_first_rows(model, batch, n):
    """HIP step on the WHOLE batch with per-utterance losses; the mean over the first n utterances is back-propagated, i.e. the
    other rows get upstream weight 0 (rows are independent: they then contribute to no gradient).  -> (loss, all nll, grads)."""
    for p in model.parameters():
        p.grad = None
    dev = tuple(x.cuda() if isinstance(x, torch.Tensor) else x for x in batch)
    nll = model.jointnet.loss(dev[0], dev[2], dev[3], dev[5], dev[6], model.blank_token_id, reduction="none", audio_lengths=dev[1])
    loss = nll[:n].mean()
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), nll.detach().cpu(), {k: p.grad.double().cpu() for k, p in model.jointnet.named_parameters()}


def _assert_step_matches(tag, loss, grads, ref_loss, ref_grads, loss_rtol=1e-5, grad_rtol=2e-4):
    assert abs(loss - ref_loss) / abs(ref_loss) < loss_rtol, f"{tag}: loss {loss} vs float64 oracle {ref_loss}"
    worst = ("", 0.0)
    for name, q in ref_grads.items():
        scale = max(q.abs().max().item(), 1e-3)
        rel = (grads[name] - q).abs().max().item() / scale
        if rel > worst[1]:
            worst = (name, rel)
        assert rel < grad_rtol, f"{tag} {name}: {rel:.3e} of max |grad| {scale:.3e}"
    print(f"{tag}: loss rel {abs(loss - ref_loss) / abs(ref_loss):.2e}; worst gradient {worst[0]} {worst[1]:.2e} of max")


def test_full_model_config2_dims_step_vs_float64_oracle():
    """BASELINE configs[1] layer sizes (enc 4x512 bi-LSTM, pred 1x512, O=512, V=72), T=1000, U=40, dropout off on both sides: loss +
    every parameter gradient against the float64 oracle on two utterances (second one ragged) —
      (a) HIP at B=2 (training_step, reduction "mean");
      (b) HIP at B=32, THE LAUNCH bench.py TIMES (8 sync groups x 32 workgroups per recurrence, 1000 tagged exchange steps x 4
          layers): the two utterances are rows 0-1 of a 32-row batch, the other 30 rows get upstream weight 0;
      (c) batch invariance: the per-utterance NLL of rows 0-1 is the same number in both launches."""
    from rnntransducer_amd import RNNTransducer
    V = 72
    tn = dict(input_size=80, hidden_size=512, output_size=512, num_layers=4, rnn_type="lstm", dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=V, hidden_size=512, output_size=512, num_layers=1, rnn_type="lstm", dropout=0.0)
    torch.manual_seed(0)
    model = RNNTransducer(dict(pn), dict(tn), dict(num_classes=V), ARGS)
    small = make_batch(2, 1000, 40, V, ragged=True, seed=7)
    ref_loss, ref_grads = _oracle_step(tn, pn, V, model, small, per_utterance=False, separable=False)
    model = model.cuda().train()
    dev_batch = tuple(x.cuda() if isinstance(x, torch.Tensor) else x for x in small)
    out = model.training_step(dev_batch, 0)
    out["loss"].backward()
    _assert_step_matches("config-2 dims, B=2", out["loss"].item(), {k: p.grad.double().cpu() for k, p in model.jointnet.named_parameters()},
                         ref_loss, ref_grads)
    _, nll2, _ = _hip_step_on_first_rows(model, small, 2)
    big = _embed_rows(small, make_batch(32, 1000, 40, V, ragged=False, seed=8))
    loss32, nll32, grads32 = _hip_step_on_first_rows(model, big, 2)
    assert torch.isfinite(nll32).all()
    _assert_step_matches("config-2 dims, B=32 launch (rows 2.. weight 0)", loss32, grads32, ref_loss, ref_grads)
    assert torch.allclose(nll32[:2], nll2, rtol=5e-6, atol=0), (nll32[:2], nll2)


def test_full_model_config3_geometry_step_vs_float64_oracle():
    """BASELINE configs[2] geometry: B=8 (the recurrences' 4-row sync groups), T=2000, U=120, V=72, 4x512 bi-LSTM / 1x512, INITIAL
    weights, dropout off.  float64 oracle (separable joint: the concat is 7.9 GB per copy at this size) on utterances 0-1 (second one
    with 2U/3 labels); the HIP path runs all 8 rows with upstream weight 0 on rows 2-7.  Loss 1e-5 relative, every gradient 2e-4 of its maximum."""
    from rnntransducer_amd import RNNTransducer
    V = 72
    tn = dict(input_size=80, hidden_size=512, output_size=512, num_layers=4, rnn_type="lstm", dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=V, hidden_size=512, output_size=512, num_layers=1, rnn_type="lstm", dropout=0.0)
    torch.manual_seed(1)
    model = RNNTransducer(dict(pn), dict(tn), dict(num_classes=V), ARGS)
    small = _two_utterances_equal_frames_ragged_labels(2000, 120, V, seed=11)
    ref_loss, ref_grads = _oracle_step(tn, pn, V, model, small, per_utterance=True, separable=True)
    model = model.cuda().train()
    big = _embed_rows(small, make_batch(8, 2000, 120, V, ragged=False, seed=12))
    loss, nll, grads = _hip_step_on_first_rows(model, big, 2)
    assert torch.isfinite(nll).all()
    _assert_step_matches("config-3 geometry, B=8 launch (rows 2.. weight 0)", loss, grads, ref_loss, ref_grads)


def _assert_b2_and_timed_launch(tag, model, small, big, ref_loss, ref_grads):
    """HIP steps against the float64 oracle of `small` (two utterances): (a) at B=2; (b) on `big`, the launch bench.py times, whose rows
    0-1 are `small` and whose other rows get upstream weight 0; (c) every NLL of (b) finite, and rows 0-1 give the same NLL in both
    launches (batch invariance).  -> allocator peak of (b) in bytes."""
    loss2, nll2, grads2 = _hip_step_on_first_rows(model, small, 2)
    _assert_step_matches(f"{tag}, B=2", loss2, grads2, ref_loss, ref_grads)
    del grads2
    torch.cuda.reset_peak_memory_stats()
    loss_b, nll_b, grads_b = _hip_step_on_first_rows(model, big, 2)
    peak = torch.cuda.max_memory_allocated()
    assert torch.isfinite(nll_b).all(), nll_b
    _assert_step_matches(f"{tag}, B={big[0].shape[0]} launch (rows 2.. weight 0)", loss_b, grads_b, ref_loss, ref_grads)
    assert torch.allclose(nll_b[:2], nll2, rtol=5e-6, atol=0), (nll_b[:2], nll2)
    return peak


def test_full_model_config5_dims_step_vs_float64_oracle():
    """BASELINE configs[4] layer sizes: 6x640 bi-LSTM encoder (20-unit workgroups, K padded to 768, two-barrier backward), 1x640
    prediction net, O=640, V=2048 (vocab-tiled lattice kernels), T=1500, U=80, two utterances (second one with 2U/3 labels), INITIAL
    weights, dropout off: loss 1e-5 relative, every parameter gradient 2e-4 of its maximum against the float64 oracle (separable joint:
    10 GB per concat copy) — at B=2 and on the B=16 launch bench.py times (two sync groups per direction, rows 2.. weight 0), plus
    batch invariance of the per-utterance NLL."""
    from rnntransducer_amd import RNNTransducer
    V = 2048
    tn = dict(input_size=80, hidden_size=640, output_size=640, num_layers=6, rnn_type="lstm", dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=V, hidden_size=640, output_size=640, num_layers=1, rnn_type="lstm", dropout=0.0)
    torch.manual_seed(2)
    model = RNNTransducer(dict(pn), dict(tn), dict(num_classes=V), ARGS)
    small = _two_utterances_equal_frames_ragged_labels(1500, 80, V, seed=13)
    ref_loss, ref_grads = _oracle_step(tn, pn, V, model, small, per_utterance=True, separable=True)
    model = model.cuda().train()
    big = _embed_rows(small, make_batch(16, 1500, 80, V, ragged=False, seed=14))
    _assert_b2_and_timed_launch("config-5 dims", model, small, big, ref_loss, ref_grads)


def test_full_model_shipped_config_step_vs_float64_oracle():
    """The reference's shipped config/config.json (bench.py --config shipped): 8x1024 bi-GRU encoder (the v3 / v4 register-form
    recurrences, two 8-row sync groups per direction at B=16; the GRU backward without the fused dX split or the grouped weight-gradient
    launch), 2x1024 LSTM prediction net, O=512, V=72, T=1000, U=40, INITIAL weights, dropout off.  Two utterances (second one with 2U/3
    labels) against the float64 oracle: loss 1e-5 relative and every parameter gradient — all 8 encoder layers, every GRU bias, both
    prediction-net layers, out_proj — 2e-4 of its maximum, at B=2 and on the B=16 launch bench.py times (rows 2.. weight 0), plus
    batch invariance of the per-utterance NLL."""
    import time
    from rnntransducer_amd import RNNTransducer
    V = 72
    tn = dict(input_size=80, hidden_size=1024, output_size=512, num_layers=8, rnn_type="gru", dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=V, hidden_size=1024, output_size=512, num_layers=2, rnn_type="lstm", dropout=0.0)
    torch.manual_seed(3)
    model = RNNTransducer(dict(pn), dict(tn), dict(num_classes=V), ARGS)
    small = _two_utterances_equal_frames_ragged_labels(1000, 40, V, seed=17)
    t0 = time.perf_counter()
    ref_loss, ref_grads = _oracle_step(tn, pn, V, model, small, per_utterance=True, separable=True)
    t1 = time.perf_counter()
    model = model.cuda().train()
    big = _embed_rows(small, make_batch(16, 1000, 40, V, ragged=False, seed=18))
    peak = _assert_b2_and_timed_launch("shipped config", model, small, big, ref_loss, ref_grads)
    print(f"shipped config: float64 oracle {t1 - t0:.1f} s, HIP steps {time.perf_counter() - t1:.1f} s; "
          f"B=16 step allocator peak {peak / 2**30:.2f} GiB")


def _lstm_float64_by_length_class(ref, x, lens, dy):
    """torch.nn.LSTM / GRU float64 on a ragged batch WITHOUT a PackedSequence (whose CPU autograd is O(T^2): 139 s at this size): rows
    of equal length form one plain batch cut to that length — a packed batch treats rows independently and ends each at its own
    length, so this is the same function.  -> (out (B,T,D*H) zero on padding, dx); parameter gradients accumulate in `ref`."""
    T = x.shape[1]
    out = torch.zeros(x.shape[0], T, dy.shape[-1], dtype=torch.float64)
    dx = torch.zeros_like(x, dtype=torch.float64)
    for n in sorted(set(lens)):
        rows = [b for b, l in enumerate(lens) if l == n]
        xr = x[rows, :n].double().requires_grad_(True)
        y, _ = ref(xr)
        y.backward(dy[rows, :n].double())
        out[rows, :n] = y.detach()
        dx[rows, :n] = xr.grad
    return out, dx


def _layer_inputs(B, T, I, H, lens, seed):
    """x (B,T,I) zero on padding, dy (B,T,2H) and the length list with its classes scattered over the rows, as a collate hands them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, I, generator=g)
    dy = torch.randn(B, T, 2 * H, generator=g)
    perm = torch.randperm(B, generator=g).tolist()
    lens = [lens[i] for i in perm]
    for b in range(B):
        x[b, lens[b]:] = 0
    return x, dy, lens


def _assert_layer_matches(tag, hip, ref, x, dy, lens, ref_out, ref_dx, lens_arg):
    """One HIP layer call (fwd + bwd) on NaN-poisoned memory against the float64 result: outputs within 2e-5, padded outputs and padded
    dx exact zeros (not masked before comparing), dx within 2e-4 of its max and every weight / bias gradient within 2e-4 of the max
    of its own gate block (the gates' rows are stacked along dim 0; a gate whose gradients are small next to the others' is held to
    its own scale — a 1e-3 relative error in the GRU z gate's bias gradient stays below 2e-4 of the whole tensor's max)."""
    B = x.shape[0]
    for q in hip.parameters():
        q.grad = None
    _poison_free_memory()
    x_tm = x.transpose(0, 1).contiguous().cuda().requires_grad_(True)
    y = hip(x_tm, lens_arg)
    y.backward(dy.transpose(0, 1).contiguous().cuda())
    torch.cuda.synchronize()
    err = (y.detach().transpose(0, 1).double().cpu() - ref_out).abs().max().item()
    assert err < 2e-5, f"{tag}: forward err {err}"
    for b in range(B):
        assert torch.all(y[lens[b]:, b] == 0), f"{tag}: output of padded frames of row {b}"
        assert torch.all(x_tm.grad[lens[b]:, b] == 0), f"{tag}: dx of padded frames of row {b}"
    worst = ("", 0.0)
    gates = ref.weight_ih_l0.shape[0] // ref.hidden_size
    blocks = [("dx", x_tm.grad.transpose(0, 1), ref_dx)]
    for k, p in ref.named_parameters():
        blocks += [(f"{k}[gate {i}]", got, want) for i, (got, want) in enumerate(zip(getattr(hip, k).grad.chunk(gates), p.grad.chunk(gates)))]
    for nm, got, want in blocks:
        scale = max(want.abs().max().item(), 1e-3)
        e = (got.double().cpu() - want).abs().max().item() / scale
        worst = max(worst, (nm, e), key=lambda t: t[1])
        assert e < 2e-4, f"{tag} {nm}: {e:.3e} of max {scale:.3e}"
    print(f"{tag}: forward err {err:.2e}, worst gradient {worst[0]} {worst[1]:.2e} of max")


@pytest.mark.parametrize("name,I,lens", [
    ("fixed lengths, inner-layer width (the launch bench.py times)", 1024, [1000] * 32),
    ("four length classes, layer-0 width (the c4 / --ragged shape)", 80, [1000] * 8 + [873] * 8 + [640] * 8 + [501] * 8),
])
def test_lstm_layer_at_the_timed_launch_geometry_vs_torch_float64(name, I, lens):
    """One bi-LSTM layer at BASELINE configs[1]'s launch geometry — B=32, T=1000, H=512: 8 sync groups x 32 workgroups, 1000 steps of
    the tagged exchange — against torch.nn.LSTM float64 on the CPU: outputs, dx and every weight gradient (VERDICT r2 weak #1b: the
    B=32 tests stopped at T=40).  Padded outputs and padded dx are exact zeros, dense and with the valid-frame table."""
    from rnntransducer_amd.networks.rnn import HipLSTM
    from rnntransducer_amd.ops import RaggedPlan
    B, T, H = 32, 1000, 512
    torch.manual_seed(31 + I)
    ref = torch.nn.LSTM(I, H, 1, batch_first=True, bidirectional=True).double()
    hip = HipLSTM(I, H, 1, dropout=0.0, bidirectional=True)
    hip.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    hip = hip.cuda()
    x, dy, lens = _layer_inputs(B, T, I, H, lens, seed=5)
    torch.set_num_threads(usable_cores())
    ref_out, ref_dx = _lstm_float64_by_length_class(ref, x, lens, dy)
    variants = [("dense", torch.tensor(lens, dtype=torch.int32, device="cuda"))]
    if min(lens) < T:   # the same launch with the valid-frame table (what training_step builds from the collate's length list)
        variants.append(("valid-frame table", RaggedPlan(lens, T, "cuda")))
    for vname, lens_arg in variants:
        _assert_layer_matches(f"B=32 T=1000 H=512 I={I} ({name}, {vname})", hip, ref, x, dy, lens, ref_out, ref_dx, lens_arg)


_FOUR_CLASSES = (1000, 873, 640, 501)


@pytest.mark.parametrize("cell,H,I,B,classes,wide", [
    ("gru", 1024, 2048, 16, (1000,), False),        # shipped encoder, inner layer, the launch bench.py times (2 x 8-row groups / dir)
    ("gru", 1024, 80, 16, _FOUR_CLASSES, True),     # shipped encoder, layer 0, ragged: in-kernel length masking over 1000 steps
    ("gru", 1024, 80, 40, _FOUR_CLASSES, False),    # beyond one launch: 32 rows (2 x 16-row groups / dir) + 8 rows (2 x 4-row groups)
    ("lstm", 1024, 1024, 16, _FOUR_CLASSES, True),  # shipped prediction-net width as a bi-LSTM layer
    ("gru", 768, 80, 16, _FOUR_CLASSES, False),     # the other width whose default is v3 / v4
], ids=["gru1024-I2048-B16-fixed", "gru1024-I80-B16-ragged", "gru1024-I80-B40-ragged", "lstm1024-I1024-B16-ragged",
        "gru768-I80-B16-ragged"])
def test_wide_recurrent_layer_at_the_timed_length_vs_torch_float64(monkeypatch, cell, H, I, B, classes, wide):
    """One bidirectional GRU / LSTM layer at H = 1024 / 768 over T = 1000 steps — the v3 / v4 register-form recurrences (8 waves) that
    the shipped config runs, which test_gpu_lstm.py checks for at most 6 steps — against torch.nn.GRU / LSTM float64 on the CPU:
    outputs, dx and every weight and bias gradient; padded outputs and padded dx exact zeros.  Ragged cases scatter the length
    classes over the rows and run dense and with a valid-frame table, which these shapes ignore (the reverse direction then starts at
    each row's own last frame by in-kernel masking alone).  `wide`: the same calls again under the opt-in v5 forms (RNNT_LSTM_V5_WIDE=1)
    against the same float64 result."""
    from rnntransducer_amd import _lib
    from rnntransducer_amd.networks.rnn import HipGRU, HipLSTM
    from rnntransducer_amd.ops import RaggedPlan
    T = 1000
    monkeypatch.delenv("RNNT_LSTM_V5_WIDE", raising=False)
    torch.manual_seed(H + I + B)
    ref = (torch.nn.GRU if cell == "gru" else torch.nn.LSTM)(I, H, 1, batch_first=True, bidirectional=True).double()
    hip = (HipGRU if cell == "gru" else HipLSTM)(I, H, 1, dropout=0.0, bidirectional=True)
    hip.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    hip = hip.cuda()
    x, dy, lens = _layer_inputs(B, T, I, H, [classes[i * len(classes) // B] for i in range(B)], seed=H + B)
    cap = _lib.lib().rnnt_hip_lstm_max_batch(H, 2, hip.CELL)
    assert (B > cap) == (B == 40), f"one launch takes {cap} rows at H={H}"   # B=40 is the one case the module splits along B
    torch.set_num_threads(usable_cores())
    ref_out, ref_dx = _lstm_float64_by_length_class(ref, x, lens, dy)
    variants = [("dense", torch.tensor(lens, dtype=torch.int32, device="cuda"))]
    if min(lens) < T:
        variants.append(("valid-frame table", RaggedPlan(lens, T, "cuda")))
    forms = [("v3/v4", False)] + ([("v5 wide", True)] if wide else [])
    for form, on in forms:
        if on:
            monkeypatch.setenv("RNNT_LSTM_V5_WIDE", "1")
        if B <= cap:   # the default forms ignore the table at this width; the v5 forms honour it
            assert _lib.lib().rnnt_hip_lstm_takes_row_idx(T, B, I, H, 2, hip.CELL) == int(on)
        for vname, lens_arg in variants:
            _assert_layer_matches(f"{cell.upper()} B={B} T={T} H={H} I={I} ({form}, {vname})", hip, ref, x, dy, lens, ref_out, ref_dx,
                                  lens_arg)


def test_config3_full_size_joint_loss_never_materialises_btuv():
    """BASELINE configs[2] (B=8, T=2000, U=120, V=72, O=512) at FULL size: allocator peak of the fused joint + loss +
    its backward stays below 30 % of ONE (B,T,U+1,V) logits tensor (the reference builds that plus three
    (B,T,U+1,2*O) tensors, networks/transducer.py:61-69)."""
    from rnntransducer_amd.ops import JointLossFn
    B, T, U, V, O = 8, 2000, 120, 72, 512
    g = torch.Generator(device="cuda").manual_seed(3)
    enc = torch.randn(T, B, O, device="cuda", generator=g).requires_grad_(True)
    dec = torch.randn(U + 1, B, O, device="cuda", generator=g).requires_grad_(True)
    W = (torch.randn(V, 2 * O, device="cuda", generator=g) * 0.05).requires_grad_(True)
    bias = torch.zeros(V, device="cuda", requires_grad=True)
    y = torch.randint(1, V, (B, U), device="cuda", generator=g, dtype=torch.int32)
    t_lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    u_lens = torch.full((B,), U, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    nll = JointLossFn.apply(enc, dec, W, bias, y, t_lens, u_lens, 0)
    nll.mean().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    logits_bytes = B * T * (U + 1) * V * 4
    assert torch.isfinite(nll).all()
    assert peak < 0.3 * logits_bytes, (peak, logits_bytes)
