"""Opt-in fp16 compute mode of the recurrent layers (include/rnnt_hip.h RNNT_PRECISION_F16, RNNT_GEMM_HP_F16):
the half-pair products and the v5 recurrences multiply only the hi halves of their operands (f16 rounding of each row-scaled
operand, fp32 accumulation).

  1. the mode is real: a product whose operands' lo pieces matter equals the fp64 product of the hi pieces, not the fp32 one;
  2. accuracy against float64 torch / the float64 oracle: single layers (every cell and v5 width, D = 1 and 2, dense and ragged) and
     the full model at config-2 dimensions;
  3. fallbacks are honest: where a layer has no one-product form the fp16 mode is bitwise the fp32 mode, and it says so;
  4. fp32 mode is untouched by the existence of the other mode;
  5. training: reproducible, autocast + GradScaler neutral, 50 AdamW steps end near the fp32 run;
  6. guards.

Bounds of the fp16 mode against float64 (the measured values are in DESIGN.md §11): layer outputs 5e-3 absolute, loss 2e-3 relative,
every gradient ||g - g64|| / ||g64|| <= 2e-2 with cosine >= 0.999.
"""
import ctypes as C
from argparse import Namespace

import pytest
import torch
import torch.nn as nn

from conftest import usable_cores

pytestmark = pytest.mark.gpu
OUT_ATOL, LOSS_RTOL, GRAD_RNORM, GRAD_COS = 5e-3, 2e-3, 2e-2, 0.999
ARGS = dict(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=100, move_metrics_to_cpu=False)


def _hi_pieces(t, rows, K):
    """The hi halves of hp planes as fp64 values of the ORIGINAL matrix: hi / row scale (gemm_hp.hip's plane layout and scale)."""
    Kp = (K + 31) // 32 * 32
    planes = t.planes[: rows * Kp * 4].view(torch.float16).view(rows, Kp // 32, 2, 32)
    hi = planes[:, :, 0, :].reshape(rows, Kp)[:, :K].double().cpu()
    eb = ((t.amax[:rows].cpu().long() >> 23) & 255).clamp(min=15)
    scale = torch.where(t.amax[:rows].cpu() == 0, torch.ones(rows, dtype=torch.float64), torch.pow(2.0, (141 - eb).double()))
    return hi / scale[:, None]


def test_gemm_hp_f16_flag_multiplies_the_hi_pieces_only():
    """A = (1 + 2^-12) * S with S a power of two per element: the f16 hi piece of every A element is S exactly (1 + 2^-12 rounds to 1
    in 11 bits), the lo piece carries the 2^-12.  With RNNT_GEMM_HP_F16 the product is the fp64 product of the hi pieces (to fp32
    accumulation error) and misses the fp64 product of the inputs by about 2^-12; without it, it is the fp32-grade product as before.
    Same for the queue-driven grouped launch."""
    from rnntransducer_amd import ops
    g = torch.Generator().manual_seed(3)
    M, N, K = 384, 320, 1024
    S = torch.pow(2.0, torch.randint(-3, 2, (M, K), generator=g).double()) * (torch.randint(0, 2, (M, K), generator=g) * 2 - 1)
    A = (S * (1.0 + 2.0 ** -12)).float()
    Bm = torch.randn(N, K, generator=g)
    exact = A.double() @ Bm.double().T
    a, b = ops.hp_split(A.cuda()), ops.hp_split(Bm.cuda())
    assert torch.equal(_hi_pieces(a, M, K), S)                          # the premise: hi(A) = S
    hi_prod = _hi_pieces(a, M, K) @ _hi_pieces(b, N, K).T
    bound = (_hi_pieces(a, M, K).abs() @ _hi_pieces(b, N, K).abs().T)   # fp32 accumulation error scale per element
    c16 = ops.gemm_hp(a, b, f16=True).double().cpu()
    c32 = ops.gemm_hp(a, b).double().cpu()
    torch.cuda.synchronize()
    assert ((c16 - hi_prod).abs() <= 1e-5 * bound).all()
    assert ((c32 - exact).abs() <= 1e-5 * (A.double().abs() @ Bm.double().abs().T)).all()
    assert (c16 - exact).abs().max().item() > 30 * (c32 - exact).abs().max().item()
    q16, q32 = ops.gemm_hp_grouped([(a, b), (b, a)], f16=True), ops.gemm_hp_grouped([(a, b)])
    assert ((q16[0].double().cpu() - hi_prod).abs() <= 1e-5 * bound).all()
    assert ((q16[1].double().cpu() - hi_prod.T).abs() <= 1e-5 * bound.T).all()
    assert ((q32[0].double().cpu() - exact).abs() <= 1e-5 * (A.double().abs() @ Bm.double().abs().T)).all()


def _ref_module(cell, I, H, bi, seed):
    torch.manual_seed(seed)
    if cell == "lstm":
        return nn.LSTM(I, H, 1, batch_first=True, bidirectional=bi).double()
    if cell == "gru":
        return nn.GRU(I, H, 1, batch_first=True, bidirectional=bi).double()
    return nn.RNN(I, H, 1, batch_first=True, bidirectional=bi, nonlinearity=cell.split("_")[1]).double()


def _hip_module(cell, I, H, bi, ref):
    from rnntransducer_amd.networks.rnn import HipGRU, HipLSTM, HipRNN
    if cell == "lstm":
        hip = HipLSTM(I, H, 1, bidirectional=bi)
    elif cell == "gru":
        hip = HipGRU(I, H, 1, bidirectional=bi)
    else:
        hip = HipRNN(I, H, 1, bidirectional=bi, nonlinearity=cell.split("_")[1])
    hip.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    return hip.cuda()


def _layer_case(cell, B, T, I, H, bi, seed=1):
    g = torch.Generator().manual_seed(seed)
    lens = [T] + torch.randint(T // 2, T + 1, (B - 1,), generator=g).tolist()
    x = torch.randn(B, T, I, generator=g)
    for b in range(B):
        x[b, lens[b]:] = 0
    dy = torch.randn(B, T, (2 if bi else 1) * H, generator=g)
    return lens, x, dy


def _oracle(ref, x, lens, dy):
    torch.set_num_threads(usable_cores())
    T = x.shape[1]
    xr = x.double().requires_grad_(True)
    packed = nn.utils.rnn.pack_padded_sequence(xr, torch.tensor(lens), batch_first=True, enforce_sorted=False)
    out, _ = ref(packed)
    out, _ = nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=T)
    out.backward(dy.double())
    return out.detach(), xr.grad, {k: p.grad for k, p in ref.named_parameters()}


def _hip_run(hip, x, lens, dy, precision, plan=False):
    from rnntransducer_amd.ops import RaggedPlan
    hip.compute_precision = precision
    hip.zero_grad()
    T = x.shape[1]
    x_tm = x.transpose(0, 1).contiguous().cuda().requires_grad_(True)
    lens_arg = RaggedPlan(lens, T, "cuda") if plan else torch.tensor(lens, dtype=torch.int32, device="cuda")
    y = hip(x_tm, lens_arg)
    y.backward(dy.transpose(0, 1).contiguous().cuda())
    torch.cuda.synchronize()
    grads = {k: p.grad.double().cpu().clone() for k, p in hip.named_parameters()}
    return y.detach().transpose(0, 1).double().cpu(), x_tm.grad.transpose(0, 1).double().cpu(), grads


def _grad_stats(got, want):
    g, w = got.flatten(), want.flatten()
    rn = ((g - w).norm() / w.norm().clamp(min=1e-30)).item()
    cos = (torch.dot(g, w) / (g.norm() * w.norm()).clamp(min=1e-30)).item()
    return rn, cos


def test_lstm_layer_at_c2_width_f16_mode_differs_from_fp32_and_is_f16_accurate():
    """One bi-LSTM layer at config-2 width (B = 32, H = 512, I = 80): the f16 mode gives different numbers from the fp32 mode, and its
    distance from float64 lies above the fp32 mode's own bound (2e-5, tests/test_gpu_lstm.py) and inside the f16 bound."""
    B, T, I, H = 32, 64, 80, 512
    ref = _ref_module("lstm", I, H, True, 5)
    hip = _hip_module("lstm", I, H, True, ref)
    lens, x, dy = _layer_case("lstm", B, T, I, H, True)
    assert hip.effective_precision(T, B) == "fp32"          # the default mode
    hip.compute_precision = "fp16"
    assert hip.effective_precision(T, B) == "fp16"
    out64, _, _ = _oracle(ref, x, lens, dy)
    y32, _, _ = _hip_run(hip, x, lens, dy, "fp32")
    y16, _, _ = _hip_run(hip, x, lens, dy, "fp16")
    e32, e16 = (y32 - out64).abs().max().item(), (y16 - out64).abs().max().item()
    print(f"c2-width layer: fp32 err {e32:.2e}, fp16 err {e16:.2e}")
    assert not torch.equal(y16, y32)
    assert e32 < 2e-5 < e16 < OUT_ATOL


@pytest.mark.parametrize("bi", [False, True])
@pytest.mark.parametrize("H", [128, 256, 384, 512, 640])
@pytest.mark.parametrize("cell", ["lstm", "gru", "rnn_tanh"])
def test_single_layer_f16_mode_vs_float64(monkeypatch, cell, H, bi):
    """Forward + backward of one layer in fp16 mode against float64 torch, every cell and v5 width, D = 1 and 2, ragged lengths both
    as masked dense rows and through the valid-frame table (RaggedPlan).  RNNT_GEMM_FORCE_HP puts these small shapes on the
    half-pair products (so the whole layer runs the one-product forms)."""
    monkeypatch.setenv("RNNT_GEMM_FORCE_HP", "1")
    B, T, I = 16, 72, 128
    ref = _ref_module(cell, I, H, bi, H + bi)
    hip = _hip_module(cell, I, H, bi, ref)
    hip.compute_precision = "fp16"
    assert hip.effective_precision(T, B) == "fp16"
    lens, x, dy = _layer_case(cell, B, T, I, H, bi, seed=H)
    out64, dx64, g64 = _oracle(ref, x, lens, dy)
    worst = {}
    for plan in (False, True):
        y, dx, grads = _hip_run(hip, x, lens, dy, "fp16", plan=plan)
        e = (y - out64).abs().max().item()
        assert e < OUT_ATOL, f"plan={plan}: output err {e}"
        for b in range(B):   # padded frames: exact zeros, with and without a plan
            assert torch.all(y[b, lens[b]:] == 0)
            assert torch.all(dx[b, lens[b]:] == 0), f"plan={plan}: dx of padded frames, row {b}"
        for name, got, want in [("dx", dx, dx64)] + [(k, grads[k], g64[k]) for k in g64]:
            rn, cos = _grad_stats(got, want)
            worst[name] = max(worst.get(name, 0.0), rn)
            assert rn <= GRAD_RNORM and cos >= GRAD_COS, f"plan={plan} {name}: rel norm {rn:.2e}, cosine {cos:.6f}"
        worst["y"] = max(worst.get("y", 0.0), e)
    print(f"{cell} H={H} D={2 if bi else 1}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


def _model(tn, pn, V, precision, seed=0):
    from rnntransducer_amd import RNNTransducer
    torch.manual_seed(seed)
    return RNNTransducer(dict(pn), dict(tn), dict(num_classes=V), Namespace(compute_precision=precision, **ARGS))


def test_full_model_config2_dims_f16_mode_vs_float64_oracle():
    """Config-2 layer sizes (enc 4x512 bi-LSTM, pred 1x512, O = 512, V = 72), T = 1000, U = 40, dropout off, in fp16 mode at B = 32
    (the launch bench.py times): the two oracle utterances are rows 0-1, the other 30 rows get upstream weight 0 (as
    tests/test_gpu_configs.py).  Loss and every parameter gradient against the float64 oracle."""
    from tests.test_gpu_configs import _embed_rows, _hip_step_on_first_rows, _oracle_step
    from oracle.rnnt_oracle import make_batch
    V = 72
    tn = dict(input_size=80, hidden_size=512, output_size=512, num_layers=4, rnn_type="lstm", dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=V, hidden_size=512, output_size=512, num_layers=1, rnn_type="lstm", dropout=0.0)
    model = _model(tn, pn, V, "fp16")
    small = make_batch(2, 1000, 40, V, ragged=True, seed=7)
    ref_loss, ref_grads = _oracle_step(tn, pn, V, model, small, per_utterance=True, separable=False)
    model = model.cuda().train()
    assert model.jointnet.encoder.rnn.effective_precision(1000, 32) == "fp16"
    big = _embed_rows(small, make_batch(32, 1000, 40, V, ragged=False, seed=8))
    loss, nll, grads = _hip_step_on_first_rows(model, big, 2)
    assert torch.isfinite(nll).all()
    lrel = abs(loss - ref_loss) / abs(ref_loss)
    worst = ("", 0.0, 1.0)
    for name, q in ref_grads.items():
        rn, cos = _grad_stats(grads[name], q)
        if rn > worst[1]:
            worst = (name, rn, cos)
        assert rn <= GRAD_RNORM and cos >= GRAD_COS, f"{name}: rel norm {rn:.2e}, cosine {cos:.6f}"
    print(f"config-2 dims fp16 mode, B=32: loss rel {lrel:.2e}; worst gradient {worst[0]} rel norm {worst[1]:.2e} cosine {worst[2]:.6f}")
    assert lrel <= LOSS_RTOL


@pytest.mark.parametrize("cell,B,T,I,H,bi,why", [
    ("lstm", 16, 64, 128, 1024, True, "v3/v4"),        # H = 1024: lstm.hip's v3 / v4 forms (no one-product variant)
    ("lstm", 4, 8, 128, 128, True, "below hp"),        # M = 32 frames: the products stay on gemm.hip
    ("rnn_relu", 16, 80, 128, 256, True, "relu"),      # the ReLU cell has no v5 form
])
def test_fallbacks_are_bitwise_fp32_and_say_so(cell, B, T, I, H, bi, why):
    from rnntransducer_amd import _lib
    ref = _ref_module(cell, I, H, bi, 9)
    hip = _hip_module(cell, I, H, bi, ref)
    lens, x, dy = _layer_case(cell, B, T, I, H, bi)
    D = 2 if bi else 1
    assert _lib.lib().rnnt_hip_lstm_takes_f16(T, B, I, H, D, hip.CELL) == 0, why
    hip.compute_precision = "fp16"
    assert hip.effective_precision(T, B) == "fp32", why
    r32 = _hip_run(hip, x, lens, dy, "fp32")
    r16 = _hip_run(hip, x, lens, dy, "fp16")
    assert torch.equal(r32[0], r16[0]) and torch.equal(r32[1], r16[1])
    for k in r32[2]:
        assert torch.equal(r32[2][k], r16[2][k]), (why, k)


def test_takes_f16_reports_the_c2_shapes():
    from rnntransducer_amd import _lib
    L = _lib.lib()
    assert L.rnnt_hip_lstm_takes_f16(1000, 32, 80, 512, 2, 0) == 1      # encoder layer 0
    assert L.rnnt_hip_lstm_takes_f16(1000, 32, 1024, 512, 2, 0) == 1    # encoder layers 1..3
    # the prediction net (U + 1 = 41 frames x 32 = 1312 rows, 4H = 2048): below the half-pair products' size limit, fp32 in both modes
    assert L.rnnt_hip_lstm_takes_f16(41, 32, 512, 512, 1, 0) == 0


def _c2_model_and_batch(precision, seed=0):
    from rnntransducer_amd.data import synthetic_batch
    V = 72
    tn = dict(input_size=80, hidden_size=512, output_size=512, num_layers=4, rnn_type="lstm", dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=V, hidden_size=512, output_size=512, num_layers=1, rnn_type="lstm", dropout=0.0)
    model = _model(tn, pn, V, precision, seed).cuda().train()
    return model, synthetic_batch(32, 1000, 40, V, ragged=False, seed=1234, device="cuda")


def _step_grads(model, batch):
    for p in model.parameters():
        p.grad = None
    loss = model.training_step(batch, 0)["loss"]
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), [p.grad.clone() for p in model.parameters()]


def test_fp32_mode_is_untouched_by_fp16_steps_in_the_same_process():
    """A config-2 step in fp32 mode is bitwise the same before and after another module ran fp16 steps; the fp16 steps are bitwise
    reproducible run to run and differ from the fp32 ones."""
    m32, batch = _c2_model_and_batch("fp32")
    m16, _ = _c2_model_and_batch("fp16")
    l_a, g_a = _step_grads(m32, batch)
    l16a, g16a = _step_grads(m16, batch)
    l16b, g16b = _step_grads(m16, batch)
    l_b, g_b = _step_grads(m32, batch)
    assert torch.equal(l_a, l_b) and all(torch.equal(a, b) for a, b in zip(g_a, g_b))
    assert torch.equal(l16a, l16b) and all(torch.equal(a, b) for a, b in zip(g16a, g16b))
    # (the loss at initial weights moves less than its fp32 rounding when the encoder's outputs move by 1e-5: compare the gradients)
    assert any(not torch.equal(a, b) for a, b in zip(g16a, g_a))


def test_ex_entries_with_precision_0_are_bitwise_the_old_entries_and_reject_unknown_values():
    """rnnt_hip_lstm_fwd_ex / _bwd_ex (precision = 0) against rnnt_hip_lstm_fwd / _bwd on the same descriptor at config-2 width; an
    unknown precision value returns RNNT_ERR_INVALID before any device work."""
    from rnntransducer_amd import _lib, ops
    L = _lib.lib()
    T, B, I, H, D = 64, 32, 80, 512, 2
    torch.manual_seed(2)
    ws_w = [torch.randn(4 * H, I, device="cuda") * 0.05, torch.randn(4 * H, H, device="cuda") * 0.05,
            torch.randn(4 * H, device="cuda") * 0.05, torch.randn(4 * H, device="cuda") * 0.05] * D
    x = torch.randn(T, B, I, device="cuda")
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    dy = torch.randn(T, B, D * H, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    res = []
    for ex in (False, True):
        ws = ops.lstm_workspace(T, B, I, H, D, "cuda")
        y = torch.empty(T, B, D * H, device="cuda")
        gates = torch.empty(T, B, D * 4 * H, device="cuda")
        cst = torch.empty(D * T * B * H, device="cuda")
        d = _lib.LstmDesc()
        ops._fill_lstm_desc(d, T, B, I, H, D, lens, x, ws_w, y, None, 0.0, 1, gates, cst, ws)
        rc = L.rnnt_hip_lstm_fwd_ex(C.byref(d), 0, stream) if ex else L.rnnt_hip_lstm_fwd(C.byref(d), stream)
        assert rc == 0
        bd = _lib.LstmBwdDesc()
        ops._fill_lstm_desc(bd.f, T, B, I, H, D, lens, x, ws_w, y, None, 0.0, 1, gates, cst, ws)
        dx = torch.empty(T, B, I, device="cuda")
        dws = [[torch.empty_like(ws_w[0]), torch.empty_like(ws_w[1]), torch.empty_like(ws_w[2])] for _ in range(D)]
        bd.dy, bd.dx = ops._addr(dy), ops._addr(dx)
        for k in range(D):
            bd.dw_ih[k], bd.dw_hh[k], bd.db[k] = ops._addr(dws[k][0]), ops._addr(dws[k][1]), ops._addr(dws[k][2])
        rc = L.rnnt_hip_lstm_bwd_ex(C.byref(bd), 0, stream) if ex else L.rnnt_hip_lstm_bwd(C.byref(bd), stream)
        assert rc == 0
        torch.cuda.synchronize()
        res.append([y.clone(), dx.clone()] + [t.clone() for row in dws for t in row])
        if ex:
            assert L.rnnt_hip_lstm_fwd_ex(C.byref(d), 2, stream) == -1
            assert L.rnnt_hip_lstm_bwd_ex(C.byref(bd), 7, stream) == -1
    for a, b in zip(*res):
        assert torch.equal(a, b)


def _small_args_model(precision, seed=6):
    from rnntransducer_amd import RNNTransducer
    torch.manual_seed(seed)
    tn = dict(input_size=80, hidden_size=128, output_size=64, num_layers=2, dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=30, hidden_size=64, output_size=64, num_layers=1, dropout=0.0)
    return RNNTransducer(pn, tn, dict(num_classes=30), Namespace(compute_precision=precision, **ARGS)).cuda().train()


def _small_batch(seed=8):
    from rnntransducer_amd.data import synthetic_batch
    return synthetic_batch(16, 80, 9, 30, ragged=True, seed=seed, device="cuda")


def test_autocast_and_grad_scaler_take_the_fp16_mode_step(monkeypatch):
    """Under torch.autocast(float16) + GradScaler the fp16-mode model takes the same step as the fp16-mode model without autocast, and
    the scaler finds no overflow (the gradients stay fp32 views of the flat buffer)."""
    monkeypatch.setenv("RNNT_GEMM_FORCE_HP", "1")   # this small encoder (M = 1280 frames) on the half-pair products: fp16 mode is real
    batch = _small_batch()
    plain, amp = _small_args_model("fp16"), _small_args_model("fp16")
    assert plain.jointnet.encoder.rnn.effective_precision(80, 16) == "fp16"
    opts = [m.configure_optimizers()["optimizer"] for m in (plain, amp)]
    opts[0].zero_grad()
    l0 = plain.training_step(batch, 0)["loss"]
    l0.backward()
    opts[0].step()
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 14)
    opts[1].zero_grad()
    with torch.autocast("cuda", dtype=torch.float16):
        l1 = amp.training_step(batch, 0)["loss"]
    assert l1.dtype == torch.float32 and torch.equal(l1, l0)
    scaler.scale(l1).backward()
    scaler.step(opts[1])
    scaler.update()
    torch.cuda.synchronize()
    assert scaler.get_scale() == 2.0 ** 14
    for (n, a), (_, b) in zip(plain.named_parameters(), amp.named_parameters()):
        assert torch.allclose(a, b, rtol=0, atol=2e-7), n


def test_fifty_adamw_steps_in_fp16_mode_end_near_the_fp32_run(monkeypatch):
    """50 AdamW steps (OneCycle schedule, as configure_optimizers sets it up) on one small synthetic batch in each mode from the same
    initial weights: the loss falls in both, and the fp16 run's final loss is within 3 % of the fp32 run's."""
    monkeypatch.setenv("RNNT_GEMM_FORCE_HP", "1")
    batch = _small_batch(seed=11)
    finals = {}
    for precision in ("fp32", "fp16"):
        m = _small_args_model(precision, seed=21)
        conf = m.configure_optimizers()
        opt, sched = conf["optimizer"], conf["lr_scheduler"]["scheduler"]
        first = None
        for _ in range(50):
            opt.zero_grad()
            loss = m.training_step(batch, 0)["loss"]
            loss.backward()
            opt.step()
            sched.step()
            first = float(loss) if first is None else first
        with torch.no_grad():
            finals[precision] = float(m.training_step(batch, 0)["loss"])
        assert finals[precision] < first, (precision, first, finals[precision])
    print(f"50 AdamW steps: first loss {first:.5f}; final loss fp32 {finals['fp32']:.5f}, fp16 {finals['fp16']:.5f}")
    assert abs(finals["fp16"] - finals["fp32"]) <= 0.03 * finals["fp32"]


def test_guards():
    from rnntransducer_amd.networks.rnn import HipLSTM
    with pytest.raises(ValueError):
        _small_args_model("bf16")
    hip = HipLSTM(16, 128, 1).cuda()
    with pytest.raises(ValueError):
        hip.compute_precision = "half"
    assert hip.compute_precision == "fp32"
