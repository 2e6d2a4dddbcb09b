"""FastEmit regularisation of the RNN-T lattice gradient (csrc/loss.hip: the FE instances of grad_sep / grad_sepv / grad_dense) on the
device, against the float64 restatement tests/fastemit_restatement.py (itself checked on the CPU by tests/test_fastemit_oracle.py).

The fused kernels are driven through the C ABI with A, C and bias handed in directly, under both kernel families
(RNNT_LOSS_SMALLV_KERNELS=1, RNNT_LOSS_LARGEV_KERNELS=1); outputs and workspace start as NaN.  Bounds are those of
tests/test_gpu_loss_edges.py and tests/test_gpu_loss.py times (1 + lambda), the factor by which lambda scales the terms they bound."""
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import fastemit_restatement as fr

pytestmark = pytest.mark.gpu
NLL_RTOL, GRAD_TOL, DENSE_ATOL = 1e-5, 5e-5, 2e-5
FAMILIES = ("RNNT_LOSS_SMALLV_KERNELS", "RNNT_LOSS_LARGEV_KERNELS")


@pytest.fixture(params=FAMILIES, ids=("smallv", "largev"))
def family(request, monkeypatch):
    """large_vocab() reads the environment at every launch: no reload needed."""
    for k in FAMILIES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(request.param, "1")
    return request.param


# (B, T, U+1, V, blank, t_lens, u_lens, lambda, layout, upstream): upstream list = per-utterance gvec, float = scalar gscale
CASES = [
    (2, 33, 9, 65, 64, [33, 1], [8, 0], 0.5, "bm", [1.3, -0.7]),         # tile edge, blank alone in the partial last tile, u_len 0
    (2, 65, 33, 129, 100, [65, 20], [32, 0], 2.0, "tm", 0.37),           # t_len 20: two whole padded tiles
    (2, 32, 65, 256, 70, [32, 31], [64, 0], 0.01, "bm", [1.0, 0.5]),     # V = 256: the natural large-V switch
    (2, 33, 193, 72, 70, [33, 1], [192, 100], 2.0, "tm", [1.0, -0.5]),   # past grad_sep's LDS table (U+1 <= 159)
    (1, 33, 318, 65, 0, [33], [317], 0.5, "bm", [1.0]),                  # past grad_sepv's whole table: two chunks, 160 + 158
    (1, 31, 512, 129, 128, [31], [511], 0.01, "tm", 0.37),               # the longest transcript
]
IDS = [f"T{c[1]}-U1_{c[2]}-V{c[3]}-lam{c[7]}-{c[8]}" for c in CASES]
SCALE = 1.5


def _problem(B, T, U1, V, blank, seed):
    """fp32 A (B,T,V), C (B,U1,V), bias (V), labels (B,U1-1) that avoid the blank; every row carries the last entry of the vocabulary
    (V-2 when that is the blank) and, where there is one, a non-blank entry of the last, partial 64-entry tile."""
    rng = np.random.default_rng(seed)
    A = (rng.normal(size=(B, T, V)) * SCALE).astype(np.float32)
    C = (rng.normal(size=(B, U1, V)) * SCALE).astype(np.float32)
    bias = (rng.normal(size=V) * 0.1 * SCALE).astype(np.float32)
    others = np.array([v for v in range(V) if v != blank])
    y = others[rng.integers(0, others.size, size=(B, U1 - 1))]
    y[:, 0] = V - 1 if blank != V - 1 else V - 2
    tail = [v for v in range(64 * ((V - 1) // 64), V) if v != blank]
    if U1 > 2 and tail:
        y[:, 1] = tail[len(tail) // 2]
    return A, C, bias, y.astype(np.int32)


def _effective(upstream, B):
    if isinstance(upstream, float):   # gscale * gvec[0] in fp32, as the kernels form it
        return [float(np.float32(upstream) * np.float32(2.0))] * B
    return list(upstream)


@functools.lru_cache(maxsize=None)
def _case(i):
    """Problem and float64 reference of CASES[i]: computed once, shared by both families and every test (treated as read-only)."""
    B, T, U1, V, blank, t_lens, u_lens, lam, layout, upstream = CASES[i]
    A, C, bias, y = _problem(B, T, U1, V, blank, seed=T * 1000 + U1 * 10 + V)
    ref = fr.fastemit_fused(A, C, bias, y, t_lens, u_lens, blank, lam, _effective(upstream, B))
    return (A, C, bias, y), ref


def _run(A, C, bias, y, t_lens, u_lens, blank, layout, upstream, lam, split=True):
    """-> nll (B,), dA (B,T,V), dC (B,U1,V) from the library.  lam = None: the entries without FastEmit; a number: the _fastemit
    entries.  upstream: a list (per-utterance gvec, stride 1) or a float (gscale, with a one-element gvec [2.0] of stride 0).
    split: the forward call, then the backward call; else one fwd_bwd call (gscale 1)."""
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import _addr
    L = _lib.lib()
    B, T, V = A.shape
    U1 = C.shape[1]
    if layout == "tm":   # what JointLossFn passes: (T,B,V) and (U1,B,V)
        a = torch.from_numpy(A).transpose(0, 1).contiguous().cuda()
        c = torch.from_numpy(C).transpose(0, 1).contiguous().cuda()
        (a_sb, a_st), (c_sb, c_su) = (V, B * V), (V, B * V)
    else:
        a, c = torch.from_numpy(A).cuda(), torch.from_numpy(C).cuda()
        (a_sb, a_st), (c_sb, c_su) = (T * V, V), (U1 * V, V)
    tb = torch.from_numpy(bias).cuda()
    yl = torch.from_numpy(y).cuda()
    tl = torch.tensor(t_lens, dtype=torch.int32, device="cuda")
    ul = torch.tensor(u_lens, dtype=torch.int32, device="cuda")
    nll = torch.full((B,), float("nan"), device="cuda")
    dA, dC = torch.full_like(a, float("nan")), torch.full_like(c, float("nan"))
    nws = L.rnnt_hip_joint_loss_workspace_bytes(B, T, U1, V)
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device="cuda")   # all-ones bytes: NaN as fp32 and as fp64
    stream = torch.cuda.current_stream().cuda_stream
    args = (_addr(a), a_sb, a_st, _addr(c), c_sb, c_su, _addr(tb), _addr(yl), _addr(tl), _addr(ul), B, T, U1, V, blank)
    extra = () if lam is None else (float(lam),)
    fwd_bwd = L.rnnt_hip_joint_loss_fwd_bwd if lam is None else L.rnnt_hip_joint_loss_fwd_bwd_fastemit
    bwd = L.rnnt_hip_joint_loss_bwd if lam is None else L.rnnt_hip_joint_loss_bwd_fastemit
    if not split:
        _lib.check(fwd_bwd(*args, 1.0, *extra, _addr(nll), _addr(dA), _addr(dC), _addr(ws), nws, stream), "fwd_bwd")
    else:
        _lib.check(fwd_bwd(*args, 1.0, *extra, _addr(nll), None, None, _addr(ws), nws, stream), "fwd")
        if isinstance(upstream, float):
            gscale, gvec, stride = upstream, torch.tensor([2.0], device="cuda"), 0
        else:
            gscale, gvec, stride = 1.0, torch.tensor(upstream, dtype=torch.float32, device="cuda"), 1
        _lib.check(bwd(*args, gscale, *extra, _addr(gvec), stride, _addr(dA), _addr(dC), _addr(ws), nws, stream), "bwd")
    torch.cuda.synchronize()
    to_bm = (lambda x: x.cpu().numpy().transpose(1, 0, 2)) if layout == "tm" else (lambda x: x.cpu().numpy())
    return nll.cpu().numpy(), to_bm(dA), to_bm(dC)


def _check(got, ref, t_lens, u_lens, lam, what=""):
    nll, dA, dC = got
    ref_nll, ref_dA, ref_dC = ref
    np.testing.assert_allclose(nll, ref_nll, rtol=NLL_RTOL, err_msg=what)
    for name, x, want in (("dA", dA, ref_dA), ("dC", dC, ref_dC)):
        err, bound = np.abs(x - want).max(), GRAD_TOL * (1.0 + lam) * max(1.0, np.abs(want).max())
        print(f"{what} {name}: err {err:.3e} bound {bound:.3e}")
        assert err < bound, f"{what} {name}: err {err} >= {bound}"
    for b, (tb, ub) in enumerate(zip(t_lens, u_lens)):   # exact zeros outside the utterance's lattice
        assert np.all(dA[b, tb:] == 0), f"{what} dA of padded frames of row {b}"
        assert np.all(dC[b, ub + 1:] == 0), f"{what} dC of label positions beyond u_len of row {b}"


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_fused_gradient_matches_restatement(family, case):
    """1. NLL, dA, dC of every kernel form against the restatement; exact zeros outside each utterance's lattice."""
    B, T, U1, V, blank, t_lens, u_lens, lam, layout, upstream = CASES[case]
    (A, C, bias, y), ref = _case(case)
    got = _run(A, C, bias, y, t_lens, u_lens, blank, layout, upstream, lam)
    _check(got, ref, t_lens, u_lens, lam, family)


@pytest.mark.parametrize("split", [False, True], ids=("fwd_bwd", "fwd_then_bwd"))
@pytest.mark.parametrize("case", [0, 2, 4], ids=[IDS[i] for i in (0, 2, 4)])
def test_lambda_zero_is_bitwise_the_entries_without_fastemit(family, case, split):
    """2. lambda = 0 through the new entries: NLL, dA and dC are bit for bit those of the old entries."""
    B, T, U1, V, blank, t_lens, u_lens, _, layout, upstream = CASES[case]
    (A, C, bias, y), _ = _case(case)
    old = _run(A, C, bias, y, t_lens, u_lens, blank, layout, upstream, None, split=split)
    new = _run(A, C, bias, y, t_lens, u_lens, blank, layout, upstream, 0.0, split=split)
    for a, b in zip(old, new):
        assert not np.isnan(a).any() and np.array_equal(a, b)


@pytest.mark.parametrize("case", [0, 1, 2], ids=[IDS[i] for i in (0, 1, 2)])
def test_nll_and_rows_without_labels_do_not_depend_on_lambda(family, case):
    """3. The NLL is bitwise independent of lambda; a row with u_len = 0 (no label transition) has bitwise its lambda = 0 gradient,
    while the rows with labels do change."""
    B, T, U1, V, blank, t_lens, u_lens, lam, layout, upstream = CASES[case]
    (A, C, bias, y), _ = _case(case)
    nll0, dA0, dC0 = _run(A, C, bias, y, t_lens, u_lens, blank, layout, upstream, 0.0)
    nll1, dA1, dC1 = _run(A, C, bias, y, t_lens, u_lens, blank, layout, upstream, lam)
    assert np.array_equal(nll0, nll1)
    assert u_lens[1] == 0 and np.array_equal(dA0[1], dA1[1]) and np.array_equal(dC0[1], dC1[1])
    assert not np.array_equal(dA0[0], dA1[0]) and not np.array_equal(dC0[0], dC1[0])


@pytest.mark.parametrize("T,U1,V,blank", [(33, 9, 65, 64), (65, 200, 72, 0)])
def test_zero_length_row_under_fastemit(family, T, U1, V, blank):
    """4. t_lens[b] = 0 with lambda > 0: nll[b] = +inf, the row's dA and dC are exact zeros, every other row is bitwise what a batch
    without that row computes (and matches the restatement)."""
    B, lam = 3, 0.5
    A, C, bias, y = _problem(B, T, U1, V, blank, seed=U1)
    t_lens, u_lens, gw = [T, 0, T - 7], [U1 - 1, 3, U1 // 2], [1.0, 0.5, -0.8]
    keep = [0, 2]
    kt, ku, kg = ([x[k] for k in keep] for x in (t_lens, u_lens, gw))
    ref = fr.fastemit_fused(A[keep], C[keep], bias, y[keep], kt, ku, blank, lam, kg)
    for layout in ("tm", "bm"):
        nll, dA, dC = _run(A, C, bias, y, t_lens, u_lens, blank, layout, gw, lam)
        assert np.isposinf(nll[1])
        assert np.all(dA[1] == 0) and np.all(dC[1] == 0)
        sub = _run(A[keep], C[keep], bias, y[keep], kt, ku, blank, layout, kg, lam)
        for full, part in zip((nll, dA, dC), sub):
            assert np.array_equal(full[keep], part)
        _check(sub, ref, kt, ku, lam, f"{family} {layout}")


@functools.lru_cache(maxsize=None)
def _dense_problem():
    rng = np.random.default_rng(33)
    B, T, U1, V = 2, 9, 5, 33
    z = (rng.normal(size=(B, T, U1, V)) * SCALE).astype(np.float32)
    y = rng.integers(1, V, size=(B, U1 - 1)).astype(np.int32)
    return z, y, [9, 6], [4, 2]


def _dense_run(z, y, t_lens, u_lens, lam, dtype):
    from rnntransducer_amd.loss import RNNTLoss
    zg = torch.from_numpy(z).to(dtype).cuda().requires_grad_(True)
    nll = RNNTLoss(0, "none", fastemit_lambda=lam)(zg, torch.from_numpy(y).cuda(), torch.tensor(t_lens, dtype=torch.int32, device="cuda"),
                                                   torch.tensor(u_lens, dtype=torch.int32, device="cuda"))
    nll.sum().backward()
    assert zg.grad.dtype == dtype
    return nll.detach().cpu().numpy(), zg.grad.float().cpu().numpy()


@pytest.mark.parametrize("lam", [0.01, 0.5, 2.0])
def test_dense_logits_fp32(lam):
    """5. grad_dense_kernel<float>: against the restatement within 2e-5 (1 + lambda) absolute; per-cell row sums below 1e-5 (1 + lambda);
    exact zeros outside the lattice; the NLL bitwise that of lambda = 0."""
    z, y, t_lens, u_lens = _dense_problem()
    ref_nll, ref_dz = fr.fastemit_loss(z, y, t_lens, u_lens, 0, lam)
    nll, g = _dense_run(z, y, t_lens, u_lens, lam, torch.float32)
    nll0, g0 = _dense_run(z, y, t_lens, u_lens, 0.0, torch.float32)
    np.testing.assert_allclose(nll, ref_nll, rtol=NLL_RTOL)
    assert np.array_equal(nll, nll0) and not np.array_equal(g, g0)
    err, rows = np.abs(g - ref_dz).max(), np.abs(g.astype(np.float64).sum(-1)).max()
    print(f"lambda {lam}: err {err:.3e} row sums {rows:.3e}")
    assert err < DENSE_ATOL * (1.0 + lam)
    assert rows < 1e-5 * (1.0 + lam)
    for b, (tb, ub) in enumerate(zip(t_lens, u_lens)):
        assert np.all(g[b, tb:] == 0) and np.all(g[b, :, ub + 1:] == 0)


@pytest.mark.parametrize("lam", [0.5, 2.0])
@pytest.mark.parametrize("dtype,grad_tol", [(torch.float16, 2e-3), (torch.bfloat16, 1.5e-2)], ids=("f16", "bf16"))
def test_dense_logits_half(dtype, grad_tol, lam):
    """5. grad_dense_kernel<__half | __hip_bfloat16>: the reference runs on the rounded logits; tests/test_gpu_loss.py's half-logit
    bounds times (1 + lambda)."""
    z, y, t_lens, u_lens = _dense_problem()
    zr = torch.from_numpy(z).to(dtype).float().numpy()
    ref_nll, ref_dz = fr.fastemit_loss(zr, y, t_lens, u_lens, 0, lam)
    nll, g = _dense_run(zr, y, t_lens, u_lens, lam, dtype)
    np.testing.assert_allclose(nll, ref_nll, rtol=NLL_RTOL)
    err = np.abs(g - ref_dz).max()
    print(f"{dtype} lambda {lam}: err {err:.3e}")
    assert err < grad_tol * (1.0 + lam)


@functools.lru_cache(maxsize=None)
def _joint_reference():
    """fp64 operands of the JointLossFn test, the materialised logits' FastEmit gradient dz (restatement) and the NLL."""
    B, T, U, V, Oe, Od = 2, 40, 199, 72, 8, 8
    g = torch.Generator().manual_seed(199)
    enc = torch.randn(B, T, Oe, generator=g, dtype=torch.float64)
    dec = torch.randn(B, U + 1, Od, generator=g, dtype=torch.float64)
    W = torch.randn(V, Oe + Od, generator=g, dtype=torch.float64) * 0.3
    bias = torch.randn(V, generator=g, dtype=torch.float64) * 0.1
    y = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
    t_lens, u_lens = [T, 27], [U, 160]
    cat = torch.cat((enc[:, :, None, :].expand(-1, -1, U + 1, -1), dec[:, None, :, :].expand(-1, T, -1, -1)), -1)
    logits = torch.nn.functional.gelu(cat, approximate="tanh") @ W.T + bias
    nll, dz = fr.fastemit_loss(logits.numpy(), y.numpy(), t_lens, u_lens, 0, 0.5)
    return (enc, dec, W, bias, y, t_lens, u_lens), nll, torch.from_numpy(dz)


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_joint_loss_fn_with_fastemit(family, reduction):
    """6. JointLossFn with lambda = 0.5 at U+1 = 200, V = 72 (the shape of test_joint_loss_fn_long_transcripts): d_enc, d_dec,
    d_fc.weight, d_fc.bias against torch-CPU float64 autograd through the materialising joint fed with the restatement's dz."""
    from rnntransducer_amd.ops import JointLossFn
    lam = 0.5
    (enc, dec, W, bias, y, t_lens, u_lens), ref_nll, dz = _joint_reference()
    B, T, U = enc.shape[0], enc.shape[1], dec.shape[1] - 1
    e, d, w, bb = (x.clone().requires_grad_(True) for x in (enc, dec, W, bias))
    cat = torch.cat((e[:, :, None, :].expand(-1, -1, U + 1, -1), d[:, None, :, :].expand(-1, T, -1, -1)), -1)
    logits = torch.nn.functional.gelu(cat, approximate="tanh") @ w.T + bb
    gw = {"none": torch.tensor([0.6, -1.2], dtype=torch.float64), "sum": torch.ones(B, dtype=torch.float64),
          "mean": torch.full((B,), 1.0 / B, dtype=torch.float64)}[reduction]
    logits.backward(dz * gw.view(-1, 1, 1, 1))
    dev = "cuda"
    te = enc.float().transpose(0, 1).contiguous().to(dev).requires_grad_(True)
    td = dec.float().transpose(0, 1).contiguous().to(dev).requires_grad_(True)
    tw = W.float().to(dev).requires_grad_(True)
    tb = bias.float().to(dev).requires_grad_(True)
    out = JointLossFn.apply(te, td, tw, tb, y.to(dev), torch.tensor(t_lens, dtype=torch.int32, device=dev),
                            torch.tensor(u_lens, dtype=torch.int32, device=dev), 0, True, reduction, lam)
    if reduction == "none":
        np.testing.assert_allclose(out.detach().cpu().numpy(), ref_nll, rtol=NLL_RTOL)
        (out * gw.float().to(dev)).sum().backward()
    else:
        want = ref_nll.sum() * (1.0 / B if reduction == "mean" else 1.0)
        assert abs(out.item() - want) < NLL_RTOL * abs(want)
        out.backward()
    for name, got, ref in (("d_enc", te.grad.transpose(0, 1), e.grad), ("d_dec", td.grad.transpose(0, 1), d.grad),
                           ("d_fc.weight", tw.grad, w.grad), ("d_fc.bias", tb.grad, bb.grad)):
        err, bound = (got.double().cpu() - ref).abs().max().item(), GRAD_TOL * (1.0 + lam) * max(1.0, ref.abs().max().item())
        print(f"{reduction} {name}: err {err:.3e} bound {bound:.3e}")
        assert err < bound, f"{name}: {err}"


def test_model_level_knobs_agree():
    """7. JointNet.loss(..., fastemit_lambda) and RNNTransducer.training_step with args.fastemit_lambda on a tiny model: the same
    loss and the same parameter gradients bit for bit; the loss is bitwise that of lambda = 0, the gradients are not."""
    from oracle.rnnt_oracle import make_batch
    from rnntransducer_amd import RNNTransducer
    lam, V = 0.5, 10
    tn = dict(input_size=12, hidden_size=16, output_size=8, num_layers=1, rnn_type="lstm", dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=V, pad_token_id=0, hidden_size=16, output_size=8, num_layers=1, rnn_type="lstm", dropout=0.0)
    batch = make_batch(3, 24, 5, V, n_mels=12, ragged=True, seed=3)
    dev = tuple(x.cuda() if isinstance(x, torch.Tensor) else x for x in batch)

    def grads(via_step, lam_):
        torch.manual_seed(0)
        args = Namespace(move_metrics_to_cpu=False, fastemit_lambda=lam_) if via_step else Namespace(move_metrics_to_cpu=False)
        model = RNNTransducer(dict(pn), dict(tn), dict(num_classes=V), args).cuda().train()
        if via_step:
            loss = model.training_step(dev, 0)["loss"]
        else:
            loss = model.jointnet.loss(dev[0], dev[2], dev[3], dev[5], dev[6], 0, reduction="mean", audio_lengths=dev[1],
                                       fastemit_lambda=lam_)
        loss.backward()
        return loss.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    l_step, g_step = grads(True, lam)
    l_loss, g_loss = grads(False, lam)
    l_zero, g_zero = grads(True, 0.0)
    assert torch.equal(l_step, l_loss) and torch.equal(l_step, l_zero) and torch.isfinite(l_step)
    assert set(g_step) == set(g_loss)
    for k in g_step:
        assert torch.equal(g_step[k], g_loss[k]), k
    assert any(not torch.equal(g_step[k], g_zero[k]) for k in g_step)
    assert not torch.equal(g_step["jointnet.fc.bias"], g_zero["jointnet.fc.bias"])


def test_fastemit_moves_emissions_earlier():
    """8. Direction of the effect.  12 utterances (T = 12, U = 4, V = 6, blank 0) whose logits are free fp32 parameters drawn from a
    seeded normal; 40 plain gradient-descent steps of size 1.0 on RNNTLoss(reduction="sum", fastemit_lambda), from the same start, for
    lambda = 0 and lambda = 1; then the forced alignment of both results.  The sum over all 48 tokens of the aligned frame must be
    smaller with lambda = 1.  In float64 on the CPU (the restatement's gradient and its best path, same draw) the sums are 299 and
    279: a margin of 20 token-frames, no utterance later, 7 of 12 strictly earlier, so fp32 tie-breaks cannot flip the sign."""
    from rnntransducer_amd.loss import RNNTLoss, rnnt_align
    B, T, U, V = 12, 12, 4, 6
    rng = np.random.default_rng(4)
    z0 = torch.from_numpy(rng.normal(size=(B, T, U + 1, V)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(1, V, size=(B, U)).astype(np.int32)).cuda()
    tl = torch.full((B,), T, dtype=torch.int32, device="cuda")
    ul = torch.full((B,), U, dtype=torch.int32, device="cuda")
    total = {}
    for lam in (0.0, 1.0):
        z = z0.clone().requires_grad_(True)
        loss_fn = RNNTLoss(0, "sum", fastemit_lambda=lam)
        for _ in range(40):
            loss_fn(z, y, tl, ul).backward()
            with torch.no_grad():
                z -= z.grad
            z.grad = None
        frames = rnnt_align(z.detach(), y, tl, ul, 0).frames
        assert frames.shape == (B, U) and bool((frames >= 0).all())
        total[lam] = int(frames.sum().item())
    print(f"aligned frame sums: lambda 0 -> {total[0.0]}, lambda 1 -> {total[1.0]}")
    assert total[1.0] < total[0.0]
