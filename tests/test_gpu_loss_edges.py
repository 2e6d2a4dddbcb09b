"""Fused RNN-T loss kernels (csrc/loss.hip: lse_sep / lse_sepv, alphabeta<K>, grad_sep / grad_sepv, reduce_dc) at their edges, through
the C ABI with A, C and bias handed in directly, against the float64 oracle (oracle/rnnt_loss_ref.c) on z = A + C + bias.

Every case runs under both kernel families (RNNT_LOSS_SMALLV_KERNELS=1, RNNT_LOSS_LARGEV_KERNELS=1).  The cases are hand-picked so that
each value of an axis meets both families: frame counts around the 32-frame tile, label positions around the alphabeta<K> switch points
and up to 512 (grad_sep's LDS table ends at U+1 = 159, grad_sepv's whole table at 317), vocabularies around the 64-lane wave, the
128-entry LSE chunk and the 256-entry grad_sepv workgroup, the blank and the labels in other 64-entry tiles than the first and in a
partial last one, per-utterance and scalar upstream gradients, both stride layouts, logit scales from flat to peaked posteriors.
Outputs and workspace start as NaN, so anything a kernel leaves unwritten, or reads without writing, shows."""
import numpy as np
import pytest
import torch

from oracle.rnnt_oracle import rnnt_loss_c

pytestmark = pytest.mark.gpu
NLL_RTOL, GRAD_TOL = 1e-5, 5e-5
FAMILIES = ("RNNT_LOSS_SMALLV_KERNELS", "RNNT_LOSS_LARGEV_KERNELS")


@pytest.fixture(params=FAMILIES, ids=("smallv", "largev"))
def family(request, monkeypatch):
    """large_vocab() reads the environment at every launch: no reload needed."""
    for k in FAMILIES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(request.param, "1")
    return request.param


def _problem(B, T, U1, V, blank, scale, seed):
    """fp32 A (B,T,V), C (B,U1,V), bias (V) and labels (B,U1-1): labels avoid the blank, and every row with room for them carries the
    last entry of the vocabulary (V-2 when that is the blank) and an entry of the last, partial 64-entry tile."""
    rng = np.random.default_rng(seed)
    A = (rng.normal(size=(B, T, V)) * scale).astype(np.float32)
    C = (rng.normal(size=(B, U1, V)) * scale).astype(np.float32)
    bias = (rng.normal(size=V) * 0.1 * scale).astype(np.float32)
    others = np.array([v for v in range(V) if v != blank])
    y = others[rng.integers(0, others.size, size=(B, U1 - 1))]
    last = V - 1 if blank != V - 1 else V - 2
    tail = [v for v in range(64 * ((V - 1) // 64), V) if v != blank]   # entries of the last 64-entry tile
    if U1 > 1:
        y[:, 0] = last
    if U1 > 2 and tail:   # (V = 65 with the blank at 64: the blank is the whole partial tile)
        y[:, 1] = tail[len(tail) // 2]
    return A, C, bias, y.astype(np.int32)


def _reference(A, C, bias, y, t_lens, u_lens, blank, gw):
    z = A.astype(np.float64)[:, :, None, :] + C.astype(np.float64)[:, None, :, :] + bias.astype(np.float64)
    nll, dz = rnnt_loss_c(z, y, t_lens, u_lens, blank)
    g = np.asarray(gw, dtype=np.float64).reshape(-1, 1, 1, 1)
    return nll, (dz * g).sum(2), (dz * g).sum(1)


def _device(A, C, bias, layout):
    """A / C on the device in the given layout and their element strides (over b, over t / u)."""
    B, T, V = A.shape
    U1 = C.shape[1]
    if layout == "tm":   # what JointLossFn passes: (T,B,V) and (U1,B,V)
        a = torch.from_numpy(A).transpose(0, 1).contiguous().cuda()
        c = torch.from_numpy(C).transpose(0, 1).contiguous().cuda()
        return a, (V, B * V), c, (V, B * V)
    a, c = torch.from_numpy(A).cuda(), torch.from_numpy(C).cuda()
    return a, (T * V, V), c, (U1 * V, V)


def _to_bm(x, layout):
    x = x.cpu().numpy()
    return x.transpose(1, 0, 2) if layout == "tm" else x


def _run(A, C, bias, y, t_lens, u_lens, blank, layout, upstream, split=True):
    """-> nll (B,), dA (B,T,V), dC (B,U1,V) from the library.  upstream: a list (per-utterance gvec, stride 1) or a float (gscale, with a
    one-element gvec of stride 0).  split: forward call, then the backward call; else one fwd_bwd call (gscale 1)."""
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import _addr
    L = _lib.lib()
    B, T, V = A.shape
    U1 = C.shape[1]
    a, (a_sb, a_st), c, (c_sb, c_su) = _device(A, C, bias, layout)
    tb = torch.from_numpy(bias).cuda()
    yl = torch.from_numpy(y).cuda() if U1 > 1 else torch.zeros(1, dtype=torch.int32, device="cuda")
    tl = torch.tensor(t_lens, dtype=torch.int32, device="cuda")
    ul = torch.tensor(u_lens, dtype=torch.int32, device="cuda")
    nll = torch.full((B,), float("nan"), device="cuda")
    dA, dC = torch.full_like(a, float("nan")), torch.full_like(c, float("nan"))
    nws = L.rnnt_hip_joint_loss_workspace_bytes(B, T, U1, V)
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device="cuda")   # all-ones bytes: NaN as fp32 and as fp64
    stream = torch.cuda.current_stream().cuda_stream
    args = (_addr(a), a_sb, a_st, _addr(c), c_sb, c_su, _addr(tb), _addr(yl), _addr(tl), _addr(ul), B, T, U1, V, blank)
    if not split:
        _lib.check(L.rnnt_hip_joint_loss_fwd_bwd(*args, 1.0, _addr(nll), _addr(dA), _addr(dC), _addr(ws), nws, stream), "fwd_bwd")
    else:
        _lib.check(L.rnnt_hip_joint_loss_fwd_bwd(*args, 1.0, _addr(nll), None, None, _addr(ws), nws, stream), "fwd")
        if isinstance(upstream, float):
            gscale, gvec, stride = upstream, torch.tensor([2.0], device="cuda"), 0
        else:
            gscale, gvec, stride = 1.0, torch.tensor(upstream, dtype=torch.float32, device="cuda"), 1
        _lib.check(L.rnnt_hip_joint_loss_bwd(*args, gscale, _addr(gvec), stride, _addr(dA), _addr(dC), _addr(ws), nws, stream), "bwd")
    torch.cuda.synchronize()
    return nll.cpu().numpy(), _to_bm(dA, layout), _to_bm(dC, layout)


def _effective(upstream, B):
    if isinstance(upstream, float):   # gscale * gvec[0] in fp32, as the kernels form it
        return [float(np.float32(upstream) * np.float32(2.0))] * B
    return list(upstream)


def _check(nll, dA, dC, ref, t_lens, u_lens, what=""):
    ref_nll, ref_dA, ref_dC = ref
    np.testing.assert_allclose(nll, ref_nll, rtol=NLL_RTOL, err_msg=what)
    for name, got, want in (("dA", dA, ref_dA), ("dC", dC, ref_dC)):
        err = np.abs(got - want).max()
        assert err < GRAD_TOL * max(1.0, np.abs(want).max()), f"{what} {name}: err {err}"
    for b, (tb, ub) in enumerate(zip(t_lens, u_lens)):   # exact zeros outside the utterance's lattice
        assert np.all(dA[b, tb:] == 0), f"{what} dA of padded frames of row {b}"
        assert np.all(dC[b, ub + 1:] == 0), f"{what} dC of label positions beyond u_len of row {b}"


# (B, T, U+1, V, blank, t_lens, u_lens, logit scale, layout, upstream): upstream list = per-utterance gvec, float = scalar gscale
CASES = [
    (1, 1, 1, 2, 0, [1], [0], 0.05, "tm", [1.0]),   # (flat: an NLL near 0 would sit below the fp32 resolution of log p)
    (3, 31, 2, 63, 62, [31, 1, 17], [1, 0, 1], 0.05, "bm", 0.37),
    (2, 32, 8, 64, 0, [32, 32], [7, 3], 1.5, "tm", [0.0, -0.7]),
    (3, 33, 9, 65, 64, [33, 1, 32], [8, 0, 5], 30.0, "bm", [1.3, -0.7, 0.0]),
    (2, 65, 33, 129, 100, [65, 20], [32, 0], 1.5, "tm", 0.37),              # t_len 20: two whole padded tiles
    (2, 33, 64, 255, 254, [33, 1], [63, 10], 30.0, "tm", [-1.0, 2.0]),
    (2, 32, 65, 256, 70, [32, 31], [64, 0], 0.05, "bm", [1.0, 0.5]),
    (2, 31, 128, 257, 0, [31, 9], [127, 50], 1.5, "tm", [0.7, -0.3]),
    (1, 33, 129, 300, 299, [33], [128], 30.0, "bm", 0.37),
    (2, 65, 64, 256, 255, [65, 1], [63, 0], 30.0, "tm", [1.0, 0.0]),
    (2, 33, 193, 72, 70, [33, 1], [192, 100], 1.5, "tm", [1.0, -0.5]),     # past grad_sep's LDS table (U+1 <= 159)
    (2, 32, 257, 63, 0, [32, 17], [256, 0], 0.05, "bm", [0.0, 1.5]),
    (1, 33, 318, 65, 0, [33], [317], 1.5, "bm", [1.0]),                     # past grad_sepv's whole table: two chunks, 160 + 158
    (1, 31, 512, 129, 128, [31], [511], 1.5, "tm", [0.8]),
    (2, 65, 512, 2, 1, [65, 33], [511, 200], 1.5, "bm", 0.37),
    (1, 9, 512, 257, 128, [9], [511], 30.0, "tm", [1.0]),
    (2, 1, 257, 300, 0, [1, 1], [256, 0], 1.5, "tm", [1.0, -2.0]),
]


@pytest.mark.parametrize("B,T,U1,V,blank,t_lens,u_lens,scale,layout,upstream", CASES,
                         ids=[f"T{c[1]}-U1_{c[2]}-V{c[3]}-blank{c[4]}-{c[8]}" for c in CASES])
def test_fused_lattice_matches_oracle(family, B, T, U1, V, blank, t_lens, u_lens, scale, layout, upstream):
    A, C, bias, y = _problem(B, T, U1, V, blank, scale, seed=T * 1000 + U1 * 10 + V)
    ref = _reference(A, C, bias, y, t_lens, u_lens, blank, _effective(upstream, B))
    nll, dA, dC = _run(A, C, bias, y, t_lens, u_lens, blank, layout, upstream)
    _check(nll, dA, dC, ref, t_lens, u_lens, family)


@pytest.mark.parametrize("case", [2, 6, 10, 13, 16])
def test_fwd_bwd_in_one_call_equals_fwd_then_bwd(family, case):
    """fwd_bwd (gscale 1, no gvec) is bitwise the forward call followed by the backward call with gvec = [1.0]."""
    B, T, U1, V, blank, t_lens, u_lens, scale, layout, _ = CASES[case]
    A, C, bias, y = _problem(B, T, U1, V, blank, scale, seed=case)
    one = _run(A, C, bias, y, t_lens, u_lens, blank, layout, None, split=False)
    two = _run(A, C, bias, y, t_lens, u_lens, blank, layout, [1.0] * B)
    for x1, x2 in zip(one, two):
        assert np.array_equal(x1, x2)
    _check(*one, _reference(A, C, bias, y, t_lens, u_lens, blank, [1.0] * B), t_lens, u_lens, family)


@pytest.mark.parametrize("T,U1,V,blank", [(33, 9, 65, 64), (65, 200, 72, 0), (31, 20, 300, 299)])
def test_zero_length_row(family, T, U1, V, blank):
    """t_lens[b] = 0 (include/rnnt_hip.h): nll[b] = +inf, the row's dA and dC are exact zeros, and every other row is bitwise what a
    batch without that row computes."""
    B = 3
    A, C, bias, y = _problem(B, T, U1, V, blank, 1.5, seed=U1)
    t_lens, u_lens, gw = [T, 0, T - 7], [U1 - 1, 3, U1 // 2], [1.0, 0.5, -0.8]
    keep = [0, 2]
    for layout in ("tm", "bm"):
        nll, dA, dC = _run(A, C, bias, y, t_lens, u_lens, blank, layout, gw)
        assert np.isposinf(nll[1])
        assert np.all(dA[1] == 0) and np.all(dC[1] == 0)
        sub = _run(A[keep], C[keep], bias, y[keep], [t_lens[k] for k in keep], [u_lens[k] for k in keep], blank, layout,
                   [gw[k] for k in keep])
        for full, part in zip((nll, dA, dC), sub):
            assert np.array_equal(full[keep], part)
        ref = _reference(A[keep], C[keep], bias, y[keep], [t_lens[k] for k in keep], [u_lens[k] for k in keep], blank,
                         [gw[k] for k in keep])
        _check(*sub, ref, [t_lens[k] for k in keep], [u_lens[k] for k in keep], f"{family} {layout}")


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_joint_loss_fn_long_transcripts(family, reduction):
    """JointLossFn at U+1 = 200, V = 72 (past grad_sep's LDS table): forward and backward against torch-CPU float64 autograd through
    the materialising joint + the oracle's loss gradient, as test_gpu_loss.py::test_fused_joint_loss_matches_oracle does."""
    from rnntransducer_amd.ops import JointLossFn
    B, T, U, V, Oe, Od = 2, 40, 199, 72, 8, 8
    g = torch.Generator().manual_seed(199)
    enc = torch.randn(B, T, Oe, generator=g, dtype=torch.float64)
    dec = torch.randn(B, U + 1, Od, generator=g, dtype=torch.float64)
    W = torch.randn(V, Oe + Od, generator=g, dtype=torch.float64) * 0.3
    bias = torch.randn(V, generator=g, dtype=torch.float64) * 0.1
    y = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
    t_lens, u_lens = [T, 27], [U, 160]
    e, d, w, bb = (x.clone().requires_grad_(True) for x in (enc, dec, W, bias))
    cat = torch.cat((e[:, :, None, :].expand(-1, -1, U + 1, -1), d[:, None, :, :].expand(-1, T, -1, -1)), -1)
    logits = torch.nn.functional.gelu(cat, approximate="tanh") @ w.T + bb
    ref_nll, dlog = rnnt_loss_c(logits.detach().numpy(), y.numpy(), t_lens, u_lens, 0)
    gw = {"none": torch.tensor([0.6, -1.2], dtype=torch.float64), "sum": torch.ones(B, dtype=torch.float64),
          "mean": torch.full((B,), 1.0 / B, dtype=torch.float64)}[reduction]
    logits.backward(torch.from_numpy(dlog) * gw.view(-1, 1, 1, 1))
    dev = "cuda"
    te = enc.float().transpose(0, 1).contiguous().to(dev).requires_grad_(True)
    td = dec.float().transpose(0, 1).contiguous().to(dev).requires_grad_(True)
    tw = W.float().to(dev).requires_grad_(True)
    tb = bias.float().to(dev).requires_grad_(True)
    out = JointLossFn.apply(te, td, tw, tb, y.to(dev), torch.tensor(t_lens, dtype=torch.int32, device=dev),
                            torch.tensor(u_lens, dtype=torch.int32, device=dev), 0, True, reduction)
    if reduction == "none":
        np.testing.assert_allclose(out.detach().cpu().numpy(), ref_nll, rtol=NLL_RTOL)
        (out * gw.float().to(dev)).sum().backward()
    else:
        want = ref_nll.sum() * (1.0 / B if reduction == "mean" else 1.0)
        assert abs(out.item() - want) < NLL_RTOL * abs(want)
        out.backward()
    for name, got, ref in (("d_enc", te.grad.transpose(0, 1), e.grad), ("d_dec", td.grad.transpose(0, 1), d.grad),
                           ("d_fc.weight", tw.grad, w.grad), ("d_fc.bias", tb.grad, bb.grad)):
        err = (got.double().cpu() - ref).abs().max().item()
        assert err < GRAD_TOL * max(1.0, ref.abs().max().item()), f"{name}: {err}"
