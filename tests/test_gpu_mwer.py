"""The MWER kernels on the GPU (csrc/mwer.hip) and the grouped loss (ops.JointLossGroupedFn): the edit distance against
metrics.edit_distance (exact), the n-best packing against a plain-Python packing of the search's host result (exact), the risk
against the float64 restatement (tests/mwer_restatement.py), the grouped loss against JointLossFn on repeated encoder rows (NLL
bits) and against float64 autograd (gradients, tests/test_gpu_loss_edges.py's tolerances)."""
import math

import numpy as np
import pytest
import torch

from rnntransducer_amd.metrics import edit_distance
from tests.mwer_restatement import risk_batch

pytestmark = pytest.mark.gpu
NLL_RTOL, GRAD_TOL = 1e-5, 5e-5          # tests/test_gpu_loss_edges.py
EDGE_LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 511]
GARBAGE = 0x7FFFFFFF


# edit distance ----------------------------------------------------------------------------------------------------------------------
def _rows(seqs, ld):
    """Sequences -> (len(seqs), ld) int32 rows with garbage behind every length, and the lengths."""
    out = np.full((len(seqs), ld), GARBAGE, dtype=np.int32)
    for i, s in enumerate(seqs):
        out[i, :len(s)] = s
    return torch.from_numpy(out).cuda(), torch.tensor([len(s) for s in seqs], dtype=torch.int32, device="cuda")


def _pairs():
    """Every pair of edge lengths over alphabets of 2 and 50 symbols, then identical pairs and pairs without a common symbol."""
    g = np.random.default_rng(7)
    hyps, refs = [], []
    for alphabet in (2, 50):
        for lh in EDGE_LENGTHS:
            for lr in EDGE_LENGTHS:
                hyps.append(g.integers(1, alphabet + 1, lh).tolist())
                refs.append(g.integers(1, alphabet + 1, lr).tolist())
    for n in EDGE_LENGTHS:
        s = g.integers(1, 51, n).tolist()
        hyps += [s, s]
        refs += [list(s), [x + 50 for x in s[:max(n - 3, 0)]]]
    return hyps, refs


@pytest.fixture(scope="module")
def pairs():
    hyps, refs = _pairs()
    return hyps, refs, [edit_distance(h, r) for h, r in zip(hyps, refs)]


def test_edit_distance_every_pair_of_edge_lengths_in_one_launch(pairs):
    from rnntransducer_amd import ops
    hyps, refs, want = pairs
    hyp, hl = _rows(hyps, 511)
    ref, rl = _rows(refs, 511)
    got = ops.edit_distance(hyp, hl, ref, rl)
    assert got.dtype == torch.int32 and got.tolist() == want
    assert ops.edit_distance(hyp, hl, ref, rl).tolist() == want
    for p in (0, 17, 80, 161, len(hyps) - 1):   # a pair alone, in rows cut to its own lengths' width
        h1, hl1 = _rows([hyps[p]], max(len(hyps[p]), 1))
        r1, rl1 = _rows([refs[p]], max(len(refs[p]), 1))
        assert ops.edit_distance(h1, hl1, r1, rl1).tolist() == [want[p]]


def test_edit_distance_shared_references():
    from rnntransducer_amd import ops
    g = np.random.default_rng(11)
    refs = [g.integers(1, 6, n).tolist() for n in (9, 0, 64, 33)]
    hyps = [g.integers(1, 6, n).tolist() for n in (8, 9, 0, 12, 1, 0, 3, 2, 65, 64, 63, 7, 33, 30, 36, 1)]
    hyp, hl = _rows(hyps, 70)
    ref, rl = _rows(refs, 64)
    got4 = ops.edit_distance(hyp, hl, ref, rl, ref_div=4).tolist()
    assert got4 == [edit_distance(h, refs[p // 4]) for p, h in enumerate(hyps)]
    ref1, rl1 = _rows([refs[p // 4] for p in range(16)], 64)
    assert ops.edit_distance(hyp, hl, ref1, rl1, ref_div=1).tolist() == got4
    empty = torch.zeros(16, 0, dtype=torch.int32, device="cuda")                  # a batch of empty hypotheses
    assert ops.edit_distance(empty, torch.zeros(16, dtype=torch.int32, device="cuda"), ref, rl, 4).tolist() == [
        len(refs[p // 4]) for p in range(16)]


# pack -------------------------------------------------------------------------------------------------------------------------------
def test_pack_equals_a_python_packing_of_the_host_result():
    """B = 3, N = 4 on a tiny model whose bias is peaked on the blank and one token, searched with a token_min_logp that only
    those two reach: the utterance with T = 1 ends with 2 < N hypotheses, the longer ones return hypotheses of different
    lengths (fewer than N too: equal sequences merge), and max_hyp_len = 2 invalidates the longest of them."""
    from rnntransducer_amd import ops
    from tests import beam_sync_cases as K
    from tests.test_gpu_beam_sync import _encode, _jointnet
    V, N, S, lens, blank, max_hyp_len = 5, 4, 1, [5, 1, 4], 0, 2
    ora, tn, pn = K.model(V, 8, 1, "lstm", 8, 3, scale=1.0)
    with torch.no_grad():
        ora.fc.bias[[0, 1]] += 20.0
    net = _jointnet(tn, pn, V, ora)
    enc = _encode(net, K.audio(max(lens), 3, B=3), lens)
    t_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    dec = net.decoder
    args = (enc, net.fc.weight, net.fc.bias, dec.embedding.weight, dec.rnn.flat_weights(), dec.rnn.CELL, dec.out_proj.weight,
            dec.out_proj.bias, blank, N, S, t_lens)
    host_hyps = ops.beam_search_sync(*args, token_min_logp=-10.0)
    tokens, dlens, counts, _, host = ops.beam_search_sync_device(*args, token_min_logp=-10.0)
    assert [len(h) for h in host_hyps] == counts.tolist() and counts.tolist()[1] == 2 and min(counts.tolist()) >= 2
    assert max(len(y) - 1 for y, _ in host_hyps[0]) > max_hyp_len               # a hypothesis the cap invalidates
    Umax = ops.nbest_umax(host, 3, N, max_hyp_len)
    texts, labels, u_lens, t_rows, valid = ops.nbest_pack(tokens, dlens, counts, t_lens, Umax, blank, max_hyp_len)
    want = dict(texts=[], labels=[], u=[], t=[], valid=[])
    for b, hyps in enumerate(host_hyps):
        for n in range(N):
            y = hyps[n][0][1:] if n < len(hyps) else None
            ok = y is not None and len(y) <= max_hyp_len
            y = y if ok else []
            want["texts"].append([blank] + y + [blank] * (Umax - len(y)))
            want["labels"].append(y + [blank] * (Umax - len(y)))
            want["u"].append(len(y))
            want["t"].append(lens[b] if ok else 0)
            want["valid"].append(int(ok))
    assert Umax == 2 and want["valid"].count(0) >= 3 and 0 in want["valid"][:4] and want["valid"][4:8] == [1, 1, 0, 0]
    assert sorted(set(want["u"])) == [0, 1, 2]
    assert texts.dtype == torch.int64 and texts.tolist() == want["texts"]
    assert labels.dtype == torch.int32 and labels.tolist() == want["labels"]
    assert (u_lens.tolist(), t_rows.tolist(), valid.tolist()) == (want["u"], want["t"], want["valid"])
    # without the cap every returned hypothesis is valid and Umax is the longest of them
    full = ops.nbest_umax(host, 3, N)
    assert full == max(len(y) - 1 for h in host_hyps for y, _ in h) > max_hyp_len
    texts2, _, u2, _, valid2 = ops.nbest_pack(tokens, dlens, counts, t_lens, full, blank)
    assert valid2.tolist() == [int(n < len(h)) for h in host_hyps for n in range(N)] and texts2.shape == (12, full + 1)
    assert u2.tolist() == [len(h[n][0]) - 1 if n < len(h) else 0 for h in host_hyps for n in range(N)]


# risk -------------------------------------------------------------------------------------------------------------------------------
def _risk_case(N, seed=0):
    """Counts 0..N as prefixes, scattered masks, and the edge rows of the CPU tests: (nll fp32, W int32, valid int32), (B, N)."""
    g = np.random.default_rng(100 + N + seed)
    rows = []
    for count in range(N + 1):
        rows.append((g.uniform(1.0, 20.0, N), g.integers(0, 31, N), np.arange(N) < count))
    for _ in range(3):                                         # valid rows anywhere
        rows.append((g.uniform(1.0, 6.0, N), g.integers(0, 12, N), g.random(N) < 0.6))
    base = g.integers(64, 256, N) / 64.0                       # multiples of 1/64 in [1, 4): base + 512 is exact in fp32
    W = g.integers(0, 9, N)
    rows.append((base, W, np.ones(N, bool)))
    rows.append((base + 512.0, W, np.ones(N, bool)))           # a constant added to every nll (exact in fp32)
    rows.append((base, np.full(N, 4), np.ones(N, bool)))       # equal W
    gap = base.copy()
    gap[N // 2] += 800.0                                       # an nll gap of 800
    rows.append((gap, W, np.ones(N, bool)))
    nll = np.stack([r[0] for r in rows]).astype(np.float32)
    valid = np.stack([r[2] for r in rows])
    nll[~valid] = np.inf                                       # what the loss returns for an invalid row
    return nll, np.stack([r[1] for r in rows]).astype(np.int32), valid.astype(np.int32)


def _risk(nll, W, valid, N, reduction="none"):
    from rnntransducer_amd import ops
    x = torch.from_numpy(nll.reshape(-1)).cuda().requires_grad_()
    out = ops.MwerRiskFn.apply(x, torch.from_numpy(W.reshape(-1)).cuda(), torch.from_numpy(valid.reshape(-1)).cuda(), N, reduction)
    return x, out


@pytest.mark.parametrize("N", [1, 2, 4, 5, 64])
def test_risk_and_weights_match_the_restatement(N):
    nll, W, valid = _risk_case(N)
    B = nll.shape[0]
    want_r, want_w = risk_batch(nll, W, valid)                 # float64, from the same fp32 inputs
    x, risk = _risk(nll, W, valid, N)
    risk.backward(torch.ones(B, device="cuda"))
    got_r, got_w = risk.detach().cpu().numpy().astype(np.float64), x.grad.cpu().numpy().astype(np.float64).reshape(B, N)
    assert risk.dtype == torch.float32 and np.isfinite(got_r).all() and np.isfinite(got_w).all()
    # fp32 rounding of the returned value: one ulp, relative 2^-23; the fp64 sums inside differ by orders less
    assert (np.abs(got_r - want_r) <= 2.0 ** -23 * np.abs(want_r) + 1e-12).all(), (got_r, want_r)
    scale = np.abs(want_w).max(axis=1, keepdims=True)
    assert (np.abs(got_w - want_w) <= 1e-6 * scale).all()
    assert (got_w[valid == 0] == 0).all() and (got_w[valid.sum(1) < 2] == 0).all() and (got_r[valid.sum(1) < 2] == 0).all()
    if N >= 2:
        assert np.abs(want_r).max() > 0.1 and np.abs(want_w).max() > 1e-2   # the case is not the trivial one
        k = B - 4                                                           # the edge rows
        assert got_r[k] == got_r[k + 1] and (got_w[k] == got_w[k + 1]).all()   # shift invariance, exact here: the shift is exact in fp32
        assert got_r[k + 2] == 0 and (got_w[k + 2] == 0).all()
        assert got_w[k + 3, N // 2] == 0
    # twice the same bits; a row alone the bits it has in the batch
    x2, risk2 = _risk(nll, W, valid, N)
    risk2.backward(torch.ones(B, device="cuda"))
    assert torch.equal(risk2, risk) and torch.equal(x2.grad, x.grad)
    for b in (0, N, B - 1):
        xa, ra = _risk(nll[b:b + 1], W[b:b + 1], valid[b:b + 1], N)
        ra.backward(torch.ones(1, device="cuda"))
        assert torch.equal(ra.detach(), risk.detach()[b:b + 1]) and torch.equal(xa.grad, x.grad.view(B, N)[b])


def test_risk_reductions_and_upstream_gradients():
    N = 4
    nll, W, valid = _risk_case(N)
    B = nll.shape[0]
    _, none = _risk(nll, W, valid, N)
    x0, r0 = _risk(nll, W, valid, N)
    r0.backward(torch.ones(B, device="cuda"))
    gvec = torch.linspace(-1.0, 2.0, B, device="cuda")
    x1, r1 = _risk(nll, W, valid, N)
    r1.backward(gvec)
    assert torch.equal(x1.grad.view(B, N), x0.grad.view(B, N) * gvec[:, None])
    for reduction, scale in (("sum", 1.0), ("mean", 1.0 / B)):
        xs, rs = _risk(nll, W, valid, N, reduction)
        (rs * 3.0).backward()
        assert rs.dim() == 0 and abs(rs.item() - none.double().sum().item() * scale) <= 1e-6 * none.abs().sum().item()
        assert torch.allclose(xs.grad, x0.grad * (3.0 * scale), rtol=1e-6, atol=0)


# grouped loss -----------------------------------------------------------------------------------------------------------------------
def _grouped_problem():
    T, B, G, U1, V, Oe, Od = 37, 3, 3, 6, 70, 24, 16
    g = torch.Generator().manual_seed(5)
    enc, dec = torch.randn(T, B, Oe, generator=g), torch.randn(U1, B * G, Od, generator=g)
    W, bias = torch.randn(V, Oe + Od, generator=g) * 0.3, torch.randn(V, generator=g) * 0.1
    labels = torch.randint(1, V, (B * G, U1 - 1), generator=g, dtype=torch.int32)
    t_lens = torch.tensor([37, 37, 0, 20, 20, 20, 33, 0, 33], dtype=torch.int32)     # 0: an invalid row
    u_lens = torch.tensor([5, 0, 0, 3, 5, 1, 2, 0, 4], dtype=torch.int32)
    gvec = torch.tensor([0.7, -0.2, 0.0, 1.0, 0.4, -0.9, 0.05, 0.0, 0.3])
    return (T, B, G, U1, V, Oe, Od), enc, dec, W, bias, labels, t_lens, u_lens, gvec


def _grouped_reference(dims, enc, dec, W, bias, labels, t_lens, u_lens, gvec):
    """float64 autograd through the materialised joint and the oracle's loss, on the rows that have frames."""
    import torch.nn.functional as F
    from oracle.rnnt_oracle import _RNNTLossFn
    T, B, G, U1, V, Oe, Od = dims
    e, d, w, b = (x.double().requires_grad_() for x in (enc, dec, W, bias))
    live = torch.nonzero(t_lens > 0).view(-1)
    A = F.gelu(e, approximate="tanh") @ w[:, :Oe].T                      # (T, B, V)
    Cm = F.gelu(d, approximate="tanh") @ w[:, Oe:].T                      # (U1, B*G, V)
    z = A[:, live // G].permute(1, 0, 2)[:, :, None, :] + Cm[:, live].permute(1, 0, 2)[:, None, :, :] + b
    nll = _RNNTLossFn.apply(z, labels[live], t_lens[live], u_lens[live], 0)
    (nll * gvec.double()[live]).sum().backward()
    full = torch.full((B * G,), math.inf, dtype=torch.float64)
    full[live] = nll.detach()
    return full, (e.grad, d.grad, w.grad, b.grad)


def test_grouped_loss_is_the_loss_on_repeated_encoder_rows():
    from rnntransducer_amd import ops
    dims, enc, dec, W, bias, labels, t_lens, u_lens, gvec = _grouped_problem()
    G = dims[2]
    want_nll, want_grads = _grouped_reference(dims, enc, dec, W, bias, labels, t_lens, u_lens, gvec)
    dev = lambda *xs: [x.cuda() for x in xs]   # noqa: E731
    lab, tl, ul, gv = dev(labels, t_lens, u_lens, gvec)

    def run(grouped):
        e, d, w, b = (x.cuda().requires_grad_() for x in (enc, dec, W, bias))
        if grouped:
            nll = ops.JointLossGroupedFn.apply(e, d, w, b, lab, tl, ul, 0, G, True)
        else:
            rep = e.repeat_interleave(G, dim=1)
            nll = ops.JointLossFn.apply(rep, d, w, b, lab, tl, ul, 0, True, "none", 0.0)
        nll.backward(gv)
        return nll.detach(), [x.grad for x in (e, d, w, b)]
    nll, grads = run(True)
    plain_nll, plain_grads = run(False)
    assert torch.equal(nll, plain_nll)                                         # the NLL bits of the ungrouped loss
    live = (t_lens > 0).numpy()
    got = nll.double().cpu().numpy()
    assert np.isinf(got[~live]).all() and (got[~live] > 0).all()
    np.testing.assert_allclose(got[live], want_nll.numpy()[live], rtol=NLL_RTOL)
    for name, g, p, want in zip(("d_enc", "d_dec", "dW", "db"), grads, plain_grads, want_grads):
        for what, x in (("grouped", g), ("ungrouped", p)):
            err = (x.double().cpu() - want).abs().max().item()
            print(f"{name} {what}: err {err:.3g}, |want|max {want.abs().max().item():.3g}")
            assert err < GRAD_TOL * max(1.0, want.abs().max().item()), (name, what, err)
    assert torch.equal(grads[1], plain_grads[1])                               # dC never meets the group sum
    dead = torch.nonzero(t_lens == 0).view(-1)
    assert bool((grads[1][:, dead] == 0).all())                               # exact zeros for the invalid rows
    nll2, grads2 = run(True)                                                   # bitwise reproducible
    assert torch.equal(nll2, nll) and all(torch.equal(a, b) for a, b in zip(grads2, grads))
    with torch.no_grad():                                                      # without a graph nothing is kept
        e, d, w, b = dev(enc, dec, W, bias)
        assert torch.equal(ops.JointLossGroupedFn.apply(e, d, w, b, lab, tl, ul, 0, G, False), nll)
