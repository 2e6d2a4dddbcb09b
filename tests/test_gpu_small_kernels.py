"""The kernels of csrc/colsum_embedding.hip through their C entries (and ops.colsum), no model around them: embedding forward,
embedding backward (written and accumulated) and the two-stage column sum (written and accumulated).

Shapes come from the kernels' own boundaries.  embedding_bwd_kernel compacts the tokens that hit a vocabulary row in batches of
CAP = 2048 tokens, 256 per ballot round, and keeps 4 x 256 features in registers with one more pass per further 1024 features;
colsum splits the rows into at most 128 chunks of ceil(M / chunks) rows, 64 columns per workgroup.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _lib():
    from rnntransducer_amd import _lib
    return _lib


def _ptr(t):
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------
# rnnt_hip_embedding_fwd
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,H,V", [(7, 33, 9),            # M * H = 231: less than one workgroup, not a multiple of 256
                                   (1001, 257, 5),         # many workgroups, ragged last one
                                   (1100, 1000, 9),        # M * H > 4096 * 256: the grid-stride loop wraps
                                   (0, 16, 5)])            # nothing to do
def test_embedding_fwd_is_a_bitwise_gather_with_zero_rows_for_ids_outside_the_table(M, H, V):
    L = _lib()
    g = torch.Generator().manual_seed(M + H)
    W = torch.randn(V, H, generator=g) * torch.exp(torch.empty(V, 1).uniform_(-20, 20, generator=g))
    idx = torch.randint(0, V, (M,), generator=g)
    if M:
        outside = torch.tensor([-1, V, V + 3, -5, 1 << 40, -(1 << 40)])
        pos = torch.randperm(M, generator=g)[:min(M // 2, len(outside))]
        idx[pos] = outside[:len(pos)]
        idx[M - 1] = V - 1                                                  # the last row of the table, by the last token
    valid = (idx >= 0) & (idx < V)
    want = torch.where(valid[:, None], W[idx.clamp(0, V - 1)], torch.zeros(1, H))
    out = torch.full((M + 1, H), float("nan"), device="cuda")             # one row more than the call may write
    W_d, idx_d = W.cuda(), idx.cuda()                                     # named: the allocations live until the result is read
    L.check(L.lib().rnnt_hip_embedding_fwd(_ptr(W_d), _ptr(idx_d), M, H, V, _ptr(out), _stream()), "embedding_fwd")
    out = out.cpu()
    assert torch.equal(_bits(out[:M]), _bits(want))
    assert torch.isnan(out[M]).all()


# ------------------------------------------------------------------------------------------------------------------
# rnnt_hip_embedding_bwd / _bwd_acc
# ------------------------------------------------------------------------------------------------------------------
PAD, HOT, NEVER = 2, 1, 3      # padding row; the row every token hits in the "one" pattern; a row no pattern hits


def _token_patterns(M, V, g):
    """name -> idx (M) int64"""
    pats = {"one": torch.full((M,), HOT, dtype=torch.int64)}          # M >= 2048: a batch's list[] filled exactly
    pool = torch.tensor([v for v in range(V) if v != NEVER])           # the padding row is in the pool: its tokens are dropped
    rnd = pool[torch.randint(0, len(pool), (M,), generator=g)]
    for m in (0, 255, 256, 2047, 2048, 4095, 4096, M - 1):             # first / last token of a ballot round, of a batch, of the call
        if 0 <= m < M:
            rnd[m] = 4
    pats["random"] = rnd
    out = rnd.clone()
    if M:
        bad = torch.tensor([-1, V, V + 100, -7, 1 << 40])
        pos = torch.randperm(M, generator=g)[:max(M // 3, 1)]
        out[pos] = bad[torch.randint(0, len(bad), (len(pos),), generator=g)]
    pats["outside"] = out                                               # ids outside the table are ignored
    return pats


def _token_order_sum(dE, idx, V):
    """dW[v] = dE rows with idx == v added one at a time in token order, in fp32 — the order the kernel promises."""
    dE, idx = dE.numpy(), idx.numpy()
    dW = np.zeros((V, dE.shape[1]), dtype=np.float32)
    for m in range(len(idx)):
        v = idx[m]
        if 0 <= v < V and v != PAD:
            dW[v] += dE[m]
    return torch.from_numpy(dW)


@pytest.mark.parametrize("H", [1, 72, 256, 1000, 1024, 1025, 2100])
@pytest.mark.parametrize("M", [0, 1, 255, 256, 257, 2047, 2048, 2049, 3872, 4097])
def test_embedding_bwd_is_the_token_order_sum_bitwise(M, H):
    """Both entries, three token patterns.  The kernel adds the rows of dE that hit a vocabulary row one by one in token order into
    fp32 registers (adds only: nothing for the compiler to contract or reassociate), across its 2048-token batches and, for H > 1024,
    once per 1024-feature pass, so the result is bitwise a sequential fp32 sum; _acc adds that sum to what dW held with one more
    add.  The padding row keeps its bits (NaN here) in both entries, a row nothing hits is zero / keeps its base, and a second run
    gives the same bits."""
    L = _lib()
    V = 5 + (M + H) % 5
    g = torch.Generator().manual_seed(M * 7 + H)
    dE = torch.randn(M, H, generator=g) * torch.exp(torch.empty(M, 1).uniform_(-12, 6, generator=g))
    dE_d = dE.cuda()
    for name, idx in _token_patterns(M, V, g).items():
        want = _token_order_sum(dE, idx, V)
        assert torch.all(want[NEVER] == 0) and torch.all(want[PAD] == 0)
        if name == "one" and M:
            assert want[HOT].abs().sum() > 0
        idx_d = idx.cuda()
        base = torch.randn(V, H, generator=g)
        base[PAD] = float("nan")
        zero = torch.zeros(V, H)
        zero[PAD] = float("nan")
        for fn, start, expect in ((L.lib().rnnt_hip_embedding_bwd, zero, want), (L.lib().rnnt_hip_embedding_bwd_acc, base, base + want)):
            got = []
            for _ in range(2):
                dW = start.cuda()
                L.check(fn(_ptr(dE_d), _ptr(idx_d), M, H, V, PAD, _ptr(dW), _stream()), "embedding_bwd")
                got.append(dW.cpu())
            assert torch.equal(_bits(got[0]), _bits(got[1])), (name, "two runs differ")
            assert torch.equal(_bits(got[0][PAD]), _bits(start[PAD])), (name, "padding row touched")
            rows = [v for v in range(V) if v != PAD]
            assert torch.equal(got[0][rows], expect[rows]), (name, (got[0][rows] - expect[rows]).abs().max().item())


# ------------------------------------------------------------------------------------------------------------------
# rnnt_hip_colsum_f32 / _acc
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, 8192, 8193])   # 8192: 128 chunks of 64 rows; 8193: 128 of 65, the last ones partial / empty
def test_colsum_of_a_column_window(M, N):
    """Column sums of an (M, N) window of a wider matrix (ld = N + 7, first column 3: not 16-byte aligned, NaN everywhere outside the
    window), written and accumulated onto a random base; M == 0 gives zeros / the base unchanged; twice the same bits.  Bound: the
    one of test_colsum."""
    from rnntransducer_amd.ops import colsum
    g = torch.Generator().manual_seed(M * 3 + N)
    c0, ld = 3, N + 7
    x = torch.randn(M, N, generator=g) * torch.exp(torch.empty(1, N).uniform_(-6, 3, generator=g))
    wide = torch.full((M, ld), float("nan"))
    wide[:, c0:c0 + N] = x
    X = wide.cuda().view(-1)[c0:]
    ref = x.double().sum(0)
    bound = 1e-5 * max(1.0, x.abs().double().sum(0).max().item() if M else 0.0)
    out, out2 = colsum(X, M, N, ld=ld), colsum(X, M, N, ld=ld)
    assert torch.equal(_bits(out), _bits(out2))
    assert (out.double().cpu() - ref).abs().max().item() <= bound
    base = torch.randn(N + 2, generator=g)
    acc = [base.cuda(), base.cuda()]
    for a in acc:
        assert colsum(X, M, N, ld=ld, into=a[1:N + 1]) is None
    assert torch.equal(_bits(acc[0]), _bits(acc[1]))
    got = acc[0].cpu()
    assert got[0] == base[0] and got[N + 1] == base[N + 1]                 # the neighbours of the (N) destination
    assert (got[1:N + 1].double() - (base[1:N + 1].double() + ref)).abs().max().item() <= bound
    if M == 0:
        assert torch.all(out == 0) and torch.equal(got, base)
