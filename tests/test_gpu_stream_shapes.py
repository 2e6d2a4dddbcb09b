"""The streaming encoder kernels of csrc/stream.hip (stream_rnn_step_kernel<G>, stream_state_out_kernel, stream_gemm_kernel)
driven through ops.stream_rnn_chunk alone, at the sizes where their code changes path: feature widths that take the scalar
staging path and leave lanes of gate_dots without an element, hidden sizes off 16 and 64, O / V around the 64-wide tile and the
K tail of both products, stream counts around the groups per pass, T * B around the M tile, fewer frames than layers, strided
chunks, both output layouts and chunkings of 1 and 2 frames.

The reference is a float64 torch.nn.LSTM / GRU / RNN (+ an out_proj Linear) run per stream over that stream's valid frames.
Its parameters are created in fp32, so the device holds exactly the reference's numbers.  Every padded frame of a chunk is NaN,
and every buffer the entry writes (out, A, its workspace) holds NaN before the call."""
import contextlib
import math

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

FWD_ATOL = 2e-5   # the project's forward tolerance against float64 (tests/test_gpu_stream.py, tests/test_gpu_lstm.py)
U32 = 2.0 ** -24  # unit roundoff of fp32
CELLS = {"lstm": 0, "gru": 1, "rnn-tanh": 2, "rnn-relu": 3}   # _lib.CELL_*
ALL_CELLS = list(CELLS)
NAN = float("nan")


def _modules(cell, F, H, L, O, V, ld_fc, seed):
    """float64 (rnn, out_proj, fc) whose parameters are fp32 numbers; fc reads ld_fc >= O columns as the model's joint does
    (its first O columns are the encoder half)."""
    torch.manual_seed(seed)
    if cell == "lstm":
        rnn = nn.LSTM(F, H, L, batch_first=True)
    elif cell == "gru":
        rnn = nn.GRU(F, H, L, batch_first=True)
    else:
        rnn = nn.RNN(F, H, L, nonlinearity=cell.split("-")[1], batch_first=True)
    return rnn.double(), nn.Linear(H, O).double(), nn.Linear(ld_fc, V).double()


def _flat(rnn, L):
    return [getattr(rnn, f"{n}_l{l}").detach().float().cuda() for l in range(L) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def _mixed_lens(B, T):
    """Lengths 0, 1 and T mixed (and one in between), stream 0 full."""
    return [(T, 1, 0, (T + 1) // 2)[b % 4] for b in range(B)]


@contextlib.contextmanager
def _poisoned_empty():
    """torch.empty hands out NaN (0xFF bytes for integers) while the entry allocates A and its workspace."""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        return t.fill_(NAN) if t.is_floating_point() else t.fill_(255)
    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


class Case:
    """One problem: modules, fp32 inputs with NaN padding, a start state, and the float64 reference computed once."""

    def __init__(self, cell, F, H, L, O, V, B, T, lens=None, ld_fc=None, seed=0):
        self.cell, self.F, self.H, self.L, self.O, self.V, self.B, self.T = cell, F, H, L, O, V, B, T
        self.lens = list(lens) if lens is not None else _mixed_lens(B, T)
        self.ld_fc = ld_fc or O
        self.rnn, self.out_proj, self.fc = _modules(cell, F, H, L, O, V, self.ld_fc, seed + 7 * F + 11 * H + 13 * O + B + T)
        g = torch.Generator().manual_seed(seed + 1)
        self.x = torch.randn(B, T, F, generator=g)
        self.h0 = 0.5 * torch.randn(L, B, H, generator=g)
        self.c0 = 0.5 * torch.randn(L, B, H, generator=g) if cell == "lstm" else None
        self.weights = _flat(self.rnn, L)
        self.dev = [p.detach().float().cuda() for p in (self.out_proj.weight, self.out_proj.bias, self.fc.weight, self.fc.bias)]
        self._ref = None

    def reference(self):
        """(out (B,T,O) with zeros past lens, h (L,B,H), c) in float64: the module per stream (streams of one length together)."""
        if self._ref is None:
            out = torch.zeros(self.B, self.T, self.O, dtype=torch.float64)
            h, c = self.h0.double().clone(), None if self.c0 is None else self.c0.double().clone()
            with torch.no_grad():
                for n in sorted(set(self.lens) - {0}):
                    idx = [b for b, m in enumerate(self.lens) if m == n]
                    st = h[:, idx].contiguous() if c is None else (h[:, idx].contiguous(), c[:, idx].contiguous())
                    y, st = self.rnn(self.x[idx, :n].double(), st)
                    out[idx, :n] = self.out_proj(y)
                    if c is None:
                        h[:, idx] = st
                    else:
                        h[:, idx], c[:, idx] = st
            self._ref = (out, h, c)
        return self._ref


def _run_chunk(case, x, lens, h, c, layout="dense", out_layout="bt", joint=True):
    """One ops.stream_rnn_chunk call on x (B,T,F) fp32 (CPU; frames past lens become NaN) from state h / c (device, updated in
    place) -> (out (B,T,O), A (B,T,V) or None) on the device."""
    from rnntransducer_amd import ops
    B, T, F = x.shape
    O = case.O
    x = x.clone()
    for b, n in enumerate(lens):
        x[b, n:] = NAN
    if layout == "dense":
        chunk = x.cuda()
    elif layout == "time-major":    # a (T,B,F) buffer viewed (B,T,F)
        chunk = x.transpose(0, 1).contiguous().cuda().transpose(0, 1)
        assert chunk.stride() == (F, B * F, 1)
    else:                           # a slice of a wider feature buffer: row stride > F, start not 16-byte aligned
        wide = torch.full((B, T, F + 7), NAN)
        wide[:, :, 3:3 + F] = x
        chunk = wide.cuda()[:, :, 3:3 + F]
        assert chunk.stride() == (T * (F + 7), F + 7, 1)
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    buf = torch.full((B * T + 1, O), NAN, device="cuda")   # one row more than needed: it must stay NaN
    strides = (T * O, O) if out_layout == "bt" else (O, B * O)
    w_o, b_o, fc_w, fc_b = case.dev
    with _poisoned_empty():
        A = ops.stream_rnn_chunk(chunk, lens_d, case.weights, CELLS[case.cell], h, c, w_o, b_o, buf, strides,
                                 fc_w if joint else None, fc_b if joint else None)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[B * T]).all()), "the row after out was written"
    out = buf[:B * T].view(B, T, O) if out_layout == "bt" else buf[:B * T].view(T, B, O).transpose(0, 1)
    return out, (A.transpose(0, 1) if A is not None else None)


def _run(case, **kw):
    h = case.h0.cuda()
    c = case.c0.cuda() if case.c0 is not None else None
    out, A = _run_chunk(case, case.x, case.lens, h, c, **kw)
    return out, A, h, c


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def _check(case, out, A, h, c):
    """Everything the issue of this file asks of one call's results."""
    B, T, O, lens = case.B, case.T, case.O, case.lens
    want_out, want_h, want_c = case.reference()
    out64, h64 = out.double().cpu(), h.double().cpu()
    assert not bool(torch.isnan(out64).any()) and not bool(torch.isnan(h64).any())
    valid = torch.zeros(B, T, dtype=torch.bool)
    for b, n in enumerate(lens):
        valid[b, :n] = True
    err_out = (out64 - want_out)[valid].abs().max().item() if valid.any() else 0.0
    err_h = (h64 - want_h).abs().max().item()
    err_c = (c.double().cpu() - want_c).abs().max().item() if want_c is not None else 0.0
    print(f"{case.cell} F={case.F} H={case.H} L={case.L} O={O} V={case.V} B={B} T={T}: |out-f64| {err_out:.2e} |h-f64| {err_h:.2e} "
          f"|c-f64| {err_c:.2e}")
    assert err_out < FWD_ATOL and err_h < FWD_ATOL and err_c < FWD_ATOL
    assert bool((out64[~valid] == 0).all()), "padded frames of out are exactly 0"
    idle = [b for b, n in enumerate(lens) if n == 0]
    assert torch.equal(h[:, idle].cpu(), case.h0[:, idle]), "state of a stream with no frames keeps its bits"
    if c is not None:
        assert torch.equal(c[:, idle].cpu(), case.c0[:, idle])
    if A is None:
        return
    # The second product alone: float64 of the device's own out.  Element (m, n) is one k-ordered fmaf chain over O terms, bias
    # added last: |error| <= (O + 1) u S with S = sum_k |gelu(out_k)| |W_nk| + |b_n|, u = 2^-24 (the standard bound of a
    # recursive sum of products).  gelu_tanh in fp32 (five roundings and a tanhf) adds a few ulp to every term: the "+ 8".
    # 8 (O + 8) u S leaves a factor of about 8 over the worst case; nothing in it comes from a run of the kernel.
    g = _gelu64(out64)
    W, bias = case.fc.weight.detach()[:, :O], case.fc.bias.detach()
    want_A = g @ W.t() + bias
    bound = 8 * (O + 8) * U32 * (g.abs() @ W.abs().t() + bias.abs())
    A64 = A.double().cpu()
    assert not bool(torch.isnan(A64).any())
    ratio = ((A64 - want_A).abs() / bound).max().item()
    print(f"    A: worst |A - f64| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    # gelu(0) = 0 and fmaf(0, w, 0) = 0: a padded frame's row is the bias, bitwise (the joint-half launch masks nothing)
    assert torch.equal(A.cpu()[~valid], case.dev[3].cpu().expand(int((~valid).sum()), case.V))


def _run_and_check(case, **kw):
    res = _run(case, **kw)
    _check(case, *res)
    return res


# 1. feature widths: the scalar staging path (F % 4 != 0), K < 64 (lanes without an element), K == 64, one element past ----------
@pytest.mark.parametrize("cell", ALL_CELLS)
@pytest.mark.parametrize("F", [1, 3, 63, 64, 65, 81, 83])
def test_feature_widths(cell, F):
    _run_and_check(Case(cell, F=F, H=8, L=2, O=5, V=7, B=5, T=6))


# 2. hidden sizes: one workgroup, H < 64, H % 16 != 0 (K tail of the out_proj product), H % 64 != 0 ----------------------------
@pytest.mark.parametrize("cell", ALL_CELLS)
@pytest.mark.parametrize("H", [4, 8, 60, 68, 132])
def test_hidden_sizes(cell, H):
    _run_and_check(Case(cell, F=16, H=H, L=3, O=5, V=7, B=5, T=6))


# 3. O and V: the N tile edge of both products and the K tail of the joint half; fc wider than O as the model passes it ---------
@pytest.mark.parametrize("cell", ALL_CELLS)
@pytest.mark.parametrize("O,V,extra", [(1, 130, 0), (15, 65, 3), (17, 64, 16), (63, 63, 0), (65, 1, 9), (17, 1, 0), (65, 130, 64)])
def test_out_and_joint_widths(cell, O, V, extra):
    _run_and_check(Case(cell, F=16, H=20, L=2, O=O, V=V, B=5, T=6, ld_fc=O + extra))


# 4. stream counts around the groups per pass (NB = 64 / (4 G): 4 LSTM, 5 GRU, 16 RNN) and a round of SR_WAVES = 4 groups ---------
@pytest.mark.parametrize("cell,B", [("lstm", B) for B in (1, 3, 4, 5, 16, 17)] + [("gru", B) for B in (4, 5, 6, 20, 21)] +
                         [(c, B) for c in ("rnn-tanh", "rnn-relu") for B in (15, 16, 17, 64, 65)])
def test_stream_counts(cell, B):
    T = 4
    lens = [(0, 1, T)[(b + b // 3) % 3] for b in range(B)]   # 0, 1 and T land on every position of a group
    lens[B - 1] = T                                            # the last stream of the last (partial) group has frames
    _run_and_check(Case(cell, F=5, H=8, L=2, O=5, V=7, B=B, T=T, lens=lens))


# 5. T * B around the 64-row tile of stream_gemm; T = 1; fewer frames than layers (the l_lo / l_hi window of the launches) ------
@pytest.mark.parametrize("cell", ALL_CELLS)
@pytest.mark.parametrize("T,B,L", [(9, 7, 2), (8, 8, 2), (5, 13, 2), (1, 63, 2), (1, 64, 3), (1, 65, 1), (2, 32, 8)])
def test_row_counts(cell, T, B, L):
    _run_and_check(Case(cell, F=6, H=8, L=L, O=17, V=65, B=B, T=T))


# 6. layouts: any chunk strides with unit feature stride, out batch-major and time-major: the dense call's bits -----------------
@pytest.mark.parametrize("cell", ALL_CELLS)
def test_layouts_give_the_dense_bits(cell):
    case = Case(cell, F=13, H=12, L=2, O=9, V=11, B=6, T=5)
    base = _run_and_check(case)
    for kw in (dict(layout="time-major"), dict(layout="wide"), dict(out_layout="tb"), dict(layout="wide", out_layout="tb")):
        got = _run(case, **kw)
        for a, b in zip(got, base):
            assert a is None and b is None or torch.equal(a, b), kw
    out, A, h, c = _run(case, joint=False)   # without the joint half: the same out and state
    assert A is None and torch.equal(out, base[0]) and torch.equal(h, base[2])


# 7. carry: one chunk, chunks of 1 frame, chunks of 2 frames; in a batch and alone ---------------------------------------------
@pytest.mark.parametrize("cell", ALL_CELLS)
@pytest.mark.parametrize("T", [8, 9])   # with chunks of 2 (and a last one of 1 at T = 9) both ring slots end a chunk
def test_chunkings_and_batches_give_the_same_bits(cell, T):
    B = 5
    case = Case(cell, F=83, H=68, L=3, O=17, V=20, B=B, T=T, lens=[T, 5, 0, 1, T - 1])
    base = _run_and_check(case)

    def chunked(rows, step):
        lens = [case.lens[b] for b in rows]
        h = case.h0[:, rows].contiguous().cuda()
        c = case.c0[:, rows].contiguous().cuda() if case.c0 is not None else None
        outs, As = [], []
        for t0 in range(0, T, step):
            n = min(step, T - t0)
            out, A = _run_chunk(case, case.x[rows, t0:t0 + n], [min(max(m - t0, 0), n) for m in lens], h, c)
            outs.append(out)
            As.append(A)
        return torch.cat(outs, 1), torch.cat(As, 1), h, c

    for step in (1, 2):
        got = chunked(list(range(B)), step)
        for a, b in zip(got, base):
            assert a is None and b is None or torch.equal(a, b), step
    for b in (0, 1, 4):   # alone: the bits it has in the batch
        out, A, h, c = chunked([b], T)
        assert torch.equal(out[0], base[0][b]) and torch.equal(A[0], base[1][b]) and torch.equal(h[:, 0], base[2][:, b])
        assert c is None or torch.equal(c[:, 0], base[3][:, b])
