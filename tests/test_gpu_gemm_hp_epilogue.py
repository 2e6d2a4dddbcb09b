"""The epilogue of the 256 x 256 half-pair tile (hp_tile256, csrc/gemm_hp.hip) at its edges: masked rows and columns, unaligned row
starts, every C map and index table, bias, accumulate, the split-K slab, the one-product form, the queue-driven launch.

The epilogue loads the row tables (descale factor and output offset of each row) before the first store of a half tile and stores
through a buffer resource with 32-bit offsets, edge rows and columns masked by an out-of-range offset; where the addressed span of C
does not fit 2 GB it uses 64-bit addresses per row.  What can go wrong there is an offset, a mask, or a table entry of the wrong row, so
every product here is a few tiles at K = 32 or 96 (the split-K one needs 65 K-tiles) and is run through SEVERAL ADDRESSINGS of the same
values, which must agree bitwise:

    dense      C contiguous (c_div = 1, c_so = N)
    view       c_so = N + 1, base one float past a 256-byte boundary: no row start is 16-byte aligned
    rowidx     c_rowidx = 0 .. M-1
    map        c_div = 8, c_so = 8 N, c_si = N: (mo / 8) * 8 N + (mo % 8) * N = mo * N, through the division

Each run asserts
  (a) every element against the fp64 product of the plane values, with the bound of tests/test_gpu_gemm_hp_forms.py
      (2e-6 of sum |a||b| + |bias| + |base|; the one-product form: 1e-5 of sum |hi_a||hi_b| against the product of the hi pieces);
  (b) two runs bitwise equal;
  (c) bitwise equality with the dense addressing of the same product;
  (d) C is filled with a sentinel first: whatever the map does not address (beyond M x N, unlisted rows, the padding between rows)
      keeps it bitwise.
Operands are the CPU-restated planes of tests/test_gpu_gemm_hp_forms.py.  Every case prints its largest error / bound before it asserts.
RNNT_HP_EPILOGUE_DUMP=<dir>: every product is also written there as <name>.npy (tools/gemm_hp_epilogue_parity.py compares two
libraries bytewise).
"""
import os

import pytest
import torch

from tests.test_gpu_gemm_hp_forms import _amax_bits, _bound_and_ref, _planes, _values

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
DEV = "cuda"


def _record(name, t):
    d = os.environ.get("RNNT_HP_EPILOGUE_DUMP")
    if d:
        import numpy as np
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, name + ".npy"), t.contiguous().view(torch.int32).numpy())


class _Operands:
    """A (PR plane rows) and W (N rows) as restated planes on the device; `extreme`: plane row 3 of A has maximum 1e30, row 5 of W 1e-30."""

    def __init__(self, seed, PR, N, K, extreme=False):
        g = torch.Generator().manual_seed(seed)
        self.PR, self.N, self.K, self.g = PR, N, K, g
        self.A, self.W = _values(g, PR, K), torch.randn(N, K, generator=g) * 0.05
        if extreme:
            self.A[3] *= 1e30 / self.A[3].abs().max()
            self.W[5] *= 1e-30 / self.W[5].abs().max()
        self.a_bits, self.b_bits = _amax_bits(self.A, 1), _amax_bits(self.W, 1)
        self.a_pl, self.b_pl = _planes(self.A, self.a_bits), _planes(self.W, self.b_bits)
        self.b_pl_d, self.b_bits_d = self.b_pl.reshape(-1).to(DEV), self.b_bits.to(DEV)

    def a_side(self, used=None):
        """device planes and amax words of A; plane rows outside `used` are 0xFF bytes (NaN halves, an amax word of all ones)."""
        pl, am = self.a_pl, self.a_bits
        if used is not None:
            pl, am = torch.full_like(self.a_pl, 0xFF), torch.full((self.PR,), -1, dtype=torch.int32)
            pl[used], am[used] = self.a_pl[used], self.a_bits[used]
        return pl.reshape(-1).to(DEV), am.to(DEV)


def _launch(op, M, *, aidx=None, cidx_rows=None, c_off=0, c_div=1, c_so=None, c_si=0, c_rows=None, bias=None, base=None, f16=False,
            a_side=None, pad=8):
    """One product of rows `aidx` (None: 0 .. M-1) of op.A into a sentinel-filled buffer, twice.  Returns (buffer as int32 on the CPU,
    flat indices (M, N) of the addressed elements)."""
    from rnntransducer_amd._lib import GEMM_ACCUM, GEMM_HP_F16
    from rnntransducer_amd.ops import gemm_hp_ex
    N, K = op.N, op.K
    c_so = N if c_so is None else c_so
    m = torch.arange(M)
    mo = m if cidx_rows is None else cidx_rows
    at = c_off + ((mo // c_div) * c_so + (mo % c_div) * c_si)[:, None] + torch.arange(N)[None, :]
    size = int(at.max()) + 1 + pad if c_rows is None else c_off + c_rows * c_so + pad
    assert 0 <= int(at.min()) and int(at.max()) < size and at.unique().numel() == M * N
    start = torch.full((size,), SENTINEL, dtype=torch.int32)
    if base is not None:
        start[at.reshape(-1)] = base.reshape(-1).view(torch.int32)
    a_pl_d, a_am_d = a_side if a_side is not None else op.a_side()
    i32 = lambda t: None if t is None else t.to(torch.int32).to(DEV)
    flags = (GEMM_ACCUM if base is not None else 0) | (GEMM_HP_F16 if f16 else 0)
    outs = [start.to(DEV).view(torch.float32), start.to(DEV).view(torch.float32)]
    for out in outs:
        gemm_hp_ex(a_pl_d, a_am_d, op.b_pl_d, op.b_bits_d, M, N, K, out, c_off=c_off, c_div=c_div, c_so=c_so, c_si=c_si,
                   bias=None if bias is None else bias.to(DEV), flags=flags, a_rowidx=i32(aidx), a_plane_rows=op.PR if aidx is not None else 0,
                   c_rowidx=i32(cidx_rows))
    torch.cuda.synchronize()
    o0, o1 = outs[0].cpu().view(torch.int32), outs[1].cpu().view(torch.int32)
    assert torch.equal(o0, o1), "two runs differ"                                                     # (b)
    untouched = torch.ones(size, dtype=torch.bool)
    untouched[at.reshape(-1)] = False
    assert torch.equal(o0[untouched], start[untouched]), "wrote outside the C map"                    # (d)
    return o0, at


def _check(name, op, rows, got_bits, bias, base, f16):
    """(a): got (M, N) as int32 bit patterns against fp64."""
    got = got_bits.view(torch.float32)
    ref, tol = _bound_and_ref(op.A[rows], op.W, op.a_pl[rows], op.a_bits[rows], op.b_pl, op.b_bits, op.K, f16, bias, base)
    err = (got.double() - ref).abs()
    assert not torch.isnan(err).any(), "NaN: an unaddressed plane row was read"
    worst = (err / tol).max().item()
    print(f"{name}: max err / bound {worst:.3g}")
    assert worst <= 1.0, (name, worst)


def _addressings(M, N):
    return [("dense", {}),
            ("view", dict(c_off=1, c_so=N + 1)),
            ("rowidx", dict(cidx_rows=torch.arange(M))),
            ("map", dict(c_div=8, c_so=8 * N, c_si=N))]


# id, (M, N, K), features: bias | accum | f16 | extreme;  plan (tiles_m, tiles_n, group_m, splits, kt_per_split)
PRODUCTS = [
    ("one", (1, 1, 32), "", (1, 1, 4, 1, 1)),                       # one element valid, everything else masked
    ("one-bias-accum", (1, 1, 32), "bias accum", (1, 1, 4, 1, 1)),
    ("remnant", (257, 259, 96), "", (2, 2, 4, 1, 3)),               # 2 x 2 tiles, a one-row and a three-column remnant; N odd
    ("remnant-bias", (257, 259, 96), "bias", (2, 2, 4, 1, 3)),
    ("remnant-accum", (257, 259, 96), "accum", (2, 2, 4, 1, 3)),
    ("remnant-f16", (257, 259, 96), "f16", (2, 2, 4, 1, 3)),
    ("n260", (300, 260, 32), "", (2, 2, 4, 1, 1)),                  # N % 4 == 0, N % 16 != 0: the last 16-column block is partly valid
    ("n260-bias-accum", (300, 260, 32), "bias accum", (2, 2, 4, 1, 1)),
    ("n260-f16", (300, 260, 32), "f16", (2, 2, 4, 1, 1)),
    ("extreme", (257, 259, 96), "extreme bias", (2, 2, 4, 1, 3)),   # 1e30 row against 1e-30 column: (acc * sa) * sb, never sa * sb
    ("split2", (70, 40, 2061), "", (1, 1, 4, 2, 33)),               # slab + reduce
    ("split2-bias-accum", (70, 40, 2061), "bias accum", (1, 1, 4, 2, 33)),
]


@pytest.mark.parametrize("case", PRODUCTS, ids=lambda c: c[0])
def test_product_under_every_addressing(case):
    from rnntransducer_amd.ops import gemm_hp_plan
    name, (M, N, K), feats, want_plan = case
    f = set(feats.split())
    plan = gemm_hp_plan(M, N, K)
    assert tuple(plan[:5]) == want_plan, plan
    assert ("split" in name) == (plan.splits > 1)
    op = _Operands(M * 31 + N * 7 + K, M, N, K, extreme="extreme" in f)
    bias = torch.randn(N, generator=op.g) if "bias" in f else None
    base = torch.randn(M, N, generator=op.g) if "accum" in f else None
    if "extreme" in f:
        assert op.A[3].abs().max().item() > 9e29 and 0 < op.W[5].abs().max().item() < 1.1e-30
    dense = None
    for aname, kw in _addressings(M, N):
        buf, at = _launch(op, M, bias=bias, base=base, f16="f16" in f, **kw)
        got = buf[at]
        _check(f"{name} / {aname} {(M, N, K)}", op, torch.arange(M), got, bias, base, "f16" in f)
        if dense is None:
            dense = got
            _record(name, got)
        assert torch.equal(got, dense), f"{aname} differs from the dense addressing"                  # (c)


@pytest.mark.parametrize("feats", ["", "bias accum", "f16"])
def test_batch_major_map(feats):
    """T = 37 frames x B = 8 utterances, rows time-major (m = t * 8 + b), written batch-major: c_div = 8, c_so = N, c_si = 37 N."""
    T, B, N, K = 37, 8, 70, 32
    M, f = T * B, set(feats.split())
    op = _Operands(296 + len(feats), M, N, K)
    bias = torch.randn(N, generator=op.g) if "bias" in f else None
    base = torch.randn(M, N, generator=op.g) if "accum" in f else None
    dense_buf, dense_at = _launch(op, M, bias=bias, base=base, f16="f16" in f)
    buf, at = _launch(op, M, c_div=B, c_so=N, c_si=T * N, bias=bias, base=base, f16="f16" in f)
    m = torch.arange(M)
    assert torch.equal(at[:, 0], (m % B) * T * N + (m // B) * N)
    got = buf[at]
    _check(f"batch-major [{feats}] {(M, N, K)}", op, m, got, bias, base, "f16" in f)
    _record("batch-major-" + feats.replace(" ", "-"), got)
    assert torch.equal(got, dense_buf[dense_at]), "the batch-major map differs from the dense addressing"
    # the same buffer read batch-major is the (B, T, N) tensor
    assert torch.equal(buf[:M * N].view(B, T, N).transpose(0, 1).reshape(M, N), got)


@pytest.mark.parametrize("feats", ["", "bias", "accum"])
def test_gather_scatter_of_listed_rows(feats):
    """270 rows listed in shuffled order out of 400: plane rows gathered by a_rowidx, output rows scattered by c_rowidx; the 130 unlisted
    rows of C keep the sentinel, the unlisted plane rows are NaN."""
    M, PR, N, K = 270, 400, 130, 96
    f = set(feats.split())
    op = _Operands(270 + len(feats), PR, N, K)
    sub = torch.randperm(PR, generator=op.g)[:M]
    assert not torch.equal(sub, sub.sort().values)
    bias = torch.randn(N, generator=op.g) if "bias" in f else None
    base = torch.randn(M, N, generator=op.g) if "accum" in f else None
    buf, at = _launch(op, M, aidx=sub, cidx_rows=sub, c_rows=PR, bias=bias, base=base, a_side=op.a_side(used=sub))
    got = buf[at]
    _check(f"gather-scatter [{feats}] {(M, N, K)}", op, sub, got, bias, base, False)
    _record("gather-scatter-" + feats, got)
    listed = torch.zeros(PR, dtype=torch.bool)
    listed[sub] = True
    assert bool((buf[:PR * N].view(PR, N)[~listed] == SENTINEL).all()), "an unlisted row was written"
    # the same plane rows, packed, through the plain form
    packed = _Operands.__new__(_Operands)
    packed.__dict__.update(op.__dict__)
    packed.PR, packed.A, packed.a_bits, packed.a_pl = M, op.A[sub], op.a_bits[sub], op.a_pl[sub]
    dbuf, dat = _launch(packed, M, bias=bias, base=base)
    assert torch.equal(got, dbuf[dat]), "differs from the dense product of the same plane rows"


def test_rows_more_than_2_gb_apart():
    """Two output rows 2^29 + 3 floats apart: the span does not fit the 32-bit offsets of the buffer path, the tile takes 64-bit
    addresses per row.  (The buffer is not initialised as a whole: the sentinel surrounds each row.)"""
    from rnntransducer_amd.ops import gemm_hp_ex
    M, N, K, c_so = 2, 37, 32, 2 ** 29 + 3
    op = _Operands(2029, M, N, K)
    a_pl_d, a_am_d = op.a_side()
    dbuf, dat = _launch(op, M)
    big = torch.empty(c_so + N + 64, dtype=torch.int32, device=DEV)
    outs = []
    for _ in range(2):
        big[:N + 64] = SENTINEL
        big[c_so - 64:] = SENTINEL
        gemm_hp_ex(a_pl_d, a_am_d, op.b_pl_d, op.b_bits_d, M, N, K, big.view(torch.float32), c_so=c_so)
        torch.cuda.synchronize()
        outs.append((big[:N + 64].cpu(), big[c_so - 64:].cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two runs differ"
    lo, hi = outs[0]
    got = torch.stack([lo[:N], hi[64:64 + N]])
    _check(f"2 GB apart {(M, N, K)}", op, torch.arange(M), got, None, None, False)
    assert torch.equal(got, dbuf[dat]), "differs from the dense addressing"
    assert bool((lo[N:] == SENTINEL).all()) and bool((hi[:64] == SENTINEL).all()) and bool((hi[64 + N:] == SENTINEL).all())


def test_grouped_launch_of_two_ragged_problems():
    """One queue-driven launch (no XCD skipped) of two problems with ragged edges, one of them a column block of a wider matrix."""
    from rnntransducer_amd.ops import HpTensor, gemm_hp_grouped
    shapes, ldcs, coffs = [(257, 259, 96), (300, 70, 32)], [259, 70 + 5], [0, 3]
    ops_ = [_Operands(500 + i, M, N, K) for i, (M, N, K) in enumerate(shapes)]
    pairs = []
    for op, (M, N, K) in zip(ops_, shapes):
        a, b = HpTensor(M, K, DEV), HpTensor(N, K, DEV)
        a.planes[:op.a_pl.numel()] = op.a_pl.reshape(-1).to(DEV)
        b.planes[:op.b_pl.numel()] = op.b_pl.reshape(-1).to(DEV)
        a.amax[:M], b.amax[:N] = op.a_bits.to(DEV), op.b_bits.to(DEV)
        pairs.append((a, b))
    ats = [co + torch.arange(M)[:, None] * ldc + torch.arange(N)[None, :] for (M, N, K), ldc, co in zip(shapes, ldcs, coffs)]
    starts = [torch.full((int(at.max()) + 9,), SENTINEL, dtype=torch.int32) for at in ats]
    runs = []
    for _ in range(2):
        dev = [s.to(DEV).view(torch.float32) for s in starts]
        views = [d[co:].as_strided((M, N), (ldc, 1)) for d, (M, N, K), ldc, co in zip(dev, shapes, ldcs, coffs)]
        gemm_hp_grouped(pairs, outs=views, check=True, xcd_skip=0x00)
        torch.cuda.synchronize()
        runs.append([d.cpu().view(torch.int32) for d in dev])
    for i, (op, (M, N, K)) in enumerate(zip(ops_, shapes)):
        o0, o1, at = runs[0][i], runs[1][i], ats[i]
        assert torch.equal(o0, o1), f"problem {i}: two runs differ"
        untouched = torch.ones(o0.numel(), dtype=torch.bool)
        untouched[at.reshape(-1)] = False
        assert bool((o0[untouched] == SENTINEL).all()), f"problem {i}: wrote outside its block"
        got = o0[at]
        _check(f"grouped problem {i} {(M, N, K)}", op, torch.arange(M), got, None, None, False)
        _record(f"grouped-{i}", got)
        dbuf, dat = _launch(op, M)
        assert torch.equal(got, dbuf[dat]), f"problem {i}: differs from the single launch"
