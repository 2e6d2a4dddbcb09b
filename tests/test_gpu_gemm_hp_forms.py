"""Every form of the half-pair kernels (csrc/gemm_hp.hip) with the index tables and C maps a ragged batch runs them with, against a CPU
restatement of the plane format (bitwise) and against float64 products (per element).

The format, restated below in plain torch (_scale, _planes): per row, amax = max |x| as fp32 bits, scale = 2^(14 - e) from the
exponent field eb of amax (eb == 0 -> 1, eb < 15 -> 15), v = x * scale, hi = fp16(v), lo = fp16(v - hi), stored as lines of
32 hi | 32 lo with K padded to 32 by zeros.  Every step is exact or ONE IEEE rounding (a power-of-two multiply, two fp32 -> fp16
roundings to nearest even, one exact fp32 subtraction), so planes and amax words are compared bitwise — f16-subnormal lo values
(about 2e-4 of the elements of such inputs) and fp32-subnormal inputs included.

  (a) test_split_* / test_colmax: every buffer a call writes into is filled with 0x5A bytes first and compared WHOLE: bytes the call
      does not own come back unchanged.  Source elements outside the view are NaN.
  (b) test_product: rnnt_hip_gemm_hp_ex.  Plane rows and amax words the maps do not address are 0xFF bytes (NaN halves), destination
      elements outside the C map hold a sentinel that must come back bit-identical, addressed ones start as NaN unless ACCUM adds
      onto them; the index tensors are checked on the host to lie inside the allocations before any launch.  Each case asserts from
      rnnt_hip_gemm_hp_plan (the function the launch takes its decisions from) the tiles, band height and split it names, runs twice
      (bitwise equal), equals bitwise the dense product of the same plane rows (the arithmetic of a row does not depend on which rows
      surround it), and is compared per element with float64:
          default:        |got - ref| <= 2e-6 * (sum_k |a||b| + |bias| + |base|)       (test_gemm_hp_matches_fp64, test_gpu_gemm_forms)
          RNNT_GEMM_HP_F16: ref = fp64 product of the hi pieces read from the planes,  |got - ref| <= 1e-5 * sum_k |hi_a||hi_b|
                                                                                      (test_gemm_hp_f16_flag_multiplies_the_hi_pieces_only)
      For scale: evaluated in fp64 from the restated planes, the three products kept are within 6.8e-9 .. 1.2e-7 of sum |a||b| at
      these shapes.
  (c) test_grouped_*: the queue-driven launch with ldc > N, a (1, 1, 1) problem, ACCUM per problem, F16, 66 K-tiles and a workspace
      that forces the slabs to shrink.
Every case prints its largest error / bound before it asserts.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, RTOL_F16 = 2e-6, 1e-5
FILL = 0x5A
FILL32 = 0x5A5A5A5A


# ------------------------------------------------------------------------------------------------------------------
# the format, on the CPU
# ------------------------------------------------------------------------------------------------------------------
def _scale(bits):
    """fp32 row scale 2^(14 - e) from amax bit patterns (int32)."""
    eb = (bits.long() >> 23) & 255
    s = ((268 - eb.clamp(min=15)) << 23).to(torch.int32).view(torch.float32)
    return torch.where(eb == 0, torch.ones_like(s), s)


def _inv_scale64(bits):
    eb = (bits.long() >> 23) & 255
    return torch.where(eb == 0, torch.ones(bits.shape, dtype=torch.float64), torch.pow(2.0, (eb.clamp(min=15) - 141).double()))


def _amax_bits(v, dim):
    return (v.contiguous().view(torch.int32) & 0x7FFFFFFF).amax(dim)


def _planes(v, bits):
    """v (R, K) fp32, bits (R,) amax words -> uint8 (R, ceil(K / 32) * 128): the plane rows."""
    R, K = v.shape
    Kp = (K + 31) // 32 * 32
    w = v * _scale(bits)[:, None]
    hi = w.half()
    lo = (w - hi.float()).half()
    pad = torch.zeros(R, Kp - K, dtype=torch.float16)
    hi, lo = torch.cat([hi, pad], 1).view(R, Kp // 32, 32), torch.cat([lo, pad], 1).view(R, Kp // 32, 32)
    return torch.stack([hi, lo], 2).reshape(R, Kp * 2).contiguous().view(torch.uint8)


def _pieces64(planes, bits, K):
    """hi and lo pieces of plane rows (uint8 (R, nkt * 128)) as fp64 values of the original matrix."""
    R = planes.shape[0]
    p = planes.contiguous().view(torch.float16).view(R, -1, 2, 32).double()
    inv = _inv_scale64(bits)[:, None]
    return p[:, :, 0, :].reshape(R, -1)[:, :K] * inv, p[:, :, 1, :].reshape(R, -1)[:, :K] * inv


def _nbytes(rows, K):
    return rows * ((K + 31) // 32) * 128


def _same(got, want, what):
    got, want = got.cpu(), want.cpu()
    if not torch.equal(got, want):
        bad = (got != want).nonzero().flatten()
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} differ, first at {bad[0].item()}: got {got[bad[0]].item():#x} want "
                             f"{want[bad[0]].item():#x}")


def _values(g, rows, K):
    """rows over seven decades (test_gemm_hp_matches_fp64)."""
    return torch.randn(rows, K, generator=g) * torch.exp(torch.empty(rows, 1).uniform_(-14, 3, generator=g))


def _special_rows(g, K):
    """an all-zero row | amax < 2^-112 (fp32-subnormal elements inside) | a subnormal amax | six decades inside one row"""
    dec = lambda: torch.pow(10.0, torch.empty(K).uniform_(-6, 0, generator=g))
    r = torch.randn(4, K, generator=g)
    out = torch.stack([torch.zeros(K), r[1] * 2.0 ** -120 * dec(), r[2] * 3e-41, r[3] * dec()])
    out[1, 0], out[2, 0], out[3, 0] = -(2.0 ** -119), 5e-40, -1.0      # the row maxima, whatever K
    return out


def _poisoned(nbytes_, words, dev, fill=FILL, fill32=FILL32, tail=256):
    return (torch.full((nbytes_ + tail,), fill, dtype=torch.uint8, device=dev),
            torch.full((words + 8,), fill32 if fill32 < 2 ** 31 else fill32 - 2 ** 32, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------------------------------------------------------
# (a) plane format, bitwise
# ------------------------------------------------------------------------------------------------------------------
# rows, K, ld, base offset (floats), listed rows (None: all; n: n rows; negative: out of order)
RM_CASES = [(5, 1, 1, 0, None),
            (33, 45, 45, 0, None),        # ld % 4 != 0: scalar loads
            (70, 40, 56, 1, None),        # unaligned base: scalar loads
            (64, 43, 48, 0, None),        # vector loads, the last 8-chunk takes the scalar tail
            (300, 264, 272, 0, None),     # more than 64 chunks per row: a lane walks two
            (33000, 8, 8, 0, None),       # more rows than 4 x 8192 workgroups cover in one pass
            (90, 40, 40, 0, -37),
            (600, 96, 96, 0, 301)]


@pytest.mark.parametrize("rows,K,ld,off,listed", RM_CASES, ids=lambda v: str(v))
def test_split_row_major(rows, K, ld, off, listed):
    from rnntransducer_amd.ops import hp_split_ex
    g = torch.Generator().manual_seed(rows * 7 + K)
    if listed is None:
        idx = torch.arange(rows)
    else:
        idx = torch.randperm(rows, generator=g)[:abs(listed)]
        idx = idx if listed < 0 else idx.sort().values
    n = idx.numel()
    X = _values(g, n, K)
    X[:4] = _special_rows(g, K)[:n]
    x_buf = torch.full((off + rows * ld + 8,), float("nan"))
    at = off + idx[:, None] * ld + torch.arange(K)[None, :]
    assert 0 <= int(idx.min()) and int(idx.max()) < rows and int(at.max()) < x_buf.numel()
    x_buf[at.reshape(-1)] = X.reshape(-1)
    bits = _amax_bits(X, 1)
    assert int((bits >> 23).min()) == 0 and 0 < int((bits[1] >> 23)) < 15
    nb = _nbytes(rows, K)
    planes, amax = _poisoned(nb, rows, "cuda")
    want_p, want_a = planes.cpu(), amax.cpu()
    want_p[:nb].view(rows, -1)[idx] = _planes(X, bits)
    want_a[idx] = bits
    hp_split_ex(x_buf.cuda(), n, K, ld, planes, amax, off=off, idx=None if listed is None else idx.to(torch.int32).cuda())
    torch.cuda.synchronize()
    sub = (want_p[:nb].view(torch.int16).view(rows, -1, 2, 32)[idx][:, :, 1, :] & 0x7C00 == 0) & \
          (want_p[:nb].view(torch.int16).view(rows, -1, 2, 32)[idx][:, :, 1, :] & 0x03FF != 0)
    print(f"row-major {(rows, K, ld, off, listed)}: {int(sub.sum())} f16-subnormal lo values of {n * K}")
    _same(amax, want_a, "amax words")
    _same(planes, want_p, "plane bytes")


def _frames(lens, B=8):
    T = max(lens)
    return torch.tensor([t * B + b for t in range(T) for b in range(B) if t < lens[b]])


LENS45, LENS64 = [9, 8, 7, 6, 5, 4, 3, 3], [9, 9, 9, 9, 8, 8, 6, 6]     # 45 / 64 valid frames of 9 x 8
# R, Ksrc, K, ld, column offset, shift, kidx (None | lens), amax_given
T_CASES = [(1, 33, 33, 1, 0, 0, None, 0),
           (255, 45, 45, 255, 0, 8, None, 0),          # odd ld: scalar loads; shift = +B
           (257, 64, 64, 260, 0, -8, None, 1),         # a second column block of one column; shift = -B
           (300, 64, 45, 300, 0, 0, None, 0),          # K < Ksrc: k = 45 .. 63 of the last line are zero, not source rows
           (1, 40, 33, 3, 1, 8, None, 1),
           (96, 72, 45, 192, 96, 0, LENS45, 0),        # the y + dir * H window of a bidirectional layer's output
           (96, 72, 45, 192, 96, 8, LENS45, 1),
           (300, 72, 45, 301, 0, -8, LENS45, 1),
           (257, 72, 33, 260, 0, -8, LENS45, 0),       # the first 33 of the valid frames
           (255, 72, 64, 256, 0, 8, LENS64, 0),        # vector loads with a 3-column scalar tail
           (300, 72, 64, 300, 0, -8, LENS64, 1)]


@pytest.mark.parametrize("R,Ksrc,K,ld,coff,shift,lens,given", T_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_split_transposed(R, Ksrc, K, ld, coff, shift, lens, given):
    from rnntransducer_amd.ops import hp_split_ex
    g = torch.Generator().manual_seed(R * 5 + K + shift + given)
    X = torch.randn(Ksrc, R, generator=g) * torch.exp(torch.empty(1, R).uniform_(-14, 3, generator=g)) \
        * torch.pow(10.0, torch.empty(Ksrc, 1).uniform_(-3, 0, generator=g))
    if R >= 4:
        sp = _special_rows(g, Ksrc)
        X[:, 0], X[:, 1], X[:, 2] = sp[0], sp[1], sp[2]
    x_buf = torch.full((Ksrc * ld + 8,), float("nan"))
    at = torch.arange(Ksrc)[:, None] * ld + coff + torch.arange(R)[None, :]
    assert coff + R <= ld and int(at.max()) < x_buf.numel()
    x_buf[at.reshape(-1)] = X.reshape(-1)
    kidx = None if lens is None else _frames(lens)[:K]
    assert kidx is None or (kidx.numel() == K and 0 <= int(kidx.min()) and int(kidx.max()) < Ksrc)
    ks = (torch.arange(K) if kidx is None else kidx) + shift
    ok = (ks >= 0) & (ks < Ksrc)
    assert shift == 0 or 0 < int(ok.sum()) < K                            # some of the contraction is zero fill
    V = torch.zeros(R, K)
    V[:, ok] = X[ks[ok]].t()
    colbits = _amax_bits(X, 0)                                            # over ALL source rows, listed or not
    nb = _nbytes(R, K)
    planes, amax = _poisoned(nb, R, "cuda")
    want_p, want_a = planes.cpu(), amax.cpu()
    if given:
        table = (X.abs().amax(0) * torch.empty(R).uniform_(1, 40, generator=g)).view(torch.int32).clone()
        table[R // 2] = torch.tensor(1e30).view(torch.int32)
        amax[:R] = table.cuda()
        want_a[:R] = table
    else:
        table = colbits
        want_a[:R] = colbits
    want_p[:nb].view(R, -1)[:] = _planes(V, table)
    hp_split_ex(x_buf.cuda(), R, K, ld, planes, amax, off=coff, transpose=True, src_rows=Ksrc, shift=shift,
                idx=None if kidx is None else kidx.to(torch.int32).cuda(), amax_given=bool(given))
    torch.cuda.synchronize()
    _same(amax, want_a, "amax words")
    _same(planes, want_p, "plane bytes")


@pytest.mark.parametrize("rows,C,ld,off", [(130, 300, 300, 0), (5000, 40, 48, 4)], ids=lambda v: str(v))
def test_colmax(rows, C, ld, off):
    """3 and 79 row chunks (64 rows at least per chunk), merged by atomicMax on the bit patterns; the sign is dropped."""
    from rnntransducer_amd.ops import hp_colmax
    g = torch.Generator().manual_seed(rows)
    X = _values(g, rows, C) * torch.exp(torch.empty(1, C).uniform_(-20, 5, generator=g))
    X[:, 0] = -0.0                                                         # a column of negative zeros: maximum +0
    X[:, 1] = -X[:, 1].abs()                                               # an all-negative column
    X[rows - 1, 2] = -1e30                                                 # the maximum is negative and in the last chunk
    X[:, 3] = torch.randn(rows, generator=g) * 3e-41                       # subnormals
    assert bool((X < 0).any()) and bool((X.view(torch.int32) == -2 ** 31).any())
    x_buf = torch.full((off + rows * ld + 8,), float("nan"))
    at = off + torch.arange(rows)[:, None] * ld + torch.arange(C)[None, :]
    x_buf[at.reshape(-1)] = X.reshape(-1)
    _, amax = _poisoned(0, C, "cuda")
    want = amax.cpu()
    want[:C] = _amax_bits(X, 0)
    assert int(want[0]) == 0 and want[2] == torch.tensor(1e30).view(torch.int32)
    hp_colmax(x_buf.cuda(), rows, C, ld, amax, off=off)
    torch.cuda.synchronize()
    _same(amax, want, "column maxima")


@pytest.mark.parametrize("Mv,Mtot,C,ld", [(77, 200, 300, 308), (33, 64, 40, 40)], ids=lambda v: str(v))
def test_split_both_with_rowidx(Mv, Mtot, C, ld):
    """Row-major lines in place at rowidx[i] (scale from rowmax[rowidx[i]]), transposed planes packed over i with zero fill up to the
    padded contraction; both tables given, some entries above the true maxima."""
    from rnntransducer_amd.ops import hp_split_both_ex
    g = torch.Generator().manual_seed(Mv + C)
    idx = torch.randperm(Mtot, generator=g)[:Mv]
    X = _values(g, Mv, C)
    X[:4] = _special_rows(g, C)
    x_buf = torch.full((Mtot * ld + 8,), float("nan"))
    at = idx[:, None] * ld + torch.arange(C)[None, :]
    assert int(idx.max()) < Mtot and int(at.max()) < x_buf.numel()
    x_buf[at.reshape(-1)] = X.reshape(-1)
    looser = lambda m, n: (m * torch.where(torch.rand(n, generator=g) < 0.3, 4.5, 1.0)).view(torch.int32).clone()
    rowbits, colbits = looser(X.abs().amax(1), Mv), looser(X.abs().amax(0), C)
    rowmax = torch.full((Mtot,), -1, dtype=torch.int32)                   # unlisted rows: NaN words
    rowmax[idx] = rowbits
    nb_rm, nb_t = _nbytes(Mtot, C), _nbytes(C, Mv)
    p_rm, _ = _poisoned(nb_rm, 0, "cuda")
    p_t, _ = _poisoned(nb_t, 0, "cuda")
    want_rm, want_t = p_rm.cpu(), p_t.cpu()
    want_rm[:nb_rm].view(Mtot, -1)[idx] = _planes(X, rowbits)
    want_t[:nb_t].view(C, -1)[:] = _planes(X.t().contiguous(), colbits)
    hp_split_both_ex(x_buf.cuda(), Mv, C, ld, rowmax.cuda(), colbits.cuda(), p_rm, p_t, rowidx=idx.to(torch.int32).cuda())
    torch.cuda.synchronize()
    _same(p_rm, want_rm, "row-major plane bytes")
    _same(p_t, want_t, "transposed plane bytes")


# ------------------------------------------------------------------------------------------------------------------
# (b) products through rnnt_hip_gemm_hp_ex
# ------------------------------------------------------------------------------------------------------------------
# id, (M, N, K), plane rows of A (0: M, dense), a map, c map, features, workspace, plan (tiles_m, tiles_n, group_m, splits, kt_per_split)
#   a map: None | "sub" (M distinct plane rows, out of order) | "repeat" | "ident";  c map: None | "a" (the a table) | "perm" | "ident"
#   features: bias | accum | f16 | ldc13 (c_so = N + 13, five elements in) | cdiv (c_div = 5, c_so = N + 3, c_si = 60 (N + 3))
#   workspace: "query" (what rnnt_hip_gemm_hp_workspace_bytes asks for) | "two" (exactly two slabs) | "none"
PRODUCTS = [
    ("gather-scatter", (257, 130, 40), 600, "sub", "a", "bias", "query", (2, 1, 4, 1, 2)),         # the second M tile has one row
    ("gather-repeats", (300, 257, 96), 320, "repeat", None, "accum ldc13", "query", (2, 2, 4, 1, 3)),
    ("scatter-cdiv-f16", (300, 130, 45), 0, None, "perm", "cdiv f16", "query", (2, 1, 4, 1, 2)),
    ("one", (1, 1, 1), 1, "ident", "ident", "", "query", (1, 1, 4, 1, 1)),
    ("exact-tile", (256, 256, 32), 256, "ident", "ident", "", "query", (1, 1, 4, 1, 1)),
    ("bands-4-2", (1300, 300, 40), 1500, "sub", "a", "", "query", (6, 2, 4, 1, 2)),               # a band of 4 tile rows and a tail band of 2
    ("split2", (70, 40, 2061), 0, None, None, "", "query", (1, 1, 4, 2, 33)),                    # 65 K-tiles: 33 + 32
    ("split2-bias-accum", (70, 40, 2061), 0, None, None, "bias accum", "query", (1, 1, 4, 2, 33)),
    ("split2-f16", (70, 40, 2061), 0, None, None, "f16", "query", (1, 1, 4, 2, 33)),
    ("split2-scatter-cdiv", (70, 40, 2061), 0, None, "perm", "cdiv accum", "query", (1, 1, 4, 2, 33)),   # the C map of the slab reduce
    ("split4-gather", (70, 40, 4100), 200, "sub", "a", "", "query", (1, 1, 4, 4, 33)),            # 129 K-tiles: the last slab has 30
    ("split4-two-slabs", (70, 40, 4100), 200, "sub", "a", "", "two", (1, 1, 4, 2, 65)),
    ("split4-no-workspace", (70, 40, 4100), 200, "sub", "a", "", "none", (1, 1, 4, 1, 129)),
]


def _bound_and_ref(A, W, a_pl, a_bits, b_pl, b_bits, K, f16, bias, base):
    """fp64 reference and per-element bound of C = A . W^T (+ bias + base) for the (M, K) rows A / plane rows a_pl the product reads."""
    if f16:
        ha, hb = _pieces64(a_pl, a_bits, K)[0], _pieces64(b_pl, b_bits, K)[0]
        assert bias is None and base is None
        return ha @ hb.t(), RTOL_F16 * (ha.abs() @ hb.abs().t()) + 1e-300
    ref, S = A.double() @ W.double().t(), A.double().abs() @ W.double().abs().t()
    if bias is not None:
        ref, S = ref + bias.double(), S + bias.double().abs()
    if base is not None:
        ref, S = ref + base.double(), S + base.double().abs()
    return ref, RTOL * S + 1e-300


@pytest.mark.parametrize("case", PRODUCTS, ids=lambda c: c[0])
def test_product(case):
    from rnntransducer_amd._lib import GEMM_ACCUM, GEMM_HP_F16
    from rnntransducer_amd.ops import gemm_hp_ex, gemm_hp_plan
    name, (M, N, K), PR, amap, cmap, feats, wsk, want_plan = case
    f, dev = set(feats.split()), "cuda"
    g = torch.Generator().manual_seed(M * 31 + N * 7 + K + len(name))
    PR = PR or M
    m = torch.arange(M)
    sub = torch.randperm(PR, generator=g)[:M]
    aidx = {None: None, "sub": sub, "ident": m, "repeat": torch.arange(0, PR, 3)[torch.randint(0, (PR + 2) // 3, (M,), generator=g)]}[amap]
    rows = m if aidx is None else aidx
    cidx_rows = {None: None, "a": aidx, "ident": m, "perm": torch.randperm(M, generator=g)}[cmap]
    mo = m if cidx_rows is None else cidx_rows
    # ---- operands: restated planes; what the A map does not address is 0xFF (NaN halves, an amax word of all ones)
    A_all, W = _values(g, PR, K), torch.randn(N, K, generator=g) * 0.05
    a_bits_all, b_bits = _amax_bits(A_all, 1), _amax_bits(W, 1)
    a_pl_all, b_pl = _planes(A_all, a_bits_all), _planes(W, b_bits)
    used = rows.unique()
    a_pl = torch.full_like(a_pl_all, 0xFF)
    a_pl[used] = a_pl_all[used]
    a_amax = torch.full((PR,), -1, dtype=torch.int32)
    a_amax[used] = a_bits_all[used]
    assert amap is None or used.numel() < PR or amap == "ident"
    # ---- destination
    if "cdiv" in f:
        c_off, c_div, c_so, c_si = 2, 5, N + 3, 60 * (N + 3)
        c_size = 5 * 60 * (N + 3) + 8
    elif "ldc13" in f:
        c_off, c_div, c_so, c_si = 5, 1, N + 13, 0
        c_size = (int(mo.max()) + 2) * (N + 13)
    else:
        c_off, c_div, c_so, c_si = 0, 1, N, 0
        c_size = (max(PR, M) + 2) * N
    cidx = c_off + ((mo // c_div) * c_so + (mo % c_div) * c_si)[:, None] + torch.arange(N)[None, :]
    # nothing addresses outside an allocation, and no two rows of the product share a destination element
    assert 0 <= int(rows.min()) and int(rows.max()) < PR and 0 <= int(cidx.min()) and int(cidx.max()) < c_size
    assert cidx.unique().numel() == M * N
    bias = torch.randn(N, generator=g) if "bias" in f else None
    c_buf = torch.randn(c_size, generator=g)
    base = c_buf[cidx].clone() if "accum" in f else None
    if base is None:
        c_buf[cidx.reshape(-1)] = float("nan")
    # ---- the plan this case names
    slab = M * N * 4
    ws_bytes = {"query": None, "two": 2 * slab, "none": 0}[wsk]
    plan = gemm_hp_plan(M, N, K, ws_bytes)
    assert tuple(plan[:5]) == want_plan, plan
    flags = (GEMM_ACCUM if "accum" in f else 0) | (GEMM_HP_F16 if "f16" in f else 0)
    i32 = lambda t: None if t is None else t.to(torch.int32).to(dev)
    kw = dict(bias=None if bias is None else bias.to(dev), flags=flags, workspace_bytes=ws_bytes)
    a_pl_d, a_amax_d, b_pl_d, b_bits_d = a_pl.reshape(-1).to(dev), a_amax.to(dev), b_pl.reshape(-1).to(dev), b_bits.to(dev)
    outs = [c_buf.to(dev), c_buf.to(dev)]
    for out in outs:
        gemm_hp_ex(a_pl_d, a_amax_d, b_pl_d, b_bits_d, M, N, K, out, c_off=c_off, c_div=c_div, c_so=c_so, c_si=c_si, a_rowidx=i32(aidx),
                   a_plane_rows=PR if aidx is not None else 0, c_rowidx=i32(cidx_rows), **kw)
    # the same plane rows, packed, through the plain form
    dense = (base.clone() if base is not None else torch.full((M, N), float("nan"))).to(dev)
    gemm_hp_ex(a_pl_all[rows].reshape(-1).to(dev), a_bits_all[rows].to(dev), b_pl_d, b_bits_d, M, N, K, dense, **kw)
    torch.cuda.synchronize()
    o0, o1 = outs[0].cpu(), outs[1].cpu()
    assert torch.equal(o0.view(torch.int32), o1.view(torch.int32)), "two runs differ"
    untouched = torch.ones(c_size, dtype=torch.bool)
    untouched[cidx.reshape(-1)] = False
    assert torch.equal(o0.view(torch.int32)[untouched], c_buf.view(torch.int32)[untouched]), "wrote outside the C map"
    got = o0[cidx]
    ref, tol = _bound_and_ref(A_all[rows], W, a_pl_all[rows], a_bits_all[rows], b_pl, b_bits, K, "f16" in f, bias, base)
    err = (got.double() - ref).abs()
    assert not torch.isnan(err).any(), "NaN: an unaddressed plane row was read, or an output element was not written"
    worst = (err / tol).max().item()
    print(f"product {name} {(M, N, K)}: plan {tuple(plan)}; max err / bound {worst:.3g}")
    assert worst <= 1.0, worst
    assert torch.equal(got.view(torch.int32), dense.cpu().view(torch.int32)), "differs from the dense product of the same plane rows"


@pytest.mark.parametrize("shift", [0, 8, -8])
def test_product_of_packed_transposed_operands(shift):
    """dW = dG^T . X over the 301 valid frames of 600 (B = 8): both operands through the transposed split with kidx, packed along
    the contraction; shift = +-B is the h_prev operand of dW_hh (frame t -+ 1 of the same utterance, zero outside the source)."""
    from rnntransducer_amd.ops import gemm_hp_ex, gemm_hp_plan, hp_split_ex
    M, N, K, Ksrc, dev = 96, 130, 301, 600, "cuda"
    g = torch.Generator().manual_seed(41 + shift)
    dG = torch.randn(Ksrc, M, generator=g) * torch.exp(torch.empty(Ksrc, 1).uniform_(-10, 0, generator=g))
    X = torch.randn(Ksrc, N, generator=g)
    kidx = torch.randperm(Ksrc, generator=g)[:K].sort().values
    ks = kidx + shift
    ok = (ks >= 0) & (ks < Ksrc)
    assert 0 <= int(kidx.min()) and int(kidx.max()) < Ksrc and (shift == 0 or int(ok.sum()) < K)
    A, Xs = dG[kidx].t().contiguous(), torch.zeros(K, N)
    Xs[ok] = X[ks[ok]]
    unread = torch.ones(Ksrc, dtype=torch.bool)
    unread[kidx] = False
    dG[unread] = float("nan")                                              # frames outside the list are never read
    unread[:] = True
    unread[ks[ok]] = False
    X[unread] = float("nan")
    (a_pl, a_amax), (b_pl, b_amax) = _poisoned(_nbytes(M, K), M, dev), _poisoned(_nbytes(N, K), N, dev)
    a_amax[:M], b_amax[:N] = _amax_bits(A, 1).to(dev), _amax_bits(Xs, 0).to(dev)     # maxima over the frames that are read
    kd = kidx.to(torch.int32).to(dev)
    hp_split_ex(dG.to(dev), M, K, M, a_pl, a_amax, transpose=True, src_rows=Ksrc, idx=kd, amax_given=True)
    hp_split_ex(X.to(dev), N, K, N, b_pl, b_amax, transpose=True, src_rows=Ksrc, shift=shift, idx=kd, amax_given=True)
    plan = gemm_hp_plan(M, N, K)
    assert tuple(plan[:5]) == (1, 1, 4, 1, 10), plan
    outs = [torch.full((M, N), float("nan"), device=dev) for _ in range(2)]
    for out in outs:
        gemm_hp_ex(a_pl, a_amax, b_pl, b_amax, M, N, K, out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two runs differ"
    ref, S = A.double() @ Xs.double(), A.double().abs() @ Xs.double().abs()
    err = (outs[0].cpu().double() - ref).abs()
    assert not torch.isnan(err).any()
    worst = (err / (RTOL * S + 1e-300)).max().item()
    print(f"packed transposed pair {(M, N, K)} shift {shift}: max err / bound {worst:.3g}")
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------------
# (c) the grouped, queue-driven launch
# ------------------------------------------------------------------------------------------------------------------
def _hp(x):
    from rnntransducer_amd.ops import hp_split
    return hp_split(x.cuda())


def _planes_of(t):
    nb = _nbytes(t.rows, t.K)
    return t.planes[:nb].cpu().view(t.rows, -1), t.amax[:t.rows].cpu()


GROUP = [(300, 130, 2100), (1, 1, 1), (70, 40, 2100), (257, 96, 45)]     # 66 K-tiles: 3 slabs of 22 at the 32-tile chunk floor


@pytest.mark.parametrize("ws", ["query", "one-slab"])
@pytest.mark.parametrize("f16", [False, True], ids=["hp", "f16"])
def test_grouped_launch_forms(ws, f16):
    """Four problems in one launch: a column block of a wider matrix (ldc > N), a (1, 1, 1), ACCUM on two of them and not on the
    others (one ACCUM through the split-K reduce, one through the tile epilogue; default mode only: the F16 bound has no base term),
    K = 2100.  With a workspace of the 256-byte header plus ONE slab of the first problem its slabs shrink from 3 to 1 and the third
    problem still splits; the results keep their bounds either way."""
    from rnntransducer_amd.ops import gemm_hp_grouped
    g = torch.Generator().manual_seed(77 + f16)
    mats = [(_values(g, M, K), torch.randn(N, K, generator=g) * 0.05) for M, N, K in GROUP]
    pairs = [(_hp(a), _hp(b)) for a, b in mats]
    acc = [False, False, not f16, not f16]
    ldcs, coffs = [130 + 13, 1, 40, 96 + 7], [5, 0, 0, 3]
    bufs = [torch.randn((M + 1) * ldc, generator=g) for (M, N, K), ldc in zip(GROUP, ldcs)]
    cidx = [co + torch.arange(M)[:, None] * ldc + torch.arange(N)[None, :] for (M, N, K), ldc, co in zip(GROUP, ldcs, coffs)]
    for b, ci in zip(bufs, cidx):
        assert int(ci.max()) < b.numel()
    bases = [b[ci].clone() if a else None for b, ci, a in zip(bufs, cidx, acc)]
    for b, ci, a in zip(bufs, cidx, acc):
        if not a:
            b[ci.reshape(-1)] = float("nan")
    nws = None if ws == "query" else 256 + (300 * 130 * 4 + 255) // 256 * 256
    runs = []
    for _ in range(2):
        dev = [b.cuda() for b in bufs]
        views = [d[co:].as_strided((M, N), (ldc, 1)) for d, (M, N, K), ldc, co in zip(dev, GROUP, ldcs, coffs)]
        gemm_hp_grouped(pairs, outs=views, accumulate=acc, check=True, f16=f16, workspace_bytes=nws)
        torch.cuda.synchronize()
        runs.append([d.cpu() for d in dev])
    for i, ((M, N, K), (A, W)) in enumerate(zip(GROUP, mats)):
        o0, o1 = runs[0][i], runs[1][i]
        assert torch.equal(o0.view(torch.int32), o1.view(torch.int32)), f"problem {i}: two runs differ"
        untouched = torch.ones(o0.numel(), dtype=torch.bool)
        untouched[cidx[i].reshape(-1)] = False
        assert torch.equal(o0.view(torch.int32)[untouched], bufs[i].view(torch.int32)[untouched]), f"problem {i}: wrote outside its block"
        (a_pl, a_bits), (b_pl, b_bits) = _planes_of(pairs[i][0]), _planes_of(pairs[i][1])
        ref, tol = _bound_and_ref(A, W, a_pl, a_bits, b_pl, b_bits, K, f16, None, bases[i])
        err = (o0[cidx[i]].double() - ref).abs()
        assert not torch.isnan(err).any(), f"problem {i}: an element was not written"
        worst = (err / tol).max().item()
        print(f"grouped {'f16' if f16 else 'hp'} workspace {ws} problem {i} {(M, N, K)}: max err / bound {worst:.3g}")
        assert worst <= 1.0, (i, worst)
