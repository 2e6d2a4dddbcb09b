"""Every kernel instance rnnt_hip_gemm_f32 can dispatch, crossed with its operand maps and epilogues, against float64.

The launch picks one compiled instance per call (csrc/gemm.hip, make_gemm_plan): a tiling (128x128, 128x256 with 256 threads; 256x256
with 512), an operand layout pair (A and B each k-contiguous or not), vector or scalar operand loads, and split-K slabs summed by
splitk_reduce_kernel or a single pass.  ROWS names, for every such instance, one shape that reaches it THROUGH THE PRODUCTION DISPATCH
(ops.gemm's own workspace rule, no environment switch) and the features that case carries.  Each case

  * asserts from the plan query (rnnt_hip_gemm_plan, the function the launch takes its decisions from) that it reaches the instance
    it names: a case that lands elsewhere fails;
  * lays its operands out in flat buffers through the maps of include/rnnt_hip.h, restated here as index tensors.  Every element the
    maps do not address is NaN in the operands (a stray load poisons the result) and a sentinel in the destination that must come
    back bit-identical; addressed destination elements start as NaN unless ACCUM adds onto them.  The index tensors are checked to
    lie inside the allocations before anything is launched;
  * runs twice and asserts the two results bitwise equal (split-K slabs are summed in a fixed order);
  * compares with a float64 CPU product of the same fp32 inputs, per element:
        |got - ref| <= 2e-6 * (sum_k |a||b| + |bias| + |base|)
    the bound of test_gemm_arithmetic_modes / test_gemm_hp_matches_fp64 for K <= 4096 in the default and the exact-fp32 modes.
    GELU / MUL_DGELU cases add the error of evaluating the activation in fp32, MEASURED on the reference side: the same formula with
    torch's fp32 gelu(approximate="tanh") (or its derivative) around the fp64 product, against the all-fp64 reference; 4x its
    largest value relative to S = sum_k |a||b| + |bias| is allowed on top (the kernel's gelu_tanh need not round like torch's).
    Measured over the rows below (it is a property of the inputs and of torch's fp32 formulas, computed on the CPU): rows with
    GELU_A / GELU_B only 6.6e-9 .. 6.0e-7 of S (largest where rows overlap and carry no scale of their own: many x < -3, where
    1 + tanh cancels), rows with MUL_DGELU 9.9e-8 .. 1.04e-6 of S; the allowance is therefore at most 4.2e-6 S next to the 2e-6 S of
    the product.  Every case prints its figure and its largest error / bound before it asserts.

test_every_dispatchable_instance_is_named closes the matrix: (tiling x layouts x vec x split) of the default mode, the two 128-row
tilings x layouts of RNNT_GEMM_EXACT_F32, and the feature x (tiling, split / vec) crossings listed in FEATURE_CROSSINGS.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 2e-6          # product bound, relative to sum_k |a||b| + |bias| + |base|
ACT_ALLOW = 4.0      # x the measured fp32-activation error of the reference side (module docstring: 6.6e-9 .. 1.04e-6 of S)
BIG = 1 << 40

T128, T256N, T256 = (128, 128), (128, 256), (256, 256)
# layouts: first letter A ("n": k-contiguous rows (M,K); "t": stored (K,M), a_mc = 1), second letter B ("t": k-contiguous rows (N,K), the
# nn.Linear weight; "n": stored (K,N))
LAYOUTS = {"nt": (True, True), "nn": (True, False), "tn": (False, False), "tt": (False, True)}

# features: bias | accum (onto a random base) | dgelu (MUL_DGELU, aux laid out like C through the same C map) | gelu_a | gelu_b |
#   csub  (c_div = 1, c_so = N + 13, c_si = 0, c_off = 5: a column block of a wider matrix, the fc.weight.grad halves) |
#   cdiv  (c_div = 5, c_so = N + 3, c_si = T (N + 3), c_off = 2: time-major rows scattered to a batch-major destination) |
#   adiv  (a_div = 5, a_so = lda, a_si = T lda: a batch-major source read as (t, b) rows) |
#   aoverlap (a_div = F, a_so = Lp, a_si = hop < K: the front-end's overlapping frames) | arowidx (repeated, out-of-order rows) |
#   bsub4 / bsub1 (B = the right half of a wider (N, K0 + K) matrix, b_off = K0 = 8 / 7; K0 = 7 must plan scalar loads although every
#   stride is a multiple of 4) | exact (RNNT_GEMM_EXACT_F32)
# columns: tiling, layouts, vec, split, (M, N, K), features
ROWS = [
    # ---- 128x128: N off the multiples of 256, or too few tiles for the wider forms
    (T128, "nt", 1, 0, (130, 70, 33), "bias gelu_a adiv"),              # K % 4 != 0 in a vector instance: the scalar K tail
    (T128, "nt", 0, 0, (130, 70, 33), "gelu_a gelu_b aoverlap csub"),
    (T128, "nn", 1, 0, (257, 129, 40), "gelu_b accum cdiv"),
    (T128, "nn", 0, 0, (257, 129, 41), "gelu_b arowidx bias"),
    (T128, "tn", 1, 0, (131, 70, 72), "gelu_a gelu_b csub"),             # ragged rows of both row-contiguous loaders
    (T128, "tn", 0, 0, (131, 70, 33), "gelu_a gelu_b dgelu cdiv"),
    (T128, "tt", 1, 0, (1000, 72, 40), "gelu_a bsub4 bias accum"),
    (T128, "tt", 0, 0, (1000, 72, 40), "gelu_a bsub1 dgelu csub"),       # strides aligned, b_off = 7: scalar
    (T128, "nt", 1, 1, (130, 70, 300), "bias accum dgelu cdiv aoverlap"),
    (T128, "nt", 0, 1, (130, 70, 301), "bias csub arowidx bsub1"),
    (T128, "nn", 1, 1, (257, 129, 260), "accum csub arowidx"),
    (T128, "nn", 0, 1, (257, 129, 261), "dgelu csub gelu_a"),
    (T128, "tn", 1, 1, (72, 200, 1000), "gelu_b accum csub"),             # the joint's dW: GELU on B, ACCUM, a column block
    (T128, "tn", 0, 1, (72, 200, 1001), "gelu_b bias cdiv"),
    (T128, "tt", 1, 1, (131, 70, 300), "dgelu bsub4"),
    (T128, "tt", 0, 1, (131, 70, 300), "accum gelu_b"),
    (T128, "nt", 1, 0, (128, 128, 16), ""),                               # exact tile
    (T128, "nt", 0, 0, (1, 1, 1), "bias"),                                # degenerate
    (T128, "tn", 1, 0, (1, 1, 1), "accum"),
    # ---- 128x256: N % 256 == 0 and >= 64 such tiles, < 64 256-row tiles (or M < 256, where the 256x256 form is not taken)
    (T256N, "nt", 1, 0, (3970, 512, 40), "bias gelu_a aoverlap cdiv"),
    (T256N, "nt", 0, 0, (3970, 512, 33), "gelu_a aoverlap accum"),
    (T256N, "nn", 1, 0, (8100, 256, 72), "dgelu csub arowidx"),
    (T256N, "nn", 0, 0, (8100, 256, 33), "gelu_b bias"),
    (T256N, "tn", 1, 0, (3970, 512, 40), "gelu_a gelu_b csub"),
    (T256N, "tn", 0, 0, (3970, 512, 33), "gelu_a gelu_b dgelu"),
    (T256N, "tt", 1, 0, (8100, 256, 40), "bsub4 accum"),
    (T256N, "tt", 0, 0, (8100, 256, 40), "bsub1 gelu_b cdiv"),
    (T256N, "nt", 1, 1, (131, 8192, 258), "bias accum dgelu csub gelu_a"),
    (T256N, "nt", 0, 1, (131, 8192, 257), "bias cdiv aoverlap"),
    (T256N, "nn", 1, 1, (131, 8192, 256), "dgelu cdiv adiv"),
    (T256N, "nn", 0, 1, (131, 8192, 257), "accum arowidx gelu_b"),
    (T256N, "tn", 1, 1, (131, 8192, 260), "gelu_b accum csub"),
    (T256N, "tn", 0, 1, (131, 8192, 257), "gelu_a bias"),
    (T256N, "tt", 1, 1, (131, 8192, 258), "bsub4 dgelu"),
    (T256N, "tt", 0, 1, (131, 8192, 258), "bsub1 accum cdiv"),
    (T256N, "nt", 1, 0, (8192, 256, 16), ""),                             # exact tiles
    # ---- 256x256, one pass: >= 64 tiles of 256x256
    (T256, "nt", 1, 0, (2100, 1800, 40), "bias gelu_a aoverlap"),
    (T256, "nt", 0, 0, (2100, 1800, 33), "gelu_a gelu_b aoverlap csub"),
    (T256, "nn", 1, 0, (2100, 1800, 72), "dgelu cdiv"),                   # the joint's dX: MUL_DGELU behind a K tail
    (T256, "nn", 0, 0, (2100, 1800, 33), "gelu_b arowidx accum"),
    (T256, "tn", 1, 0, (2100, 1800, 40), "gelu_a gelu_b accum csub"),
    (T256, "tn", 0, 0, (2100, 1800, 33), "gelu_a gelu_b bias"),
    (T256, "tt", 1, 0, (2100, 1800, 72), "bsub4 gelu_a dgelu csub"),
    (T256, "tt", 0, 0, (2100, 1800, 40), "bsub1 cdiv"),
    (T256, "nt", 1, 0, (2048, 2048, 16), ""),                             # exact tiles
    # ---- 256x256 with split-K: fewer tiles, K >= 128 and a workspace, tiles x slabs >= 64
    (T256, "nt", 1, 1, (515, 515, 1030), "bias accum dgelu csub gelu_a"),
    (T256, "nt", 0, 1, (515, 515, 1030), "bias cdiv aoverlap"),
    (T256, "nn", 1, 1, (515, 515, 1030), "dgelu cdiv arowidx"),
    (T256, "nn", 0, 1, (515, 515, 1025), "accum adiv gelu_b"),
    (T256, "tn", 1, 1, (515, 515, 1030), "gelu_b accum csub"),            # config 5's dW of the joint
    (T256, "tn", 0, 1, (515, 515, 1025), "gelu_a bias"),
    (T256, "tt", 1, 1, (515, 515, 1030), "bsub4 dgelu"),
    (T256, "tt", 0, 1, (515, 515, 1030), "bsub1 accum cdiv gelu_b"),
    # ---- RNNT_GEMM_EXACT_F32 (gemm_f32_kernel): the two 128-row tilings x four layouts
    (T128, "nt", 1, 0, (130, 70, 33), "exact bias gelu_a"),
    (T128, "nn", 0, 0, (257, 129, 41), "exact gelu_b accum"),
    (T128, "tn", 1, 1, (72, 200, 1000), "exact gelu_b accum csub"),
    (T128, "tt", 0, 0, (131, 70, 33), "exact gelu_a dgelu cdiv"),
    (T256N, "nt", 0, 0, (3970, 512, 33), "exact gelu_a aoverlap"),
    (T256N, "nn", 1, 0, (8100, 256, 40), "exact dgelu csub"),
    (T256N, "tn", 0, 0, (3970, 512, 33), "exact gelu_a gelu_b bias"),
    (T256N, "tt", 1, 1, (131, 8192, 258), "exact bsub4 accum cdiv"),
]

# feature -> what it must be crossed with: "split" = every tiling, one pass and split-K (it passes through splitk_reduce_kernel);
# "vec" = every tiling, vector and scalar loads (it touches a loader); "tile" = every tiling
FEATURE_CROSSINGS = {"bias": "split", "accum": "split", "dgelu": "split", "csub": "split", "cdiv": "split",
                     "gelu_a": "vec", "gelu_b": "vec", "adiv": "tile", "aoverlap": "vec", "arowidx": "vec", "bsub4": "tile", "bsub1": "tile"}


def _row_id(row):
    tile, lay, vec, split, (M, N, K), feats = row
    return f"{tile[0]}x{tile[1]}-{lay}-{'vec' if vec else 'scalar'}-{'split' if split else 'onepass'}-{M}x{N}x{K}-{feats.replace(' ', '+') or 'plain'}"


def _stride(n, aligned, odd=1):
    s = (n + 3) // 4 * 4 + 4          # always at least 4 elements of padding behind the payload
    return s if aligned else s + odd


def gelu64(x):
    return torch.nn.functional.gelu(x.double(), approximate="tanh")


def _dgelu(x):
    x = x.clone().requires_grad_(True)
    torch.nn.functional.gelu(x, approximate="tanh").sum().backward()
    return x.grad


def _build(row):
    """CPU side of one case: flat operand / destination buffers, the gemm() keywords, and the index tensors of the maps."""
    tile, lay, vec, split, (M, N, K), feats = row
    f = set(feats.split())
    a_kc, b_kc = LAYOUTS[lay]
    al = bool(vec) or "bsub1" in f       # bsub1: every stride a multiple of 4, only b_off breaks the alignment
    g = torch.Generator().manual_seed(M * 31 + N * 7 + K + 1000 * len(feats))
    kw = {}
    m, n, k = torch.arange(M), torch.arange(N), torch.arange(K)
    # ---- A
    rowidx = None
    if a_kc:
        if "adiv" in f:
            Bb, lda = 5, _stride(K, al)
            T = -(-M // Bb)
            kw.update(a_div=Bb, a_so=lda, a_si=T * lda)
            a_size = Bb * T * lda
        elif "aoverlap" in f:
            F = min(37, M)
            hop = 4 * max(K // 12, 1) + (0 if al else 1)
            assert hop < K
            Lp = _stride((F - 1) * hop + K, al)
            kw.update(a_div=F, a_so=Lp, a_si=hop)
            a_size = -(-M // F) * Lp
        elif "arowidx" in f:
            R, lda = 11, _stride(K, al)
            pool = torch.tensor([r for r in range(R) if r != 3])      # table row 3 is never gathered and stays NaN
            rowidx = pool[torch.randint(0, len(pool), (M,), generator=g)]
            kw.update(a_si=lda)
            a_size = R * lda
        else:
            lda = _stride(K, al)
            kw.update(a_si=lda)
            a_size = (M + 1) * lda
        rowoff = rowidx * kw["a_si"] if rowidx is not None else (m // kw.get("a_div", BIG)) * kw.get("a_so", 0) + (m % kw.get("a_div", BIG)) * kw["a_si"]
        aidx = rowoff[:, None] + k[None, :]
    else:
        lda = _stride(M, al)
        kw.update(a_mc=True, a_sk=lda)
        a_size = (K + 1) * lda
        aidx = k[None, :] * lda + m[:, None]
    # ---- B
    b_off = 8 if "bsub4" in f else 7 if "bsub1" in f else 0
    if b_kc:
        ldb = _stride(b_off + K, al, odd=3)
        kw.update(b_off=b_off, b_sn=ldb, b_sk=1)
        b_size = (N + 1) * ldb
        bidx = b_off + n[None, :] * ldb + k[:, None]
    else:
        assert not b_off
        ldb = _stride(N, al, odd=3)
        kw.update(b_sn=1, b_sk=ldb)
        b_size = (K + 1) * ldb
        bidx = n[None, :] + k[:, None] * ldb
    # ---- C
    if "csub" in f:
        ldc = N + 13
        kw.update(c_off=5, c_div=1, c_so=ldc, c_si=0)
        c_size = (M + 1) * ldc
        cidx = 5 + m[:, None] * ldc + n[None, :]
    elif "cdiv" in f:
        Bb, ldc = 5, N + 3
        T = -(-M // Bb)
        kw.update(c_off=2, c_div=Bb, c_so=ldc, c_si=T * ldc)
        c_size = Bb * T * ldc
        cidx = 2 + ((m // Bb) * ldc + (m % Bb) * T * ldc)[:, None] + n[None, :]
    else:
        c_size = (M + 2) * N
        cidx = m[:, None] * N + n[None, :]
    # no case addresses outside an allocation
    assert 0 <= int(aidx.min()) and int(aidx.max()) < a_size and int(bidx.max()) < b_size and int(cidx.max()) < c_size
    assert cidx.unique().numel() == M * N

    # wide-range values: rows over several decades so that piece exponents matter; an operand that goes through GELU stays within
    # a few units and mostly small, where gelu(x) is far from x (x / 2 for small |x|, about 0 for x < -3)
    def values(rows, cols, gelu):
        lo, hi = (-6.0, 1.0) if gelu else (-14.0, 3.0)
        return torch.randn(rows, cols, generator=g) * torch.exp(torch.empty(rows, 1).uniform_(lo, hi, generator=g))
    a_buf = torch.full((a_size,), float("nan"))
    a_buf[aidx.reshape(-1)] = values(M, K, "gelu_a" in f).reshape(-1)
    b_buf = torch.full((b_size,), float("nan"))
    b_buf[bidx.reshape(-1)] = (values(N, K, "gelu_b" in f) * 0.05).t().reshape(-1)
    A, Bm = a_buf[aidx], b_buf[bidx]          # the logical (M,K) and (K,N) operands (overlapping rows: what was written last)
    assert not torch.isnan(A).any() and not torch.isnan(Bm).any()
    bias = torch.randn(N, generator=g) if "bias" in f else None
    c_buf = torch.randn(c_size, generator=g)  # sentinel outside the addressed elements, the ACCUM base inside
    base = c_buf[cidx].clone() if "accum" in f else None
    if base is None:
        c_buf[cidx.reshape(-1)] = float("nan")
    aux_buf = aux = None
    if "dgelu" in f:
        aux = torch.randn(M, N, generator=g) * 2.0
        aux_buf = torch.full((c_size,), float("nan"))
        aux_buf[cidx.reshape(-1)] = aux.reshape(-1)
    return dict(f=f, kw=kw, a_buf=a_buf, b_buf=b_buf, c_buf=c_buf, aux_buf=aux_buf, rowidx=rowidx, bias=bias, cidx=cidx, A=A, Bm=Bm,
                base=base, aux=aux)


def _flags(f):
    from rnntransducer_amd._lib import GEMM_ACCUM, GEMM_EXACT_F32, GEMM_GELU_A, GEMM_GELU_B, GEMM_MUL_DGELU
    return ((GEMM_GELU_A if "gelu_a" in f else 0) | (GEMM_GELU_B if "gelu_b" in f else 0) | (GEMM_ACCUM if "accum" in f else 0)
            | (GEMM_MUL_DGELU if "dgelu" in f else 0) | (GEMM_EXACT_F32 if "exact" in f else 0))


def _reference(c):
    """float64 result, per-element tolerance and the measured fp32-activation figure of one case."""
    f, A, Bm = c["f"], c["A"], c["Bm"]
    act = lambda x, on, f64: (gelu64(x) if f64 else torch.nn.functional.gelu(x, approximate="tanh").double()) if on else x.double()
    a64, b64 = act(A, "gelu_a" in f, True), act(Bm, "gelu_b" in f, True)
    P = a64 @ b64
    S = (a64.abs().float() @ b64.abs().float()).double()     # a scale: fp32 is accurate enough for it (1e-6 of itself)
    bias = c["bias"].double() if c["bias"] is not None else torch.zeros(Bm.shape[1], dtype=torch.float64)
    base = c["base"].double() if c["base"] is not None else 0.0
    Sb = S + bias.abs() + 1e-300
    P32 = act(A, True, False) @ b64 if "gelu_a" in f else P
    if "gelu_b" in f:
        P32 = (act(A, "gelu_a" in f, False)) @ act(Bm, True, False)
    if "dgelu" in f:
        g64, g32 = _dgelu(c["aux"].double()), _dgelu(c["aux"]).double()
        ref, ref32 = (P + bias) * g64 + base, (P32 + bias) * g32 + base
        tol = RTOL * (Sb * g64.abs() + abs(base))
    else:
        ref, ref32 = P + bias + base, P32 + bias + base
        tol = RTOL * (Sb + abs(base))
    extra = ((ref32 - ref).abs() / Sb).max().item()          # fp32 activation error of the reference side, relative to S
    return ref, tol + ACT_ALLOW * extra * Sb, extra


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_gemm_form(row):
    from rnntransducer_amd.ops import gemm, gemm_plan
    tile, lay, vec, split, (M, N, K), feats = row
    c = _build(row)
    f, dev = c["f"], "cuda"
    a, b = c["a_buf"].to(dev), c["b_buf"].to(dev)
    kw = dict(c["kw"], flags=_flags(f))
    if c["rowidx"] is not None:
        kw["a_rowidx"] = c["rowidx"].to(dev)
    if c["bias"] is not None:
        kw["bias"] = c["bias"].to(dev)
    if c["aux_buf"] is not None:
        kw["aux"] = c["aux_buf"].to(dev)
    outs = [c["c_buf"].to(dev), c["c_buf"].to(dev)]
    # the instance this case names is the instance the launch takes
    plan = gemm_plan(M, N, K, a, b, outs[0], **kw)
    want = dict(mode=0 if "exact" in f else 6, tile=tile, a_kc=LAYOUTS[lay][0], b_kc=LAYOUTS[lay][1], vec=bool(vec), split=bool(split))
    got = dict(mode=plan.mode, tile=plan.tile, a_kc=plan.a_kc, b_kc=plan.b_kc, vec=plan.vec, split=plan.splits > 1)
    assert got == want, plan
    if split:
        assert plan.splits * plan.kchunk >= K > (plan.splits - 1) * plan.kchunk and plan.kchunk % 16 == 0, plan
    for out in outs:
        gemm(M, N, K, a, b, out, **kw)
    torch.cuda.synchronize()
    o0, o1 = outs[0].cpu(), outs[1].cpu()
    assert torch.equal(o0.view(torch.int32), o1.view(torch.int32)), "two runs differ"
    # everything outside the addressed elements comes back bit-identical
    untouched = torch.ones(o0.numel(), dtype=torch.bool)
    untouched[c["cidx"].reshape(-1)] = False
    assert torch.equal(o0.view(torch.int32)[untouched], c["c_buf"].view(torch.int32)[untouched]), "wrote outside the C map"
    ref, tol, extra = _reference(c)
    err = (o0[c["cidx"]].double() - ref).abs()
    assert not torch.isnan(err).any(), "NaN: an unaddressed operand element was read, or an output element was not written"
    worst = (err / tol).max().item()
    print(f"{_row_id(row)}: plan {plan}; fp32 activation figure {extra:.3g} of S; max err / bound {worst:.3g}")
    assert worst <= 1.0, (worst, extra)


def test_every_dispatchable_instance_is_named():
    """The table covers the whole dispatch.  Default mode: every (tiling, layout pair, vec, split) — all 48 are reachable without a
    switch (the 128x256 tiling splits only where the 256x256 form is not taken, M < 256).  Exact-fp32 mode: the two 128-row tilings x
    layout pairs (it has no 256x256 form).  Every feature meets what FEATURE_CROSSINGS asks of it, and every tiling has an exact-tile
    case; the 128x128 tiling, the only one that admits it, has a (1, 1, 1) case."""
    named = {(r[0], r[1], r[2], r[3]) for r in ROWS if "exact" not in r[5].split()}
    want = {(t, l, v, s) for t in (T128, T256N, T256) for l in LAYOUTS for v in (0, 1) for s in (0, 1)}
    assert named == want, sorted(want - named)
    exact = {(r[0], r[1]) for r in ROWS if "exact" in r[5].split()}
    assert exact == {(t, l) for t in (T128, T256N) for l in LAYOUTS}, exact
    for feat, crossing in FEATURE_CROSSINGS.items():
        hit = {(r[0], r[2], r[3]) for r in ROWS if feat in r[5].split()}
        for t in (T128, T256N, T256):
            if crossing == "split":
                assert {s for (tt, _, s) in hit if tt == t} == {0, 1}, (feat, t)
            elif crossing == "vec" and feat != "bsub1":
                assert {v for (tt, v, _) in hit if tt == t} == {0, 1}, (feat, t)
            else:
                assert any(tt == t for (tt, _, _) in hit), (feat, t)
    for t in (T128, T256N, T256):
        assert any(r[0] == t and r[4][0] % t[0] == 0 and r[4][1] % t[1] == 0 and r[4][2] % 16 == 0 for r in ROWS), t
    assert any(r[4] == (1, 1, 1) for r in ROWS)
    assert len({_row_id(r) for r in ROWS}) == len(ROWS)
