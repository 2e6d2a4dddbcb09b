"""CTC kernels (csrc/ctc.hip: ctc_terms, ctc_sweep<K>, ctc_grad, ctc_greedy) through the C ABI against torch's CPU CTC loss in
float64, F.ctc_loss(F.log_softmax(z.double(), -1)), with autograd for the gradient with respect to the raw logits.

Outputs and workspace start as NaN bytes, the logits handed to the device are NaN at every frame t >= T_b and the labels junk
(-1 or V + 7) at every k >= U_b: anything read that must not be read shows.  Tolerances are those of tests/test_gpu_loss_edges.py for
the same arithmetic (fp32 per-frame terms, fp64 lattice sums).  Rows designed to have no path (T_b < U_b + repeats) are the only
ones exempt from the gradient comparison: there the library gives NLL = +inf and an exactly zero gradient row, torch NaN."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import usable_cores

pytestmark = pytest.mark.gpu
NLL_RTOL, GRAD_TOL = 1e-5, 5e-5


@pytest.fixture(autouse=True, scope="module")
def _oracle_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(usable_cores())
    yield
    torch.set_num_threads(before)


def _labels(rng, B, U, V, blank, p_repeat=0.0):
    """(B,U) labels that avoid the blank; y_k repeats y_{k-1} with probability p_repeat, otherwise it differs from it (when the
    vocabulary has a second non-blank entry)."""
    others = np.array([v for v in range(V) if v != blank])
    y = np.zeros((B, U), dtype=np.int32)
    for b in range(B):
        for k in range(U):
            if k and (others.size == 1 or rng.random() < p_repeat):
                y[b, k] = y[b, k - 1]
            else:
                c = others[rng.integers(0, others.size)]
                while k and others.size > 1 and c == y[b, k - 1]:
                    c = others[rng.integers(0, others.size)]
                y[b, k] = c
    return y


def _repeats(y, u):
    return int(sum(y[k] == y[k + 1] for k in range(u - 1)))


def _feasible(y, t_lens, u_lens):
    return [t >= u + _repeats(y[b], u) for b, (t, u) in enumerate(zip(t_lens, u_lens))]


def _oracle(z, y, t_lens, u_lens, blank, gw):
    """float64 NLL (B,) and d(sum_b gw[b] NLL_b)/dz (B,T,V) over the rows that have a path (NaN-free there)."""
    B, T, V = z.shape
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(y, dtype=torch.long) if y is not None and y.shape[1] else torch.ones(B, 1, dtype=torch.long)
    yt = yt.clamp(0, V - 1)
    nll = F.ctc_loss(F.log_softmax(zt, -1).transpose(0, 1), yt, torch.tensor(t_lens), torch.tensor(u_lens), blank=blank,
                     reduction="none", zero_infinity=False)
    ok = torch.tensor(_feasible(yt.numpy(), t_lens, u_lens))
    g = torch.tensor(gw, dtype=torch.float64)
    if ok.any():
        (nll[ok] * g[ok]).sum().backward()
    grad = zt.grad.numpy() if zt.grad is not None else np.zeros_like(z, dtype=np.float64)
    return nll.detach().numpy(), grad


def _poison(z, y, t_lens, u_lens):
    V = z.shape[2]
    z, y = z.copy(), (None if y is None else y.copy())
    for b, (t, u) in enumerate(zip(t_lens, u_lens)):
        z[b, t:] = np.nan
        if y is not None:
            y[b, u:] = [-1 if k % 2 else V + 7 for k in range(y.shape[1] - u)]
    return z, y


def _run(z, y, t_lens, u_lens, blank, layout="bm", upstream=None):
    """-> nll (B,), dz (B,T,V) from the library.  upstream: a list (per-utterance gvec, stride 1), a float (gscale, with a
    one-element gvec [2.0] of stride 0) or None (gvec NULL)."""
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import _addr
    L = _lib.lib()
    B, T, V = z.shape
    U = 0 if y is None else y.shape[1]
    zp, yp = _poison(z, y, t_lens, u_lens)
    if layout == "tm":
        zd, (z_sb, z_st) = torch.from_numpy(zp).transpose(0, 1).contiguous().cuda(), (V, B * V)
    else:
        zd, (z_sb, z_st) = torch.from_numpy(zp).cuda(), (T * V, V)
    yd = torch.from_numpy(yp).cuda() if U else None
    tl = torch.tensor(t_lens, dtype=torch.int32, device="cuda")
    ul = torch.tensor(u_lens, dtype=torch.int32, device="cuda")
    nll = torch.full((B,), float("nan"), device="cuda")
    dz = torch.full_like(zd, float("nan"))
    nws = L.rnnt_hip_ctc_loss_workspace_bytes(B, T, U, V)
    assert nws > 0
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device="cuda")   # all-ones bytes: NaN as fp32 and as fp64
    stream = torch.cuda.current_stream().cuda_stream
    args = (_addr(zd), z_sb, z_st, _addr(yd), _addr(tl), _addr(ul), B, T, U, V, blank)
    _lib.check(L.rnnt_hip_ctc_loss_fwd(*args, _addr(nll), _addr(ws), nws, stream), "ctc fwd")
    if isinstance(upstream, float):
        gscale, gvec, stride = upstream, torch.tensor([2.0], device="cuda"), 0
    elif upstream is None:
        gscale, gvec, stride = 1.0, None, 0
    else:
        gscale, gvec, stride = 1.0, torch.tensor(upstream, dtype=torch.float32, device="cuda"), 1
    _lib.check(L.rnnt_hip_ctc_loss_bwd(*args, gscale, _addr(gvec), stride, _addr(dz), _addr(ws), nws, stream), "ctc bwd")
    torch.cuda.synchronize()
    dz = dz.cpu().numpy()
    return nll.cpu().numpy(), (dz.transpose(1, 0, 2) if layout == "tm" else dz)


def _effective(upstream, B):
    if isinstance(upstream, float):   # gscale * gvec[0] in fp32, as the kernel forms it
        return [float(np.float32(upstream) * np.float32(2.0))] * B
    return [1.0] * B if upstream is None else list(upstream)


def _check(nll, dz, ref_nll, ref_dz, y, t_lens, u_lens, what=""):
    ok = _feasible(y, t_lens, u_lens) if y is not None else [True] * len(t_lens)
    assert not np.isnan(dz).any() and not np.isnan(nll).any(), f"{what}: NaN in the outputs"
    for b, (tb, ub) in enumerate(zip(t_lens, u_lens)):
        assert np.all(dz[b, tb:] == 0), f"{what} dz of padded frames of row {b}"
        if not ok[b]:   # designed to have no path
            assert np.isposinf(nll[b]) and np.isposinf(ref_nll[b]), f"{what} row {b}: nll {nll[b]} (oracle {ref_nll[b]})"
            assert np.all(dz[b] == 0), f"{what} row {b} has no path: its gradient must be exactly zero"
            continue
        print(f"{what} row {b}: nll {nll[b]:.9g} oracle {ref_nll[b]:.9g}")
        np.testing.assert_allclose(nll[b], ref_nll[b], rtol=NLL_RTOL, err_msg=f"{what} row {b}")
        want = ref_dz[b, :tb]
        err = np.abs(dz[b, :tb] - want).max() if tb else 0.0
        print(f"{what} row {b}: gradient err {err:.3g} (max |want| {np.abs(want).max() if tb else 0:.3g})")
        assert err < GRAD_TOL * max(1.0, np.abs(want).max() if tb else 0.0), f"{what} row {b}: gradient err {err}"


def _case(B, T, U, V, blank, t_lens, u_lens, scale=1.0, seed=0, layout="bm", upstream=None, p_repeat=0.0, y=None, what=""):
    rng = np.random.default_rng(seed)
    z = (rng.normal(size=(B, T, V)) * scale).astype(np.float32)
    if y is None and U:
        y = _labels(rng, B, U, V, blank, p_repeat)
    ref = _oracle(z, y, t_lens, u_lens, blank, _effective(upstream, B))
    got = _run(z, y, t_lens, u_lens, blank, layout, upstream)
    _check(*got, *ref, y, t_lens, u_lens, what)
    return z, y, got, ref


@pytest.mark.parametrize("U", [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511])
def test_label_counts_around_the_lane_ownership_switches(U):
    """ctc_sweep_kernel<K>: K = ceil((U+1)/64) positions per lane, instances 1, 2, 3, 4, 8.  V = 5, so equal neighbours are frequent
    (kept at about 40 per row at most, so that T = U + 90 frames leave a path)."""
    T = U + 90
    rng = np.random.default_rng(U)
    y = _labels(rng, 2, U, 5, 0, p_repeat=min(0.3, 40.0 / U))
    t_lens, u_lens = [T, T - 7], [U, max(U // 2, 1)]
    assert all(_feasible(y, t_lens, u_lens))
    _case(2, T, U, 5, 0, t_lens, u_lens, seed=U, y=y, upstream=[1.0, -0.6], layout="tm" if U % 2 else "bm", what=f"U{U}")


@pytest.mark.parametrize("t_lens,u_lens", [([65, 1, 32, 33], [3, 1, 0, 3]), ([64, 2, 31, 65], [1, 1, 3, 0]), ([1, 2, 33, 64], [0, 0, 1, 3])])
def test_frame_counts_around_the_tile(t_lens, u_lens):
    _case(4, 65, 3, 7, 3, t_lens, u_lens, seed=sum(t_lens), upstream=[1.0, 0.5, -0.8, 1.2], what=f"T_b{t_lens}")


def _softmax64(z):
    e = np.exp(z.astype(np.float64) - z.astype(np.float64).max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _single_path_batch(kind, us, short=0):
    """One row per U_b in `us` with one alignment each: `equal` — all labels equal with T_b = 2 U_b - 1 (y, blank, y, ..., y);
    `distinct` — all labels distinct with T_b = U_b (one label per frame).  short = 1 takes one frame away: no path is left."""
    V, blank, U = 64, 9, 40
    y = np.zeros((len(us), U), dtype=np.int32)
    paths = []
    for b, u in enumerate(us):
        if kind == "equal":
            y[b] = 11 + b
            paths.append([11 + b if k % 2 == 0 else blank for k in range(2 * u - 1)])
        else:
            y[b] = [v for v in range(V) if v != blank][:U]
            paths.append(list(y[b, :u]))
    t_lens = [len(p) - short for p in paths]
    return V, blank, U, y, t_lens, list(us), paths


@pytest.mark.parametrize("kind", ["equal", "distinct"])
def test_single_path_lattices(kind):
    """One alignment: NLL = -sum_t lp[t, path_t] and the gradient is softmax - onehot(path_t), as the oracle gives too."""
    V, blank, U, y, t_lens, u_lens, paths = _single_path_batch(kind, [1, 4, 40])
    T = max(t_lens)
    z, _, (nll, dz), _ = _case(3, T, U, V, blank, t_lens, u_lens, seed=5, y=y, what=kind)
    p = _softmax64(z)
    for b, path in enumerate(paths):
        want = p[b, :len(path)].copy()
        want[np.arange(len(path)), path] -= 1.0
        assert np.abs(dz[b, :len(path)] - want).max() < GRAD_TOL
        np.testing.assert_allclose(nll[b], -np.log(p[b, np.arange(len(path)), path]).sum(), rtol=NLL_RTOL)


@pytest.mark.parametrize("kind", ["equal", "distinct"])
def test_rows_without_a_path(kind):
    """The single-path rows with one frame fewer, and T_b = 1 with U_b = 2, next to a row that has paths: NLL = +inf (0 through
    CTCLoss(zero_infinity=True)), an exactly zero gradient row, and the feasible row is bitwise what it is alone."""
    from rnntransducer_amd import CTCLoss
    V, blank, U, y, t_lens, u_lens, _ = _single_path_batch(kind, [4, 40, 2], short=1)
    rng = np.random.default_rng(17)
    y = np.concatenate([y, _labels(rng, 1, U, V, blank)])
    t_lens, u_lens = t_lens[:2] + [1, 50], u_lens + [12]              # row 2: T_b = 1 with U_b = 2
    assert _feasible(y, t_lens, u_lens) == [False, False, False, True]
    gw = [1.0, -0.5, 2.0, 0.7]
    z, _, (nll, dz), _ = _case(4, 80, U, V, blank, t_lens, u_lens, seed=23, y=y, upstream=gw, what=kind)
    assert np.isposinf(nll[:3]).all() and np.all(dz[:3] == 0)
    alone = _run(z[3:], y[3:], t_lens[3:], u_lens[3:], blank, "bm", gw[3:])
    assert np.array_equal(alone[0], nll[3:]) and np.array_equal(alone[1], dz[3:])
    zp, yp = _poison(z, y, t_lens, u_lens)
    zd = torch.from_numpy(zp).cuda().requires_grad_(True)
    lens = [torch.tensor(x, dtype=torch.int32, device="cuda") for x in (t_lens, u_lens)]
    out = CTCLoss(blank=blank, reduction="none", zero_infinity=True)(zd, torch.from_numpy(yp).cuda(), *lens)
    assert torch.all(out[:3] == 0) and out[3].item() == nll[3]
    out.sum().backward()
    assert torch.all(zd.grad[:3] == 0) and not torch.isnan(zd.grad).any()
    plain = CTCLoss(blank=blank, reduction="none")(zd.detach(), torch.from_numpy(yp).cuda(), *lens)
    assert torch.isposinf(plain[:3]).all()


def test_empty_transcripts():
    """U_b = 0 inside a batch, and U = 0 for the whole call (no labels tensor): NLL = -sum_t lp[t, blank]."""
    B, T, V, blank = 3, 40, 11, 4
    t_lens = [40, 1, 33]
    z, y, (nll, _), _ = _case(B, T, 2, V, blank, t_lens, [0, 0, 2], seed=3, upstream=[1.0, 1.0, 0.5], what="U_b=0")
    lp = np.log(_softmax64(z))
    for b in (0, 1):
        np.testing.assert_allclose(nll[b], -lp[b, :t_lens[b], blank].sum(), rtol=NLL_RTOL)
    _, _, (nll0, dz0), _ = _case(B, T, 0, V, blank, t_lens, [0, 0, 0], seed=3, what="U=0")
    for b in range(B):
        np.testing.assert_allclose(nll0[b], -lp[b, :t_lens[b], blank].sum(), rtol=NLL_RTOL)
    assert np.array_equal(nll0[:2], nll[:2])


@pytest.mark.parametrize("V,blank,T,layout", [(2, 0, 33, "bm"), (2, 1, 33, "tm"), (63, 62, 33, "bm"), (64, 0, 33, "tm"), (65, 64, 33, "bm"),
                                              (128, 100, 33, "tm"), (255, 254, 33, "bm"), (256, 70, 33, "tm"), (257, 0, 33, "bm"),
                                              (257, 200, 33, "tm"), (2048, 1000, 40, "bm")])
def test_vocabularies(V, blank, T, layout):
    """Around the 64-lane wave: the blank at 0, at V - 1 and in the middle of a 64-entry tile other than the first; every row carries
    the last entry of the vocabulary (V - 2 when that is the blank) and an entry of the last, partial tile."""
    B, U = 2, 6
    rng = np.random.default_rng(V + blank)
    y = _labels(rng, B, U, V, blank)
    if V > 2:
        tail = [v for v in range(64 * ((V - 1) // 64), V) if v != blank]
        y[:, 0] = V - 1 if blank != V - 1 else V - 2
        if tail:   # (V = 65 with the blank at 64: the blank is the whole partial tile)
            y[:, 2] = tail[len(tail) // 2]
        y[:, 4] = y[:, 0]
    _case(B, T, U, V, blank, [T, 20], [U, 3], seed=V, y=y, layout=layout, upstream=[0.8, -1.1], what=f"V{V}")


@pytest.mark.parametrize("scale", [0.01, 1.0, 30.0])
def test_flat_and_peaked_posteriors(scale):
    """Logit scale 30: most occupancies underflow to 0; no NaN anywhere (checked by _check)."""
    _case(2, 50, 10, 20, 0, [50, 37], [10, 6], scale=scale, seed=8, p_repeat=0.2, upstream=0.37, what=f"scale{scale}")


def test_one_long_chain():
    _case(2, 1500, 80, 72, 0, [1500, 1111], [80, 55], seed=4, p_repeat=0.1, layout="tm", upstream=[1.0, 0.5], what="T1500")


def test_reductions_through_the_module():
    """CTCLoss "none" / "sum" / "mean" with autograd: "mean" is sum_b NLL_b / B (not torch.nn.CTCLoss's)."""
    from rnntransducer_amd import CTCLoss
    B, T, U, V, blank = 3, 45, 7, 30, 0
    t_lens, u_lens = [45, 30, 12], [7, 4, 0]
    rng = np.random.default_rng(12)
    z = rng.normal(size=(B, T, V)).astype(np.float32)
    y = _labels(rng, B, U, V, blank, 0.2)
    zp, yp = _poison(z, y, t_lens, u_lens)
    lens = [torch.tensor(x, dtype=torch.int32, device="cuda") for x in (t_lens, u_lens)]
    for reduction, gw in (("none", [0.6, -1.2, 0.0]), ("sum", [1.0] * B), ("mean", [1.0 / B] * B)):
        ref_nll, ref_dz = _oracle(z, y, t_lens, u_lens, blank, gw)
        zd = torch.from_numpy(zp).cuda().requires_grad_(True)
        out = CTCLoss(blank=blank, reduction=reduction)(zd, torch.from_numpy(yp).cuda(), *lens)
        if reduction == "none":
            np.testing.assert_allclose(out.detach().cpu().numpy(), ref_nll, rtol=NLL_RTOL)
            (out * torch.tensor(gw, device="cuda")).sum().backward()
        else:
            want = float(np.dot(ref_nll, gw))
            assert out.dim() == 0 and abs(out.item() - want) < NLL_RTOL * abs(want)
            out.backward()
        got = zd.grad.cpu().numpy()
        for b in range(B):
            assert np.abs(got[b, :t_lens[b]] - ref_dz[b, :t_lens[b]]).max() < GRAD_TOL * max(1.0, np.abs(ref_dz[b]).max())
            assert np.all(got[b, t_lens[b]:] == 0)
        with torch.no_grad():
            again = CTCLoss(blank=blank, reduction=reduction)(zd, torch.from_numpy(yp).cuda(), *lens)
        assert torch.equal(again, out.detach())


def test_same_bits_twice_and_alone():
    B, T, U, V, blank = 4, 80, 66, 40, 39
    t_lens, u_lens = [80, 64, 33, 80], [40, 20, 8, 66]
    rng = np.random.default_rng(31)
    z = rng.normal(size=(B, T, V)).astype(np.float32)
    y = _labels(rng, B, U, V, blank)
    y[3, ::3] = y[3, 0]                                               # one value at many positions of row 3: a long chain of equal labels
    assert all(_feasible(y, t_lens, u_lens))
    gw = [1.0, -0.3, 0.5, 2.0]
    one, two = _run(z, y, t_lens, u_lens, blank, "bm", gw), _run(z, y, t_lens, u_lens, blank, "bm", gw)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
    _check(*one, *_oracle(z, y, t_lens, u_lens, blank, gw), y, t_lens, u_lens, "bits")
    for b in (1, 3):
        alone = _run(z[b:b + 1], y[b:b + 1], t_lens[b:b + 1], u_lens[b:b + 1], blank, "bm", gw[b:b + 1])
        assert np.array_equal(alone[0], one[0][b:b + 1]) and np.array_equal(alone[1], one[1][b:b + 1])
    tm = _run(z, y, t_lens, u_lens, blank, "tm", gw)                  # the layout changes addresses only
    assert np.array_equal(tm[0], one[0]) and np.array_equal(tm[1], one[1])


# ---- greedy decode -------------------------------------------------------------------------------------------------------------
def _greedy_np(z, t_lens, blank):
    """The rule restated: argmax per frame (numpy: the first of equal maxima), keep frame t's token when it is not the blank and
    differs from frame t-1's argmax; a kept token's frame is the first frame of its run."""
    out = []
    for b, tb in enumerate(t_lens):
        am = z[b, :tb].argmax(-1)
        keep = (am != blank) & (am != np.concatenate(([-1], am[:-1])))
        out.append((am[keep].astype(np.int64), np.nonzero(keep)[0].astype(np.int64)))
    return out


def _greedy_dev(z, t_lens, blank, layout="bm", frames=True):
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import _addr
    L = _lib.lib()
    B, T, V = z.shape
    zp = z.copy()
    for b, tb in enumerate(t_lens):
        zp[b, tb:] = np.nan
    if layout == "tm":
        zd, (z_sb, z_st) = torch.from_numpy(zp).transpose(0, 1).contiguous().cuda(), (V, B * V)
    else:
        zd, (z_sb, z_st) = torch.from_numpy(zp).cuda(), (T * V, V)
    tl = torch.tensor(t_lens, dtype=torch.int32, device="cuda")
    tokens = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    fr = torch.full((B, T), -7, dtype=torch.int32, device="cuda") if frames else None
    counts = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    _lib.check(L.rnnt_hip_ctc_greedy(_addr(zd), z_sb, z_st, _addr(tl), B, T, V, blank, _addr(tokens), _addr(counts), _addr(fr),
                                     torch.cuda.current_stream().cuda_stream), "ctc greedy")
    n = counts.cpu().numpy()
    tokens = tokens.cpu().numpy()
    fr = fr.cpu().numpy() if frames else None
    return [(tokens[b, :n[b]], fr[b, :n[b]] if frames else None) for b in range(B)]   # entries beyond counts[b] are never inspected


def _greedy_check(z, t_lens, blank, layout="bm"):
    want = _greedy_np(z, t_lens, blank)
    for frames in (True, False):
        got = _greedy_dev(z, t_lens, blank, layout, frames)
        for b, ((wt, wf), (gt, gf)) in enumerate(zip(want, got)):
            assert np.array_equal(gt, wt), f"row {b} tokens"
            if frames:
                assert np.array_equal(gf, wf), f"row {b} frames"
    return want


def _runs(rng, B, T, V, winner_of):
    """Logits whose argmax stays on one entry for runs of 1..15 frames."""
    z = rng.normal(size=(B, T, V)).astype(np.float32) * 0.1
    for b in range(B):
        t = 0
        while t < T:
            n = int(rng.integers(1, 16))
            z[b, t:t + n, winner_of(rng)] += 3.0
            t += n
    return z


@pytest.mark.parametrize("T,t_lens,layout", [(200, [200, 1, 63, 64], "bm"), (200, [65, 200, 64, 1], "tm"), (1100, [1100, 1025, 1024, 1023], "bm")])
def test_greedy_long_runs(T, t_lens, layout):
    """V = 3: runs are long and blanks frequent; frame counts around the wave, and past the 1024 frames of one chunk."""
    rng = np.random.default_rng(T)
    z = _runs(rng, 4, T, 3, lambda r: int(r.integers(0, 3)))
    want = _greedy_check(z, t_lens, 1, layout)
    # the case is what it claims: runs average 8 frames, two in three are no blank -- several tokens, far fewer than frames
    assert max(t_lens) // 32 <= max(len(w[0]) for w in want) <= max(t_lens) // 4


def test_greedy_exact_ties_go_to_the_lowest_index():
    """Small integers as logits: maxima that are exactly equal at indices spanning two 64-entry tiles."""
    B, T, V, blank = 2, 12, 130, 0
    z = np.zeros((B, T, V), dtype=np.float32)
    ties = [(5, 70), (63, 64), (64, 129), (0, 129), (70, 5, 128), (129,), (1, 65, 129), (64, 65), (127, 128), (0, 1), (63, 127), (2, 66)]
    for t, idx in enumerate(ties):
        z[0, t, list(idx)] = 3.0
        z[1, t, list(idx)] = -1.0          # row 1: the tie is among all the OTHER entries (zeros): index 0 = blank, or the first untouched
        z[1, t, 0] = -2.0 if t % 2 else 0.0
    want = _greedy_check(z, [T, T], blank)
    assert list(want[0][0][:3]) == [5, 63, 64]
    _greedy_check(z, [T, 7], blank, "tm")


def test_greedy_all_blank_rows_and_large_vocabulary():
    rng = np.random.default_rng(9)
    B, T, V, blank = 3, 70, 2048, 1500
    z = rng.normal(size=(B, T, V)).astype(np.float32)
    z[1, :, blank] += 20.0                                             # an all-blank row: count 0
    want = _greedy_check(z, [70, 70, 33], blank)
    assert len(want[1][0]) == 0 and len(want[0][0]) > 30
    z3 = _runs(rng, 2, 64, 3, lambda r: 2)
    z3[0, :, 2] -= 10.0
    z3[0, :, 0] += 5.0
    want = _greedy_check(z3, [64, 64], 0)
    assert len(want[0][0]) == 0 and list(want[1][0]) == [2]            # one token for the whole utterance: a single run
