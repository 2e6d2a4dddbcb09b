"""Lattice knowledge distillation in the fused RNN-T loss (csrc/loss.hip: the KD instances of lse_sep / lse_sepv / grad_sep /
grad_sepv, kd_value_kernel, rnnt_hip_joint_cell_logprobs) on the device, against the float64 restatement tests/kd_restatement.py
(itself checked on the CPU by tests/test_kd_oracle.py).

The kernels are driven through the C ABI with A, C and bias handed in directly, under both kernel families; outputs and workspace
start as NaN.  Shapes: the six of tests/test_gpu_fastemit.py (tile edges, the V = 256 switch, U+1 = 193 past grad_sep's table, 318 =
two chunks, 512).  Student and teacher operands are drawn independently; the teacher's planes handed to the loss are the
restatement's, rounded to fp32 (the library's own teacher planes are checked against the restatement separately).
Bounds: planes 2e-5 absolute (DENSE_ATOL of the loss tests); kd within NLL_RTOL = 1e-5 of the sum of its |class terms| (the terms
cancel); every gradient entry within GRAD_TOL = 5e-5 of max(1, S), S the entry's own sum of |per-cell contributions|."""
import functools

import numpy as np
import pytest
import torch

from tests import kd_restatement as kr
from tests.test_gpu_fastemit import CASES, FAMILIES, IDS, _problem

pytestmark = pytest.mark.gpu
NLL_RTOL, GRAD_TOL, DENSE_ATOL = 1e-5, 5e-5, 2e-5


@pytest.fixture(params=FAMILIES, ids=("smallv", "largev"))
def family(request, monkeypatch):
    for k in FAMILIES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(request.param, "1")
    return request.param


# per case of CASES: (upstream of the NLL, upstream of kd, FastEmit lambda, student's blank logit raised by).  A list is a
# per-utterance gvec (stride 1); a pair (gscale, g) is a scalar: gscale with a one-element gvec [g] of stride 0.
KD = [
    ([1.3, -0.7], [0.5, 1.1], 0.0, 0.0),
    ((0.37, 2.0), (0.8, 0.5), 0.5, 0.0),        # scalar upstreams, FastEmit on the transducer term
    ([0.0, 0.0], [1.0, 0.5], 0.0, 0.0),         # pure distillation: an NLL upstream of exactly 0
    ([1.0, -0.5], [1.0, 0.7], 0.0, 30.0),       # a peaked student: p(blank) ~ 1 - 1e-12 in every cell
    ([1.0], [0.6], 0.0, 0.0),
    ((0.37, 2.0), (1.0, 1.5), 0.0, 0.0),
]


def _effective(up, B):
    if isinstance(up, tuple):   # gscale * gvec[0] in fp32, as the kernels form it
        return [float(np.float32(up[0]) * np.float32(up[1]))] * B
    return list(up)


@functools.lru_cache(maxsize=None)
def _case(i):
    """Operands, teacher planes (fp32-rounded restatement) and the float64 reference of case i: computed once, shared by both
    families and every test (treated as read-only)."""
    B, T, U1, V, blank, t_lens, u_lens, _, layout, _ = CASES[i]
    g_nll, g_kd, lam, peak = KD[i]
    A, C, bias, y = _problem(B, T, U1, V, blank, seed=T * 1000 + U1 * 10 + V)
    At, Ct, bt, _ = _problem(B, T, U1, V, blank, seed=T * 1000 + U1 * 10 + V + 7)
    if peak:
        A = A.copy()
        A[:, :, blank] += np.float32(peak)
    t_exact = kr.cell_planes(At, Ct, bt, y, u_lens, blank)
    teacher = tuple(x.astype(np.float32) for x in t_exact)
    ref = kr.kd_fused(A, C, bias, y, t_lens, u_lens, blank, tuple(x.astype(np.float64) for x in teacher), _effective(g_nll, B),
                      _effective(g_kd, B), lam)
    return (A, C, bias, y), (At, Ct, bt), t_exact, teacher, ref


class _Dev:
    """The operands of one call on the device, in the layout asked for."""

    def __init__(self, A, C, bias, y, t_lens, u_lens, blank, layout):
        from rnntransducer_amd.ops import _addr
        B, T, V = A.shape
        U1 = C.shape[1]
        self.B, self.T, self.U1, self.V, self.layout = B, T, U1, V, layout
        if layout == "tm":   # what JointLossFn passes: (T,B,V) and (U1,B,V)
            self.a = torch.from_numpy(A).transpose(0, 1).contiguous().cuda()
            self.c = torch.from_numpy(C).transpose(0, 1).contiguous().cuda()
            strides = (V, B * V, V, B * V)
        else:
            self.a, self.c = torch.from_numpy(A).cuda(), torch.from_numpy(C).cuda()
            strides = (T * V, V, U1 * V, V)
        self.keep = (torch.from_numpy(bias).cuda(), torch.from_numpy(np.ascontiguousarray(y)).cuda(),
                     torch.tensor(t_lens, dtype=torch.int32, device="cuda"), torch.tensor(u_lens, dtype=torch.int32, device="cuda"))
        tb, yl, tl, ul = self.keep
        self.args = (_addr(self.a), strides[0], strides[1], _addr(self.c), strides[2], strides[3], _addr(tb), _addr(yl), _addr(tl),
                     _addr(ul), B, T, U1, V, blank)
        self.stream = torch.cuda.current_stream().cuda_stream

    def to_bm(self, x):
        return x.cpu().numpy().transpose(1, 0, 2) if self.layout == "tm" else x.cpu().numpy()


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _planes(d):
    """rnnt_hip_joint_cell_logprobs -> three (B,U1,T) device tensors (NaN before the call)."""
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import _addr
    out = tuple(_nan(d.B, d.U1, d.T) for _ in range(3))
    _lib.check(_lib.lib().rnnt_hip_joint_cell_logprobs(*d.args, *(_addr(x) for x in out), d.stream), "cell_logprobs")
    torch.cuda.synchronize()
    return out


def _up(up):
    """-> (gscale, gvec tensor, stride)"""
    if isinstance(up, tuple):
        return up[0], torch.tensor([up[1]], dtype=torch.float32, device="cuda"), 0
    return 1.0, torch.tensor(up, dtype=torch.float32, device="cuda"), 1


def _run_kd(d, teacher, g_nll, g_kd, lam, split=True):
    """-> nll (B,), kd (B,), dA (B,T,V), dC (B,U1,V) from the KD entries.  teacher: three (B,U1,T) device tensors.  split: the forward
    call, then the backward call with both upstreams; else one fwd_bwd call, whose upstreams are the scalars gscale / kd_gscale."""
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import _addr
    L = _lib.lib()
    nll, kd = _nan(d.B), _nan(d.B)
    dA, dC = torch.full_like(d.a, float("nan")), torch.full_like(d.c, float("nan"))
    nws = L.rnnt_hip_joint_loss_kd_workspace_bytes(d.B, d.T, d.U1, d.V)
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device="cuda")   # all-ones bytes: NaN as fp32 and as fp64
    tp = tuple(_addr(x) for x in teacher)
    if not split:
        _lib.check(L.rnnt_hip_joint_loss_fwd_bwd_kd(*d.args, float(g_nll), lam, *tp, float(g_kd), _addr(nll), _addr(kd), _addr(dA), _addr(dC),
                                                    _addr(ws), nws, d.stream), "fwd_bwd_kd")
    else:
        _lib.check(L.rnnt_hip_joint_loss_fwd_bwd_kd(*d.args, 1.0, lam, *tp, 1.0, _addr(nll), _addr(kd), None, None, _addr(ws), nws, d.stream),
                   "fwd_kd")
        (gs, gv, gst), (ks, kv, kst) = _up(g_nll), _up(g_kd)
        _lib.check(L.rnnt_hip_joint_loss_bwd_kd(*d.args, gs, lam, _addr(gv), gst, *tp, ks, _addr(kv), kst, _addr(dA), _addr(dC), _addr(ws),
                                                nws, d.stream), "bwd_kd")
    torch.cuda.synchronize()
    return nll.cpu().numpy(), kd.cpu().numpy(), d.to_bm(dA), d.to_bm(dC)


def _run_plain(d, g_nll, lam):
    """nll, dA, dC of the entries without KD on the same operands (forward, then backward)."""
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import _addr
    L = _lib.lib()
    nll = _nan(d.B)
    dA, dC = torch.full_like(d.a, float("nan")), torch.full_like(d.c, float("nan"))
    nws = L.rnnt_hip_joint_loss_workspace_bytes(d.B, d.T, d.U1, d.V)
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device="cuda")
    _lib.check(L.rnnt_hip_joint_loss_fwd_bwd_fastemit(*d.args, 1.0, lam, _addr(nll), None, None, _addr(ws), nws, d.stream), "fwd")
    gs, gv, gst = _up(g_nll)
    _lib.check(L.rnnt_hip_joint_loss_bwd_fastemit(*d.args, gs, lam, _addr(gv), gst, _addr(dA), _addr(dC), _addr(ws), nws, d.stream), "bwd")
    torch.cuda.synchronize()
    return nll.cpu().numpy(), d.to_bm(dA), d.to_bm(dC)


def _check_planes(got, want, what):
    for name, x, w in zip(("blk", "emit", "rest"), got, want):
        x = x.cpu().numpy()
        assert np.isfinite(x).all(), f"{what} {name}: not finite"
        err = np.abs(x - w).max()
        print(f"{what} plane {name}: err {err:.3e} bound {DENSE_ATOL:.1e} (min {w.min():.2f})")
        assert err < DENSE_ATOL, f"{what} {name}: err {err}"


def _check_grads(got, ref, t_lens, u_lens, what):
    worst = 0.0
    for name, x, want, S in (("dA", got[0], ref["dA"], ref["S_A"]), ("dC", got[1], ref["dC"], ref["S_C"])):
        assert np.isfinite(x).all(), f"{what} {name}: not finite"
        ratio = (np.abs(x - want) / (GRAD_TOL * np.maximum(1.0, S))).max()
        print(f"{what} {name}: largest error / bound {ratio:.3f} (largest |entry| {np.abs(want).max():.3e}, largest S {S.max():.3e})")
        worst = max(worst, ratio)
    assert worst < 1.0, f"{what}: a gradient entry is {worst:.3f} times its bound"
    for b, (tb, ub) in enumerate(zip(t_lens, u_lens)):   # exact zeros outside the utterance's lattice
        assert np.all(got[0][b, tb:] == 0), f"{what} dA of padded frames of row {b}"
        assert np.all(got[1][b, ub + 1:] == 0), f"{what} dC of label positions beyond u_len of row {b}"


def _check_kd(kd, ref, what):
    bound = NLL_RTOL * ref["kd_mag"]
    print(f"{what} kd: {kd} ref {ref['kd']} err/bound {(np.abs(kd - ref['kd']) / bound).max():.3f}")
    assert np.all(np.abs(kd - ref["kd"]) <= bound), f"{what} kd {kd} vs {ref['kd']} (bound {bound})"


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_kd_loss_matches_restatement(family, case):
    """1. Planes (the teacher's and the student's own, the peaked student included), the NLL bitwise the plain entry's, kd, dA and dC
    (forward call then backward call, both upstreams) and exact zeros on the padding, for every kernel form."""
    B, T, U1, V, blank, t_lens, u_lens, _, layout, _ = CASES[case]
    g_nll, g_kd, lam, peak = KD[case]
    (A, C, bias, y), (At, Ct, bt), t_exact, teacher, ref = _case(case)
    d = _Dev(A, C, bias, y, t_lens, u_lens, blank, layout)
    _check_planes(_planes(_Dev(At, Ct, bt, y, t_lens, u_lens, blank, layout)), t_exact, f"{family} teacher")
    _check_planes(_planes(d), ref["planes"], f"{family} student")
    if peak:
        assert np.median(ref["planes"][2]) < -20.0      # the case is what it says: 1 - p_b - p_y is all rounding error in most cells
    nll, kd, dA, dC = _run_kd(d, tuple(torch.from_numpy(x).cuda() for x in teacher), g_nll, g_kd, lam)
    plain_nll, _, _ = _run_plain(d, g_nll, lam)
    assert not np.isnan(nll).any() and np.array_equal(nll, plain_nll)
    np.testing.assert_allclose(nll, ref["nll"], rtol=NLL_RTOL)
    _check_kd(kd, ref, family)
    _check_grads((dA, dC), ref, t_lens, u_lens, family)


@pytest.mark.parametrize("case", [0, 2, 4], ids=[IDS[i] for i in (0, 2, 4)])
def test_fused_call(family, case):
    """2. One fwd_bwd_kd call (scalar upstreams gscale, kd_gscale) in the other layout: the same values."""
    B, T, U1, V, blank, t_lens, u_lens, _, layout, _ = CASES[case]
    (A, C, bias, y), _, _, teacher, _ = _case(case)
    layout = "bm" if layout == "tm" else "tm"
    gn, gk = (0.0, 1.0) if case == 2 else (0.75, 0.4)
    ref = kr.kd_fused(A, C, bias, y, t_lens, u_lens, blank, tuple(x.astype(np.float64) for x in teacher), [gn] * B, [gk] * B, 0.0)
    d = _Dev(A, C, bias, y, t_lens, u_lens, blank, layout)
    nll, kd, dA, dC = _run_kd(d, tuple(torch.from_numpy(x).cuda() for x in teacher), gn, gk, 0.0, split=False)
    np.testing.assert_allclose(nll, ref["nll"], rtol=NLL_RTOL)
    _check_kd(kd, ref, family)
    _check_grads((dA, dC), ref, t_lens, u_lens, f"{family} fused")


@pytest.mark.parametrize("case", [0, 2, 3], ids=[IDS[i] for i in (0, 2, 3)])
def test_teacher_equal_to_student(family, case):
    """3. The student's own planes as the teacher's: kd at most 1e-5 per cell of the row, and the gradient is the plain call's scaled
    gradient (the KD scalars vanish) within GRAD_TOL."""
    B, T, U1, V, blank, t_lens, u_lens, _, layout, _ = CASES[case]
    (A, C, bias, y), _, _, _, _ = _case(case)
    d = _Dev(A, C, bias, y, t_lens, u_lens, blank, layout)
    g_nll = [1.3, -0.7]
    nll, kd, dA, dC = _run_kd(d, _planes(d), g_nll, [1.0, 2.0], 0.0)
    _, pA, pC = _run_plain(d, g_nll, 0.0)
    for b in range(B):
        print(f"{family} row {b}: kd {kd[b]:.3e} bound {1e-5 * t_lens[b] * (u_lens[b] + 1):.3e}")
        assert abs(kd[b]) <= 1e-5 * t_lens[b] * (u_lens[b] + 1)
    for name, x, want in (("dA", dA, pA), ("dC", dC, pC)):
        err, bound = np.abs(x - want).max(), GRAD_TOL * max(1.0, np.abs(want).max())
        print(f"{family} {name}: err {err:.3e} bound {bound:.3e}")
        assert err < bound


@pytest.mark.parametrize("case", [0, 3], ids=[IDS[i] for i in (0, 3)])
def test_rows_alone_and_twice(family, case):
    """4. Two runs give the same bits; a row alone gives the bits it gives in the batch (kd, nll, its dA and dC rows)."""
    B, T, U1, V, blank, t_lens, u_lens, _, layout, _ = CASES[case]
    g_nll, g_kd, lam, _ = KD[case]
    (A, C, bias, y), _, _, teacher, _ = _case(case)
    full = _run_kd(_Dev(A, C, bias, y, t_lens, u_lens, blank, layout), tuple(torch.from_numpy(x).cuda() for x in teacher), g_nll, g_kd, lam)
    again = _run_kd(_Dev(A, C, bias, y, t_lens, u_lens, blank, layout), tuple(torch.from_numpy(x).cuda() for x in teacher), g_nll, g_kd, lam)
    for a, b in zip(full, again):
        assert not np.isnan(a).any() and np.array_equal(a, b)
    for r in range(B):
        one = _run_kd(_Dev(A[r:r + 1], C[r:r + 1], bias, y[r:r + 1], t_lens[r:r + 1], u_lens[r:r + 1], blank, layout),
                      tuple(torch.from_numpy(np.ascontiguousarray(x[r:r + 1])).cuda() for x in teacher), g_nll[r:r + 1], g_kd[r:r + 1], lam)
        for a, b in zip(full, one):
            assert np.array_equal(a[r:r + 1], b), f"row {r}"


def test_rows_without_cells_and_teacher_zero_classes(family):
    """5. t_lens[b] = 0: kd = 0, nll = +inf, exact-zero gradient rows, the other rows bitwise those of a batch without that row.  A
    teacher plane entry of -inf (P_T = 0) contributes exactly 0: kd stays finite and equals the value without that class."""
    B, T, U1, V, blank = 3, 33, 9, 65, 64
    A, C, bias, y = _problem(B, T, U1, V, blank, seed=11)
    At, Ct, bt, _ = _problem(B, T, U1, V, blank, seed=12)
    t_lens, u_lens, g_nll, g_kd = [T, 0, T - 7], [U1 - 1, 3, U1 // 2], [1.0, 0.5, -0.8], [0.5, 1.0, 2.0]
    teacher = tuple(x.astype(np.float32) for x in kr.cell_planes(At, Ct, bt, y, u_lens, blank))
    teacher[1][0, 2] = -np.inf                     # row 0 never emits label 2
    td = tuple(torch.from_numpy(x).cuda() for x in teacher)
    nll, kd, dA, dC = _run_kd(_Dev(A, C, bias, y, t_lens, u_lens, blank, "bm"), td, g_nll, g_kd, 0.0)
    assert np.isposinf(nll[1]) and kd[1] == 0.0 and np.all(dA[1] == 0) and np.all(dC[1] == 0)
    keep = [0, 2]
    sub = _run_kd(_Dev(A[keep], C[keep], bias, y[keep], [t_lens[k] for k in keep], [u_lens[k] for k in keep], blank, "bm"),
                  tuple(torch.from_numpy(np.ascontiguousarray(x[keep])).cuda() for x in teacher), [g_nll[k] for k in keep],
                  [g_kd[k] for k in keep], 0.0)
    for full, part in zip((nll, kd, dA, dC), sub):
        assert np.array_equal(full[keep], part)
    ref = kr.kd_fused(A[keep], C[keep], bias, y[keep], [t_lens[k] for k in keep], [u_lens[k] for k in keep], blank,
                      tuple(x[keep].astype(np.float64) for x in teacher), [g_nll[k] for k in keep], [g_kd[k] for k in keep])
    assert np.isfinite(kd).all() and np.isfinite(dA).all() and np.isfinite(dC).all()
    _check_kd(sub[1], ref, family)
    _check_grads(sub[2:], ref, [t_lens[k] for k in keep], [u_lens[k] for k in keep], family)
