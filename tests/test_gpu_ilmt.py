"""The internal-LM loss kernels (csrc/ilm_loss.hip: ilm_fwd_kernel, ilm_bwd_kernel) through the C ABI against the float64
restatement of their definition (tests/ilmt_restatement.py), on the same fp32 inputs.

Outputs start as NaN, C handed to the device is NaN in every row u >= u_lens[b] and the labels junk (-1 or V + 7) at every
k >= u_lens[b]: anything read that must not be read shows.  Tolerances are the project's own for its other log-softmax loss
(tests/test_gpu_ctc.py): 1e-5 relative on the per-utterance NLL, 5e-5 * max(1, |want|max) on the gradient.  The largest errors seen
are printed (DESIGN.md §26 records them)."""
import numpy as np
import pytest
import torch

from tests.conftest import usable_cores
from tests.ilmt_restatement import ilm_restatement

pytestmark = pytest.mark.gpu
NLL_RTOL, GRAD_TOL = 1e-5, 5e-5
PAD = 5                      # "pad" layout: c_su = V + PAD
WORST = {"nll": 0.0, "grad": 0.0}


@pytest.fixture(autouse=True, scope="module")
def _oracle_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(usable_cores())
    yield
    torch.set_num_threads(before)
    print(f"largest errors seen: nll relative {WORST['nll']:.3g}, gradient {WORST['grad']:.3g} (of max(1, |want|max))")


def _labels(rng, B, U, V, blank):
    others = np.array([v for v in range(V) if v != blank], dtype=np.int32)
    return others[rng.integers(0, others.size, size=(B, U))].astype(np.int32).reshape(B, U)


def _poison(C, y, u_lens):
    V = C.shape[2]
    C, y = C.copy(), y.copy()
    for b, u in enumerate(u_lens):
        C[u:, b] = np.nan
        y[b, u:] = [-1 if k % 2 else V + 7 for k in range(y.shape[1] - u)]
    return C, y


def _to_layout(x, layout, fill):
    """x (U1,B,V) numpy -> device buffer in `layout`, (c_sb, c_su)."""
    U1, B, V = x.shape
    if layout == "tm":
        return torch.from_numpy(np.ascontiguousarray(x)).cuda(), (V, B * V)
    if layout == "bm":
        return torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).cuda(), (U1 * V, V)
    buf = np.full((B, U1, V + PAD), fill, dtype=np.float32)
    buf[:, :, :V] = x.transpose(1, 0, 2)
    return torch.from_numpy(buf).cuda(), (U1 * (V + PAD), V + PAD)


def _from_layout(t, layout, V):
    a = t.cpu().numpy()
    if layout == "tm":
        return a
    return a[:, :, :V].transpose(1, 0, 2)


def _upstream(upstream):
    if isinstance(upstream, float):
        return upstream, torch.tensor([2.0], device="cuda"), 0
    if upstream is None:
        return 1.0, None, 0
    return 1.0, torch.tensor(upstream, dtype=torch.float32, device="cuda"), 1


def _effective(upstream, B):
    if isinstance(upstream, float):   # gscale * gvec[0] in fp32, as the kernel forms it
        return [float(np.float32(upstream) * np.float32(2.0))] * B
    return [1.0] * B if upstream is None else list(upstream)


def _run(C, bias, y, u_lens, blank, layout="tm", upstream=None, use_lse=True, prefill=None, poison=True):
    """-> nll (B,), dC (U1,B,V), lse (U1,B) from the library.  prefill (U1,B,V): accumulate = 1 into it; None: accumulate = 0 into
    NaN.  use_lse False: the backward gets lse = NULL and recomputes."""
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import _addr
    L = _lib.lib()
    U1, B, V = C.shape
    Cp, yp = _poison(C, y, u_lens) if poison else (C, y)
    Cd, (c_sb, c_su) = _to_layout(Cp, layout, np.nan)
    bd = torch.from_numpy(bias).cuda()
    yd = torch.from_numpy(yp).cuda() if y.shape[1] else torch.zeros(B, 1, dtype=torch.int32, device="cuda")
    ul = torch.tensor(u_lens, dtype=torch.int32, device="cuda")
    nll = torch.full((B,), float("nan"), device="cuda")
    lse = torch.full((U1 * B,), float("nan"), device="cuda")
    if prefill is None:
        dC = torch.full_like(Cd, float("nan"))
    else:
        dC, _ = _to_layout(prefill, layout, 7.25)
    stream = torch.cuda.current_stream().cuda_stream
    head = (_addr(Cd), c_sb, c_su, _addr(bd), _addr(yd), _addr(ul))
    _lib.check(L.rnnt_hip_ilm_loss_fwd(*head, B, U1, V, blank, _addr(nll), _addr(lse), stream), "ilm fwd")
    gscale, gvec, stride = _upstream(upstream)
    _lib.check(L.rnnt_hip_ilm_loss_bwd(*head, _addr(lse) if use_lse else None, B, U1, V, blank, gscale, _addr(gvec), stride,
                                       0 if prefill is None else 1, _addr(dC), stream), "ilm bwd")
    torch.cuda.synchronize()
    if layout == "pad":     # the padding behind every row is nobody's to write
        tail = dC.cpu().numpy()[:, :, V:]
        assert np.isnan(tail).all() if prefill is None else np.all(tail == np.float32(7.25))
    return nll.cpu().numpy(), _from_layout(dC, layout, V), lse.cpu().numpy().reshape(U1, B)


def _check(nll, dC, lse, C, bias, y, u_lens, blank, upstream, what=""):
    U1, B, V = C.shape
    ref_nll, ref_dC, ref_lse = (t.numpy() for t in ilm_restatement(C, bias, y, u_lens, blank, _effective(upstream, B)))
    assert not np.isnan(dC).any() and not np.isnan(nll).any(), f"{what}: NaN in the outputs"
    assert np.all(dC[..., blank] == 0), f"{what}: blank column"
    for b, ub in enumerate(u_lens):
        assert np.all(dC[ub:, b] == 0), f"{what}: uncounted rows of utterance {b}"
        assert np.isnan(lse[ub:, b]).all(), f"{what}: lse of uncounted rows is not written"
        if np.isposinf(ref_nll[b]):
            assert np.isposinf(nll[b]) and np.all(dC[:, b] == 0), f"{what}: infeasible utterance {b}"
            continue
        np.testing.assert_allclose(nll[b], ref_nll[b], rtol=NLL_RTOL, atol=0, err_msg=f"{what} utterance {b}")
        if ref_nll[b] != 0:
            WORST["nll"] = max(WORST["nll"], abs(nll[b] - ref_nll[b]) / abs(ref_nll[b]))
        if ub:
            np.testing.assert_allclose(lse[:ub, b], ref_lse[:ub, b], rtol=NLL_RTOL, atol=1e-6, err_msg=f"{what} lse {b}")
        want = ref_dC[:, b]
        scale = max(1.0, np.abs(want).max())
        err = np.abs(dC[:, b] - want).max()
        WORST["grad"] = max(WORST["grad"], err / scale)
        assert err < GRAD_TOL * scale, f"{what} utterance {b}: gradient err {err} (scale {scale})"
    return ref_nll


def _inputs(seed, U1, B, V, blank, scale=2.0):
    rng = np.random.default_rng(seed)
    C = (rng.normal(size=(U1, B, V)) * scale).astype(np.float32)
    bias = rng.normal(size=(V,)).astype(np.float32)
    y = _labels(rng, B, U1 - 1, V, blank)
    return rng, C, bias, y


def _ragged(rng, B, U):
    """u_lens with U first, then 0, then anything."""
    return ([U, 0] + [int(rng.integers(0, U + 1)) for _ in range(B)])[:B]


@pytest.mark.parametrize("V", [2, 3, 63, 64, 65, 72, 257, 2048, 2049])
def test_shapes_layouts_and_blank_positions(V):
    """Every V x U1 in {1, 2, 5, 41} x B in {1, 3}; layouts, blank positions and upstream forms cycle over the combinations so that
    each V meets all of them.  Per combination also: lse = NULL recomputes the same bits, and a second call returns the same bits."""
    n = 0
    for U1 in (1, 2, 5, 41):
        for B in (1, 3):
            blank = (0, V - 1, V // 2)[n % 3]
            layout = ("tm", "bm", "pad")[(n + n // 3) % 3]
            rng, C, bias, y = _inputs(1000 * V + n, U1, B, V, blank)
            u_lens = _ragged(rng, B, U1 - 1)
            upstream = (None, 0.125, [float(x) for x in rng.normal(size=B)])[(n + 2 * (n // 3)) % 3]
            what = f"V={V} U1={U1} B={B} blank={blank} {layout}"
            nll, dC, lse = _run(C, bias, y, u_lens, blank, layout, upstream)
            _check(nll, dC, lse, C, bias, y, u_lens, blank, upstream, what)
            nll2, dC2, _ = _run(C, bias, y, u_lens, blank, layout, upstream, use_lse=False)
            assert nll2.tobytes() == nll.tobytes() and dC2.tobytes() == dC.tobytes(), f"{what}: lse = NULL / second call"
            n += 1


STRESS_V = [3, 72, 2049]


def _stress(kind, V, blank, seed):
    U1, B = 5, 3
    rng, C, bias, y = _inputs(seed, U1, B, V, blank, scale=1.0)
    if kind == "equal":
        C[:], bias[:] = 1.5, -0.25
    elif kind == "one_high":      # one entry +90 above the rest; never the label (see the test's docstring) nor the blank
        for u in range(U1 - 1):
            for b in range(B):
                free = [v for v in range(V) if v != blank and v != y[b, u]]
                C[u, b, free[int(rng.integers(0, len(free)))]] += 90.0
    elif kind == "label_low":     # the label's logit 90 below the rest
        for u in range(U1 - 1):
            for b in range(B):
                C[u, b, y[b, u]] -= 90.0
    elif kind == "blank_high":    # every non-blank logit at -80, the blank's at +80: the blank must be ignored
        C[:], bias[:] = -80.0, 0.0
        C[..., blank] = 80.0
    return C, bias, y, [U1 - 1, 2, 3]


@pytest.mark.parametrize("V", STRESS_V)
@pytest.mark.parametrize("kind", ["equal", "one_high", "label_low", "blank_high"])
def test_rows_that_stress_the_max_subtraction(kind, V):
    """In "one_high" the +90 entry is a non-label token: were it the label, the row's NLL would be about V e^-90, below what fp32
    resolves next to logits of size 90, and a purely relative bound on it would test nothing the format can deliver."""
    blank = V // 2
    C, bias, y, u_lens = _stress(kind, V, blank, seed=V + len(kind))
    upstream = [1.0, -0.5, 2.0]
    for layout in ("tm", "pad"):
        nll, dC, lse = _run(C, bias, y, u_lens, blank, layout, upstream)
        ref = _check(nll, dC, lse, C, bias, y, u_lens, blank, upstream, f"{kind} V={V} {layout}")
    if kind in ("equal", "blank_high"):
        np.testing.assert_allclose(ref, [u * np.log(V - 1) for u in u_lens], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("blank", [0, 1])
def test_a_single_non_blank_token_gives_exact_zeros(blank):
    rng, C, bias, y = _inputs(3 + blank, 6, 3, 2, blank, scale=30.0)
    u_lens = [5, 0, 3]
    for upstream in (None, [3.0, -2.0, 1e6]):
        nll, dC, _ = _run(C, bias, y, u_lens, blank, "bm", upstream)
        assert np.all(nll == 0) and np.all(dC == 0)
        pre = rng.normal(size=C.shape).astype(np.float32)
        _, acc, _ = _run(C, bias, y, u_lens, blank, "bm", upstream, prefill=pre)
        assert acc.tobytes() == pre.tobytes()


@pytest.mark.parametrize("V", [72, 2049])
@pytest.mark.parametrize("bad", ["blank", "V", "-1"])
def test_an_invalid_counted_label_makes_its_utterance_infeasible(bad, V):
    blank, U1, B = 7, 6, 3
    rng, C, bias, y = _inputs(V + len(bad), U1, B, V, blank)
    u_lens = [5, 4, 3]
    upstream = [1.5, 0.5, -1.0]
    good = _run(C, bias, y, u_lens, blank, "tm", upstream)
    yb = y.copy()
    yb[1, 2] = {"blank": blank, "V": V, "-1": -1}[bad]
    nll, dC, lse = _run(C, bias, yb, u_lens, blank, "tm", upstream)
    _check(nll, dC, lse, C, bias, yb, u_lens, blank, upstream, f"bad label {bad}")
    assert np.isposinf(nll[1]) and np.all(dC[:, 1] == 0)
    for b in (0, 2):                                            # the other utterances: not a bit changes
        assert nll[b].tobytes() == good[0][b].tobytes() and dC[:, b].tobytes() == good[1][:, b].tobytes()
    pre = rng.normal(size=C.shape).astype(np.float32)
    _, acc, _ = _run(C, bias, yb, u_lens, blank, "tm", upstream, prefill=pre)
    assert acc[:, 1].tobytes() == pre[:, 1].tobytes()           # accumulate = 1: the infeasible utterance's rows stay as they were


@pytest.mark.parametrize("layout", ["tm", "bm", "pad"])
@pytest.mark.parametrize("V", [65, 2049])
def test_accumulate_adds_one_rounded_value_per_counted_cell(V, layout):
    blank, U1, B = V - 1, 5, 3
    rng, C, bias, y = _inputs(V, U1, B, V, blank)
    u_lens = [4, 0, 2]
    upstream = [0.7, 1.0, -1.3]
    _, plain, _ = _run(C, bias, y, u_lens, blank, layout, upstream)
    pre = (rng.normal(size=C.shape) * 0.1).astype(np.float32)
    _, acc, _ = _run(C, bias, y, u_lens, blank, layout, upstream, prefill=pre)
    want = pre.copy()
    for b, ub in enumerate(u_lens):
        want[:ub, b] = pre[:ub, b] + plain[:ub, b]              # fp32 + fp32, rounded once
    want[..., blank] = pre[..., blank]
    assert acc.tobytes() == want.tobytes()
    assert acc[..., blank].tobytes() == pre[..., blank].tobytes() and acc[4:].tobytes() == pre[4:].tobytes()


@pytest.mark.parametrize("V", [72, 2049])
def test_an_utterance_alone_gives_the_bits_it_gives_in_a_batch(V):
    blank, U1, B = 0, 41, 3
    rng, C, bias, y = _inputs(V + 1, U1, B, V, blank)
    u_lens = [40, 17, 33]
    upstream = [1.0, 0.25, -3.0]
    nll, dC, lse = _run(C, bias, y, u_lens, blank, "tm", upstream)
    for b in range(B):
        n1, d1, l1 = _run(C[:, b:b + 1], bias, y[b:b + 1], u_lens[b:b + 1], blank, "tm", upstream[b:b + 1])
        assert n1[0].tobytes() == nll[b].tobytes() and d1[:, 0].tobytes() == dC[:, b].tobytes()
        assert l1[:u_lens[b], 0].tobytes() == lse[:u_lens[b], b].tobytes()
