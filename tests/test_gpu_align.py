"""GPU tests of the forced alignment (rnnt_hip_joint_align / rnnt_hip_align_from_logits_ex, JointNet.align, rnnt_align) against
the float64 restatement in tests/align_restatement.py.

Rules, per utterance (TOL = NLL_RTOL * |best float64 score|, NLL_RTOL = 1e-5 as tests/test_gpu_loss.py uses for nll: a path
score is a sum of the same per-cell terms whose log-sum-exp is nll):
  * the returned path is valid: frames non-decreasing in u, inside [0, t_lens[b]), -1 past u_lens[b];
  * the returned score equals the float64 score of THAT path within TOL;
  * that float64 score is at least the restatement's best minus TOL (optimality);
  * where the float64 margin (best minus second-best path) exceeds 2 TOL, the frames equal the restatement's exactly;
  * at most one utterance in ten of a test's set may lie below that margin — a property of the float64 side alone, fixed by the
    seeds and scales chosen here and asserted.
Inputs.  `random_sep`: unit-variance A, C, bias (small lattices only: on a long lattice of random terms the second-best path
is closer to the best than fp32 cell terms can resolve).  `scheduled_sep`: the blank's logit leads the V - 1 labels together by
BLANK_LEAD (p(blank) about 0.8 on a free frame, so every frame of every path costs about 0.2: no path score is so close to 0 that
a tolerance relative to it falls below what an fp32 log-sum-exp of magnitude 5 .. 15 resolves), and every label has one frame
where its logit leads the blank by LABEL_LEAD, so moving one label costs about LABEL_LEAD while |best| is about 0.2 T +
LABEL_LEAD U: relative margins of 1e-3 and more at any lattice size.  Noise of standard deviation NOISE on A and bias; NOISE_C on C
is small on purpose: the blank term of a free frame moves with C[u, blank] by (1 - p(blank)) of it, and on T >> U lattices a path
can collect that difference over hundreds of frames by waiting in a favourable label row, which with noise of 0.25 there outweighs
any label's lead (found on the float64 side alone: relative margins of 1e-6 .. 8e-6 at T = 1000).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_restatement as ar  # noqa: E402

pytestmark = pytest.mark.gpu

NLL_RTOL = 1e-5
BLANK_LEAD, LABEL_LEAD, NOISE, NOISE_C = 1.5, 8.0, 0.25, 0.01
I32 = dict(dtype=torch.int32)


# ---- inputs (numpy float32 values; the float64 side reads the same float32 numbers) ----
def _lengths(rng, B, T, U, ragged):
    if not ragged:
        return [T] * B, [U] * B
    t = [T] + [int(x) for x in rng.integers(max(1, T // 2), T + 1, size=B - 1)]
    u = [U] + [int(x) for x in rng.integers(0, U + 1, size=B - 1)]
    return t, u


def random_sep(seed, B, T, U, V, blank=0, ragged=True):
    rng = np.random.default_rng(seed)
    A, C, bias = (rng.normal(size=s).astype(np.float32) for s in ((B, T, V), (B, U + 1, V), (V,)))
    vals = np.array([v for v in range(V) if v != blank])
    labels = vals[rng.integers(0, len(vals), size=(B, U))].astype(np.int32)
    t_lens, u_lens = _lengths(rng, B, T, U, ragged)
    return A, C, bias, labels, t_lens, u_lens


def scheduled_sep(seed, B, T, U, V, blank=0, ragged=True):
    rng = np.random.default_rng(seed)
    A, C, bias = ((n * rng.normal(size=s)).astype(np.float32) for n, s in ((NOISE, (B, T, V)), (NOISE_C, (B, U + 1, V)), (NOISE, (V,))))
    vals = np.array([v for v in range(V) if v != blank])
    labels = np.tile(vals[np.arange(U) % len(vals)].astype(np.int32), (B, 1))   # neighbours differ (V > 2)
    t_lens, u_lens = _lengths(rng, B, T, U, ragged)
    blank_boost = float(np.log(max(V - 1, 1))) + BLANK_LEAD
    A[:, :, blank] += blank_boost
    for b in range(B):
        f = np.sort(rng.choice(t_lens[b], size=u_lens[b], replace=False) if u_lens[b] <= t_lens[b]
                    else rng.integers(0, t_lens[b], size=u_lens[b]))
        A[b, f, labels[b, :u_lens[b]]] += blank_boost + LABEL_LEAD
    return A, C, bias, labels, t_lens, u_lens


def known_answer_sep(f_rows, T, V, blank):
    """Label u (all labels of a row distinct) can only be emitted at frame f_rows[b][u]: its logit is 40 there and 0 elsewhere,
    the blank's is 20 everywhere.  Every frame charges the same blank whatever the label row, so the best path is f exactly."""
    B, U = len(f_rows), max(len(f) for f in f_rows)
    vals = [v for v in range(V) if v != blank]
    assert U <= len(vals)
    A, C, bias = np.zeros((B, T, V), np.float32), np.zeros((B, U + 1, V), np.float32), np.zeros(V, np.float32)
    labels = np.tile(np.array(vals[:U], np.int32), (B, 1))
    A[:, :, blank] = 20.0
    for b, f in enumerate(f_rows):
        for u, t in enumerate(f):
            A[b, t, labels[b, u]] = 40.0
    return A, C, bias, labels, [T] * B, [len(f) for f in f_rows]


# ---- device calls ----
def _dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def run_fused(A, C, bias, labels, t_lens, u_lens, blank, rows=None):
    from rnntransducer_amd import ops
    sl = slice(None) if rows is None else rows
    res = ops.joint_align(_dev(A[sl]), _dev(C[sl]), _dev(bias), _dev(labels[sl]), _dev(np.array(t_lens)[sl], torch.int32),
                          _dev(np.array(u_lens)[sl], torch.int32), blank, batch_first=True)
    torch.cuda.synchronize()
    return res.frames.cpu().numpy(), res.score.cpu().numpy(), res


def run_dense(logits_dev, labels, t_lens, u_lens, blank):
    from rnntransducer_amd.loss import rnnt_align
    res = rnnt_align(logits_dev, _dev(labels), _dev(np.array(t_lens), torch.int32), _dev(np.array(u_lens), torch.int32), blank)
    torch.cuda.synchronize()
    return res.frames.cpu().numpy(), res.score.cpu().numpy(), res


def fused_nll(A, C, bias, labels, t_lens, u_lens, blank):
    """nll of the existing fused loss (forward only) on the same operands."""
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import _addr, _stream, check
    B, T, V = A.shape
    U1 = C.shape[1]
    dA, dC, db, dl, dt, du = _dev(A), _dev(C), _dev(bias), _dev(labels), _dev(np.array(t_lens), torch.int32), _dev(np.array(u_lens), torch.int32)
    nll = torch.empty(B, device="cuda")
    nws = _lib.lib().rnnt_hip_joint_loss_workspace_bytes(B, T, U1, V)
    ws = torch.empty(nws, device="cuda", dtype=torch.uint8)
    check(_lib.lib().rnnt_hip_joint_loss_fwd_bwd(_addr(dA), T * V, V, _addr(dC), U1 * V, V, _addr(db), _addr(dl), _addr(dt), _addr(du),
                                                 B, T, U1, V, blank, 1.0, _addr(nll), None, None, _addr(ws), nws, _stream()), "loss")
    torch.cuda.synchronize()
    return nll.cpu().numpy().astype(np.float64)


# ---- the rules ----
def check_utterance(tag, blk, emit, Tb, Ub, got_row, got_score):
    """-> True when the utterance lies below the margin (covered by the optimality check only)."""
    U = len(got_row)
    got = [int(x) for x in got_row[:Ub]]
    assert all(int(x) == -1 for x in got_row[Ub:]), f"{tag}: frames past u_lens are not -1: {got_row[Ub:]}"
    assert got == sorted(got) and all(0 <= f < Tb for f in got), f"{tag}: invalid path {got} (Tb = {Tb})"
    want, best, M = ar.viterbi(blk, emit, Tb, Ub)
    mg = ar.margin(want, best, M)
    tol = NLL_RTOL * abs(best)
    ps = ar.path_score(blk, emit, got, Tb)
    print(f"{tag}: T={Tb} U={Ub} of {U} best={best:.6f} device={got_score:.6f} |device - path64|={abs(got_score - ps):.3e} "
          f"best - path64={best - ps:.3e} tol={tol:.3e} margin={mg:.3e} ({mg / max(abs(best), 1e-300):.2e} rel) same={got == want}")
    assert abs(got_score - ps) <= tol, f"{tag}: score {got_score} vs float64 score of the returned path {ps} (tol {tol})"
    assert ps >= best - tol, f"{tag}: returned path scores {ps}, the best path {best} (tol {tol})"
    if mg > 2 * tol:
        assert got == want, f"{tag}: margin {mg} > 2 tol {2 * tol} but frames differ: {got} vs {want}"
        return False
    return True


def check_score_below_ll(tag, blk, emit, Tb, Ub, score, nll):
    """score <= -nll: a path is one term of the sum over paths.  On the device both numbers are built from the SAME fp32 cell terms
    (one log-softmax kernel serves the loss and the alignment), and the score is a plain fp64 sum of them, so in exact arithmetic
    on those terms the inequality holds without slack.  What the loss adds on its side: nll is returned as fp32 (a relative
    rounding of 2^-24), and each of the Tb + Ub steps of its fp64 alpha chain adds an fp32 log1p(exp(.)) correction term in
    [0, ln 2] computed by the hardware exp / log, whose absolute error csrc/loss.hip puts at about 1e-7.  Slack:
    2^-23 |nll| + 2e-7 (Tb + Ub), twice each source.  The bound binds where there is a single path (Ub = 0 or Tb = 1): there
    score and -nll are the same sum.  Printed: both device numbers against their float64 values, and the observed score + nll."""
    best64, ll64 = ar.viterbi(blk, emit, Tb, Ub)[1], ar.log_likelihood(blk, emit, Tb, Ub)
    slack = 2.0 ** -23 * abs(nll) + 2e-7 * (Tb + Ub)
    print(f"{tag}: score - best64 = {score - best64:.3e}  (-nll) - ll64 = {-nll - ll64:.3e}  best64 - ll64 = {best64 - ll64:.3e}  "
          f"device score + nll = {score + nll:.3e}  slack = {slack:.3e}")
    return score <= -nll + slack


def check_sep_batch(tag, data, blank, frames, score, nll=None):
    A, C, bias, labels, t_lens, u_lens = data
    below = 0
    for b in range(A.shape[0]):
        if t_lens[b] == 0:
            assert score[b] == -np.inf and (frames[b] == -1).all(), f"{tag}[{b}]: empty utterance"
            continue
        blk, emit = ar.lattice_sep(A[b], C[b], bias, labels[b], blank)
        below += check_utterance(f"{tag}[{b}]", blk, emit, t_lens[b], u_lens[b], frames[b], score[b])
        if nll is not None:
            below_ll = check_score_below_ll(f"{tag}[{b}]", blk, emit, t_lens[b], u_lens[b], score[b], nll[b])
            assert below_ll
    n = sum(1 for t in t_lens if t > 0)
    assert below * 10 <= n, f"{tag}: {below} of {n} utterances below the margin: choose other seeds / scales"


# ---- 1. known answers ----
KNOWN = [[0, 0, 3, 3, 3, 11], [], [5], [0, 11], [11, 11, 11], [0, 1, 2, 3, 4, 5]]


@pytest.mark.parametrize("V,blank", [(8, 0), (8, 3), (300, 0), (300, 299)])
def test_known_answers_fused(V, blank):
    data = known_answer_sep(KNOWN, 12, V, blank)
    frames, score, res = run_fused(*data, blank)
    for b, f in enumerate(KNOWN):
        assert frames[b, :len(f)].tolist() == f and (frames[b, len(f):] == -1).all(), (b, frames[b])
        assert res.token_frames(b) == f
    # (the score rules are not applied here: these logits put probability 1 - 1e-8 on the path, so |best| is ~1e-7 .. 1e-6 while an
    # fp32 log-sum-exp of magnitude 20 .. 40 resolves 2e-6 .. 4e-6 per cell: a tolerance relative to |best| says nothing about them)
    assert np.isfinite(score).all() and (score <= 0).all() and score.dtype == np.float64


def test_known_answers_dense_fp32():
    blank, T, V = 2, 12, 8
    A, C, bias, labels, t_lens, u_lens = known_answer_sep(KNOWN, T, V, blank)
    logits = A[:, :, None, :] + C[:, None, :, :] + bias
    frames, score, _ = run_dense(_dev(logits), labels, t_lens, u_lens, blank)
    for b, f in enumerate(KNOWN):
        assert frames[b, :len(f)].tolist() == f and (frames[b, len(f):] == -1).all(), (b, frames[b])
    f2, s2, _ = run_fused(A, C, bias, labels, t_lens, u_lens, blank)
    assert (f2 == frames).all()


# ---- the tie rule on the device ----
@pytest.mark.parametrize("entry,V", [("fused", 8), ("fused", 300), ("dense", 8)])
def test_exact_ties_keep_the_blank_predecessor(entry, V):
    """All-zero logits: every cell term is the same number (-log V, bit for bit: the same instructions on the same inputs), and every
    v(t,u) is that number added t + u times from 0 whatever the path, so ALL paths tie exactly.  Under the rule (blank predecessor
    wins) every label lands on frame 0, where alone the label predecessor is strictly greater (there is no blank predecessor);
    with the opposite rule every label would land on the last frame."""
    B, T, U, blank = 4, 70, 9, 0
    A, C, bias = np.zeros((B, T, V), np.float32), np.zeros((B, U + 1, V), np.float32), np.zeros(V, np.float32)
    labels = np.tile(np.arange(1, U + 1, dtype=np.int32) % (V - 1) + 1, (B, 1))
    t_lens, u_lens = [70, 33, 64, 1], [9, 4, 0, 9]
    if entry == "fused":
        frames, score, _ = run_fused(A, C, bias, labels, t_lens, u_lens, blank)
    else:
        frames, score, _ = run_dense(_dev(A[:, :, None, :] + C[:, None, :, :] + bias), labels, t_lens, u_lens, blank)
    for b in range(B):
        blk, emit = ar.lattice_sep(A[b], C[b], bias, labels[b], blank)
        want = ar.viterbi(blk, emit, t_lens[b], u_lens[b])[0]
        assert want == [0] * u_lens[b]
        assert frames[b, :u_lens[b]].tolist() == want and (frames[b, u_lens[b]:] == -1).all(), (b, frames[b])
        assert abs(score[b] + (t_lens[b] + u_lens[b]) * np.log(V)) <= NLL_RTOL * abs(score[b])


# ---- 2-4. against float64: small random lattices ----
@pytest.mark.parametrize("seed,B,T,U,V,blank", [(11, 10, 119, 24, 72, 0), (12, 10, 60, 12, 72, 71), (13, 10, 20, 3, 2, 0),
                                              (14, 10, 20, 3, 2, 1), (15, 10, 40, 8, 256, 5), (17, 10, 33, 6, 2048, 100)])
def test_random_lattices(seed, B, T, U, V, blank):
    data = random_sep(seed, B, T, U, V, blank)
    frames, score, _ = run_fused(*data, blank)
    check_sep_batch(f"random seed={seed}", data, blank, frames, score, nll=fused_nll(*data, blank))


# U+1 crosses every K of the sweep (1: <= 64, 2: <= 128, 3: <= 192, 4: <= 256, 8: beyond), T the 32-frame word
SHAPES = [(21, 3, 1, 0, 72, 0), (22, 3, 31, 1, 72, 0), (23, 3, 32, 63, 72, 1), (24, 3, 33, 64, 72, 0), (25, 2, 1000, 158, 72, 0),
          (26, 2, 1000, 159, 256, 7), (27, 2, 33, 511, 72, 0), (28, 2, 1000, 511, 72, 0), (29, 2, 1000, 255, 2048, 0),
          (30, 2, 1, 511, 256, 0), (31, 3, 64, 0, 2, 0), (32, 2, 1000, 64, 2048, 2047), (33, 3, 65, 300, 72, 0),
          # the back-trace's table: up to 64 KiB in LDS (everything above; (28) is exactly 64 KiB), 64 .. 160 KiB in LDS with the raised
          # dynamic-LDS limit (34: 512 rows x 63 words = 126 KiB), beyond 160 KiB read from the workspace (35: 512 x 82 words = 164 KiB;
          # 36: 301 x 141 words = 166 KiB)
          (34, 2, 2000, 511, 72, 0), (35, 2, 2600, 511, 72, 0), (36, 2, 4500, 300, 72, 0)]


@pytest.mark.parametrize("seed,B,T,U,V,blank", SHAPES)
def test_shapes(seed, B, T, U, V, blank):
    data = scheduled_sep(seed, B, T, U, V, blank)
    frames, score, _ = run_fused(*data, blank)
    check_sep_batch(f"shape seed={seed}", data, blank, frames, score, nll=fused_nll(*data, blank))


def test_empty_utterance_leaves_other_rows_bitwise_unchanged():
    blank = 0
    A, C, bias, labels, t_lens, u_lens = scheduled_sep(41, 4, 70, 20, 72, blank)
    f0, s0, _ = run_fused(A, C, bias, labels, t_lens, u_lens, blank)
    t2 = list(t_lens)
    t2[1] = 0
    f1, s1, _ = run_fused(A, C, bias, labels, t2, u_lens, blank)
    assert s1[1] == -np.inf and (f1[1] == -1).all()
    keep = [0, 2, 3]
    assert (f1[keep] == f0[keep]).all() and s1[keep].tobytes() == s0[keep].tobytes()
    check_sep_batch("empty row", (A, C, bias, labels, t2, u_lens), blank, f1, s1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_dense_logits(dtype):
    blank = 4
    A, C, bias, labels, t_lens, u_lens = scheduled_sep(51, 10, 45, 9, 40, blank)
    logits = torch.as_tensor(A[:, :, None, :] + C[:, None, :, :] + bias).to(dtype).cuda()
    frames, score, _ = run_dense(logits, labels, t_lens, u_lens, blank)
    z = logits.float().cpu().numpy().astype(np.float64)     # the rounded logits are the float64 side's input
    below = 0
    for b in range(len(t_lens)):
        blk, emit = ar.lattice(z[b], labels[b], blank)
        below += check_utterance(f"dense {dtype}[{b}]", blk, emit, t_lens[b], u_lens[b], frames[b], score[b])
    assert below * 10 <= len(t_lens)


# ---- 5. independence ----
@pytest.mark.parametrize("case", ["random", "scheduled", "largeV"])
def test_rows_do_not_depend_on_the_batch_and_calls_repeat(case):
    blank = 0
    data = {"random": lambda: random_sep(61, 5, 50, 10, 72), "scheduled": lambda: scheduled_sep(62, 4, 100, 200, 72),
            "largeV": lambda: scheduled_sep(63, 4, 70, 30, 300)}[case]()
    f0, s0, _ = run_fused(*data, blank)
    f1, s1, _ = run_fused(*data, blank)
    assert (f0 == f1).all() and s0.tobytes() == s1.tobytes()
    for b in range(f0.shape[0]):
        fb, sb, _ = run_fused(*data, blank, rows=slice(b, b + 1))
        assert (fb[0] == f0[b]).all() and sb.tobytes() == s0[b:b + 1].tobytes(), f"row {b} alone differs from the batch"
    # a caller-owned workspace and output buffers, filled with junk first
    from rnntransducer_amd import ops
    A, C, bias, labels, t_lens, u_lens = data
    B, T, V = A.shape
    ws = torch.full((ops.align_workspace_bytes(B, T, C.shape[1], V) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    fr, sc = torch.full((B, C.shape[1] - 1), 77, device="cuda", **I32), torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
    ops.joint_align(_dev(A), _dev(C), _dev(bias), _dev(labels), _dev(np.array(t_lens), torch.int32), _dev(np.array(u_lens), torch.int32),
                    blank, batch_first=True, workspace=ws, frames=fr, score=sc)
    torch.cuda.synchronize()
    assert (fr.cpu().numpy() == f0).all() and sc.cpu().numpy().tobytes() == s0.tobytes()


# ---- 6. model level ----
def _model(bidirectional, V=72):
    from argparse import Namespace
    from rnntransducer_amd import RNNTransducer
    torch.manual_seed(5)
    args = Namespace(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=10)
    tn = dict(input_size=80, hidden_size=128, output_size=128, num_layers=2, dropout=0.0, bidirectional=bidirectional)
    pn = dict(embedding_size=V, hidden_size=128, output_size=128, num_layers=1, dropout=0.0)
    m = RNNTransducer(dict(pn), dict(tn), dict(num_classes=V), args)
    with torch.no_grad():   # random init gives logits of scale 0.1, where near-ties are common: scale to about unit variance
        for n, p in m.jointnet.named_parameters():
            p.mul_(8.0 if n.startswith("fc.") else 2.0)
        m.jointnet.decoder.embedding.weight[0].zero_()
    return m.cuda().eval()


@pytest.mark.parametrize("bidirectional", [False, True])
def test_model_align(bidirectional):
    from rnntransducer_amd import ops
    from rnntransducer_amd.data import synthetic_batch
    from rnntransducer_amd.networks.encoder import lengths_to_device
    V, blank = 72, 0
    m = _model(bidirectional)
    jn = m.jointnet
    batch = synthetic_batch(10, 40, 8, V, ragged=True, seed=9)
    dev_batch = tuple(x.cuda() if isinstance(x, torch.Tensor) else x for x in batch)
    audios, alist, t_lens, texts, tlist, targets, u_lens = dev_batch
    plain = jn.align(audios, t_lens, texts, targets, u_lens, blank)
    ragged = jn.align(audios, t_lens, texts, targets, u_lens, blank, audio_lengths=alist)
    whole = m.align(dev_batch)
    torch.cuda.synchronize()
    assert plain.frames.dtype == torch.int32 and plain.frames.shape == (10, 8)
    assert plain.score.dtype == torch.float64 and plain.score.shape == (10,)
    # the model's own enc / dec through ops.joint_align: the same bits
    with torch.no_grad():
        enc = jn.encoder.forward_time_major(audios, t_lens)
        dec = jn.decoder.forward_time_major(texts, u_lens + 1)
        A, Cm = ops._joint_ac(enc, dec, jn.fc.weight, jn.enc_out, jn.dec_out, V)
        direct = ops.joint_align(A, Cm, jn.fc.bias, targets, t_lens, u_lens, blank)
        logits = m(audios, alist, texts, tlist)
    torch.cuda.synchronize()
    assert torch.equal(direct.frames, plain.frames) and torch.equal(direct.score, plain.score)
    assert torch.equal(whole.frames, ragged.frames) and torch.equal(whole.score, ragged.score)
    # against float64 on the logits model.forward() returns; the sorted-and-packed ragged path under the same rules
    z = logits.double().cpu().numpy()
    tl, ul, lab = t_lens.tolist(), u_lens.tolist(), targets.cpu().numpy()
    for name, res in (("plain", plain), ("ragged", ragged)):
        frames, score = res.frames.cpu().numpy(), res.score.cpu().numpy()
        below = 0
        for b in range(10):
            blk, emit = ar.lattice(z[b], lab[b], blank)
            below += check_utterance(f"model bi={bidirectional} {name}[{b}]", blk, emit, tl[b], ul[b], frames[b], score[b])
            assert res.token_frames(b) == frames[b, :ul[b]].tolist()
        assert below * 10 <= 10
    nll = jn.loss(audios, t_lens, texts, targets, u_lens, blank).detach().double().cpu().numpy()
    slack = 2.0 ** -23 * np.abs(nll) + 2e-7 * (t_lens.cpu().numpy() + u_lens.cpu().numpy())   # check_score_below_ll: same cell terms
    print(f"model bi={bidirectional}: score + nll = {plain.score.cpu().numpy() + nll}  slack = {slack}")
    assert (plain.score.cpu().numpy() <= -nll + slack).all()
    jn.train()
    with pytest.raises(RuntimeError, match="eval"):
        jn.align(audios, t_lens, texts, targets, u_lens, blank)
