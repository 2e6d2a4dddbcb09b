"""CPU checks of the CTC prefix beam search's definition (tests/ctc_beam_restatement.py, the yardstick of tests/test_gpu_ctc_beam.py)
against quantities that do not depend on a search — torch's CTC loss, symmetry, TokenFusion.score — and the host-side argument
checks of ops.ctc_beam_search and recognize_ctc_beams.  No device work."""
import itertools
import math
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ctc_beam_restatement as R
from tests.ctc_beam_cases import MARGIN, REREACH_CASES, SHAPES, fused_case, fusion_for, rereach_logits, shape_case

P, Q = 0x10000, 0x20000   # stand-ins for device pointers


def ctc_logp(z, tokens, blank):
    """The exact CTC log-probability of a labelling: -F.ctc_loss on the fp64 log-softmax of the fp32-rounded logits."""
    T = z.shape[0]
    lp = F.log_softmax(torch.from_numpy(np.asarray(z, dtype=np.float32)).double(), -1).unsqueeze(1)
    y = torch.tensor([tokens], dtype=torch.long).reshape(1, len(tokens))
    nll = F.ctc_loss(lp, y, torch.tensor([T]), torch.tensor([len(tokens)]), blank=blank, reduction="none")
    return -float(nll[0])


def labellings(T, V, blank):
    """Every labelling that has a path over T frames: length + number of adjacent repeats <= T."""
    toks = [k for k in range(V) if k != blank]
    out = []
    for n in range(T + 1):
        for y in itertools.product(toks, repeat=n):
            if n + sum(a == b for a, b in zip(y, y[1:])) <= T:
                out.append(list(y))
    return out


@pytest.mark.parametrize("T,blank,seed", [(1, 0, 0), (2, 1, 1), (3, 2, 2), (4, 0, 3), (4, 1, 4)])
def test_exhaustive_beam_gives_the_exact_ctc_probability(T, blank, seed):
    z = (2.0 * np.random.default_rng(seed).standard_normal((T, 3))).astype(np.float32)
    hyps, bm, _ = R.search(z, blank, 32)
    want = labellings(T, 3, blank)
    assert len(want) <= 32 and bm == math.inf                      # nothing was ever pruned
    assert sorted(h["tokens"] for h in hyps) == sorted(want)
    for h in hyps:
        assert abs(h["score"] - ctc_logp(z, h["tokens"], blank)) < 1e-12, h
    assert abs(np.logaddexp.reduce([h["score"] for h in hyps])) < 1e-12   # the masses of all labellings sum to one
    assert all(a["score"] >= b["score"] for a, b in zip(hyps, hyps[1:]))


def test_uniform_logits_tie_in_id_order():
    """All candidates of a frame with equal keys: the order is the id order r (V+1) + j, blank = 0 so tokens 1, 2."""
    hyps, _, om = R.search(np.zeros((1, 3), np.float32), 0, 3)
    assert [h["tokens"] for h in hyps] == [[], [1], [2]] and om == 0.0
    assert all(abs(h["score"] - math.log(1 / 3)) < 1e-15 for h in hyps)
    # T = 2: (), (1), (2) carry 1/9, 3/9, 3/9; (1,2) and (2,1) carry 1/9 and are cut by W = 3 with (): lowest id first
    hyps, _, _ = R.search(np.zeros((2, 3), np.float32), 0, 3)
    assert [h["tokens"] for h in hyps] == [[1], [2], []]
    assert [round(math.exp(h["score"]) * 9) for h in hyps] == [3, 3, 1]
    # blank in the middle: the tokens are 0 and 2
    hyps, _, _ = R.search(np.zeros((1, 3), np.float32), 1, 3)
    assert [h["tokens"] for h in hyps] == [[], [0], [2]]


def test_the_stay_term_survives_pruning():
    """Frame 1 makes token 1 fall below token_min_logp: (1) cannot be extended by 1 there, but its stay term pnb + lp[1,1] counts."""
    z = np.log(np.array([[0.2, 0.7, 0.1], [0.9, 0.01, 0.09]], dtype=np.float64)).astype(np.float32)
    lp = R.log_softmax(z)
    thr = math.log(0.05)
    hyps, _, _ = R.search(z, 0, 8, token_min_logp=thr)
    by = {tuple(h["tokens"]): h["score"] for h in hyps}
    # (1): frame 0 emits 1; frame 1 is blank or stays on 1 (kept), plus "blank then 1", which needs the pruned extension (lost)
    assert abs(by[(1,)] - np.logaddexp(lp[0, 1] + lp[1, 0], lp[0, 1] + lp[1, 1])) < 1e-12
    full = {tuple(h["tokens"]): h["score"] for h in R.search(z, 0, 8)[0]}
    assert abs(full[(1,)] - np.logaddexp(by[(1,)], lp[0, 0] + lp[1, 1])) < 1e-12
    assert (1, 1) not in by and (2, 1) not in by and (1, 2) in by and (1, 1) not in full   # (1,1) needs three frames


@pytest.mark.parametrize("kind", ["hotwords", "bigram"])
def test_fused_scores_are_score_plus_total_plus_final(kind):
    T, V, W, blank = 12, 9, 6, 0
    z = (2.0 * np.random.default_rng(7).standard_normal((T, V))).astype(np.float32)
    fusion = fusion_for(kind, V, blank, 7)
    plain, _, _ = R.search(z, blank, W)
    hyps, _, _ = R.search(z, blank, W, fusion=fusion)
    assert any(h["total"] != 0.0 for h in hyps)
    for h in hyps:
        total, final, _ = fusion.score([blank] + h["tokens"])
        assert abs(h["total"] - total) < 1e-12 and abs(h["fused"] - (h["score"] + total + final)) < 1e-12
    assert all(a["fused"] >= b["fused"] for a, b in zip(hyps, hyps[1:]))
    assert [h["tokens"] for h in hyps] != [h["tokens"] for h in plain]   # the automaton changes the list or its order
    from tests.fusion_cases import zero_fusion
    zero, _, _ = R.search(z, blank, W, fusion=zero_fusion(V))
    assert [(h["tokens"], h["score"]) for h in zero] == [(h["tokens"], h["score"]) for h in plain]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d-V%d-W%d" % s[:3])
@pytest.mark.parametrize("scale", [1, 4])
def test_gpu_cases_keep_their_margin(shape, scale):
    """The cases of tests/test_gpu_ctc_beam.py: one of 20 seeds keeps a boundary margin >= 1e-4 (so the GPU test is never the first
    to see a case), frames increase along every hypothesis."""
    T, V, W, thr = shape
    case = shape_case(T, V, W, thr, scale)
    assert case is not None, "no seed of 20 keeps the margin"
    seed, z, hyps, bm, om = case
    assert bm >= 1e-4 and 1 <= len(hyps) <= W
    for h in hyps:
        assert len(h["frames"]) == len(h["tokens"]) and all(a < b for a, b in zip(h["frames"], h["frames"][1:]))
        assert all(0 <= f < T for f in h["frames"])
    assert len({tuple(h["tokens"]) for h in hyps}) == len(hyps)   # a labelling appears once


@pytest.mark.parametrize("V,W,T,seed", REREACH_CASES)
def test_a_prefix_reached_again_keeps_one_entry(V, W, T, seed):
    """A pruned prefix that is reached again: the labelling appears once, carries no more than its exact CTC mass, and its frames
    are those of its first entry (increasing)."""
    z = rereach_logits(V, T, seed)
    stats = {}
    hyps, bm, _ = R.search(z, 0, W, stats=stats)
    assert stats.get("rereached", 0) >= 1 and bm >= MARGIN
    assert len({tuple(h["tokens"]) for h in hyps}) == len(hyps) == W
    for h in hyps:
        assert h["score"] <= ctc_logp(z, h["tokens"], 0) + 1e-12
        assert all(a < b for a, b in zip(h["frames"], h["frames"][1:]))


@pytest.mark.parametrize("kind", ["hotwords", "bigram"])
@pytest.mark.parametrize("blank", [0, 5])
def test_gpu_fused_cases_keep_their_margin(kind, blank):
    case = fused_case(30, 40, 8, 2, blank, kind)
    assert case is not None
    seed, z, hyps, bm, om, fusion = case
    assert bm >= MARGIN and any(h["total"] != 0.0 for h in hyps)


# ---------------------------------------------------------------------------------------------------------------------------------
def _jointnet(aux=True):
    from rnntransducer_amd import JointNet
    torch.manual_seed(0)
    tn = dict(input_size=12, hidden_size=8, output_size=12, num_layers=1)
    pn = dict(embedding_size=10, hidden_size=8, output_size=8, num_layers=1, pad_token_id=0)
    return JointNet(tn, pn, 10, aux_ctc=aux)


def test_ops_argument_errors_come_before_any_launch():
    from rnntransducer_amd import TokenFusion
    from rnntransducer_amd._lib import RnntHipError
    from rnntransducer_amd.ops import ctc_beam_search
    z, tl = torch.zeros(2, 5, 10), torch.tensor([5, 4], dtype=torch.int32)
    for W in (0, 129, -1, 2.0, True):
        with pytest.raises(ValueError, match="beam width"):
            ctc_beam_search(z, tl, 0, W)
    for thr in (math.nan, math.inf, "x"):
        with pytest.raises(ValueError, match="token_min_logp"):
            ctc_beam_search(z, tl, 0, 4, token_min_logp=thr)
    for blank in (-1, 10):
        with pytest.raises(ValueError, match="blank"):
            ctc_beam_search(z, tl, blank, 4)
    with pytest.raises(ValueError):
        ctc_beam_search(z[0], tl, 0, 4)
    with pytest.raises(ValueError, match="V = 1"):
        ctc_beam_search(z[:, :, :1], tl, 0, 4)
    wrong = TokenFusion(torch.zeros(1, 9, dtype=torch.int32), torch.zeros(1, 9), torch.zeros(1))
    with pytest.raises(ValueError, match="9 tokens"):
        ctc_beam_search(z, tl, 0, 4, fusion=wrong)
    with pytest.raises(ValueError, match="TokenFusion"):
        ctc_beam_search(z, tl, 0, 4, fusion=object())
    with pytest.raises(RnntHipError):                      # valid arguments, CPU tensors: no CPU or eager fallback
        ctc_beam_search(z, tl, 0, 4)


def test_model_argument_errors_come_before_any_launch():
    from rnntransducer_amd import RNNTransducer, TokenFusion
    x, tl = torch.zeros(2, 5, 12), torch.tensor([5, 4], dtype=torch.int32)
    with pytest.raises(ValueError, match="aux_ctc"):
        _jointnet(aux=False).eval().recognize_ctc_beams(x, tl, 0)
    net = _jointnet()
    with pytest.raises(ValueError, match="eval"):
        net.train().recognize_ctc_beams(x, tl, 0)
    net.eval()
    for W in (0, 129):
        with pytest.raises(ValueError, match="beam width"):
            net.recognize_ctc_beams(x, tl, 0, W)
    with pytest.raises(ValueError, match="token_min_logp"):
        net.recognize_ctc_beams(x, tl, 0, 4, token_min_logp=math.nan)
    wrong = TokenFusion(torch.zeros(1, 9, dtype=torch.int32), torch.zeros(1, 9), torch.zeros(1))
    with pytest.raises(ValueError, match="9 tokens"):
        net.recognize_ctc_beams(x, tl, 0, 4, fusion=wrong)
    args = Namespace(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=10)
    cfg = (dict(embedding_size=10, hidden_size=8, output_size=8, num_layers=1), dict(input_size=12, hidden_size=8, output_size=12, num_layers=1))
    with pytest.raises(ValueError, match="aux_ctc"):
        RNNTransducer(*cfg, dict(num_classes=10), args).eval().recognize_ctc_beams(x, tl)
    with pytest.raises(ValueError, match="beam width"):
        RNNTransducer(*cfg, dict(num_classes=10, aux_ctc=True), args).eval().recognize_ctc_beams(x, tl, 0)


def test_c_abi_refuses_bad_arguments_before_any_launch():
    from rnntransducer_amd import _lib
    L = _lib.lib()
    B, T, V, W = 2, 10, 5, 4
    need = L.rnnt_hip_ctc_beam_workspace_bytes(B, T, V, W)
    assert need > 0 and L.rnnt_hip_ctc_beam_workspace_bytes(B, T, V, 8) > need
    for bad in ((0, T, V, W), (B, 0, V, W), (B, T, 1, W), (B, T, V, 0), (B, T, V, 129), (B, T, 1 << 20, 128)):
        assert L.rnnt_hip_ctc_beam_workspace_bytes(*bad) == 0
    fus = _lib.BeamFusion(P, P, P, 3, P)

    def call(logits=P, t_lens=Q, V=V, blank=0, W=W, thr=-math.inf, fusion=None, tokens=P, lens=P, scores=P, counts=P, ws=P, nws=need,
             z_st=V):
        return L.rnnt_hip_ctc_beam_search(logits, T * V, z_st, t_lens, B, T, V, blank, W, thr, fusion, tokens, lens, scores, None, counts,
                                          ws, nws, None)

    err = L.rnnt_hip_last_error
    for W_ in (0, 129):
        assert call(W=W_) == -1 and b"beam width" in err()
    assert call(V=1) == -1 and b"V = 1" in err()
    for blank in (-1, V):
        assert call(blank=blank) == -1 and b"blank" in err()
    for thr in (math.nan, math.inf):
        assert call(thr=thr) == -1 and b"token_min_logp" in err()
    for kw in ("logits", "t_lens", "tokens", "lens", "scores", "counts"):
        assert call(**{kw: None}) == -1 and b"null" in err()
    assert call(z_st=V - 1) == -1 and b"stride" in err()
    assert call(ws=None) == -1 and call(nws=need - 1) == -1 and b"workspace too small" in err()
    assert call(fusion=_lib.BeamFusion(None, P, P, 3, P)) == -1 and b"fusion table" in err()
    assert call(fusion=_lib.BeamFusion(P, P, P, 0, P)) == -1 and b"n_states" in err()
    assert call(fusion=_lib.BeamFusion(P, P, P, 3, None)) == -1 and b"fused_scores" in err()
    assert call(fusion=fus, nws=need - 1) == -1 and b"workspace" in err()
    assert L.rnnt_hip_version() == 4
