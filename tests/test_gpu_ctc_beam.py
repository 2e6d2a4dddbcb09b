"""The CTC prefix beam search on the device (csrc/ctc_beam.hip, ops.ctc_beam_search, recognize_ctc_beams) against the numpy fp64
restatement of its definition (tests/ctc_beam_restatement.py), the CTC loss kernels, and itself (bitwise properties).

Decision margin: a case is compared with the restatement only if its boundary margin there (the smallest gap between the W-th and
the (W+1)-th candidate of a frame) is at least 1e-4, asserted on the CPU before the GPU call; the seed walk (20 seeds from 0) must
find such a seed.  Token lists: exact.  Scores: 1e-5 relative, tests/test_gpu_ctc.py's NLL bound (the same quantity and
arithmetic: fp32 log-softmax, fp64 sums with the fp32 logaddexp correction).  Output order: only across adjacent pairs whose gap in
the restatement is at least 1e-4."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import ctc_beam_restatement as R
from tests.ctc_beam_cases import MARGIN, REREACH_CASES, SHAPES, batch_of, blank_of, fused_case, fusion_for, rereach_logits, shape_case

pytestmark = pytest.mark.gpu
SENT_I, PAD_T = -77, 3


def search(z, tl, blank, W, **kw):
    from rnntransducer_amd.ops import ctc_beam_search
    return ctc_beam_search(z.cuda(), tl.cuda(), blank, W, **kw)


def compare(got, want, fused=False, frames=False):
    """got: the entries of one utterance from ops.ctc_beam_search; want: the restatement's hyps."""
    assert len(got) == len(want)
    pos = {tuple(e[0]): i for i, e in enumerate(got)}
    assert len(pos) == len(got), "a labelling is returned twice"
    assert set(pos) == {tuple(h["tokens"]) for h in want}
    for h in want:
        e = got[pos[tuple(h["tokens"])]]
        assert abs(e[1] - h["score"]) <= 1e-5 * abs(h["score"]), (h["tokens"], e[1], h["score"])
        if fused:
            assert abs(e[2] - h["fused"]) <= 1e-5 * max(abs(h["fused"]), abs(h["score"])), (h["tokens"], e[2], h["fused"])
        if frames:
            assert e[-1] == h["frames"], (h["tokens"], e[-1], h["frames"])
    for a, b in zip(want, want[1:]):
        if a["fused"] - b["fused"] >= MARGIN:
            assert pos[tuple(a["tokens"])] < pos[tuple(b["tokens"])], (a, b)


@pytest.mark.parametrize("scale", [1, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d-V%d-W%d" % s[:3])
def test_shapes_against_the_restatement(shape, scale):
    T, V, W, thr = shape
    case = shape_case(T, V, W, thr, scale)
    assert case is not None, "none of 20 seeds keeps a boundary margin of 1e-4"
    seed, z, want, bm, om = case
    assert bm >= MARGIN
    zb, tl = batch_of([z], T + PAD_T, V)            # NaN in every frame >= T_b
    got = search(zb, tl, 0, W, token_min_logp=thr, return_frames=True)[0]
    print(f"seed {seed} boundary margin {bm:.3g} order margin {om:.3g} hypotheses {len(got)}")
    compare(got, want, frames=True)
    for e in got:
        assert all(a < b for a, b in zip(e[-1], e[-1][1:])) and all(0 <= f < T for f in e[-1])


@pytest.mark.parametrize("V,W,T,seed", REREACH_CASES)
def test_a_prefix_reached_again_keeps_its_node(V, W, T, seed):
    """A prefix falls out of the beam while an extension of it stays, and is reached again: no labelling twice, the restatement's
    lists, scores and (first-entry) frames."""
    z = rereach_logits(V, T, seed)
    stats = {}
    want, bm, _ = R.search(z, 0, W, stats=stats)
    assert stats.get("rereached", 0) >= 1 and bm >= MARGIN
    got = search(*batch_of([z], T + PAD_T, V), 0, W, return_frames=True)[0]
    compare(got, want, frames=True)


def test_exhaustive_beam_matches_the_ctc_loss_kernels():
    """V = 3, T = 4, W = 32: every labelling with a path is returned, and its score is minus the NLL of CtcLossFn for it."""
    from rnntransducer_amd.ops import CtcLossFn
    T, V, W, blank = 4, 3, 32, 0
    z = (2.0 * np.random.default_rng(3).standard_normal((T, V))).astype(np.float32)
    got = search(*batch_of([z], T, V), blank, W)[0]
    assert len(got) == 15 and len({tuple(y) for y, _ in got}) == 15          # 1 + 2 + 4 + 6 + 2 labellings have a path over four frames
    n = len(got)
    labels = torch.zeros(n, T, dtype=torch.int32)
    for i, (y, _) in enumerate(got):
        labels[i, :len(y)] = torch.tensor(y, dtype=torch.int32)
    u_lens = torch.tensor([len(y) for y, _ in got], dtype=torch.int32)
    zz = torch.from_numpy(z).unsqueeze(0).repeat(n, 1, 1).cuda()
    nll = CtcLossFn.apply(zz, labels.cuda(), torch.full((n,), T, dtype=torch.int32).cuda(), u_lens.cuda(), blank, False, "none").cpu()
    for (y, s), want in zip(got, (-nll.double()).tolist()):
        assert math.isfinite(want) and abs(s - want) <= 1e-5 * abs(want), (y, s, want)
    assert all(a[1] >= b[1] for a, b in zip(got, got[1:]))


TIE_EXPECTED = {(1, 0): [[], [1], [2]], (2, 0): [[1], [2], []], (1, 1): [[], [0], [2]], (2, 2): [[0], [1], []]}


# (the V = 3 cases keep the ids they always had)
@pytest.mark.parametrize("V,T,blank", [pytest.param(V, T, blank, id=f"{T}-{blank}" if V == 3 else f"{V}-{T}-{blank}")
                                       for V in (3, 300, 70000) for T, blank in TIE_EXPECTED])
def test_uniform_logits_tie_in_id_order(V, T, blank):
    """Every candidate of frame 0 has the same key bit for bit: the select picks the three lowest ids by its id passes alone.
    V = 3: only the last 8-bit digit of the id has more than one bin populated; V = 300: the middle digit too; V = 70000: the
    first as well (ids cross 65536)."""
    want, _, _ = R.search(np.zeros((T, V), np.float32), blank, 3)
    got = search(torch.zeros(1, T, V), torch.tensor([T], dtype=torch.int32), blank, 3)[0]
    assert [y for y, _ in got] == [h["tokens"] for h in want] == TIE_EXPECTED[T, blank]
    for (y, s), h in zip(got, want):
        assert abs(s - h["score"]) <= 1e-5 * abs(h["score"])


# ---------------------------------------------------------------------------------------------------------------------------------
def raw_search(z, tl, blank, W, thr=-math.inf, fusion=None, want_frames=False, time_major=False):
    """The C entry on buffers filled beforehand: outputs with a sentinel, the workspace with 0xff bytes (NaN as fp32 and fp64)."""
    from rnntransducer_amd import _lib
    from rnntransducer_amd.ops import fusion_struct
    L = _lib.lib()
    z, tl = z.cuda(), tl.cuda()
    if time_major:
        z = z.transpose(0, 1).contiguous()
        T, B, V = z.shape
        z_sb, z_st = V, B * V
    else:
        B, T, V = z.shape
        z_sb, z_st = T * V, V
    out = dict(tokens=torch.full((B, W, T), SENT_I, dtype=torch.int32, device="cuda"),
               lens=torch.full((B, W), SENT_I, dtype=torch.int32, device="cuda"),
               scores=torch.full((B, W), math.nan, dtype=torch.float64, device="cuda"),
               counts=torch.full((B,), SENT_I, dtype=torch.int32, device="cuda"),
               frames=torch.full((B, W, T), SENT_I, dtype=torch.int32, device="cuda") if want_frames else None,
               fused=torch.full((B, W), math.nan, dtype=torch.float64, device="cuda") if fusion is not None else None)
    nws = L.rnnt_hip_ctc_beam_workspace_bytes(B, T, V, W)
    assert nws > 0
    ws = torch.full((nws,), 0xff, dtype=torch.uint8, device="cuda")
    fs = fusion_struct(fusion, out["fused"]) if fusion is not None else None
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = L.rnnt_hip_ctc_beam_search(ptr(z), z_sb, z_st, ptr(tl), B, T, V, blank, W, thr, C.byref(fs) if fs is not None else None,
                                    ptr(out["tokens"]), ptr(out["lens"]), ptr(out["scores"]), ptr(out["frames"]), ptr(out["counts"]),
                                    ptr(ws), nws, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.rnnt_hip_last_error()
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu()) for k, v in out.items()}


def same_bits(a, b, rows_a=None, rows_b=None):
    for k in ("tokens", "lens", "counts", "frames"):
        if a[k] is not None and b[k] is not None:
            x = a[k] if rows_a is None else a[k][rows_a]
            y = b[k] if rows_b is None else b[k][rows_b]
            assert torch.equal(x, y), k
    for k in ("scores", "fused"):
        if a[k] is not None and b[k] is not None:
            x = a[k] if rows_a is None else a[k][rows_a]
            y = b[k] if rows_b is None else b[k][rows_b]
            assert torch.equal(x.view(torch.int64), y.view(torch.int64)), k


def unwritten_is_untouched(out, T_lens):
    B, W, T = out["tokens"].shape
    counts, lens = out["counts"].tolist(), out["lens"].tolist()
    for b in range(B):
        n = counts[b]
        assert 1 <= n <= W
        assert bool((out["lens"][b, n:] == SENT_I).all()) and bool(out["scores"][b, n:].isnan().all())
        assert bool((out["tokens"][b, n:] == SENT_I).all())
        assert not bool(out["scores"][b, :n].isnan().any())
        for o in range(n):
            assert 0 <= lens[b][o] <= T_lens[b]
            assert bool((out["tokens"][b, o, lens[b][o]:] == SENT_I).all()) and bool((out["tokens"][b, o, :lens[b][o]] >= 0).all())
            if out["frames"] is not None:
                assert bool((out["frames"][b, o, lens[b][o]:] == SENT_I).all())
        if out["frames"] is not None:
            assert bool((out["frames"][b, n:] == SENT_I).all())
        if out["fused"] is not None:
            assert bool(out["fused"][b, n:].isnan().all()) and not bool(out["fused"][b, :n].isnan().any())


HYG = dict(T=20, V=37, W=8)


def hygiene_batch(scale=2.0):
    T, V = HYG["T"], HYG["V"]
    rows = [(scale * np.random.default_rng(50 + b).standard_normal((tb, V))).astype(np.float32) for b, tb in enumerate((T, 0, 13))]
    return rows, batch_of(rows, T, V)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_hygiene_padding_sentinels_and_bitwise_properties(where):
    """NaN logits in every frame >= T_b, NaN-filled outputs and workspace, a T_b = 0 row, T_b < T rows; batch-major against
    time-major, twice, and each row alone against in the batch: the same bits; the blank first, in the middle and last."""
    T, V, W = HYG["T"], HYG["V"], HYG["W"]
    blank = blank_of(V, where)
    rows, (zb, tl) = hygiene_batch()
    out = raw_search(zb, tl, blank, W, want_frames=True)
    unwritten_is_untouched(out, tl.tolist())
    assert out["counts"].tolist()[1] == 1 and out["lens"][1, 0].item() == 0 and out["scores"][1, 0].item() == 0.0   # T_b = 0: [()]
    assert not bool((out["tokens"][out["tokens"] != SENT_I] == blank).any())
    same_bits(out, raw_search(zb, tl, blank, W, want_frames=True))
    same_bits(out, raw_search(zb, tl, blank, W, want_frames=True, time_major=True))
    same_bits(out, raw_search(zb, tl, blank, W))                                      # without frames: the same lists and scores
    for b in range(3):
        alone = raw_search(zb[b:b + 1], tl[b:b + 1], blank, W, want_frames=True)
        same_bits(out, alone, rows_a=slice(b, b + 1))
    # the restatement of each row, where it keeps the margin (at least one row must)
    compared = 0
    for b in (0, 2):
        want, bm, _ = R.search(rows[b], blank, W)
        if bm >= MARGIN:
            n = out["counts"][b].item()
            got = [(out["tokens"][b, o, :out["lens"][b, o]].tolist(), out["scores"][b, o].item(),
                    out["frames"][b, o, :out["lens"][b, o]].tolist()) for o in range(n)]
            compare(got, want, frames=True)
            compared += 1
    assert compared >= 1


def test_fewer_candidates_than_the_beam_is_wide():
    """One frame over three classes has three candidates: counts = 3 < W, nothing is written past them."""
    z = torch.tensor([[[0.5, 1.5, -0.25]]])
    out = raw_search(z, torch.tensor([1], dtype=torch.int32), 0, 8, want_frames=True)
    unwritten_is_untouched(out, [1])
    assert out["counts"].tolist() == [3] and out["lens"][0, :3].tolist() == [1, 0, 1]
    assert out["tokens"][0, 0, 0].item() == 1 and out["tokens"][0, 2, 0].item() == 2 and out["frames"][0, 0, 0].item() == 0
    lp = R.log_softmax(z[0].numpy())[0]
    for o, k in enumerate((1, 0, 2)):
        assert abs(out["scores"][0, o].item() - lp[k]) <= 1e-5 * abs(lp[k])


# ---------------------------------------------------------------------------------------------------------------------------------
FUS = dict(T=30, V=40, W=8, scale=2)


def test_zero_automaton_gives_the_unfused_bits():
    rows, (zb, tl) = hygiene_batch()
    V, W = HYG["V"], HYG["W"]
    plain = raw_search(zb, tl, 0, W, want_frames=True)
    fused = raw_search(zb, tl, 0, W, fusion=fusion_for("zero", V, 0, 0).to("cuda"), want_frames=True)
    same_bits(plain, dict(fused, fused=None))
    n = plain["counts"].tolist()
    for b in range(3):
        assert torch.equal(fused["fused"][b, :n[b]].view(torch.int64), plain["scores"][b, :n[b]].view(torch.int64))
    unwritten_is_untouched(fused, tl.tolist())


@pytest.mark.parametrize("kind", ["hotwords", "bigram"])
@pytest.mark.parametrize("blank", [0, 5])
def test_fused_search_against_the_restatement(kind, blank):
    T, V, W, scale = FUS["T"], FUS["V"], FUS["W"], FUS["scale"]
    case = fused_case(T, V, W, scale, blank, kind)
    assert case is not None, "none of 20 seeds keeps a boundary margin of 1e-4 on score + total"
    seed, z, want, bm, om, fusion = case
    assert bm >= MARGIN
    assert any(h["total"] != 0.0 for h in want)
    got = search(*batch_of([z], T + PAD_T, V), blank, W, fusion=fusion.to("cuda"), return_frames=True)[0]
    print(f"seed {seed} boundary margin {bm:.3g} order margin {om:.3g}")
    compare(got, want, fused=True, frames=True)
    for y, score, fused_score, _ in got:                    # fused_score reproduces from TokenFusion.score
        total, final, _ = fusion.score([blank] + y)
        assert abs(fused_score - (score + total + final)) <= 1e-12 * max(1.0, abs(score))


def test_return_frames_changes_nothing_else():
    T, V, W, thr = SHAPES[5]
    seed, z, want, bm, _ = shape_case(T, V, W, thr, 4)
    zb, tl = batch_of([z, z[:T // 2]], T, V)
    a = search(zb, tl, 0, W)
    b = search(zb, tl, 0, W, return_frames=True)
    for ha, hb in zip(a, b):
        assert [(y, s) for y, s in ha] == [(y, s) for y, s, _ in hb]
    for hyps, tb in zip(b, tl.tolist()):
        for y, _, fr in hyps:
            assert len(fr) == len(y) and all(x <= y_ for x, y_ in zip(fr, fr[1:])) and all(0 <= f < tb for f in fr)
    compare(b[0], want, frames=True)


# ---------------------------------------------------------------------------------------------------------------------------------
def _jointnet(bidirectional, seed):
    from rnntransducer_amd import JointNet
    torch.manual_seed(seed)
    tn = dict(input_size=12, hidden_size=16, output_size=12, num_layers=1, rnn_type="lstm", dropout=0.0, bidirectional=bidirectional)
    pn = dict(embedding_size=10, hidden_size=8, output_size=8, num_layers=1, pad_token_id=0)
    net = JointNet(tn, pn, 10, aux_ctc=True)
    with torch.no_grad():
        net.ctc_head.weight.mul_(8.0)      # logits with some contrast: an untrained head is close to uniform
    return net.cuda().eval()


@pytest.mark.parametrize("bidirectional", [False, True], ids=["uni", "bi"])
def test_model_level(bidirectional):
    from rnntransducer_amd.networks.encoder import lengths_to_device
    lens = [9, 6]
    x = torch.randn(2, 9, 12, generator=torch.Generator().manual_seed(5)).cuda()
    for seed in range(20):
        net = _jointnet(bidirectional, seed)
        tl = lengths_to_device(lens, x.device)
        z = net.ctc_head(net.encoder.forward_time_major(x, tl))              # (T, B, V)
        zc = z.detach().cpu().numpy()
        rest = [R.search(zc[:lens[b], b], 0, 1) for b in range(2)]
        if min(r[1] for r in rest) >= MARGIN:
            break
    else:
        pytest.fail("no model seed of 20 keeps the margin at W = 1")
    one = net.recognize_ctc_beams(x, lens, 0, 1, return_scores=True)
    for b in range(2):
        assert one[b][0][0] == rest[b][0][0]["tokens"]
        assert abs(one[b][0][1] - rest[b][0][0]["score"]) <= 1e-5 * abs(rest[b][0][0]["score"])
    from rnntransducer_amd.ops import ctc_beam_search
    direct = ctc_beam_search(z, tl, 0, 4, time_major=True, return_frames=True)
    full = net.recognize_ctc_beams(x, lens, 0, 4, return_scores=True, return_frames=True)
    assert full == direct
    assert net.recognize_ctc_beams(x, lens, 0, 4) == [[e[0] for e in hyps] for hyps in direct]
    assert net.recognize_ctc_beams(x, lens, 0, 4, return_frames=True) == [[(e[0], e[-1]) for e in hyps] for hyps in direct]
    single = net.recognize_ctc_beams(x[:1, :lens[0]], lens[:1], 0, 4, return_scores=True)       # one utterance: the list itself
    assert 1 <= len(single) <= 4 and all(isinstance(y, list) and isinstance(sc, float) for y, sc in single)
    fusion = fusion_for("hotwords", 10, 0, 0).to("cuda")
    fz = ctc_beam_search(z, tl, 0, 4, time_major=True, fusion=fusion)
    assert net.recognize_ctc_beams(x, lens, 0, 4, fusion=fusion, return_scores=True) == fz
    # guards: before any launch
    for kw in (dict(beam_widths=0), dict(beam_widths=129), dict(token_min_logp=math.nan), dict(fusion=fusion_for("zero", 9, 0, 0))):
        with pytest.raises(ValueError):
            net.recognize_ctc_beams(x, lens, 0, **kw)
    with pytest.raises(ValueError):
        net.recognize_ctc_beams(x, lens, 0, fusion=fusion_for("zero", 10, 0, 0))       # tables on the CPU, search on the GPU
    net.train()
    with pytest.raises(ValueError):
        net.recognize_ctc_beams(x, lens, 0)
