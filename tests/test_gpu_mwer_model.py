"""MWER training end to end (JointNet.mwer_loss, RNNTransducer with args.mwer_weight) against float64 autograd through the oracle
networks, on the tiny configs of tests/test_gpu_ctc_model.py, B = 3 ragged, N = 4, max_symbols = 2 (tests/mwer_cases.py).

The gradient check factors the softmax out: with the hypotheses and the fp32 NLLs the DEVICE produced, the restatement's weights
w_j = d risk / d nll_j are constants, and the exact chain rule gives the parameter gradient of the step as that of
mean(rnnt_ref) + mwer_weight * sum_j w_j nll_j — float64 autograd of which, through OracleJointNet, is the reference, held to the
project's bound 2e-4 * max(|ref|max, 1e-2).  The total loss is compared with the all-float64 value within
2 * mwer_weight * max|W - Wbar| * max|nll_device - nll_oracle| + 1e-5 * |rnnt|: the first-order sensitivity of the softmax to the
NLL error, times 2, plus tests/test_gpu_ctc_model.py's relative loss tolerance on the reference-row term."""
import numpy as np
import pytest
import torch

from rnntransducer_amd.metrics import edit_distance
from tests import mwer_cases as M
from tests.conftest import usable_cores
from tests.mwer_restatement import risk_and_weights

pytestmark = pytest.mark.gpu
MW = 0.5


@pytest.fixture(autouse=True, scope="module")
def _oracle_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(usable_cores())
    yield
    torch.set_num_threads(before)


def _cuda(batch):
    return tuple(x.cuda() if isinstance(x, torch.Tensor) else x for x in batch)


def _record(monkeypatch):
    """What mwer_loss hands to the edit distance and the risk, recorded: the packed hypotheses (rows in the encoder's
    length-sorted order), the sorted references, the device distances, NLLs and the valid flags."""
    from rnntransducer_amd.networks import transducer as TR
    rec = {}
    real_ed, real_risk = TR.edit_distance, TR.MwerRiskFn

    def ed(labels, u_lens, targets, ref_lens, ref_div):
        dist = real_ed(labels, u_lens, targets, ref_lens, ref_div)
        rec.update(labels=labels.cpu(), u_lens=u_lens.cpu(), targets=targets.cpu(), ref_lens=ref_lens.cpu(), dist=dist.cpu())
        return dist

    class Risk:
        @staticmethod
        def apply(nll, dist, valid, n, reduction):
            rec.update(nll=nll.detach().cpu(), valid=valid.cpu(), risk_dist=dist.cpu())
            return real_risk.apply(nll, dist, valid, n, reduction)
    monkeypatch.setattr(TR, "edit_distance", ed)
    monkeypatch.setattr(TR, "MwerRiskFn", Risk)
    return rec


@pytest.fixture(scope="module")
def reference():
    """Per case and per recorded device result: the float64 values, computed once and shared by the direct_grads on / off runs
    when the device returns the same hypotheses and NLL bits in both (it does: the forward does not depend on the optimizer)."""
    return {}


def _oracle_reference(name, rec):
    c = M.cpu_case(name)
    oracle, batch = c["oracle"], c["batch"]
    lens = batch[1]
    order = sorted(range(M.B), key=lambda b: (-lens[b], b))                  # the encoder's row order
    refs = M.references(batch)
    hyps, nll_dev, W = [None] * M.B, [None] * M.B, [None] * M.B
    for i, b in enumerate(order):
        rows = [i * M.N + n for n in range(M.N) if rec["valid"][i * M.N + n]]
        assert rec["targets"][i, :rec["ref_lens"][i]].tolist() == refs[b]
        hyps[b] = [rec["labels"][r, :rec["u_lens"][r]].tolist() for r in rows]
        nll_dev[b] = [float(rec["nll"][r]) for r in rows]
        W[b] = [edit_distance(y, refs[b]) for y in hyps[b]]
        assert [int(rec["dist"][r]) for r in rows] == W[b]                    # the device's distances are the host's
    weights = [risk_and_weights(nll_dev[b], W[b], [True] * len(W[b]))[1] for b in range(M.B)]
    oracle.zero_grad()
    from oracle.rnnt_oracle import _RNNTLossFn
    audios, audio_lens, t_lens, texts, text_lens, targets, u_lens = batch
    rnnt = _RNNTLossFn.apply(oracle(audios.double(), audio_lens, texts, text_lens), targets, t_lens, u_lens, 0)
    nll64 = M.oracle_nbest_nll(oracle, batch, hyps)
    flat_w = torch.tensor([w for ws in weights for w in ws], dtype=torch.float64)
    (rnnt.mean() + MW * (flat_w * nll64).sum() / M.B).backward()
    grads = {k: p.grad.clone() for k, p in oracle.named_parameters()}
    nll64 = M.split_rows(nll64.detach().tolist(), hyps)
    risk64 = [risk_and_weights(nll64[b], W[b], [True] * len(W[b]))[0] for b in range(M.B)]
    return dict(hyps=hyps, W=W, weights=weights, nll_dev=nll_dev, nll64=nll64, grads=grads, rnnt=rnnt.detach().mean().item(),
                risk=float(np.mean(risk64)), cpu_hyps=c["hyps"])


@pytest.mark.parametrize("direct", [False, True], ids=["autograd-accumulation", "direct-grads"])
@pytest.mark.parametrize("name", sorted(M.CASES))
def test_mwer_step_matches_float64_autograd(name, direct, monkeypatch, reference):
    cfg, seed = M.CASES[name]["cfg"], M.CASES[name]["seed"]
    rec = _record(monkeypatch)
    model = M.build_model(cfg, seed, direct_flat_grads=direct).cuda().train()
    dev = _cuda(M.cpu_case(name)["batch"])
    opt = model.configure_optimizers()["optimizer"]
    assert opt.flat.direct_grads == direct
    opt.zero_grad()
    total, rnnt, risk, err1 = model.jointnet.mwer_loss(dev[0], dev[2], dev[3], dev[5], dev[6], 0, nbest=M.N, max_symbols=M.S,
                                                       mwer_weight=MW, reduction="mean", audio_lengths=dev[1], return_parts=True)
    total.backward()
    key = (name, rec["nll"].numpy().tobytes(), rec["labels"].numpy().tobytes())
    if key not in reference:
        reference[key] = _oracle_reference(name, rec)
    ref = reference[key]
    # non-vacuity, on what the device produced
    assert M.non_vacuous(ref["W"], ref["weights"]), (ref["W"], ref["weights"])
    assert sorted(map(tuple, sum(ref["hyps"], []))) == sorted(map(tuple, sum(ref["cpu_hyps"], [])))   # the lists of the fp64 search
    # the loss
    want = ref["rnnt"] + MW * ref["risk"]
    spread = max(abs(w - np.mean(ws)) for ws in ref["W"] for w in ws)
    nll_err = max(abs(a - b) for da, db in zip(ref["nll_dev"], ref["nll64"]) for a, b in zip(da, db))
    bound = 2 * MW * spread * nll_err + 1e-5 * abs(ref["rnnt"])
    print(f"{name} direct={direct}: total {total.item():.8f} want {want:.8f} |diff| {abs(total.item() - want):.3g} bound {bound:.3g} "
          f"(max|W - Wbar| {spread:.3g}, max nll error {nll_err:.3g}); risk {risk.item():.6f} want {ref['risk']:.6f}; "
          f"max|w| {max(abs(w) for ws in ref['weights'] for w in ws):.3g}")
    assert abs(total.item() - want) <= bound
    assert abs(rnnt.item() - ref["rnnt"]) <= 1e-5 * abs(ref["rnnt"])
    assert torch.equal(total, rnnt + MW * risk)
    best = [ws[0] for ws in ref["W"]]
    assert abs(err1.item() - float(np.mean(best))) < 1e-6
    # the gradients
    for pname, p in model.jointnet.named_parameters():
        q = ref["grads"][pname]
        scale = max(q.abs().max().item(), 1e-2)
        err = (p.grad.double().cpu() - q).abs().max().item()
        assert err < 2e-4 * scale, f"{name} direct={direct} {pname}: {err} vs scale {scale}"


def test_zero_weight_is_todays_training_step_bit_for_bit():
    cfg, seed = M.CASES["bilstm1"]["cfg"], M.CASES["bilstm1"]["seed"]
    dev = _cuda(M.make_case_batch(seed))
    res = []
    for kw in (dict(), dict(mwer_weight=0.0, mwer_nbest=M.N, mwer_max_symbols=M.S)):
        model = M.build_model(cfg, seed, **kw).cuda().train()
        loss = model.training_step(dev, 0)["loss"]
        loss.backward()
        res.append((loss.detach(), [p.grad for p in model.parameters()]))
    (la, ga), (lb, gb) = res
    assert torch.equal(la, lb) and all(torch.equal(a, b) for a, b in zip(ga, gb))


def test_two_identical_steps_are_bitwise_equal_and_the_optimizer_moves():
    cfg, seed = M.CASES["bilstm1"]["cfg"], M.CASES["bilstm1"]["seed"]
    dev = _cuda(M.make_case_batch(seed))

    def run():
        model = M.build_model(cfg, seed, mwer_weight=MW, mwer_nbest=M.N, mwer_max_symbols=M.S).cuda().train()
        before = [p.detach().clone() for p in model.parameters()]
        opt = model.configure_optimizers()["optimizer"]
        opt.zero_grad()
        loss = model.training_step(dev, 0)["loss"]
        loss.backward()
        grads = [p.grad.clone() for p in model.parameters()]
        opt.step()
        return loss.detach(), grads, before, [p.detach().clone() for p in model.parameters()], model, opt
    la, ga, before, after, model, opt = run()
    lb, gb, _, after_b, _, _ = run()
    from rnntransducer_amd.optim import FlatAdamW
    assert isinstance(opt, FlatAdamW)
    assert torch.equal(la, lb) and all(torch.equal(a, b) for a, b in zip(ga, gb)) and all(torch.equal(a, b) for a, b in zip(after, after_b))
    assert all((a - b).abs().max().item() > 1e-6 for a, b in zip(after, before))
    # the MWER term is in the step: the loss and the gradients differ from the plain step's
    plain = M.build_model(cfg, seed).cuda().train()
    lp = plain.training_step(dev, 0)["loss"]
    lp.backward()
    assert not torch.equal(lp.detach(), la)
    assert any(not torch.equal(p.grad, g) for p, g in zip(plain.parameters(), ga))


def test_per_utterance_reduction_comes_back_in_the_callers_order(monkeypatch):
    """reduction="none" on the ragged batch (the rows are sorted inside): every part is (B,), the reference-row part is loss()'s,
    and the mean of the risks is the "mean" call's."""
    cfg, seed = M.CASES["bilstm1"]["cfg"], M.CASES["bilstm1"]["seed"]
    dev = _cuda(M.make_case_batch(seed))
    net = M.build_model(cfg, seed).cuda().train().jointnet
    kw = dict(nbest=M.N, max_symbols=M.S, mwer_weight=MW, audio_lengths=dev[1], return_parts=True)
    with torch.no_grad():
        total, rnnt, risk, err1 = net.mwer_loss(dev[0], dev[2], dev[3], dev[5], dev[6], 0, reduction="none", **kw)
        mean = net.mwer_loss(dev[0], dev[2], dev[3], dev[5], dev[6], 0, reduction="mean", **kw)
        plain = net.loss(dev[0], dev[2], dev[3], dev[5], dev[6], 0, reduction="none", audio_lengths=dev[1])
    assert total.shape == rnnt.shape == risk.shape == (M.B,) and err1.dim() == 0
    assert torch.equal(rnnt, plain) and torch.equal(total, rnnt + MW * risk)
    # the same B fp32 risks, summed in fp32 by the library instead of by torch: a few roundings of the largest of them
    assert abs(risk.mean().item() - mean[2].item()) <= 4 * 2.0 ** -23 * risk.abs().max().item() and torch.equal(err1, mean[3])
    order = sorted(range(M.B), key=lambda b: (-dev[1][b], b))
    assert order != list(range(M.B))                                           # the rows did move inside
    rec = _record(monkeypatch)
    with torch.no_grad():
        again = net.mwer_loss(dev[0], dev[2], dev[3], dev[5], dev[6], 0, reduction="none", **kw)
    assert torch.equal(again[2], risk)
    refs = M.references(M.make_case_batch(seed))
    for b in range(M.B):   # what the risk kernel saw for utterance b: its own hypotheses against its own transcript
        i = order.index(b)
        ok = [n for n in range(M.N) if rec["valid"][b * M.N + n]]
        W = [edit_distance(rec["labels"][i * M.N + n, :rec["u_lens"][i * M.N + n]].tolist(), refs[b]) for n in ok]
        assert [int(rec["risk_dist"][b * M.N + n]) for n in ok] == W and len(ok) >= 2
        want = risk_and_weights([float(rec["nll"][b * M.N + n]) for n in ok], W, [True] * len(ok))[0]
        assert abs(risk[b].item() - want) <= 2.0 ** -23 * abs(want) + 1e-12
