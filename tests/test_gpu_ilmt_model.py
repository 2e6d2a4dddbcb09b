"""Internal-LM training at model level (JointNet.loss(ilmt_weight=...), JointNet.ilm_loss, RNNTransducer with args.ilmt_weight)
against the float64 CPU oracle: OracleJointNet's RNN-T loss plus the internal-LM term restated in tests/ilmt_restatement.py on the
oracle's own prediction net and fc.  Tolerances are tests/test_gpu_ctc_model.py's: 1e-5 relative on losses, 2e-4 * max(|grad|max,
1e-2) on every parameter gradient.  Dropout is 0 everywhere, B = 3 ragged."""
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import usable_cores
from tests.ilmt_restatement import ilm_nll_autograd
from tests.test_gpu_ctc_model import LSTM1, SMALL, _cuda, _model

pytestmark = pytest.mark.gpu
W = 0.3
NLL_RTOL = 1e-5


@pytest.fixture(autouse=True, scope="module")
def _oracle_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(usable_cores())
    yield
    torch.set_num_threads(before)


def _oracle_of(model, cfg):
    from oracle.rnnt_oracle import OracleJointNet
    tn, pn, V = cfg
    sd = {k[len("jointnet."):]: v.double().cpu() for k, v in model.state_dict().items() if "ctc_head" not in k}
    oracle = OracleJointNet(dict(tn), dict(pn), V).double()
    oracle.load_state_dict(sd)
    return oracle


def _oracle_ilm(oracle, batch):
    """per-utterance internal-LM NLL (B,) in float64 from the oracle's prediction net and the decoder half of its fc."""
    texts, text_lens, targets, u_lens = batch[3], batch[4], batch[5], batch[6]
    dec = oracle.decoder(texts, text_lens)                                  # (B, U1, Od)
    Oe = oracle.fc.weight.shape[1] - dec.shape[-1]
    C = F.gelu(dec, approximate="tanh") @ oracle.fc.weight[:, Oe:].T        # (B, U1, V)
    return ilm_nll_autograd(C.transpose(0, 1), oracle.fc.bias, targets, u_lens.tolist(), 0)


def _oracle_rnnt(oracle, batch):
    from oracle.rnnt_oracle import _RNNTLossFn
    audios, audio_lens, t_lens, texts, text_lens, targets, u_lens = batch
    enc = oracle.encoder(audios.double(), audio_lens)
    return _RNNTLossFn.apply(oracle.joint(enc, oracle.decoder(texts, text_lens)), targets, t_lens, u_lens, 0)


def _check_grads(model, oracle, what="", only=None):
    ref = {k: p.grad for k, p in oracle.named_parameters()}
    for name, p in model.jointnet.named_parameters():
        if "ctc_head" in name or (only is not None and not name.startswith(only)):
            continue
        q = ref[name]
        scale = max(q.abs().max().item(), 1e-2)
        err = (p.grad.double().cpu() - q).abs().max().item()
        print(f"{what} {name}: err {err:.3g} scale {scale:.3g}")
        assert err < 2e-4 * scale, f"{what} {name}: {err} vs scale {scale}"


def _grads(model):
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.jointnet.named_parameters()}


def _loss_args(dev):
    return (dev[0], dev[2], dev[3], dev[5], dev[6], 0)


def test_training_step_with_the_ilm_term_matches_the_oracle():
    from oracle.rnnt_oracle import make_batch
    model = _model(LSTM1, aux=False, ilmt_weight=W)
    oracle = _oracle_of(model, LSTM1)
    batch = make_batch(3, 60, 9, 72, ragged=True, seed=31)
    r, i = _oracle_rnnt(oracle, batch), _oracle_ilm(oracle, batch)
    ref = r.mean() + W * i.mean()
    ref.backward()
    model = model.cuda().train()
    dev = _cuda(batch)
    out = model.training_step(dev, 0)["loss"]
    out.backward()
    assert out.dim() == 0 and abs(out.item() - ref.item()) < 1e-5 * abs(ref.item()), (out.item(), ref.item())
    _check_grads(model, oracle, "mean")
    with torch.no_grad():   # training_step is loss(..., ilmt_weight=args.ilmt_weight) with the collate's list of lengths
        same = model.jointnet.loss(*_loss_args(dev), reduction="mean", audio_lengths=dev[1], ilmt_weight=W)
        plain = model.jointnet.loss(*_loss_args(dev), reduction="mean", audio_lengths=dev[1])
    assert torch.equal(same, out.detach())
    assert abs(plain.item() - r.mean().item()) < 1e-5 * abs(r.mean().item()) and not torch.equal(plain, same)


def test_per_utterance_losses_in_collate_order_with_upstream_weights():
    """reduction="none" on rows in collate order (unsorted lengths: the module sorts them and un-sorts both terms), with a
    different upstream weight per utterance: the gvec path of both gradient kernels."""
    from oracle.rnnt_oracle import make_batch
    tn, pn, V = SMALL
    model = _model(SMALL, seed=2, aux=False)
    oracle = _oracle_of(model, SMALL)
    batch = list(make_batch(3, 40, 6, V, n_mels=12, ragged=True, seed=8))
    lens = [25, 40, 31]
    for b in range(3):
        batch[0][b, lens[b]:] = 0
    batch[1], batch[2] = lens, torch.tensor(lens, dtype=torch.int32)
    batch = tuple(batch)
    gw = torch.tensor([1.0, -0.5, 2.0], dtype=torch.float64)
    r, i = _oracle_rnnt(oracle, batch), _oracle_ilm(oracle, batch)
    ((r + W * i) * gw).sum().backward()
    model = model.cuda().train()
    dev = _cuda(batch)
    out = model.jointnet.loss(*_loss_args(dev), audio_lengths=dev[1], ilmt_weight=W)
    assert out.shape == (3,) and torch.allclose(out.double().cpu(), (r + W * i).detach(), rtol=1e-5, atol=0)
    (out * gw.float().cuda()).sum().backward()
    _check_grads(model, oracle, "none")
    for reduction, want in (("sum", (r + W * i).sum()), ("mean", (r + W * i).mean())):
        with torch.no_grad():
            got = model.jointnet.loss(*_loss_args(dev), reduction=reduction, ilmt_weight=W)
        assert got.dim() == 0 and abs(got.item() - want.item()) < 1e-5 * abs(want.item())


def test_zero_weight_changes_no_bit_and_the_term_leaves_the_encoder_alone():
    from oracle.rnnt_oracle import make_batch
    dev = _cuda(make_batch(3, 60, 9, 72, ragged=True, seed=3))
    model = _model(LSTM1, seed=4, aux=False).cuda().train()
    res = []
    for kw in (dict(), dict(ilmt_weight=0), dict(ilmt_weight=0.0), dict(ilmt_weight=W)):
        model.zero_grad(set_to_none=True)
        loss = model.jointnet.loss(*_loss_args(dev), reduction="mean", audio_lengths=dev[1], **kw)
        loss.backward()
        res.append((loss.detach().clone(), _grads(model)))
    (l0, g0), (la, ga), (lb, gb), (lw, gw) = res
    for l, g in ((la, ga), (lb, gb)):
        assert torch.equal(l, l0) and all(torch.equal(g[k], g0[k]) for k in g0)
    assert not torch.equal(lw, l0)
    for k in g0:
        if k.startswith("encoder."):     # the internal LM has no encoder: these gradients are the lattice's, bit for bit
            assert torch.equal(gw[k], g0[k]), k
        elif k.startswith("fc."):
            assert not torch.equal(gw[k], g0[k]), k


def test_composition_with_fastemit_windows_and_ctc():
    from oracle.rnnt_oracle import make_batch
    from rnntransducer_amd.ops import emit_windows
    tn, pn, V = SMALL
    B, T, U, CW = 3, 40, 6, 0.4
    batch = make_batch(B, T, U, V, n_mels=12, ragged=True, seed=12)
    dev = _cuda(batch)
    frames = torch.stack([((torch.arange(U) + 0.5) * batch[1][b] / max(int(batch[6][b]), 1)).long().clamp(0, T - 1) for b in range(B)])
    win = emit_windows(frames.cuda(), dev[2], dev[6], 12, 12)
    model = _model(SMALL, seed=6, aux=True).cuda().train()
    kw = dict(reduction="mean", audio_lengths=dev[1], ctc_weight=CW, fastemit_lambda=0.01, emit_windows=win)

    def grads_of(fn):
        model.zero_grad(set_to_none=True)
        out = fn()
        (out[0] if isinstance(out, tuple) else out).backward()
        return out, _grads(model)

    parts, g_all = grads_of(lambda: model.jointnet.loss(*_loss_args(dev), ilmt_weight=W, return_parts=True, **kw))
    base, g_base = grads_of(lambda: model.jointnet.loss(*_loss_args(dev), return_parts=True, **kw))
    ilm, g_ilm = grads_of(lambda: model.jointnet.ilm_loss(dev[3], dev[5], dev[6], 0, reduction="mean"))
    assert len(parts) == 4 and len(base) == 3 and all(p.dim() == 0 and torch.isfinite(p) for p in parts)
    total, rnnt, ctc, ilm_part = (p.detach() for p in parts)
    assert torch.equal(total, rnnt + CW * ctc + W * ilm_part)
    assert torch.equal(rnnt, base[1].detach()) and torch.equal(ctc, base[2].detach())   # the other terms: untouched, bit for bit
    # the same kernel on the same C; loss() runs the rows length-sorted, so the batch mean adds them in another order
    assert torch.allclose(ilm_part, ilm.detach(), rtol=2e-6, atol=0)
    for k, g in g_all.items():
        want = g_base[k].double() + (0.0 if g_ilm[k] is None else W * g_ilm[k].double())
        scale = max(want.abs().max().item(), 1e-2)
        assert (g.double() - want).abs().max().item() < 2e-4 * scale, k
    with torch.no_grad():   # per-utterance parts
        pn_ = model.jointnet.loss(*_loss_args(dev), ilmt_weight=W, return_parts=True, ctc_weight=CW, audio_lengths=dev[1])
    assert len(pn_) == 4 and all(p.shape == (B,) for p in pn_)
    assert torch.equal(pn_[0], pn_[1] + CW * pn_[2] + W * pn_[3])


def test_text_only_ilm_loss_matches_the_oracle_and_spares_the_encoder():
    from oracle.rnnt_oracle import make_batch
    model = _model(LSTM1, seed=9, aux=False)
    oracle = _oracle_of(model, LSTM1)
    batch = make_batch(3, 20, 11, 72, ragged=True, seed=17)
    gw = torch.tensor([0.5, 2.0, -1.0], dtype=torch.float64)
    i = _oracle_ilm(oracle, batch)
    (i * gw).sum().backward()
    model = model.cuda().train()
    dev = _cuda(batch)
    Oe = model.jointnet.enc_out
    out = model.jointnet.ilm_loss(dev[3], dev[5], dev[6], 0)
    assert out.shape == (3,) and torch.allclose(out.double().cpu(), i.detach(), rtol=NLL_RTOL, atol=0)
    (out * gw.float().cuda()).sum().backward()
    for name, p in model.jointnet.named_parameters():
        if name.startswith("encoder."):
            assert p.grad is None, name
    assert torch.all(model.jointnet.fc.weight.grad[:, :Oe] == 0)
    oracle.fc.weight.grad[:, :Oe] = 0.0                          # (autograd gives exact zeros there too)
    _check_grads(model, oracle, "text-only", only=("decoder.", "fc."))
    for reduction, want in (("sum", i.sum()), ("mean", i.mean())):
        with torch.no_grad():
            got = model.jointnet.ilm_loss(dev[3], dev[5], dev[6], 0, reduction=reduction)
        assert got.dim() == 0 and abs(got.item() - want.item()) < NLL_RTOL * abs(want.item())
    with torch.no_grad():
        assert torch.equal(model.ilm_loss(dev[3], dev[5], dev[6]), got)      # RNNTransducer.ilm_loss: the model's blank, "mean"


def test_eval_route_is_minus_ilm_score():
    from oracle.rnnt_oracle import make_batch
    model = _model(LSTM1, seed=1, aux=False).cuda().eval()
    dev = _cuda(make_batch(3, 20, 11, 72, ragged=True, seed=5))
    with torch.no_grad():
        got = model.jointnet.ilm_loss(dev[3], dev[5], dev[6], 0)
    want = -model.jointnet.ilm_score(dev[5], dev[6], 0)
    assert want.dtype == torch.float64 and torch.all(want > 0)
    assert torch.allclose(got.double(), want, rtol=NLL_RTOL, atol=0), (got, want)


@pytest.mark.parametrize("text_only", [False, True], ids=["loss", "ilm_loss"])
def test_flat_gradients_equal_the_autograd_path(text_only):
    """FlatAdamW(direct_grads=True): the backward adds into the flat gradient views (fc.weight's decoder columns, fc.bias from
    dC's column sums); after one backward the flat buffer holds what autograd's own accumulation gives."""
    from oracle.rnnt_oracle import make_batch
    from rnntransducer_amd.optim import FlatAdamW
    dev = _cuda(make_batch(3, 60, 9, 72, ragged=True, seed=23))
    res = []
    for direct in (False, True):
        model = _model(LSTM1, seed=7, aux=False, direct_flat_grads=direct).cuda().train()
        if direct:
            opt = model.configure_optimizers()["optimizer"]
            assert isinstance(opt, FlatAdamW) and opt.flat.direct_grads
            opt.zero_grad()
        if text_only:
            loss = model.ilm_loss(dev[3], dev[5], dev[6])
        else:
            loss = model.jointnet.loss(*_loss_args(dev), reduction="mean", audio_lengths=dev[1], ilmt_weight=W)
        loss.backward()
        res.append((loss.detach().clone(), _grads(model)))
    (la, ga), (lb, gb) = res
    assert torch.equal(la, lb)
    for k, g in ga.items():
        if g is None:                    # text-only, autograd path: no encoder gradient; the flat view stays zero
            assert k.startswith("encoder.") and torch.all(gb[k] == 0), k
            continue
        scale = max(g.abs().max().item(), 1e-2)
        assert (gb[k] - g).abs().max().item() < 2e-4 * scale, k
    if text_only:
        assert torch.all(gb["fc.weight"][:, :model.jointnet.enc_out] == 0)
