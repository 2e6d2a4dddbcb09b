"""Lattice knowledge distillation at model level (JointNet.cell_logprobs, JointNet.loss(kd_teacher=, kd_weight=), RNNTransducer with
args.kd_weight and set_teacher) against the float64 CPU composite: the networks of oracle/ for the teacher and the student, the
materialised collapsed KL of tests/kd_restatement.py on their joint outputs, the transducer term (and FastEmit's gradient) of
tests/fastemit_restatement.py.  Tolerances are tests/test_gpu_ilmt_model.py's: 1e-5 relative on losses, 2e-4 * max(|grad|max, 1e-2)
on every parameter gradient.  A bidirectional 2x32 LSTM teacher, a unidirectional student; dropout 0, B = 3 ragged."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import fastemit_restatement as fr
from tests import kd_restatement as kr
from tests.conftest import usable_cores

pytestmark = pytest.mark.gpu
KW, V, MELS = 0.5, 9, 12
TEACHER = dict(input_size=MELS, hidden_size=32, output_size=16, num_layers=2, rnn_type="lstm", dropout=0.0, bidirectional=True)
STUDENT = dict(input_size=MELS, hidden_size=32, output_size=16, num_layers=1, rnn_type="lstm", dropout=0.0, bidirectional=False)
PRED = dict(embedding_size=V, pad_token_id=0, hidden_size=16, output_size=8, num_layers=1, rnn_type="lstm", dropout=0.0)


@pytest.fixture(autouse=True, scope="module")
def _oracle_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(usable_cores())
    yield
    torch.set_num_threads(before)


def _model(tn, seed, classes=V, **args):
    from rnntransducer_amd import RNNTransducer
    torch.manual_seed(seed)
    ns = Namespace(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=100,
                   move_metrics_to_cpu=False, **args)
    return RNNTransducer(dict(PRED, embedding_size=classes), dict(tn), dict(num_classes=classes), ns)


def _oracle_of(model, tn):
    from oracle.rnnt_oracle import OracleJointNet
    oracle = OracleJointNet(dict(tn), dict(PRED), V).double()
    oracle.load_state_dict({k[len("jointnet."):]: v.double().cpu() for k, v in model.state_dict().items()})
    return oracle


def _cuda(batch):
    return tuple(x.cuda() if isinstance(x, torch.Tensor) else x for x in batch)


def _logits(oracle, batch):
    audios, audio_lens, _, texts, text_lens = batch[:5]
    return oracle.joint(oracle.encoder(audios.double(), audio_lens), oracle.decoder(texts, text_lens))


def _composite(student, teacher, batch, lam):
    """float64: -> rnnt (B,), kd (B,) and, after this call, the student oracle's .grad of mean(rnnt) + KW mean(kd) (FastEmit's
    gradient for the transducer term when lam > 0)."""
    t_lens, targets, u_lens = batch[2].tolist(), batch[5].numpy(), batch[6].tolist()
    with torch.no_grad():
        planes = kr.planes_from_logits(_logits(teacher, batch).numpy(), targets, u_lens, 0)
    z = _logits(student, batch)
    nll, dz = fr.fastemit_loss(z.detach().numpy(), targets, t_lens, u_lens, 0, lam)
    kd = kr.kd_autograd_from_logits(z, targets, t_lens, u_lens, 0, planes)
    B = z.shape[0]
    ((z * torch.from_numpy(dz / B)).sum() + KW * kd.mean()).backward()
    return torch.from_numpy(nll), kd.detach(), planes


def _check_grads(model, oracle, what):
    ref = {k: p.grad for k, p in oracle.named_parameters()}
    for name, p in model.jointnet.named_parameters():
        q = ref[name]
        scale = max(q.abs().max().item(), 1e-2)
        err = (p.grad.double().cpu() - q).abs().max().item()
        print(f"{what} {name}: err {err:.3g} scale {scale:.3g}")
        assert err < 2e-4 * scale, f"{what} {name}: {err} vs scale {scale}"


def _grads(model):
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.jointnet.named_parameters()}


def _batch(seed=5):
    from oracle.rnnt_oracle import make_batch
    return make_batch(3, 33, 5, V, n_mels=MELS, ragged=True, seed=seed)


@pytest.mark.parametrize("lam", [0.0, 0.5], ids=("plain", "fastemit"))
def test_training_step_matches_the_float64_composite(lam):
    teacher, student = _model(TEACHER, 1), _model(STUDENT, 2, kd_weight=KW, fastemit_lambda=lam)
    t_or, s_or = _oracle_of(teacher, TEACHER), _oracle_of(student, STUDENT)
    batch = _batch()
    rnnt, kd, planes = _composite(s_or, t_or, batch, lam)
    ref = rnnt.mean() + KW * kd.mean()
    teacher, student = teacher.cuda(), student.cuda().train()
    student.set_teacher(teacher)
    dev = _cuda(batch)
    out = student.training_step(dev, 0)["loss"]
    out.backward()
    print(f"loss {out.item():.7f} composite {ref.item():.7f} (rnnt {rnnt.mean().item():.6f} kd {kd.mean().item():.6f})")
    assert out.dim() == 0 and abs(out.item() - ref.item()) < 1e-5 * abs(ref.item())
    _check_grads(student, s_or, f"lambda {lam}")
    assert all(p.grad is None for p in teacher.parameters())
    # the teacher's planes, in the caller's (collate) row order, against the float64 ones
    got = teacher.jointnet.cell_logprobs(dev[0], dev[2], dev[3], dev[5], dev[6], 0, audio_lengths=dev[1])
    for b in range(3):
        tb, ub = batch[1][b], int(batch[6][b])
        for k, name in enumerate(("blk", "emit", "rest")):
            nu = ub if k == 1 else ub + 1
            err = np.abs(got[k][b, :nu, :tb].double().cpu().numpy() - planes[k][b, :nu, :tb]).max() if nu else 0.0
            assert err < 2e-4, (name, b, err)
    # the parts, per utterance, in collate order
    with torch.no_grad():
        parts = student.jointnet.loss(dev[0], dev[2], dev[3], dev[5], dev[6], 0, audio_lengths=dev[1], kd_teacher=got, kd_weight=KW,
                                      fastemit_lambda=lam, return_parts=False)
        only = student.jointnet.loss(dev[0], dev[2], dev[3], dev[5], dev[6], 0, audio_lengths=dev[1])
    assert parts.shape == (3,) and torch.allclose(parts.double().cpu(), rnnt + KW * kd, rtol=1e-5, atol=0)
    assert torch.allclose(only.double().cpu(), rnnt, rtol=1e-5, atol=0)


def test_unsorted_rows_and_upstream_weights():
    """reduction="none" on rows whose lengths are not sorted (the module sorts them; the planes follow their rows), a different
    upstream weight per utterance, and return_parts on a model with the CTC head."""
    from rnntransducer_amd import RNNTransducer
    torch.manual_seed(3)
    ns = Namespace(move_metrics_to_cpu=False)
    student = RNNTransducer(dict(PRED), dict(STUDENT), dict(num_classes=V, aux_ctc=True), ns)
    teacher = _model(TEACHER, 4)
    batch = list(_batch(seed=8))
    lens = [20, 33, 27]
    for b in range(3):
        batch[0][b, lens[b]:] = 0
    batch[1], batch[2] = lens, torch.tensor(lens, dtype=torch.int32)
    batch = tuple(batch)
    t_or = _oracle_of(teacher, TEACHER)
    from oracle.rnnt_oracle import OracleJointNet
    s_or = OracleJointNet(dict(STUDENT), dict(PRED), V).double()
    s_or.load_state_dict({k[len("jointnet."):]: v.double() for k, v in student.state_dict().items() if "ctc_head" not in k})
    t_lens, targets, u_lens = lens, batch[5].numpy(), batch[6].tolist()
    with torch.no_grad():
        planes = kr.planes_from_logits(_logits(t_or, batch).numpy(), targets, u_lens, 0)
    z = _logits(s_or, batch)
    nll, dz = fr.fastemit_loss(z.detach().numpy(), targets, t_lens, u_lens, 0, 0.0)
    kd = kr.kd_autograd_from_logits(z, targets, t_lens, u_lens, 0, planes)
    gw = torch.tensor([1.0, -0.5, 2.0], dtype=torch.float64)
    ((z * torch.from_numpy(dz) * gw.view(-1, 1, 1, 1)).sum() + KW * (kd * gw).sum()).backward()
    teacher, student = teacher.cuda().eval(), student.cuda().train()
    dev = _cuda(batch)
    tp = teacher.jointnet.cell_logprobs(dev[0], dev[2], dev[3], dev[5], dev[6], 0, audio_lengths=dev[1])
    parts = student.jointnet.loss(dev[0], dev[2], dev[3], dev[5], dev[6], 0, audio_lengths=dev[1], kd_teacher=tp, kd_weight=KW,
                                  return_parts=True)
    assert len(parts) == 4 and all(p.shape == (3,) for p in parts)
    total, rnnt_p, _, kd_p = parts
    assert torch.equal(total.detach(), (rnnt_p + KW * kd_p).detach())
    assert torch.allclose(rnnt_p.detach().double().cpu(), torch.from_numpy(nll), rtol=1e-5, atol=0)
    # the kd part alone: its class terms cancel (two freshly initialised models nearly agree), so 1e-5 of their absolute sum,
    # as tests/test_gpu_kd.py bounds the kernel's value
    _, mag = kr.kd_value(kr.planes_from_logits(z.detach().numpy(), targets, u_lens, 0), planes, t_lens, u_lens)
    err = (kd_p.detach().double().cpu() - kd.detach()).abs().numpy()
    print(f"kd {kd.detach().numpy()} err {err} bound {1e-5 * mag}")
    assert np.all(err <= 1e-5 * mag)
    (total * gw.float().cuda()).sum().backward()
    ref = {k: p.grad for k, p in s_or.named_parameters()}
    for name, p in student.jointnet.named_parameters():
        if "ctc_head" in name:
            continue
        scale = max(ref[name].abs().max().item(), 1e-2)
        err = (p.grad.double().cpu() - ref[name]).abs().max().item()
        assert err < 2e-4 * scale, f"{name}: {err} vs scale {scale}"


def test_off_means_off():
    """kd_weight = 0 (with a teacher set) and a positive weight without a teacher (JointNet.loss) are bitwise the step of a model built
    without the argument; set_teacher leaves state_dict and parameters alone; the teacher receives no gradient."""
    dev = _cuda(_batch(seed=9))
    teacher = _model(TEACHER, 1).cuda()
    res = []
    for args, with_teacher in ((dict(), False), (dict(kd_weight=0.0), True), (dict(kd_weight=0), True), (dict(kd_weight=KW), True)):
        model = _model(STUDENT, 2, **args).cuda().train()
        keys = list(model.state_dict().keys())
        if with_teacher:
            model.set_teacher(teacher)
            assert list(model.state_dict().keys()) == keys and not any(k.startswith("_kd") for k in keys)
        loss = model.training_step(dev, 0)["loss"]
        loss.backward()
        res.append((loss.detach().clone(), _grads(model)))
    (l0, g0), (la, ga), (lb, gb), (lw, gw) = res
    for l, g in ((la, ga), (lb, gb)):
        assert torch.equal(l, l0) and all(torch.equal(g[k], g0[k]) for k in g0)
    assert not torch.equal(lw, l0) and any(not torch.equal(gw[k], g0[k]) for k in g0)
    assert all(p.grad is None and not p.requires_grad for p in teacher.parameters())
    model = _model(STUDENT, 2).cuda().train()
    tp = teacher.jointnet.cell_logprobs(dev[0], dev[2], dev[3], dev[5], dev[6], 0, audio_lengths=dev[1])
    args = (dev[0], dev[2], dev[3], dev[5], dev[6], 0)
    for kw in (dict(kd_weight=KW), dict(kd_teacher=tp), dict(kd_teacher=tp, kd_weight=0.0)):
        model.zero_grad(set_to_none=True)
        loss = model.jointnet.loss(*args, reduction="mean", audio_lengths=dev[1], **kw)
        loss.backward()
        assert torch.equal(loss.detach(), l0) and all(torch.equal(g, g0[k]) for k, g in _grads(model).items())


def test_refusals():
    from rnntransducer_amd.ops import CellLogProbs, emit_windows
    dev = _cuda(_batch(seed=9))
    B, T, U = 3, 33, 5
    teacher, model = _model(TEACHER, 1).cuda(), _model(STUDENT, 2).cuda().train()
    args = (dev[0], dev[2], dev[3], dev[5], dev[6], 0)
    with pytest.raises(RuntimeError, match="eval"):
        teacher.train().jointnet.cell_logprobs(*args)
    tp = teacher.eval().jointnet.cell_logprobs(*args, audio_lengths=dev[1])
    assert all(p.shape == (B, U + 1, T) and p.dtype == torch.float32 and not p.requires_grad for p in tp)
    win = emit_windows(torch.zeros(B, U, dtype=torch.int32, device="cuda"), dev[2], dev[6], 40, 40)
    bad = [dict(kd_teacher=tp, kd_weight=KW, emit_windows=win), dict(kd_teacher=tp, kd_weight=-1.0), dict(kd_teacher=tp, kd_weight=float("inf")),
           dict(kd_teacher=CellLogProbs(tp.blk, tp.emit, tp.rest[:, :, :-1]), kd_weight=KW),
           dict(kd_teacher=CellLogProbs(tp.blk.double(), tp.emit, tp.rest), kd_weight=KW),
           dict(kd_teacher=CellLogProbs(tp.blk, tp.emit.cpu(), tp.rest), kd_weight=KW), dict(kd_teacher=tp[:2], kd_weight=KW)]
    for kw in bad:
        with pytest.raises(ValueError):
            model.jointnet.loss(*args, **kw)
    with pytest.raises(TypeError):
        model.jointnet.mwer_loss(*args, kd_teacher=tp)
    two = _model(STUDENT, 2, classes=2).cuda()
    t2 = (dev[0], dev[2], dev[3].clamp(max=1), dev[5].clamp(max=1), dev[6], 0)
    with pytest.raises(ValueError, match="at least 3"):
        two.eval().jointnet.cell_logprobs(*t2)
    with pytest.raises(ValueError, match="at least 3"):
        two.train().jointnet.loss(*t2, kd_teacher=tp, kd_weight=KW)
    with pytest.raises(ValueError, match="vocabulary"):
        two.set_teacher(teacher)


def test_one_flat_adamw_step_with_direct_grads():
    """FlatAdamW(direct_grads=True): the KD backward adds into the flat gradient views; the flat buffer holds what autograd's own
    accumulation gives, and one optimizer step runs."""
    from rnntransducer_amd.optim import FlatAdamW
    dev = _cuda(_batch(seed=13))
    teacher = _model(TEACHER, 1).cuda()
    res = []
    for direct in (False, True):
        model = _model(STUDENT, 7, kd_weight=KW, fastemit_lambda=0.01, direct_flat_grads=direct).cuda().train().set_teacher(teacher)
        if direct:
            opt = model.configure_optimizers()["optimizer"]
            assert isinstance(opt, FlatAdamW) and opt.flat.direct_grads
            opt.zero_grad()
        before = {k: p.detach().clone() for k, p in model.jointnet.named_parameters()}
        loss = model.training_step(dev, 0)["loss"]
        loss.backward()
        res.append((loss.detach().clone(), _grads(model)))
        if direct:
            opt.step()
            after = dict(model.jointnet.named_parameters())
            assert all(torch.isfinite(p).all() for p in after.values()) and all(not torch.equal(before[k], after[k]) for k in before)
    (la, ga), (lb, gb) = res
    assert torch.equal(la, lb)
    for k, g in ga.items():
        scale = max(g.abs().max().item(), 1e-2)
        assert (gb[k] - g).abs().max().item() < 2e-4 * scale, k
