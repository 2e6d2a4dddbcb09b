"""Shared inputs of the end-to-end MWER tests (CPU and GPU): the tiny models of tests/test_gpu_ctc_model.py (config-1 dims with a
bi-LSTM encoder, and a two-layer bi-GRU encoder), a ragged batch of B = 3, N = 4 hypotheses and max_symbols = 2, with the seed at
which the float64 restatement of the search (tests/beam_sync_restatement.py) on the oracle networks gives a non-trivial MWER
problem: a decision margin >= 1e-4 (fp32 against fp64 log-probabilities differ by about 1e-6, so the device finds the same
lists), at least two utterances with two or more hypotheses of unequal edit distance, and a largest risk weight above 1e-3.
tests/test_mwer_oracle_model.py asserts all of that on the CPU, so the GPU test is never the first to see a case."""
import functools
from argparse import Namespace

import torch

from rnntransducer_amd.metrics import edit_distance
from tests import beam_sync_restatement as R
from tests.mwer_restatement import risk_and_weights
from tests.test_oracle_networks import CONFIGS

B, T, U, V, N, S = 3, 24, 5, 72, 4, 2
MARGIN = 1e-4
SCALE, BLANK_BIAS = 3.0, 2.0
LSTM1 = CONFIGS["g1_cfg1"]
GRU2 = (dict(input_size=80, hidden_size=128, output_size=128, num_layers=2, rnn_type="gru", dropout=0.0, bidirectional=True), LSTM1[1], 72)
CASES = {"bilstm1": dict(cfg=LSTM1, seed=1), "bigru2": dict(cfg=GRU2, seed=1)}


def args(**kw):
    return Namespace(learning_rate=1e-3, weight_decay=1e-4, warmup_ratio=0.2, final_div_factor=1e4, total_steps=100,
                     move_metrics_to_cpu=False, **kw)


def build_model(cfg, seed, **kw):
    """The RNNTransducer (on the CPU) the GPU test moves to the device: default initialisation under `seed`, then every
    parameter times SCALE (fc twice as much, as tests/beam_sync_cases.py sharpens its models) and BLANK_BIAS on the blank's
    bias.  A freshly initialised model is all but uniform over the vocabulary: every hypothesis would emit max_symbols tokens in
    every frame (or, with any bias on the blank, none at all), all edit distances of an utterance would be equal and the risk
    identically 0.  The sharper model with a favoured blank behaves more like a trained one: hypotheses of different lengths."""
    from rnntransducer_amd import RNNTransducer
    tn, pn, v = cfg
    torch.manual_seed(seed)
    model = RNNTransducer(dict(pn), dict(tn), dict(num_classes=v), args(**kw))
    with torch.no_grad():
        for n, p in model.jointnet.named_parameters():
            p.mul_(2.0 * SCALE if n.startswith("fc.") else SCALE)
        model.jointnet.decoder.embedding.weight[0].zero_()
        model.jointnet.fc.bias[0] += BLANK_BIAS
    return model


def oracle_of(model, cfg):
    """float64 OracleJointNet carrying the model's parameters."""
    from oracle.rnnt_oracle import OracleJointNet
    tn, pn, v = cfg
    oracle = OracleJointNet(dict(tn), dict(pn), v).double()
    oracle.load_state_dict({k[len("jointnet."):]: p.double().cpu() for k, p in model.state_dict().items()})
    return oracle


def make_case_batch(seed):
    from oracle.rnnt_oracle import make_batch
    return make_batch(B, T, U, V, ragged=True, seed=100 + seed)


def references(batch):
    return [batch[5][b, :int(batch[6][b])].tolist() for b in range(batch[5].size(0))]


def oracle_nbest_nll(oracle, batch, hyps):
    """hyps: per utterance a list of token lists (no leading blank).  -> float64 NLL of every hypothesis, flat in (b, n) order,
    with the graph to the oracle's parameters: encoder once, prediction net and materialised joint on the hypothesis rows."""
    from oracle.rnnt_oracle import _RNNTLossFn
    audios, audio_lens, t_lens = batch[0], batch[1], batch[2]
    enc = oracle.encoder(audios.double(), audio_lens)
    rows = [(b, y) for b, hs in enumerate(hyps) for y in hs]
    umax = max(1, max(len(y) for _, y in rows))
    texts = torch.zeros(len(rows), umax + 1, dtype=torch.int64)
    for r, (_, y) in enumerate(rows):
        texts[r, 1:len(y) + 1] = torch.tensor(y, dtype=torch.int64)
    bidx = torch.tensor([b for b, _ in rows])
    dec = oracle.decoder(texts, [len(y) + 1 for _, y in rows])
    return _RNNTLossFn.apply(oracle.joint(enc[bidx], dec), texts[:, 1:].to(torch.int32).contiguous(), t_lens[bidx],
                             torch.tensor([len(y) for _, y in rows], dtype=torch.int32), 0)


def split_rows(flat, hyps):
    out, k = [], 0
    for hs in hyps:
        out.append(list(flat[k:k + len(hs)]))
        k += len(hs)
    return out


@functools.lru_cache(maxsize=None)
def cpu_case(name):
    """-> dict(model, oracle, batch, hyps, margin, nll, W, weights): the restatement's lists for the case's seed, their float64
    NLLs, edit distances and risk weights per utterance."""
    cfg, seed = CASES[name]["cfg"], CASES[name]["seed"]
    model = build_model(cfg, seed)
    oracle = oracle_of(model, cfg)
    batch = make_case_batch(seed)
    res = R.search(oracle, batch[0], batch[1], 0, N, S)
    hyps = [[y[1:] for y, _, _ in r.hyps] for r in res]
    refs = references(batch)
    with torch.no_grad():
        nll = split_rows(oracle_nbest_nll(oracle, batch, hyps).tolist(), hyps)
    W = [[edit_distance(y, refs[b]) for y in hs] for b, hs in enumerate(hyps)]
    weights = [risk_and_weights(nll[b], W[b], [True] * len(W[b]))[1] for b in range(len(hyps))]
    return dict(model=model, oracle=oracle, batch=batch, hyps=hyps, margin=min(min(r.boundary_margin, r.order_margin) for r in res),
                nll=nll, W=W, weights=weights)


def non_vacuous(W, weights):
    """At least two utterances with two or more hypotheses of unequal W, and a largest |weight| above 1e-3."""
    return sum(len(w) >= 2 and len(set(w)) > 1 for w in W) >= 2 and max(abs(x) for ws in weights for x in ws) > 1e-3
