"""Float64 restatement of streaming greedy recognition (CPU, no GPU needed): torch.nn.LSTM / GRU / RNN fed chunk by chunk with
the state carried, and the greedy loop of networks/transducer.py:95-145 with its prediction-net state, joint half and last
token carried between chunks.  Pinned here against oracle.rnnt_oracle.OracleJointNet run offline on whole utterances; the GPU
tests (tests/test_gpu_stream.py) use it as their yardstick."""
import random

import pytest
import torch
import torch.nn.functional as F


def random_schedules(lens, seed: int, max_chunk: int = 9):
    """Per-stream chunkings that include 0-frame chunks: a list of (T_c, [n_b]) with sum_k n_b == lens[b]."""
    rng = random.Random(seed)
    left, out = list(lens), []
    while any(left):
        Tc = rng.randint(1, max_chunk)
        ns = [0 if rng.random() < 0.25 else min(left[b], rng.randint(0, Tc)) for b in range(len(lens))]
        out.append((Tc, ns))
        left = [l - n for l, n in zip(left, ns)]
    return out


def chunk_batches(audios: torch.Tensor, lens, schedule):
    """(B,T,F) utterances + a schedule [(T_c, [n_b])] -> [(chunk (B,T_c,F), [n_b])]: stream b's next n_b frames, zero padding."""
    B, _, Fdim = audios.shape
    pos, out = [0] * B, []
    for Tc, ns in schedule:
        x = torch.zeros(B, Tc, Fdim, dtype=audios.dtype)
        for b, n in enumerate(ns):
            x[b, :n] = audios[b, pos[b]:pos[b] + n]
            pos[b] += n
        out.append((x, list(ns)))
    assert pos == [int(n) for n in lens]
    return out


def uniform_schedule(lens, chunk: int):
    """Every stream fed `chunk` frames at a time (the last chunk of a stream shorter, later ones 0)."""
    T = max(lens)
    return [(min(chunk, T - t0), [max(0, min(chunk, n - t0)) for n in lens]) for t0 in range(0, T, chunk)]


class StreamRef:
    """The restatement.  `net` is an OracleJointNet (any dtype); the encoder must be unidirectional."""

    def __init__(self, net, B: int, blank: int, max_iters: int = 3):
        self.net, self.blank, self.max_iters = net, blank, max_iters
        self.enc_state = [None] * B
        self.dec = [self._prime() for _ in range(B)]   # (state, d, last)
        self.tokens = [[] for _ in range(B)]

    def _prime(self):
        dn = self.net.decoder
        y, st = dn.rnn(dn.embedding(torch.tensor([[self.blank]])), None)
        return st, dn.out_proj(y).view(-1), self.blank

    def reset(self, rows):
        for b in rows:
            self.enc_state[b], self.dec[b], self.tokens[b] = None, self._prime(), []

    def encode(self, chunk: torch.Tensor, ns):
        """-> (B,T_c,O) encoder outputs, zeros past n_b; carries the encoder states."""
        enc = self.net.encoder
        out = torch.zeros(chunk.size(0), chunk.size(1), enc.out_proj.out_features, dtype=chunk.dtype)
        for b, n in enumerate(ns):
            if n:
                y, self.enc_state[b] = enc.rnn(chunk[b:b + 1, :n], self.enc_state[b])
                out[b, :n] = enc.out_proj(y[0])
        return out

    def feed(self, chunk: torch.Tensor, ns):
        """One chunk of recognize_greedy_stream -> (tokens appended per stream, smallest top-1/top-2 logit gap seen)."""
        enc = self.encode(chunk, ns)
        dn, new, margin = self.net.decoder, [], float("inf")
        for b, n in enumerate(ns):
            st, d, last = self.dec[b]
            got = []
            for t in range(n):
                for _ in range(self.max_iters):
                    z = self.net.fc(F.gelu(torch.cat((enc[b, t], d)), approximate="tanh"))
                    top2 = torch.topk(z, 2).values
                    margin = min(margin, float(top2[0] - top2[1]))
                    k = int(z.argmax())
                    if k == self.blank:
                        break
                    if k != last:
                        got.append(k)
                        last = k
                    y, st = dn.rnn(dn.embedding(torch.tensor([[k]])), st)
                    d = dn.out_proj(y).view(-1)
            self.dec[b] = (st, d, last)
            self.tokens[b] += got
            new.append(got)
        return new, margin


def make_oracle(enc_cell="lstm", enc_layers=2, H=48, dec_cell="lstm", dec_layers=1, Hp=40, V=12, F_in=16, O=24, seed=3,
                scale=3.0, fc_scale=6.0, dtype=torch.float64):
    """A unidirectional OracleJointNet with weights scaled so that greedy search emits real tokens (as the decode tests do)."""
    from oracle.rnnt_oracle import OracleJointNet
    tn = dict(input_size=F_in, hidden_size=H, output_size=O, num_layers=enc_layers, rnn_type=enc_cell, dropout=0.0,
              bidirectional=False)
    pn = dict(embedding_size=V, pad_token_id=0, hidden_size=Hp, output_size=O, num_layers=dec_layers, rnn_type=dec_cell,
              dropout=0.0)
    torch.manual_seed(seed)
    ora = OracleJointNet(tn, pn, V).eval()
    with torch.no_grad():
        for n, p in ora.named_parameters():
            p.mul_(fc_scale if n.startswith("fc.") else scale)
        ora.decoder.embedding.weight[0].zero_()
    return ora.to(dtype), tn, pn


@pytest.mark.parametrize("cells", [("lstm", "lstm"), ("gru", "lstm"), ("rnn", "gru")])
def test_streaming_restatement_equals_offline_oracle(cells):
    ora, _, _ = make_oracle(enc_cell=cells[0], dec_cell=cells[1])
    lens = [30, 17, 1, 24]
    audios = torch.randn(4, 30, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    for b, n in enumerate(lens):
        audios[b, n:] = 0
    with torch.no_grad():
        want_enc = ora.encoder(audios, lens)
        want_tok, margin = ora.recognize_greedy(audios, lens, 0, 3, return_margin=True)
        assert sum(map(len, want_tok)) > 10 and margin > 1e-6
        for sched in (uniform_schedule(lens, 30), uniform_schedule(lens, 1), uniform_schedule(lens, 7), random_schedules(lens, 4)):
            ref = StreamRef(ora, 4, 0)
            encs = [[] for _ in lens]
            for x, ns in chunk_batches(audios, lens, sched):
                ref.feed(x, ns)
            assert ref.tokens == want_tok
            # encoder outputs on their own, with the same chunking
            ref2 = StreamRef(ora, 4, 0)
            for x, ns in chunk_batches(audios, lens, sched):
                y = ref2.encode(x, ns)
                for b, n in enumerate(ns):
                    encs[b].append(y[b, :n])
            for b, n in enumerate(lens):
                got = torch.cat(encs[b])
                assert got.shape[0] == n
                torch.testing.assert_close(got, want_enc[b, :n], rtol=0, atol=1e-12)


def test_restatement_reset_starts_a_fresh_utterance():
    ora, _, _ = make_oracle()
    g = torch.Generator().manual_seed(2)
    first, second = torch.randn(2, 12, 16, dtype=torch.float64, generator=g), torch.randn(2, 20, 16, dtype=torch.float64, generator=g)
    with torch.no_grad():
        ref = StreamRef(ora, 2, 0)
        ref.feed(first, [12, 12])
        ref.reset([1])
        ref.feed(second, [20, 20])
        fresh = StreamRef(ora, 2, 0)
        fresh.feed(second, [20, 20])
        cont = StreamRef(ora, 2, 0)
        cont.feed(first, [12, 12])
        cont.feed(second, [20, 20])
    assert ref.tokens[1] == fresh.tokens[1]
    assert ref.tokens[0] == cont.tokens[0]
