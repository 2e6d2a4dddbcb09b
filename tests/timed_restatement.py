"""Plain CPU restatements of recognition WITH token timestamps and confidences, test side (torch CPU over the oracle
networks, float64 when the network is; written from the semantics of include/rnnt_hip.h, independently of the kernels).

Greedy (networks/transducer.py:95-145 of the reference): `GreedyTimedRef` carries the search between `feed()` calls, so one
feed is the offline search and many are the streaming one.  Per stream: tokens, frames (absolute: counted from the stream's
last reset), logp (log_softmax of the joint at the evaluation that chose the token, at that token) and two flags, "a duplicate
was dropped" (a symbol equal to the last appended one advanced the prediction net without an entry) and "some frame used all
max_iters".  `margin` is the smallest top-1 / top-2 logit gap of any evaluation.

Beam (networks/transducer.py:215-361 with lm=None, hotwords=None): `BeamTimedRef`, the frame loop of tests/beam_restatement.py
with the set B carried between feeds as in tests/beam_stream_restatement.py, every hypothesis holding, beside its y_star, the
frame at which each token was appended (-1 for the leading blank).  `margin` as there.

The cases the GPU tests run (tests/test_gpu_timed.py) are defined at the bottom, each computed once per process; the CPU tests
(tests/test_timed_oracle.py) check on them what the GPU tests rely on.
"""
import functools
import math

import torch
import torch.nn.functional as F

from tests.beam_restatement import _step
from tests.test_stream_oracle import make_oracle


def encode_alone(net, audios, lens):
    """Per utterance its own encoder outputs (n_b, Oe), each utterance encoded alone; an empty one gives (0, Oe)."""
    Oe = net.encoder.out_proj.out_features
    return [net.encoder(audios[b:b + 1, :n], [n])[0, :n] if n else audios.new_zeros(0, Oe) for b, n in enumerate(lens)]


class GreedyTimedRef:
    def __init__(self, net, B: int, blank: int, max_iters: int = 3):
        self.net, self.blank, self.max_iters = net, blank, max_iters
        self.margin = math.inf
        self.enc_state = [None] * B
        self.dec = [self._prime() for _ in range(B)]   # (state, d, last)
        self.seen = [0] * B
        self.tokens, self.frames, self.logp = ([[] for _ in range(B)] for _ in range(3))
        self.dropped, self.exhausted = [False] * B, [False] * B

    def _prime(self):
        d, st = _step(self.net.decoder, self.blank, None)
        return st, d, self.blank

    def reset(self, rows):
        for b in rows:
            self.enc_state[b], self.dec[b], self.seen[b] = None, self._prime(), 0
            self.tokens[b], self.frames[b], self.logp[b] = [], [], []
            self.dropped[b], self.exhausted[b] = False, False

    @torch.no_grad()
    def search(self, b: int, rows: torch.Tensor):
        """Stream b consumes encoder outputs rows (n, Oe) -> the (tokens, frames, logp) appended."""
        st, d, last = self.dec[b]
        new = ([], [], [])
        for t in range(rows.size(0)):
            emitted = 0
            for _ in range(self.max_iters):
                z = self.net.fc(F.gelu(torch.cat((rows[t], d)), approximate="tanh"))
                top2 = torch.topk(z, 2).values
                self.margin = min(self.margin, float(top2[0] - top2[1]))
                k = int(z.argmax())
                if k == self.blank:
                    break
                emitted += 1
                if k != last:
                    new[0].append(k)
                    new[1].append(self.seen[b] + t)
                    new[2].append(float(torch.log_softmax(z, dim=0)[k]))
                    last = k
                else:
                    self.dropped[b] = True
                d, st = _step(self.net.decoder, k, st)
            self.exhausted[b] |= emitted == self.max_iters
        self.dec[b] = (st, d, last)
        self.seen[b] += rows.size(0)
        for mine, got in zip((self.tokens[b], self.frames[b], self.logp[b]), new):
            mine += got
        return new

    @torch.no_grad()
    def feed(self, chunk: torch.Tensor, ns):
        """chunk (B,T_c,F), unidirectional encoder with carried state: stream b consumes its first ns[b] frames."""
        enc, out = self.net.encoder, []
        for b, n in enumerate(ns):
            if n == 0:
                out.append(([], [], []))
                continue
            y, self.enc_state[b] = enc.rnn(chunk[b:b + 1, :n], self.enc_state[b])
            out.append(self.search(b, enc.out_proj(y[0])))
        return out


@torch.no_grad()
def greedy_timed(net, audios, lens, blank: int, max_iters: int = 3) -> GreedyTimedRef:
    """The offline search: every utterance's own frames, each utterance encoded alone (any encoder)."""
    ref = GreedyTimedRef(net, len(lens), blank, max_iters)
    for b, rows in enumerate(encode_alone(net, audios, lens)):
        ref.search(b, rows)
    return ref


class BeamTimedRef:
    def __init__(self, net, B: int, blank: int, beam: int, improved: bool = False, state_beam: float = 4.6,
                 expand_beam: float = 2.3):
        self.net, self.blank, self.beam, self.improved = net, blank, beam, improved
        self.state_beam, self.expand_beam = state_beam, expand_beam
        self.margin = math.inf
        self.enc_state = [None] * B
        self.hyps = [self._start() for _ in range(B)]
        self.seen = [0] * B

    def _start(self):
        return [{"score": 0.0, "y": [self.blank], "f": [-1], "state": None}]   # transducer.py:276-284

    def reset(self, rows):
        for b in rows:
            self.enc_state[b], self.hyps[b], self.seen[b] = None, self._start(), 0

    def _gap(self, x, y):
        self.margin = min(self.margin, abs(float(x) - float(y)))

    def _frame(self, enc_t, t_abs: int, B_prev):
        A_hyps, B_hyps = B_prev, []
        while A_hyps:
            scores = [h["score"] for h in A_hyps]
            i_best = max(range(len(A_hyps)), key=lambda i: scores[i])   # first of equal maxima (python's max)
            a_best = scores[i_best]
            if len(scores) > 1:
                self._gap(a_best, max(s for i, s in enumerate(scores) if i != i_best))
            b_best = max(h["score"] for h in B_hyps) if B_hyps else -9999.0
            if self.improved:
                self._gap(b_best, self.state_beam + a_best)
                if b_best >= self.state_beam + a_best:
                    break
            a = A_hyps.pop(i_best)
            d, new_state = _step(self.net.decoder, a["y"][-1], a["state"])
            logp = torch.log_softmax(self.net.fc(F.gelu(torch.cat((enc_t, d)), approximate="tanh")), dim=0)
            thr = torch.max(logp[1:]) - self.expand_beam   # index 0 skipped whatever the blank is (transducer.py:317)
            for k in range(logp.numel()):
                score = a["score"] + float(logp[k])
                if k == self.blank:
                    B_hyps.append({"score": score, "y": list(a["y"]), "f": list(a["f"]), "state": a["state"]})
                    continue
                if self.improved:
                    self._gap(logp[k], thr)
                    if not bool(logp[k] >= thr):
                        continue
                if a["y"][-1] == k:   # the dedupe rule: same y_star, new state, no new entry
                    A_hyps.append({"score": score, "y": a["y"], "f": a["f"], "state": new_state})
                else:                 # token k is appended in this frame
                    A_hyps.append({"score": score, "y": a["y"] + [k], "f": a["f"] + [t_abs], "state": new_state})
            if not A_hyps:   # the reference's max() would raise here (improved mode); the frame ends
                break
            if len(B_hyps) >= self.beam:
                max_a, max_b = max(h["score"] for h in A_hyps), max(h["score"] for h in B_hyps)
                self._gap(max_b, max_a)
                if max_b > max_a:
                    break
        return B_hyps

    @torch.no_grad()
    def search(self, b: int, rows: torch.Tensor):
        for t in range(rows.size(0)):
            self.hyps[b] = self._frame(rows[t], self.seen[b] + t, self.hyps[b])
        self.seen[b] += rows.size(0)

    @torch.no_grad()
    def feed(self, chunk: torch.Tensor, ns):
        enc = self.net.encoder
        for b, n in enumerate(ns):
            if n:
                y, self.enc_state[b] = enc.rnn(chunk[b:b + 1, :n], self.enc_state[b])
                self.search(b, enc.out_proj(y[0]))

    def nbest(self, b: int):
        """[(y_star, frames, score)], best first: stable sort by score / len(y_star), first `beam`."""
        hyps = self.hyps[b]
        keys = [h["score"] / len(h["y"]) for h in hyps]
        order = sorted(range(len(hyps)), key=lambda i: keys[i], reverse=True)
        for r in range(min(self.beam, len(order) - 1)):
            self._gap(keys[order[r]], keys[order[r + 1]])
        return [(list(hyps[i]["y"]), list(hyps[i]["f"]), hyps[i]["score"]) for i in order[:self.beam]]

    def stable_prefix(self, b: int):
        """(tokens, frames) of the longest common prefix of ALL carried hypotheses, as (y_star, frame) pairs: two hypotheses
        share a prefix entry only if the token was appended at the same frame."""
        pairs = [list(zip(h["y"], h["f"])) for h in self.hyps[b]]
        n = 0
        while all(len(p) > n for p in pairs) and all(p[n] == pairs[0][n] for p in pairs):
            n += 1
        return [y for y, _ in pairs[0][:n]], [f for _, f in pairs[0][:n]]


@torch.no_grad()
def beam_timed(net, audios, lens, blank: int, beam: int, improved: bool = False, state_beam: float = 4.6, expand_beam: float = 2.3,
               padded_batch: bool = False) -> BeamTimedRef:
    """The offline search.  padded_batch: the encoder runs on the padded batch as the reference's fixtures were made
    (tests/beam_restatement.beam_search); otherwise every utterance is encoded alone."""
    ref = BeamTimedRef(net, len(lens), blank, beam, improved, state_beam, expand_beam)
    rows = [e[:n] for e, n in zip(net.encoder(audios, list(lens)), lens)] if padded_batch else encode_alone(net, audios, lens)
    for b, r in enumerate(rows):
        ref.search(b, r)
    return ref


# ---- the cases of tests/test_gpu_timed.py ----------------------------------------------------------------------------
def utterances(B, T, Fdim, lens, seed):
    x = torch.randn(B, T, Fdim, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(lens):
        x[b, n:] = 0
    return x


# name -> (encoder cell, prediction-net cell, H (both nets), layers (both nets), V, lens, max_iters, model seed, blank bias,
# scale of the prediction-net half of fc).  A random model emits the same symbol over and over; a bias towards blank and a joint
# that listens to the prediction net make it emit and fall back to blank, as a trained recogniser does, so that utterances
# without a dropped duplicate and without an exhausted frame exist (tests/test_timed_oracle.py checks how many).
GREEDY_CASES = {
    "lstm_h32_l1": ("lstm", "lstm", 32, 1, 72, [40, 23, 0, 11], 3, 24, 2.0, 4.0),
    "gru_h64_l2": ("gru", "gru", 64, 2, 72, [37, 40, 5, 0], 2, 12, 4.0, 3.0),
    "gru_lstm_h32_l2": ("gru", "lstm", 32, 2, 72, [19, 0, 40, 28], 3, 23, 6.0, 4.0),
    "lstm_gru_h64_l1_v1100": ("lstm", "gru", 64, 1, 1100, [24, 9, 0, 16], 3, 20, 4.0, 2.0),   # V > 1024 threads, V % 64 != 0
}
F_IN, O_ENC = 16, 24


@functools.lru_cache(maxsize=None)
def greedy_case(name: str):
    """-> (oracle float64, transnet params, prednet params, audios float64 (B,T,F), lens, max_iters, GreedyTimedRef offline)."""
    enc_cell, dec_cell, H, L, V, lens, max_iters, seed, bias, dec_scale = GREEDY_CASES[name]
    ora, tn, pn = make_oracle(enc_cell=enc_cell, enc_layers=L, H=H, dec_cell=dec_cell, dec_layers=L, Hp=H, V=V, F_in=F_IN, O=O_ENC,
                              seed=seed)
    with torch.no_grad():
        ora.fc.bias[0] += bias
        ora.fc.weight[:, O_ENC:] *= dec_scale
    audios = utterances(len(lens), max(lens), F_IN, lens, 100 + seed)
    return ora, tn, pn, audios, lens, max_iters, greedy_timed(ora, audios, lens, 0, max_iters)


def qualifies(ref: GreedyTimedRef, b: int) -> bool:
    """Utterance b can be checked against the dense joint: the prediction net consumed exactly [blank] + tokens."""
    return bool(ref.tokens[b]) and not ref.dropped[b] and not ref.exhausted[b]


# name -> (encoder cell, prediction-net cell, H, layers, beam, improved, lens, model seed); V = 12.  Seeds whose every decision,
# after every frame, has a margin >= 1e-4 (tests/test_timed_oracle.py checks it): fp32 summation order cannot flip one.
BEAM_CASES = {
    "lstm_h32_l1_b5_improved": ("lstm", "lstm", 32, 1, 5, True, [12, 7, 3], 9),
    "gru_h64_l2_b2_improved": ("gru", "gru", 64, 2, 2, True, [11, 12, 4], 1),
    "gru_lstm_h32_l2_b2_plain": ("gru", "lstm", 32, 2, 2, False, [5, 3, 1], 3),
    "lstm_gru_h64_l1_b5_plain": ("lstm", "gru", 64, 1, 5, False, [4, 5, 2], 2),
}
BEAM_V = 12


@functools.lru_cache(maxsize=None)
def beam_model(name: str):
    enc_cell, dec_cell, H, L, beam, improved, lens, seed = BEAM_CASES[name]
    ora, tn, pn = make_oracle(enc_cell=enc_cell, enc_layers=L, H=H, dec_cell=dec_cell, dec_layers=L, Hp=H, V=BEAM_V, F_in=F_IN,
                              O=O_ENC, seed=seed)
    return ora, tn, pn, utterances(len(lens), max(lens), F_IN, lens, 200 + seed), lens, beam, improved


@functools.lru_cache(maxsize=None)
def beam_case(name: str):
    """-> beam_model(name) + (BeamTimedRef offline,)."""
    ora, tn, pn, audios, lens, beam, improved = beam_model(name)
    return ora, tn, pn, audios, lens, beam, improved, beam_timed(ora, audios, lens, 0, beam, improved)
