"""Plain CPU restatement of STREAMING beam search, test side: the frame loop of tests/beam_restatement.beam_search_one
(networks/transducer.py:285-358 of the reference with lm=None, hotwords=None) with the hypothesis set B carried between
`feed()` calls.  Written from the semantics, independently of csrc/beam_stream.hip: hypotheses are dicts with their own y_star
list and hidden state, every pop runs a prediction-net step, nothing is memoised, nothing is collected.

    ref = BeamStreamRef(net, n_streams, blank, beam, improved)
    ref.feed(chunk, frames_per_stream)      # any number of times, 0 frames allowed
    ref.nbest(b)                            # [(y_star, score)]: what the offline search returns for the frames fed so far
    ref.stable_prefix(b)                    # longest common prefix of the y_star of ALL carried hypotheses
    ref.reset(rows)

`margin` is the smallest gap over every decision taken so far (as in beam_restatement), the n-best sorts asked for included.
"""
import math

import torch
import torch.nn.functional as F

from tests.beam_restatement import _step


def common_prefix(lists):
    out = list(lists[0])
    for y in lists[1:]:
        n = 0
        while n < min(len(out), len(y)) and out[n] == y[n]:
            n += 1
        out = out[:n]
    return out


class BeamStreamRef:
    def __init__(self, net, B: int, blank: int, beam: int, improved: bool = False, state_beam: float = 4.6,
                 expand_beam: float = 2.3):
        self.net, self.blank, self.beam, self.improved = net, blank, beam, improved
        self.state_beam, self.expand_beam = state_beam, expand_beam
        self.margin = math.inf
        self.pops = 0
        self.enc_state = [None] * B
        self.hyps = [self._start() for _ in range(B)]
        self.frames = [0] * B

    def _start(self):
        return [{"score": 0.0, "y": [self.blank], "state": None}]   # transducer.py:276-284

    def reset(self, rows):
        for b in rows:
            self.enc_state[b], self.hyps[b], self.frames[b] = None, self._start(), 0

    def _gap(self, x, y):
        self.margin = min(self.margin, abs(float(x) - float(y)))

    def _frame(self, enc_t, B_prev):
        """One frame: A = B_prev, B = [] ... -> the new B (all of it: the reference prunes nothing between frames)."""
        A_hyps, B_hyps = B_prev, []
        while A_hyps:
            scores = [h["score"] for h in A_hyps]
            i_best = max(range(len(A_hyps)), key=lambda i: scores[i])   # first of equal maxima
            a_best = scores[i_best]
            if len(scores) > 1:
                self._gap(a_best, max(s for i, s in enumerate(scores) if i != i_best))
            b_best = max(h["score"] for h in B_hyps) if B_hyps else -9999.0
            if self.improved:
                self._gap(b_best, self.state_beam + a_best)
                if b_best >= self.state_beam + a_best:
                    break
            a = A_hyps.pop(i_best)
            self.pops += 1
            d, new_state = _step(self.net.decoder, a["y"][-1], a["state"])
            logp = torch.log_softmax(self.net.fc(F.gelu(torch.cat((enc_t, d)), approximate="tanh")), dim=0)
            thr = torch.max(logp[1:]) - self.expand_beam   # fp32 tensor arithmetic; index 0 skipped whatever the blank is
            for k in range(logp.numel()):
                score = a["score"] + float(logp[k])
                if k == self.blank:
                    B_hyps.append({"score": score, "y": list(a["y"]), "state": a["state"]})
                    continue
                if self.improved:
                    self._gap(logp[k], thr)
                    if not bool(logp[k] >= thr):
                        continue
                same = a["y"][-1] == k
                A_hyps.append({"score": score, "y": a["y"] if same else a["y"] + [k], "state": new_state})
            if not A_hyps:   # the reference's max() would raise here (improved mode); the frame ends
                break
            if len(B_hyps) >= self.beam:
                max_a, max_b = max(h["score"] for h in A_hyps), max(h["score"] for h in B_hyps)
                self._gap(max_b, max_a)
                if max_b > max_a:
                    break
        return B_hyps

    @torch.no_grad()
    def feed(self, chunk: torch.Tensor, ns):
        """chunk (B,T_c,F); stream b consumes its first ns[b] frames."""
        enc = self.net.encoder
        for b, n in enumerate(ns):
            if n == 0:
                continue
            y, self.enc_state[b] = enc.rnn(chunk[b:b + 1, :n], self.enc_state[b])
            rows = enc.out_proj(y[0])
            for t in range(n):
                self.hyps[b] = self._frame(rows[t], self.hyps[b])
            self.frames[b] += n

    def nbest(self, b: int):
        hyps = self.hyps[b]
        keys = [h["score"] / len(h["y"]) for h in hyps]
        order = sorted(range(len(hyps)), key=lambda i: keys[i], reverse=True)   # stable, like the reference's sorted()
        for r in range(min(self.beam, len(order) - 1)):
            self._gap(keys[order[r]], keys[order[r + 1]])
        return [(list(hyps[i]["y"]), hyps[i]["score"]) for i in order[:self.beam]]

    def stable_prefix(self, b: int):
        """Every hypothesis of a later frame extends the y_star of a carried one, so their common prefix is final.  With an
        empty carried set (possible only through the improved early-out at scores below -9999) nothing further is decided."""
        hyps = self.hyps[b]
        return common_prefix([h["y"] for h in hyps]) if hyps else None
