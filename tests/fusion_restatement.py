"""Plain CPU restatement of beam search with token-level fusion, test side: the reference's search (networks/transducer.py:
215-361) on its compare_key = "lm_score" branch, with the score that depends on y_star alone given by a weighted deterministic
automaton over token ids (rnntransducer_amd/fusion.py) instead of pyctcdecode / KenLM over text.

Written from the semantics of include/rnnt_hip.h, independently of csrc/beam_shared.hpp: hypotheses are dicts holding their own
y_star list, hidden state, automaton state and fusion total; every pop runs a prediction-net step; A and B are python lists.
  * total(y) = sum of arc[s_{i-1}][y_i] over the tokens after the leading blank, python floats (fp64), in append order;
  * the automaton advances only when a token is appended (a blank child and a child whose token equals y_star[-1] copy both);
  * every comparison uses key = score + total: the pop argmax, the best of B, the improved early-out, the stop test;
  * the n-best is the stable sort by (score + total + final[state]) / len(y_star); `final` is never stored back;
  * the prune test stays on the fp32 ASR log-probabilities.
`margin` is the smallest gap over every decision taken, as in tests/beam_restatement.py.  One frame function serves the
offline search and the streaming reference (the carried set B between `feed()` calls), as the kernel template does.
"""
import math

import torch
import torch.nn.functional as F

from tests.beam_restatement import _step
from tests.beam_stream_restatement import common_prefix


class Tables:
    """The automaton as python lists (exact: float32 -> python float)."""

    def __init__(self, fusion):
        self.next = fusion.next.cpu().tolist()
        self.arc = fusion.arc.cpu().tolist()
        self.final = fusion.final.cpu().tolist()


def start_hyp(blank):
    return {"score": 0.0, "y": [blank], "state": None, "fstate": 0, "total": 0.0}   # state 0 belongs to [blank]


def key(h):
    return h["score"] + h["total"]


def frame(net, enc_t, B_prev, tab, blank, beam, improved, state_beam, expand_beam, gap, stats):
    """One frame: A = B_prev, B = [] ... -> the new B (all of it)."""
    A_hyps, B_hyps = B_prev, []
    pops = 0
    while A_hyps:
        keys = [key(h) for h in A_hyps]
        i_best = max(range(len(A_hyps)), key=lambda i: keys[i])   # first of equal maxima (python's max)
        a_best = keys[i_best]
        if len(keys) > 1:
            gap(a_best, max(s for i, s in enumerate(keys) if i != i_best))
        b_best = max(key(h) for h in B_hyps) if B_hyps else -9999.0
        if improved:
            gap(b_best, state_beam + a_best)
            if b_best >= state_beam + a_best:
                break
        a = A_hyps.pop(i_best)
        pops += 1
        stats["pops"] += 1
        d, new_state = _step(net.decoder, a["y"][-1], a["state"])
        logp = torch.log_softmax(net.fc(F.gelu(torch.cat((enc_t, d)), approximate="tanh")), dim=0)
        thr = torch.max(logp[1:]) - expand_beam   # fp32 tensor arithmetic; index 0 skipped whatever the blank is
        for k in range(logp.numel()):
            score = a["score"] + float(logp[k])
            if k == blank:   # appends nothing: automaton state and total as popped
                B_hyps.append({"score": score, "y": list(a["y"]), "state": a["state"], "fstate": a["fstate"], "total": a["total"]})
                continue
            if improved:
                gap(logp[k], thr)
                if not bool(logp[k] >= thr):
                    continue
            if a["y"][-1] == k:   # the dedupe rule: not appended, so the automaton does not move
                A_hyps.append({"score": score, "y": a["y"], "state": new_state, "fstate": a["fstate"], "total": a["total"]})
            else:
                A_hyps.append({"score": score, "y": a["y"] + [k], "state": new_state, "fstate": tab.next[a["fstate"]][k],
                               "total": a["total"] + tab.arc[a["fstate"]][k]})
        if not A_hyps:   # the reference's max() would raise here (improved mode); the frame ends
            break
        if len(B_hyps) >= beam:
            max_a, max_b = max(key(h) for h in A_hyps), max(key(h) for h in B_hyps)
            gap(max_b, max_a)
            if max_b > max_a:
                break
        if pops > stats.get("max_pops", 1 << 30):
            raise RuntimeError("runaway frame")
    stats["max_pops_frame"] = max(stats["max_pops_frame"], pops)
    return B_hyps


def nbest_of(B_hyps, tab, beam, gap):
    """[(y_star, asr_score, fused_score)], best first."""
    fused = [h["score"] + h["total"] + tab.final[h["fstate"]] for h in B_hyps]
    keys = [f / len(h["y"]) for f, h in zip(fused, B_hyps)]
    order = sorted(range(len(B_hyps)), key=lambda i: keys[i], reverse=True)   # stable, like the reference's sorted()
    for r in range(min(beam, len(order) - 1)):
        gap(keys[order[r]], keys[order[r + 1]])
    return [(list(B_hyps[i]["y"]), B_hyps[i]["score"], fused[i]) for i in order[:beam]]


class _Margin:
    def __init__(self):
        self.value = math.inf

    def __call__(self, x, y):
        self.value = min(self.value, abs(float(x) - float(y)))


def fused_beam_search_one(net, enc_rows, fusion, blank, beam, improved=False, state_beam=4.6, expand_beam=2.3, max_pops=None):
    """enc_rows (T, Oe): one utterance's encoder outputs -> (nbest [(y_star, asr_score, fused_score)], margin, stats).
    max_pops: raise RuntimeError when a frame pops more (a runaway frame), instead of looping."""
    tab, gap = Tables(fusion), _Margin()
    stats = {"pops": 0, "max_pops_frame": 0}
    if max_pops is not None:
        stats["max_pops"] = max_pops
    B_hyps = [start_hyp(blank)]
    for t in range(enc_rows.size(0)):
        B_hyps = frame(net, enc_rows[t], B_hyps, tab, blank, beam, improved, state_beam, expand_beam, gap, stats)
    return nbest_of(B_hyps, tab, beam, gap), gap.value, stats


@torch.no_grad()
def fused_beam_search(net, audios, lens, fusion, blank, beam, improved=False, state_beam=4.6, expand_beam=2.3, max_pops=None):
    """Batched front: encoder on the padded batch, then every utterance on its own frames.  -> (per-utterance nbest lists,
    min margin, per-utterance margins, per-utterance stats)."""
    enc = net.encoder(audios, list(lens))
    outs, margins, stats = [], [], []
    for b in range(enc.size(0)):
        nb, m, st = fused_beam_search_one(net, enc[b, :int(lens[b])], fusion, blank, beam, improved, state_beam, expand_beam, max_pops)
        outs.append(nb)
        margins.append(m)
        stats.append(st)
    return outs, min(margins), margins, stats


class FusedBeamStreamRef:
    """Streaming: the same frame function with B carried between `feed()` calls (tests/beam_stream_restatement.BeamStreamRef
    with the fusion fields).  One margin per stream, the n-best sorts asked for included."""

    def __init__(self, net, B, fusion, blank, beam, improved=False, state_beam=4.6, expand_beam=2.3, only=None):
        self.only = None if only is None else set(only)   # restate these streams alone (the others' frames are skipped)
        self.net, self.tab, self.blank, self.beam, self.improved = net, Tables(fusion), blank, beam, improved
        self.state_beam, self.expand_beam = state_beam, expand_beam
        self.gaps = [_Margin() for _ in range(B)]
        self.stats = {"pops": 0, "max_pops_frame": 0}
        self.enc_state = [None] * B
        self.hyps = [[start_hyp(blank)] for _ in range(B)]

    def reset(self, rows):
        for b in rows:
            self.enc_state[b], self.hyps[b] = None, [start_hyp(self.blank)]

    def margin(self, b=None):
        return self.gaps[b].value if b is not None else min(g.value for g in self.gaps)

    @torch.no_grad()
    def feed(self, chunk, ns):
        enc = self.net.encoder
        for b, n in enumerate(ns):
            if n == 0 or (self.only is not None and b not in self.only):
                continue
            y, self.enc_state[b] = enc.rnn(chunk[b:b + 1, :n], self.enc_state[b])
            rows = enc.out_proj(y[0])
            for t in range(n):
                self.hyps[b] = frame(self.net, rows[t], self.hyps[b], self.tab, self.blank, self.beam, self.improved,
                                     self.state_beam, self.expand_beam, self.gaps[b], self.stats)

    def nbest(self, b):
        return nbest_of(self.hyps[b], self.tab, self.beam, self.gaps[b])

    def stable_prefix(self, b):
        hyps = self.hyps[b]
        return common_prefix([h["y"] for h in hyps]) if hyps else None
