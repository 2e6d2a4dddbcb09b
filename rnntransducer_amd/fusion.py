"""Token-level fusion for the beam searches: hotword boosting and token / grapheme LM tables.

The reference's `recognize_beams(lm=..., hotwords=...)` (networks/transducer.py:147-213, 253-264, 352-361) ranks a hypothesis by
its ASR score plus a score that depends on its decoded y_star alone, computed by pyctcdecode and KenLM over text.  Here that
score is the one of a weighted deterministic automaton over TOKEN IDS, which the search kernel (csrc/beam_shared.hpp, FUSED)
walks on the device: contextual biasing and shallow fusion with a token LM are both such automata.

    fusion = TokenFusion.from_hotwords([[4, 6, 4], [9, 2]], weight=0.5, vocab_size=72, blank=0).to("cuda")
    nbest = jointnet.recognize_beams(audio, lengths, 0, 5, improved=True, fusion=fusion, return_scores=True)
    # [(y_star, asr_score, fused_score), ...]
    state = jointnet.init_beam_stream(B, 0, 5, improved=True, fusion=fusion)

Semantics (include/rnnt_hip.h): state 0 belongs to y_star = [blank]; total(y) = sum of arc[s_{i-1}, y_i] over the tokens after
the leading blank, in fp64, in append order; every comparison of the search uses asr_score + total; `final[state]` is added
once, only where the hypotheses are ranked for output.  The automaton advances only when a token is appended: a blank and a
token equal to y_star[-1] (which the search does not append) leave state and total as they are.

Runaway frames: with positive arcs a frame's pop loop need not end — a hypothesis that keeps completing a boosted phrase can
gain more per token than its log-probability falls (the reference has the same hazard with hotwords).  The search's `max_pops`
cap bounds it: the call raises RnntHipError naming max_pops and the next call succeeds.  Keep hotword weights below the
typical -log p of a token.
"""
from __future__ import annotations

import math
from typing import List, Sequence

import torch

MAX_ENTRIES = 1 << 27   # S * V: the kernel indexes the dense tables with 32-bit arithmetic to spare


class TokenFusion:
    """A weighted deterministic automaton over token ids as dense tables:
      next  (S, V) int32    state after appending token k in state s
      arc   (S, V) float32  score added by that append
      final (S,)   float32  added once when a hypothesis is ranked for output
    State 0 is the start state.  The tables are dense by design: the kernel's threads run along k, so both lookups are
    coalesced, and V = 72 with thousands of states or V = 2048 with hundreds fit.  Validated here, on the host, once."""

    def __init__(self, next: torch.Tensor, arc: torch.Tensor, final: torch.Tensor):
        for name, t, dt in (("next", next, torch.int32), ("arc", arc, torch.float32), ("final", final, torch.float32)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt:
                raise ValueError(f"TokenFusion: {name} must be a {dt} tensor, got "
                                 f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
        if next.dim() != 2 or next.shape[0] < 1 or next.shape[1] < 1:
            raise ValueError(f"TokenFusion: next must be (S, V) with S, V >= 1, got {tuple(next.shape)}")
        S, V = next.shape
        if tuple(arc.shape) != (S, V) or tuple(final.shape) != (S,):
            raise ValueError(f"TokenFusion: next {tuple(next.shape)}, arc {tuple(arc.shape)} and final {tuple(final.shape)} must be "
                             "(S, V), (S, V) and (S,)")
        if S * V > MAX_ENTRIES:
            raise ValueError(f"TokenFusion: S * V = {S * V} exceeds 2^27 entries (the tables are dense; a sparse form is out of scope)")
        if not (next.device == arc.device == final.device):
            raise ValueError("TokenFusion: next, arc and final must live on one device")
        if int(next.min()) < 0 or int(next.max()) >= S:
            raise ValueError(f"TokenFusion: next must lie in [0, {S})")
        if not bool(torch.isfinite(arc).all()) or not bool(torch.isfinite(final).all()):
            raise ValueError("TokenFusion: arc and final must be finite")
        self.next, self.arc, self.final = next.contiguous(), arc.contiguous(), final.contiguous()

    @property
    def n_states(self) -> int:
        return self.next.shape[0]

    @property
    def vocab_size(self) -> int:
        return self.next.shape[1]

    @property
    def device(self) -> torch.device:
        return self.next.device

    def to(self, device) -> "TokenFusion":
        """The same automaton on `device` (self if it is there already).  The values were validated when it was built."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None and torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.device:
            return self
        out = object.__new__(TokenFusion)
        out.next, out.arc, out.final = self.next.to(device), self.arc.to(device), self.final.to(device)
        return out

    def score(self, y_star: Sequence[int]):
        """(total, final, state) of a y_star (leading blank included), as the search computes them: fp64, append order.
        Host-side, for inspection and tests."""
        nxt, arc = self.next.cpu(), self.arc.cpu()
        s, total = 0, 0.0
        for k in list(y_star)[1:]:
            total += float(arc[s, k])
            s = int(nxt[s, k])
        return total, float(self.final[s]), s

    # ------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_hotwords(cls, phrases: Sequence[Sequence[int]], weight: float, vocab_size: int, blank: int) -> "TokenFusion":
        """Contextual biasing: an Aho-Corasick automaton over `phrases` (lists of token ids; the tokenizer is the caller's) with
        the failure links resolved into the dense table.  Every matched token of a phrase in progress earns +weight; falling
        out of a partial match revokes what that match had earned; completing a phrase keeps its bonus and restarts matching at
        the root.  So total(y) = weight * (sum of the lengths of the completed phrases) + weight * depth(state(y)), with
        arc[s, k] = weight * (depth(s') - depth(s)) for the Aho-Corasick goto target s' (next[s, k] = 0 and the arc unreduced
        when s' completes a phrase), and final[s] = -weight * depth(s): a match left unfinished at the end of the utterance
        earns nothing.
        Keep `weight` below the typical -log p of a token: a larger bonus can make a frame's pop loop run away (a hypothesis
        that keeps completing a phrase gains more than it loses), which ends in RnntHipError naming max_pops.
        ValueError: an empty phrase list or phrase; a token outside [0, vocab_size); `blank` inside a phrase; two equal
        adjacent tokens in a phrase (y_star never holds them); a phrase that is a proper prefix of (or equal to) another
        (ambiguous under restart-on-completion); a non-finite or non-positive weight."""
        if not isinstance(vocab_size, int) or vocab_size < 1:
            raise ValueError(f"from_hotwords: vocab_size must be an integer >= 1, got {vocab_size!r}")
        if not isinstance(weight, (int, float)) or not math.isfinite(weight) or weight <= 0:
            raise ValueError(f"from_hotwords: weight must be finite and > 0, got {weight!r}")
        phrases = [[int(k) for k in p] for p in phrases]
        if not phrases:
            raise ValueError("from_hotwords: no phrases")
        for p in phrases:
            if not p:
                raise ValueError("from_hotwords: an empty phrase")
            if any(not 0 <= k < vocab_size for k in p):
                raise ValueError(f"from_hotwords: phrase {p} holds a token outside [0, {vocab_size})")
            if blank in p:
                raise ValueError(f"from_hotwords: phrase {p} holds the blank ({blank})")
            if any(a == b for a, b in zip(p, p[1:])):
                raise ValueError(f"from_hotwords: phrase {p} repeats a token back to back, which y_star never does")
        for i, p in enumerate(phrases):
            for j, q in enumerate(phrases):
                if i != j and len(p) <= len(q) and q[:len(p)] == p:
                    raise ValueError(f"from_hotwords: phrase {p} is a prefix of phrase {q}: ambiguous when matching restarts "
                                     "on completion")
        # trie: node 0 = root; a node that completes a phrase is a leaf (no phrase is a prefix of another) and gets no state
        children: List[dict] = [{}]
        depth, done = [0], [False]
        for p in phrases:
            n = 0
            for k in p:
                if k not in children[n]:
                    children[n][k] = len(children)
                    children.append({})
                    depth.append(depth[n] + 1)
                    done.append(False)
                n = children[n][k]
            done[n] = True
        if (len(children) - sum(done)) * vocab_size > MAX_ENTRIES:
            raise ValueError(f"from_hotwords: {len(children) - sum(done)} states x {vocab_size} tokens exceed 2^27 table entries")
        # goto with failure links resolved, breadth first (a node's failure target is shallower, so its row is complete)
        goto = [[0] * vocab_size for _ in children]
        fail = [0] * len(children)
        order = [0]
        for n in order:
            row = goto[n]
            if n:
                row[:] = goto[fail[n]]
            for k, c in children[n].items():
                fail[c] = goto[fail[n]][k] if n else 0
                row[k] = c
                order.append(c)
        state_of = {n: i for i, n in enumerate(n for n in order if not done[n])}   # root first: state 0
        S = len(state_of)
        nxt = torch.zeros(S, vocab_size, dtype=torch.int32)
        arc = torch.zeros(S, vocab_size, dtype=torch.float32)
        fin = torch.zeros(S, dtype=torch.float32)
        for n, s in state_of.items():
            tgt = goto[n]
            nxt[s] = torch.tensor([0 if done[t] else state_of[t] for t in tgt], dtype=torch.int32)
            arc[s] = torch.tensor([weight * (depth[t] - depth[n]) for t in tgt], dtype=torch.float64).to(torch.float32)
            fin[s] = -weight * depth[n] if depth[n] else 0.0
        return cls(nxt, arc, fin)

    @classmethod
    def from_bigram(cls, logp: torch.Tensor, weight: float, blank: int) -> "TokenFusion":
        """Shallow fusion with a bigram token LM: logp (V, V), logp[prev, k]; one state per last appended token, the start
        context being row `blank` (renumbered to state 0: states 0 and `blank` swap); arc = weight * logp, final = 0."""
        if not isinstance(logp, torch.Tensor) or logp.dim() != 2 or logp.shape[0] != logp.shape[1] or not logp.is_floating_point():
            raise ValueError("from_bigram: logp must be a floating-point (V, V) tensor")
        V = logp.shape[0]
        if not 0 <= blank < V:
            raise ValueError(f"from_bigram: blank {blank} outside [0, {V})")
        if not isinstance(weight, (int, float)) or not math.isfinite(weight):
            raise ValueError(f"from_bigram: weight must be finite, got {weight!r}")
        perm = list(range(V))            # state s holds the context of token perm[s]
        perm[0], perm[blank] = blank, 0
        state_of = torch.tensor(perm, dtype=torch.int32)   # the swap is its own inverse: token k -> state perm[k]
        rows = logp.detach().cpu().to(torch.float64)[torch.tensor(perm)]
        arc = (weight * rows).to(torch.float32)
        nxt = state_of.unsqueeze(0).expand(V, V).contiguous()
        return cls(nxt, arc, torch.zeros(V, dtype=torch.float32))
