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

Backoff n-gram models (the kind the reference decodes with: an ARPA file) do not fit dense tables: `NgramFusion` holds one in
sparse form and the searches whose cost per frame is bounded walk it on the device (csrc/search_shared.hpp, ngram_lookup):

    lm = NgramFusion.from_arpa("lm.arpa", symbols, weight=0.3, blank=0).to("cuda")      # symbols[i]: the ARPA word of token i
    nbest = jointnet.recognize_beams_sync(audio, lengths, 0, 16, fusion=lm, return_scores=True)
    nbest = jointnet.recognize_ctc_beams(audio, lengths, 0, 16, fusion=lm, return_scores=True)
    state = jointnet.init_beam_sync_stream(B, 0, 16, fusion=lm)
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
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
            raise ValueError(f"TokenFusion: S * V = {S * V} exceeds 2^27 entries (the tables are dense; NgramFusion is the sparse "
                             "form for backoff n-gram models)")
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


MAX_ORDER = 8   # the device walks at most this many backoff levels per lookup


class NgramFusion:
    """A backoff n-gram model over token ids as a weighted deterministic automaton in sparse (CSR) form: one state per context
    (history of at most order - 1 tokens), whose row lists only the tokens the model lists after that context; every other
    token backs off to the context without its oldest token.
      row_ptr (S+1) int32    arcs of state s are [row_ptr[s], row_ptr[s+1])
      tok     (E)   int32    token ids, strictly ascending inside a state
      arc     (E)   float32  weight * ln p(token | the state's context)
      next    (E)   int32    state after the append
      bow     (S)   float32  weight * ln backoff(context)
      backoff (S)   int32    state of the context without its oldest token; the root backs off to itself
      final   (S)   float32  weight * ln p(</s> | context), backoff resolved here; 0 when the model has no </s>
    State 0 is the start state (the context [<s>] when the model has one, else the empty context).  `root` is the empty
    context: its row lists every token 0..V-1, so a lookup always ends.

    Lookup of token k in state s, the same on the host (`score`, `to_dense`) and on the device (csrc/search_shared.hpp):
        acc = 0.0 (fp64); h = s
        repeat at most `order` times:
            if k is listed in h at e:  return (float)(acc + (double)arc[e]), next[e]
            if h == root: break
            acc += (double)bow[h];  h = backoff[h]
    The value is rounded to float32, so a dense TokenFusion (`to_dense`) can hold the very same automaton: a search returns
    the same bits with either.  The searches whose cost per frame is bounded take it as fusion=: recognize_beams_sync, its
    streaming form and recognize_ctc_beams.  Validated here, on the host, once."""

    BOS, EOS = -1, -2   # sentinel ids of <s> and </s> in from_ngrams' tuples

    def __init__(self, row_ptr: torch.Tensor, tok: torch.Tensor, arc: torch.Tensor, next: torch.Tensor, bow: torch.Tensor,
                 backoff: torch.Tensor, final: torch.Tensor, root: int, order: int, vocab_size: int):
        i32, f32 = torch.int32, torch.float32
        tabs = (("row_ptr", row_ptr, i32), ("tok", tok, i32), ("arc", arc, f32), ("next", next, i32), ("bow", bow, f32),
                ("backoff", backoff, i32), ("final", final, f32))
        for name, t, dt in tabs:
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1:
                raise ValueError(f"NgramFusion: {name} must be a 1-D {dt} tensor, got "
                                 f"{(tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__}")
        if len({t.device for _, t, _ in tabs}) != 1:
            raise ValueError("NgramFusion: the tables must live on one device")
        for name, v in (("root", root), ("order", order), ("vocab_size", vocab_size)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"NgramFusion: {name} must be an integer, got {v!r}")
        S, E, V = bow.numel(), tok.numel(), vocab_size
        if S < 1 or V < 1 or row_ptr.numel() != S + 1 or backoff.numel() != S or final.numel() != S:
            raise ValueError(f"NgramFusion: row_ptr {tuple(row_ptr.shape)}, bow {tuple(bow.shape)}, backoff {tuple(backoff.shape)} and "
                             f"final {tuple(final.shape)} must be (S+1), (S), (S), (S) with S >= 1, and vocab_size >= 1")
        if arc.numel() != E or next.numel() != E or E >= 1 << 31 or S >= 1 << 31:
            raise ValueError(f"NgramFusion: tok {tuple(tok.shape)}, arc {tuple(arc.shape)} and next {tuple(next.shape)} must be (E) "
                             "with E < 2^31")
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"NgramFusion: order {order} outside [1, {MAX_ORDER}]")
        if not 0 <= root < S:
            raise ValueError(f"NgramFusion: root {root} outside [0, {S})")
        rp = row_ptr.to(torch.int64)
        if int(rp[0]) != 0 or int(rp[-1]) != E or bool((rp[1:] < rp[:-1]).any()):
            raise ValueError("NgramFusion: row_ptr must rise from 0 to the number of arcs")
        if E and (int(tok.min()) < 0 or int(tok.max()) >= V):
            raise ValueError(f"NgramFusion: tok must lie in [0, {V})")
        if E > 1:   # strictly ascending inside a state: every step down is a row's start
            down = torch.nonzero(tok[1:] <= tok[:-1]).reshape(-1) + 1
            starts = torch.zeros(E + 1, dtype=torch.bool, device=tok.device)
            starts[rp[:-1]] = True
            if not bool(starts[down].all()):
                raise ValueError("NgramFusion: the tokens of a state must be strictly ascending")
        lo, hi = int(rp[root]), int(rp[root + 1])
        if hi - lo != V or not bool((tok[lo:hi] == torch.arange(V, dtype=i32, device=tok.device)).all()):
            raise ValueError(f"NgramFusion: the root's row must list every token 0..{V - 1}")
        if E and (int(next.min()) < 0 or int(next.max()) >= S):
            raise ValueError(f"NgramFusion: next must lie in [0, {S})")
        if int(backoff.min()) < 0 or int(backoff.max()) >= S or int(backoff[root]) != root:
            raise ValueError(f"NgramFusion: backoff must lie in [0, {S}) and the root must back off to itself")
        bk, h = backoff.to(torch.int64), torch.arange(S, device=backoff.device)
        for _ in range(order - 1):
            h = bk[h]
        if not bool((h == root).all()):
            raise ValueError(f"NgramFusion: a backoff chain does not reach the root in order - 1 = {order - 1} steps")
        if not all(bool(torch.isfinite(t).all()) for t in (arc, bow, final)):
            raise ValueError("NgramFusion: arc, bow and final must be finite")
        self.row_ptr, self.tok, self.arc, self.next = row_ptr.contiguous(), tok.contiguous(), arc.contiguous(), next.contiguous()
        self.bow, self.backoff, self.final = bow.contiguous(), backoff.contiguous(), final.contiguous()
        self.root, self.order, self._V = root, order, V
        self._host = None

    _TABLES = ("row_ptr", "tok", "arc", "next", "bow", "backoff", "final")

    @property
    def n_states(self) -> int:
        return self.bow.numel()

    @property
    def n_arcs(self) -> int:
        return self.tok.numel()

    @property
    def vocab_size(self) -> int:
        return self._V

    @property
    def device(self) -> torch.device:
        return self.tok.device

    def to(self, device) -> "NgramFusion":
        """The same automaton on `device` (self if it is there already).  The values were validated when it was built."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None and torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.device:
            return self
        out = object.__new__(NgramFusion)
        for name in self._TABLES:
            setattr(out, name, getattr(self, name).to(device))
        out.root, out.order, out._V, out._host = self.root, self.order, self._V, self._host
        return out

    def _tables(self):
        """The tables as numpy arrays on the host (copied once)."""
        if self._host is None:
            self._host = tuple(getattr(self, name).cpu().numpy() for name in self._TABLES)
        return self._host

    def lookup(self, s: int, k: int) -> Tuple[float, int]:
        """(arc', next) of appending token k in state s: the definition in the class docstring, on the host."""
        row_ptr, tok, arc, nxt, bow, backoff, _ = self._tables()
        acc, h = 0.0, s
        for _ in range(self.order):
            lo, hi = int(row_ptr[h]), int(row_ptr[h + 1])
            e = lo + int(np.searchsorted(tok[lo:hi], k))
            if e < hi and int(tok[e]) == k:
                return float(np.float32(acc + float(arc[e]))), int(nxt[e])
            if h == self.root:
                break
            acc += float(bow[h])
            h = int(backoff[h])
        return float(np.float32(acc)), self.root

    def score(self, y_star: Sequence[int]):
        """(total, final, state) of a y_star (leading blank included), as the search computes them: fp64, append order, each
        append's value by the lookup above.  Host-side, for inspection and tests."""
        s, total = 0, 0.0
        for k in list(y_star)[1:]:
            if not 0 <= int(k) < self._V:
                raise ValueError(f"NgramFusion.score: token {k} outside [0, {self._V})")
            a, s = self.lookup(s, int(k))
            total += a
        return total, float(self._tables()[6][s]), s

    def to_dense(self) -> TokenFusion:
        """The same automaton as dense tables: arc[s, k] and next[s, k] are the lookup's float32 and state for every (s, k).
        TokenFusion's ValueError when S * V exceeds its 2^27 entries."""
        S, V = self.n_states, self._V
        if S * V > MAX_ENTRIES:
            raise ValueError(f"TokenFusion: S * V = {S * V} exceeds 2^27 entries (the tables are dense; NgramFusion is the sparse "
                             "form for backoff n-gram models)")
        row_ptr, tok, arc, nxt, bow, backoff, final = self._tables()
        d_arc, d_next = np.empty((S, V), dtype=np.float32), np.empty((S, V), dtype=np.int32)
        for s in range(S):
            chain, accs, acc, h = [], [], 0.0, s
            for _ in range(self.order):          # the levels of the walk and the backoff accumulated when each is reached
                chain.append(h)
                accs.append(acc)
                if h == self.root:
                    break
                acc += float(bow[h])
                h = int(backoff[h])
            for h, acc in zip(reversed(chain), reversed(accs)):   # the root's full row first; a higher level overwrites its tokens
                lo, hi = int(row_ptr[h]), int(row_ptr[h + 1])
                d_arc[s, tok[lo:hi]] = (acc + arc[lo:hi].astype(np.float64)).astype(np.float32)
                d_next[s, tok[lo:hi]] = nxt[lo:hi]
        return TokenFusion(torch.from_numpy(d_next), torch.from_numpy(d_arc), torch.from_numpy(final.copy()))

    # ------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_ngrams(cls, ngrams: Dict[Tuple[int, ...], Tuple[float, Optional[float]]], vocab_size: int, weight: float, blank: int,
                    *, oov_logp: Optional[float] = None) -> "NgramFusion":
        """From a mapping of token-id tuples to (ln p, ln backoff) (natural logarithms; a backoff of None is 0).  A tuple
        (w_1 .. w_n) gives p(w_n | w_1 .. w_{n-1}); NgramFusion.BOS may stand first (<s>; the unigram (BOS,) carries only its
        backoff) and NgramFusion.EOS last (</s>: it is no arc, it makes `final`).  The order is the longest tuple's length.
        States: the empty context (the root), and every listed tuple shorter than the order that does not end in EOS; state 0 is
        (BOS,) when that unigram is listed, else the root.  The arc (h, k) leads to the longest suffix of h + (k,) that is a
        state.  The root lists every token: one without a unigram, the blank included, gets oov_logp there.
        ValueError: no n-grams; a token outside [0, vocab_size) that is no sentinel; the blank in a tuple; BOS past the first
        position or predicted by a longer tuple's context only; EOS before the last position; an EOS tuple without the unigram
        (EOS,); a tuple whose context (all but its last token) is not listed; a non-finite number; an order above 8; tokens
        without a unigram and no oov_logp."""
        if isinstance(vocab_size, bool) or not isinstance(vocab_size, int) or vocab_size < 1:
            raise ValueError(f"from_ngrams: vocab_size must be an integer >= 1, got {vocab_size!r}")
        if not isinstance(weight, (int, float)) or not math.isfinite(weight):
            raise ValueError(f"from_ngrams: weight must be finite, got {weight!r}")
        if oov_logp is not None and (not isinstance(oov_logp, (int, float)) or not math.isfinite(oov_logp)):
            raise ValueError(f"from_ngrams: oov_logp must be finite, got {oov_logp!r}")
        if not ngrams:
            raise ValueError("from_ngrams: no n-grams")
        V, BOS, EOS = vocab_size, cls.BOS, cls.EOS
        listed: Dict[Tuple[int, ...], Tuple[float, float]] = {}
        for g, val in ngrams.items():
            g = tuple(int(k) for k in g)
            p, b = (val[0], val[1]) if isinstance(val, (tuple, list)) else (val, None)
            p, b = float(p), 0.0 if b is None else float(b)
            if not g:
                raise ValueError("from_ngrams: an empty n-gram")
            if not math.isfinite(p) or not math.isfinite(b):
                raise ValueError(f"from_ngrams: n-gram {g} has a non-finite number ({p}, {b})")
            if any(not (0 <= k < V or k in (BOS, EOS)) for k in g):
                raise ValueError(f"from_ngrams: n-gram {g} holds a token outside [0, {V})")
            if blank in g:
                raise ValueError(f"from_ngrams: n-gram {g} holds the blank ({blank})")
            if BOS in g[1:] or EOS in g[:-1]:
                raise ValueError(f"from_ngrams: n-gram {g} has <s> past its first position or </s> before its last")
            listed[g] = (p, b)
        order = max(len(g) for g in listed)
        if (BOS,) in listed:
            order = max(order, 2)   # the start state is a one-token context
        if order > MAX_ORDER:
            raise ValueError(f"from_ngrams: order {order} exceeds {MAX_ORDER}")
        for g in listed:
            if len(g) > 1 and g[:-1] not in listed:
                raise ValueError(f"from_ngrams: n-gram {g} is listed but its context {g[:-1]} is not")
        has_eos = (EOS,) in listed
        if not has_eos and any(g[-1] == EOS for g in listed):
            raise ValueError("from_ngrams: an n-gram ends in </s> but the unigram of </s> is not listed")
        # states: root and start first, the others by (length, tokens)
        ctxs = sorted((g for g in listed if len(g) < order and g[-1] != EOS and g != (BOS,)), key=lambda g: (len(g), g))
        names = ([(BOS,), ()] if (BOS,) in listed else [()]) + ctxs
        state_of = {g: i for i, g in enumerate(names)}
        S, root = len(names), state_of[()]

        def longest_state(g):
            while g not in state_of:
                g = g[1:]
            return state_of[g]

        rows: List[List[Tuple[int, float]]] = [[] for _ in names]
        eos_p: Dict[Tuple[int, ...], float] = {}
        for g, (p, _) in listed.items():
            if g[-1] == EOS:
                eos_p[g[:-1]] = p
            elif g != (BOS,):
                rows[state_of[g[:-1]]].append((g[-1], p))
        have = {k for k, _ in rows[root]}
        if len(have) < V:
            if oov_logp is None:
                missing = [k for k in range(V) if k not in have]
                raise ValueError(f"from_ngrams: {len(missing)} tokens have no unigram (the first: {missing[:8]}; the blank is one "
                                 "unless listed) and no oov_logp is given for them")
            rows[root].extend((k, float(oov_logp)) for k in range(V) if k not in have)
        keep = order - 1
        row_ptr, tok, arc, nxt = [0], [], [], []
        for g, row in zip(names, rows):
            row.sort()
            for k, p in row:
                tok.append(k)
                arc.append(weight * p)
                nxt.append(longest_state((g + (k,))[-keep:] if keep else ()))
            row_ptr.append(len(tok))
        bow = [weight * listed[g][1] if g else 0.0 for g in names]
        backoff = [longest_state(g[1:]) if g else root for g in names]
        f32 = lambda xs: torch.tensor(xs, dtype=torch.float64).to(torch.float32)
        i32 = lambda xs: torch.tensor(xs, dtype=torch.int32)
        out = cls(i32(row_ptr), i32(tok), f32(arc), i32(nxt), f32(bow), i32(backoff), torch.zeros(S, dtype=torch.float32), root, order, V)
        if has_eos:   # final: the lookup of </s>, whose arcs live beside the table
            eos_arc = {state_of[g]: float(np.float32(weight * p)) for g, p in eos_p.items()}
            bw, bk = out._tables()[4], out._tables()[5]
            fin = np.zeros(S, dtype=np.float32)
            for s in range(S):
                acc, h = 0.0, s
                while h not in eos_arc:       # the root lists </s>: the walk ends there at the latest
                    acc += float(bw[h])
                    h = int(bk[h])
                fin[s] = np.float32(acc + eos_arc[h])
            out.final = torch.from_numpy(fin)
            out._host = None
        return out

    @classmethod
    def from_arpa(cls, source: Union[str, Iterable[str]], symbols: Sequence[Optional[str]], weight: float, blank: int, *,
                  bos: str = "<s>", eos: str = "</s>", unk: str = "<unk>", oov_logp: Optional[float] = None) -> "NgramFusion":
        """From an ARPA file: `source` is a path or an iterable of lines; symbols[i] is the ARPA word of token id i, or None for
        an id the model does not know (the blank).  ARPA numbers are log10: each is multiplied by ln 10; a missing backoff is 0.
        Dropped: an n-gram with a word outside `symbols` (bos and eos aside), with <s> past its first position or with </s>
        before its last.  The unigram of `unk` supplies oov_logp when the caller gives none.
        ValueError: from_ngrams' cases (an n-gram whose context is not listed, a non-finite number, order > 8, tokens without
        a unigram and no oov_logp); a duplicate n-gram; a count line that disagrees with its section; a malformed line; two ids
        with the same word."""
        if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
            with open(source, "r", encoding="utf-8") as f:
                lines = f.read().splitlines()
        else:
            lines = [str(l).rstrip("\r\n") for l in source]
        id_of: Dict[str, int] = {}
        for i, w in enumerate(symbols):
            if w is None:
                continue
            if w in id_of or w in (bos, eos):
                raise ValueError(f"from_arpa: symbols lists {w!r} twice, or as an ordinary word")
            id_of[w] = i
        id_of[bos], id_of[eos] = cls.BOS, cls.EOS
        ln10 = math.log(10.0)
        counts: Dict[int, int] = {}
        seen: Dict[int, int] = {}
        raw = set()
        ngrams: Dict[Tuple[int, ...], Tuple[float, float]] = {}
        unk_logp = None
        section, in_data = 0, False
        for no, line in enumerate(lines, 1):
            line = line.strip()
            if not line:
                continue
            if line == "\\data\\":
                in_data = True
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                try:
                    section = int(line[1:-len("-grams:")])
                except ValueError:
                    raise ValueError(f"from_arpa: line {no}: bad section header {line!r}") from None
                if section not in counts:
                    raise ValueError(f"from_arpa: line {no}: section {section} has no count line")
                in_data, seen[section] = False, 0
                continue
            if in_data:
                if not line.startswith("ngram ") or "=" not in line:
                    raise ValueError(f"from_arpa: line {no}: expected 'ngram N=count', got {line!r}")
                n, c = line[len("ngram "):].split("=", 1)
                try:
                    counts[int(n)] = int(c)
                except ValueError:
                    raise ValueError(f"from_arpa: line {no}: bad count line {line!r}") from None
                continue
            if section == 0:
                continue   # a header before \data\
            f = line.split()
            if len(f) not in (section + 1, section + 2):
                raise ValueError(f"from_arpa: line {no}: a {section}-gram line has {len(f)} fields")
            try:
                p, b = float(f[0]), float(f[section + 1]) if len(f) == section + 2 else 0.0
            except ValueError:
                raise ValueError(f"from_arpa: line {no}: bad number in {line!r}") from None
            if not math.isfinite(p) or not math.isfinite(b):
                raise ValueError(f"from_arpa: line {no}: non-finite number in {line!r}")
            words = tuple(f[1:section + 1])
            if words in raw:
                raise ValueError(f"from_arpa: line {no}: the n-gram {' '.join(words)!r} is listed twice")
            raw.add(words)
            seen[section] += 1
            if words == (unk,):
                unk_logp = p * ln10
            if any(w not in id_of for w in words) or bos in words[1:] or eos in words[:-1]:
                continue
            ngrams[tuple(id_of[w] for w in words)] = (p * ln10, b * ln10)
        for n, c in counts.items():
            if seen.get(n, 0) != c:
                raise ValueError(f"from_arpa: the header counts {c} {n}-grams, the section lists {seen.get(n, 0)}")
        if not ngrams:
            raise ValueError("from_arpa: no n-gram over the given symbols")
        if max(counts, default=0) > MAX_ORDER:
            raise ValueError(f"from_arpa: order {max(counts)} exceeds {MAX_ORDER}")
        return cls.from_ngrams(ngrams, len(symbols), weight, blank, oov_logp=oov_logp if oov_logp is not None else unk_logp)
