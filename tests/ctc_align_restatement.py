"""Float64 restatement of the CTC forced alignment (include/rnnt_hip.h: rnnt_hip_ctc_align), test support only.

Per utterance: lp (T, V) float64 log-probabilities (any matrix will do: the lattice does not care whether rows are normalised), labels
y_0..y_{U-1}, extended sequence l' of S = 2U + 1 states (l'_{2k} = blank, l'_{2k+1} = y_k).
    v_0(0) = lp[0,blank], v_0(1) = lp[0,y_0], everything else -inf
    v_t(s) = lp[t,l'_s] + max( v_{t-1}(s), v_{t-1}(s-1), [l'_s != blank and l'_s != l'_{s-2}] v_{t-1}(s-2) )
    score  = max( v_{T-1}(S-1), v_{T-1}(S-2) )
Tie rule: candidates in the order written (stay, s-1, s-2), a later one wins only when strictly greater; at the end the last label
state S-2 wins only when strictly greater than the trailing blank S-1.

`viterbi` is the forward pass with that rule, `margin` adds the backward pass (best minus the best path that leaves the best one
at some frame), `brute_force` enumerates every state sequence of a tiny lattice.  The second half builds the seeded inputs the GPU
tests use, so that the CPU tests can assert the float64 side's properties of exactly those inputs.
"""
import itertools

import numpy as np

NEG = -np.inf


def log_softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def extended(labels, blank):
    ext = np.full(2 * len(labels) + 1, blank, dtype=np.int64)
    ext[1::2] = np.asarray(labels, dtype=np.int64)
    return ext


def skip_allowed(ext, blank):
    skip = np.zeros(len(ext), dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    return skip


def _shift(v, n):
    out = np.full_like(v, NEG)
    out[n:] = v[:len(v) - n]
    return out


class Path:
    """states (T,) int, first / last (U,) int, token_logp (U,) float64, score float64; `ok` False for a lattice without any path
    (then score = -inf, first = last = -1, token_logp = 0, states = -1)."""

    def __init__(self, ok, states, first, last, token_logp, score):
        self.ok, self.states, self.first, self.last, self.token_logp, self.score = ok, states, first, last, token_logp, score

    def tokens(self, labels, blank):
        ext = extended(labels, blank)
        return np.array([ext[s] if s >= 0 else -1 for s in self.states], dtype=np.int64)


def spans(states, U):
    first, last = np.full(U, -1, dtype=np.int64), np.full(U, -1, dtype=np.int64)
    for t, s in enumerate(states):
        if s % 2 == 1:
            u = s // 2
            if first[u] < 0:
                first[u] = t
            last[u] = t
    return first, last


def path_score(lp, labels, blank, states):
    ext = extended(labels, blank)
    return float(sum(lp[t, ext[s]] for t, s in enumerate(states)))   # ascending t


def _no_path(T, U):
    return Path(False, np.full(T, -1, dtype=np.int64), np.full(U, -1, dtype=np.int64), np.full(U, -1, dtype=np.int64),
                np.zeros(U), NEG)


def forward(lp, labels, blank):
    """-> v (T, S) float64 and the back-pointers (T, S) in {0: stay, 1: s-1, 2: s-2}, with the tie rule."""
    lp = np.asarray(lp, dtype=np.float64)
    T, ext = lp.shape[0], extended(labels, blank)
    S, skip = len(ext), skip_allowed(extended(labels, blank), blank)
    e = lp[:, ext]
    v, bp = np.full((T, S), NEG), np.zeros((T, S), dtype=np.int8)
    v[0, 0] = e[0, 0]
    if S > 1:
        v[0, 1] = e[0, 1]
    for t in range(1, T):
        best, arg = v[t - 1].copy(), np.zeros(S, dtype=np.int8)
        c1 = _shift(v[t - 1], 1)
        m = c1 > best
        best, arg = np.where(m, c1, best), np.where(m, 1, arg)
        c2 = np.where(skip, _shift(v[t - 1], 2), NEG)
        m = c2 > best
        best, arg = np.where(m, c2, best), np.where(m, 2, arg)
        v[t], bp[t] = e[t] + best, arg
    return v, bp


def viterbi(lp, labels, blank):
    lp = np.asarray(lp, dtype=np.float64)
    T, U = lp.shape[0], len(labels)
    if T == 0:
        return _no_path(T, U)
    v, bp = forward(lp, labels, blank)
    S = 2 * U + 1
    vB, vL = v[T - 1, S - 1], (v[T - 1, S - 2] if S > 1 else NEG)
    s = S - 2 if vL > vB else S - 1
    score = float(max(vB, vL))
    if score == NEG:
        return _no_path(T, U)
    states = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    first, last = spans(states, U)
    tl = np.zeros(U)
    for u in range(U):
        acc = 0.0
        for t in range(first[u], last[u] + 1):   # ascending t
            acc += lp[t, labels[u]]
        tl[u] = acc
    return Path(True, states, first, last, tl, score)


def backward(lp, labels, blank):
    """w_t(s) = the best score of the frames AFTER t of a path that is in state s at frame t and ends legally (-inf: none)."""
    lp = np.asarray(lp, dtype=np.float64)
    T, ext = lp.shape[0], extended(labels, blank)
    S, skip = len(ext), skip_allowed(extended(labels, blank), blank)
    e = lp[:, ext]
    w = np.full((T, S), NEG)
    w[T - 1, S - 1] = 0.0
    if S > 1:
        w[T - 1, S - 2] = 0.0
    for t in range(T - 2, -1, -1):
        nxt = e[t + 1] + w[t + 1]
        best = nxt.copy()
        up1 = np.full(S, NEG)
        up1[:S - 1] = nxt[1:]
        up2 = np.full(S, NEG)
        up2[:S - 2] = np.where(skip[2:], nxt[2:], NEG)
        w[t] = np.maximum(best, np.maximum(up1, up2))
    return w


def margin(lp, labels, blank, best=None):
    """best score minus the best score of any path that differs from the best path: every other path leaves it at some frame, so
    the second best is the maximum of fwd_t(s) + bwd_t(s) over the (t, s) OFF the best path.  +inf when the best path is the only
    one (and for a lattice without any path)."""
    best = viterbi(lp, labels, blank) if best is None else best
    if not best.ok:
        return np.inf
    v, _ = forward(lp, labels, blank)
    through = v + backward(lp, labels, blank)
    through[np.arange(len(best.states)), best.states] = NEG
    second = through.max()
    return np.inf if second == NEG else best.score - second


def brute_force(lp, labels, blank):
    """Every legal state sequence with its score (ascending-t sum), best first; equal scores in the tie rule's order: the end
    state S-1 before S-2, then walking backwards the smaller jump first."""
    lp = np.asarray(lp, dtype=np.float64)
    T, ext = lp.shape[0], extended(labels, blank)
    S, skip = len(ext), skip_allowed(extended(labels, blank), blank)
    out = []
    for seq in itertools.product(range(S), repeat=T):
        if seq[0] > 1 or seq[-1] < S - 2:
            continue
        jumps = [b - a for a, b in zip(seq, seq[1:])]
        if any(j < 0 or j > 2 or (j == 2 and not skip[b]) for j, b in zip(jumps, seq[1:])):
            continue
        key = (S - 1 - seq[-1],) + tuple(reversed(jumps))
        out.append((path_score(lp, labels, blank, seq), key, seq))
    out.sort(key=lambda x: (-x[0], x[1]))
    return out


def repeats(labels):
    return sum(1 for a, b in zip(labels, labels[1:]) if a == b)


# --------------------------------------------------------------------------------------------------
# the seeded inputs of tests/test_gpu_ctc_align.py (numpy float32 logits; the float64 side reads the same float32 numbers).
# As tests/test_gpu_align.py documents for the transducer: the blank's logit leads the V - 1 labels together by BLANK_LEAD on every
# frame (p(blank) about 0.73 on a free frame), every label leads the blank by LABEL_LEAD on ONE frame of its own (p(label) about 0.7
# there; equal neighbours get a free frame between theirs), noise of standard deviation NOISE on everything.  So EVERY frame of every
# path costs about 0.3, label frames included: no score is so close to 0 that a tolerance relative to it (1e-5 * 0.3 = 3e-6 per frame)
# falls below what an fp32 log-softmax of logits of magnitude 5 .. 11 resolves (an ulp is 5e-7 .. 1e-6 there).  A label that led its
# frame by much more would cost nothing there, and a T = 1 row made of one such frame would have a score of -4e-4 that fp32 terms
# cannot give to 1e-5 relative.  Moving, stretching or dropping a label's frame trades a cost of about 0.3 for one of log(V-1) + 1 and
# more, while |best| is about 0.3 T: relative margins of 1e-3 and more at every size used here.
NLL_RTOL = 1e-5
BLANK_LEAD, LABEL_LEAD, NOISE = 1.0, 1.0, 0.25


class Case:
    def __init__(self, name, logits, labels, t_lens, u_lens, blank):
        self.name, self.logits, self.labels, self.t_lens, self.u_lens, self.blank = name, logits, labels, t_lens, u_lens, blank
        self.B, self.T, self.V = logits.shape
        self.U = labels.shape[1]
        self._oracle = None

    def row(self, b):
        Tb, Ub = self.t_lens[b], self.u_lens[b]
        return log_softmax64(self.logits[b, :Tb]), [int(x) for x in self.labels[b, :Ub]]

    def oracle(self):
        """[(best Path, margin, TOL)] per row, computed once."""
        if self._oracle is None:
            self._oracle = []
            for b in range(self.B):
                lp, y = self.row(b)
                best = viterbi(lp, y, self.blank)
                self._oracle.append((best, margin(lp, y, self.blank, best), NLL_RTOL * abs(best.score) if best.ok else 0.0))
        return self._oracle


def _fit(labels_row, want, Tb):
    """the longest prefix of at most `want` labels that still has a path in Tb frames"""
    u = want
    while u > 0 and u + repeats(list(labels_row[:u])) > Tb:
        u -= 1
    return u


def scheduled(name, seed, B, T, U, V, blank, ragged=True, rep=False, t_lens=None, u_lens=None):
    rng = np.random.default_rng(seed)
    logits = (NOISE * rng.normal(size=(B, T, V))).astype(np.float32)
    vals = np.array([v for v in range(V) if v != blank])
    labels = vals[rng.integers(0, len(vals), size=(B, max(U, 0)))].astype(np.int32)
    if rep and U >= 2:   # aa.., aab.., and a run of 5 where there is room
        labels[:, 1] = labels[:, 0]
        if U >= 8:
            labels[:, 3:8] = labels[:, 3:4]
    if t_lens is None:
        t_lens = [T] + ([int(x) for x in rng.integers(max(1, T // 2), T + 1, size=B - 1)] if ragged else [T] * (B - 1))
    if u_lens is None:
        want = [U] + ([int(x) for x in rng.integers(0, U + 1, size=B - 1)] if ragged else [U] * (B - 1))
        u_lens = [_fit(labels[b], want[b], t_lens[b]) for b in range(B)]
    boost = float(np.log(max(V - 1, 1))) + BLANK_LEAD
    logits[:, :, blank] += boost
    for b in range(B):
        Tb, Ub = t_lens[b], u_lens[b]
        y = list(labels[b, :Ub])
        gaps = np.cumsum([0] + [1 if y[k] == y[k - 1] else 0 for k in range(1, Ub)]) if Ub else np.zeros(0, dtype=np.int64)
        room = Tb - (int(gaps[-1]) if Ub else 0)
        if Ub and room >= Ub:
            f = np.sort(rng.choice(room, size=Ub, replace=False)) + gaps
        elif Ub and Tb > 0:   # a row without any path: the frames do not matter
            f = np.sort(rng.integers(0, Tb, size=Ub))
        else:
            f = np.zeros(0, dtype=np.int64)
        for u in range(len(f)):
            logits[b, f[u], y[u]] += boost + LABEL_LEAD   # (the blank keeps its boost there: the label leads it by LABEL_LEAD)
    return Case(name, logits, labels, list(t_lens), list(u_lens), blank)


def known_answer(name, spans_rows, T, V, blank):
    """Label u leads by 20 on the frames [a_u, b_u] of spans_rows[b][u] and the blank leads by 20 everywhere else: the spans of
    the best path are exactly those (equal neighbours must be given a free frame between their spans)."""
    B, U = len(spans_rows), max(len(r) for r in spans_rows)
    vals = [v for v in range(V) if v != blank]
    logits = np.zeros((B, T, V), np.float32)
    labels = np.tile(np.array([vals[u % len(vals)] for u in range(U)], np.int32), (B, 1))
    logits[:, :, blank] = 20.0
    for b, row in enumerate(spans_rows):
        for u, (a, z) in enumerate(row):
            logits[b, a:z + 1, blank] = 0.0
            logits[b, a:z + 1, labels[b, u]] = 20.0
    return Case(name, logits, labels, [T] * B, [len(r) for r in spans_rows], blank)


def margin_cases():
    """The seeded sets of the GPU file's margin rule: U in {0, 1, 63, 64, 65, 200, 511} (every K instance of the sweep and the lane
    boundaries), T in {1, 2, 7, 8, 9, 33, 70} (the PF ring and the 32-frame tile) and, where a full row of U labels needs them,
    U + a few frames; V in {2, 3, 72, 2048}, the largest at small T only; blank 0 and V - 1; repeated labels; ragged batches."""
    return [
        scheduled("T1_U0", 1, 4, 1, 0, 3, 0),
        scheduled("T1_U1", 2, 4, 1, 1, 3, 2),
        scheduled("T2_U1_V2", 3, 4, 2, 1, 2, 0),
        scheduled("T7_U3_rep", 4, 4, 7, 3, 3, 0, rep=True),
        scheduled("T8_U5_blank_last", 5, 4, 8, 5, 72, 71),
        scheduled("T9_U9", 6, 4, 9, 9, 72, 0),
        scheduled("T33_U20_V2048", 7, 3, 33, 20, 2048, 2047),
        scheduled("T33_U12_rep_V2", 8, 4, 33, 12, 2, 1, rep=True),
        scheduled("T70_U63", 9, 3, 70, 63, 72, 0),
        scheduled("T70_U64", 10, 3, 70, 64, 72, 71),
        scheduled("T70_U65_rep", 11, 3, 70, 65, 72, 0, rep=True),
        scheduled("T210_U200", 12, 3, 210, 200, 72, 0),
        scheduled("T520_U511", 13, 2, 520, 511, 72, 0),
        scheduled("T70_U511_short_rows", 14, 4, 70, 511, 3, 2, u_lens=[30, 0, 17, 5], rep=True),
    ]


def edge_case():
    """Rows 0, 2: T_b = U_b + repeats (a single path); rows 1, 3: one frame less (no path); row 4: no frame; row 5: an ordinary row."""
    c = scheduled("edges", 21, 6, 12, 6, 5, 0, rep=True, t_lens=[12] * 6, u_lens=[6] * 6)
    u_lens = [6, 6, 4, 4, 3, 6]
    need = [u_lens[b] + repeats(list(c.labels[b, :u_lens[b]])) for b in range(6)]   # (the labels depend on the seed and shapes only)
    return scheduled("edges", 21, 6, 12, 6, 5, 0, rep=True, t_lens=[need[0], need[1] - 1, need[2], need[3] - 1, 0, 12], u_lens=u_lens)


def known_answer_case():
    return known_answer("known", [[(0, 0), (1, 3), (9, 9)], [(2, 5), (7, 7)], [], [(39, 39)], [(0, 39)]], 40, 4, 3)
