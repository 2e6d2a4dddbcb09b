"""CPU restatement of the STREAMING frame-synchronous beam search (include/rnnt_hip.h: rnnt_hip_beam_sync_stream_chunk), test
side, float64.  The definition is one sentence: after the chunks fed so far, a stream's n-best is `search_one`
(tests/beam_sync_restatement.py) on the encoder rows fed since its reset, whatever the chunking, and its stable prefix is the
longest common prefix of those hypotheses.  A unidirectional encoder's row t depends on frames <= t only, so the rows are
computed once and sliced.

`traced` runs the same search (written again here, from the definition, with the prefix tree made explicit) and reports what
the device's tree collection has to get right:
  rereached   the prefixes that were created, then pruned (no beam member had them as a prefix when a frame started) and
              later reached again, with the frames of creation and of the first re-reach.  A collection that kept only the
              paths to the beam members would re-create them with the later frame.
  tree[t]     the nodes of the append-only offline tree after frame t
  keep[t]     the nodes of the exact keep set after frame t: with R = the longest common prefix of the beam members, the
              prefixes of a member from R on, and every created prefix that a member is a proper prefix of
"""
import math

import torch
import torch.nn.functional as F

from tests import beam_sync_restatement as R


def common_prefix(seqs):
    seqs = [list(s) for s in seqs]
    out = []
    for column in zip(*seqs):
        if any(k != column[0] for k in column):
            break
        out.append(column[0])
    return out


@torch.no_grad()
def encode(net64, audio, n):
    """Rows (n, Oe) float64 of utterance `audio` (1, T, F) through a unidirectional float64 oracle encoder."""
    if n == 0:
        return torch.zeros(0, net64.encoder.out_proj.out_features, dtype=torch.float64)
    return net64.encoder(audio[:, :n].double(), [n])[0]


class Stream:
    """One stream fed in chunks: `feed(k)` consumes k more frames and returns the Result of search_one on everything fed."""

    def __init__(self, net64, audio, blank, W, S=1, token_min_logp=-math.inf, fusion=None):
        self.net, self.args = net64, (blank, W, S, token_min_logp, fusion)
        self.rows = encode(net64, audio, audio.size(1))
        self.n = 0
        self.result = R.search_one(net64, self.rows[:0], *self.args)

    def feed(self, k):
        if k > 0:
            self.n += k
            self.result = R.search_one(self.net, self.rows[:self.n], *self.args)
        return self.result

    def stable_prefix(self):
        """(tokens, frames): the common prefix of the hypotheses' sequences; the frames of a common prefix are common too."""
        ys = [h[0] for h in self.result.hyps]
        p = common_prefix(ys)
        return p, self.result.hyps[0][-1][:len(p)]


class Trace:
    def __init__(self):
        self.hyps, self.rereached, self.tree, self.keep, self.final_rereached = [], {}, [], [], []


@torch.no_grad()
def traced(net, enc_rows, blank, W, S=1):
    """The unfused search with no threshold on enc_rows (T, Oe) float64, the tree explicit.  -> Trace: hyps [(y, score, frames)]
    best first, rereached {y: (frame created, frame first reached again)}, tree[t], keep[t], final_rereached (the re-reached
    prefixes that a final hypothesis starts with)."""
    V = net.fc.out_features
    steps = R._Steps(net)
    root = (blank,)
    born = {root: -1}
    A = [(root, 0.0)]
    tr = Trace()
    for t in range(enc_rows.size(0)):
        live = {m[:k] for m, _ in A for k in range(1, len(m) + 1)}   # every prefix of a member: what "paths only" would keep
        C, D, order = A, {}, []

        def add(y, s):
            if y in D:
                D[y] = R.logaddexp(D[y], s)
            else:
                D[y] = s
                order.append(y)
        for r in range(S):
            if not C:
                break
            d = torch.stack([steps(y)[0] for y, _ in C])
            z = net.fc(F.gelu(torch.cat((enc_rows[t].expand(len(C), -1), d), dim=1), approximate="tanh"))
            val = torch.tensor([s for _, s in C], dtype=torch.float64)[:, None] + torch.log_softmax(z, dim=1)
            flat = val.reshape(-1)
            sel = torch.sort(flat, descending=True, stable=True).indices[:W].tolist()
            nxt = []
            for cid in sel:
                if float(flat[cid]) == -math.inf:
                    continue
                i, v = divmod(cid, V)
                y, s = C[i][0], float(flat[cid])
                if v == blank:
                    add(y, s)
                    continue
                y = y + (v,)
                if y in born and born[y] < t and y not in live and y not in tr.rereached:
                    tr.rereached[y] = (born[y], t)
                born.setdefault(y, t)
                if r < S - 1:
                    nxt.append((y, s))
                else:
                    add(y, s)
            C = nxt
        A = [(y, D[y]) for y in sorted(order, key=lambda y: -D[y])][:W]   # stable: first insertion first
        root_len = len(common_prefix([m for m, _ in A]))
        members = [m for m, _ in A]
        keep = {m[:k] for m in members for k in range(root_len, len(m) + 1)}
        keep |= {y for y in born if any(len(y) > len(m) and y[:len(m)] == m for m in members)}
        tr.tree.append(len(born))
        tr.keep.append(len(keep))
    idx = sorted(range(len(A)), key=lambda i: -A[i][1])
    tr.hyps = [(list(A[i][0]), A[i][1], [born[A[i][0][:k + 1]] for k in range(len(A[i][0]))]) for i in idx]
    tr.final_rereached = [y for y in tr.rereached if any(tuple(h[0][:len(y)]) == y for h in tr.hyps)]
    return tr
