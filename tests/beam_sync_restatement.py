"""Plain CPU restatement of the frame-synchronous transducer beam search (include/rnnt_hip.h: rnnt_hip_beam_sync_search), test
side, in float64 on the torch-CPU oracle networks: fp64 prediction net, joint and log-softmax.  Written from the definition,
independently of csrc/beam_sync.hip: hypotheses are dicts holding their own token tuple; D is a python dict.

Definition.  Inputs: the encoder rows of one utterance, the prediction net and its half of the joint, blank, W = beam width in
[1,64], S = max_symbols in [1,4], token_min_logp (default -inf), an optional TokenFusion.
A hypothesis is a token sequence y (the root is [blank]; one prefix-tree node per prefix), an fp64 score, the prediction-net
state after y with its output d, and with fusion an automaton state and an fp64 total.  lp_h = log_softmax(joint(enc_t, d_h)).
  start   one hypothesis: the root, score 0; its state is one step on blank from the zero state
  frame   for each frame t, with C = the beam A and D = empty, rounds r = 0..S-1; an empty C stops the rounds:
    1. candidates of the member h at rank i of C: blank with value score_h + lp_h[blank]; every v != blank with
       lp_h[v] >= token_min_logp with value score_h + lp_h[v]; candidate id i V + v.  With fusion the rank key is value + total',
       total' = total_h for blank and total_h + arc[s_h, v] otherwise; the pruning test stays on lp.
    2. the min(W, #candidates) best by (key descending, id ascending) are selected; a value (or key) of -inf is dropped.
    3. in rank order: a selected blank closes h: it is added to D under y_h; if y_h is in D already the scores merge,
       score = logaddexp(old, new).  A selected token v makes the child y_h + [v] with the new score, the automaton advanced and
       the state one step further; if r < S-1 it joins the next round's C in rank order, if r = S-1 it is added to D like a
       closed one.
    4. the next A = the min(W, |D|) best of D by (score [+ total] descending, order of first insertion into D ascending).
  output  A after the last frame, best first by score (fused: score + total + final[state]), ties in A's order; no length
          normalisation; no frames gives [[blank]] with score 0.  Per token: the frame at which its prefix was first made
          (-1 for the leading blank).

Two margins come back with the hypotheses: the BOUNDARY margin, the smallest gap between the last kept and the first dropped key
over every round's select and every frame's top-W of D (with a finite token_min_logp also the distance of a log-probability
from the threshold, for tokens whose key is within 1e-4 of the select's boundary or above it), and the ORDER margin, the smallest
gap between adjacent output keys.
"""
import copy
import math

import torch
import torch.nn.functional as F


def logaddexp(a, b):
    m = max(a, b)
    if m == -math.inf:
        return -math.inf
    return m + math.log1p(math.exp(min(a, b) - m))


def double_net(net):
    return copy.deepcopy(net).double().eval()


class _Steps:
    """The prediction net after a token sequence: a pure function of y, computed once per prefix."""

    def __init__(self, net):
        self.dec, self.memo = net.decoder, {}

    def __call__(self, y):
        if y not in self.memo:
            prev = self(y[:-1])[1] if len(y) > 1 else None
            out, state = self.dec.rnn(self.dec.embedding(torch.tensor([[y[-1]]], dtype=torch.long)), prev)
            self.memo[y] = (self.dec.out_proj(out).view(-1), state)
        return self.memo[y]


class Result:
    def __init__(self, hyps, boundary, order, merges):
        self.hyps, self.boundary_margin, self.order_margin, self.merges = hyps, boundary, order, merges


@torch.no_grad()
def search_one(net, enc_rows, blank, W, S=1, token_min_logp=-math.inf, fusion=None):
    """net: a float64 OracleJointNet; enc_rows (T, Oe) float64 -> Result: hyps = [(y, score[, fused], frames)] best first."""
    V = net.fc.out_features
    steps = _Steps(net)
    tab = None
    if fusion is not None:
        tab = (fusion.next.cpu().tolist(), fusion.arc.cpu().double(), fusion.final.cpu().tolist())
    root = (blank,)
    born = {root: -1}
    A = [{"y": root, "score": 0.0, "fs": 0, "total": 0.0}]
    boundary, merges = math.inf, 0
    for t in range(enc_rows.size(0)):
        C, D = A, {}

        def add(h):
            nonlocal merges
            if h["y"] in D:
                D[h["y"]]["score"] = logaddexp(D[h["y"]]["score"], h["score"])
                merges += 1
            else:
                D[h["y"]] = h
        for r in range(S):
            if not C:
                break
            d = torch.stack([steps(h["y"])[0] for h in C])
            z = net.fc(F.gelu(torch.cat((enc_rows[t].expand(len(C), -1), d), dim=1), approximate="tanh"))
            lp = torch.log_softmax(z, dim=1)
            val = torch.tensor([h["score"] for h in C], dtype=torch.float64)[:, None] + lp
            key = val.clone()
            if tab is not None:
                tot = torch.tensor([h["total"] for h in C], dtype=torch.float64)[:, None] + tab[1][[h["fs"] for h in C]]
                tot[:, blank] = torch.tensor([h["total"] for h in C], dtype=torch.float64)
                key = val + tot
            keep = lp >= token_min_logp
            keep[:, blank] = True
            keep &= (val > -math.inf) & (key > -math.inf)
            flat = torch.where(keep, key, torch.full_like(key, -math.inf)).reshape(-1)
            order = torch.sort(flat, descending=True, stable=True).indices[:W + 1].tolist()   # stable: equal keys in id order
            order = [i for i in order if bool(keep.reshape(-1)[i])]
            sel = order[:W]
            edge = float(flat[order[W]]) if len(order) > W else -math.inf
            if len(order) > W:
                boundary = min(boundary, float(flat[sel[-1]]) - edge)
            if token_min_logp > -math.inf:   # a threshold decision that the select's outcome depends on
                near = ((lp - token_min_logp).abs() < 1e-4) & (key >= edge - 1e-4)
                near[:, blank] = False
                if bool(near.any()):
                    boundary = min(boundary, float((lp - token_min_logp).abs()[near].min()))
            nxt = []
            for cid in sel:
                i, v = divmod(cid, V)
                h = C[i]
                if v == blank:
                    add({"y": h["y"], "score": float(val[i, v]), "fs": h["fs"], "total": h["total"]})
                    continue
                y = h["y"] + (v,)
                born.setdefault(y, t)
                child = {"y": y, "score": float(val[i, v]), "fs": 0, "total": 0.0}
                if tab is not None:
                    child["fs"], child["total"] = tab[0][h["fs"]][v], h["total"] + float(tab[1][h["fs"], v])
                if r < S - 1:
                    nxt.append(child)
                else:
                    add(child)
            C = nxt
        ranked = sorted(D.values(), key=lambda h: -(h["score"] + h["total"]))   # stable: first insertion first
        if len(ranked) > W:
            boundary = min(boundary, (ranked[W - 1]["score"] + ranked[W - 1]["total"]) - (ranked[W]["score"] + ranked[W]["total"]))
        A = ranked[:W]
    out_key = [h["score"] + h["total"] + (tab[2][h["fs"]] if tab is not None else 0.0) for h in A]
    idx = sorted(range(len(A)), key=lambda i: -out_key[i])
    order_margin = min([out_key[idx[i]] - out_key[idx[i + 1]] for i in range(len(idx) - 1)], default=math.inf)
    hyps = []
    for i in idx:
        y = A[i]["y"]
        frames = [born[y[:k + 1]] for k in range(len(y))]
        hyps.append((list(y), A[i]["score"], out_key[i], frames) if tab is not None else (list(y), A[i]["score"], frames))
    return Result(hyps, boundary, order_margin, merges)


@torch.no_grad()
def search(net, audios, lens, blank, W, S=1, token_min_logp=-math.inf, fusion=None):
    """Batched front: net an fp32 OracleJointNet (converted here), every utterance on its own frames (none: no encoder call).
    -> list of Result."""
    net64 = double_net(net)
    out = []
    for b, n in enumerate(int(n) for n in lens):
        enc = net64.encoder(audios[b:b + 1, :n].double(), [n])[0] if n > 0 else torch.zeros(0, net64.encoder.out_proj.out_features,
                                                                                             dtype=torch.float64)
        out.append(search_one(net64, enc, blank, W, S, token_min_logp, fusion))
    return out


@torch.no_grad()
def greedy_one(net, enc_rows, blank, max_iters):
    """The oracle's greedy search (oracle/rnnt_oracle.py: recognize_greedy) in float64 WITHOUT its drop of a token that repeats
    the last appended one, with the log-probability of every choice.  -> (tokens with the leading blank, [(frame, token, lp)])."""
    steps = _Steps(net)
    y, picks = (blank,), []
    for t in range(enc_rows.size(0)):
        for _ in range(max_iters):
            lp = torch.log_softmax(net.fc(F.gelu(torch.cat((enc_rows[t], steps(y)[0])), approximate="tanh")), dim=0)
            k = int(lp.argmax())
            picks.append((t, k, float(lp[k])))
            if k == blank:
                break
            y = y + (k,)
    return list(y), picks


def drop_repeats(tokens, blank):
    """The reference's greedy rule (networks/transducer.py:132-133): a token equal to the last appended one is not appended."""
    out, last = [], blank
    for k in tokens:
        if k != last:
            out.append(k)
            last = k
    return out


@torch.no_grad()
def brute_force(net, enc_rows, blank, S):
    """Every path of the topology: in each frame a path emits j <= S tokens, followed by a blank iff j < S.  -> {y: log-mass}."""
    steps, acc = _Steps(net), {}
    T = enc_rows.size(0)
    lps = {}

    def lp_of(t, y):
        if (t, y) not in lps:
            lps[(t, y)] = torch.log_softmax(net.fc(F.gelu(torch.cat((enc_rows[t], steps(y)[0])), approximate="tanh")), dim=0).tolist()
        return lps[(t, y)]

    def rec(t, j, y, s):
        if t == T:
            acc[y] = logaddexp(acc.get(y, -math.inf), s)
            return
        lp = lp_of(t, y)
        for v in range(len(lp)):
            if v == blank:
                rec(t + 1, 0, y, s + lp[v])
            elif j + 1 == S:
                rec(t + 1, 0, y + (v,), s + lp[v])
            else:
                rec(t, j + 1, y + (v,), s + lp[v])
    rec(0, 0, (blank,), 0.0)
    return acc
