"""Plain CPU restatement of the frame-synchronous beam search with internal-LM subtraction (include/rnnt_hip.h:
rnnt_hip_beam_sync_search_ilm), test side, in float64 on the torch-CPU oracle networks.  tests/beam_sync_restatement.py's
search_one written out again with the one extra term; its helpers are imported, the search loop is not.

The internal LM of a hypothesis h with prediction-net output d_h: the joint with the encoder vector zeroed BEFORE the activation,
fc(gelu(cat(0, d_h))), restricted to the non-blank tokens, log-softmax over those:  ilm_h[v], v != blank.  With weight mu the
total of a child is  total' = (total_h + arc[s_h, v]) - mu * ilm_h[v];  the blank's is total_h.  Everything else is
search_one's: ranking by value + total', the top-W of D by score + total, the output by score + total + final, the prune test on
the ASR log-probability.  Without a fusion automaton and mu > 0 the all-zero one-state automaton stands in (entries then carry a
fused score); mu = 0 is search_one itself.

The BOUNDARY margin includes the term in every key it compares.  `ilm_score_fp64` is the independent teacher-forced scorer: its
own step loop over the prediction net, not the search's memo.
"""
import math

import torch
import torch.nn.functional as F

from tests.beam_sync_restatement import Result, _Steps, double_net, logaddexp   # noqa: F401  (double_net: for the callers)
from tests.beam_sync_stream_restatement import common_prefix


def ilm_row(net, d, blank):
    """d (n, Od) float64 prediction-net outputs -> (n, V) float64: the internal LM's log-probabilities, -inf at the blank."""
    Oe = net.fc.in_features - d.size(1)
    z = net.fc(F.gelu(torch.cat((torch.zeros(d.size(0), Oe, dtype=d.dtype), d), dim=1), approximate="tanh"))
    keep = [v for v in range(z.size(1)) if v != blank]
    out = torch.full_like(z, -math.inf)
    out[:, keep] = torch.log_softmax(z[:, keep], dim=1)
    return out


@torch.no_grad()
def ilm_score_fp64(net, y, blank):
    """net: a float64 OracleJointNet; y: tokens with the leading blank -> sum over u >= 1 of ilm(y_u | y_<u), teacher forced."""
    dec = net.decoder
    state, total = None, 0.0
    for u in range(1, len(y)):
        out, state = dec.rnn(dec.embedding(torch.tensor([[y[u - 1]]], dtype=torch.long)), state)
        total += float(ilm_row(net, dec.out_proj(out).view(1, -1), blank)[0, y[u]])
    return total


@torch.no_grad()
def search_one(net, enc_rows, blank, W, S=1, token_min_logp=-math.inf, fusion=None, mu=0.0):
    """net: a float64 OracleJointNet; enc_rows (T, Oe) float64 -> Result: hyps = [(y, score[, fused], frames)] best first; the
    fused score is there with a fusion automaton or mu > 0."""
    V = net.fc.out_features
    steps = _Steps(net)
    tab = None
    if fusion is not None:
        tab = (fusion.next.cpu().tolist(), fusion.arc.cpu().double(), fusion.final.cpu().tolist())
    elif mu > 0.0:
        tab = ([[0] * V], torch.zeros(1, V, dtype=torch.float64), [0.0])
    root = (blank,)
    born = {root: -1}
    A = [{"y": root, "score": 0.0, "fs": 0, "total": 0.0}]
    boundary, merges = math.inf, 0
    keep_n, tree_n = [], []
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
            tot = None
            if tab is not None:
                own = torch.tensor([h["total"] for h in C], dtype=torch.float64)
                tot = own[:, None] + tab[1][[h["fs"] for h in C]]
                if mu > 0.0:
                    ilm = ilm_row(net, d, blank)
                    ilm[:, blank] = 0.0                      # (no term for the blank; keeps the product finite)
                    tot = tot - mu * ilm
                tot[:, blank] = own
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
                    child["fs"], child["total"] = tab[0][h["fs"]][v], float(tot[i, v])
                if r < S - 1:
                    nxt.append(child)
                else:
                    add(child)
            C = nxt
        ranked = sorted(D.values(), key=lambda h: -(h["score"] + h["total"]))   # stable: first insertion first
        if len(ranked) > W:
            boundary = min(boundary, (ranked[W - 1]["score"] + ranked[W - 1]["total"]) - (ranked[W]["score"] + ranked[W]["total"]))
        A = ranked[:W]
        # what a stream's tree collection keeps after this frame (beam_sync_stream_restatement.traced's keep set), and the
        # append-only tree beside it
        members = [h["y"] for h in A]
        root_len = len(common_prefix(members))
        kept = {m[:k] for m in members for k in range(root_len, len(m) + 1)}
        kept |= {y for y in born if any(len(y) > len(m) and y[:len(m)] == m for m in members)}
        keep_n.append(len(kept))
        tree_n.append(len(born))
    out_key = [h["score"] + h["total"] + (tab[2][h["fs"]] if tab is not None else 0.0) for h in A]
    idx = sorted(range(len(A)), key=lambda i: -out_key[i])
    order_margin = min([out_key[idx[i]] - out_key[idx[i + 1]] for i in range(len(idx) - 1)], default=math.inf)
    hyps = []
    for i in idx:
        y = A[i]["y"]
        frames = [born[y[:k + 1]] for k in range(len(y))]
        hyps.append((list(y), A[i]["score"], out_key[i], frames) if tab is not None else (list(y), A[i]["score"], frames))
    res = Result(hyps, boundary, order_margin, merges)
    res.keep, res.tree = keep_n, tree_n   # per frame: nodes of the exact keep set, nodes of the uncollected tree
    return res


@torch.no_grad()
def search(net, audios, lens, blank, W, S=1, token_min_logp=-math.inf, fusion=None, mu=0.0):
    """Batched front, as beam_sync_restatement.search: net an fp32 OracleJointNet (converted here) -> list of Result."""
    net64 = double_net(net)
    out = []
    for b, n in enumerate(int(n) for n in lens):
        enc = net64.encoder(audios[b:b + 1, :n].double(), [n])[0] if n > 0 else torch.zeros(0, net64.encoder.out_proj.out_features,
                                                                                             dtype=torch.float64)
        out.append(search_one(net64, enc, blank, W, S, token_min_logp, fusion, mu))
    return out
