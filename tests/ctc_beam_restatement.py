"""numpy float64 restatement of the CTC prefix beam search that include/rnnt_hip.h defines (rnnt_hip_ctc_beam_search):
fp32-rounded logits in, a dict of prefixes per frame, the kernel's candidate ids and tie rule.  No device work.

    hyps, boundary_margin, order_margin = search(z, blank, W, token_min_logp=-inf, fusion=None)

z (T, V) holds the frames of ONE utterance (already cut to its length).  hyps: best first, dicts with `tokens`, `score`, `fused`
(score + total + final[state]; equal to score without fusion), `total`, `frames`.
boundary_margin: the minimum over frames of the gap between the rank keys of the W-th and the (W+1)-th candidate (inf where a
frame has at most W candidates): above it the kernel's fp32 log-sum-exp and logaddexp corrections cannot change a beam.
order_margin: the minimum gap between the output keys of adjacent final hypotheses (inf for fewer than two)."""
import math

import numpy as np

NEG = -math.inf


def log_softmax(z):
    """fp64 log-softmax of the fp32-rounded logits, per row."""
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))


def lae(a, b):
    return float(np.logaddexp(a, b)) if max(a, b) > NEG else NEG


def fusion_tables(fusion):
    """(next, arc, final) of a TokenFusion as numpy arrays (arc and final in float64), or None."""
    if fusion is None:
        return None
    return (fusion.next.cpu().numpy(), fusion.arc.cpu().numpy().astype(np.float64), fusion.final.cpu().numpy().astype(np.float64))


def search(z, blank, W, token_min_logp=NEG, fusion=None, stats=None):
    """stats: a dict that receives `rereached`, the number of times a prefix entered a beam that had been in one before and was
    pruned since (it keeps its first node and frame)."""
    lp = log_softmax(z)
    T, V = lp.shape if lp.ndim == 2 else (0, 0)
    tab = fusion_tables(fusion)
    beam = [dict(prefix=(), pb=0.0, pnb=NEG, state=0, total=0.0)]
    created = {}          # prefix -> the frame at which it first entered the beam: one node per prefix, however often it is pruned
    bmargin = math.inf
    for t in range(T):
        row = lp[t]
        C = [k for k in range(V) if k != blank and row[k] >= token_min_logp]
        members = {h["prefix"]: r for r, h in enumerate(beam)}
        cand = {}
        for r, h in enumerate(beam):
            p = lae(h["pb"], h["pnb"])
            stay = h["pnb"] + row[h["prefix"][-1]] if h["prefix"] else NEG
            cand[r * (V + 1)] = dict(prefix=h["prefix"], pb=p + row[blank], stay=stay, ext=NEG, state=h["state"], total=h["total"])
        for r, h in enumerate(beam):
            p = lae(h["pb"], h["pnb"])
            e = h["prefix"][-1] if h["prefix"] else None
            for k in C:
                ext = (h["pb"] if k == e else p) + row[k]
                new = h["prefix"] + (k,)
                if new in members:       # the same candidate as that member's survivor
                    cand[members[new] * (V + 1)]["ext"] = ext
                else:
                    state, total = h["state"], h["total"]
                    if tab is not None:
                        total = total + tab[1][state, k]
                        state = int(tab[0][state, k])
                    cand[r * (V + 1) + 1 + k] = dict(prefix=new, pb=NEG, stay=NEG, ext=ext, state=state, total=total)
        keyed = []
        for i, c in cand.items():
            c["pnb"] = lae(c["stay"], c["ext"])
            score = lae(c["pb"], c["pnb"])
            if score > NEG:
                keyed.append((-(score + c["total"]), i))
        keyed.sort()
        if len(keyed) > W:
            bmargin = min(bmargin, keyed[W][0] - keyed[W - 1][0])
        beam = []
        for _, i in keyed[:W]:
            c = cand[i]
            if stats is not None and c["prefix"] in created and c["prefix"] not in members:
                stats["rereached"] = stats.get("rereached", 0) + 1
            created.setdefault(c["prefix"], t)
            beam.append(dict(prefix=c["prefix"], pb=c["pb"], pnb=c["pnb"], state=c["state"], total=c["total"]))
    hyps = []
    for r, h in enumerate(beam):
        score = lae(h["pb"], h["pnb"])
        fused = score + h["total"] + (tab[2][h["state"]] if tab is not None else 0.0)
        hyps.append(dict(tokens=list(h["prefix"]), score=score, fused=float(fused), total=float(h["total"]),
                         frames=[created[h["prefix"][:i + 1]] for i in range(len(h["prefix"]))], rank=r))
    hyps.sort(key=lambda h: (-h["fused"], h["rank"]))
    omargin = min([a["fused"] - b["fused"] for a, b in zip(hyps, hyps[1:])], default=math.inf)
    return hyps, bmargin, omargin


def first_seed(T, V, W, scale, token_min_logp=NEG, blank=0, fusion=None, start=0, tries=20, margin=1e-4):
    """The first seed of `tries` from `start` whose search keeps a boundary margin >= `margin`: (seed, logits (T,V) fp32, hyps,
    boundary margin, order margin), logits = scale * standard normal from numpy.random.default_rng(1000 + seed).  None if none does."""
    for seed in range(start, start + tries):
        z = (scale * np.random.default_rng(1000 + seed).standard_normal((T, V))).astype(np.float32)
        hyps, bm, om = search(z, blank, W, token_min_logp, fusion)
        if bm >= margin:
            return seed, z, hyps, bm, om
    return None
