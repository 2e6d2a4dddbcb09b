"""Plain CPU restatement of the reference's beam search (networks/transducer.py:215-361 with lm=None, hotwords=None), test side.

Written from the reference's semantics, independently of csrc/beam.hip: hypotheses are dicts holding their own y_star list
and hidden state, every pop runs a prediction-net step (no memo), A and B are python lists.  Log-probabilities are fp32
torch tensors (the reference's tensor arithmetic, including the fp32 prune test), scores are python floats (fp64).

`margin` is the smallest gap over every decision the search takes: each pop's argmax (best vs second-best A score), each
improved early-out and each stop comparison, each prune comparison, and the final sort up to the cut.  A result whose margin
is >= 1e-4 does not hang on fp32 summation order.
"""
import math

import torch
import torch.nn.functional as F


def _step(dec, token: int, state):
    y, state = dec.rnn(dec.embedding(torch.tensor([[token]], dtype=torch.long)), state)
    return dec.out_proj(y).view(-1), state


def beam_search_one(net, enc_rows: torch.Tensor, blank: int, beam: int, improved: bool = False, state_beam: float = 4.6,
                    expand_beam: float = 2.3):
    """enc_rows (T, Oe): one utterance's encoder outputs.  net: an OracleJointNet (or anything with .decoder.{embedding,rnn,
    out_proj} and .fc).  Returns (nbest [(y_star, score)], margin, stats dict)."""
    margin = math.inf
    stats = {"pops": 0, "dedupe_pops": 0, "empty_a": 0, "max_pops_frame": 0}

    def gap(x, y):
        nonlocal margin
        margin = min(margin, abs(float(x) - float(y)))

    B_hyps = [{"score": 0.0, "y": [blank], "state": None, "dedupe": False}]
    for t in range(enc_rows.size(0)):
        A_hyps, B_hyps = B_hyps, []
        pops = 0
        while A_hyps:
            scores = [h["score"] for h in A_hyps]
            i_best = max(range(len(A_hyps)), key=lambda i: scores[i])   # first of equal maxima (python's max)
            a_best = scores[i_best]
            if len(scores) > 1:
                gap(a_best, max(s for i, s in enumerate(scores) if i != i_best))
            b_best = max(h["score"] for h in B_hyps) if B_hyps else -9999.0
            if improved:
                gap(b_best, state_beam + a_best)
                if b_best >= state_beam + a_best:
                    break
            a = A_hyps.pop(i_best)
            pops += 1
            stats["pops"] += 1
            stats["dedupe_pops"] += int(a["dedupe"])
            d, new_state = _step(net.decoder, a["y"][-1], a["state"])
            z = net.fc(F.gelu(torch.cat((enc_rows[t], d)), approximate="tanh"))
            logp = torch.log_softmax(z, dim=0)
            best_prob = torch.max(logp[1:])
            thr = best_prob - expand_beam   # fp32 tensor arithmetic
            for k in range(logp.numel()):
                score = a["score"] + float(logp[k])
                if k == blank:
                    B_hyps.append({"score": score, "y": list(a["y"]), "state": a["state"], "dedupe": False})
                    continue
                if improved:
                    gap(logp[k], thr)
                    if not bool(logp[k] >= thr):
                        continue
                same = a["y"][-1] == k
                A_hyps.append({"score": score, "y": a["y"] if same else a["y"] + [k], "state": new_state, "dedupe": same})
            if not A_hyps:   # the reference's max() would raise ValueError here (improved mode); the frame ends
                stats["empty_a"] += 1
                break
            if len(B_hyps) >= beam:
                max_a, max_b = max(h["score"] for h in A_hyps), max(h["score"] for h in B_hyps)
                gap(max_b, max_a)
                if max_b > max_a:
                    break
        stats["max_pops_frame"] = max(stats["max_pops_frame"], pops)
    keys = [h["score"] / len(h["y"]) for h in B_hyps]
    order = sorted(range(len(B_hyps)), key=lambda i: keys[i], reverse=True)   # stable, like the reference's sorted()
    for r in range(min(beam, len(order) - 1)):
        gap(keys[order[r]], keys[order[r + 1]])
    return [(B_hyps[i]["y"], B_hyps[i]["score"]) for i in order[:beam]], margin, stats


@torch.no_grad()
def beam_search(net, audios: torch.Tensor, lens, blank: int, beam: int, improved: bool = False, state_beam: float = 4.6,
                expand_beam: float = 2.3, visit_padded_frames: bool = False):
    """Batched front: encoder on the padded batch, then every utterance on its own frames (all T frames with
    visit_padded_frames).  Returns (per-utterance nbest lists, min margin, per-utterance stats)."""
    enc = net.encoder(audios, list(lens))
    outs, margin, stats = [], math.inf, []
    for b in range(enc.size(0)):
        T = enc.size(1) if visit_padded_frames else int(lens[b])
        nb, m, st = beam_search_one(net, enc[b, :T], blank, beam, improved, state_beam, expand_beam)
        outs.append(nb)
        margin = min(margin, m)
        stats.append(st)
    return outs, margin, stats
