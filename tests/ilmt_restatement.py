"""float64 torch restatement of the internal-LM training term (include/rnnt_hip.h, rnnt_hip_ilm_loss_*), written from
the definition and sharing no code with the library:

    z(u,b,v)   = C(u,b,v) + bias[v]                                        v != blank
    lse(u,b)   = log sum_{v != blank} exp z(u,b,v)
    ilm_nll[b] = sum_{u < u_lens[b]} (lse(u,b) - z(u,b,labels[b,u]))
    dC(u,b,v)  = gw[b] (exp(z(u,b,v) - lse(u,b)) - [v == labels[b,u]])     u < u_lens[b], v != blank;   0 elsewhere

A counted label that is the blank or outside [0, V) makes its utterance infeasible: ilm_nll[b] = +inf and row b of dC exactly zero."""
import torch


def ilm_nll_autograd(C, bias, labels, u_lens, blank):
    """The same per-utterance NLL (B,) as a differentiable float64 torch expression of C (U1,B,V) and bias (V), for oracle
    networks: every counted label must be valid (+inf has no gradient to compare)."""
    U1, B, V = C.shape
    keep = torch.tensor([v for v in range(V) if v != blank])
    z = (C + bias)[..., keep]
    lse = torch.logsumexp(z, dim=-1)
    labels = torch.as_tensor(labels).long()
    out = []
    for b in range(B):
        ub = int(u_lens[b])
        y = labels[b, :ub]
        assert not bool(((y < 0) | (y >= V) | (y == blank)).any())
        picked = (C[:ub, b] + bias).gather(1, y[:, None]).squeeze(1)
        out.append((lse[:ub, b] - picked).sum())
    return torch.stack(out)


def ilm_restatement(C, bias, labels, u_lens, blank, gw=None):
    """C (U1,B,V), bias (V), labels (B,U) integers, u_lens B integers, gw (B,) upstream weights (None: ones)
    -> ilm_nll (B,) float64, dC (U1,B,V) float64, lse (U1,B) float64."""
    C = torch.as_tensor(C).double()
    bias = torch.as_tensor(bias).double()
    labels = torch.as_tensor(labels).long()
    U1, B, V = C.shape
    gw = torch.ones(B, dtype=torch.float64) if gw is None else torch.as_tensor(gw).double()
    z = C + bias
    z[..., blank] = -float("inf")
    lse = torch.logsumexp(z, dim=-1)
    p = torch.exp(z - lse[..., None])   # exactly 0 in the blank column
    nll = torch.zeros(B, dtype=torch.float64)
    dC = torch.zeros(U1, B, V, dtype=torch.float64)
    for b in range(B):
        ub = int(u_lens[b])
        y = labels[b, :ub]
        if bool(((y < 0) | (y >= V) | (y == blank)).any()):
            nll[b] = float("inf")
            continue
        for u in range(ub):
            nll[b] += lse[u, b] - z[u, b, y[u]]
            dC[u, b] = p[u, b]
            dC[u, b, y[u]] -= 1.0
            dC[u, b] *= gw[b]
    return nll, dC, lse
