"""Lattice knowledge distillation for the fused RNN-T loss in float64 numpy, written from the definition (include/rnnt_hip.h,
DESIGN.md §27), for the tests.

Per lattice cell (t,u) of an utterance (cells t < Tb, u <= Ub) a softmax p over V entries is collapsed to three classes: the blank,
the cell's label y_u (only where u < Ub) and everything else.  With (a, c, r) the teacher's collapsed probabilities and
(p_b, p_y, p_r) the student's,
    kd = sum over cells and classes of P_T(k) (log P_T(k) - log P_S(k)),
    d kd / dz[v] = p[v] (1 - rho) - [v = blank] (a - rho p_b) - [v = y_u] (c - rho p_y),     rho = r / p_r,
i.e. w = 1 - rho, cb = a - rho p_b, ce = c - rho p_y in the lattice gradient's dz[v] = w p[v] - [v = blank] cb - [v = y_u] ce.
The planes are laid out (B, U+1, T) as the library's.  The transducer term (and FastEmit) comes from tests/fastemit_restatement.py.
Nothing here is shared with the library or with oracle/."""
import numpy as np

from tests import fastemit_restatement as fr


def _labels(labels, b, U1):
    return np.asarray(labels[b][:U1 - 1], dtype=np.int64) if U1 > 1 else np.zeros(0, dtype=np.int64)


def planes_from_logits(z, labels, u_lens, blank):
    """Materialised logits z (B,T,U1,V) -> blk, emit, rest (B,U1,T) float64.  rest is the log-sum-exp of the log-softmax over every
    entry but the blank and (u < u_lens[b]) the label; emit is 0 at u = U1-1 and the padded label's value at u_lens[b] <= u < U1-1."""
    z = np.asarray(z, dtype=np.float64)
    B, T, U1, V = z.shape
    blk, emit, rest = (np.zeros((B, U1, T)) for _ in range(3))
    for b in range(B):
        lp = fr.log_softmax(z[b])
        y = _labels(labels, b, U1)
        blk[b] = lp[:, :, blank].T
        for u in range(U1):
            keep = np.ones(V, dtype=bool)
            keep[blank] = False
            if u < U1 - 1:
                emit[b, u] = lp[:, u, y[u]]
            if u < int(u_lens[b]):
                keep[y[u]] = False
            x = lp[:, u, keep]
            m = x.max(axis=1)
            rest[b, u] = m + np.log(np.exp(x - m[:, None]).sum(axis=1))
    return blk, emit, rest


def cell_planes(A, C, bias, labels, u_lens, blank):
    """planes_from_logits for the separable form: A (B,T,V), C (B,U1,V), bias (V), one utterance at a time."""
    A, C, bias = (np.asarray(x, dtype=np.float64) for x in (A, C, bias))
    rows = [planes_from_logits((A[b][:, None, :] + C[b][None, :, :] + bias)[None], labels[b:b + 1], u_lens[b:b + 1], blank)
            for b in range(A.shape[0])]
    return tuple(np.concatenate([r[k] for r in rows]) for k in range(3))


def kd_value(student, teacher, t_lens, u_lens):
    """(blk, emit, rest) planes of both sides -> kd (B,), and per row the sum of the absolute values of the class terms."""
    B = student[0].shape[0]
    kd, mag = np.zeros(B), np.zeros(B)
    for b in range(B):
        Tb, Ub = int(t_lens[b]), int(u_lens[b])
        for k, (s, t) in enumerate(zip(student, teacher)):
            nu = Ub if k == 1 else Ub + 1          # the label class: u < Ub only
            lt, ls = t[b, :nu, :Tb], s[b, :nu, :Tb]
            p = np.exp(lt)
            with np.errstate(invalid="ignore"):
                term = np.where(p > 0, p * (lt - ls), 0.0)
            kd[b] += term.sum()
            mag[b] += np.abs(term).sum()
    return kd, mag


def kd_cell_gradient(lp, y, Tb, Ub, blank, t_blk, t_emit, t_rest):
    """One utterance: lp (T,U1,V) the student's log-softmax, teacher planes (U1,T) -> d kd / dz (T,U1,V), zeros outside the lattice.
    The scalar formula, evaluated as p[v] - q[v] with q = a on the blank, c on the label and rho p[v] elsewhere, which is the same
    expression without the cancellation p_b (1 - rho) + rho p_b has in floating point once rho is large."""
    T, U1, V = lp.shape
    dz = np.zeros_like(lp)
    p = np.exp(lp)
    for u in range(Ub + 1):
        keep = np.ones(V, dtype=bool)
        keep[blank] = False
        if u < Ub:
            keep[y[u]] = False
        x = lp[:Tb, u][:, keep]
        m = x.max(axis=1)
        rest_s = m + np.log(np.exp(x - m[:, None]).sum(axis=1))
        rho = np.exp(t_rest[u, :Tb] - rest_s)
        g = p[:Tb, u] * (1.0 - rho)[:, None]
        g[:, blank] = p[:Tb, u, blank] - np.exp(t_blk[u, :Tb])
        if u < Ub:
            g[:, y[u]] = p[:Tb, u, y[u]] - np.exp(t_emit[u, :Tb])
        dz[:Tb, u] = g
    return dz


def kd_fused(A, C, bias, labels, t_lens, u_lens, blank, teacher, g_nll, g_kd, lam=0.0):
    """The separable form z[b,t,u,:] = A[b,t,:] + C[b,u,:] + bias against a teacher's planes, with per-utterance upstream gradients
    g_nll (of the transducer term, FastEmit weight lam) and g_kd (of the distillation term).
    -> dict: planes (the student's), nll (B,), kd (B,), kd_mag (B,), dA (B,T,V), dC (B,U1,V), and S_A / S_C: per gradient entry the
    sum over the cells that feed it of |that cell's contribution| (the bound's scale)."""
    A, C, bias = (np.asarray(x, dtype=np.float64) for x in (A, C, bias))
    B, T, V = A.shape
    U1 = C.shape[1]
    planes = cell_planes(A, C, bias, labels, u_lens, blank)
    kd, mag = kd_value(planes, teacher, t_lens, u_lens)
    out = dict(planes=planes, kd=kd, kd_mag=mag, nll=np.zeros(B), dA=np.zeros_like(A), dC=np.zeros_like(C), S_A=np.zeros_like(A),
               S_C=np.zeros_like(C))
    for b in range(B):
        Tb, Ub = int(t_lens[b]), int(u_lens[b])
        z = A[b][:, None, :] + C[b][None, :, :] + bias
        n, dz = fr.fastemit_loss(z[None], labels[b:b + 1], t_lens[b:b + 1], u_lens[b:b + 1], blank, lam)
        out["nll"][b] = n[0]
        if Tb == 0:
            continue
        dk = kd_cell_gradient(fr.log_softmax(z), _labels(labels, b, U1), Tb, Ub, blank, teacher[0][b], teacher[1][b], teacher[2][b])
        tot = float(g_nll[b]) * dz[0] + float(g_kd[b]) * dk
        out["dA"][b], out["dC"][b] = tot.sum(1), tot.sum(0)
        out["S_A"][b], out["S_C"][b] = np.abs(tot).sum(1), np.abs(tot).sum(0)
    return out


def kd_autograd_from_logits(z, labels, t_lens, u_lens, blank, teacher):
    """torch float64: z (B,T,U1,V) logits WITH a graph, teacher planes (numpy) -> kd (B,) with a graph: the materialised collapsed KL."""
    import torch
    B, T, U1, V = z.shape
    lp = torch.log_softmax(z, dim=-1)
    kd = []
    for b in range(B):
        Tb, Ub = int(t_lens[b]), int(u_lens[b])
        total = torch.zeros((), dtype=torch.float64)
        for u in range(Ub + 1):
            keep = torch.ones(V, dtype=torch.bool)
            keep[blank] = False
            cls = [lp[b, :Tb, u, blank]]
            tch = [teacher[0][b, u, :Tb]]
            if u < Ub:
                yu = int(labels[b][u])
                keep[yu] = False
                cls.append(lp[b, :Tb, u, yu])
                tch.append(teacher[1][b, u, :Tb])
            cls.append(torch.logsumexp(lp[b, :Tb, u][:, keep], dim=1))
            tch.append(teacher[2][b, u, :Tb])
            for ls, lt in zip(cls, tch):
                lt = torch.as_tensor(np.asarray(lt, dtype=np.float64))
                total = total + (lt.exp() * (lt - ls)).sum()
        kd.append(total)
    return torch.stack(kd)


def kd_materialised_autograd(A, C, bias, labels, t_lens, u_lens, blank, teacher):
    """torch float64 autograd through the materialised (B,T,U1,V) collapsed KL -> kd (B,), d sum(kd) / dA, dC.  The check of the
    formulas above (tests/test_kd_oracle.py); tiny shapes only."""
    import torch
    A, C = (torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True) for x in (A, C))
    bias = torch.tensor(np.asarray(bias, dtype=np.float64))
    kd = kd_autograd_from_logits(A[:, :, None, :] + C[:, None, :, :] + bias, labels, t_lens, u_lens, blank, teacher)
    kd.sum().backward()
    return kd.detach().numpy(), A.grad.numpy(), C.grad.numpy()
