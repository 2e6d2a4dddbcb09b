"""RNNTLoss — drop-in for the two loss modules the reference constructs at model.py:31,39
(`warprnnt_pytorch.RNNTLoss(blank, reduction="mean")` / `torchaudio.transforms.RNNTLoss(...)`) and calls at
model.py:57 as `loss(logits, targets, logit_lengths, target_lengths)`, on the HIP alpha/beta kernels.
Returns a 0-d tensor for "mean"/"sum" (the warp-transducer build returns shape (1,), model.py:83-88; documented
difference), or (B,) for reduction="none".

CTCLoss — the CTC loss on per-frame logits (the auxiliary loss on the encoder's output, csrc/ctc.hip), same call shape.
"""
import torch
import torch.nn as nn

from .ops import Alignment, CtcLossFn, RnntLossFromLogitsFn, align_from_logits, check_fastemit_lambda


class RNNTLoss(nn.Module):
    """`fastemit_lambda` > 0 (finite, >= 0; default 0) adds FastEmit regularisation (Yu et al., ICASSP 2021): the gradient with respect
    to the label log-probabilities of every lattice cell is scaled by 1 + lambda and taken through the log-softmax exactly
    (include/rnnt_hip.h), which trains the model to emit sooner.  ONLY THE GRADIENT CHANGES: the returned loss is the unregularised
    negative log-likelihood, bit for bit what lambda = 0 returns.
    `forward(..., emit_windows=(lo, hi))`, two (B, U) int32 tensors, gives the alignment-restricted loss (Ar-RNN-T): label u of row b
    may be emitted only at frames lo[b,u] .. hi[b,u] (ops.emit_windows builds them around a reference alignment); a row whose windows
    leave no path has loss +inf and a zero gradient.  None (the default): the unrestricted loss."""

    def __init__(self, blank: int = 0, reduction: str = "mean", fastemit_lambda: float = 0.0):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"reduction must be mean|sum|none, got {reduction!r}")
        self.blank, self.reduction = int(blank), reduction
        self.fastemit_lambda = check_fastemit_lambda(fastemit_lambda)

    def forward(self, logits: torch.Tensor, targets: torch.Tensor, logit_lengths: torch.Tensor,
                target_lengths: torch.Tensor, emit_windows=None) -> torch.Tensor:
        if logits.dim() != 4:
            raise ValueError("logits must be (B, T, U+1, V)")
        nll = RnntLossFromLogitsFn.apply(logits, targets, logit_lengths, target_lengths, self.blank, self.fastemit_lambda,
                                         emit_windows)
        if self.reduction == "mean":
            return nll.mean()
        if self.reduction == "sum":
            return nll.sum()
        return nll


class CTCLoss(nn.Module):
    """CTC negative log-likelihood of `targets` given per-frame `logits` (raw, the log-softmax is fused), on the HIP kernels of
    csrc/ctc.hip: `loss(logits (B,T,V) fp32, targets (B,U) int32, logit_lengths (B,) int32, target_lengths (B,) int32)`.
    reduction "none" gives (B,); "sum" and "mean" are reductions over the BATCH, exactly like RNNTLoss here: "mean" is
    sum_b NLL_b / B.  It is NOT torch.nn.CTCLoss's "mean", which first divides each NLL by its target length.
    An utterance with fewer frames than its transcript needs (labels + adjacent repeats) has NLL +inf, or 0 with
    zero_infinity=True; its gradient row is exactly zero in both cases (torch gives NaN there).  U <= 511.  Same bits on every call."""

    def __init__(self, blank: int = 0, reduction: str = "mean", zero_infinity: bool = False):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"reduction must be mean|sum|none, got {reduction!r}")
        self.blank, self.reduction, self.zero_infinity = int(blank), reduction, bool(zero_infinity)

    def forward(self, logits: torch.Tensor, targets: torch.Tensor, logit_lengths: torch.Tensor,
                target_lengths: torch.Tensor) -> torch.Tensor:
        if logits.dim() != 3:
            raise ValueError("logits must be (B, T, V)")
        return CtcLossFn.apply(logits, targets, logit_lengths, target_lengths, self.blank, torch.is_grad_enabled(), self.reduction,
                               False, self.zero_infinity)


@torch.no_grad()
def rnnt_align(logits: torch.Tensor, targets: torch.Tensor, logit_lengths: torch.Tensor, target_lengths: torch.Tensor,
               blank: int = 0) -> Alignment:
    """Forced alignment on dense logits (B, T, U+1, V), arguments as RNNTLoss.forward: the best path of `targets` per utterance.
    Returns an ops.Alignment (`frames` (B,U) int32: the frame at which each label is emitted, -1 past target_lengths[b];
    `score` (B,) float64: the path's log-probability; `token_frames(b)`).  On exactly equal candidates blank wins."""
    if logits.dim() != 4:
        raise ValueError("logits must be (B, T, U+1, V)")
    return align_from_logits(logits, targets, logit_lengths, target_lengths, blank)
