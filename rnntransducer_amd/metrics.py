"""Word / character error rates of the validation side (model.py:7,41-42,94-95 use torchmetrics' WordErrorRate and
CharErrorRate, which is not a dependency here).  Same definition: sum of Levenshtein distances over sum of reference
lengths, words = str.split(), characters = every character of the string including spaces.  Host-side integer work on a few
hundred short strings per validation run: nothing to accelerate.  `token_error_rate` is the same ratio on token-id
sequences (what validation_step returns when no tokenizer is attached)."""
from typing import Iterable, Sequence, Union

import torch


def edit_distance(pred: Sequence, ref: Sequence) -> int:
    """Levenshtein distance (substitution = insertion = deletion = 1), two-row DP."""
    if len(pred) == 0:
        return len(ref)
    prev = list(range(len(ref) + 1))
    for i, p in enumerate(pred, 1):
        cur = [i] + [0] * len(ref)
        for j, r in enumerate(ref, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (p != r))
        prev = cur
    return prev[-1]


def _rate(pairs: Iterable) -> torch.Tensor:
    errors = total = 0
    for p, r in pairs:
        errors += edit_distance(p, r)
        total += len(r)
    return torch.tensor(errors / total if total else 0.0)


def _as_list(x: Union[str, Sequence[str]]):
    return [x] if isinstance(x, str) else list(x)


def word_error_rate(preds: Union[str, Sequence[str]], target: Union[str, Sequence[str]]) -> torch.Tensor:
    preds, target = _as_list(preds), _as_list(target)
    if len(preds) != len(target):
        raise ValueError("preds and target need the same number of sentences")
    return _rate((p.split(), t.split()) for p, t in zip(preds, target))


def char_error_rate(preds: Union[str, Sequence[str]], target: Union[str, Sequence[str]]) -> torch.Tensor:
    preds, target = _as_list(preds), _as_list(target)
    if len(preds) != len(target):
        raise ValueError("preds and target need the same number of sentences")
    return _rate((list(p), list(t)) for p, t in zip(preds, target))


def token_error_rate(preds: Sequence, target: Sequence) -> torch.Tensor:
    """Edit distance over reference length on token-id sequences (tensors or lists)."""
    to_list = lambda s: s.tolist() if isinstance(s, torch.Tensor) else list(s)  # noqa: E731
    return _rate((to_list(p), to_list(t)) for p, t in zip(preds, target))


def emission_delay(frames, ref_frames) -> dict:
    """How much later (+) or earlier (-) tokens are emitted than in a reference alignment, in frames.
    `frames`, `ref_frames`: two (B,U) integer frame tables padded with -1, as `Alignment.frames` (JointNet.align, loss.rnnt_align) and
    the searches' `return_frames` / `TimedTokens.frames` give them (tensors, arrays or nested lists; the narrower table is padded).
    Only positions that hold a frame (>= 0) in BOTH tables count.  Returns {"mean", "median", "p90", "count"} of
    frames - ref_frames over those positions (floats; p90 is the 90th percentile with linear interpolation; NaN when count = 0).
    Typical use: a model's own align() frames before and after fine-tuning with fastemit_lambda, or greedy token frames against an
    external alignment.  Host-side work on a few thousand integers."""
    to_t = lambda x: (x.detach().cpu() if isinstance(x, torch.Tensor) else torch.as_tensor(x)).to(torch.int64)  # noqa: E731
    a, r = to_t(frames), to_t(ref_frames)
    if a.dim() != 2 or r.dim() != 2 or a.size(0) != r.size(0):
        raise ValueError(f"frames and ref_frames must be (B,U) tables of the same B, got {tuple(a.shape)} and {tuple(r.shape)}")
    U = max(a.size(1), r.size(1))
    a = torch.nn.functional.pad(a, (0, U - a.size(1)), value=-1)
    r = torch.nn.functional.pad(r, (0, U - r.size(1)), value=-1)
    valid = (a >= 0) & (r >= 0)
    d = (a - r)[valid].to(torch.float64)
    n = int(d.numel())
    if n == 0:
        nan = float("nan")
        return {"mean": nan, "median": nan, "p90": nan, "count": 0}
    return {"mean": d.mean().item(), "median": torch.quantile(d, 0.5).item(), "p90": torch.quantile(d, 0.9).item(), "count": n}
