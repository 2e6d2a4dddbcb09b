"""JointNet — encoder + prediction net + joint, on the MI355X HIP path.

Mirrors networks/transducer.py:27-39 (ctor), :41-71 (joint), :73-93 (forward) of the reference: attributes
`encoder`, `decoder`, `fc` (Linear(O_e + O_d -> V), enc half first: transducer.py:64), GELU(tanh).

The reference's joint materialises (B,T,U+1,2*O) three times; here logits[b,t,u,:] = A[b,t,:] + C[b,u,:] + bias
with A = gelu(enc) W_e^T, C = gelu(dec) W_d^T (GELU is element-wise, fc is linear: SURVEY.md §0), so:
  * `loss(...)`  — fused joint + log-softmax + alpha/beta + gradient; (B,T,U+1,V) is never built;
  * `joint()/forward()` — still return the full logits tensor for callers that ask for it.
`recognize_greedy` (transducer.py:95-145) runs as ONE kernel launch (a workgroup per utterance, csrc/decode.hip) instead of
a host loop with a device sync per symbol.  `recognize_beams` (transducer.py:215-361, lm=None / hotwords=None) is one persistent
launch too (csrc/beam.hip): the reference's pop / expand / prune / stop decisions, with memoised prediction-net steps and a
prefix tree for y_star; LM and hotword rescoring over text (pyctcdecode / KenLM) stay out of scope, their mechanism is `fusion=`:
a weighted automaton over token ids (hotword boosting, token LM tables; rnntransducer_amd/fusion.py) that the same kernel walks.
`init_stream` / `recognize_greedy_stream` run the same greedy search over a batch of streams fed in chunks, with the encoder,
prediction-net and search state carried between chunks (rnntransducer_amd/streaming.py, csrc/stream.hip).
`init_beam_stream` / `recognize_beams_stream` do the same for the beam search: the whole hypothesis set is carried on the device
(csrc/beam_stream.hip, the offline kernel's frame loop), with the stable prefix of every stream exposed after each chunk.
`align` returns the best path of a known transcript (the frame at which every label is emitted, and the path's score) from the
fused loss's per-cell terms: the loss's lattice sweep in the (max, +) semiring (csrc/loss.hip).
`aux_ctc=True` adds `ctc_head`, a Linear(O_e -> V) on the encoder's output, for the auxiliary CTC loss of joint CTC + transducer
training (`loss(..., ctc_weight=w)`, `ctc_loss` for CTC pre-training of the encoder) and an encoder-only greedy decode
(`recognize_ctc_greedy`); csrc/ctc.hip.  Off by default: parameters, their initialisation and every result stay as without it.
`mwer_loss` is minimum word error rate fine-tuning: the reference term of `loss` plus the expected number of token errors over
the n-best list of the frame-synchronous search, with the hypotheses' losses from the fused loss over the shared encoder row
(csrc/mwer.hip, ops.JointLossGroupedFn).
`loss(..., ilmt_weight=w)` adds internal-LM training: w times the cross-entropy of the internal LM (the joint with the encoder half
zeroed, minus `ilm_score`) on the transcripts, from the joint's decoder half the fused loss already holds; `ilm_loss` is that term
alone on text, with no audio and no encoder call (csrc/ilm_loss.hip, ops.IlmLossFn).
`cell_logprobs` / `loss(..., kd_teacher=, kd_weight=w)` are lattice knowledge distillation: a teacher (any JointNet with the same
vocabulary: a bidirectional offline model for a streaming student) hands over three floats per lattice cell, and w times the
collapsed KL between its cells and the student's joins the loss, its gradient through the KD instances of the lattice gradient
kernels (csrc/loss.hip).
`ctc_align` is the forced alignment of a known transcript under the CTC head: per label the span of frames it holds on the best CTC
path, the path's score, on request the token per frame and per-label log-probabilities, from the encoder alone (csrc/ctc.hip,
DESIGN.md §28); `loss(..., emit_windows=ops.CtcEmitWindows(left, right))` feeds the alignment-restricted loss from it every step.
`ctc_skip=p` of `recognize_greedy` / `recognize_beams` / `recognize_beams_sync` / `mwer_loss` is CTC-guided blank-frame skipping:
the frames whose CTC blank posterior exceeds p are dropped in one pass on the device and the unchanged search runs on the rest,
its frames reported in the encoder's numbering (csrc/ctc_skip.hip, ops.ctc_frame_skip).
"""
import math

import torch
import torch.nn as nn

from ..ops import (MWER_MAX_LEN, CtcLossFn, IlmLossFn, JointLogitsFn, JointLossFn, JointLossGroupedFn, JointLossKdFn, MwerRiskFn,
                   TimedTokens, CtcEmitWindows, check_ctc_emit_windows, ctc_align, ctc_emit_windows, check_ctc_skip, ctc_frame_skip,
                   map_frames,
                   beam_search, beam_search_sync, beam_search_sync_device, check_beam_sync_args, check_ctc_beam_args,
                   check_emit_windows, check_fastemit_lambda, check_ilm_weight, check_ilmt_weight, check_kd_teacher, check_kd_weight,
                   refuse_ilm_weight,
                   check_fusion, ctc_beam_search, ctc_greedy, edit_distance, greedy_decode, nbest_pack, nbest_umax, stream_greedy)
from .decoder import TextPredNet
from .encoder import AudioTransNet, HipLinear, lengths_to_device
from .rnn import HipLSTM


class JointNet(nn.Module):
    def __init__(self, transnet_params: dict, prednet_params: dict, num_classes: int, aux_ctc: bool = False):
        super().__init__()
        self.encoder = AudioTransNet(**transnet_params)
        self.decoder = TextPredNet(**prednet_params)
        self.num_classes = num_classes
        self.enc_out = transnet_params["output_size"]
        self.dec_out = prednet_params["output_size"]
        # parameter container only: fc is applied inside the fused kernels (A/C pre-GEMMs), never as one Linear
        self.fc = HipLinear(self.enc_out + self.dec_out, num_classes)
        # created LAST: under a given seed every other parameter initialises to the same bits as without the head
        self.aux_ctc = bool(aux_ctc)
        if self.aux_ctc:
            self.ctc_head = HipLinear(self.enc_out, num_classes)

    def _need_ctc_head(self, what: str) -> None:
        if not self.aux_ctc:
            raise ValueError(f"{what} needs the CTC head: build the JointNet with aux_ctc=True (jointnet_params['aux_ctc'])")

    def _check_ctc_skip(self, ctc_skip, blank, what: str, visit_padded_frames: bool = False) -> None:
        """The argument checks of `ctc_skip=p` (not None), before anything runs: p a probability in (0, 1], the CTC head present,
        the blank inside the vocabulary, and no visit_padded_frames (a skipped utterance has no padded frames to visit)."""
        check_ctc_skip(ctc_skip, what)
        self._need_ctc_head(f"{what}(ctc_skip=)")
        if visit_padded_frames:
            raise ValueError(f"{what}: visit_padded_frames=True cannot be combined with ctc_skip (the compacted rows behind an "
                             "utterance's kept frames hold nothing)")
        if isinstance(blank, bool) or not 0 <= int(blank) < self.num_classes:
            raise ValueError(f"{what}: blank {blank!r} outside [0,{self.num_classes})")

    def _skip_blank_frames(self, enc, t_lens, blank, ctc_skip):
        """ctc_skip=p of the searches: ctc_head(enc) once, then ops.ctc_frame_skip -> FrameSkip(enc, t_lens,
        frame_map): the search's operands and the table that turns its frames back into encoder frames.  No graph, no host sync."""
        with torch.no_grad():
            enc = enc.detach()
            return ctc_frame_skip(self.ctc_head(enc), t_lens, int(blank), ctc_skip, enc)

    def search_weights(self, fc_bias: bool = True) -> tuple:
        """The prediction-net / joint weights in the order the ops searches take them: fc.weight, fc.bias, the embedding, the
        prediction net's flat weights and cell, out_proj's weight and bias.  fc_bias=False: without fc.bias, as the streaming
        entries take them (their encoder step has added it)."""
        dec = self.decoder
        return (self.fc.weight, *((self.fc.bias,) if fc_bias else ()), dec.embedding.weight, dec.rnn.flat_weights(), dec.rnn.CELL,
                dec.out_proj.weight, dec.out_proj.bias)

    def _search_encoder(self, inputs, inputs_lengths, blank, ctc_skip):
        """The prologue of the offline searches, behind their argument checks: lengths to the device, the encoder, and with
        ctc_skip the blank frames dropped.  -> (the search's encoder output, its t_lens, the FrameSkip record or None)"""
        t_lens = lengths_to_device(inputs_lengths, inputs.device)
        enc = self.encoder.forward_time_major(inputs, t_lens)
        if ctc_skip is None:
            return enc, t_lens, None
        skip = self._skip_blank_frames(enc, t_lens, blank, ctc_skip)
        return skip.enc, skip.t_lens, skip

    def _nbest_lists(self, res, skip, return_scores: bool, return_frames: bool):
        """The beam searches' host lists (an entry is (y, score[, fused_score][, frames])) as recognize_beams and
        recognize_beams_sync return them: frames back in the encoder's numbering after a skip, frames second in an entry,
        scores on request, the list itself for a single utterance."""
        if skip is not None and return_frames:
            res = self._original_frames(res, skip.frame_map)
        if return_frames:
            outs = [[(e[0], e[-1], *e[1:-1]) if return_scores else (e[0], e[-1]) for e in hyps] for hyps in res]
        else:
            outs = [hyps if return_scores else [e[0] for e in hyps] for hyps in res]
        return outs[0] if len(outs) == 1 else outs

    def _stream_encoder(self, chunk, lens, T_run: int, state):
        """The encoder step of the three streaming searches over the first T_run = max(lens) frames of a chunk, in place on the
        state's encoder rows.  -> (A (T_run, B, V), the encoder half of the joint; lens on the device, int32: one copy, shared by
        the encoder's and the search's launches)"""
        B = chunk.shape[0]
        lens_dev = torch.tensor(lens, dtype=torch.int32, device=chunk.device)
        enc = torch.empty(T_run, B, self.enc_out, device=chunk.device)
        A = self.encoder.stream_chunk(chunk, lens_dev, T_run, state.enc_h, state.enc_c, enc, (self.enc_out, B * self.enc_out),
                                      (self.fc.weight, self.fc.bias))
        return A, lens_dev

    @staticmethod
    def _original_frames(res, frame_map):
        """The beam searches' host lists (entries end in `frames`) with every frame >= 0 mapped through frame_map (B, T): one
        host copy, behind the search's own."""
        fm = frame_map.cpu().tolist()
        return [[(*e[:-1], [f if f < 0 else fm[b][f] for f in e[-1]]) for e in hyps] for b, hyps in enumerate(res)]

    @staticmethod
    def _ragged_rows(audio_lengths, T, B, dev, t_lens, u_lens, rows, want_inv):
        """The ragged handling of loss(): with the collate's python list of frame counts, rows sorted by descending length (the
        per-row tensors `rows` and both length tensors follow) and an ops.RaggedPlan for the encoder; `inv` restores the
        caller's row order.  -> rows, t_lens, u_lens, enc_lens, inv"""
        enc_lens, inv = t_lens, None
        if audio_lengths is not None and len(audio_lengths) == B and B > 1 and min(audio_lengths) < T:
            from ..ops import RaggedPlan
            host = [int(n) for n in audio_lengths]
            order = sorted(range(B), key=lambda b: (-host[b], b))
            if order != list(range(B)):   # length-sorted rows (encoder.py:94-96); the small per-utterance tensors follow, nll is un-sorted below
                perm = torch.tensor(order, dtype=torch.int64, device=dev)
                rows = tuple(x.index_select(0, perm) for x in rows)
                t_lens, u_lens = t_lens.index_select(0, perm), u_lens.index_select(0, perm)
                host = [host[b] for b in order]
                if want_inv:
                    inv = torch.empty_like(perm)
                    inv[perm] = torch.arange(B, dtype=torch.int64, device=dev)
            enc_lens = RaggedPlan(host, T, dev)
        return rows, t_lens, u_lens, enc_lens, inv

    def set_compute_precision(self, p: str):
        """"fp32" | "fp16" for every recurrent stack below this module (HipLSTM.compute_precision); returns self."""
        for m in self.modules():
            if isinstance(m, HipLSTM):
                m.compute_precision = p
        return self

    def joint(self, encoder_outputs: torch.Tensor, decoder_outputs: torch.Tensor) -> torch.Tensor:
        """(B,T,O_e), (B,U+1,O_d) -> logits (B,T,U+1,V) (materialising; transducer.py:54-69).  1-D inputs (one encoder frame,
        one prediction-net output: the search loops' call at transducer.py:125,309) -> logits (V,)."""
        if encoder_outputs.dim() == 1 and decoder_outputs.dim() == 1:
            from ..ops import LinearFn
            z = torch.cat((encoder_outputs, decoder_outputs)).unsqueeze(0)
            return LinearFn.apply(torch.nn.functional.gelu(z, approximate="tanh"), self.fc.weight, self.fc.bias).squeeze(0)
        if encoder_outputs.dim() != 3 or decoder_outputs.dim() != 3:
            raise ValueError("joint takes (B,T,O) with (B,U+1,O), or two 1-D vectors")
        return JointLogitsFn.apply(encoder_outputs.transpose(0, 1).contiguous(),
                                   decoder_outputs.transpose(0, 1).contiguous(), self.fc.weight, self.fc.bias)

    def forward(self, input_audios, audio_lengths, input_texts, text_lengths) -> torch.Tensor:
        dev = input_audios.device
        enc = self.encoder.forward_time_major(input_audios, lengths_to_device(audio_lengths, dev))
        dec = self.decoder.forward_time_major(input_texts, lengths_to_device(text_lengths, dev))
        return JointLogitsFn.apply(enc, dec, self.fc.weight, self.fc.bias)

    def loss(self, input_audios, tensor_audio_lengths, input_texts, targets, target_lengths, blank: int,
             reduction: str = "none", audio_lengths=None, ctc_weight: float = 0.0, return_parts: bool = False,
             fastemit_lambda: float = 0.0, emit_windows=None, ilmt_weight: float = 0.0, kd_teacher=None, kd_weight: float = 0.0):
        """-log P(y|x) through the fused path (no (B,T,U+1,V) tensor): per utterance, shape (B,) (reduction "none"), or the 0-d
        "mean" / "sum" over the batch (model.py:39 builds the reference's loss with reduction="mean").
        `audio_lengths`: the python list of frame counts the reference's collate hands over next to the tensor (dataloader.py:20,49).
        With it a ragged batch is handled as the reference handles it (networks/encoder.py:93-96: sort by length, pack): rows are
        sorted by descending length so that the recurrences' sync groups are length-homogeneous, and a valid-frame table lets the
        big products and the recurrences skip the padding (ops.RaggedPlan) — all planned on the host, no device synchronisation.
        Results do not depend on it.
        `ctc_weight` != 0 (aux_ctc=True only): the result is rnnt + ctc_weight * ctc under the same reduction, the CTC term
        being the CTC loss of `targets` on ctc_head(encoder output); ONE encoder forward feeds both.  return_parts=True returns
        (total, rnnt, ctc); with ctc_weight = 0 the CTC part is then computed without a graph and total is the RNN-T loss.
        With ctc_weight = 0 and return_parts=False the head is not touched: same bits as a model without it.
        `fastemit_lambda` > 0: FastEmit regularisation of the transducer term's GRADIENT (label log-probability gradients scaled by
        1 + lambda, through the log-softmax exactly: include/rnnt_hip.h), which trains the model to emit sooner.  The returned value
        stays the unregularised loss, bit for bit that of lambda = 0; the CTC term is untouched.  Finite and >= 0.
        `emit_windows` = (lo, hi), two (B, U) int32 tensors in the CALLER's row order (they follow their rows through the ragged
        sort): the alignment-restricted transducer term, label u of row b only at frames lo[b,u] .. hi[b,u] (ops.emit_windows builds
        them around a reference alignment; include/rnnt_hip.h).  A row whose windows leave no path has loss +inf and a zero gradient.
        The CTC term is untouched.  None: the unrestricted loss.
        `emit_windows` = ops.CtcEmitWindows(left, right) (aux_ctc=True only): the windows come from the model's own CTC head.  After
        the one encoder forward, ctc_head(encoder output) is computed once (shared with the CTC term when that is on), its detached
        values are aligned to `targets` without a graph (ops.ctc_align), and label u may be emitted at frames first[u] - left ..
        last[u] + right of the head's best path; a row without a CTC path gets the full window.  No host sync, no second encoder
        call.  This cannot produce +inf on a row that has a CTC path: there first[u] <= last[u] < first[u+1], so the transducer
        path that emits label u at frame first[u] is monotone, inside every window and inside [0, T_b).
        `ilmt_weight` > 0: internal-LM training (ILMT): the result is rnnt + ctc_weight * ctc + ilmt_weight * ilm,
        ilm being the cross-entropy of the internal LM (the joint with the encoder half zeroed, over the non-blank tokens: minus
        `ilm_score`) on `targets`, a per-utterance sum over tokens under the same reduction.  It costs one launch in the forward and
        one in the backward on the joint's decoder half the loss already holds; the encoder gets no gradient from it.  FastEmit,
        the windows and the CTC term do not touch it.  A counted target that is the blank gives that row +inf and a zero gradient
        of the term.  With return_parts=True the tuple gains a last element: (total, rnnt, ctc, ilm).  Finite and >= 0; at 0 the
        term is not computed and every result is bitwise that of a call without the argument.
        `kd_teacher` (an ops.CellLogProbs: a teacher's `cell_logprobs` on THIS batch, rows in the caller's order -- they follow their
        rows through the ragged sort) with `kd_weight` > 0: lattice knowledge distillation.  The result is rnnt +
        ctc_weight * ctc + ilmt_weight * ilm + kd_weight * kd, kd being per utterance the sum over its lattice cells of the KL
        divergence between the teacher's and this model's distributions collapsed to (blank, the cell's label, everything else),
        under the same reduction.  One small launch in the forward; the gradient comes out of the lattice gradient kernels' KD
        instances with the transducer term's, FastEmit included.  With return_parts=True the tuple gains a last element, kd.
        ValueError for a teacher next to emit_windows, planes that are not (B, U+1, T) float32 on the inputs' device, or fewer than 3
        classes.  Finite and >= 0; at 0, or without a teacher, nothing of it runs and every result is bitwise that of a call without
        the arguments."""
        return self._reference_terms(input_audios, tensor_audio_lengths, input_texts, targets, target_lengths, blank, reduction,
                                     audio_lengths, ctc_weight, return_parts, fastemit_lambda, emit_windows=emit_windows,
                                     ilmt_weight=ilmt_weight, kd_teacher=kd_teacher, kd_weight=kd_weight)[0]

    def _reference_terms(self, input_audios, tensor_audio_lengths, input_texts, targets, target_lengths, blank, reduction,
                         audio_lengths, ctc_weight, return_parts, fastemit_lambda, want_inv=False, emit_windows=None,
                         ilmt_weight=0.0, kd_teacher=None, kd_weight=0.0):
        """The body of loss(): -> (what loss() returns, (enc, targets, t_lens, u_lens, inv)) with the encoder output and the
        per-row tensors in the row order the encoder ran in (length-sorted for a ragged batch; `inv` restores the caller's order,
        None when nothing moved or nobody needs it).  mwer_loss builds its hypothesis term on the same encoder output."""
        ilmt_weight = check_ilmt_weight(ilmt_weight)
        with_ctc = ctc_weight != 0.0 or return_parts
        if with_ctc:
            self._need_ctc_head("loss(ctc_weight != 0 or return_parts=True)")
        dev = input_audios.device
        t_lens = lengths_to_device(tensor_audio_lengths, dev)
        u_lens = lengths_to_device(target_lengths, dev)
        T, B = input_audios.size(1), input_audios.size(0)
        ctc_win = None
        if isinstance(emit_windows, CtcEmitWindows):   # windows from the CTC head's own alignment, built below on the encoder output
            self._need_ctc_head("loss(emit_windows=CtcEmitWindows(...))")
            ctc_win = check_ctc_emit_windows(emit_windows)
        win = None if ctc_win is not None else check_emit_windows(emit_windows, B, targets.size(1), dev)
        kd_weight = check_kd_weight(kd_weight)
        teacher = check_kd_teacher(kd_teacher, B, targets.size(1) + 1, T, self.num_classes, dev, emit_windows)
        if kd_weight == 0.0:
            teacher = None
        # the windows, and a teacher's planes, are sorted with their rows
        rows = (input_audios, input_texts, targets) + (() if win is None else (win[0], win[1])) + (() if teacher is None else tuple(teacher))
        rows, t_lens, u_lens, enc_lens, inv = self._ragged_rows(audio_lengths, T, B, dev, t_lens, u_lens, rows,
                                                                reduction == "none" or want_inv)
        input_audios, input_texts, targets = rows[:3]
        enc = self.encoder.forward_time_major(input_audios, enc_lens)
        dec = self.decoder.forward_time_major(input_texts, u_lens + 1)  # text length = label length + 1 (dataloader.py:39-40)
        ilm = kd = None
        track = ctc_weight != 0.0 and torch.is_grad_enabled()
        head, win_pair = None, (None if win is None else (rows[3], rows[4]))
        if ctc_win is not None:   # ONE ctc_head(enc), shared with the CTC term; its detached values are aligned without a graph
            with torch.set_grad_enabled(track):
                head = self.ctc_head(enc)
            win_pair = ctc_emit_windows(head, targets, t_lens, u_lens, blank, ctc_win)
        if teacher is not None:
            outs = JointLossKdFn.apply(enc, dec, self.fc.weight, self.fc.bias, targets, t_lens, u_lens, blank, torch.is_grad_enabled(),
                                     reduction, fastemit_lambda, None, ilmt_weight, rows[-3:], kd_weight)
            out, kd = outs[0], outs[-1]
            ilm = outs[1] if ilmt_weight > 0.0 else None
        elif ilmt_weight > 0.0:
            out, ilm = JointLossFn.apply(enc, dec, self.fc.weight, self.fc.bias, targets, t_lens, u_lens, blank, torch.is_grad_enabled(),
                                         reduction, fastemit_lambda, win_pair, ilmt_weight)
        elif win_pair is None:
            out = JointLossFn.apply(enc, dec, self.fc.weight, self.fc.bias, targets, t_lens, u_lens, blank, torch.is_grad_enabled(),
                                    reduction, fastemit_lambda)
        else:
            out = JointLossFn.apply(enc, dec, self.fc.weight, self.fc.bias, targets, t_lens, u_lens, blank, torch.is_grad_enabled(),
                                    reduction, fastemit_lambda, win_pair)
        unsort = inv is not None and reduction == "none"
        shared = (enc, targets, t_lens, u_lens, inv)
        out = out.index_select(0, inv) if unsort else out
        if ilm is not None:
            ilm = ilm.index_select(0, inv) if unsort else ilm
        if kd is not None:
            kd = kd.index_select(0, inv) if unsort else kd
        if not with_ctc:
            total = out if ilm is None else out + ilmt_weight * ilm
            return (total if kd is None else total + kd_weight * kd), shared
        with torch.set_grad_enabled(track):
            ctc = CtcLossFn.apply(self.ctc_head(enc) if head is None else head, targets, t_lens, u_lens, blank, track, reduction, True)
        ctc = ctc.index_select(0, inv) if unsort else ctc
        total = out + ctc_weight * ctc if ctc_weight != 0.0 else out
        if ilm is not None:
            total = total + ilmt_weight * ilm
        if kd is not None:
            total = total + kd_weight * kd
        parts = (total, out, ctc) + (() if ilm is None else (ilm,)) + (() if kd is None else (kd,))
        return (parts if return_parts else total), shared

    def ilm_loss(self, input_texts, targets, target_lengths, blank: int, reduction: str = "none") -> torch.Tensor:
        """The internal-LM term alone, on text (text-only internal-LM adaptation): no audio and no encoder call.
        input_texts (B, U+1) int64 (the blank, then the tokens, as `loss` takes them), targets (B, U) int32, target_lengths B
        values in [0, U] -> per utterance the cross-entropy of the internal LM on the targets, summed over tokens (shape (B,)),
        or its "mean" / "sum" over the batch.  The prediction net, fc.weight[:, enc_out:] and fc.bias receive gradients; the
        encoder's parameters receive none and fc.weight[:, :enc_out] exact zeros.  Freeze the encoder (requires_grad_(False))
        BEFORE building the optimizer for text-only adaptation: a decoupled weight decay still moves a parameter whose gradient
        is zero.  In eval() under torch.no_grad() this is -ilm_score(targets, target_lengths, blank) in fp32: the internal LM's
        perplexity on a text is exp(ilm_loss / length), computed on the device.  A counted target that is the blank or outside
        the vocabulary gives that row +inf and a zero gradient (no host check: it would cost a synchronisation)."""
        if reduction not in ("none", "mean", "sum"):
            raise ValueError(f"ilm_loss: reduction must be 'none', 'mean' or 'sum', got {reduction!r}")
        if not 0 <= int(blank) < self.num_classes:
            raise ValueError(f"ilm_loss: blank {blank} outside [0,{self.num_classes})")
        if input_texts.dim() != 2 or targets.dim() != 2 or tuple(input_texts.shape) != (targets.size(0), targets.size(1) + 1):
            raise ValueError(f"ilm_loss: input_texts must be (B, U+1) and targets (B, U), got {tuple(input_texts.shape)} and "
                             f"{tuple(targets.shape)}")
        u_lens = lengths_to_device(target_lengths, input_texts.device)
        dec = self.decoder.forward_time_major(input_texts, u_lens + 1)  # text length = label length + 1, as in loss()
        return IlmLossFn.apply(dec, self.fc.weight, self.fc.bias, targets, u_lens, int(blank), torch.is_grad_enabled(), reduction)

    def ctc_loss(self, input_audios, tensor_audio_lengths, targets, target_lengths, blank: int, reduction: str = "none",
                 audio_lengths=None) -> torch.Tensor:
        """The CTC term alone (CTC pre-training of the encoder): the CTC loss of `targets` on ctc_head(encoder output); the
        prediction net and the joint are not run.  Arguments, reductions and the ragged handling as in `loss`."""
        self._need_ctc_head("ctc_loss")
        dev = input_audios.device
        t_lens = lengths_to_device(tensor_audio_lengths, dev)
        u_lens = lengths_to_device(target_lengths, dev)
        T, B = input_audios.size(1), input_audios.size(0)
        (input_audios, targets), t_lens, u_lens, enc_lens, inv = self._ragged_rows(
            audio_lengths, T, B, dev, t_lens, u_lens, (input_audios, targets), reduction == "none")
        enc = self.encoder.forward_time_major(input_audios, enc_lens)
        out = CtcLossFn.apply(self.ctc_head(enc), targets, t_lens, u_lens, blank, torch.is_grad_enabled(), reduction, True)
        return out if inv is None else out.index_select(0, inv)

    @torch.no_grad()
    def ctc_align(self, input_audios, tensor_audio_lengths, targets, target_lengths, blank: int, audio_lengths=None,
                  return_path: bool = False, return_token_logp: bool = False):
        """CTC forced alignment through the CTC head (csrc/ctc.hip): the best CTC path of the KNOWN transcript
        `targets` per utterance on ctc_head(encoder output); the prediction net and the joint are not run and no (T, U) lattice is
        built, so this works with bidirectional encoders and before the transducer is trained.  Arguments and the ragged handling
        as in `ctc_loss`; results come back in the caller's row order.  Returns an ops.CtcAlignment: `first`, `last` (B,U) int32,
        the first and last encoder frame each label's state holds on the best path (-1 past target_lengths[b] and in a row
        without a path), `score` (B,) float64 (-inf without a path), and on request `path` (B,T) int32 (the token per frame, the
        blank in blank states, -1 past the row's frames) and `token_logp` (B,U) float64 (per label the sum of its
        log-probabilities over its span).  No host sync."""
        self._need_ctc_head("ctc_align")
        dev = input_audios.device
        t_lens = lengths_to_device(tensor_audio_lengths, dev)
        u_lens = lengths_to_device(target_lengths, dev)
        T, B = input_audios.size(1), input_audios.size(0)
        (input_audios, targets), t_lens, u_lens, enc_lens, inv = self._ragged_rows(
            audio_lengths, T, B, dev, t_lens, u_lens, (input_audios, targets), True)
        enc = self.encoder.forward_time_major(input_audios, enc_lens)
        res = ctc_align(self.ctc_head(enc), targets, t_lens, u_lens, blank, time_major=True, return_path=return_path,
                        return_token_logp=return_token_logp)
        if inv is None:
            return res
        return type(res)(*(None if x is None else x.index_select(0, inv) for x in res))

    @staticmethod
    def check_mwer_args(nbest, max_symbols, token_min_logp, max_hyp_len, mwer_weight, what: str) -> float:
        """ValueError unless 1 <= nbest <= 64, 1 <= max_symbols <= 4, 1 <= max_hyp_len <= 511, token_min_logp is a number below
        +inf and mwer_weight is finite and >= 0; -> mwer_weight as a float."""
        check_beam_sync_args(nbest, max_symbols, token_min_logp, what)
        if isinstance(max_hyp_len, bool) or not isinstance(max_hyp_len, int) or not 1 <= max_hyp_len <= MWER_MAX_LEN:
            raise ValueError(f"{what}: max_hyp_len must be an integer in [1, {MWER_MAX_LEN}], got {max_hyp_len!r}")
        if isinstance(mwer_weight, bool) or not isinstance(mwer_weight, (int, float)) or not math.isfinite(mwer_weight) \
                or mwer_weight < 0:
            raise ValueError(f"{what}: mwer_weight must be finite and >= 0, got {mwer_weight!r}")
        return float(mwer_weight)

    def mwer_loss(self, input_audios, tensor_audio_lengths, input_texts, targets, target_lengths, blank: int, *, nbest: int = 4,
                  max_symbols: int = 1, token_min_logp: float = -math.inf, max_hyp_len: int = MWER_MAX_LEN,
                  mwer_weight: float = 1.0, reduction: str = "mean", audio_lengths=None, ctc_weight: float = 0.0,
                  fastemit_lambda: float = 0.0, return_parts: bool = False, ctc_skip=None):
        """Minimum word error rate fine-tuning: rnnt + ctc_weight * ctc + mwer_weight * risk, where risk is the
        expected number of TOKEN errors over the model's own n-best list, relative to the list's mean:
            risk_b = sum_i P^_i (W_i - mean W),   P^_i = softmax_i(-nll_i)   over the valid hypotheses i of utterance b,
        nll_i = -log P(y_i | x) from the fused loss (the full lattice sum, not the search's score) and W_i the Levenshtein
        distance between y_i and the transcript, on token ids.  Per step:
          1. ONE encoder forward in the module's current mode (it feeds every term);
          2. the frame-synchronous search (recognize_beams_sync's kernel: nbest <= 64 hypotheses, max_symbols <= 4, token_min_logp)
             on the detached encoder output, without a graph.  The hypotheses therefore come from the TRAIN-mode encoder output
             (dropout active if the module is in train()); the search itself never applies dropout to the prediction net;
          3. the reference term exactly as loss() computes it (same code: ragged handling, ctc_weight, fastemit_lambda);
          4. the prediction net on the packed hypotheses, the fused loss for the nbest rows of each utterance over its one encoder
             row (ops.JointLossGroupedFn; FastEmit does not apply to them), the edit distances and the risk, all on the device.
        No emission windows (loss()'s emit_windows): the rows of the risk term are hypotheses and have no reference alignment.
        A hypothesis longer than max_hyp_len (<= 511) tokens is left out, as are the ranks the search did not fill; an utterance
        with fewer than two valid hypotheses has risk 0.  No host sync beyond the search's one copy of counts and lengths.
        ctc_skip=p (needs the CTC head): the n-best search alone runs on the frames whose CTC blank posterior
        (the head on the detached encoder output, without a graph) is at most p; every loss term stays on all frames.
        reduction: "none" (B,), "mean" or "sum" over B, for every term.  return_parts=True -> (total, rnnt[, ctc], risk,
        err1) with ctc present when the module has the CTC head, err1 the mean edit distance of the 1-best hypotheses (fp32, 0-d).
        ValueError for bad arguments before anything runs."""
        what = "mwer_loss"
        mwer_weight = self.check_mwer_args(nbest, max_symbols, token_min_logp, max_hyp_len, mwer_weight, what)
        check_fastemit_lambda(fastemit_lambda)
        if reduction not in ("none", "mean", "sum"):
            raise ValueError(f"{what}: reduction must be 'none', 'mean' or 'sum', got {reduction!r}")
        if not 0 <= int(blank) < self.num_classes:
            raise ValueError(f"{what}: blank {blank} outside [0,{self.num_classes})")
        if ctc_skip is not None:
            self._check_ctc_skip(ctc_skip, blank, what)
        parts = return_parts and self.aux_ctc
        ref, (enc, targets, t_lens, u_lens, inv) = self._reference_terms(
            input_audios, tensor_audio_lengths, input_texts, targets, target_lengths, blank, reduction, audio_lengths, ctc_weight,
            parts, fastemit_lambda, want_inv=True)
        dec, B, N = self.decoder, enc.shape[1], nbest
        s_enc, s_lens = enc.detach(), t_lens
        if ctc_skip is not None:   # the search alone sees the kept frames; nbest_pack and the losses below keep the originals
            s_enc, s_lens = self._skip_blank_frames(enc, t_lens, blank, ctc_skip)[:2]
        tokens, lens, counts, _, host = beam_search_sync_device(s_enc, *self.search_weights(), int(blank), N, max_symbols, s_lens,
                                                                token_min_logp=token_min_logp)
        texts, labels, hu_lens, ht_lens, valid = nbest_pack(tokens, lens, counts, t_lens, nbest_umax(host, B, N, max_hyp_len),
                                                            int(blank), max_hyp_len)
        hdec = dec.forward_time_major(texts, hu_lens + 1)
        nll = JointLossGroupedFn.apply(enc, hdec, self.fc.weight, self.fc.bias, labels, ht_lens, hu_lens, int(blank), N,
                                       torch.is_grad_enabled())
        dist = edit_distance(labels, hu_lens, targets, u_lens, N)
        if inv is not None and reduction == "none":   # the caller's row order, as the reference terms come back
            rows = (inv.unsqueeze(1) * N + torch.arange(N, device=inv.device)).reshape(-1)
            nll, dist, valid = nll.index_select(0, rows), dist.index_select(0, rows), valid.index_select(0, rows)
        risk = MwerRiskFn.apply(nll, dist, valid, N, reduction)
        total = (ref[0] if parts else ref) + mwer_weight * risk
        if not return_parts:
            return total
        err1 = dist.view(B, N)[:, 0].to(torch.float32).mean()
        return (total, *ref[1:], risk, err1) if parts else (total, ref, risk, err1)

    @torch.no_grad()
    def recognize_ctc_greedy(self, inputs: torch.Tensor, inputs_lengths, blank_token_id: int, return_frames: bool = False):
        """Encoder-only greedy decode through the CTC head: per frame the argmax of ctc_head(encoder output) (ties to the lowest
        index), repeats collapsed, blanks dropped; one launch and one host sync (csrc/ctc.hip).  Returns a list of B 1-D
        LongTensors; with return_frames a list of (tokens, frames) pairs, frames int32: the encoder frame at which each token's
        run starts.  Works with bidirectional encoders.  eval() mode only, like recognize_greedy."""
        self._need_ctc_head("recognize_ctc_greedy")
        if self.training:
            raise RuntimeError("recognize_ctc_greedy expects eval() mode (dropout inactive), like recognize_greedy")
        t_lens = lengths_to_device(inputs_lengths, inputs.device)
        enc = self.encoder.forward_time_major(inputs, t_lens)
        return ctc_greedy(self.ctc_head(enc), t_lens, blank_token_id, time_major=True, return_frames=return_frames)

    @torch.no_grad()
    def recognize_ctc_beams(self, inputs: torch.Tensor, inputs_lengths, blank_token_id: int, beam_widths: int = 16, *,
                            token_min_logp: float = -math.inf, fusion=None, return_scores: bool = False,
                            return_frames: bool = False, ilm_weight=None):
        """Encoder-only CTC prefix beam search through the CTC head (csrc/ctc_beam.hip): up to `beam_widths`
        (<= 128) token lists per utterance (no blanks, no leading blank), best first by the CTC log-probability mass the search
        kept for each labelling; no length normalisation.  The prediction net is not run, so this works before it is trained
        and with bidirectional encoders.  For a single utterance the list itself, otherwise one list per utterance (as
        recognize_beams).  token_min_logp: per frame only tokens whose log-softmax reaches it extend a prefix (-inf: all).
        return_scores: (tokens, score) pairs, score fp64.  return_frames: frames is appended last, per token the encoder frame
        at which its prefix first entered the beam.
        fusion (a TokenFusion or an NgramFusion on the model's device, used as it is): the search ranks by score + the automaton's
        total, the output by score + total + final; with return_scores the entries are (tokens, score, fused_score).  A CTC hypothesis has
        no leading blank: its totals are fusion.score([blank] + tokens).  Limitation: TokenFusion.from_hotwords refuses a phrase
        that repeats a token back to back (the transducer's y_star never holds one), although a CTC hypothesis can.
        ilm_weight: refused with a ValueError: no prediction net runs here, so there is no internal LM to subtract.
        eval() mode only; ValueError for a missing head, training mode or bad arguments, before anything is launched."""
        refuse_ilm_weight(ilm_weight, "recognize_ctc_beams", "the CTC search runs no prediction net: there is no internal LM")
        self._need_ctc_head("recognize_ctc_beams")
        if self.training:
            raise ValueError("recognize_ctc_beams expects eval() mode (dropout inactive), like recognize_ctc_greedy")
        check_ctc_beam_args(beam_widths, token_min_logp, "recognize_ctc_beams")
        check_fusion(fusion, self.num_classes, self.ctc_head.weight.device, "recognize_ctc_beams", ngram=True)
        t_lens = lengths_to_device(inputs_lengths, inputs.device)
        enc = self.encoder.forward_time_major(inputs, t_lens)
        res = ctc_beam_search(self.ctc_head(enc), t_lens, blank_token_id, beam_widths, token_min_logp=token_min_logp,
                              time_major=True, fusion=fusion, return_frames=return_frames)
        if not return_scores:   # an entry is (tokens, score[, fused_score][, frames])
            res = [[(e[0], e[-1]) if return_frames else e[0] for e in hyps] for hyps in res]
        return res[0] if len(res) == 1 else res

    @torch.no_grad()
    def align(self, input_audios, tensor_audio_lengths, input_texts, targets, target_lengths, blank: int, audio_lengths=None):
        """Forced alignment: the best RNN-T path of the KNOWN transcript `targets` per utterance (csrc/loss.hip: the loss's
        log-softmax kernels, then its lattice sweep in the (max, +) semiring with one back-pointer bit per cell; no (B,T,U+1,V)
        tensor).  Arguments as `loss`, with the same ragged handling under `audio_lengths` (results come back in the caller's row
        order).  Returns an ops.Alignment: `frames` (B,U) int32 — the frame at which each label is emitted, -1 past
        target_lengths[b] —, `score` (B,) float64 — the log-probability of that path, <= -loss —, and `token_frames(b)`, the
        un-padded list of one utterance after one host copy.  Frames count encoder output frames.  On exactly equal candidates
        the path stays on a frame (blank) rather than emit.  eval() mode only, like recognize_greedy."""
        from ..ops import Alignment, _joint_ac, _need_gpu, joint_align
        if self.training:
            raise RuntimeError("align expects eval() mode (dropout inactive), like recognize_greedy")
        _need_gpu(input_audios, input_texts, targets)
        dev = input_audios.device
        t_lens = lengths_to_device(tensor_audio_lengths, dev)
        u_lens = lengths_to_device(target_lengths, dev)
        T, B = input_audios.size(1), input_audios.size(0)
        (input_audios, input_texts, targets), t_lens, u_lens, enc_lens, inv = self._ragged_rows(
            audio_lengths, T, B, dev, t_lens, u_lens, (input_audios, input_texts, targets), True)   # frames and scores are un-sorted below
        enc = self.encoder.forward_time_major(input_audios, enc_lens)
        dec = self.decoder.forward_time_major(input_texts, u_lens + 1)
        A, Cm = _joint_ac(enc, dec, self.fc.weight, self.enc_out, self.dec_out, self.num_classes)
        res = joint_align(A, Cm, self.fc.bias, targets, t_lens, u_lens, blank)
        if inv is None:
            return res
        return Alignment(res.frames.index_select(0, inv), res.score.index_select(0, inv), u_lens.index_select(0, inv))

    @torch.no_grad()
    def cell_logprobs(self, input_audios, tensor_audio_lengths, input_texts, targets, target_lengths, blank: int, audio_lengths=None):
        """The teacher's side of lattice knowledge distillation: this model's distribution in every lattice cell of
        the batch, collapsed to (blank, the cell's label, everything else).  Arguments as `loss`, with the same ragged handling
        under `audio_lengths`.  Returns an ops.CellLogProbs of three (B, U+1, T) fp32 planes in the caller's row order, for another
        model's `loss(..., kd_teacher=)` on the same batch: the encoder, the prediction net, the joint's two small products and one
        launch; no lattice sweep, no (B,T,U+1,V) tensor, no graph.  Any encoder will do (a bidirectional one for a streaming
        student); the vocabulary and the blank must be the student's.  eval() mode only, like align."""
        from ..ops import CellLogProbs, joint_cell_logprobs, _need_gpu
        if self.training:
            raise RuntimeError("cell_logprobs expects eval() mode (dropout inactive), like align")
        if not 0 <= int(blank) < self.num_classes:
            raise ValueError(f"cell_logprobs: blank {blank} outside [0,{self.num_classes})")
        _need_gpu(input_audios, input_texts, targets)
        dev = input_audios.device
        t_lens = lengths_to_device(tensor_audio_lengths, dev)
        u_lens = lengths_to_device(target_lengths, dev)
        T, B = input_audios.size(1), input_audios.size(0)
        (input_audios, input_texts, targets), t_lens, u_lens, enc_lens, inv = self._ragged_rows(
            audio_lengths, T, B, dev, t_lens, u_lens, (input_audios, input_texts, targets), True)
        enc = self.encoder.forward_time_major(input_audios, enc_lens)
        dec = self.decoder.forward_time_major(input_texts, u_lens + 1)
        res = joint_cell_logprobs(enc, dec, self.fc.weight, self.fc.bias, targets, t_lens, u_lens, int(blank))
        return res if inv is None else CellLogProbs(*(x.index_select(0, inv) for x in res))

    @torch.no_grad()
    def recognize_greedy(self, inputs: torch.Tensor, inputs_lengths, blank_token_id: int, max_iters: int = 3,
                         visit_padded_frames: bool = False, return_timing: bool = False, max_out=None, ctc_skip=None):
        """Greedy search, same result as transducer.py:95-145: per frame up to `max_iters` non-blank symbols, a symbol
        equal to the previously appended one is dropped (but still advances the prediction net).  Returns a LongTensor
        (1, n) for a single utterance, as the reference's `torch.stack` does.  For B > 1 (where the reference's stack
        raises on ragged outputs) a list of B 1-D LongTensors, each equal to what the reference returns for that
        utterance decoded alone; `visit_padded_frames=True` instead walks all max(lengths) frames for every utterance,
        which is what the reference's loop bound (transducer.py:115,121) does inside a batched call.
        return_timing=True returns per utterance an ops.TimedTokens (tokens int64, frames int32, logp float32), three 1-D
        tensors of equal length, instead of the tokens alone (one tuple for a single utterance, else a list): for every
        appended token the encoder frame at which the search chose it and the log-softmax of the joint at that evaluation,
        at that token (fp32).  A symbol dropped as a repeat has no entry.  `LogMelFrontend.frame_seconds` turns frames into
        seconds.  max_out caps the entries kept per utterance (default: max_iters per frame, which never truncates).
        ctc_skip=p (a probability in (0, 1]; needs the CTC head): the search walks only the frames whose CTC blank
        posterior is at most p (ctc_head on the encoder output, one pass on the device, no host sync); the frames of
        return_timing still count the encoder's frames.  None (the default): every frame, the head is not evaluated.  1.0 skips
        nothing.  ValueError with visit_padded_frames=True, without the head or for p outside (0, 1], before anything runs."""
        if self.training:
            raise RuntimeError("recognize_greedy expects eval() mode (dropout inactive), like the reference's validation_step")
        if ctc_skip is not None:
            self._check_ctc_skip(ctc_skip, blank_token_id, "recognize_greedy", visit_padded_frames)
        enc, t_lens, skip = self._search_encoder(inputs, inputs_lengths, blank_token_id, ctc_skip)
        res = greedy_decode(enc, *self.search_weights(), blank_token_id, max_iters, None if visit_padded_frames else t_lens,
                            timing=return_timing, max_out=max_out)
        if skip is not None and return_timing:   # one device gather: compacted frame -> encoder frame
            res = (res[0], res[1], map_frames(res[2], skip.frame_map), res[3])
        tokens, ntok = res[0], res[1]
        n = ntok.tolist()  # the only host sync of the decode
        if return_timing:
            outs = [TimedTokens(tokens[b, :n[b]], res[2][b, :n[b]], res[3][b, :n[b]]) for b in range(tokens.shape[0])]
            return outs[0] if len(outs) == 1 else outs
        outs = [tokens[b, :n[b]] for b in range(tokens.shape[0])]
        return outs[0].unsqueeze(0) if len(outs) == 1 else outs

    @torch.no_grad()
    def recognize_beams(self, inputs: torch.Tensor, inputs_lengths, blank_token_id: int, beam_widths: int = 100,
                        improved: bool = False, state_beam: float = 4.6, expand_beam: float = 2.3, lm=None, tokenizer=None,
                        hotwords=None, hotword_weight: float = 10.0, *, visit_padded_frames: bool = False,
                        return_scores: bool = False, return_frames: bool = False, fusion=None, ilm_weight=None, ctc_skip=None,
                        **caps):
        """Beam search, same result as transducer.py:215-361 with lm=None and hotwords=None: a list of up to `beam_widths`
        y_star token lists (leading blank included), best first by asr_score / len(y_star), duplicates kept.  `tokenizer` is
        accepted and ignored: without an LM or hotwords the reference only uses it for lm_score, which never decides anything.
        `lm` / `hotwords` raise NotImplementedError (rescoring needs pyctcdecode and KenLM; out of scope).
        For a single utterance the list itself, as the reference returns.  For B > 1 (the reference decodes only the first
        utterance of a batch) one such list per utterance, each equal to decoding that utterance alone; `visit_padded_frames=True`
        walks all max(lengths) frames for every utterance.  return_scores=True returns (y_star, asr_score) pairs instead
        (fp64 scores).  `caps`: max_pops / max_candidates / max_states / max_nodes / max_len of ops.beam_search; a search that
        outgrows one raises RnntHipError naming it (the reference's loop is unbounded there).
        return_frames=True returns (y_star, frames) pairs, (y_star, frames, asr_score) with return_scores as well: frames is a
        list aligned with y_star, the encoder frame at which the search appended each token (-1 for the leading blank).
        Divergence: where the reference's max() over an empty A raises ValueError (improved mode) the frame ends instead.
        fusion (a TokenFusion on the model's device; rnntransducer_amd/fusion.py): the mechanism of the reference's lm= /
        hotwords= branch (transducer.py:253-256, 285-295, 355-360) over token ids instead of text.  Every comparison of the
        search uses asr_score + the automaton's total for the hypothesis' y_star, the n-best is sorted by (asr_score + total +
        final) / len(y_star), the prune test stays on the ASR log-probabilities.  With return_scores each hypothesis carries
        asr_score (what it is without fusion: the sum of the ASR log-probabilities) and then fused_score = asr_score + total +
        final, both fp64.  A positive bonus can make a frame's pop loop run away (so can the reference's hotwords): the
        max_pops cap ends it in RnntHipError naming max_pops, and the next call succeeds.  A backoff n-gram model (NgramFusion)
        is refused here with a ValueError that names the searches that take one: those whose cost per frame is bounded.
        ilm_weight (internal-LM subtraction) is refused the same way: it is a bonus for every emitted token, the kind of score
        that makes this search's pop loop run away; the frame-synchronous searches take it.
        ctc_skip=p: as in recognize_greedy, the search walks only the frames whose CTC blank posterior is at most p; the frames
        of return_frames still count the encoder's frames (mapped on the host behind the search's own copy)."""
        refuse_ilm_weight(ilm_weight, "recognize_beams", "a per-token bonus can make the best-first pop loop run away")
        if ctc_skip is not None:
            self._check_ctc_skip(ctc_skip, blank_token_id, "recognize_beams", visit_padded_frames)
        if lm is not None or hotwords is not None:
            raise NotImplementedError("recognize_beams: LM / hotword rescoring (pyctcdecode, KenLM) is not implemented; pass "
                                      "lm=None and hotwords=None, and give token-level hotwords or an LM table as fusion= "
                                      "(rnntransducer_amd.TokenFusion.from_hotwords / from_bigram)")
        if self.training:
            raise RuntimeError("recognize_beams expects eval() mode (dropout inactive), like the reference's inference script")
        check_fusion(fusion, self.num_classes, self.fc.weight.device, "recognize_beams")   # before anything is launched
        enc, t_lens, skip = self._search_encoder(inputs, inputs_lengths, blank_token_id, ctc_skip)
        res = beam_search(enc, *self.search_weights(), blank_token_id, beam_widths, improved, state_beam, expand_beam,
                          None if visit_padded_frames else t_lens, frames=return_frames, fusion=fusion, **caps)
        return self._nbest_lists(res, skip, return_scores, return_frames)

    @torch.no_grad()
    def recognize_beams_sync(self, inputs: torch.Tensor, inputs_lengths, blank_token_id: int, beam_widths: int = 16,
                             max_symbols: int = 1, *, token_min_logp: float = -math.inf, fusion=None,
                             return_scores: bool = False, return_frames: bool = False, ilm_weight: float = 0.0, ctc_skip=None):
        """Frame-synchronous beam search (csrc/beam_sync.hip), the search other transducer toolkits decode with:
        per frame the whole beam (beam_widths <= 64) expands at once, at most max_symbols (<= 4) tokens are emitted,
        hypotheses with the same token sequence are merged by logaddexp (a score is probability mass, not one path), and the
        prediction net advances once for all new hypotheses together.  Its cost per frame is bounded by beam_widths, V and
        max_symbols alone, so it cannot run away, with or without fusion, and no cap can overflow; recognize_beams stays the
        reference-faithful best-first search.  Returns up to beam_widths token lists y (leading blank included, as
        recognize_beams returns y_star), best first by score, no length normalisation; the list itself for a single utterance,
        otherwise one list per utterance.  return_scores: (y, score) pairs, fp64.  return_frames: (y, frames) pairs, (y, frames,
        score) with return_scores: per token the encoder frame at which its prefix first appeared (-1 for the leading blank);
        frames do not decrease along a hypothesis and at most max_symbols are equal.  token_min_logp: per frame only tokens
        whose log-softmax reaches it extend a hypothesis (-inf: all).
        fusion (a TokenFusion, or an NgramFusion: a backoff n-gram model built from an ARPA file or from token-id n-grams, on
        the model's device): the search ranks by score + the automaton's total, the output by score + total + final; with
        return_scores the entries carry score and then fused_score.
        ilm_weight = mu > 0: internal-LM subtraction (ILME).  The prediction net is itself a language model of
        the training transcripts, so plain fusion counts a language prior twice; with mu every emitted token v also adds
        -mu * ilm(v | y) to the total, ilm = the log-softmax over the non-blank tokens of the joint with the encoder's
        contribution zeroed (`ilm_score` gives its sum over a sequence).  fused_score = score + the automaton's part -
        mu * ilm_score(y).  With fusion=None the all-zero automaton is used: subtraction alone, and entries carry fused_score
        like any fused call.  0 (the default): the search above, untouched.  Finite and >= 0, ValueError otherwise.
        ctc_skip=p: as in recognize_greedy, the search walks only the frames whose CTC blank posterior is at most p; the frames
        of return_frames still count the encoder's frames.
        Any encoder direction.  eval() mode only; ValueError for training mode or bad arguments, before anything is launched."""
        if self.training:
            raise ValueError("recognize_beams_sync expects eval() mode (dropout inactive), like recognize_beams")
        check_beam_sync_args(beam_widths, max_symbols, token_min_logp, "recognize_beams_sync")
        check_ilm_weight(ilm_weight, "recognize_beams_sync")
        check_fusion(fusion, self.num_classes, self.fc.weight.device, "recognize_beams_sync", ngram=True)
        if not 0 <= int(blank_token_id) < self.num_classes:
            raise ValueError(f"recognize_beams_sync: blank {blank_token_id} outside [0,{self.num_classes})")
        if ctc_skip is not None:
            self._check_ctc_skip(ctc_skip, blank_token_id, "recognize_beams_sync")
        enc, t_lens, skip = self._search_encoder(inputs, inputs_lengths, blank_token_id, ctc_skip)
        res = beam_search_sync(enc, *self.search_weights(), int(blank_token_id), beam_widths, max_symbols, t_lens,
                               token_min_logp=token_min_logp, frames=return_frames, fusion=fusion, ilm_weight=ilm_weight)
        return self._nbest_lists(res, skip, return_scores, return_frames)

    @torch.no_grad()
    def ilm_score(self, targets: torch.Tensor, target_lengths, blank: int) -> torch.Tensor:
        """The internal LM's log-probability of given token sequences: targets (B, U) token ids without the
        leading blank, target_lengths B values in [0, U] -> (B,) float64 on targets' device,
            sum over u < target_lengths[b] of ilm(y_u | y_<u),
        ilm(. | y_<u) = the log-softmax over the NON-BLANK tokens of gelu(dec_u) W_d^T + fc.bias: the joint with the encoder's
        contribution zeroed, dec_u the prediction net's output after blank, y_0 .. y_{u-1} (started on blank from the zero state,
        as the searches prime an utterance).  It is what recognize_beams_sync(ilm_weight=mu) subtracts mu times per hypothesis
        (fused_score = score + the automaton's part - mu * ilm_score(y[1:])), and exp(-ilm_score / length) is the internal LM's
        perplexity on a text.  fp32 network arithmetic, the sum in fp64.  eval() mode only; ValueError for a blank among the
        counted tokens or bad shapes."""
        if self.training:
            raise ValueError("ilm_score expects eval() mode (dropout inactive), like recognize_beams_sync")
        V = self.num_classes
        if not 0 <= int(blank) < V:
            raise ValueError(f"ilm_score: blank {blank} outside [0,{V})")
        if not isinstance(targets, torch.Tensor) or targets.dim() != 2 or targets.dtype not in (torch.int32, torch.int64):
            raise ValueError("ilm_score: targets must be a (B, U) integer tensor")
        B, U = targets.shape
        dev = targets.device
        u_lens = lengths_to_device(target_lengths, dev).to(torch.int64)
        if tuple(u_lens.shape) != (B,) or bool(((u_lens < 0) | (u_lens > U)).any()):
            raise ValueError(f"ilm_score: target_lengths must be {B} values in [0, {U}]")
        tok = targets.to(torch.int64)
        valid = torch.arange(U, device=dev)[None, :] < u_lens[:, None]
        if bool((((tok == int(blank)) | (tok < 0) | (tok >= V)) & valid).any()):
            raise ValueError("ilm_score: a counted token is the blank or outside the vocabulary")
        if U == 0:
            return torch.zeros(B, dtype=torch.float64, device=dev)
        tok = torch.where(valid, tok, torch.full_like(tok, int(blank)))
        text = torch.cat((torch.full((B, 1), int(blank), dtype=torch.int64, device=dev), tok), dim=1)   # blank first: U + 1 steps
        dec = self.decoder.forward_time_major(text, torch.full((B,), U + 1, dtype=torch.int32, device=dev))   # (U+1, B, O_d)
        z = torch.nn.functional.gelu(dec[:U].float(), approximate="tanh") @ self.fc.weight[:, self.enc_out:].t() + self.fc.bias
        z[..., int(blank)] = -math.inf   # the blank is no word of the internal LM
        lp = torch.log_softmax(z, dim=-1).gather(2, tok.t().unsqueeze(-1)).squeeze(-1)   # (U, B)
        return torch.where(valid.t(), lp.double(), torch.zeros((), dtype=torch.float64, device=dev)).sum(0)   # (padding: -inf)

    def init_stream(self, batch_size: int, blank_token_id: int, device=None):
        """A GreedyStreamState for `batch_size` streams, each starting as recognize_greedy starts an utterance
        (transducer.py:116-119): zero encoder state, prediction net primed with one blank step from zero state, last token =
        blank.  `device`, if given, must be the model's: the state lives beside the weights."""
        from ..streaming import GreedyStreamState
        self.encoder.check_streamable("init_stream")
        return GreedyStreamState(self, batch_size, blank_token_id, device)

    @torch.no_grad()
    def recognize_greedy_stream(self, chunk: torch.Tensor, chunk_lengths, state, max_iters: int = 3, return_timing: bool = False):
        """Greedy search over the next chunk of every stream: chunk (B,T_c,F) fp32 on the GPU, chunk_lengths B values in
        [0,T_c] (frames past a stream's length are ignored; a stream with 0 frames is left bitwise unchanged), `state` from
        this model's init_stream, updated in place.  Returns a list of B 1-D LongTensors: the tokens appended during this chunk.
        The per-frame rule is recognize_greedy's; any chunking of an utterance gives the same bits as one chunk holding all of
        it, and the tokens of recognize_greedy wherever no two logits are within fp32 rounding of each other.
        return_timing=True returns ops.TimedTokens (tokens, frames, logp) per stream instead, as recognize_greedy does, with
        absolute frames: counted from the stream's last reset (the base is state.frames_seen, read on the device; still one
        host sync per chunk).  Frames and logp are chunk-invariant bit for bit like the tokens.
        Unidirectional encoders only; fp32 whatever compute_precision says."""
        from ..streaming import GreedyStreamState, host_lengths
        self.encoder.check_streamable("recognize_greedy_stream")
        self.encoder.check_stream_chunk(chunk, "recognize_greedy_stream")
        if not isinstance(state, GreedyStreamState):
            raise ValueError(f"recognize_greedy_stream takes the state of init_stream, got {type(state).__name__}")
        B, T, _ = chunk.shape
        state.check_fits(self, B, chunk.device)
        if max_iters < 1:
            raise ValueError(f"max_iters must be >= 1, got {max_iters}")
        lens = host_lengths(chunk_lengths, B, T)
        T_run = max(lens)
        if T_run == 0:
            empty = lambda dt: torch.empty(0, dtype=dt, device=chunk.device)
            if return_timing:
                return [TimedTokens(empty(torch.int64), empty(torch.int32), empty(torch.float32)) for _ in range(B)]
            return [empty(torch.int64) for _ in range(B)]
        A, lens_dev = self._stream_encoder(chunk, lens, T_run, state)
        res = stream_greedy(A, lens_dev, *self.search_weights(fc_bias=False), state.blank, max_iters, state.pred_h, state.pred_c,
                            state.pred_joint, state.last_token, frame_base=state.frames_seen if return_timing else None)
        tokens, ntok = res[0], res[1]
        state.frames_seen += lens_dev   # after the search's launch on this stream: the kernel read the count before the chunk
        n = ntok.tolist()  # the only host sync of the chunk
        if return_timing:
            return [TimedTokens(tokens[b, :n[b]], res[2][b, :n[b]], res[3][b, :n[b]]) for b in range(B)]
        return [tokens[b, :n[b]] for b in range(B)]

    def init_beam_stream(self, batch_size: int, blank_token_id: int, beam_widths: int = 100, improved: bool = False,
                         state_beam: float = 4.6, expand_beam: float = 2.3, device=None, fusion=None, ilm_weight=None, **caps):
        """A streaming.BeamStreamState for `batch_size` streams, each starting as recognize_beams starts an utterance
        (transducer.py:276-284): y_star = [blank], score 0, no prediction-net state.  The search options are fixed here: they
        size the workspace and belong to the utterance.  `caps`: max_pops / max_candidates / max_states / max_nodes / max_len as
        in ops.beam_search, with streaming defaults (ops.beam_stream_caps; max_nodes bounds the LIVE prefix tree, max_len the
        uncommitted tail of a y_star); `state.workspace_bytes` / `state.bytes_per_stream` tell what they cost.  `device`, if
        given, must be the model's.  The weights must not change while the state is open.
        fusion (a TokenFusion on the model's device): the streams search as recognize_beams(fusion=...) does; the automaton is
        fixed here, its state and total are carried with every hypothesis, and recognize_beams_stream(return_scores=True)
        returns asr_score and then fused_score per hypothesis.  ilm_weight is refused (ValueError), as recognize_beams
        refuses it."""
        from ..streaming import BeamStreamState
        refuse_ilm_weight(ilm_weight, "init_beam_stream", "a per-token bonus can make the best-first pop loop run away")
        self.encoder.check_streamable("init_beam_stream")
        return BeamStreamState(self, batch_size, blank_token_id, beam_widths, improved, state_beam, expand_beam, device,
                               fusion=fusion, **caps)

    @torch.no_grad()
    def recognize_beams_stream(self, chunk: torch.Tensor, chunk_lengths, state, *, return_scores: bool = False,
                               return_frames: bool = False):
        """Beam search over the next chunk of every stream: chunk (B,T_c,F) fp32 on the GPU, chunk_lengths B values in [0,T_c],
        `state` from this model's init_beam_stream, updated in place.  Returns a list of B n-best lists, each what
        recognize_beams returns for the frames that stream has been fed so far (transducer.py:215-361 with lm=None: full y_star
        with the leading blank, best first by asr_score / len(y_star), duplicates kept; (y_star, asr_score) pairs with
        return_scores=True), whatever the chunking: same tokens, bitwise the same fp64 scores.  A stream that has seen no
        frames returns [[blank]]; a stream with 0 frames in this chunk is left bitwise unchanged and returns its previous list.
        `state.stable_prefix(b)` is the part of stream b's answer that no later chunk can change.
        return_frames=True returns (y_star, frames) pairs ((y_star, frames, asr_score) with return_scores), frames as in
        recognize_beams but absolute: counted from the stream's last reset.  Ask for them from a stream's first chunk after a
        reset on: a chunk fed without them leaves that stream's frames unknown (ValueError) until its next reset.
        One launch for the search and one host sync per call.  A stream that outgrows a cap raises RnntHipError naming it after
        the other streams have been updated; it must be reset before it is fed again.
        Unidirectional encoders only; fp32 whatever compute_precision says."""
        from ..streaming import BeamStreamState, host_lengths
        self.encoder.check_streamable("recognize_beams_stream")
        self.encoder.check_stream_chunk(chunk, "recognize_beams_stream")
        if not isinstance(state, BeamStreamState):
            raise ValueError(f"recognize_beams_stream takes the state of init_beam_stream, got {type(state).__name__}")
        B, T, _ = chunk.shape
        state.check_fits(self, B, chunk.device)
        lens = host_lengths(chunk_lengths, B, T)
        state.check_feedable(lens)
        if return_frames:
            state.check_frames_known()   # before the encoder runs: a refused call leaves the state untouched
        T_run = max(lens)
        if T_run > 0:
            state.run_chunk(*self._stream_encoder(chunk, lens, T_run, state), return_frames)
        return state.results(return_scores, return_frames)

    def init_beam_sync_stream(self, batch_size: int, blank_token_id: int, beam_widths: int = 16, max_symbols: int = 1, *,
                              token_min_logp: float = -math.inf, fusion=None, device=None, max_nodes: int = 8192,
                              max_len: int = 256, ilm_weight: float = 0.0):
        """A streaming.BeamSyncStreamState for `batch_size` streams, each starting as recognize_beams_sync starts an utterance:
        the root [blank] with score 0 and one prediction-net step on blank pending.  The search options (beam_widths <= 64,
        max_symbols <= 4, token_min_logp, fusion: a TokenFusion or NgramFusion on the model's device) and the two caps are fixed here: max_nodes
        bounds the LIVE prefix tree (>= 1 + 4 * beam_widths * max_symbols), max_len the uncommitted tail of a returned sequence;
        `state.workspace_bytes` / `state.bytes_per_stream` tell what they cost.  `device`, if given, must be the model's.  The
        weights must not change while the state is open.  Unidirectional encoders only.  ValueError for bad arguments, before
        anything is allocated or launched.
        ilm_weight > 0: internal-LM subtraction as in recognize_beams_sync, fixed for the life of the state (`state.ilm_weight`);
        the streams then search as recognize_beams_sync(ilm_weight=...) does, with the same bits whatever the chunking."""
        from ..streaming import BeamSyncStreamState
        check_ilm_weight(ilm_weight, "init_beam_sync_stream")
        if self.training:
            raise ValueError("init_beam_sync_stream expects eval() mode (dropout inactive), like recognize_beams_sync")
        self.encoder.check_streamable("init_beam_sync_stream")
        return BeamSyncStreamState(self, batch_size, blank_token_id, beam_widths, max_symbols, token_min_logp=token_min_logp,
                                   fusion=fusion, device=device, max_nodes=max_nodes, max_len=max_len, ilm_weight=ilm_weight)

    @torch.no_grad()
    def recognize_beams_sync_stream(self, chunk: torch.Tensor, chunk_lengths, state, *, return_scores: bool = False,
                                    return_frames: bool = False):
        """Frame-synchronous beam search over the next chunk of every stream (csrc/beam_sync_stream.hip): chunk
        (B,T_c,F) fp32 on the GPU, chunk_lengths B values in [0,T_c], `state` from this model's init_beam_sync_stream, updated in
        place.  Returns a list of B n-best lists, each exactly what the offline search (recognize_beams_sync on this
        encoder's outputs) gives for the frames that stream has been fed since its last reset, whatever the chunking: the same
        token lists (leading blank included), bitwise the same fp64 scores and the same frames.  return_scores: (y, score)
        pairs ((y, score, fused_score) with fusion); return_frames: (y, frames[, score[, fused_score]]), frames absolute, counted
        from the reset, -1 for the leading blank.  A stream that has seen no frames returns [[blank]] with score 0 (fused_score
        final[0]); a stream with 0 frames in this chunk is left bitwise unchanged and returns its previous list.
        `state.stable_prefix(b)` is the part of stream b's answer that no later chunk can change.
        The cost of a frame is fixed by beam_widths, V and max_symbols.  One launch for the search and one host sync per call.
        The only run-time errors are the two caps: a stream that outgrows max_nodes or max_len raises RnntHipError naming it
        after the other streams have been updated, and must be reset before it is fed again.
        Unidirectional encoders only; eval() mode only; fp32 whatever compute_precision says.  Every guard runs before any launch
        (ValueError; RnntHipError for a failed stream that is fed again): a refused call leaves the state bitwise untouched."""
        from ..streaming import BeamSyncStreamState, host_lengths
        if self.training:
            raise ValueError("recognize_beams_sync_stream expects eval() mode (dropout inactive), like recognize_beams_sync")
        self.encoder.check_streamable("recognize_beams_sync_stream")
        if not isinstance(state, BeamSyncStreamState):
            raise ValueError(f"recognize_beams_sync_stream takes the state of init_beam_sync_stream, got {type(state).__name__}")
        self.encoder.check_stream_chunk(chunk, "recognize_beams_sync_stream")
        B, T, _ = chunk.shape
        state.check_fits(self, B, chunk.device)
        lens = host_lengths(chunk_lengths, B, T)
        state.check_feedable(lens)
        T_run = max(lens)
        if T_run > 0:
            state.run_chunk(*self._stream_encoder(chunk, lens, T_run, state), lens)
        return state.results(return_scores, return_frames)
