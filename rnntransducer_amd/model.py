"""RNNTransducer — the LightningModule surface of the reference's model.py on the MI355X HIP path.

Same constructor `(prednet_params, transnet_params, jointnet_params, args)`, same `forward`, `training_step`
(7-tuple batch of dataloader.py:49) and `configure_optimizers` (AdamW + OneCycleLR per step, model.py:110-126),
same attribute `jointnet` and therefore the same state_dict keys.  Inherits
pytorch_lightning.LightningModule when that package is importable, torch.nn.Module otherwise.

Differences, all inside the hot path:
  * `training_step` runs the FUSED joint + RNN-T loss (`JointNet.loss`): the (B,T,U+1,V) logits tensor the
    reference builds at model.py:56 is never materialised.  `forward()` still returns it on request.
  * blank/pad id comes from `args.blank_token_id` / `prednet_params["pad_token_id"]` (default 0, as in the shipped
    config.json:37,40) instead of loading a tokenizer (model.py:24-26): tokenizer and WER/CER are validation-side
    and out of scope.
  * `jointnet_params["aux_ctc"] = True` adds a CTC head on the encoder (JointNet.ctc_head) and `args.ctc_weight` (default 0.0) the
    auxiliary CTC loss of joint CTC + transducer training to `training_step`: loss = rnnt + ctc_weight * ctc.  Both are off by
    default; the reference has neither.
  * `args.fastemit_lambda` (default 0.0: off) adds FastEmit regularisation to `training_step`: the lattice gradient is changed so that
    the model learns to emit sooner, the logged loss stays the unregularised one (JointNet.loss).  The reference has no such knob.
  * `args.ar_left` / `args.ar_right` (default None: off) make `training_step` train the alignment-restricted loss (Ar-RNN-T): the batch
    then carries an 8th element, a (B, U) int32 table of reference frames (a teacher's `align`, `recognize_ctc_greedy(...,
    return_frames=True)`, an external aligner), and label u may be emitted only at frames [frame - ar_left, frame + ar_right].
    `args.ar_source = "ctc"` (default "frames": the 8-element contract above) takes the reference from the model's own CTC head
    instead, on the ordinary 7-element batch: each step aligns ctc_head(encoder output) to the transcript on the device
    (JointNet.ctc_align's kernels, no second encoder call, no host sync) and label u may be emitted at frames
    [first[u] - ar_left, last[u] + ar_right] of that best CTC path.  It needs `aux_ctc` and both ar knobs.
  * `args.mwer_weight` (default 0.0: off), `args.mwer_nbest` (4) and `args.mwer_max_symbols` (1) add minimum word error rate
    fine-tuning to `training_step`: loss = rnnt + ctc_weight * ctc + mwer_weight * risk, the risk being the expected number of token
    errors over the model's own n-best list (JointNet.mwer_loss).  With the weight at 0 the step is today's, bit for bit.
  * `args.kd_weight` (default 0.0: off) with `set_teacher(teacher)` adds lattice knowledge distillation to `training_step`: loss =
    rnnt + ctc_weight * ctc + ilmt_weight * ilm + kd_weight * kd, kd being the collapsed per-cell KL between a frozen teacher model
    (say the bidirectional offline model, for a unidirectional streaming student) and this one (JointNet.loss's kd_teacher).  The
    teacher is held outside the module tree: parameters, state_dict, optimizer and checkpoints are those of the student alone.
  * `validation_step` stays on the GPU (the reference moves the module to the CPU at model.py:65-72 because its
    decode is a host loop): fused loss + on-device greedy search; it returns token ids, and texts only if a
    tokenizer object was attached as `self.tokenizer`.
"""
from argparse import Namespace

import torch

from .loss import RNNTLoss
from .networks import JointNet
from .ops import CtcEmitWindows, check_ctc_skip, check_fastemit_lambda, check_ilmt_weight, check_kd_weight, emit_windows

try:  # pragma: no cover - not installed in the build image
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except Exception:  # noqa: BLE001
    pl = None
    _Base = torch.nn.Module


class RNNTransducer(_Base):
    def __init__(self, prednet_params: dict, transnet_params: dict, jointnet_params: dict, args: Namespace):
        super().__init__()
        if pl is not None:
            self.save_hyperparameters(prednet_params, transnet_params, jointnet_params, args)
        self.args = args
        self._ctor_args = {"prednet_params": dict(prednet_params), "transnet_params": dict(transnet_params),
                           "jointnet_params": dict(jointnet_params), "args": args}
        prednet_params = dict(prednet_params)
        blank = getattr(args, "blank_token_id", None)
        if blank is None:
            blank = prednet_params.get("pad_token_id", 0)
        self.blank_token_id = int(blank)
        prednet_params["pad_token_id"] = self.blank_token_id  # model.py:26
        self.jointnet = JointNet(dict(transnet_params), prednet_params, **jointnet_params)
        # Opt-in compute mode of the recurrent layers (include/rnnt_hip.h, RNNT_PRECISION_F16).  An explicit choice: NOT derived from
        # args.precision (reference checkpoints carry precision=16 in their saved args) nor from autocast, which changes nothing here.
        cp = getattr(args, "compute_precision", "fp32")
        if cp not in ("fp32", "fp16"):
            raise ValueError(f"args.compute_precision must be 'fp32' or 'fp16', got {cp!r}")
        self.jointnet.set_compute_precision(cp)
        # model.py:28-39 picks torchaudio (precision 16) or warp-transducer; both are this one HIP module here
        self.fastemit_lambda = check_fastemit_lambda(getattr(args, "fastemit_lambda", 0.0) or 0.0)
        self.rnnt_loss = RNNTLoss(blank=self.blank_token_id, reduction="mean", fastemit_lambda=self.fastemit_lambda)
        # alignment-restricted loss (JointNet.loss's emit_windows): both knobs or neither; None leaves training_step as it is
        self.ar_left, self.ar_right = getattr(args, "ar_left", None), getattr(args, "ar_right", None)
        if (self.ar_left is None) != (self.ar_right is None):
            raise ValueError("args.ar_left and args.ar_right must be set together")
        for name, v in (("args.ar_left", self.ar_left), ("args.ar_right", self.ar_right)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 0):
                raise ValueError(f"{name} must be an integer >= 0 or None, got {v!r}")
        # where the windows' reference comes from: "frames" (the batch's 8th element) or "ctc" (the model's own CTC head, every step)
        ar_source = getattr(args, "ar_source", None)
        self.ar_source = "frames" if ar_source is None else ar_source
        if self.ar_source not in ("frames", "ctc"):
            raise ValueError(f"args.ar_source must be 'frames' or 'ctc', got {ar_source!r}")
        if self.ar_source == "ctc":
            if self.ar_left is None:
                raise ValueError("args.ar_source = 'ctc' needs args.ar_left and args.ar_right")
            if not self.jointnet.aux_ctc:
                raise ValueError("args.ar_source = 'ctc' needs the CTC head: set jointnet_params['aux_ctc'] = True")
        self.ctc_weight = float(getattr(args, "ctc_weight", 0.0) or 0.0)
        if self.ctc_weight > 0.0 and not self.jointnet.aux_ctc:
            raise ValueError("args.ctc_weight > 0 needs the CTC head: set jointnet_params['aux_ctc'] = True")
        # MWER fine-tuning (JointNet.mwer_loss): off at weight 0, and training_step then takes the plain path
        mwer_weight = getattr(args, "mwer_weight", 0.0)
        nbest, max_symbols = getattr(args, "mwer_nbest", 4), getattr(args, "mwer_max_symbols", 1)
        self.mwer_nbest, self.mwer_max_symbols = (4 if nbest is None else nbest), (1 if max_symbols is None else max_symbols)
        self.mwer_weight = JointNet.check_mwer_args(self.mwer_nbest, self.mwer_max_symbols, 0.0, 511,
                                                    0.0 if mwer_weight is None else mwer_weight, "args.mwer_*")
        # CTC-guided blank-frame skipping (ctc_skip= of JointNet.mwer_loss / recognize_greedy): a blank-posterior threshold in (0, 1]
        # for MWER's n-best search and for validation_step's greedy search; None (the default) leaves both as they are
        self.mwer_ctc_skip, self.val_ctc_skip = getattr(args, "mwer_ctc_skip", None), getattr(args, "val_ctc_skip", None)
        for name, p in (("args.mwer_ctc_skip", self.mwer_ctc_skip), ("args.val_ctc_skip", self.val_ctc_skip)):
            if p is not None:
                check_ctc_skip(p, name)
                if not self.jointnet.aux_ctc:
                    raise ValueError(f"{name} needs the CTC head: set jointnet_params['aux_ctc'] = True")
        # internal-LM training (JointNet.loss's ilmt_weight): off at 0; the MWER path has no such term
        ilmt_weight = getattr(args, "ilmt_weight", 0.0)
        self.ilmt_weight = check_ilmt_weight(0.0 if ilmt_weight is None else ilmt_weight)
        if self.mwer_weight > 0.0 and self.ilmt_weight > 0.0:
            raise ValueError("args.mwer_weight > 0 does not combine with args.ilmt_weight > 0: mwer_loss takes no internal-LM term")
        # lattice knowledge distillation (JointNet.loss's kd_teacher / kd_weight): off at 0; needs set_teacher() before the first step
        kd_weight = getattr(args, "kd_weight", 0.0)
        self.kd_weight = check_kd_weight(0.0 if kd_weight is None else kd_weight)
        if self.kd_weight > 0.0 and self.ar_left is not None:
            raise ValueError("args.kd_weight > 0 does not combine with args.ar_left / args.ar_right: the distillation term has no windowed form")
        if self.kd_weight > 0.0 and self.mwer_weight > 0.0:
            raise ValueError("args.kd_weight > 0 does not combine with args.mwer_weight > 0: mwer_loss takes no teacher")
        object.__setattr__(self, "_kd_teacher", None)   # a plain attribute: never a submodule (set_teacher)

    def set_teacher(self, teacher):
        """The teacher of lattice knowledge distillation (args.kd_weight): another RNNTransducer with the same vocabulary and blank,
        on the same device.  It is put in eval() and its parameters stop requiring grad; it is kept OUTSIDE the module tree, so
        parameters(), state_dict(), the optimizer and checkpoints stay the student's alone (and .to() / .cuda() do not move it).
        training_step asks it for its cell log-probabilities on each batch, without a graph.  None removes it.  Returns self."""
        if teacher is not None:
            if not isinstance(teacher, RNNTransducer):
                raise ValueError(f"set_teacher takes an RNNTransducer (or None), got {type(teacher).__name__}")
            if teacher is self:
                raise ValueError("set_teacher: a model cannot be its own teacher")
            if teacher.jointnet.num_classes != self.jointnet.num_classes or teacher.blank_token_id != self.blank_token_id:
                raise ValueError(f"set_teacher: the teacher's vocabulary ({teacher.jointnet.num_classes} classes, blank "
                                 f"{teacher.blank_token_id}) must be the student's ({self.jointnet.num_classes}, {self.blank_token_id})")
            teacher.eval()
            teacher.requires_grad_(False)
        object.__setattr__(self, "_kd_teacher", teacher)
        return self

    def forward(self, input_audios, audio_lengths, input_texts, text_lengths):
        # the reference hands these two as python lists (dataloader.py:20,37): validating them costs no device sync
        if isinstance(audio_lengths, (list, tuple)) and (max(audio_lengths) > input_audios.size(1) or min(audio_lengths) < 1):
            raise ValueError(f"audio_lengths must lie in [1, {input_audios.size(1)}]")
        if isinstance(text_lengths, (list, tuple)) and (max(text_lengths) > input_texts.size(1) or min(text_lengths) < 1):
            raise ValueError(f"text_lengths must lie in [1, {input_texts.size(1)}]")
        return self.jointnet(input_audios, audio_lengths, input_texts, text_lengths)

    # ---- checkpoint wire format -------------------------------------------------------------------
    @staticmethod
    def read_reference_checkpoint(path: str) -> dict:
        """Reads a Lightning .ckpt as the reference trainer writes it (train.py:31-37 ModelCheckpoint; `save_hyperparameters`
        at model.py:22 stores the three parameter dicts AND the `argparse.Namespace` under `hyper_parameters`).  Weights-only
        unpickling: nothing from the file is executed; `argparse.Namespace` — a plain attribute container — is the one
        extra class allowed."""
        with torch.serialization.safe_globals([Namespace]):
            return torch.load(path, map_location="cpu", weights_only=True)

    AUX_KEYS = ("jointnet.ctc_head.weight", "jointnet.ctc_head.bias")   # what the reference's model does not have

    def load_reference_checkpoint(self, path: str, strict: bool = True):
        """Loads the `state_dict` (keys `jointnet.*`) of a reference-written Lightning .ckpt into this module.
        A model with the CTC head tolerates exactly the two `jointnet.ctc_head.*` keys missing from the file (the head keeps
        its initialisation); anything else missing or unexpected still raises under strict=True."""
        blob = self.read_reference_checkpoint(path)
        sd = {k: v for k, v in blob.get("state_dict", blob).items() if k.startswith("jointnet.")}
        if not (self.jointnet.aux_ctc and strict and not any(k in sd for k in self.AUX_KEYS)):
            return self.load_state_dict(sd, strict=strict)
        res = self.load_state_dict(sd, strict=False)
        missing = [k for k in res.missing_keys if k not in self.AUX_KEYS]
        if missing or res.unexpected_keys:
            raise RuntimeError(f"load_reference_checkpoint: missing keys {missing}, unexpected keys {list(res.unexpected_keys)}")
        return res

    @classmethod
    def from_reference_checkpoint(cls, path: str, **overrides):
        """`RNNTransducer.load_from_checkpoint(path, prednet_params=..., ...)` of inference.py:19-25 without Lightning:
        constructor arguments come from the file's `hyper_parameters` unless overridden."""
        blob = cls.read_reference_checkpoint(path)
        hp = dict(blob.get("hyper_parameters", {}))
        hp.update(overrides)
        model = cls(hp["prednet_params"], hp["transnet_params"], hp["jointnet_params"], hp["args"])
        sd = blob["state_dict"]
        model.load_state_dict({k: v for k, v in sd.items() if k.startswith("jointnet.")})
        return model

    def save_reference_checkpoint(self, path: str, epoch: int = 0, global_step: int = 0, optimizer=None,
                                  include_aux: bool = False) -> None:
        """Writes a Lightning-1.8-shaped .ckpt the reference's `load_from_checkpoint` / `--resume_from_checkpoint` accept:
        `state_dict` (CPU tensors, keys `jointnet.*`), `hyper_parameters` = what model.py:22 saves (three dicts + the
        Namespace), epoch / global_step, `optimizer_states` in torch's format when an optimizer is given.
        include_aux=False (default) drops the `jointnet.ctc_head.*` tensors, the `aux_ctc` entry of jointnet_params and a positive
        args.ctc_weight, so the reference's strict loader (and a model without the head) still accepts the file;
        include_aux=True keeps them (for `from_reference_checkpoint` of a model with the head)."""
        jp = dict(self._ctor_args["jointnet_params"])
        args = self._ctor_args["args"]
        sd = self.state_dict()
        if not include_aux:
            jp.pop("aux_ctc", None)
            sd = {k: v for k, v in sd.items() if k not in self.AUX_KEYS}
            if getattr(args, "ctc_weight", 0.0):
                args = Namespace(**{**vars(args), "ctc_weight": 0.0})
        blob = {
            "epoch": int(epoch), "global_step": int(global_step), "pytorch-lightning_version": "1.8.0",
            "state_dict": {k: v.detach().cpu().clone() for k, v in sd.items()},
            "hyper_parameters": {"prednet_params": dict(self._ctor_args["prednet_params"]),
                                 "transnet_params": dict(self._ctor_args["transnet_params"]), "jointnet_params": jp,
                                 "args": args},
            "hparams_name": "kwargs",
        }
        if optimizer is not None:
            osd = optimizer.state_dict()
            osd["state"] = {k: {n: (t.detach().cpu().clone() if isinstance(t, torch.Tensor) else t) for n, t in st.items()}
                            for k, st in osd["state"].items()}
            blob["optimizer_states"] = [osd]
        torch.save(blob, path)

    def training_step(self, batch, batch_idx):
        assert not getattr(self.args, "move_metrics_to_cpu", False), "DDP only (model.py:53)"
        windows = None
        if self.ar_left is not None and self.ar_source == "ctc":   # alignment-restricted loss around the CTC head's own best path
            if len(batch) != 7:
                raise ValueError(f"args.ar_source = 'ctc': training_step takes the ordinary 7-element batch, got {len(batch)} elements")
            windows = CtcEmitWindows(self.ar_left, self.ar_right)
        elif self.ar_left is not None:   # alignment-restricted loss: the batch's 8th element is the (B, U) reference frame table
            if len(batch) != 8:
                raise ValueError(f"args.ar_left / args.ar_right are set: training_step takes an 8-element batch whose last element is "
                                 f"the (B, U) int32 reference frame table, got {len(batch)} elements")
            windows = emit_windows(batch[7], batch[2], batch[6], self.ar_left, self.ar_right)
            batch = batch[:7]
        input_audios, audio_lengths, tensor_audio_lengths, input_texts, text_lengths, targets, target_lengths = batch
        lengths = audio_lengths if isinstance(audio_lengths, (list, tuple)) else None
        logging = pl is not None and getattr(self, "_trainer", None) is not None
        teacher_planes = None
        if self.kd_weight > 0.0:
            if self._kd_teacher is None:
                raise ValueError("args.kd_weight > 0 needs a teacher: call set_teacher(teacher) before training")
            teacher_planes = self._kd_teacher.jointnet.cell_logprobs(input_audios, tensor_audio_lengths, input_texts, targets,
                                                                     target_lengths, self.blank_token_id, audio_lengths=lengths)
        if windows is not None and self.mwer_weight > 0.0:
            raise ValueError("args.ar_left / args.ar_right do not combine with args.mwer_weight > 0: mwer_loss takes no emission windows")
        if self.mwer_weight > 0.0:   # rnnt + ctc_weight * ctc + mwer_weight * risk over the model's own n-best list
            out = self.jointnet.mwer_loss(
                input_audios, tensor_audio_lengths, input_texts, targets, target_lengths, self.blank_token_id,
                nbest=self.mwer_nbest, max_symbols=self.mwer_max_symbols, mwer_weight=self.mwer_weight, reduction="mean",
                audio_lengths=lengths, ctc_weight=self.ctc_weight, fastemit_lambda=self.fastemit_lambda, return_parts=logging,
                ctc_skip=self.mwer_ctc_skip)
            if logging:   # the parts are (total, rnnt[, ctc], risk, err1)
                self.log("train_loss", out[0], sync_dist=True)
                self.log("train_mwer_risk", out[-2].detach(), sync_dist=True)
            return {"loss": out[0] if logging else out}
        loss = self.jointnet.loss(input_audios, tensor_audio_lengths, input_texts, targets, target_lengths,
                                  self.blank_token_id, reduction="mean",   # reduction="mean" (model.py:39), inside the library
                                  audio_lengths=lengths, ctc_weight=self.ctc_weight, fastemit_lambda=self.fastemit_lambda,
                                  emit_windows=windows, ilmt_weight=self.ilmt_weight, kd_teacher=teacher_planes,
                                  kd_weight=self.kd_weight)
        if logging:
            self.log("train_loss", loss, sync_dist=True)
        return {"loss": loss}

    def align(self, batch):
        """JointNet.align on the 7-tuple batch of training_step with this model's blank: per utterance the frame at which each
        label of the transcript is emitted on the best path, and that path's score (ops.Alignment)."""
        input_audios, audio_lengths, tensor_audio_lengths, input_texts, text_lengths, targets, target_lengths = batch
        return self.jointnet.align(input_audios, tensor_audio_lengths, input_texts, targets, target_lengths, self.blank_token_id,
                                   audio_lengths=audio_lengths if isinstance(audio_lengths, (list, tuple)) else None)

    def ctc_align(self, batch, **kw):
        """JointNet.ctc_align on the 7-tuple batch of training_step with this model's blank: per utterance the first and last frame of
        each label on the CTC head's best path, and that path's score (ops.CtcAlignment; return_path=, return_token_logp=)."""
        input_audios, audio_lengths, tensor_audio_lengths, input_texts, text_lengths, targets, target_lengths = batch
        return self.jointnet.ctc_align(input_audios, tensor_audio_lengths, targets, target_lengths, self.blank_token_id,
                                       audio_lengths=audio_lengths if isinstance(audio_lengths, (list, tuple)) else None, **kw)

    def ilm_loss(self, input_texts, targets, target_lengths, reduction: str = "mean"):
        """JointNet.ilm_loss with this model's blank: the internal-LM loss on text alone (text-only internal-LM adaptation; no
        audio, no encoder call).  Freeze the encoder before building the optimizer: weight decay moves zero-gradient parameters."""
        return self.jointnet.ilm_loss(input_texts, targets, target_lengths, self.blank_token_id, reduction)

    def recognize_ctc_greedy(self, inputs, inputs_lengths, return_frames: bool = False):
        """JointNet.recognize_ctc_greedy with this model's blank: the encoder-only greedy decode through the CTC head."""
        return self.jointnet.recognize_ctc_greedy(inputs, inputs_lengths, self.blank_token_id, return_frames)

    def recognize_ctc_beams(self, inputs, inputs_lengths, beam_widths: int = 16, **kw):
        """JointNet.recognize_ctc_beams with this model's blank: the encoder-only CTC prefix beam search through the CTC head
        (token_min_logp=, fusion=, return_scores=, return_frames=; ilm_weight= is refused: no prediction net runs here)."""
        return self.jointnet.recognize_ctc_beams(inputs, inputs_lengths, self.blank_token_id, beam_widths, **kw)

    def recognize_beams_sync(self, inputs, inputs_lengths, **kw):
        """JointNet.recognize_beams_sync with this model's blank: the frame-synchronous transducer beam search with batched
        hypothesis steps (beam_widths=, max_symbols=, token_min_logp=, fusion=, ilm_weight=, return_scores=, return_frames=).
        ilm_weight > 0 subtracts the prediction net's internal language model per emitted token (ILME; JointNet.ilm_score
        scores a token sequence under it)."""
        return self.jointnet.recognize_beams_sync(inputs, inputs_lengths, self.blank_token_id, **kw)

    def init_stream(self, batch_size: int, device=None):
        """JointNet.init_stream with this model's blank: per-stream state for recognize_greedy_stream."""
        return self.jointnet.init_stream(batch_size, self.blank_token_id, device)

    def recognize_greedy_stream(self, chunk, chunk_lengths, state, max_iters: int = 3, return_timing: bool = False):
        """JointNet.recognize_greedy_stream: the tokens each stream appends during this chunk of features (with
        return_timing, their absolute frames and log-probabilities too)."""
        return self.jointnet.recognize_greedy_stream(chunk, chunk_lengths, state, max_iters, return_timing=return_timing)

    def init_beam_stream(self, batch_size: int, beam_widths: int = 100, improved: bool = False, state_beam: float = 4.6,
                         expand_beam: float = 2.3, device=None, fusion=None, **caps):
        """JointNet.init_beam_stream with this model's blank: per-stream state for recognize_beams_stream (fusion: a
        TokenFusion, fixed for the life of the state; ilm_weight= is refused: the frame-synchronous searches take it)."""
        return self.jointnet.init_beam_stream(batch_size, self.blank_token_id, beam_widths, improved, state_beam, expand_beam,
                                              device, fusion=fusion, **caps)

    def recognize_beams_stream(self, chunk, chunk_lengths, state, *, return_scores: bool = False, return_frames: bool = False):
        """JointNet.recognize_beams_stream: per stream the n-best list for the frames fed so far (with return_frames, the
        frame at which every token was appended too)."""
        return self.jointnet.recognize_beams_stream(chunk, chunk_lengths, state, return_scores=return_scores,
                                                    return_frames=return_frames)

    def init_beam_sync_stream(self, batch_size: int, beam_widths: int = 16, max_symbols: int = 1, **kw):
        """JointNet.init_beam_sync_stream with this model's blank: per-stream state for recognize_beams_sync_stream
        (token_min_logp=, fusion=, ilm_weight=, device=, max_nodes=, max_len=; all fixed for the life of the state)."""
        return self.jointnet.init_beam_sync_stream(batch_size, self.blank_token_id, beam_widths, max_symbols, **kw)

    def recognize_beams_sync_stream(self, chunk, chunk_lengths, state, *, return_scores: bool = False, return_frames: bool = False):
        """JointNet.recognize_beams_sync_stream: per stream the frame-synchronous search's n-best list for the frames fed so
        far, bitwise the offline search's (with return_frames, the frame of every token too)."""
        return self.jointnet.recognize_beams_sync_stream(chunk, chunk_lengths, state, return_scores=return_scores,
                                                         return_frames=return_frames)

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        """model.py:62-79: loss + greedy search (max 3 symbols per frame).  `pred_tokens` is a list of B 1-D LongTensors
        (each what the reference's batch-1 recognize_greedy returns for that utterance), `label_tokens` the un-padded targets.
        A model with the CTC head adds `ctc_loss` (the mean CTC term; `loss` stays the RNN-T loss) and `ctc_pred_tokens` (the
        encoder-only greedy decode, a list like `pred_tokens`)."""
        input_audios, audio_lengths, tensor_audio_lengths, input_texts, text_lengths, targets, target_lengths = batch
        aux = self.jointnet.aux_ctc
        nll = self.jointnet.loss(input_audios, tensor_audio_lengths, input_texts, targets, target_lengths, self.blank_token_id,
                                 return_parts=aux)
        if aux:
            _, nll, ctc_nll = nll
        was_training = self.jointnet.training
        self.jointnet.eval()
        try:
            pred = self.jointnet.recognize_greedy(input_audios, tensor_audio_lengths, self.blank_token_id, 3,
                                                  ctc_skip=self.val_ctc_skip)
            if aux:
                ctc_pred = self.jointnet.recognize_ctc_greedy(input_audios, tensor_audio_lengths, self.blank_token_id)
        finally:
            self.jointnet.train(was_training)
        pred = [p for p in pred] if isinstance(pred, list) else [pred[0]]
        u = target_lengths.tolist() if isinstance(target_lengths, torch.Tensor) else list(target_lengths)
        labels = [targets[b, :u[b]].long() for b in range(targets.size(0))]
        out = {"loss": nll.mean(), "pred_tokens": pred, "label_tokens": labels}
        if aux:
            out["ctc_loss"], out["ctc_pred_tokens"] = ctc_nll.mean(), ctc_pred
        tok = getattr(self, "tokenizer", None)
        if tok is not None:
            out["pred_texts"] = tok.batch_decode([p.tolist() for p in pred])
            out["label_texts"] = tok.batch_decode([l.tolist() for l in labels])
        return out

    def validation_epoch_end(self, validation_step_outputs):
        """model.py:81-108: mean validation loss + error rates over the epoch's validation_step outputs.  WER/CER when the
        steps carried texts (tokenizer attached), otherwise the token error rate on ids.  Returns the dict it logs."""
        from .metrics import char_error_rate, token_error_rate, word_error_rate
        out = {"val_loss": torch.stack([x["loss"].detach().reshape(()) for x in validation_step_outputs]).mean()}
        if validation_step_outputs and "pred_texts" in validation_step_outputs[0]:
            preds = [t for x in validation_step_outputs for t in x["pred_texts"]]
            labels = [t for x in validation_step_outputs for t in x["label_texts"]]
            out["val_wer"], out["val_cer"] = word_error_rate(preds, labels), char_error_rate(preds, labels)
        else:
            out["val_ter"] = token_error_rate([t for x in validation_step_outputs for t in x["pred_tokens"]],
                                              [t for x in validation_step_outputs for t in x["label_tokens"]])
        if pl is not None and getattr(self, "_trainer", None) is not None:
            for k, v in out.items():
                self.log(k, v.to(self.device) if isinstance(v, torch.Tensor) else v, sync_dist=True)
        return out

    def configure_optimizers(self):
        group = [{"params": [p for p in self.parameters()], "name": "OneCycleLR"}]
        trainer = getattr(self, "_trainer", None)
        if next(self.parameters()).is_cuda:
            # same optimiser, same hyper-parameters: parameters/gradients/moments flattened, one fused HIP step.
            # direct_grads (backward kernels add into the flat gradient views, no autograd accumulation kernels) is for loops
            # that use FlatAdamW.all_reduce_grads() as the DP exchange; under a Lightning trainer / DistributedDataParallel the
            # reducer needs autograd's accumulation hooks, so it stays off there.  args.direct_flat_grads overrides.
            from .optim import FlatAdamW
            direct = getattr(self.args, "direct_flat_grads", None)
            direct = (trainer is None) if direct is None else bool(direct)
            optimizer = FlatAdamW(group, lr=self.args.learning_rate, weight_decay=self.args.weight_decay, direct_grads=direct)
        else:
            optimizer = torch.optim.AdamW(group, lr=self.args.learning_rate, weight_decay=self.args.weight_decay)
        total = trainer.estimated_stepping_batches if trainer is not None else int(getattr(self.args, "total_steps"))
        scheduler = torch.optim.lr_scheduler.OneCycleLR(optimizer, max_lr=self.args.learning_rate, total_steps=total,
                                                        pct_start=self.args.warmup_ratio,
                                                        final_div_factor=self.args.final_div_factor)
        return {"optimizer": optimizer, "lr_scheduler": {"interval": "step", "scheduler": scheduler, "name": "AdamW"}}
