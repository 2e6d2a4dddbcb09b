"""Streaming greedy recognition: a batch of independent streams whose features arrive in chunks (the reference's
"continuously processes input samples and streams output symbols", model.py:12-18).

Per stream the encoder state, the prediction-net state and the greedy bookkeeping carry from one chunk to the next, so
feeding an utterance in any chunking gives the same bits as one chunk holding all of it: every per-element product of the
kernels (csrc/stream.hip) is computed in an order that depends neither on the chunk length, nor on where the chunk
boundaries fall, nor on the number of streams.  Against the offline `recognize_greedy` (other kernels, another product
order) the tokens agree wherever no two logits are within fp32 rounding of each other.  Streaming computes fp32 whatever `compute_precision` says.

    state = jointnet.init_stream(batch_size, blank)
    for chunk, lengths in feed:                  # chunk (B, T_c, F) on the GPU, lengths in [0, T_c] per stream
        new_tokens = jointnet.recognize_greedy_stream(chunk, lengths, state)
    state.reset([slot])                          # a new utterance in one slot; the other slots are not touched
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import torch

from . import ops
from ._lib import CELL_LSTM


def host_lengths(chunk_lengths: Union[Sequence[int], torch.Tensor], B: int, T: int) -> List[int]:
    """chunk_lengths (list or tensor of B values) -> python list, each in [0, T] (ValueError otherwise)."""
    if isinstance(chunk_lengths, torch.Tensor):
        chunk_lengths = chunk_lengths.reshape(-1).tolist()
    lens = [int(n) for n in chunk_lengths]
    if len(lens) != B:
        raise ValueError(f"chunk_lengths has {len(lens)} values for a batch of {B} streams")
    bad = [n for n in lens if not 0 <= n <= T]
    if bad:
        raise ValueError(f"chunk_lengths must lie in [0, {T}] (the chunk's frames), got {bad[:4]}")
    return lens


def check_chunk(chunk: torch.Tensor) -> None:
    ops._need_gpu(chunk)
    if chunk.dim() != 3:
        raise ValueError(f"a chunk is (B, T_c, F), got shape {tuple(chunk.shape)}")
    if chunk.dtype != torch.float32:
        raise ValueError(f"a chunk must be float32, got {chunk.dtype}")


class GreedyStreamState:
    """Per-stream state of `JointNet.recognize_greedy_stream`, all on the device:
      enc_h / enc_c   (L_enc, B, H)   encoder state (enc_c None unless the encoder is an LSTM)
      pred_h / pred_c (L_pred, B, Hp) prediction-net state (pred_c None unless LSTM)
      pred_joint      (B, V)          the prediction-net half of the joint for that state, gelu(out_proj(h)) fc.weight[:, O_enc:]^T
      last_token      (B,) int64      last appended token (blank at the start of an utterance)
      frames_seen     (B,) int64      frames consumed since the stream's last reset
    Built by `JointNet.init_stream`; updated in place by each chunk."""

    def __init__(self, jointnet, batch_size: int, blank_token_id: int, device=None):
        if batch_size < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        enc, dec = jointnet.encoder.rnn, jointnet.decoder.rnn
        home = jointnet.fc.weight.device
        device = torch.device(device) if device is not None else home
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device != home:
            raise ValueError(f"init_stream: device {device} is not the model's ({home}); the state lives beside the weights")
        if not 0 <= blank_token_id < jointnet.num_classes:
            raise ValueError(f"blank_token_id {blank_token_id} outside [0, {jointnet.num_classes})")
        self._net = jointnet
        self.batch_size, self.blank = int(batch_size), int(blank_token_id)
        z = lambda L, H: torch.zeros(L, batch_size, H, device=device, dtype=torch.float32)
        self.enc_h = z(enc.num_layers, enc.hidden_size)
        self.enc_c = z(enc.num_layers, enc.hidden_size) if enc.CELL == CELL_LSTM else None
        self.pred_h = z(dec.num_layers, dec.hidden_size)
        self.pred_c = z(dec.num_layers, dec.hidden_size) if dec.CELL == CELL_LSTM else None
        self.pred_joint = torch.zeros(batch_size, jointnet.num_classes, device=device, dtype=torch.float32)
        self.last_token = torch.full((batch_size,), self.blank, device=device, dtype=torch.int64)
        self.frames_seen = torch.zeros(batch_size, device=device, dtype=torch.int64)
        self.reset(range(batch_size))

    @property
    def device(self) -> torch.device:
        return self.enc_h.device

    def check_fits(self, jointnet, B: int, device) -> None:
        """ValueError unless this state was opened by `jointnet` for B streams on `device` and still has that layout."""
        if self._net is not jointnet:
            raise ValueError("this GreedyStreamState was opened by another model: open one with this model's init_stream")
        if B != self.batch_size:
            raise ValueError(f"a chunk of {B} streams for a state of {self.batch_size}")
        if device != self.device:
            raise ValueError(f"chunk on {device}, state on {self.device}")
        enc, dec = jointnet.encoder.rnn, jointnet.decoder.rnn
        want = [("enc_h", self.enc_h, (enc.num_layers, B, enc.hidden_size), torch.float32),
                ("pred_h", self.pred_h, (dec.num_layers, B, dec.hidden_size), torch.float32),
                ("pred_joint", self.pred_joint, (B, jointnet.num_classes), torch.float32),
                ("last_token", self.last_token, (B,), torch.int64), ("frames_seen", self.frames_seen, (B,), torch.int64)]
        if enc.CELL == CELL_LSTM:
            want.append(("enc_c", self.enc_c, (enc.num_layers, B, enc.hidden_size), torch.float32))
        if dec.CELL == CELL_LSTM:
            want.append(("pred_c", self.pred_c, (dec.num_layers, B, dec.hidden_size), torch.float32))
        for name, t, shape, dtype in want:
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device \
                    or not t.is_contiguous():
                raise ValueError(f"state.{name} is not a contiguous {dtype} tensor of shape {shape} on {self.device}")

    @torch.no_grad()
    def reset(self, rows) -> "GreedyStreamState":
        """Start a new utterance in the listed rows (zero encoder state, prediction net primed with one blank step from zero
        state, last token = blank, frames_seen = 0).  Every other row is left bitwise as it is."""
        rows = sorted({int(r) for r in (rows.tolist() if isinstance(rows, torch.Tensor) else rows)})
        if any(not 0 <= r < self.batch_size for r in rows):
            raise ValueError(f"reset: rows must lie in [0, {self.batch_size})")
        if not rows:
            return self
        idx = torch.tensor(rows, device=self.device, dtype=torch.int64)
        for t in (self.enc_h, self.enc_c):
            if t is not None:
                t.index_fill_(1, idx, 0.0)
        self.frames_seen.index_fill_(0, idx, 0)
        net, dec = self._net, self._net.decoder
        ops.stream_greedy_reset(idx.to(torch.int32), net.fc.weight, dec.embedding.weight, dec.rnn.flat_weights(), dec.rnn.CELL,
                                dec.out_proj.weight, dec.out_proj.bias, self.blank, self.pred_h, self.pred_c, self.pred_joint,
                                self.last_token)
        return self
