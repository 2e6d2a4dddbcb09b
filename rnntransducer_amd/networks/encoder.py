"""AudioTransNet — transcription network of the RNN-Transducer on the MI355X HIP path.

Mirrors the constructor and forward signature of the reference's networks/encoder.py:54-76,78-108 (same
argument names, same parameter names `rnn.*`, `out_proj.*`).  What differs is HOW: no sort / pack /
unpack / unsort and no cuDNN/MIOpen; sequences are masked per row inside the persistent HIP LSTM kernel,
which gives the same result (zero outputs on padded frames, reverse direction starting at each sequence's
last frame).  rnn_type is one of the reference's supported_rnns (lstm | gru | rnn, encoder.py:48-52).
"""
from typing import Sequence, Union

import torch
import torch.nn as nn

from ..ops import LinearFn
from .rnn import RNN_CELLS, HipLSTM


def lengths_to_device(lengths: Union[Sequence[int], torch.Tensor], device) -> torch.Tensor:
    """The reference hands lengths as python lists (dataloader.py:20,37); the kernels want int32 on device."""
    if isinstance(lengths, torch.Tensor):
        return lengths.to(device=device, dtype=torch.int32, non_blocking=True)
    return torch.tensor(list(lengths), dtype=torch.int32, device=device)


class HipLinear(nn.Linear):
    """nn.Linear parameters (same names / init), forward on the MFMA GEMM of librnnt_hip."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return LinearFn.apply(x, self.weight, self.bias)


class AudioTransNet(nn.Module):
    supported_rnns = RNN_CELLS

    def __init__(self, input_size: int, hidden_size: int, output_size: int, num_layers: int, rnn_type: str = "lstm",
                 dropout: float = 0.2, bidirectional: bool = True):
        super().__init__()
        if rnn_type.lower() not in self.supported_rnns:
            raise NotImplementedError(f"rnn_type={rnn_type!r}: supported {sorted(self.supported_rnns)}")
        self.hidden_size = hidden_size
        self.rnn = self.supported_rnns[rnn_type.lower()](input_size, hidden_size, num_layers,
                                                         dropout=(dropout if num_layers > 1 else 0.0),
                                                         bidirectional=bidirectional)
        self.out_proj = HipLinear(2 * hidden_size if bidirectional else hidden_size, output_size)

    def forward_time_major(self, inputs: torch.Tensor, lens_dev) -> torch.Tensor:
        """(B,T,F) mel + int32 device lengths (or an ops.RaggedPlan built from the host list of lengths) -> (T,B,O) time-major
        (what the fused joint+loss consumes)."""
        x_tm = inputs.transpose(0, 1).contiguous()
        return self.out_proj(self.rnn(x_tm, lens_dev))

    def set_compute_precision(self, p: str):
        """"fp32" | "fp16" for every recurrent stack below this module (HipLSTM.compute_precision); returns self."""
        for m in self.modules():
            if isinstance(m, HipLSTM):
                m.compute_precision = p
        return self

    def stream_chunk(self, chunk: torch.Tensor, lens_dev: torch.Tensor, T_run: int, h: torch.Tensor, c, out: torch.Tensor,
                     out_strides, fc=None):
        """One chunk of the unidirectional encoder on carried state (csrc/stream.hip), in place on h / c.  lens_dev (B) int32 on
        the device; only the first T_run = max(lens) frames run.  fc: (weight, bias) of the joint -> also returns its encoder
        half A.  The callers check the lengths and the chunk's width; ops.stream_rnn_chunk checks every shape again."""
        from ..ops import stream_rnn_chunk
        return stream_rnn_chunk(chunk[:, :T_run], lens_dev, self.rnn.flat_weights(), self.rnn.CELL, h, c, self.out_proj.weight,
                                self.out_proj.bias, out, out_strides, *(fc or (None, None)))

    def check_stream_chunk(self, chunk: torch.Tensor, what: str) -> None:
        """A chunk (B,T_c,F) float32 on the GPU with F = the encoder's input width."""
        from ..streaming import check_chunk
        check_chunk(chunk)
        if chunk.shape[2] != self.rnn.input_size:
            raise ValueError(f"{what}: chunk has {chunk.shape[2]} features, the encoder takes {self.rnn.input_size}")

    def check_streamable(self, what: str) -> None:
        if self.rnn.bidirectional:
            raise ValueError(f"{what}: a bidirectional encoder needs future frames and cannot stream")
        if self.training:
            raise RuntimeError(f"{what} expects eval() mode (dropout inactive), like recognize_greedy")

    @torch.no_grad()
    def forward_stream(self, chunk: torch.Tensor, chunk_lengths, state=None):
        """The encoder over one chunk with carried state: chunk (B,T_c,F) fp32 on the GPU, chunk_lengths B values in [0,T_c],
        state None (zeros) or what the previous call returned -> (out (B,T_c,O), state).  state is torch's format: (h, c) of
        (L,B,H) for LSTM, h otherwise; frames past a stream's length are ignored (its state carries unchanged) and come out as
        zeros, as in `forward`.  Unidirectional encoders only; fp32 whatever compute_precision says.  Feeding an utterance
        in any chunking gives the same bits."""
        from ..streaming import host_lengths
        self.check_streamable("forward_stream")
        self.check_stream_chunk(chunk, "forward_stream")
        B, T, _ = chunk.shape
        lens = host_lengths(chunk_lengths, B, T)
        L, H, lstm = self.rnn.num_layers, self.rnn.hidden_size, self.rnn.CELL == 0
        if state is None:
            h = torch.zeros(L, B, H, device=chunk.device)
            c = torch.zeros_like(h) if lstm else None
        else:
            h, c = state if lstm else (state, None)
            for name, t in (("h", h), ("c", c)) if lstm else (("h", h),):
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != (L, B, H) or t.dtype != torch.float32 \
                        or t.device != chunk.device:
                    raise ValueError(f"forward_stream: state {name} must be a float32 ({L},{B},{H}) tensor on {chunk.device} "
                                     "(torch's format: (h, c) for LSTM, h otherwise)")
            # a private dense copy: the caller's tensors stay as they are, whatever their strides
            h, c = h.detach().clone(memory_format=torch.contiguous_format), \
                (c.detach().clone(memory_format=torch.contiguous_format) if lstm else None)
        O = self.out_proj.out_features
        out = torch.zeros(B, T, O, device=chunk.device)
        T_run = max(lens)
        if T_run > 0:
            lens_dev = torch.tensor(lens, dtype=torch.int32, device=chunk.device)
            self.stream_chunk(chunk, lens_dev, T_run, h, c, out, (T * O, O))
        return out, ((h, c) if lstm else h)

    def forward(self, inputs: torch.Tensor, inputs_lengths) -> torch.Tensor:
        """Reference surface (encoder.py:78): (B,T,F), lengths -> (B,T,O)."""
        lens = lengths_to_device(inputs_lengths, inputs.device)
        return self.forward_time_major(inputs, lens).transpose(0, 1).contiguous()
