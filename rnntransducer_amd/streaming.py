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

Streaming beam search (`JointNet.init_beam_stream` / `recognize_beams_stream`, csrc/beam_stream.hip) carries the search of
`recognize_beams` the same way: after every chunk each stream's n-best is what `recognize_beams` gives for the frames fed so far.

    state = jointnet.init_beam_stream(batch_size, blank, beam_widths=5, improved=True)
    for chunk, lengths in feed:
        nbest = jointnet.recognize_beams_stream(chunk, lengths, state)    # per stream: y_star lists, best first
        partial = state.stable_prefix(0)                                  # the tokens of stream 0 no later chunk can change

`init_beam_stream(..., fusion=TokenFusion)` makes the streams search with token-level fusion (fusion.py): the automaton is fixed
when the state is opened, every carried hypothesis keeps its automaton state and total on the device, and `final` is applied
only where the n-best is ranked, so the n-best after every chunk is still the offline fused result for the frames fed so far.

Streaming frame-synchronous beam search (`JointNet.init_beam_sync_stream` / `recognize_beams_sync_stream`,
csrc/beam_sync_stream.hip) carries the search of `recognize_beams_sync`: a fixed cost per frame, at most
beam_widths hypotheses and (max_symbols + 2) * beam_widths state slots per stream, and after every chunk bitwise the offline
search's n-best for the frames fed so far.

    state = jointnet.init_beam_sync_stream(batch_size, blank, beam_widths=16, max_symbols=1)
    for chunk, lengths in feed:
        nbest = jointnet.recognize_beams_sync_stream(chunk, lengths, state, return_scores=True)
        partial = state.stable_prefix(0)

The three state classes are layered.  `_StreamState` is what every state is: the model it was opened by, the opening guards
(batch size, device, blank), the encoder's carried state and `frames_seen`, `check_fits` over a per-class layout list, and
`reset(rows)`.  `_BeamStreamBase` adds what the two beam states share: the carried workspace and its rows, the output buffers of
a chunk, the host-side `committed` / `nbest` lists with their frames, `results`, and the two halves of a chunk's epilogue (read
the results of the streams that ran; mark the failed ones and raise the cap error).  GreedyStreamState, BeamStreamState and
BeamSyncStreamState keep only what is theirs.
"""
from __future__ import annotations

from typing import List, Sequence, Union

import torch

from . import ops
from ._lib import BEAM_NSTATS, BEAM_STATUS, BEAM_SYNC_STREAM_HEADER, CELL_LSTM, RnntHipError


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


class _StreamState:
    """What every streaming state is: opened by one model for `batch_size` streams on the model's device, with the encoder's
    carried state (enc_h / enc_c) and frames_seen.  A subclass names the JointNet method that opens it (INIT), extends
    `_layout` with its own tensors and resets its own part of the listed rows in `_reset`."""
    INIT = ""

    def _open(self, jointnet, batch_size: int, blank_token_id: int, device) -> torch.device:
        """The guards of opening a state, before anything is allocated: batch_size, `device` against the model's, the blank.
        Sets _net, batch_size and blank.  -> the device"""
        if batch_size < 1:
            raise ValueError(f"{self.INIT}: batch_size must be >= 1, got {batch_size}")
        home = jointnet.fc.weight.device
        device = torch.device(device) if device is not None else home
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device != home:
            raise ValueError(f"{self.INIT}: device {device} is not the model's ({home}); the state lives beside the weights")
        if not 0 <= blank_token_id < jointnet.num_classes:
            raise ValueError(f"{self.INIT}: blank_token_id {blank_token_id} outside [0, {jointnet.num_classes})")
        self._net = jointnet
        self.batch_size, self.blank = int(batch_size), int(blank_token_id)
        return device

    def _alloc_encoder(self, device) -> None:
        enc = self._net.encoder.rnn
        z = lambda: torch.zeros(enc.num_layers, self.batch_size, enc.hidden_size, device=device, dtype=torch.float32)
        self.enc_h = z()
        self.enc_c = z() if enc.CELL == CELL_LSTM else None
        self.frames_seen = torch.zeros(self.batch_size, device=device, dtype=torch.int64)

    @property
    def device(self) -> torch.device:
        return self.enc_h.device

    def _layout(self) -> list:
        """(name, tensor, shape, dtype) of every device tensor of the state a chunk's kernels index as a dense array."""
        enc, B = self._net.encoder.rnn, self.batch_size
        want = [("enc_h", self.enc_h, (enc.num_layers, B, enc.hidden_size), torch.float32),
                ("frames_seen", self.frames_seen, (B,), torch.int64)]
        if enc.CELL == CELL_LSTM:
            want.append(("enc_c", self.enc_c, (enc.num_layers, B, enc.hidden_size), torch.float32))
        return want

    def check_fits(self, jointnet, B: int, device) -> None:
        """ValueError unless this state was opened by `jointnet` for B streams on `device` and still has that layout."""
        if self._net is not jointnet:
            raise ValueError(f"this {type(self).__name__} was opened by another model: open one with this model's {self.INIT}")
        if B != self.batch_size:
            raise ValueError(f"a chunk of {B} streams for a state of {self.batch_size}")
        if device != self.device:
            raise ValueError(f"chunk on {device}, state on {self.device}")
        for name, t, shape, dtype in self._layout():
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device \
                    or not t.is_contiguous():
                raise ValueError(f"state.{name} is not a contiguous {dtype} tensor of shape {shape} on {self.device}")

    @torch.no_grad()
    def reset(self, rows):
        """Start a new utterance in the listed rows: zero encoder state, frames_seen = 0, and the search as the offline call
        starts an utterance (each class's `_reset`).  Every other row is left bitwise as it is.  -> self"""
        rows = sorted({int(r) for r in (rows.tolist() if isinstance(rows, torch.Tensor) else rows)})
        if any(not 0 <= r < self.batch_size for r in rows):
            raise ValueError(f"reset: rows must lie in [0, {self.batch_size})")
        if rows:
            self._reset(rows)
        return self

    def _zero_encoder_rows(self, rows: List[int]) -> torch.Tensor:
        """Zero encoder state and frames_seen = 0 in `rows`.  -> rows as an int32 tensor on the device, for the search's reset"""
        idx = torch.tensor(rows, device=self.device, dtype=torch.int64)
        for t in (self.enc_h, self.enc_c):
            if t is not None:
                t.index_fill_(1, idx, 0.0)
        self.frames_seen.index_fill_(0, idx, 0)
        return idx.to(torch.int32)


class GreedyStreamState(_StreamState):
    """Per-stream state of `JointNet.recognize_greedy_stream`, all on the device:
      enc_h / enc_c   (L_enc, B, H)   encoder state (enc_c None unless the encoder is an LSTM)
      pred_h / pred_c (L_pred, B, Hp) prediction-net state (pred_c None unless LSTM)
      pred_joint      (B, V)          the prediction-net half of the joint for that state, gelu(out_proj(h)) fc.weight[:, O_enc:]^T
      last_token      (B,) int64      last appended token (blank at the start of an utterance)
      frames_seen     (B,) int64      frames consumed since the stream's last reset
    Built by `JointNet.init_stream`; updated in place by each chunk.  `reset(rows)` primes the prediction net of the rows with one
    blank step from zero state and sets last token = blank."""
    INIT = "init_stream"

    def __init__(self, jointnet, batch_size: int, blank_token_id: int, device=None):
        device = self._open(jointnet, batch_size, blank_token_id, device)
        self._alloc_encoder(device)
        dec = jointnet.decoder.rnn
        z = lambda: torch.zeros(dec.num_layers, batch_size, dec.hidden_size, device=device, dtype=torch.float32)
        self.pred_h = z()
        self.pred_c = z() if dec.CELL == CELL_LSTM else None
        self.pred_joint = torch.zeros(batch_size, jointnet.num_classes, device=device, dtype=torch.float32)
        self.last_token = torch.full((batch_size,), self.blank, device=device, dtype=torch.int64)
        self.reset(range(batch_size))

    def _layout(self) -> list:
        dec, B = self._net.decoder.rnn, self.batch_size
        want = super()._layout() + [("pred_h", self.pred_h, (dec.num_layers, B, dec.hidden_size), torch.float32),
                                    ("pred_joint", self.pred_joint, (B, self._net.num_classes), torch.float32),
                                    ("last_token", self.last_token, (B,), torch.int64)]
        if dec.CELL == CELL_LSTM:
            want.append(("pred_c", self.pred_c, (dec.num_layers, B, dec.hidden_size), torch.float32))
        return want

    def _reset(self, rows: List[int]) -> None:
        ops.stream_greedy_reset(self._zero_encoder_rows(rows), *self._net.search_weights(fc_bias=False), self.blank, self.pred_h,
                                self.pred_c, self.pred_joint, self.last_token)


class _BeamStreamBase(_StreamState):
    """What the two streaming beam searches share.  On the device the carried `workspace` (the layer-0 input table of the
    prediction net, then one part per stream: `workspace_row`) and the outputs of a chunk (_small: count | status | ncommit
    rows, one transfer; _tokens, _lens, _scores, _fused; _commit and the two frame buffers, which each class sizes itself).  On the
    host `committed` / `nbest` with their frames and `failed`.  A subclass names its search (SEARCH, in the messages) and provides:
    `_descriptor(bare)`, `_workspace_query(d)` and `_launch_reset(d, rows, build_table)`; the buffers `_commit`, `_frames` and
    `_commit_frames` that `_read_results` reads (present before a chunk whose results are read with them); `_tail_width(lens_h,
    count, ran)`, the width of the `_tokens` / `_frames` slice that reaches the host; and, if it wants, `_failed_after(b)`."""
    SEARCH = ""

    def _alloc(self, device, fusion, small_rows: int) -> None:
        """Everything but the search options: `fusion` as the state keeps it, the encoder state, the zero-filled workspace at
        its 256-byte boundary, the chunk outputs and the host lists of streams that have seen no frames."""
        self.fusion = fusion
        self._final0 = float(fusion.final[0]) if fusion is not None else 0.0   # read once: a reset does not sync for it
        self._alloc_encoder(device)
        B, W, V, dec = self.batch_size, self.beam, self._net.num_classes, self._net.decoder.rnn
        d, _ = self._descriptor(bare=True)
        self.workspace_bytes = self._workspace_query(d)
        self.workspace = torch.zeros(self.workspace_bytes + 256, device=device, dtype=torch.uint8)
        self._ws_off = -self.workspace.data_ptr() % 256
        ngate = {0: 4, 1: 3}.get(dec.CELL, 1)
        self._table_bytes = (V * ngate * dec.hidden_size * 4 + 255) // 256 * 256
        self.bytes_per_stream = (self.workspace_bytes - self._table_bytes) // B
        self._small = torch.zeros(small_rows, B, device=device, dtype=torch.int32)
        self._tokens = torch.zeros(B, W, self.caps["max_len"], device=device, dtype=torch.int32)
        self._lens = torch.zeros(B, W, device=device, dtype=torch.int32)
        self._scores = torch.zeros(B, W, device=device, dtype=torch.float64)
        self._fused = torch.zeros(B, W, device=device, dtype=torch.float64) if fusion is not None else None
        self.committed = [[self.blank] for _ in range(B)]
        self.committed_frames = [[-1] for _ in range(B)]
        self.nbest = [[self._start_entry()] for _ in range(B)]
        self.nbest_frames = [[[-1]] for _ in range(B)]
        self.failed = [False] * B

    def _start_entry(self):
        """The n-best entry of a stream that has seen no frames: (y, score[, fused_score]); final[0] belongs to it."""
        return ([self.blank], 0.0) if self.fusion is None else ([self.blank], 0.0, self._final0)

    def _fusion_struct(self):
        return None if self.fusion is None else ops.fusion_struct(self.fusion, self._fused)

    def _point(self, d) -> None:
        """The state's buffers into a descriptor: the aligned workspace, the n-best outputs and the three rows of _small."""
        B, base = self.batch_size, self._small.data_ptr()
        d.workspace, d.workspace_bytes = self.workspace.data_ptr() + self._ws_off, self.workspace_bytes
        d.tokens, d.out_lens, d.scores = self._tokens.data_ptr(), self._lens.data_ptr(), self._scores.data_ptr()
        d.count, d.status, d.ncommit = base, base + 4 * B, base + 8 * B

    def workspace_row(self, b: int) -> torch.Tensor:
        """The bytes of stream b's part of the workspace (a view)."""
        lo = self._ws_off + self._table_bytes + b * self.bytes_per_stream
        return self.workspace[lo:lo + self.bytes_per_stream]

    def stable_prefix(self, b: int, return_frames: bool = False):
        """The committed tokens of stream b, leading blank included: the longest common prefix of the token sequences of ALL
        carried hypotheses.  Every hypothesis of any later frame extends one of those, so no later chunk can change it.
        return_frames=True: (tokens, frames), frames aligned with the tokens (absolute; -1 for the leading blank)."""
        if not return_frames:
            return list(self.committed[b])
        return list(self.committed[b]), list(self.committed_frames[b])

    def _layout(self) -> list:
        return super()._layout() + [("workspace", self.workspace, (self.workspace_bytes + 256,), torch.uint8)]

    def check_fits(self, jointnet, B: int, device) -> None:
        super().check_fits(jointnet, B, device)
        if -self.workspace.data_ptr() % 256 != self._ws_off:
            raise ValueError("state.workspace was replaced: its alignment offset no longer holds")

    def check_feedable(self, lens: Sequence[int]) -> None:
        bad = [b for b, n in enumerate(lens) if n > 0 and self.failed[b]]
        if bad:
            raise RnntHipError(f"{self.SEARCH}: stream(s) {bad[:4]} exceeded a cap in an earlier chunk and must be reset "
                               "(state.reset(rows)) before they are fed again")

    def _reset(self, rows: List[int], build_table: bool = False) -> None:
        idx = self._zero_encoder_rows(rows)
        d, keep = self._descriptor()
        self._launch_reset(d, idx, build_table)
        for r in rows:
            self.committed[r], self.committed_frames[r] = [self.blank], [-1]
            self.nbest[r], self.nbest_frames[r], self.failed[r] = [self._start_entry()], [[-1]], False

    def results(self, return_scores: bool, return_frames: bool = False):
        if not return_frames:   # an entry is (y, score[, fused_score])
            return [[(list(y), *s) for y, *s in hyps] if return_scores else [list(y) for y, *_ in hyps] for hyps in self.nbest]
        return [[(list(y), list(f), *s) if return_scores else (list(y), list(f)) for (y, *s), f in zip(hyps, frs)]
                for hyps, frs in zip(self.nbest, self.nbest_frames)]

    def _read_results(self, ran: List[int], count, ncommit, timed: bool) -> None:
        """A chunk's device outputs into `committed` / `nbest` of the streams `ran` (behind the chunk's host sync: the slices are
        copied from an idle stream), with their frames if `timed`; without, those streams' frames become unknown (None)."""
        lens_h, scores_h = self._lens.cpu().tolist(), self._scores.cpu().tolist()
        fused_h = self._fused.cpu().tolist() if self.fusion is not None else None
        nt, nc = max(1, self._tail_width(lens_h, count, ran)), max(1, max(ncommit[b] for b in ran))
        tok_h, com_h = self._tokens[:, :, :nt].cpu(), self._commit[:, :nc].cpu()
        if timed:
            fr_h, cfr_h = self._frames[:, :, :nt].cpu(), self._commit_frames[:, :nc].cpu()
        for b in ran:
            self.committed[b] += com_h[b, :ncommit[b]].tolist()
            self.nbest[b] = [(self.committed[b] + tok_h[b, r, :lens_h[b][r]].tolist(), scores_h[b][r]) +
                             (() if fused_h is None else (fused_h[b][r],)) for r in range(count[b])]
            if timed:
                self.committed_frames[b] += cfr_h[b, :ncommit[b]].tolist()
                self.nbest_frames[b] = [self.committed_frames[b] + fr_h[b, r, :lens_h[b][r]].tolist() for r in range(count[b])]
            else:
                self.committed_frames[b], self.nbest_frames[b] = None, None

    def _failed_after(self, b: int) -> str:
        return ""

    def _raise_failed(self, bad: List[int], status) -> None:
        """Mark the streams `bad` (a cap overflowed in this chunk) and raise for the first, after every other stream's update."""
        for b in bad:
            self.failed[b] = True
        if bad:
            b = bad[0]
            what, kw = BEAM_STATUS.get(status[b], ("unknown", "?"))
            raise RnntHipError(f"{self.SEARCH}: stream {b} exceeded the cap on {what} ({kw}={self.caps.get(kw)})"
                               f"{self._failed_after(b)}; open the state with a larger {kw}= keyword.  The other streams are "
                               f"unaffected; stream(s) {bad[:4]} must be reset (state.reset(rows)) before they are fed again")


class BeamStreamState(_BeamStreamBase):
    """Per-stream state of `JointNet.recognize_beams_stream`.  On the device:
      enc_h / enc_c   (L_enc, B, H)   encoder state (enc_c None unless the encoder is an LSTM)
      workspace       uint8           the carried search: the layer-0 input table of the prediction net, then per stream a
                                      header (len(B), state slots, prefix nodes, committed length, status), the WHOLE last-frame
                                      B set (fp64 score, prefix node, state slot, memo slot per entry), the prediction-net state
                                      slots those entries reference and the prefix-tree nodes (include/rnnt_hip.h)
      frames_seen     (B,) int64      frames consumed since the stream's last reset
    On the host: the committed tokens per stream (`stable_prefix`) and the n-best list of the last chunk that fed it.
    The search options and the caps are fixed here: they size the workspace and belong to the utterance.  The table is built
    from the prediction net's weights when the state is opened, so the weights must not change while it is open (as
    GreedyStreamState assumes for pred_joint).  `reset(rows)` starts the rows with the hypothesis set {[blank], score 0, no
    state} and committed = [blank].

    Caps (`ops.beam_stream_caps`; each overflow raises RnntHipError naming it): max_pops = max(128, 4 * beam_widths) pops per
    frame, max_candidates = max_pops * V, max_states = 3 * max_pops, max_nodes = 8192 live prefix nodes (the tree is collected
    after every chunk), max_len = 256 uncommitted tokens of a y_star.  Bytes per stream (`bytes_per_stream`; all of them,
    `workspace_bytes`): 32 * (max_candidates + max_pops) + 4 * max_states * (slot + 1) + 20 * max_nodes + 256 with slot =
    L * Hp * (2 if LSTM else 1) + V floats; at Hp = 512, V = 72, one LSTM layer and beam 5 that is 2.15 MB (0.29 MB A entries,
    1.69 MB state slots, 0.16 MB nodes) against about 20 MB for the offline defaults.

    fusion (a TokenFusion over the model's V tokens, on the state's device; ValueError otherwise): the search of
    recognize_beams(fusion=...).  It is fixed here; the workspace grows by 12 * (max_candidates + max_pops) bytes per stream
    (automaton state and fp64 total beside every A and B entry) and `nbest` entries are (y_star, asr_score, fused_score).  A
    positive bonus can make a frame's pop loop run away: max_pops ends it (RnntHipError), the stream must then be reset.

    Frames: `committed_frames[b]` / `nbest_frames[b]` are None once stream b took a chunk without return_frames=True since its
    last reset (`check_frames_known`); the frame buffers are made by the first chunk that asks for frames."""
    INIT, SEARCH = "init_beam_stream", "streaming beam search"

    def __init__(self, jointnet, batch_size: int, blank_token_id: int, beam_widths: int = 100, improved: bool = False,
                 state_beam: float = 4.6, expand_beam: float = 2.3, device=None, fusion=None, **caps):
        device = self._open(jointnet, batch_size, blank_token_id, device)
        unknown = set(caps) - set(ops.BEAM_STREAM_CAPS)
        if unknown:
            raise TypeError(f"init_beam_stream: unknown keyword(s) {sorted(unknown)}; the caps are {ops.BEAM_STREAM_CAPS}")
        ops.check_fusion(fusion, jointnet.num_classes, device, "init_beam_stream")
        self.beam, self.improved = int(beam_widths), bool(improved)
        self.state_beam, self.expand_beam = float(state_beam), float(expand_beam)
        self.caps = ops.beam_stream_caps(jointnet.num_classes, self.beam, **caps)
        self._alloc(device, fusion, 3 + BEAM_NSTATS)   # _small: count | status | ncommit | stats rows
        B = self.batch_size
        self._commit = torch.zeros(B, self.caps["max_nodes"], device=device, dtype=torch.int32)
        self._frames = self._commit_frames = None   # the timed chunk entry's outputs
        self.last_stats = torch.zeros(B, BEAM_NSTATS, dtype=torch.int32)   # of the last chunk: ops.beam_search's stats columns
        self._reset(list(range(B)), build_table=True)

    def _descriptor(self, bare: bool = False):
        d, keep = ops.beam_stream_desc(self.batch_size, *self._net.search_weights(fc_bias=False), self.blank, self.beam,
                                       self.improved, self.state_beam, self.expand_beam, self.caps)
        if not bare:
            self._point(d)
            d.stats, d.commit = self._small.data_ptr() + 12 * self.batch_size, self._commit.data_ptr()
        return d, keep

    def _workspace_query(self, d) -> int:
        return ops.beam_stream_workspace_bytes(d, fused=self.fusion is not None)

    def _launch_reset(self, d, rows: torch.Tensor, build_table: bool) -> None:
        ops.beam_stream_reset(d, rows, build_table, self._fusion_struct())

    def stable_prefix(self, b: int, return_frames: bool = False):
        if return_frames and self.committed_frames[b] is None:
            raise ValueError(f"stream {b} was fed a chunk without return_frames=True since its last reset: its frames are unknown")
        return super().stable_prefix(b, return_frames)

    def check_frames_known(self) -> None:
        """ValueError if a stream took a chunk without return_frames=True since its last reset (a call that returns frames
        returns them for every stream).  Called before anything is launched, like every guard of a chunk: a refused call
        leaves the state bitwise as it is."""
        unknown = [b for b, f in enumerate(self.committed_frames) if f is None]
        if unknown:
            raise ValueError(f"stream(s) {unknown[:4]} were fed a chunk without return_frames=True since their last reset: "
                             "their frames are unknown")

    def results(self, return_scores: bool, return_frames: bool = False):
        unknown = [b for b, f in enumerate(self.nbest_frames) if f is None] if return_frames else []
        if unknown:
            raise ValueError(f"stream(s) {unknown[:4]} were fed a chunk without return_frames=True since their last reset: their "
                             "frames are unknown")
        return super().results(return_scores, return_frames)

    @staticmethod
    def _tail_width(lens_h, count, ran) -> int:
        return max(max(lens_h[b]) for b in ran)

    def run_chunk(self, A: torch.Tensor, lens_dev: torch.Tensor, timed: bool = False) -> None:
        """The search over one chunk (A (T,B,V), lens_dev (B) int32; `timed` after check_frames_known): updates the workspace,
        `committed`, `nbest`, `frames_seen` and, with `timed`, their frames (the timed entry; without it the fed streams'
        frames become unknown); raises RnntHipError for a stream that outgrew a cap, after every other stream has been updated."""
        B = self.batch_size
        d, keep = self._descriptor()
        if timed:
            if self._frames is None:
                self._frames = torch.zeros_like(self._tokens)
                self._commit_frames = torch.zeros_like(self._commit)
            ops.beam_stream_chunk(d, A, lens_dev, self._frames, self._commit_frames, fusion=self._fusion_struct())
        else:
            ops.beam_stream_chunk(d, A, lens_dev, fusion=self._fusion_struct())
        self.frames_seen += lens_dev
        host = self._small.cpu()   # the host sync of the chunk
        count, status, ncommit = host[0].tolist(), host[1].tolist(), host[2].tolist()
        self.last_stats = host[3:].reshape(B, BEAM_NSTATS)
        ran = [b for b in range(B) if count[b] >= 0 and status[b] == 0]
        if ran:
            self._read_results(ran, count, ncommit, timed)
        self._raise_failed([b for b in range(B) if status[b] != 0], status)


class BeamSyncStreamState(_BeamStreamBase):
    """Per-stream state of `JointNet.recognize_beams_sync_stream`.  On the device:
      enc_h / enc_c   (L_enc, B, H)   encoder state (enc_c None unless the encoder is an LSTM)
      workspace       uint8           the carried search (include/rnnt_hip.h): the layer-0 input table of the prediction net,
                                      then per stream a header (`header(b)`), the beam in rank order (fp64 score, fusion total,
                                      automaton state, prefix node, state slot, pending token per member), the
                                      (max_symbols + 2) * beam_widths state slots, a round's candidate keys and the prefix tree
      frames_seen     (B,) int64      frames consumed since the stream's last reset
    On the host: the committed tokens and their frames per stream (`stable_prefix`) and the n-best list of the last chunk that
    fed it.  The search options, the fusion automaton and the caps are fixed here; the table is built from the prediction
    net's weights when the state is opened, so the weights must not change while it is open.  `reset(rows)` starts the rows with
    the beam = the root [blank] with score 0 and a pending prediction-net step on blank from the zero state, committed = [blank].

    Caps (`ops.beam_sync_stream_caps`): max_nodes = 8192 live prefix nodes (at least 1 + 4 * beam_widths * max_symbols; the
    tree is collected at every chunk's end and inside a chunk when a frame needs the room), max_len = 256 uncommitted tokens of
    a returned sequence.  These two are the ONLY run-time error paths (RnntHipError naming the cap; the stream must be reset):
    the cost of a frame is fixed by beam_widths, V and max_symbols, there is no pop loop, and a hotword weight cannot reach
    either cap through the scores.  Bytes per stream (`bytes_per_stream`; all of them, `workspace_bytes`): 256 + 32 W +
    4 (S + 2) W slot + 8 W V + 28 max_nodes, each part rounded up to 256, with slot = L * Hp * (2 if LSTM else 1) + V floats.
    ilm_weight > 0 (internal-LM subtraction; fixed here like the fusion automaton, kept as `state.ilm_weight`): the
    stream also carries the (m, lse) pair of every state slot, 8 (S + 2) W bytes more; without a fusion automaton the all-zero
    one is used, and entries carry fused_score like any fused stream's."""
    INIT, SEARCH = "init_beam_sync_stream", "streaming frame-synchronous beam search"

    def __init__(self, jointnet, batch_size: int, blank_token_id: int, beam_widths: int = 16, max_symbols: int = 1, *,
                 token_min_logp: float = float("-inf"), fusion=None, device=None, max_nodes: int = 8192, max_len: int = 256,
                 step_group: int = 0, ilm_weight: float = 0.0):
        what = self.INIT
        self.ilm_weight = ops.check_ilm_weight(ilm_weight, what)
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:   # stricter than _open's, and first
            raise ValueError(f"{what}: batch_size must be an integer >= 1, got {batch_size!r}")
        ops.check_beam_sync_args(beam_widths, max_symbols, token_min_logp, what)
        self.caps = ops.beam_sync_stream_caps(beam_widths, max_symbols, max_nodes=max_nodes, max_len=max_len)
        device = self._open(jointnet, batch_size, int(blank_token_id), device)
        ops.check_fusion(fusion, jointnet.num_classes, device, what, ngram=True)
        if self.ilm_weight > 0.0:
            fusion = ops.ilm_fusion(fusion, jointnet.num_classes, device)
        self.beam, self.max_symbols, self.token_min_logp = int(beam_widths), int(max_symbols), float(token_min_logp)
        self.step_group = step_group
        self._alloc(device, fusion, 3)   # (needs the GPU from here on)
        self._frames = torch.zeros_like(self._tokens)
        self._commit = self._commit_frames = None   # (B, max_nodes + S T): sized by the longest chunk so far
        self._reset(list(range(self.batch_size)), build_table=True)

    def _descriptor(self, bare: bool = False):
        d, keep = ops.beam_sync_stream_desc(self.batch_size, *self._net.search_weights(fc_bias=False), self.blank, self.beam,
                                            self.max_symbols, self.token_min_logp, self.caps, self.step_group)
        if not bare:
            self._point(d)
        return d, keep

    def _workspace_query(self, d) -> int:
        return ops.beam_sync_stream_workspace_bytes(d, ilm=self.ilm_weight > 0.0)

    def _launch_reset(self, d, rows: torch.Tensor, build_table: bool) -> None:
        ops.beam_sync_stream_reset(d, rows, build_table, ilm=self.ilm_weight > 0.0)

    def header(self, b: int) -> dict:
        """The header words of stream b's workspace part (one small copy from the device): n_beam, nodes, committed, frames,
        status, collections, collections_in_chunk (those run at a frame's start, for room), peak_nodes."""
        words = self.workspace_row(b)[:4 * len(BEAM_SYNC_STREAM_HEADER)].view(torch.int32).tolist()
        return dict(zip(BEAM_SYNC_STREAM_HEADER, words))

    @staticmethod
    def _tail_width(lens_h, count, ran) -> int:
        return max(max(lens_h[b][:count[b]], default=0) for b in ran)

    def _failed_after(self, b: int) -> str:
        return f" after {self.header(b)['frames']} frames"   # one more small copy, on the error path only

    def run_chunk(self, A: torch.Tensor, lens_dev: torch.Tensor, fed: Sequence[int]) -> None:
        """The search over one chunk (A (T,B,V), lens_dev (B) int32, `fed` the same on the host): one launch and one host sync.
        Updates the workspace, `committed`, `nbest`, their frames and `frames_seen`; raises RnntHipError for a stream that
        outgrew a cap, after every other stream has been updated."""
        B, T = self.batch_size, A.shape[0]
        ncom = self.caps["max_nodes"] + self.max_symbols * T
        if self._commit is None or self._commit.shape[1] != ncom:
            self._commit = torch.empty(B, ncom, device=self.device, dtype=torch.int32)
            self._commit_frames = torch.empty_like(self._commit)
        d, keep = self._descriptor()
        ilm = None
        if self.ilm_weight > 0.0:   # fc.bias is read at every chunk, like the other weights
            ilm = ops.ilm_struct(self._net.fc.bias, self.ilm_weight)
        ops.beam_sync_stream_chunk(d, A, lens_dev, self._commit, self._frames, self._commit_frames, fusion=self._fusion_struct(),
                                   ilm=ilm)
        self.frames_seen += lens_dev   # (a stream that fails here is reset before it is fed again)
        host = self._small.cpu()   # the host sync of the chunk
        count, status, ncommit = host[0].tolist(), host[1].tolist(), host[2].tolist()
        ran = [b for b in range(B) if fed[b] > 0 and status[b] == 0 and count[b] >= 0]
        if ran:
            self._read_results(ran, count, ncommit, True)
        self._raise_failed([b for b in range(B) if fed[b] > 0 and status[b] != 0], status)
