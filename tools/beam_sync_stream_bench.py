"""Times the streaming frame-synchronous beam search (JointNet.recognize_beams_sync_stream, csrc/beam_sync_stream.hip) against
the two things a caller can do without it, over the same frames.

    python tools/beam_sync_stream_bench.py [--chunks 30] [--points B:Tc,...] [--width 16] [--symbols 1] [--max-len 1024]
                                           [--max-nodes 8192] [--out FILE.jsonl]

Model: tools/stream_bench.py's (4 x 512 unidirectional LSTM encoder, 1 x 512 LSTM prediction net, V = 72, random-init weights
scaled so that the search emits tokens): config-2 sizes.  The 16 hypotheses of a random model do not settle on a common prefix
the way a trained model's do, so the uncommitted tails grow with the utterance and --max-len defaults to 1024 here, above the
state's default of 256.  Each stream is fed --chunks chunks of T_c frames; every call is timed
with HIP events around the whole call (encoder chunk, joint half, search launch, the host sync and the result copies).  One JSON
line per point:
  us_per_chunk      median over the chunks after the first (which pays the lazy allocations); rtf = chunk time / (T_c x 10 ms)
  stream_total_ms   sum over ALL chunks: the comparison is over the same frames
  offline_ms        (a) one recognize_beams_sync call on the whole utterance (second of two calls)
  redecode_total_ms (b) recognize_beams_sync on everything heard so far after each chunk: what a caller does without streaming
  same_as_offline   the final streaming n-best equals (a)'s token lists (other encoder kernels: expected, not guaranteed)
  collections       tree collections per stream over the run, and those that ran inside a chunk; peak_nodes; bytes_per_stream"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from stream_bench import FRAME_MS, make_net  # noqa: E402
from stream_beam_bench import timed  # noqa: E402

DEFAULT_POINTS = [(32, 16), (1, 16), (32, 1)]


def run_point(B: int, Tc: int, chunks: int, width: int, symbols: int, redecode: bool, max_len: int, max_nodes: int) -> dict:
    net, _ = make_net(72)
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + Tc)
    feats = torch.randn(B, chunks * Tc, 80, device="cuda", generator=g)
    state = net.init_beam_sync_stream(B, 0, width, symbols, max_len=max_len, max_nodes=max_nodes)
    times, out = [], None
    for i in range(chunks):
        out, ms = timed(lambda: net.recognize_beams_sync_stream(feats[:, i * Tc:(i + 1) * Tc], [Tc] * B, state))
        times.append(ms)
    us = statistics.median(times[1:] or times) * 1e3
    offline = lambda T: net.recognize_beams_sync(feats[:, :T], [T] * B, 0, width, symbols)
    offline(chunks * Tc)
    off, off_ms = timed(lambda: offline(chunks * Tc))
    off = [off] if B == 1 else off
    heads = [state.header(b) for b in range(min(B, 4))]
    res = dict(B=B, T_c=Tc, V=72, enc="4x512 lstm uni", pred="1x512 lstm", width=width, max_symbols=symbols, chunks=chunks,
               frames=chunks * Tc, us_per_chunk=round(us, 1), us_min=round(min(times[1:] or times) * 1e3, 1),
               us_max=round(max(times[1:] or times) * 1e3, 1), rtf=round(us / (Tc * FRAME_MS * 1e3), 5),
               stream_total_ms=round(sum(times), 2), offline_ms=round(off_ms, 2), same_as_offline=out == off,
               stable_prefix_len=[len(state.stable_prefix(b)) for b in range(min(B, 4))],
               final_len=[len(out[b][0]) for b in range(min(B, 4))], collections=[h["collections"] for h in heads],
               collections_in_chunk=[h["collections_in_chunk"] for h in heads], peak_nodes=[h["peak_nodes"] for h in heads],
               bytes_per_stream=state.bytes_per_stream, workspace_bytes=state.workspace_bytes, max_len=max_len, max_nodes=max_nodes)
    res["stream_over_offline"] = round(res["stream_total_ms"] / off_ms, 3)
    if redecode:
        res["redecode_total_ms"] = round(sum(timed(lambda: offline((i + 1) * Tc))[1] for i in range(chunks)), 2)
        res["redecode_over_stream"] = round(res["redecode_total_ms"] / res["stream_total_ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=30)
    ap.add_argument("--points", default="", help="B:Tc,... (default: 32:16, 1:16, 32:1)")
    ap.add_argument("--width", type=int, default=16)
    ap.add_argument("--symbols", type=int, default=1)
    ap.add_argument("--max-len", type=int, default=1024)
    ap.add_argument("--max-nodes", type=int, default=8192)
    ap.add_argument("--no-redecode", action="store_true", help="skip (b), the longest leg")
    ap.add_argument("--out", default="", help="also append the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beam_sync_stream_bench needs the GPU")
    points = [tuple(int(v) for v in p.split(":")) for p in a.points.split(",")] if a.points else DEFAULT_POINTS
    with torch.no_grad():
        for B, Tc in points:
            line = json.dumps(run_point(B, Tc, a.chunks, a.width, a.symbols, not a.no_redecode, a.max_len, a.max_nodes))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
