"""Times streaming beam search (JointNet.recognize_beams_stream, csrc/beam_stream.hip) against the two things a caller can do
without it, over the same frames.

    python tools/stream_beam_bench.py [--chunks 25] [--warmup 5] [--points B:Tc,...] [--out FILE.jsonl]

Model: tools/stream_bench.py's (4 x 512 unidirectional LSTM encoder, 1 x 512 LSTM prediction net, V = 72, random-init weights
scaled so that the search emits tokens), improved=True, beam 5, max_pops 1024 for every search (a random model pops far more
than a trained one).  Each stream is fed warmup + chunks chunks of T_c frames; every call is timed with HIP events around the
whole call (encoder chunk, joint half, search launch, the host sync and the result copies).  One JSON line per point:
  us_per_chunk      median over the timed chunks;  pops / steps per chunk and stream;  rtf = chunk time / (T_c x 10 ms)
  stream_total_ms   sum over ALL chunks (warm-up included: the comparison is over the same frames)
  offline_ms        (a) one recognize_beams call on the whole utterance (second of two calls)
  redecode_total_ms (b) recognize_beams on everything heard so far after each chunk: what a caller does without streaming
  same_as_offline   the final streaming n-best equals (a)'s token lists (other encoder kernels: expected, not guaranteed)"""
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

DEFAULT_POINTS = [(1, 4), (1, 16), (8, 16), (64, 16), (8, 64)]
OPTS = dict(beam_widths=5, improved=True)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return out, s.elapsed_time(e)


def run_point(B: int, Tc: int, chunks: int, warmup: int, redecode: bool) -> dict:
    net, _ = make_net(72)
    n = warmup + chunks
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + Tc)
    feats = torch.randn(B, n * Tc, 80, device="cuda", generator=g)
    state = net.init_beam_stream(B, 0, max_pops=1024, **OPTS)
    times, pops, steps, out = [], 0, 0, None
    for i in range(n):
        out, ms = timed(lambda: net.recognize_beams_stream(feats[:, i * Tc:(i + 1) * Tc], [Tc] * B, state))
        times.append(ms)
        if i >= warmup:
            pops += int(state.last_stats[:, 0].sum())
            steps += int(state.last_stats[:, 1].sum())
    us = statistics.median(times[warmup:]) * 1e3
    lens = [n * Tc] * B
    offline = lambda T: net.recognize_beams(feats[:, :T], [T] * B, 0, max_pops=1024, **OPTS)
    offline(n * Tc)
    off, off_ms = timed(lambda: offline(n * Tc))
    off = [off] if B == 1 else off
    res = dict(B=B, T_c=Tc, V=72, enc="4x512 lstm uni", pred="1x512 lstm", beam=5, improved=True, chunks=chunks, warmup=warmup,
               frames=n * Tc, us_per_chunk=round(us, 1), us_min=round(min(times[warmup:]) * 1e3, 1),
               us_max=round(max(times[warmup:]) * 1e3, 1), pops_per_chunk=round(pops / chunks / B, 1),
               steps_per_chunk=round(steps / chunks / B, 1), rtf=round(us / (Tc * FRAME_MS * 1e3), 5),
               stream_total_ms=round(sum(times), 2), offline_ms=round(off_ms, 2), same_as_offline=out == off,
               stable_prefix_len=[len(state.stable_prefix(b)) for b in range(min(B, 4))],
               final_len=[len(out[b][0]) for b in range(min(B, 4))], bytes_per_stream=state.bytes_per_stream)
    if redecode:
        res["redecode_total_ms"] = round(sum(timed(lambda: offline((i + 1) * Tc))[1] for i in range(n)), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", default="", help="B:Tc,... (default: 1:4, 1:16, 8:16, 64:16, 8:64)")
    ap.add_argument("--no-redecode", action="store_true", help="skip (b), the longest leg")
    ap.add_argument("--out", default="", help="also append the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_beam_bench needs the GPU")
    points = [tuple(int(v) for v in p.split(":")) for p in a.points.split(",")] if a.points else DEFAULT_POINTS
    with torch.no_grad():
        for B, Tc in points:
            line = json.dumps(run_point(B, Tc, a.chunks, a.warmup, not a.no_redecode))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
