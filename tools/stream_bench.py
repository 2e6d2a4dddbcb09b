"""Times streaming greedy recognition (JointNet.recognize_greedy_stream, csrc/stream.hip): one chunk of T_c feature frames for
each of B streams, state carried from chunk to chunk.

    python tools/stream_bench.py [--chunks 25] [--warmup 5] [--points B:Tc:V,...]

Model: a 4 x 512 unidirectional LSTM encoder (80 mel, O = 320), a 1 x 512 LSTM prediction net, V = 72 (and one V = 2048
point); random-init weights scaled so that the search emits tokens, synthetic features.  Each chunk is timed with HIP events
around the whole call (it ends with the one host sync that reads the token counts); the median over --chunks chunks after
--warmup chunks is reported, and the same for the encoder alone (forward_stream).  One JSON line per point: us_per_chunk,
encoder_us, the library's kernel launches per chunk (csrc/stream.hip: T_c + L - 1 recurrence steps, the state copy-out, two
products, the search; torch adds per call one host-to-device copy of the lengths, three small fills / adds and the
device-to-host read of the token counts), tokens emitted per chunk and the real-time factor
rtf = chunk time / (T_c x 10 ms of audio)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_POINTS = [(b, t, 72) for b in (1, 8, 64, 256) for t in (4, 16, 64)] + [(64, 16, 2048)]
FRAME_MS = 10.0   # hop of the log-mel front-end (160 samples at 16 kHz)


def make_net(V: int, device="cuda"):
    from rnntransducer_amd.networks import JointNet
    tn = dict(input_size=80, hidden_size=512, output_size=320, num_layers=4, rnn_type="lstm", dropout=0.0, bidirectional=False)
    pn = dict(embedding_size=V, pad_token_id=0, hidden_size=512, output_size=320, num_layers=1, rnn_type="lstm", dropout=0.0)
    torch.manual_seed(0)
    net = JointNet(tn, pn, V)
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.mul_(4.0 if n.startswith("fc.") else 2.0)
        net.decoder.embedding.weight[0].zero_()
    return net.to(device).eval(), tn["num_layers"]


def run_point(B: int, Tc: int, V: int, chunks: int, warmup: int, timing: bool = False) -> dict:
    net, L_enc = make_net(V)
    state = net.init_stream(B, 0)
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + Tc)
    feats = [torch.randn(B, Tc, 80, device="cuda", generator=g) for _ in range(8)]
    lens = [Tc] * B
    times, ntok = [], 0
    for i in range(warmup + chunks):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = net.recognize_greedy_stream(feats[i % len(feats)], lens, state, return_timing=timing)
        e.record()
        e.synchronize()
        if i >= warmup:
            times.append(s.elapsed_time(e) * 1e3)
            ntok += sum((t.tokens if timing else t).numel() for t in out)
    us = statistics.median(times)
    # the encoder alone (recurrence + out_proj, forward_stream) on the same chunks: the rest is the joint half and the search
    enc_times, enc_state = [], None
    for i in range(warmup + chunks):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        _, enc_state = net.encoder.forward_stream(feats[i % len(feats)], lens, enc_state)
        e.record()
        e.synchronize()
        if i >= warmup:
            enc_times.append(s.elapsed_time(e) * 1e3)
    return dict(B=B, T_c=Tc, V=V, timing=timing, enc="4x512 lstm uni", pred="1x512 lstm", us_per_chunk=round(us, 1),
                us_min=round(min(times), 1), us_max=round(max(times), 1), encoder_us=round(statistics.median(enc_times), 1), chunks=chunks,
                library_launches_per_chunk=Tc + L_enc + 3, tokens_per_chunk=round(ntok / chunks, 2),
                rtf=round(us / (Tc * FRAME_MS * 1e3), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", default="", help="B:Tc:V,... (default: the sweep of the module docstring)")
    ap.add_argument("--timing", action="store_true", help="time recognize_greedy_stream(return_timing=True)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench needs the GPU")
    points = [tuple(int(v) for v in p.split(":")) for p in a.points.split(",")] if a.points else DEFAULT_POINTS
    with torch.no_grad():
        for B, Tc, V in points:
            print(json.dumps(run_point(B, Tc, V, a.chunks, a.warmup, a.timing)), flush=True)


if __name__ == "__main__":
    main()
