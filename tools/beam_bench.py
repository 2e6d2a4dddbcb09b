"""Times JointNet.recognize_beams (one persistent launch per batch, csrc/beam.hip) at the config-2 layer sizes and, on a
bounded sample, the CPU restatement of networks/transducer.py:215-361 (tests/beam_restatement.py).

    python tools/beam_bench.py [--batch 32] [--frames 1000] [--beam 5] [--no-improved] [--reps 2] [--cpu-frames 40]

Weights are random-init scaled as in tools/decode_bench.py; data synthetic.  Reports utt/s, pops and prediction-net steps
per utterance (steps < pops: pops served from the memo), the encoder / search split and the per-pop time of the search
launch.  The CPU baseline decodes the first --cpu-frames frames of one utterance and is scaled to --frames (marked so).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--no-improved", action="store_true", help="the reference's default improved=False")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--cpu-frames", type=int, default=40)
    a = ap.parse_args()
    improved = not a.no_improved
    from oracle.rnnt_oracle import OracleJointNet
    from rnntransducer_amd import ops
    from rnntransducer_amd.networks import JointNet
    from tests.beam_restatement import beam_search as cpu_beam_search
    tn = dict(input_size=80, hidden_size=512, output_size=320, num_layers=3, rnn_type="lstm", dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=72, pad_token_id=0, hidden_size=512, output_size=320, num_layers=1, rnn_type="lstm", dropout=0.0)
    torch.manual_seed(0)
    net = JointNet(dict(tn), dict(pn), 72)
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.mul_(4.0 if n.startswith("fc.") else 2.0)
        net.decoder.embedding.weight[0].zero_()
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net = net.cuda().eval()
    audios = torch.randn(a.batch, a.frames, 80)
    lens = [a.frames] * a.batch
    dev_audio = audios.cuda()
    t_dev = torch.tensor(lens, dtype=torch.int32, device="cuda")
    d = net.decoder

    def search(enc):
        return ops.beam_search(enc, net.fc.weight, net.fc.bias, d.embedding.weight, d.rnn.flat_weights(), d.rnn.CELL,
                               d.out_proj.weight, d.out_proj.bias, 0, a.beam, improved, t_lens=t_dev, stats=True)

    with torch.no_grad():
        enc = net.encoder.forward_time_major(dev_audio, t_dev)
        res, st = search(enc)   # warm-up; also the stats
        torch.cuda.synchronize()
        t_enc = t_search = 0.0
        for _ in range(a.reps):
            t0 = time.perf_counter()
            enc = net.encoder.forward_time_major(dev_audio, t_dev)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            search(enc)   # ends with its host sync
            t2 = time.perf_counter()
            t_enc += t1 - t0
            t_search += t2 - t1
    t_enc, t_search = t_enc / a.reps, t_search / a.reps
    dt = t_enc + t_search
    pops, steps = st[:, 0].double(), st[:, 1].double()
    # CPU restatement on a bounded sample (one utterance, the first cpu_frames frames), scaled to the full length
    ora = OracleJointNet(dict(tn), dict(pn), 72).eval()
    ora.load_state_dict(sd)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cf = min(a.cpu_frames, a.frames)
    t0 = time.perf_counter()
    want, margin, _ = cpu_beam_search(ora, audios[:1, :cf], [cf], 0, a.beam, improved)
    cpu_dt = time.perf_counter() - t0
    got = net.recognize_beams(dev_audio[:1, :cf].contiguous(), [cf], 0, a.beam, improved)
    cpu_utt_s = 1.0 / (cpu_dt * a.frames / cf)
    print(json.dumps({
        "metric": "beam search utterances/sec", "value": round(a.batch / dt, 3), "ms_per_batch": round(dt * 1e3, 1),
        "batch": a.batch, "frames": a.frames, "beam": a.beam, "improved": improved,
        "encoder_ms": round(t_enc * 1e3, 1), "search_ms": round(t_search * 1e3, 1),
        "pops_per_utt": round(float(pops.mean()), 1), "steps_per_utt": round(float(steps.mean()), 1),
        "memo_fraction": round(1.0 - float(steps.sum() / pops.sum()), 4),
        "max_pops_per_frame": int(st[:, 2].max()), "max_candidates_per_frame": int(st[:, 3].max()),
        "max_live_states": int(st[:, 4].max()), "prefix_nodes_per_utt": round(float(st[:, 5].double().mean()), 1),
        "search_us_per_pop": round(t_search * 1e6 / float(pops.max()), 2),
        "search_us_per_step": round(t_search * 1e6 / float(steps.max()), 2),
        "nbest_len_mean": round(sum(len(y) for h in res for y, _ in h) / max(1, sum(len(h) for h in res)), 1),
        "cpu_baseline": {"value": round(cpu_utt_s, 5), "unit": "utterances/sec", "kind": "restatement",
                         "sample": f"1 utterance, first {cf} frames, scaled to {a.frames}", "seconds": round(cpu_dt, 2),
                         "cores": torch.get_num_threads()},
        "speedup_vs_cpu": round(a.batch / dt / cpu_utt_s, 1),
        "agreement_on_cpu_sample": got == [y for y, _ in want[0]], "cpu_sample_margin": margin,
        "dtype": "f32 (scores f64)", "data": "synthetic"}))


if __name__ == "__main__":
    main()
