"""Times the search launch of JointNet.recognize_beams with and without token-level fusion (csrc/beam_shared.hpp, FUSED) at the
config-2 layer sizes, on the model and input of tools/beam_bench.py.

    python tools/fusion_bench.py [--batch 32] [--frames 1000] [--beam 5] [--no-improved] [--reps 5] [--parent-root DIR]

One JSON line per measurement, each the search (ops.beam_search on a precomputed encoder output, ending with its host sync)
timed --reps times after a warm-up:
    unfused          this tree, fusion=None: the unfused kernel instance
    unfused_parent   the same call in a BUILT checkout of the parent commit (--parent-root; run in a child process started before
                     this one touches the GPU, with that checkout's package and library), same inputs
    fused_zero       an all-zero automaton (S = 1): the fused instance doing the unfused search
    fused_hotwords   a two-phrase hotword automaton built from the unfused result (weight 0.3)
The cost of fusion is reported as measured; the unfused time has to lie within the parent's own run-to-run spread (its min..max
over the repeats), which the last line states.  --only NAME runs one measurement (what the child does)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def model_and_input(batch, frames):
    """tools/beam_bench.py's."""
    from rnntransducer_amd.networks import JointNet
    tn = dict(input_size=80, hidden_size=512, output_size=320, num_layers=3, rnn_type="lstm", dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=72, pad_token_id=0, hidden_size=512, output_size=320, num_layers=1, rnn_type="lstm", dropout=0.0)
    torch.manual_seed(0)
    net = JointNet(dict(tn), dict(pn), 72)
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.mul_(4.0 if n.startswith("fc.") else 2.0)
        net.decoder.embedding.weight[0].zero_()
    return net.cuda().eval(), torch.randn(batch, frames, 80).cuda()


def measure(name, a, fusion_of=None):
    from rnntransducer_amd import ops
    net, audio = model_and_input(a.batch, a.frames)
    improved = not a.no_improved
    t_dev = torch.tensor([a.frames] * a.batch, dtype=torch.int32, device="cuda")
    d = net.decoder

    def search(enc, **kw):
        return ops.beam_search(enc, net.fc.weight, net.fc.bias, d.embedding.weight, d.rnn.flat_weights(), d.rnn.CELL,
                               d.out_proj.weight, d.out_proj.bias, 0, a.beam, improved, t_lens=t_dev, stats=True, **kw)

    with torch.no_grad():
        enc = net.encoder.forward_time_major(audio, t_dev)
        res, st = search(enc)
        kw = {}
        if fusion_of is not None:
            kw["fusion"] = fusion_of(res).to("cuda")
            res, st = search(enc, **kw)   # warm-up of the fused instance; its stats
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            search(enc, **kw)
            times.append((time.perf_counter() - t0) * 1e3)
    pops = st[:, 0].double()
    out = {"measurement": name, "search_ms_median": round(statistics.median(times), 2), "search_ms_min": round(min(times), 2),
           "search_ms_max": round(max(times), 2), "reps": a.reps, "batch": a.batch, "frames": a.frames, "beam": a.beam,
           "improved": improved, "pops_per_utt": round(float(pops.mean()), 1), "max_pops_per_frame": int(st[:, 2].max()),
           "search_us_per_pop": round(statistics.median(times) * 1e3 / float(pops.max()), 2)}
    if fusion_of is not None:
        out["states"] = kw["fusion"].n_states
        out["hyps_with_nonzero_total"] = sum(e[2] != e[1] for h in res for e in h)
    print(json.dumps(out), flush=True)
    return out


def zero_fusion(_res):
    from rnntransducer_amd import TokenFusion
    return TokenFusion(torch.zeros(1, 72, dtype=torch.int32), torch.zeros(1, 72), torch.zeros(1))


def hotword_fusion(res):
    """Two phrases the search meets: the first two tokens of the best hypothesis of utterance 0 and of utterance 1."""
    from rnntransducer_amd import TokenFusion
    phrases = []
    for hyps in res[:2]:
        y = next((e[0] for e in hyps if len(e[0]) >= 3), None)
        if y is not None and y[1:3] not in phrases:   # equal lengths: prefix-free unless equal
            phrases.append(y[1:3])
    return TokenFusion.from_hotwords(phrases or [[1, 2]], 0.3, 72, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--no-improved", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-root", help="a built checkout of the parent commit")
    ap.add_argument("--only", choices=["unfused", "unfused_parent", "fused_zero", "fused_hotwords"])
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the tree whose package is measured (the child's: --parent-root)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    if a.only:
        measure(a.only, a, {"fused_zero": zero_fusion, "fused_hotwords": hotword_fusion}.get(a.only))
        return
    parent = None
    if a.parent_root:   # a fresh child process, before this one opens the GPU; its own package and library
        a.parent_root = os.path.abspath(a.parent_root)
        cmd = [sys.executable, os.path.abspath(__file__), "--only", "unfused_parent", "--root", a.parent_root, "--batch", str(a.batch),
               "--frames", str(a.frames), "--beam", str(a.beam), "--reps", str(a.reps)] + (["--no-improved"] if a.no_improved else [])
        env = {k: v for k, v in os.environ.items() if k != "RNNT_HIP_LIB"}
        line = subprocess.run(cmd, check=True, capture_output=True, text=True, env=env, cwd=a.parent_root).stdout.strip().splitlines()[-1]
        print(line, flush=True)
        parent = json.loads(line)
    here = measure("unfused", a)
    zero = measure("fused_zero", a, zero_fusion)
    hot = measure("fused_hotwords", a, hotword_fusion)
    out = {"summary": "fusion cost", "fused_zero_over_unfused": round(zero["search_ms_median"] / here["search_ms_median"], 4),
           "fused_hotwords_us_per_pop": hot["search_us_per_pop"], "unfused_us_per_pop": here["search_us_per_pop"]}
    if parent:
        out["unfused_over_parent"] = round(here["search_ms_median"] / parent["search_ms_median"], 4)
        out["parent_spread_ms"] = [parent["search_ms_min"], parent["search_ms_max"]]
        out["unfused_within_parent_spread"] = parent["search_ms_min"] <= here["search_ms_median"] <= parent["search_ms_max"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
