"""Bitwise comparison of the searches' Python host path (rnntransducer_amd/streaming.py, networks/transducer.py, ops.py) between
this tree and OTHER_TREE (e.g. the parent commit in a git worktree): one fresh process per source tree, every result as a .npy /
.json file, compared byte for byte.  Only Python differs, so every child loads THIS tree's built library through RNNT_HIP_LIB.
The method of tools/loss_host_parity.py.
   python tools/search_host_parity.py OTHER_TREE OUTDIR
   model:    F = 6, encoder 2 x 8 unidirectional, prediction net one layer of width 12, V = 7, aux_ctc=True; an LSTM pair and a GRU
             pair (the c states are None for the GRU); seeded weights times 3 (fc times 6) so that the searches emit tokens.
   batch:    B = 3, T = 12, lengths 12 / 7 / 9.
   offline:  recognize_greedy (plain, return_timing, visit_padded_frames, ctc_skip with timing); recognize_beams (plain, improved,
             scores + frames, a bigram TokenFusion, ctc_skip with frames, and max_pops = 1: the error's text); recognize_beams_sync
             (max_symbols 1 and 2, TokenFusion, NgramFusion, ilm_weight with and without fusion, frames, ctc_skip); mwer_loss (the
             value, the gradient of one encoder and one prediction-net weight; with and without ctc_skip); align with audio_lengths.
   streams:  each of the three streaming searches over the same utterances under two chunkings (4 / 3 / 5, and 2 / 6 / 4 with no
             frames for stream 1 in the last chunk), a reset([1]) after the first chunk; with and without frames / timing,
             fusion (both beam streams; the best-first ones open with max_pops = 1024) and ilm_weight (sync stream).  After
             the last chunk: the returned lists, stable_prefix, every state tensor, workspace_row(b), header(b) and last_stats.
             One sync stream with max_nodes at its minimum is fed until it raises (the error's text), reset, and fed one more
             chunk.
   The tool first runs OTHER_TREE twice: a file that differs between those two runs cannot be compared, is listed by name and left
   out (none is expected, and none of the streaming files may be).  Then "N of N files bytewise equal".  A file that one run
   wrote and another did not is MISSING: it is never left out, it fails the comparison.
A call that raises RnntHipError (a cap) is recorded with its text and compared like any result.
Exit status 1 when a file differs or is missing on one side, a streaming file is not reproducible, or a child fails (nothing more
is started then)."""
import json, math, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, B, T, LENS = 7, 3, 12, [12, 7, 9]
CHUNKINGS = {"a": [4, 3, 5], "b": [2, 6, 4]}   # frames [n0, n0 + k) per chunk; stream 1 (7 frames) gets none in the last chunk
W, S, MU = 4, 2, 0.3


def dump(tree, out):
    """Child: run every case with the package of `tree` and write the results to `out`."""
    import numpy as np, torch
    sys.path.insert(0, tree)
    from rnntransducer_amd import NgramFusion, TokenFusion, _lib
    from rnntransducer_amd.networks import JointNet
    assert os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))) == os.path.abspath(tree), _lib.__file__
    os.makedirs(out, exist_ok=True)
    dev = "cuda"

    def plain(x):
        """Any result as JSON-able data: tensors to lists, tuples to lists, floats by repr (bit-exact)."""
        if isinstance(x, torch.Tensor):
            return plain(x.detach().cpu().tolist())
        if isinstance(x, float):
            return repr(x)
        if isinstance(x, (list, tuple)):
            return [plain(e) for e in x]
        if isinstance(x, dict):
            return {k: plain(v) for k, v in x.items()}
        return x

    def save(name, x):
        if isinstance(x, torch.Tensor):
            np.save(os.path.join(out, name + ".npy"), x.detach().cpu().numpy())
        else:
            with open(os.path.join(out, name + ".json"), "w") as f:
                json.dump(plain(x), f)

    def attempt(call):
        try:
            return call()
        except _lib.RnntHipError as e:
            return {"error": str(e)}

    def model(cell):
        tn = dict(input_size=6, hidden_size=8, output_size=8, num_layers=2, rnn_type=cell, dropout=0.0, bidirectional=False)
        pn = dict(embedding_size=V, pad_token_id=0, hidden_size=12, output_size=8, num_layers=1, rnn_type=cell, dropout=0.0)
        torch.manual_seed(11)
        net = JointNet(tn, pn, V, aux_ctc=True)
        with torch.no_grad():
            for n, p in net.named_parameters():
                p.mul_(6.0 if n.startswith("fc.") else 3.0)
            net.decoder.embedding.weight[0].zero_()
        return net.to(dev).eval()

    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, 6, generator=gen).to(dev)
    long_x = torch.randn(1, 90, 6, generator=gen).to(dev)
    texts = torch.tensor([[0, 1, 2, 3, 4], [0, 5, 6, 0, 0], [0, 2, 2, 1, 0]], dtype=torch.int64, device=dev)
    targets, u_lens = texts[:, 1:].to(torch.int32).contiguous(), [4, 2, 3]
    hot = TokenFusion.from_hotwords([[1, 2], [3]], 1.5, V, 0).to(dev)
    # the best-first searches get an LM table: its arcs are <= 0, so it cannot make their pop loop run away as a bonus can
    lm = TokenFusion.from_bigram(torch.log_softmax(torch.randn(V, V, generator=gen), dim=1), 0.3, 0).to(dev)
    grams = {(k,): (math.log(0.05 + 0.03 * k), -0.3) for k in range(1, V)}
    grams.update({(1, 2): (-0.5, None), (2, 3): (-0.7, None), (3, 1): (-0.4, None), (5, 6): (-0.2, None)})
    ngram = NgramFusion.from_ngrams(grams, V, 0.5, 0, oov_logp=-4.0).to(dev)

    for cell in ("lstm", "gru"):
        net = model(cell)
        tag = cell + "_"
        # offline
        for name, kw in (("plain", {}), ("timing", dict(return_timing=True)), ("padded", dict(visit_padded_frames=True)),
                         ("skip_timing", dict(ctc_skip=0.6, return_timing=True))):
            save(tag + "greedy_" + name, attempt(lambda: net.recognize_greedy(x, LENS, 0, **kw)))
        for name, kw in (("plain", {}), ("improved", dict(improved=True)), ("scores_frames", dict(return_scores=True, return_frames=True)),
                         ("fusion", dict(fusion=lm, return_scores=True)), ("skip_frames", dict(ctc_skip=0.6, return_frames=True)),
                         ("max_pops", dict(max_pops=1))):
            save(tag + "beams_" + name, attempt(lambda: net.recognize_beams(x, LENS, 0, W, **kw)))
        for name, kw in (("s1", dict(max_symbols=1)), ("s2", dict(max_symbols=2)), ("token", dict(max_symbols=S, fusion=hot)),
                         ("ngram", dict(max_symbols=S, fusion=ngram)), ("ilm", dict(max_symbols=S, ilm_weight=MU)),
                         ("ilm_token", dict(max_symbols=S, ilm_weight=MU, fusion=hot)), ("frames", dict(max_symbols=S, return_frames=True)),
                         ("skip", dict(max_symbols=S, ctc_skip=0.6, return_frames=True))):
            save(tag + "sync_" + name, attempt(lambda: net.recognize_beams_sync(x, LENS, 0, W, return_scores=True, **kw)))
        for name, kw in (("plain", {}), ("skip", dict(ctc_skip=0.6))):
            net.zero_grad()
            loss = net.mwer_loss(x, LENS, texts, targets, u_lens, 0, nbest=W, max_symbols=S, audio_lengths=LENS, **kw)
            loss.backward()
            save(tag + "mwer_" + name, loss)
            save(tag + "mwer_" + name + "_g_enc", net.encoder.rnn.weight_hh_l0.grad)
            save(tag + "mwer_" + name + "_g_pred", net.decoder.rnn.weight_ih_l0.grad)
        net.zero_grad()
        al = net.align(x, LENS, texts, targets, u_lens, 0, audio_lengths=LENS)
        save(tag + "align_frames", al.frames), save(tag + "align_score", al.score)

        # the three streams
        def feed(state, call, name, **kw):
            """The utterances of `x` through `call` under one chunking, reset([1]) after the first chunk; saves what the
            calls returned and the state after the last chunk."""
            n0, returned = 0, []
            for i, k in enumerate(CHUNKINGS[name[-1]]):
                part = [max(0, min(m, n0 + k) - n0) for m in LENS]
                returned.append(attempt(lambda: call(x[:, n0:n0 + k], part, state, **kw)))
                n0 += k
                if i == 0:
                    state.reset([1])
            save(name + "_returned", returned)
            save(name + "_frames_seen", state.frames_seen), save(name + "_enc_h", state.enc_h)
            for attr in ("enc_c", "pred_h", "pred_c", "pred_joint", "last_token", "last_stats"):
                if getattr(state, attr, None) is not None:
                    save(name + "_" + attr, getattr(state, attr))
            if hasattr(state, "workspace_row"):
                save(name + "_prefix", [state.stable_prefix(b) for b in range(B)])
                save(name + "_committed", [state.committed, state.committed_frames, state.nbest, state.nbest_frames, state.failed])
                for b in range(B):
                    save(f"{name}_row{b}", state.workspace_row(b))
                if hasattr(state, "header"):
                    save(name + "_headers", [state.header(b) for b in range(B)])

        for c in CHUNKINGS:
            for name, kw in (("plain", {}), ("timing", dict(return_timing=True))):
                feed(net.init_stream(B, 0), net.recognize_greedy_stream, f"{tag}gstream_{name}_{c}", **kw)
            for name, init, kw in (("plain", {}, {}), ("frames", dict(improved=True), dict(return_scores=True, return_frames=True)),
                                   ("fusion", dict(fusion=lm), dict(return_scores=True))):
                feed(net.init_beam_stream(B, 0, W, max_pops=1024, **init), net.recognize_beams_stream, f"{tag}bstream_{name}_{c}", **kw)
            for name, init, kw in (("plain", dict(max_symbols=1), {}), ("frames", {}, dict(return_scores=True, return_frames=True)),
                                   ("token", dict(fusion=hot), dict(return_scores=True)), ("ngram", dict(fusion=ngram), dict(return_scores=True)),
                                   ("ilm", dict(ilm_weight=MU), dict(return_scores=True, return_frames=True)),
                                   ("ilm_token", dict(ilm_weight=MU, fusion=hot), dict(return_scores=True))):
                feed(net.init_beam_sync_stream(B, 0, W, **{"max_symbols": S, **init}), net.recognize_beams_sync_stream,
                     f"{tag}sstream_{name}_{c}", **kw)
        # the cap: max_nodes at its minimum, fed until it raises; then a reset and one more chunk
        state = net.init_beam_sync_stream(1, 0, W, S, max_nodes=1 + 4 * W * S)
        log = []
        for n0 in range(0, long_x.shape[1], 5):
            log.append(attempt(lambda: net.recognize_beams_sync_stream(long_x[:, n0:n0 + 5], [5], state, return_scores=True)))
            if isinstance(log[-1], dict):
                break
        log.append([state.failed[0], state.header(0)])
        state.reset([0])
        log.append(net.recognize_beams_sync_stream(long_x[:, :5], [5], state, return_scores=True, return_frames=True))
        save(tag + "sstream_cap", log), save(tag + "sstream_cap_row", state.workspace_row(0))
    torch.cuda.synchronize()
    print(f"dumped {len(os.listdir(out))} files from {tree}")


def run(tree, out):
    env = dict(os.environ, RNNT_HIP_LIB=os.path.join(ROOT, "rnntransducer_amd", "csrc", "librnnt_hip.so"))
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--dump", tree, out]
    r = subprocess.run(cmd, cwd=tree, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        print(r.stdout[-3000:])
        sys.exit(f"FAILED ({r.returncode}): {' '.join(cmd)}")
    print(r.stdout.strip().splitlines()[-1])


def differing(a, b):
    """-> (all names, those whose bytes differ, those missing on one side)"""
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    bad, missing = [], []
    for n in names:
        pa, pb = os.path.join(a, n), os.path.join(b, n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"{n} MISSING on one side"); missing.append(n)
        elif open(pa, "rb").read() != open(pb, "rb").read():
            bad.append(n)
    return names, bad, missing


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--dump":
        return dump(sys.argv[2], sys.argv[3])
    if len(sys.argv) != 3:
        sys.exit("usage: python tools/search_host_parity.py OTHER_TREE OUTDIR")
    other, out = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    dirs = [os.path.join(out, d) for d in ("other_1", "other_2", "main")]
    for tree, d in zip((other, other, ROOT), dirs):
        run(tree, d)
    _, unstable, missing = differing(dirs[0], dirs[1])
    for n in unstable:
        print(f"not reproducible between two runs of {other}, left out: {n}")
    names, bad, missing_main = differing(dirs[0], dirs[2])
    bad = [n for n in bad if n not in unstable]
    for n in bad:
        print(f"{n} DIFFERS")
    missing = sorted(set(missing) | set(missing_main))
    used = [n for n in names if n not in unstable and n not in missing]
    print(f"{len(used) - len(bad)} of {len(used)} files bytewise equal ({len(unstable)} left out, {len(missing)} missing)")
    sys.exit(1 if bad or missing or any("stream_" in n for n in unstable) else 0)


if __name__ == "__main__":
    main()
