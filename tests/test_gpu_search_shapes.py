"""The search kernels' shared device code (csrc/decode_shared.hpp: matvec, prednet_cells, prednet_joint_half, frame_argmax,
token_logp; csrc/beam_shared.hpp: the children loop) at the shapes where it can go wrong: hidden and output sizes off the 256
columns of a matvec pass (4, 60, 252, 260, 508, 516, 1028), 8 layers, dynamic LDS above 64 KiB and at the 160 KiB limit, more
tokens than the 1024 threads of a workgroup in the best-first beam search, and exact ties of the frame argmax.

Every comparison is against float64 on the same fp32 weights (tests/search_shape_cases.py; tests/test_search_shapes_oracle.py
checks the cases without a GPU).  Buffers this module hands to an entry are prefilled with NaN / 0xFF bytes, and the blocks the
ops will allocate for their outputs are left holding NaN, so an element an entry does not write shows."""
import ctypes as C
import math

import pytest
import torch

from tests import search_shape_cases as sc

pytestmark = pytest.mark.gpu
FWD_ATOL = 2e-5          # the project's forward bound against float64 (tests/test_gpu_stream_shapes.py, tests/test_gpu_lstm.py)
LOGP_ATOL = 2 * 2e-5     # tests/test_gpu_timed.py's bound on a token's logp
DEV = "cuda"


def _leave_nan(*shape):
    """The caching allocator hands a freed block to the next request of its size: the ops' torch.empty outputs start as NaN."""
    torch.full(shape, math.nan, device=DEV)


# ---- 1. rnnt_hip_prednet_step ----------------------------------------------------------------------------------------
def _run_step(Hp, L, cell, B=sc.STEP_B):
    from rnntransducer_amd import ops
    emb, rnn, tokens, (h_in, c_in), want = sc.step_case(Hp, L, cell, B)
    lstm = cell == "lstm"
    w = [t.to(DEV).contiguous() for t in sc.flat_weights(rnn)]
    emb_d, tok_d = emb.to(DEV), tokens.to(DEV)

    def step(h, c):
        for _ in range(2 if lstm else 1):
            _leave_nan(L, B, Hp)
        return ops.prednet_step(tok_d, emb_d, w, sc.CELLS[cell], h, c)

    s1 = step(None, None)
    s2 = step(*s1)
    s3 = step(h_in.to(DEV), c_in.to(DEV) if lstm else None)
    worst = 0.0
    for i, ((h, c), (wh, wc)) in enumerate(zip((s1, s2, s3), want)):
        assert h.shape == (L, B, Hp) and (c is None) == (not lstm)
        for got, ref in ((h, wh), (c, wc)) if lstm else ((h, wh),):
            err = float((got.double().cpu() - ref).abs().max())   # NaN if anything was left unwritten
            worst = max(worst, err)
            assert err <= FWD_ATOL, (i, err)
    print(f"Hp={Hp} L={L} {cell}: largest |h, c - float64| = {worst:.3e}; LDS {sc.step_lds_bytes(L, Hp)} B")


@pytest.mark.parametrize("Hp,L,cell", sc.STEP_CASES, ids=[f"H{h}-L{l}-{c}" for h, l, c in sc.STEP_CASES])
def test_prednet_step_vs_float64(Hp, L, cell):
    _run_step(Hp, L, cell)


def test_prednet_step_at_the_lds_limit():
    """8 layers at Hp = 1636: 163600 of the 163840 B a workgroup can have, with 1024 threads.  (Hp = 1640 is refused on the host:
    tests/test_search_shapes_oracle.py.)"""
    L, Hp, cell, B = sc.STEP_LDS_FITS
    assert sc.step_lds_bytes(L, Hp) == 163600
    _run_step(Hp, L, cell, B)


# ---- 2. greedy search with timing ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.GREEDY_CASES))
def test_greedy_timed_vs_float64(name):
    from rnntransducer_amd import ops
    seed, net, enc, lens, ref, _ = sc.greedy_case(name)
    blank, T, case_lens = sc.GREEDY_CASES[name][6:9]
    t_lens = None if case_lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    tok, ntok, fr, lp = ops.greedy_decode(enc.to(DEV), *sc.ops_weights(net, DEV), blank, sc.GREEDY_MAX_ITERS, t_lens=t_lens,
                                          timing=True)
    tok, ntok, fr, lp = tok.cpu(), ntok.tolist(), fr.cpu(), lp.cpu()
    worst = 0.0
    for b in range(sc.GREEDY_B):
        n = len(ref.tokens[b])
        assert ntok[b] == n, (b, ntok[b], n)
        assert tok[b, :n].tolist() == ref.tokens[b] and fr[b, :n].tolist() == ref.frames[b], b
        err = max([abs(x - y) for x, y in zip(lp[b, :n].tolist(), ref.logp[b])] or [0.0])
        worst = max(worst, err)
        assert err <= LOGP_ATOL, (b, err)
        # nothing past ntok: the fills of ops.greedy_decode are still there
        assert bool((tok[b, n:] == blank).all()) and bool((fr[b, n:] == -1).all()) and bool((lp[b, n:] == 0).all())
    print(f"{name}: seed {seed}, {sum(ntok)} tokens, largest |logp - float64| = {worst:.3e}")


# ---- 3. exact ties of frame_argmax -----------------------------------------------------------------------------------
def _greedy_timed_on_A(net, A, blank):
    """rnnt_hip_greedy_decode_timed through its descriptor with the encoder half A of the logits handed in (no GEMM: tied columns
    of A are copies) and net.fc.weight as the whole prediction-net half -> (tokens, ntok, frames, logp) on the host; past ntok
    they hold the 0xFF bytes / NaN they were filled with."""
    from rnntransducer_amd import _lib, ops
    T, B, V = A.shape
    max_out = T * sc.GREEDY_MAX_ITERS
    dec = net.decoder
    to = lambda t: t.detach().to(DEV).contiguous()  # noqa: E731
    w_d, out_w, out_b, A_d = to(net.fc.weight), to(dec.out_proj.weight), to(dec.out_proj.bias), A.to(DEV).contiguous()
    d = _lib.DecodeDesc()
    keep = ops._fill_prednet_weights(d, to(dec.embedding.weight), [to(w) for w in sc.flat_weights(dec.rnn)], sc.CELLS[net.cell],
                                     "greedy decode")
    d.T, d.B, d.V, d.O, d.blank, d.max_iters, d.max_out = T, B, V, w_d.shape[1], blank, sc.GREEDY_MAX_ITERS, max_out
    d.w_o, d.b_o, d.w_d, d.ld_d = out_w.data_ptr(), out_b.data_ptr(), w_d.data_ptr(), w_d.shape[1]
    tokens = torch.full((B, max_out), -1, dtype=torch.int64, device=DEV)        # 0xFF bytes
    ntok = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    frames = torch.full((B, max_out), -1, dtype=torch.int32, device=DEV)
    logp = torch.full((B, max_out), math.nan, device=DEV)
    d.A, d.t_lens, d.tokens, d.ntok = A_d.data_ptr(), None, tokens.data_ptr(), ntok.data_ptr()
    tm = _lib.GreedyTiming(frames.data_ptr(), logp.data_ptr(), None)
    _lib.check(_lib.lib().rnnt_hip_greedy_decode_timed(C.byref(d), C.byref(tm), torch.cuda.current_stream().cuda_stream),
               "rnnt_hip_greedy_decode_timed")
    out = tokens.cpu(), ntok.tolist(), frames.cpu(), logp.cpu()   # (the copies wait for the kernel: the weights may go)
    del keep
    return out


@pytest.mark.parametrize("name", list(sc.TIE_CASES))
def test_frame_argmax_takes_the_lowest_of_equal_maxima(name):
    """Token rows that are copies of each other tie bit for bit, and the lowest index wins (torch.argmax).  This rests on matvec
    rounding a row's sum the same way in each of a wave's 8 row slots; before the sum was an explicit fmaf chain, blank_lowest
    emitted token 38 on a frame where the blank 37 was due."""
    seed, net, A, want, margin, wins = sc.tie_case(name)
    group, blank = sc.TIE_CASES[name]
    tokens, ntok, frames, logp = _greedy_timed_on_A(net, A, blank)
    for b, (toks, frs) in enumerate(want):
        n = ntok[b]
        got = tokens[b, :max(n, 0)].tolist()
        assert not set(got) & set(group[1:]), (b, got)     # never a higher twin
        assert n == len(toks) and got == toks and frames[b, :n].tolist() == frs, (b, got, toks)
        assert bool(torch.isfinite(logp[b, :n]).all())
        assert bool((tokens[b, n:] == -1).all()) and bool((frames[b, n:] == -1).all()) and bool(torch.isnan(logp[b, n:]).all())


# ---- 4. best-first beam search with V > 1024 -------------------------------------------------------------------------
def _same_nbest(got, want, cols=1):
    """The criterion of tests/test_gpu_beam.py: identical token lists, scores within 1e-4 * max(1, |score|)."""
    assert [[e[0] for e in h] for h in got] == [[list(e[0]) for e in h] for h in want], (got, want)
    for gh, wh in zip(got, want):
        for g, w in zip(gh, wh):
            for s, r in zip(g[1:1 + cols], w[1:1 + cols]):
                assert abs(s - r) <= 1e-4 * max(1.0, abs(r)), (g, w)


@pytest.mark.parametrize("name", list(sc.BEAM_CASES))
def test_beam_offline_vs_restatement(name):
    from rnntransducer_amd import ops
    seed, net, enc, want, margin, pops, _ = sc.beam_case(name)
    Hp, O, V, beam, improved, cell, lens, _ = sc.BEAM_CASES[name]
    t_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    got, st = ops.beam_search(enc.to(DEV), *sc.ops_weights(net, DEV), 0, beam, improved, t_lens=t_dev, stats=True, **sc.beam_caps(V))
    print(f"{name}: seed {seed}, margin {margin:.2e}, pops {st[:, 0].tolist()} (restatement: {pops}), A entries {st[:, 3].tolist()}")
    _same_nbest(got, want)
    assert int(st[:, 0].sum()) == pops


@pytest.mark.parametrize("name", list(sc.BEAM_CASES))
def test_beam_stream_vs_restatement_after_every_chunk(name):
    from rnntransducer_amd import _lib, ops
    seed, net, enc = sc.beam_case(name)[:3]
    want_after, _ = sc.beam_stream_case(name)
    Hp, O, V, beam, improved, cell, lens, _ = sc.BEAM_CASES[name]
    B, Oe = len(lens), sc.BEAM_OE
    fc_w, fc_b, emb_w, rnn_w, code, out_w, out_b = sc.ops_weights(net, DEV)
    caps = ops.beam_stream_caps(V, beam, **sc.beam_caps(V))
    d, keep = ops.beam_stream_desc(B, fc_w, emb_w, rnn_w, code, out_w, out_b, 0, beam, improved, 4.6, 2.3, caps)
    ws_bytes = ops.beam_stream_workspace_bytes(d)
    ws = torch.zeros(ws_bytes + 256, dtype=torch.uint8, device=DEV)   # carried state, zeroed as streaming.BeamStreamState does
    d.workspace, d.workspace_bytes = (ws.data_ptr() + 255) // 256 * 256, ws_bytes
    i32 = lambda *shape: torch.full(shape, -1, dtype=torch.int32, device=DEV)  # noqa: E731
    tokens, out_lens, commit = i32(B, beam, caps["max_len"]), i32(B, beam), i32(B, caps["max_nodes"])
    small = i32(3 + _lib.BEAM_NSTATS, B)   # count | status | ncommit | stats
    scores = torch.full((B, beam), math.nan, dtype=torch.float64, device=DEV)
    d.tokens, d.out_lens, d.scores, d.commit = tokens.data_ptr(), out_lens.data_ptr(), scores.data_ptr(), commit.data_ptr()
    base = small.data_ptr()
    d.count, d.status, d.ncommit, d.stats = base, base + 4 * B, base + 8 * B, base + 12 * B
    ops.beam_stream_reset(d, torch.arange(B, dtype=torch.int32, device=DEV), True)
    committed, pos = [[0] for _ in range(B)], [0] * B
    for (Tc, ns), want in zip(sc.stream_schedule(lens), want_after):
        x = torch.zeros(Tc, B, Oe)
        for b, n in enumerate(ns):
            x[:n, b] = enc[pos[b]:pos[b] + n, b]
            pos[b] += n
        A = torch.full((Tc, B, V), math.nan, device=DEV)
        ops.gemm(Tc * B, V, Oe, x.to(DEV), fc_w, A, b_sn=fc_w.shape[1], b_sk=1, bias=fc_b, flags=ops.GEMM_GELU_A)
        for t in (tokens, out_lens, commit, small):
            t.fill_(-1)
        scores.fill_(math.nan)
        ops.beam_stream_chunk(d, A, torch.tensor(ns, dtype=torch.int32, device=DEV))
        host = small.cpu()
        count, status, ncommit = host[0].tolist(), host[1].tolist(), host[2].tolist()
        assert status == [0] * B and all(c >= 1 for c in count), (status, count)
        lens_h, scores_h, tok_h, com_h = out_lens.cpu().tolist(), scores.cpu().tolist(), tokens.cpu(), commit.cpu()
        got = []
        for b in range(B):
            committed[b] += com_h[b, :ncommit[b]].tolist()
            got.append([(committed[b] + tok_h[b, r, :lens_h[b][r]].tolist(), scores_h[b][r]) for r in range(count[b])])
        _same_nbest(got, want)
    assert pos == lens
    del keep


def test_beam_fused_vs_restatement():
    from rnntransducer_amd import ops
    seed, net, enc, fusion, want, margin, pops, _ = sc.fused_case()
    Hp, O, V, beam, improved, cell, lens, _ = sc.BEAM_CASES[sc.FUSED_CASE]
    t_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    got, st = ops.beam_search(enc.to(DEV), *sc.ops_weights(net, DEV), 0, beam, improved, t_lens=t_dev, stats=True,
                              fusion=fusion.to(DEV), **sc.beam_caps(V))
    print(f"fused: seed {seed}, margin {margin:.2e}, pops {st[:, 0].tolist()} (restatement: {pops})")
    _same_nbest(got, want, cols=2)   # asr_score and fused_score
    assert int(st[:, 0].sum()) == pops


def test_beam_candidate_cap_raises_at_two_passes_and_the_next_call_succeeds():
    """max_candidates = V = 1100: the plain search's second pop of a frame adds V - 1 children to the V the first left.  The
    contract of tests/test_gpu_beam.py::test_beam_caps_raise_and_the_next_call_succeeds, with a children loop of two passes."""
    from rnntransducer_amd import ops
    from rnntransducer_amd._lib import RnntHipError
    name = "h260_v1100_b2_plain_lstm"
    seed, net, enc, want = sc.beam_case(name)[:4]
    Hp, O, V, beam, improved, cell, lens, _ = sc.BEAM_CASES[name]
    assert V == 1100 and not improved
    t_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    args = (enc.to(DEV), *sc.ops_weights(net, DEV), 0, beam, improved)
    with pytest.raises(RnntHipError, match="max_candidates"):
        ops.beam_search(*args, t_lens=t_dev, **{**sc.beam_caps(V), "max_candidates": V})
    _same_nbest(ops.beam_search(*args, t_lens=t_dev, **sc.beam_caps(V)), want)
