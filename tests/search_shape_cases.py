"""Shared inputs of the search kernels' shape-edge tests (CPU: tests/test_search_shapes_oracle.py, GPU:
tests/test_gpu_search_shapes.py): prediction nets and joints at hidden / output sizes off the 256-column pass of `matvec`, with
8 layers, and with more tokens than the 1024 threads of a search workgroup; the cases; and for every search the seed at which the
float64 restatement keeps a decision margin >= MARGIN (fp32 against fp64 scores differ by about 1e-6).  The CPU test asserts
that every case finds its seed, so the GPU tests are never the first to see a case.  References are computed once per process
and shared; nobody modifies them.

No encoder anywhere: the searches take encoder outputs (or the encoder half A of the logits) directly.  Parameters are created in
fp32 and the float64 reference is a copy of them, so the device holds exactly the reference's numbers."""
import copy
import functools
import math
import time

import torch
import torch.nn.functional as F

from tests.beam_restatement import _step, beam_search_one
from tests.beam_stream_restatement import BeamStreamRef
from tests.fusion_restatement import fused_beam_search_one
from tests.timed_restatement import GreedyTimedRef

MARGIN = 1e-4
SEEDS = range(20)
CELLS = {"lstm": 0, "gru": 1, "rnn_tanh": 2, "rnn_relu": 3}   # RNNT_CELL_*
THREADS = 1024   # DEC_THREADS: a V-wide loop takes a second pass past it


# ---- models ----------------------------------------------------------------------------------------------------------
def make_rnn(cell: str, Hp: int, L: int) -> torch.nn.Module:
    if cell == "lstm":
        return torch.nn.LSTM(Hp, Hp, L, batch_first=True)
    if cell == "gru":
        return torch.nn.GRU(Hp, Hp, L, batch_first=True)
    return torch.nn.RNN(Hp, Hp, L, nonlinearity=cell[4:], batch_first=True)


def flat_weights(rnn):
    """[w_ih, w_hh, b_ih, b_hh] per layer, as the ops take them."""
    return [getattr(rnn, f"{n}_l{l}").detach() for l in range(rnn.num_layers) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


class PredNet(torch.nn.Module):
    def __init__(self, V, Hp, L, cell, O):
        super().__init__()
        self.embedding = torch.nn.Embedding(V, Hp)
        self.rnn = make_rnn(cell, Hp, L)
        self.out_proj = torch.nn.Linear(Hp, O)


class SearchNet(torch.nn.Module):
    """What the restatements read of a model: .decoder.{embedding, rnn, out_proj} and .fc over cat(enc, dec)."""

    def __init__(self, V, Hp, L, cell, O, Oe):
        super().__init__()
        self.decoder = PredNet(V, Hp, L, cell, O)
        self.fc = torch.nn.Linear(Oe + O, V)
        self.cell, self.Oe = cell, Oe


def search_net(V, Hp, L, cell, O, Oe, seed, blank=0, scale=3.0, fc_scale=6.0, peaks=(), peak=0.0, dec_scale=1.0, blank_peak=None):
    """fp32 SearchNet scaled as tests/test_stream_oracle.make_oracle scales its oracle (so that a search emits real tokens), with
    fc.bias raised by `peak` on the tokens `peaks` and by `blank_peak` (default `peak`) on the blank, and the prediction-net half of
    fc times dec_scale."""
    torch.manual_seed(seed)
    net = SearchNet(V, Hp, L, cell, O, Oe).eval()
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.mul_(fc_scale if n.startswith("fc.") else scale)
        net.decoder.embedding.weight[blank].zero_()
        net.fc.weight[:, Oe:] *= dec_scale
        for k in peaks:
            net.fc.bias[k] += peak
        net.fc.bias[blank] += peak if blank_peak is None else blank_peak
    return net


def double_net(net):
    return copy.deepcopy(net).double()


def ops_weights(net, device):
    """The positional arguments of the ops-level searches after enc_tm: fc_w, fc_b, emb_w, rnn_weights, cell, out_w, out_b."""
    d = net.decoder
    to = lambda t: t.detach().to(device).contiguous()  # noqa: E731
    return (to(net.fc.weight), to(net.fc.bias), to(d.embedding.weight), [to(w) for w in flat_weights(d.rnn)], CELLS[net.cell],
            to(d.out_proj.weight), to(d.out_proj.bias))


def enc_rows(T, B, Oe, seed, scale=2.0):
    """(T, B, Oe) fp32 encoder outputs, time-major."""
    return scale * torch.randn(T, B, Oe, generator=torch.Generator().manual_seed(500 + seed))


# ---- 1. the batched prediction-net step ------------------------------------------------------------------------------
# (Hp, L, cell): every Hp once with one LSTM layer (4: one live lane in all; 252 / 508: the last lane of a pass idle; 260 / 516 /
# 1028: one live lane in the last pass), all four cells and 3 / 8 layers at 60 and 260, and 8 GRU layers at 1024, whose
# (2 * 8 + 9) * 1024 * 4 = 102400 B of LDS need the opt-in above 64 KiB
STEP_CASES = [(Hp, 1, "lstm") for Hp in (4, 8, 60, 252, 256, 260, 508, 516, 1024, 1028)]
STEP_CASES += [(Hp, 1, cell) for Hp in (60, 260) for cell in ("gru", "rnn_tanh", "rnn_relu")]
STEP_CASES += [(60, 3, "gru"), (60, 8, "lstm"), (260, 3, "rnn_relu"), (260, 8, "lstm"), (516, 3, "rnn_tanh"), (1028, 2, "gru"),
               (1024, 8, "gru")]
STEP_B, STEP_V = 3, 11
DEC_MAX_LDS = 160 * 1024
# lds = (2 L + 9) * Hp * 4: with 8 layers 100 * Hp bytes.  The largest Hp that fits, and the next multiple of 4
STEP_LDS_FITS, STEP_LDS_OVER = (8, 1636, "rnn_tanh", 2), (8, 1640, "rnn_tanh", 2)   # (L, Hp, cell, B)


def step_lds_bytes(L, Hp):
    return (2 * L + 9) * Hp * 4


def step_case(Hp, L, cell, B=STEP_B, V=STEP_V, seed=0):
    """-> (emb (V,Hp) fp32, rnn fp32 (torch's own initialisation), tokens (B,) with token 0 and the embedding's last row,
    (h_in, c_in) (L,B,Hp) fp32 random nonzero, want): want = three float64 (h, c) pairs (c None unless LSTM): the step from no
    state, the step from that step's state, and the step from (h_in, c_in).  Not cached: the largest weigh 200 MB."""
    torch.manual_seed(1000 * L + Hp + seed)
    rnn = make_rnn(cell, Hp, L).eval()
    emb = torch.randn(V, Hp)
    tokens = torch.tensor(([0, V - 1, V // 2] * B)[:B])
    h_in, c_in = 0.5 * torch.randn(L, B, Hp), 0.5 * torch.randn(L, B, Hp)
    ref = copy.deepcopy(rnn).double()
    x = emb.double()[tokens][:, None]   # (B, 1, Hp)
    lstm = cell == "lstm"
    with torch.no_grad():
        _, s1 = ref(x, None)
        _, s2 = ref(x, s1)
        _, s3 = ref(x, (h_in.double(), c_in.double()) if lstm else h_in.double())
    want = [(s if lstm else (s, None)) for s in (s1, s2, s3)]
    return emb, rnn, tokens, (h_in, c_in), want


# ---- 2. greedy search with timing ------------------------------------------------------------------------------------
# name -> (Hp, O, Oe, V, L, cell, blank, T, lens).  Oe a multiple of 4 keeps fc.weight[:, Oe:] 16-byte aligned.  lens None: every
# utterance has T frames.  V = 2 has one token beside the blank and a repeated token is not appended twice, so such a search can
# emit one token only: T = 2 there.
GREEDY_CASES = {
    "h4_o4_v2_lstm": (4, 4, 4, 2, 1, "lstm", 0, 2, None),
    "h260_o12_v65_gru_blank64": (260, 12, 20, 65, 1, "gru", 64, 12, [12, 0, 1]),
    "h516_o260_v72_lstm2": (516, 260, 8, 72, 2, "lstm", 0, 10, None),
    "h1028_o36_v1030_relu_blank1029": (1028, 36, 12, 1030, 1, "rnn_relu", 1029, 12, None),
    "h1024_o320_v72_lstm8": (1024, 320, 320, 72, 8, "lstm", 0, 8, None),   # 104 KB of LDS
    "h60_o8_v7_gru8_blank3": (60, 8, 8, 7, 8, "gru", 3, 12, None),
}
GREEDY_B, GREEDY_MAX_ITERS = 3, 3


def greedy_lds_bytes(L, Hp, O, V):
    return (2 * L * Hp + 9 * Hp + O + V + 40) * 4


def _greedy_peaks(V, blank):
    """Tokens whose fc.bias is raised with the blank's when V > 1024, on both sides of the second pass of a V-wide loop."""
    return [k for k in (3, 700, 1023, 1024, 1026, V - 1, V - 2) if k != blank and k < V][:6] if V > THREADS else []


def greedy_try(name, seed):
    """-> (net fp32, enc (T,B,Oe) fp32, lens, ref: GreedyTimedRef in float64 after the whole search)."""
    Hp, O, Oe, V, L, cell, blank, T, lens = GREEDY_CASES[name]
    peaks = _greedy_peaks(V, blank)
    net = search_net(V, Hp, L, cell, O, Oe, seed, blank, peaks=peaks, peak=3.0 if peaks else 1.0, dec_scale=2.0)
    enc = enc_rows(T, GREEDY_B, Oe, seed)
    lens = list(lens) if lens is not None else [T] * GREEDY_B
    ref = GreedyTimedRef(double_net(net), GREEDY_B, blank, GREEDY_MAX_ITERS)
    for b, n in enumerate(lens):
        ref.search(b, enc[:n, b].double())
    return net, enc, lens, ref


def greedy_ok(name, lens, ref):
    V = GREEDY_CASES[name][3]
    if ref.margin < MARGIN or any(2 * len(ref.tokens[b]) < n for b, n in enumerate(lens)):
        return False
    return V <= THREADS or any(k >= THREADS for toks in ref.tokens for k in toks)


@functools.lru_cache(maxsize=None)
def greedy_case(name):
    """-> (seed, net, enc, lens, ref, seconds of the reference) at the first seed that qualifies, or None."""
    for seed in SEEDS:
        t0 = time.perf_counter()
        net, enc, lens, ref = greedy_try(name, seed)
        if greedy_ok(name, lens, ref):
            return seed, net, enc, lens, ref, time.perf_counter() - t0
    return None


# ---- 3. exact ties of the frame argmax -------------------------------------------------------------------------------
# V = 1100, Hp = 64, O = 8.  name -> (tie group, blank).  The members of a group have the same row of w_d (the prediction-net half of
# the joint) and the same column of A, so their logits are equal bit for bit; on the frames TIE_FRAMES a constant in A lifts the
# group above every other token.
TIE_V, TIE_HP, TIE_O, TIE_T, TIE_B = 1100, 64, 8, 8, 2
TIE_LIFT = 40.0
TIE_FRAMES = (0, 2, 3, 5, 7)
TIE_CASES = {
    "neighbouring_lanes": ((37, 38), 0),
    "two_waves": ((37, 101), 0),
    "two_passes_of_a_thread": ((37, 1061), 0),
    "three_way": ((37, 38, 101, 1061), 0),
    "blank_lowest": ((37, 38, 1061), 37),
    "blank_highest": ((37, 101, 1061), 1061),
}


def tie_try(name, seed):
    """-> (net fp32 with fc = (V, O): its weight IS w_d, A (T,B,V) fp32, want [(tokens, frames)] per utterance, margin): the greedy
    loop in float64 on A with torch.argmax (lowest index among equal maxima); margin = the smallest gap between the winner and the
    best token that is not one of its twins."""
    group, blank = TIE_CASES[name]
    net = search_net(TIE_V, TIE_HP, 1, "lstm", TIE_O, 0, seed, blank, dec_scale=2.0)   # Oe = 0: fc.weight is the prediction-net half
    g = torch.Generator().manual_seed(700 + seed)
    A = 3.0 * torch.randn(TIE_T, TIE_B, TIE_V, generator=g)
    lo, twins = group[0], list(group[1:])
    with torch.no_grad():
        net.fc.weight[twins] = net.fc.weight[lo].clone()
    A[:, :, twins] = A[:, :, lo:lo + 1].clone()
    for t in TIE_FRAMES:
        A[t, :, list(group)] += TIE_LIFT
    ref = double_net(net)
    w_d, A64 = ref.fc.weight.detach(), A.double()
    want, margin, wins = [], math.inf, 0
    with torch.no_grad():
        for b in range(TIE_B):
            d, st = _step(ref.decoder, blank, None)
            last, toks, frames = blank, [], []
            for t in range(TIE_T):
                for _ in range(GREEDY_MAX_ITERS):
                    c = w_d @ F.gelu(d, approximate="tanh")
                    c[twins] = c[lo].clone()  # one row, one sum: the twins' ties are exact here as on the device
                    z = A64[t, b] + c
                    k = int(torch.argmax(z))
                    rest = z.clone()
                    rest[list(group) if k in group else [k]] = -math.inf
                    margin = min(margin, float(z[k] - rest.max()))
                    wins += k == lo
                    if k == blank:
                        break
                    if k != last:
                        toks.append(k)
                        frames.append(t)
                        last = k
                    d, st = _step(ref.decoder, k, st)
            want.append((toks, frames))
    return net, A, want, margin, wins


@functools.lru_cache(maxsize=None)
def tie_case(name):
    """-> (seed, net, A, want, margin, evaluations the group won) at the first seed with a margin, or None."""
    for seed in SEEDS:
        net, A, want, margin, wins = tie_try(name, seed)
        if margin >= MARGIN and wins >= TIE_B * len(TIE_FRAMES) and all(len(t) >= 2 for t, _ in want):
            return seed, net, A, want, margin, wins
    return None


# ---- 4. best-first beam search with V > 1024 -------------------------------------------------------------------------
# name -> (Hp, O, V, beam, improved, cell, lens, what fc.bias[blank] has over the peaked tokens).  fc.bias is peaked on the blank and
# on six tokens, three below 1024 and three at or above it, and the joint's weights are small beside the peak, so the expand_beam
# threshold keeps children from both passes of the children loop and no others, and the pop count stays small (an un-peaked
# model at V = 1100 takes 15 s per restated search).  The improved search pops until the best of A lies state_beam = 4.6 below the
# best of B: with the blank as likely as a token that is thousands of pops a frame, with the blank e^3 times as likely a few dozen.
BEAM_CASES = {
    "h260_v1100_b4_improved_lstm": (260, 12, 1100, 4, True, "lstm", [3, 2], 2.5),
    "h64_v2049_b3_improved_gru": (64, 8, 2049, 3, True, "gru", [3, 2], 2.5),
    "h260_v1100_b2_plain_lstm": (260, 12, 1100, 2, False, "lstm", [2, 2], 1.0),
}
BEAM_OE, BEAM_PEAK, BEAM_FC_SCALE = 8, 9.0, 2.0
FUSED_CASE = "h260_v1100_b4_improved_lstm"


def stream_schedule(lens):
    """Chunks of 1 and 2 frames in turn, [(T_c, [n_b])]: lens [3, 2] -> [(1, [1, 1]), (2, [2, 1])]."""
    left, out, Tc = list(lens), [], 1
    while any(left):
        ns = [min(Tc, n) for n in left]
        out.append((Tc, ns))
        left, Tc = [n - k for n, k in zip(left, ns)], 3 - Tc
    return out


def beam_peaks(V):
    return [5, 400, 1023, 1024, 1030, V - 1]


def beam_caps(V):
    """Explicit caps no case reaches: a frame of max_pops pops leaves fewer than max_pops * V entries in A."""
    return dict(max_pops=64, max_candidates=64 * V, max_states=192, max_nodes=2048, max_len=32)


def bigram_fusion(V, blank, seed, weight=0.3):
    from rnntransducer_amd import TokenFusion
    logp = torch.log_softmax(torch.randn(V, V, generator=torch.Generator().manual_seed(2000 + seed)), dim=1)
    return TokenFusion.from_bigram(logp, weight, blank)


def beam_model(name, seed):
    Hp, O, V, beam, improved, cell, lens, blank_over = BEAM_CASES[name]
    net = search_net(V, Hp, 1, cell, O, BEAM_OE, seed, 0, fc_scale=BEAM_FC_SCALE, peaks=beam_peaks(V), peak=BEAM_PEAK,
                     blank_peak=BEAM_PEAK + blank_over)
    return net, enc_rows(max(lens), len(lens), BEAM_OE, seed)


def _wide(nbests):
    """The n-best lists hold a token of either pass of the children loop."""
    toks = [k for nb in nbests for y, *_ in nb for k in y]
    return any(k >= THREADS for k in toks) and any(0 < k < THREADS for k in toks)


@functools.lru_cache(maxsize=None)
def beam_case(name):
    """Offline -> (seed, net, enc (T,B,Oe), want [nbest [(y, score)]] per utterance, margin, pops, seconds of the slowest
    restated search) at the first seed whose margin is >= MARGIN, whose n-best holds a token >= 1024 and whose searches pop more
    than twice per frame, and at which the streaming restatement keeps the margin too; or None."""
    Hp, O, V, beam, improved, cell, lens, _ = BEAM_CASES[name]
    for seed in SEEDS:
        net, enc = beam_model(name, seed)
        ref = double_net(net)
        want, margin, pops, secs = [], math.inf, 0, 0.0
        with torch.no_grad():
            for b, n in enumerate(lens):
                t0 = time.perf_counter()
                nb, m, st = beam_search_one(ref, enc[:n, b].double(), 0, beam, improved)
                secs = max(secs, time.perf_counter() - t0)
                want.append(nb)
                margin, pops = min(margin, m), pops + st["pops"]
        if margin >= MARGIN and _wide(want) and pops > 2 * sum(lens) and _stream_restated(name, net, enc)[1] >= MARGIN:
            return seed, net, enc, want, margin, pops, secs
    return None


def _stream_restated(name, net, enc):
    """The streaming restatement fed stream_schedule(lens), its n-best asked for after every chunk (those sorts count towards the
    margin) -> (per chunk the n-best per stream, margin)."""
    Hp, O, V, beam, improved, cell, lens, _ = BEAM_CASES[name]
    ref = BeamStreamRef(double_net(net), len(lens), 0, beam, improved)
    pos, out = [0] * len(lens), []
    with torch.no_grad():
        for _, ns in stream_schedule(lens):
            for b, n in enumerate(ns):
                for t in range(pos[b], pos[b] + n):
                    ref.hyps[b] = ref._frame(enc[t, b].double(), ref.hyps[b])
                pos[b] += n
            out.append([ref.nbest(b) for b in range(len(lens))])
    assert pos == lens
    return out, ref.margin


@functools.lru_cache(maxsize=None)
def beam_stream_case(name):
    """Streaming, at the offline case's seed -> (want_after_chunk: per chunk of stream_schedule(lens) the n-best per stream, margin)."""
    seed, net, enc = beam_case(name)[:3]
    return _stream_restated(name, net, enc)


@functools.lru_cache(maxsize=None)
def fused_case():
    """The fused offline search of FUSED_CASE with a bigram TokenFusion -> (seed, net, enc, fusion, want [nbest [(y, asr_score,
    fused_score)]], margin, pops, seconds) at the first seed that qualifies as in beam_case, or None."""
    Hp, O, V, beam, improved, cell, lens, _ = BEAM_CASES[FUSED_CASE]
    for seed in SEEDS:
        net, enc = beam_model(FUSED_CASE, seed)
        fusion = bigram_fusion(V, 0, seed)
        ref = double_net(net)
        want, margin, pops, secs = [], math.inf, 0, 0.0
        with torch.no_grad():
            for b, n in enumerate(lens):
                t0 = time.perf_counter()
                nb, m, st = fused_beam_search_one(ref, enc[:n, b].double(), fusion, 0, beam, improved, max_pops=64)
                secs = max(secs, time.perf_counter() - t0)
                want.append(nb)
                margin, pops = min(margin, m), pops + st["pops"]
        if margin >= MARGIN and _wide(want) and pops > 2 * sum(lens):
            return seed, net, enc, fusion, want, margin, pops, secs
    return None
