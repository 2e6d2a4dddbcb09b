"""Shared inputs of the fusion tests (CPU and GPU): models, automata and the cases whose decision margins were computed with
tests/fusion_restatement.py on the CPU.  tests/test_fusion_oracle.py asserts those margins, so that the GPU tests are never the
first to see a case."""
import torch

from tests import beam_restatement

# (fixture, weight, phrases, rows): restatement margins on the CPU, per row, in the comment; every kept row is >= 1e-4
FIXTURE_CASES = [
    ("b2_beams", 0.5, [[4, 6, 4]], [0, 1]),            # 5.2e-3 (top hypothesis changes), 1.1e-3
    ("b2_beams", 0.5, [[4, 5], [4, 6, 4]], [0, 1]),    # 1.6e-4, 1.1e-3: both lists change, nonzero totals in the output
    ("b1_beams", 1.5, [[4, 6, 4]], [0, 1, 2]),         # 3.8e-3, 3.7e-3, 1.1e-2: row 2's list changes
]
STREAM_PHRASES, STREAM_WEIGHT = [[4, 6, 4]], 0.5
# streams whose one-frame-at-a-time restatement keeps a margin >= 1e-4, the n-best sort after every frame included (s1 rows 0
# and 1 fall to 1.1e-5 and 8.9e-5; row 2 holds 1.9e-4 and its list changes)
STREAM_ROWS = {"s1_beams": [2], "s2_beams": [0, 1], "s3_beams": [0, 1]}

# config-2 prediction-net size (H = 512, V = 72): (cell, layers, beam, improved, automaton)
CONFIG2_CASES = [(cell, layers, beam, improved, kind)
                 for cell, layers, beam, improved in (("lstm", 1, 5, True), ("gru", 1, 5, False), ("lstm", 2, 5, True))
                 for kind in ("bigram", "hotwords")]
CONFIG2_SEEDS = range(40, 52)
# the first seed of the range whose fused restatement has a decision margin >= 1e-4 (found on the CPU; the CPU test asserts that
# margin, the GPU test starts its seed loop there)
CONFIG2_FIRST_SEED = {("lstm", 1, "bigram"): 40, ("lstm", 1, "hotwords"): 47, ("gru", 1, "bigram"): 40, ("gru", 1, "hotwords"): 40,
                      ("lstm", 2, "bigram"): 40, ("lstm", 2, "hotwords"): 51}
CONFIG2_LENS = [3, 2]
BIGRAM_WEIGHT, HOTWORD_WEIGHT = 0.3, 0.3


def zero_fusion(V):
    from rnntransducer_amd import TokenFusion
    return TokenFusion(torch.zeros(1, V, dtype=torch.int32), torch.zeros(1, V), torch.zeros(1))


def bigram_fusion(V, blank, seed, weight=BIGRAM_WEIGHT):
    from rnntransducer_amd import TokenFusion
    logp = torch.log_softmax(torch.randn(V, V, generator=torch.Generator().manual_seed(1000 + seed)), dim=1)
    return TokenFusion.from_bigram(logp, weight, blank)


def config2_model(cell, layers, seed, V=72, H=512):
    """The model and input of test_gpu_beam.test_beams_vs_restatement_config2_sizes."""
    from oracle.rnnt_oracle import OracleJointNet
    tn = dict(input_size=80, hidden_size=256, output_size=320, num_layers=1, rnn_type="lstm", dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=V, pad_token_id=0, hidden_size=H, output_size=320, num_layers=layers, rnn_type=cell, dropout=0.0)
    torch.manual_seed(seed)
    ora = OracleJointNet(tn, pn, V).eval()
    with torch.no_grad():
        for n, p in ora.named_parameters():
            p.mul_(6.0 if n.startswith("fc.") else 3.0)
        ora.decoder.embedding.weight[0].zero_()
    lens = CONFIG2_LENS
    audios = torch.randn(len(lens), max(lens), 80, generator=torch.Generator().manual_seed(seed))
    for b, t in enumerate(lens):
        audios[b, t:] = 0
    return ora, tn, pn, audios, lens


def phrases_from(unfused, blank=0):
    """Two hotword phrases that a search over a few frames meets (its hypotheses hold one or two tokens): the first token of the
    best unfused hypothesis of the first utterance that has one, alone (completed, and banked, whenever it is appended), and
    another token followed by it (begun by some hypotheses and mostly not finished: the bonus is revoked or taken back by
    `final`)."""
    t1 = next((y[1] for y, _ in unfused[0] if len(y) >= 2), 1)
    other = next(k for k in range(1, 8) if k not in (t1, blank))
    return [[t1], [other, t1]]


def config2_fusion(kind, ora, audios, lens, beam, improved, seed, V=72):
    from rnntransducer_amd import TokenFusion
    if kind == "bigram":
        return bigram_fusion(V, 0, seed)
    unfused, _, _ = beam_restatement.beam_search(ora, audios, lens, 0, beam, improved)
    return TokenFusion.from_hotwords(phrases_from(unfused), HOTWORD_WEIGHT, V, 0)


# a vocabulary larger than the workgroup: the children loop takes several passes with fusion loads
BIGV = dict(V=300, H=16, lens=[3, 2], beam=4, improved=True)
BIGV_SEEDS = range(40, 52)
BIGV_FIRST_SEED = 48   # 40..47 take a decision within 1e-4


def bigv_model(seed):
    from oracle.rnnt_oracle import OracleJointNet
    V, H = BIGV["V"], BIGV["H"]
    tn = dict(input_size=20, hidden_size=16, output_size=24, num_layers=1, rnn_type="lstm", dropout=0.0, bidirectional=True)
    pn = dict(embedding_size=V, pad_token_id=0, hidden_size=H, output_size=24, num_layers=1, rnn_type="lstm", dropout=0.0)
    torch.manual_seed(seed)
    ora = OracleJointNet(tn, pn, V).eval()
    with torch.no_grad():
        for n, p in ora.named_parameters():
            p.mul_(6.0 if n.startswith("fc.") else 3.0)
        ora.decoder.embedding.weight[0].zero_()
    lens = BIGV["lens"]
    audios = torch.randn(len(lens), max(lens), 20, generator=torch.Generator().manual_seed(seed))
    for b, t in enumerate(lens):
        audios[b, t:] = 0
    return ora, tn, pn, audios, lens


def config2_first_seed(cell, layers, beam, improved, kind, seeds=None):
    """The first seed of the range whose fused restatement has a decision margin >= 1e-4 -> (seed, n-best, fusion), or
    (None, None, None).  A runaway frame (more than 1024 pops, the kernel's default cap) disqualifies a seed too."""
    from tests import fusion_restatement
    for seed in (CONFIG2_SEEDS if seeds is None else seeds):
        ora, tn, pn, audios, lens = config2_model(cell, layers, seed)
        fusion = config2_fusion(kind, ora, audios, lens, beam, improved, seed)
        try:
            want, margin, _, _ = fusion_restatement.fused_beam_search(ora, audios, lens, fusion, 0, beam, improved, max_pops=1024)
        except RuntimeError:
            continue
        if margin >= 1e-4:
            return seed, want, fusion
    return None, None, None


def bigv_first_seed(seeds=None):
    from tests import fusion_restatement
    for seed in (BIGV_SEEDS if seeds is None else seeds):
        ora, tn, pn, audios, lens = bigv_model(seed)
        fusion = bigram_fusion(BIGV["V"], 0, seed)
        want, margin, _, _ = fusion_restatement.fused_beam_search(ora, audios, lens, fusion, 0, BIGV["beam"], BIGV["improved"],
                                                                  max_pops=1024)
        if margin >= 1e-4:
            return seed, want, fusion
    return None, None, None
