"""Generates tests/golden/s*_beams.npz from the REFERENCE's own JointNet.recognize_beams on UNIDIRECTIONAL encoders, the
only ones that can be streamed (all b*_beams fixtures are bidirectional).  Same recipe, checks and file format as
make_golden_beams.py, whose `run` / `first_kept` it reuses: a seed is kept only if the CPU restatement reproduces the
reference's lists and its decision margin is >= 1e-4.

Run ONLY where the reference sources are available:  REFERENCE=/path/to/reference python tests/golden/make_golden_beams_uni.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_beams import first_kept, run  # noqa: E402,F401

ENC_UNI = dict(input_size=12, hidden_size=16, output_size=8, num_layers=1, rnn_type="lstm", dropout=0.0, bidirectional=False)
SCALE = dict(fc=3.0, rest=2.0)


def pred(rnn_type, V, layers=1, blank=0):
    return dict(embedding_size=V, pad_token_id=blank, hidden_size=16, output_size=8, num_layers=layers, rnn_type=rnn_type, dropout=0.0)


if __name__ == "__main__":
    only = sys.argv[1:]
    if not only or "s1" in only:   # S1: 2-layer LSTM encoder, the reference's inference setting (improved, beam 5), ragged
        first_kept("s1_beams", dict(ENC_UNI, num_layers=2), pred("lstm", 10), 10, [24, 17, 9], seeds=range(21, 61), scale=SCALE,
                   beam=5, improved=True)
    if not only or "s2" in only:   # S2: GRU encoder, 2-layer LSTM prediction net, not improved (few frames)
        first_kept("s2_beams", dict(ENC_UNI, rnn_type="gru"), pred("lstm", 8, layers=2), 8, [6, 4], seeds=range(23, 63),
                   scale=SCALE, beam=3, improved=False)
    if not only or "s3" in only:   # S3: Elman encoder, GRU prediction net with blank = 3, improved
        first_kept("s3_beams", dict(ENC_UNI, rnn_type="rnn"), pred("gru", 10, blank=3), 10, [16, 11], seeds=range(25, 65),
                   scale=SCALE, beam=4, improved=True)
