"""The CPU beam-search restatement (tests/beam_restatement.py) vs fixtures produced by the REFERENCE's
JointNet.recognize_beams (tests/golden/b*_beams.npz, made by tests/golden/make_golden_beams.py)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import beam_restatement

FIXTURES = ["b1_beams", "b2_beams", "b3_beams", "b4_beams", "b5_beams"]


def load_fixture(golden_dir, tag):
    g = dict(np.load(os.path.join(golden_dir, tag + ".npz")))
    cfg = json.loads(str(g["config"]))
    sd = {k[6:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    return g, cfg, sd


def fixture_nbest(g):
    return [[g["tokens"][b, r, :g["lens"][b, r]].tolist() for r in range(n)] for b, n in enumerate(g["count"].tolist())]


@pytest.mark.parametrize("tag", FIXTURES)
def test_restatement_matches_reference_fixture(golden_dir, tag):
    from oracle.rnnt_oracle import OracleJointNet
    g, cfg, sd = load_fixture(golden_dir, tag)
    net = OracleJointNet(cfg["transnet"], cfg["prednet"], cfg["V"])
    net.load_state_dict(sd)
    net.eval()
    blank = cfg["prednet"]["pad_token_id"]
    audios, t_list = torch.from_numpy(g["audios"]), g["t_lens"].tolist()
    got, margin, _ = beam_restatement.beam_search(net, audios, t_list, blank, cfg["beam"], cfg["improved"], cfg["state_beam"],
                                                  cfg["expand_beam"])
    want = fixture_nbest(g)
    assert [[y for y, _ in h] for h in got] == want
    assert margin >= 1e-4
    # scores: fp32 log-probs from another CPU's kernels may differ in the last bits; the decisions may not (margin above)
    got_scores = np.array([[s for _, s in h] + [0.0] * (g["scores"].shape[1] - len(h)) for h in got])
    assert np.allclose(got_scores, g["scores"], rtol=1e-5, atol=1e-5)
    for hyps in want:   # every y_star starts with the blank and never repeats a token back to back (the dedupe rule)
        assert all(y[0] == blank and all(a != b for a, b in zip(y[1:], y[2:])) for y in hyps)


def test_fixtures_cover_the_required_cases(golden_dir):
    seen = set()
    for tag in FIXTURES:
        g, cfg, _ = load_fixture(golden_dir, tag)
        pn = cfg["prednet"]
        seen.add((pn["rnn_type"], pn["num_layers"] > 1, cfg["improved"]))
        if pn["pad_token_id"] != 0:
            seen.add("blank!=0")
        if cfg["beam"] == 1:
            seen.add("beam1")
        if cfg["beam"] >= 100:
            seen.add("wide")
    assert {("lstm", False, True), ("lstm", True, False), "blank!=0", "beam1", "wide"} <= seen, seen


def test_restatement_counts_dedupe_pops_on_a_fixture(golden_dir):
    """b1 is kept only if a child whose token equals y_star[-1] (same y_star, new state) is popped somewhere."""
    from oracle.rnnt_oracle import OracleJointNet
    g, cfg, sd = load_fixture(golden_dir, "b1_beams")
    net = OracleJointNet(cfg["transnet"], cfg["prednet"], cfg["V"])
    net.load_state_dict(sd)
    net.eval()
    _, _, stats = beam_restatement.beam_search(net, torch.from_numpy(g["audios"]), g["t_lens"].tolist(), 0, cfg["beam"],
                                               cfg["improved"])
    assert sum(s["dedupe_pops"] for s in stats) > 0
