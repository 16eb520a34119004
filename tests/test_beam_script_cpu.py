"""The scripted-search helper (tests/beam_script.py) against the oracle's beam search, the coverage its
committed tables must reach, and the hand cases.  No GPU: tests/test_gpu_decode.py compares the device with
reference_search on these same tables."""
import numpy as np
import pytest

import beam_script as bs
from oracle import s2s_oracle as orc


def _tiny_decoder(O):
    """A GRU decoder of width 4: its arithmetic is irrelevant, the scripted mlp ignores it."""
    rng = np.random.default_rng(0)
    S = A = Sc = 4
    cfg = orc.ModelConfig(inputFrameSize=2, hiddenFrameSize=2, outputFrameSize=A // 2, scoreDepth=Sc, stateDepth=S,
                          outputDepth=O, mlpDepth=1, maxoutWindow=1, numLayers=1)
    shapes = dict(orc.param_shapes(cfg))
    P = {n: rng.standard_normal(shapes[n]) * 0.1 for n in ("V", "Ws", "bs", "we", "Wy", "by", "Wc", "bc", "Wd", "bd",
                                                           "dec.Wz", "dec.Wr", "dec.Wh")}
    return cfg, P, rng.standard_normal((3, A))


def _same_as_oracle(table, eos, K, maxlen):
    cfg, P, h = _tiny_decoder(table.shape[-1])
    for b in range(table.shape[1]):
        fin, pred, score, trace = bs.reference_search(table[:, b], eos, K, maxlen)
        mlp = bs.StatefulScript(table[:, b], [st["active"] for st in trace])
        ofin = []
        oseq, oscore = orc.beam_search(h, P, cfg, eos, K, maxlen, mlp=mlp, finished=ofin)
        assert mlp.n == len(mlp.calls), (b, mlp.n, len(mlp.calls))  # the oracle extended exactly the traced rows
        assert list(oseq) == pred and oscore == score, (b, oseq, pred, oscore, score)
        assert [(list(s), p) for s, p in ofin] == fin, b
        assert np.float64(np.float32(score)) == score  # the grid keeps every score exact in fp32


@pytest.mark.parametrize("name", sorted(bs.CASES))
def test_reference_search_equals_oracle_on_committed_tables(name):
    K, O, B, maxlen, eos = bs.CASES[name][:5]
    table = bs.case_table(name)
    assert table.shape == (maxlen + 1, B, K, O)
    finite = table[np.isfinite(table)]
    assert finite.min() >= -3.25 and finite.max() <= 0 and (finite * 4 == np.round(finite * 4)).all()
    _same_as_oracle(table, eos, K, maxlen)


@pytest.mark.parametrize("name", sorted(bs.hand_tables()))
def test_reference_search_equals_oracle_on_hand_tables(name):
    table, eos, K, maxlen = bs.hand_tables()[name]
    _same_as_oracle(table, eos, K, maxlen)


def _case_events(name):
    K, O, B, maxlen, eos = bs.CASES[name][:5]
    table = bs.case_table(name)
    out = []
    for b in range(B):
        fin, _, _, trace = bs.reference_search(table[:, b], eos, K, maxlen)
        out.append((bs.events(trace), fin, trace))
    return out


def test_committed_tables_reach_the_coverage_conditions():
    """Over the union of the committed cases (the hand cases and the gather steering aside): every situation
    the bookkeeping can be wrong in occurs at least once; asserted from the reference's trace alone."""
    total = {}
    for name in sorted(set(bs.CASES) - {"gather"}):
        for ev, _, _ in _case_events(name):
            for k, v in ev.items():
                total[k] = total.get(k, 0) + v
    print(total)
    for k in ("multi_finish", "cut_tie", "shared_parent", "parents_out_of_order", "forced_and_eos",
              "done_off_poll"):
        assert total[k] >= 1, (k, total)


def test_utterances_of_a_batch_finish_at_different_counts():
    for name in ("stride310", "k1", "k_eq_o", "neginf"):
        last = {tr[-1]["count"] for _, _, tr in _case_events(name)}
        assert len(last) >= 3, (name, last)


def test_long_case_finishes_hypotheses_past_257_tokens():
    per = _case_events("long300")
    assert sum(bs.long_finished(fin) for _, fin, _ in per) >= 1
    # and not only by running into maxlen: an eos finish past 257 tokens copies a long history too
    assert any(len(s) > 257 and s[-1] == bs.CASES["long300"][4] and len(s) < 301 for _, fin, _ in per for s, _ in fin)


def test_neg_inf_tokens_are_never_chosen():
    K, O, B, maxlen, eos, _, _, neg = bs.CASES["neginf"]
    for _, fin, _ in _case_events("neginf"):
        assert len(fin) == K
        for seq, score in fin:
            assert np.isfinite(score) and not set(seq) & set(neg)


def test_gather_steering_shares_and_permutes_parents():
    per = _case_events("gather")
    assert sum(ev["shared_parent"] for ev, _, _ in per) >= 1
    assert sum(ev["parents_out_of_order"] for ev, _, _ in per) >= 1
    # an utterance already done while others continue
    assert len({tr[-1]["count"] for _, _, tr in per}) >= 2


def test_hand_all_equal_selects_tokens_in_index_order():
    table, eos, K, maxlen = bs.hand_tables()["all_equal"]
    fin, pred, score, trace = bs.reference_search(table[:, 0], eos, K, maxlen)
    assert trace[0]["tokens"] == list(range(K)) and trace[0]["parents"] == [0] * K
    for st in trace[1:-1]:  # every later count: row 0's tokens 0..K-1, the lowest flat indices
        assert st["parents"] == [0] * K and st["tokens"] == list(range(K))
    assert [s for s, _ in fin] == [[0] * maxlen + [j] for j in range(K)]
    assert pred == [0] * (maxlen + 1) and score == 0.0


def test_hand_no_eos_runs_every_hypothesis_to_maxlen():
    table, eos, K, maxlen = bs.hand_tables()["no_eos"]
    for b in range(table.shape[1]):
        fin, _, _, trace = bs.reference_search(table[:, b], eos, K, maxlen)
        assert len(fin) == K and all(len(s) == maxlen + 1 and eos not in s for s, _ in fin)
        assert all(r == "maxlen" for st in trace for _, _, r in st["finished"])


def test_hand_eos_on_top_at_count_0_with_one_beam():
    table, eos, K, maxlen = bs.hand_tables()["eos_first"]
    fin, pred, score, trace = bs.reference_search(table[:, 0], eos, K, maxlen)
    assert K == 1 and fin == [([eos], -0.25)] and pred == [eos] and len(trace) == 1
    for b in (1, 2):
        assert len(bs.reference_search(table[:, b], eos, K, maxlen)[1]) == maxlen + 1
