"""Scripted beam search: Attention:BeamSearch (Attention.lua:332-438) driven by a prescribed table of
log-probabilities instead of a decoder, so the search is a pure function of the table and its bookkeeping
(survivor order, parent gather, finished slots, tie-breaks) can be compared exactly.

script_table draws the table on a grid of 1/4 in [-3.25, 0]: a running score is a sum of at most 301 such
values, below 1000 in magnitude, so it is exact in fp32 (and in float64), ties are exact and scores compare
bitwise.  reference_search is a plain Python restatement of the search for one utterance, with a trace of every
decision; events counts the situations the tests must reach.  Host only (numpy)."""
import numpy as np

GRID = 0.25
LOW = -3.25


def script_table(rng, B, K, O, maxlen, eos, eos_rates=(0.15, 0.7), neg_inf=()):
    """float64 (maxlen + 1, B, K, O) log-probabilities for (count, utterance, hypothesis row, token): values
    -j/4, j = 1..13.  The eos column is high (0, -1/4 or -1/2) with utterance b's probability -- spread evenly
    over eos_rates = (lowest, highest), so the utterances of a batch finish at different counts -- and low
    (-3.25) otherwise.  neg_inf: tokens scripted to -inf in every row.  Not normalised: the search never
    needs it."""
    assert 0 <= eos < O and eos not in neg_inf and O - len(neg_inf) >= K
    t = -GRID * rng.integers(1, 14, size=(maxlen + 1, B, K, O)).astype(np.float64)
    rates = np.linspace(eos_rates[0], eos_rates[1], B)
    high = rng.random((maxlen + 1, B, K)) < rates[None, :, None]
    t[..., eos] = np.where(high, -GRID * rng.integers(0, 3, size=high.shape), LOW)
    for j in neg_inf:
        t[..., j] = -np.inf
    return t


def reference_search(table_b, eos, K, maxlen):
    """The search of one utterance under its (maxlen + 1, K, O) table: hypothesis row j at a count is the j-th
    survivor of the previous count's sorted selection (count 0: the one zero-state row 0).  Returns
    (finished, prediction, score, trace): finished = [(sequence, score)] in finishing order, prediction / score
    = the first maximum of it, trace = one dict per count with
      active    rows extended at this count,
      parents   parent row of each survivor, in survivor (= next count's row) order,
      tokens    the token each survivor appended,
      finished  [(parent row, token, "eos" | "maxlen")] in finishing order,
      cut_tie   the last candidate taken and the first one left out score the same and have different parents,
      done      the utterance is done after this count,
      at_maxlen count == maxlen."""
    O = table_b.shape[-1]
    beams = [([], 0.0)]  # (tokens, score) per row
    fin, trace = [], []
    for count in range(maxlen + 1):
        cands = []
        for i, (_, p) in enumerate(beams):
            for j in range(O):
                cands.append((float(table_b[count, i, j]) + p, i, j))
        # torch.topk, sorted, ties to the lower flat index (the candidates are generated in flat-index order
        # and Python's sort is stable)
        ranked = sorted(cands, key=lambda c: -c[0])
        take = K - len(fin)
        chosen = ranked[:K][:take]
        step = {"count": count, "at_maxlen": count == maxlen, "active": len(beams), "parents": [], "tokens": [],
                "finished": [],
                "cut_tie": len(ranked) > take and ranked[take - 1][0] == ranked[take][0]
                and ranked[take - 1][1] != ranked[take][1]}
        new = []
        for v, i, j in chosen:
            seq = beams[i][0] + [j]
            if j == eos or count == maxlen:
                fin.append((seq, v))
                step["finished"].append((i, j, "eos" if j == eos else "maxlen"))
            else:
                new.append((seq, v))
                step["parents"].append(i)
                step["tokens"].append(j)
        beams = new
        step["done"] = len(fin) >= K or count >= maxlen
        trace.append(step)
        if step["done"]:
            break
    best = 0
    for f in range(1, len(fin)):
        if fin[f][1] > fin[best][1]:
            best = f
    return fin, fin[best][0], fin[best][1], trace


def events(trace):
    """Counts, for one utterance's trace, the situations the scripted tests must reach."""
    ev = {"multi_finish": 0, "cut_tie": 0, "shared_parent": 0, "parents_out_of_order": 0}
    reasons = set()
    for st in trace:
        ev["multi_finish"] += len(st["finished"]) >= 2
        ev["cut_tie"] += bool(st["cut_tie"])
        par = st["parents"]
        ev["shared_parent"] += len(set(par)) < len(par)
        ev["parents_out_of_order"] += any(a > b for a, b in zip(par, par[1:]))
        reasons |= {r for _, _, r in st["finished"]}
    last = trace[-1]
    ev["forced_and_eos"] = int(reasons == {"eos", "maxlen"})
    # done between two of the host's every-fourth-count polls: the device steps on past a finished utterance
    ev["done_off_poll"] = int(last["count"] % 4 != 3 and not last["at_maxlen"])
    return ev


def long_finished(finished, n=257):
    return sum(len(seq) > n for seq, _ in finished)


class StatefulScript:
    """decoder_mlp for oracle.s2s_oracle.beam_search: ignores its input and returns table_b[count, row] by
    counting its own calls -- one at count 0, then one per active hypothesis per count in row order (active:
    the rows per count, from the reference trace).  Keeps every input it was handed as seen[(count, row)]."""

    def __init__(self, table_b, active):
        self.table, self.calls, self.seen = table_b, [(c, r) for c, n in enumerate(active) for r in range(n)], {}
        self.n = 0

    def __call__(self, v):
        c, r = self.calls[self.n]
        self.n += 1
        self.seen[(c, r)] = np.array(v, dtype=np.float64)
        return self.table[c, r]


# ----------------------------------------------------------------------------- the committed cases
# name -> (K, O, B, maxlen, eos, seed, eos_rates, neg_inf); tables are script_table(default_rng(seed), ...)
CASES = {
    "stride310": (5, 62, 64, 12, 23, 101, (0.15, 0.7), ()),    # 310 candidates: the stride past 256 threads
    "maxk992": (16, 62, 16, 9, 61, 102, (0.15, 0.7), ()),      # 992 candidates, the widest beam
    "k1": (1, 11, 32, 6, 2, 103, (0.15, 0.7), ()),
    "k_eq_o": (7, 7, 16, 5, 0, 104, (0.15, 0.7), ()),          # K = outputDepth, the API's bound
    "long300": (4, 29, 8, 300, 3, 105, (0.002, 0.006), ()),    # histories and finished sequences past 256 tokens
    "maxlen1": (3, 11, 8, 1, 2, 106, (0.15, 0.7), ()),
    "neginf": (5, 20, 16, 8, 4, 107, (0.15, 0.7), (0, 7, 8, 19)),
    "gather": (4, 11, 5, 8, 2, 108, (0.1, 0.3), ()),           # the state-gather tests' steering
}


def case_table(name):
    K, O, B, maxlen, eos, seed, rates, neg = CASES[name]
    return script_table(np.random.default_rng(seed), B, K, O, maxlen, eos, rates, neg)


def hand_tables():
    """name -> (table (maxlen + 1, B, K, O), eos, K, maxlen): the hand cases.
    all_equal: every log-probability 0 (eos = O - 1 >= K is never among the first K).
    no_eos: eos scripted to -inf, so K hypotheses run to maxlen + 1 tokens.
    eos_first: K = 1; utterance 0 has eos alone on top at count 0 and finishes as [eos], while utterances
    1 and 2 never see eos and run to maxlen."""
    rng = np.random.default_rng(7)
    out = {}
    out["all_equal"] = (np.zeros((7, 2, 4, 9)), 8, 4, 6)
    t = script_table(rng, 3, 3, 9, 5, 2)
    t[..., 2] = -np.inf
    out["no_eos"] = (t, 2, 3, 5)
    t = script_table(rng, 3, 1, 9, 9, 4)
    t[..., 4] = -np.inf
    t[0, 0, 0, :] = -1.0
    t[0, 0, 0, 4] = -0.25
    out["eos_first"] = (t, 4, 1, 9)
    return out
