"""not-gpu: every capacity case (capacity_cases.py) crosses the kernel capacities it claims, with the caps read from the source.  If a
cap is raised or the generator changes so that a case no longer crosses, this fails instead of test_gpu_capacity.py quietly losing
the second code path it exists for."""
import numpy as np
import pytest

import capacity_cases as K
import oracle_lib as O


@pytest.mark.parametrize("name", list(K.CASES))
def test_case_crosses_what_it_claims(name):
    cs = K.CASES[name]
    cap = K.caps()
    sb = K.generate(name)
    assert 1 <= sb.n_targets <= 3
    st = K.oracle_stats(sb, cs["W"])
    ev = K.insertion_events(sb, cs["W"])
    seen = {"RW_ICAP": int(st["irows"].max()), "CP_ICAP": int(st["irows"].max()), "CP_OCAP": int(st["lp"].max()),
            "QEVCAP": int(ev.max()), "FUSED_ROWS": int(st["nsup"].max())}
    print(name, {k: (seen[k], cap[k]) for k in seen})
    for k in cs["crosses"]:
        assert seen[k] > cap[k], f"{name} no longer crosses {k}: largest {seen[k]} <= {cap[k]}"
    for k in K.STAYS_UNDER.get(name, ()):
        assert seen[k] <= cap[k], f"{name} was meant to stay under {k}: largest {seen[k]} > {cap[k]}"
    if "CP_ICAP" in cs["crosses"] and "CP_OCAP" in cs["crosses"]:   # the pairing: votes in global memory AND byte stores, in ONE window
        both = (st["irows"] > cap["CP_ICAP"]) & (st["lp"] > cap["CP_OCAP"])
        assert both.any(), name


def test_corrected_window_lengths_add_up_to_the_oracle_consensus():
    """capacity_cases.corrected_window (what the GPU test takes a window's corrected length from) against the oracle's decoder: the
    windows of a target, concatenated, are the oracle's FASTA sequence, on random logits."""
    sb = K.generate("D_w2048")
    W = K.CASES["D_w2048"]["W"]
    store = O.store_from_synth(sb)
    g = np.random.default_rng(7)
    for t in range(sb.n_targets):
        rid, rows, cigs = O.target_alignments(sb, t)
        res = store.extract_features(rid, rows, cigs, W)
        wins = [res.window(wi) for wi in range(len(res))]
        lg = [g.standard_normal((len(ow.sup_pos), 5)).astype(np.float32) for ow in wins]
        want = res.consensus_fasta(np.concatenate(lg) if lg else np.zeros((0, 5), np.float32))
        seqs = [line for line in want.splitlines() if not line.startswith(">")]
        assert len(seqs) == 1
        assert b"".join(K.corrected_window(ow, l) for ow, l in zip(wins, lg)).decode() == seqs[0]
