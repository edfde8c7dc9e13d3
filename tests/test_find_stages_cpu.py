"""The inputs of tests/find_stage_cases.py are the stages they are named after: the plain models alone (tests/find_cases.py,
tests/find_del_cases.py, tests/find_snp_cases.py, tests/find_msnp_cases.py, tests/find_het_cases.py), no device.  tests/test_gpu_find_stages.py runs the same inputs through the library."""
import pytest

from tests import find_stage_cases as sc


def test_every_layer_has_every_stage_within_the_size_limits():
    for layer in sc.LAYERS:
        assert set(sc.STAGES[layer]) == set(sc.STAGE_NAMES)
        for stage, seqs in sc.STAGES[layer].items():
            assert len(seqs) <= 4 and all(len(s) <= 200 for s in seqs), (layer, stage)
    assert len(sc.ALL_LAYERS) <= 4 and all(len(s) <= 200 for s in sc.ALL_LAYERS)
    assert len(sc.UNJUDGED) == 1 and 200 < len(sc.UNJUDGED[0]) <= 320
    assert set(sc.inputs("msnp")) == set(sc.STAGE_NAMES) | {"unjudged"} and all(sc.inputs(layer) is sc.STAGES[layer] for layer in sc.LAYERS if layer != "msnp")


@pytest.mark.parametrize("layer", sc.LAYERS)
def test_each_input_is_the_stage_it_claims(layer):
    k, inputs = sc.K, sc.STAGES[layer]
    res = {stage: sc.model(layer, sc.SOLID, seqs) for stage, seqs in inputs.items()}
    positions = {stage: sum(max(len(s) - k + 1, 0) for s in seqs) for stage, seqs in inputs.items()}
    seen = "n_candidates" if layer == "het" else "n_gaps"   # what the first pass of the layer counts

    assert inputs["none"] == [] and res["none"][0] == [] and not any(res["none"][1].values())
    assert inputs["short"] and max(len(s) for s in inputs["short"]) == k - 1 and positions["short"] == 0
    assert res["short"][0] == [] and not any(res["short"][1].values())
    assert positions["in_graph"] > 100 and res["in_graph"][0] == [] and not any(res["in_graph"][1].values())
    g = sc.fc.Graph(sc.SOLID, k)
    assert all(g.contains(s[p:p + k]) for s in inputs["in_graph"] for p in range(len(s) - k + 1))

    calls, st = res["unseen"]
    assert calls == [] and st["n_candidates"] == 0
    if layer == "het":
        assert sc.in_degree_2_positions(sc.SOLID, inputs["unseen"]) > 0
    else:
        assert st["n_gaps"] > 0
        lengths = [n for _, _, n, fresh in sc.fc.gaps_by_anchors(sc.SOLID, k, inputs["unseen"]) if fresh]
        if layer == "snp":
            assert lengths and all(n != k for n in lengths)
        elif layer == "msnp":
            assert lengths and all(n <= k + sc.SNP_MIN_VAL for n in lengths)
        else:
            assert lengths and all(n > k - 1 if layer == "homo" else n < k - sc.MAX_REPEAT for n in lengths)

    calls, st = res["uncalled"]
    assert calls == [] and st["n_candidates"] > 0 and st[seen] > 0
    assert not any(v for key, v in st.items() if key not in ("n_gaps", "n_candidates"))

    calls, st = res["calls"]
    if layer == "msnp":   # several calls per gap
        recs = sc.msnp_gap_records(sc.SOLID, inputs["calls"])
        assert len(calls) >= 3 and st["n_candidates"] == len(recs) == 2 and [r[2:] for r in recs] == [(k + 7, k + 7, 2), (k + 9, k + 9, 2)]
        assert {c[2] for c in calls} == {6} and st["n_calls"] == len(calls) and st["n_full"] == 2
        return
    assert len(calls) >= 3 and st["n_candidates"] >= len(calls)
    if layer == "snp":
        assert {c[2] for c in calls} == {5} and sorted(c[0] for c in calls) == [0, 1, 2] and st["n_calls"] == 3
    elif layer == "homo":
        assert {c[2] for c in calls} == {0, 1} and {c[3] for c in calls} == {0, 2}
    elif layer == "del":
        assert {c[2] for c in calls} == {4} and sorted(c[6] for c in calls) == [5, 20, 40] and st["n_calls"] == 3
    else:
        assert {c[2] for c in calls} == {2, 3} and {c[3] for c in calls} == {0, 2}


def test_the_unjudged_input_has_a_candidate_and_nothing_to_list():
    """one candidate gap of 255 positions or more and no other candidate: counted in n_long, consumed 0, no call, no slab"""
    calls, st = sc.model("msnp", sc.SOLID, sc.UNJUDGED)
    recs = sc.msnp_gap_records(sc.SOLID, sc.UNJUDGED)
    assert calls == [] and len(recs) == 1 and recs[0][2] >= 255 and recs[0][3:] == (0, 0)
    assert st["n_candidates"] == 1 and st["n_long"] == 1 and not any(st[x] for x in ("n_calls", "n_full", "n_partial"))
    # the uncalled input is the other way round: judged, and stopped at its first step
    recs = sc.msnp_gap_records(sc.SOLID, sc.STAGES["msnp"]["uncalled"])
    assert len(recs) == 1 and k_plus(recs[0][2]) and recs[0][3:] == (0, 0)


def k_plus(length):
    """a gap the multi-SNP observer judges: longer than k + snp_min_val, shorter than 255"""
    return sc.K + sc.SNP_MIN_VAL < length < 255


def test_every_layer_calls_on_the_shared_input():
    for layer in sc.LAYERS:
        calls, st = sc.model(layer, sc.SOLID, sc.ALL_LAYERS)
        assert calls, layer
