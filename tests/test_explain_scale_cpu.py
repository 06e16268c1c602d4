"""The cases of tests/explain_scale_cases.py held to the three conditions of tests/scale_cases.py without a GPU — every reference is
finite, the rows of an output cover all of it, torch's fp32 error E_t stays within 256 u in every group — and, on fp32 emulations on the
CPU, that the rule rejects the lazy forms on the cases named for them while it passes the sound form beside each: a softmax without the
maximum subtracted, exp as exp2 of a rounded product on the selected-tail rows, a rollout chain started from the old R[i,j], and a
single-accumulator position sum."""
import pytest
import torch

import explain_scale_cases as E
import scale_cases as SC

IDS = [f"{n}-{'-'.join(str(a) for a in args)}" if args else n for n, _, args in E.ALL_CASES]


@pytest.mark.parametrize("name,make,args", E.ALL_CASES, ids=IDS)
def test_case_keeps_the_three_conditions(name, make, args):
    case = make(*args)
    bad = []
    for key, o in case["outs"].items():
        assert o.ref.dtype == torch.float64 and o.ref.dim() == 2 and len(o.group) == o.ref.shape[0]
        bad += [f"{key}: {b}" for b in SC.conditions(o)]
        for g, e in SC.yardstick(o).items():
            print(f"[scale] {name} {args} {key} | {g} | E_t/u {e / SC.U:.2f}")
    assert not bad, "\n".join(bad)


def test_rows_cover_every_element():
    case = E.attention_map_case(7, 33, 64, False)
    S, Lq, Lk = E.N_SEQ, 7, 33
    assert case["outs"]["probabilities per head"].ref.shape == (S * E.H * Lq, Lk) and case["outs"]["abar"].ref.shape == (S * Lq, Lk)
    assert E.attention_map_case(7, 33, 64, False, 16)["outs"]["abar"].ref.shape == (16 * S * Lq, Lk)
    r = E.rollout_case(65)
    assert r["outs"]["R"].ref.numel() == r["abar"][0].numel() and r["outs"]["relevance"].ref.numel() == 5 * 65 * E.N_OBJ
    j = E.joint_case(7, 33, True)
    assert j["outs"]["R"].ref.numel() == 5 * 40 * 40 and j["outs"]["appearance relevance"].ref.shape == (5, 33)
    for C in E.CAM_C:
        c = E.cam_case(33, C, "ncdhw")
        assert c["g"].shape == (3, C, 33) and sorted(set(c["index"]["alpha"].reshape(-1).tolist())) == list(range(3 * C))
        assert c["outs"]["alpha"].ref.shape[0] == 9 and c["outs"]["hirescam relu"].ref.shape == (3, 33)
    e = E.embed_bwd_case(768, True)
    assert e["outs"]["d_boxes"].ref.numel() == 37 * 4 and e["outs"]["d_scores"].ref.numel() == 37
    assert E.upsample_case(1)["outs"]["map"].ref.shape == (3, 8 * 16 * 16)


def test_the_designed_rows_are_what_they_claim():
    """The selected tail: the peak key's gradient is negative and every positive entry of a row lies 20 to 40 score units below the peak;
    the single-key sequence has probability exactly 1; the masked sequence is zeros; every visible score is far inside -1e29."""
    for Lq, Lk, dh, causal, reps in E.ATTENTION_CASES:
        case = E.attention_map_case(Lq, Lk, dh, causal, reps)
        pr = case["outs"]["probabilities per head"].ref.reshape(-1, E.H, Lq, Lk)
        ab = case["outs"]["abar"].ref.reshape(-1, Lq, Lk)
        assert bool((pr[5] == 0).all()) and bool((ab[5] == 0).all())
        assert bool((pr[6].amax(-1) == 1.0).all())
        tail = pr[7]
        band = tail[tail > 0]
        assert bool((ab[7][:, 0] == 0).all())
        if Lk > 1:
            low = band[band < 0.5]
            assert low.numel() and float(low.max()) <= 2.1e-9 and float(low.min()) >= 1e-18
            assert float(ab[7].amax()) > 0 and float(ab[7].amax()) < 1e-8
        scores = torch.einsum("sihd,sjhd->shij", case["q"].double().reshape(-1, Lq, E.H, dh), case["k"].double().reshape(-1, Lk, E.H, dh)) / dh ** 0.5
        assert float(scores.abs().max()) < 1e4


@pytest.mark.parametrize("Lq,Lk,dh,causal,reps", [c for c in dict.fromkeys(E.ATTENTION_CASES) if c[4] == 1])
def test_softmax_without_the_maximum_subtracted_is_rejected(Lq, Lk, dh, causal, reps):
    """exp overflows from scores of 89 on: rows at q / k 5.5 and 17 come out as NaN -> 0 or inf; the shifted form passes every row."""
    case = E.attention_map_case(Lq, Lk, dh, causal, reps)
    o = case["outs"]["probabilities"]
    assert SC.judge("cpu emulation, shifted softmax", E.lazy_softmax_probs(case, True), o)[1] == []
    fails = SC.judge("cpu emulation, softmax without the maximum", E.lazy_softmax_probs(case, False), o)[1]
    assert any("17" in f for f in fails) and all("q/k 5.5" in f or "q/k 17" in f for f in fails)


@pytest.mark.parametrize("Lq,Lk,dh,causal,reps", [c for c in dict.fromkeys(E.ATTENTION_CASES) if c[2] == 64 and c[4] == 1 and c[1] >= 17])
def test_exp2_of_a_rounded_product_is_rejected_on_the_selected_tail(Lq, Lk, dh, causal, reps):
    """x * log2(e) rounded to fp32 at x = -20 .. -40 is off by up to ulp(58) / 2 = 2^-19, a relative error of exp of 1.3e-6 = 22 u, and it
    lands on the row's largest element.  Carrying the product's rounding error passes.  From 17 keys on: a row of 7 keys, some masked,
    may hold no product that rounds badly (its worst row: 3.6 u against a bar of 8 u)."""
    case = E.attention_map_case(Lq, Lk, dh, causal, reps)
    o = case["outs"]["abar"]
    assert SC.judge("cpu emulation, exp2 with the carried error", E.lazy_exp_abar(case, True), o)[1] == []
    fails = SC.judge("cpu emulation, exp2 of the rounded product", E.lazy_exp_abar(case, False), o)[1]
    assert any("selected tail" in f for f in fails), fails


@pytest.mark.parametrize("L", [64, 65])
def test_rollout_chain_started_from_the_old_value_is_rejected(L):
    """At map scale 1e-2 the diagonal of R is 1 + 1e-2: L products of 1e-4 .. 1e-2 each round at the magnitude of 1 when the chain starts
    there, once when the sum is added last."""
    case = E.rollout_case(L)
    o = case["outs"]["R"]
    assert SC.judge("cpu emulation, old value added last", E.rollout_by(E.chain_added_last, case["abar"]), o)[1] == []
    fails = SC.judge("cpu emulation, chain started from the old value", E.rollout_by(E.chain_from_old, case["abar"]), o)[1]
    assert any("maps 0.01" in f for f in fails), fails


def test_single_accumulator_position_sum_is_rejected():
    """1000 positions (CAM_LONG): one accumulator rounds every addition at the running sum's magnitude and misses the bar in several
    groups, by 1.5 to 2.5 times; the kernels' order (chunks of 32 on four accumulators, the partials added in turn) stays under it.  At
    the 100 positions of CAM_P a single accumulator is 2 to 4.2 times torch's error, at or under the bar: too short to tell."""
    case = E.cam_case(*E.CAM_LONG, "ndhwc")
    o = case["outs"]["alpha"]
    idx = case["index"]["alpha"]
    g = case["g"]
    assert SC.judge("cpu emulation, torch's own mean", E.indexed(g.mean(1), idx), o)[1] == []
    assert SC.judge("cpu emulation, chunks of 32 on four accumulators", E.indexed(E.chunked_mean(g), idx), o)[1] == []
    e_k, _ = SC.row_errors(E.indexed(E.single_accumulator_mean(g), idx), o.ref)
    e_t = SC.yardstick(o)
    share = [e / (SC.MARGIN * max(e_t[grp], SC.U)) for e, grp in zip(e_k.tolist(), o.group)]
    print("[scale] cpu emulation, one accumulator: share of the bar by group", [round(x, 2) for x in share])
    assert sum(x > 1.5 for x in share) >= 3, share
