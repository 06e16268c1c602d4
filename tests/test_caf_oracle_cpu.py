"""The fusion oracle's fp64 and dropout-masked modes (oracle/caf_oracle.py) on the CPU: the fp64 run reproduces the
reference's goldens, a masked run at p = 0 is the unmasked one, and the attention mask for Lq != Lk keeps the square
case's numbers.  The GPU sweep (test_fusion_train_gpu.py) trusts these modes."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_case
from oracle import caf_oracle as CO
from oracle import stlt_oracle as O

FWD = {"caf": CO.caf_forward, "cacnf": CO.cacnf_forward, "lcf": CO.lcf_forward}


def _golden_case(synth, model_name):
    z = np.load(os.path.join(GOLDEN, f"{model_name}_cfg1.npz"))
    meta = json.load(open(os.path.join(GOLDEN, f"{model_name}_cfg1_schema.json")))
    c = synth.CONFIGS["cfg1"]
    sd = synth.make_state_dict({k: tuple(v) for k, v in meta["keys"].items()}, seed=meta["weight_seed"])
    batch = synth.make_batch(meta["batch"], c["T"], c["N"], seed=meta["input_seed"])
    batch["appearance_features"] = synth.make_appearance_features(meta["batch"], seed=meta["feature_seed"])
    return z, sd, batch, c["num_attention_heads"]


@pytest.mark.parametrize("model_name", ["caf", "cacnf", "lcf"])
def test_fp64_oracle_matches_the_reference_goldens(synth, model_name):
    """The goldens are the reference's fp32 logits: the fp64 oracle sits within their own rounding (|z| * 2^-24 per op,
    a few e-6 here) — bound 1e-5 — and no farther from them than the fp32 oracle plus that bound."""
    z, sd, batch, H = _golden_case(synth, model_name)
    with torch.no_grad():
        o64 = FWD[model_name](sd, batch, H, dtype=torch.float64)
        o32 = FWD[model_name](sd, batch, H)
    assert set(o64) == set(z.files)
    for k in z.files:
        assert o64[k].dtype == torch.float64, k
        d64 = np.abs(o64[k].numpy() - z[k]).max()
        d32 = np.abs(o32[k].numpy() - z[k]).max()
        assert d64 <= 1e-5 and d64 <= d32 + 1e-5, (k, d64, d32)


@pytest.mark.parametrize("layout", ["tape", "ops", "frozen"])
@pytest.mark.parametrize("model_name", ["caf", "cacnf", "lcf"])
def test_masked_oracle_at_p0_is_the_unmasked_oracle(synth, model_name, layout, monkeypatch):
    z, sd, batch, H = _golden_case(synth, model_name)
    with torch.no_grad():
        plain = FWD[model_name](sd, batch, H, dtype=torch.float64)
        # hidden_dropout_prob = 0 leaves the appearance encoder's fixed 0.1: two block calls per appearance layer (2 here) draw
        calls = O.CallSeeds(range(1, 1000), layout)
        app_only = FWD[model_name](sd, batch, H, dtype=torch.float64, drop=calls, p=0.0)
        assert [k for k, _, _ in calls.log] == ["attn", "ffn"] * 2 and [s for _, _, s in calls.log] == [1, 2, 3, 4]
        assert max((app_only[k] - plain[k]).abs().max().item() for k in plain) > 1e-3
        # with that rate at 0 too, nothing draws and the masked oracle is the unmasked one, bit for bit
        monkeypatch.setattr(CO, "APPEARANCE_DROPOUT", 0.0)
        calls = O.CallSeeds(range(1, 1000), layout)
        masked = FWD[model_name](sd, batch, H, dtype=torch.float64, drop=calls, p=0.0)
    assert not calls.log
    for k in plain:
        assert torch.equal(masked[k], plain[k]), k


def test_layout_op_level_masks_at_p0_and_the_call_sequence(synth):
    """StltBackbone.forward_train's op-level schedule in the oracle: p = 0 is the plain backbone; p > 0 takes one seed per
    DropoutFn / block call in forward order (embedding dropout, two blocks per spatial layer, frames dropout, two per temporal
    layer) and differs from the tape's single-seed masks."""
    sd, batch, z, meta = golden_case("cfg1")
    with torch.no_grad():
        plain = O.backbone_forward(sd, batch, 4, prefix="backbone.", dtype=torch.float64)
        calls = O.CallSeeds(range(5, 100), "ops")
        same = O.backbone_forward(sd, batch, 4, prefix="backbone.", dtype=torch.float64, drop=calls, drop_p=0.0)
        assert not calls.log and torch.equal(same, plain)
        calls = O.CallSeeds(range(5, 100), "ops")
        ops = O.backbone_forward(sd, batch, 4, prefix="backbone.", dtype=torch.float64, drop=calls, drop_p=0.2)
        tape = O.backbone_forward(sd, batch, 4, prefix="backbone.", dtype=torch.float64, drop=O.Dropout(0.2, 5))
    B, T, N = batch["categories"].shape
    kinds = ["dropout"] + ["attn", "ffn"] * 4 + ["dropout"] + ["attn", "ffn"] * 8
    assert [k for k, _, _ in calls.log] == kinds
    assert [s for _, _, s in calls.log] == list(range(5, 5 + len(kinds)))
    assert calls.log[1][1] == (B * T, N, N) and calls.log[-2][1] == (B, T, T) and calls.log[-1][1] == (B * T,)
    assert (ops - plain).abs().max().item() > 1e-2 and (ops - tape).abs().max().item() > 1e-2


def _attention_square_before(drop: O.Dropout, site: int, probs: torch.Tensor) -> torch.Tensor:
    """Dropout.attention as it was for square attention only: idx = (((s*L+i)*H + h) << 8) | j."""
    S, H, L, _ = probs.shape
    s_, h_, i_, j_ = np.meshgrid(np.arange(S, dtype=np.uint64), np.arange(H, dtype=np.uint64),
                                 np.arange(L, dtype=np.uint64), np.arange(L, dtype=np.uint64), indexing="ij")
    idx = ((((s_ * np.uint64(L) + i_) * np.uint64(H)) + h_) << np.uint64(8)) | j_
    keep = O.dropout_keep(drop.p, drop.seed, site, idx)
    return probs * (torch.from_numpy(keep).to(probs.dtype) * drop.scale)


@pytest.mark.parametrize("S,H,L", [(3, 4, 7), (2, 12, 33), (1, 1, 1), (2, 2, 65), (1, 3, 256)])
def test_general_attention_mask_keeps_the_square_numbers(S, H, L):
    probs = torch.rand(S, H, L, L, dtype=torch.float64, generator=torch.Generator().manual_seed(L))
    d = O.Dropout(0.3, 1234567 + L)
    assert torch.equal(d.attention(0x400000, probs), _attention_square_before(d, 0x400000, probs))


@pytest.mark.parametrize("S,H,Lq,Lk", [(2, 4, 17, 5), (3, 2, 9, 33), (1, 12, 65, 100)])
def test_cross_attention_mask_index_is_the_kernels(S, H, Lq, Lk):
    """Lq != Lk: element (s, h, i, j) is kept iff stlt_keep(idx) with idx = ((query token * H + head) << 8) | key position and
    query token = s * Lq + i (attn_any.hip, bwd_api.hip) — spelled out per element here, not through the vectorised form."""
    probs = torch.ones(S, H, Lq, Lk, dtype=torch.float64)
    d = O.Dropout(0.4, 77 + Lk)
    got = d.attention(0x400000, probs)
    rng = np.random.default_rng(Lq)
    for _ in range(64):
        s, h, i, j = (int(rng.integers(n)) for n in (S, H, Lq, Lk))
        idx = np.array([(((s * Lq + i) * H + h) << 8) | j], dtype=np.uint64)
        keep = bool(O.dropout_keep(0.4, 77 + Lk, 0x400000, idx)[0])
        assert got[s, h, i, j].item() == (d.scale if keep else 0.0), (s, h, i, j)
    # a query token's mask does not depend on Lk (the key-side count only bounds j): the square case's row prefix
    sq = d.attention(0x400000, torch.ones(S, H, Lq, Lq, dtype=torch.float64))
    n = min(Lq, Lk)
    assert torch.equal(sq[..., :n], got[..., :n])


def test_appearance_grid_default_is_unchanged(synth):
    a = synth.make_appearance_features(3, seed=11)
    assert a.shape == (3, 2048, 2, 4, 4)
    assert torch.equal(a, synth.make_appearance_features(3, seed=11, grid=(2, 4, 4)))
    b = synth.make_appearance_features(2, seed=11, grid=(1, 2, 4), channels=64)
    assert b.shape == (2, 64, 1, 2, 4) and b.min().item() >= 0.0
    # the same stream, cut to the grid's length: the first clip's first values agree with the default grid's
    assert torch.equal(b.flatten()[:64], synth.make_appearance_features(2, seed=11, channels=64).flatten()[:64])
