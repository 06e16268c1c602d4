"""Per-prefix logits, host side: the two-stream restatement (tests/prefix_restated.py) equals the definition — the oracle's Stlt.forward on
`collate.prefix_batch(batch, t)` — and `prefix_batch` itself does what its words say.  fp64 against fp64, no GPU."""
import pytest
import torch

import prefix_restated as R
from oracle import stlt_oracle as O


def _case(pkg, name, B=5):
    c = pkg.synth.CONFIGS[name]
    model = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs(name)))
    sd = pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=5, gain=2.0)
    batch = pkg.synth.make_batch(B, c["T"], c["N"], dataset=c["dataset"], seed=3, min_len=2)
    return sd, batch, c["num_attention_heads"]


@pytest.mark.parametrize("name", ["micro", "cfg1", "heads", "odd"])
def test_restatement_equals_the_oracle_on_truncated_batches(pkg, name):
    """Every t, every clip that has that prefix: <= 1e-12 (fp64 against fp64; the two differ by summation order only).  The full-clip prefix
    is the ordinary forward, and the prefixes of one clip differ by far more than the bound, so mixed-up prefixes cannot pass."""
    sd, batch, H = _case(pkg, name)
    got, valid = R.forward_prefixes(sd, batch, H)
    want, valid2 = R.truncated_oracle(sd, batch, H, pkg.collate.prefix_batch)
    assert torch.equal(valid, valid2) and torch.equal(valid, torch.arange(batch["categories"].shape[1])[None] < batch["lengths"][:, None])
    assert valid.sum() == batch["lengths"].sum() and got.shape == want.shape and got.dtype == torch.float64
    err = (got - want).abs().max().item()
    print(f"{name}: lengths {batch['lengths'].tolist()} restatement vs truncated oracle {err:.3g}")
    assert err <= 1e-12
    assert (got[~valid] == 0).all()
    rows = torch.arange(got.shape[0])
    full = O.stlt_forward(sd, batch, H, dtype=torch.float64)["stlt"]
    assert (got[rows, batch["lengths"] - 1] - full).abs().max().item() <= 1e-12
    assert (got[0, 0] - got[0, -1]).abs().max().item() > 1e-3  # clip 0 is full length: its first and last prefix are different predictions


@pytest.mark.parametrize("dataset,T,N", [("something", 6, 4), ("action_genome", 5, 3)])
def test_prefix_batch_is_the_definition(pkg, dataset, T, N):
    batch = pkg.synth.make_batch(4, T, N, dataset=dataset, seed=11, min_len=2)
    batch["labels"] = torch.arange(4)
    B = 4
    keys = ["categories", "boxes", "frame_types", "src_key_padding_mask_boxes", "src_key_padding_mask_frames"] + (["scores"] if dataset == "action_genome" else [])
    assert ("scores" in batch) == (dataset == "action_genome")
    for t in range(T):
        pb = pkg.collate.prefix_batch(batch, t)
        assert torch.equal(pb["lengths"], torch.full((B,), t + 1, dtype=torch.int64)) and torch.equal(pb["labels"], batch["labels"])
        assert set(keys) <= set(pb) and ("scores" in pb) == ("scores" in batch)
        for k in keys:
            assert pb[k].shape == batch[k].shape[:1] + (t + 1,) + batch[k].shape[2:] and pb[k].dtype == batch[k].dtype and pb[k].is_contiguous(), k
            for b in range(B):
                ln = int(batch["lengths"][b])
                assert torch.equal(pb[k][b, :t], batch[k][b, :t]), (k, b, t)          # the observed frames
                assert torch.equal(pb[k][b, t], batch[k][b, ln - 1]), (k, b, t)       # ... then the clip's own extract frame
                if t == ln - 1:  # the last prefix of a clip is the clip's real frames
                    assert torch.equal(pb[k][b], batch[k][b, :ln]), (k, b)
        ext = pkg.synth.DATASETS[dataset]["extract"]
        assert (pb["frame_types"][:, t] == ext).all() and not pb["src_key_padding_mask_frames"][:, t].any()
    assert batch["categories"].shape[1] == T  # the input is not modified
    with pytest.raises(ValueError):
        pkg.collate.prefix_batch(batch, T)
    with pytest.raises(ValueError):
        pkg.collate.prefix_batch(batch, -1)
