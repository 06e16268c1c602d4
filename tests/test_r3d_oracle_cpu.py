"""The R3D-50 oracle (oracle/r3d_oracle.py) pinned to the reference on CPU, at the golden shape (2, 32, 112, 112): its float64 run against
the reference's float64 run stored in tests/golden/r3d.npz (features, the five stage probes) and tests/golden/r3d_train.npz (the res_* part:
loss, per-conv gradient samples and norms, classifier gradients).

The goldens hold float64 values rounded to float32, so each comparison allows 4 · 2^-24 · max|golden array| (two float32 ulps of the
array's largest entry): twice the storage rounding, far above the float64 runs' own difference and far below any real error."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from oracle import r3d_oracle as O

EPS32 = 2.0 ** -24
BOUND_ULPS = 4


def _bound(arr) -> float:
    return BOUND_ULPS * EPS32 * float(np.abs(np.asarray(arr, dtype=np.float64)).max())


@pytest.fixture(scope="module")
def case(synth):
    gold, meta = load_golden("r3d")
    sd = synth.make_r3d_state_dict({k: tuple(v["shape"]) for k, v in meta["keys"].items()}, seed=meta["weight_seed"])
    video = synth.make_video(meta["clips"], seed=meta["video_seed"])
    return sd, video, gold


@pytest.fixture(scope="module")
def fwd(case):
    sd, video, _ = case
    return O.forward(sd, video, torch.float64, with_stages=True)


def test_conv_keys_match_the_package(pkg, case):
    sd, _, _ = case
    trunk = pkg.modelling.resnet3d.make_trunk()
    names = {id(m): n for n, m in trunk.named_modules()}
    want = ["resnet." + names[id(c)] + ".weight" for c, _ in pkg.modelling.resnet3d.trunk_convs(trunk)]
    assert O.conv_weight_keys() == want and len(want) == 53
    assert {k for k in sd if k.startswith("resnet.")} == {"resnet." + k for k in trunk.state_dict()}


def test_features_against_float64_golden(case, fwd):
    _, _, gold = case
    want = gold["features_f64"].astype(np.float64)
    got = fwd["features"].numpy()
    assert got.shape == want.shape
    err, bound = np.abs(got - want).max(), _bound(want)
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("stage", O.STAGES)
def test_stage_probes_against_float64_golden(case, fwd, stage):
    _, _, gold = case
    t = fwd["stages"][stage]
    assert list(t.shape) == gold[f"{stage}_shape"].tolist()
    mean = t.mean(dim=(0, 2, 3, 4)).numpy()
    want_mean = gold[f"{stage}_mean"].astype(np.float64)
    assert np.abs(mean - want_mean).max() <= _bound(want_mean), stage
    idx = torch.from_numpy(gold[f"{stage}_idx"].astype(np.int64))
    val = t.reshape(-1)[idx].numpy()
    want_val = gold[f"{stage}_val"].astype(np.float64)
    assert np.abs(val - want_val).max() <= _bound(want_val), stage


@pytest.fixture(scope="module")
def res_grads(case):
    sd, video, _ = case
    gold = np.load(os.path.join(GOLDEN, "r3d_train.npz"))
    labels = torch.from_numpy(gold["labels"].astype(np.int64))
    return O.weight_grads(sd, video, torch.float64, labels=labels), gold


def test_loss_and_conv_gradients_against_float64_golden(res_grads):
    out, gold = res_grads
    loss = float(gold["res_loss"])
    assert abs(out["loss"] - loss) <= BOUND_ULPS * EPS32 * abs(loss)
    grads = out["grads"]
    assert len(grads) == 53
    bad = []
    for i, g in enumerate(grads):
        gmax = float(gold["res_gmax"][i])
        idx = torch.from_numpy(gold[f"res_g{i}_idx"].astype(np.int64))
        err = np.abs(g.reshape(-1)[idx].numpy() - gold[f"res_g{i}_val"].astype(np.float64)).max()
        err_max = abs(g.abs().max().item() - gmax)
        norm = float(gold["res_norm"][i])
        err_norm = abs(g.norm().item() - norm)
        if err > BOUND_ULPS * EPS32 * gmax or err_max > BOUND_ULPS * EPS32 * gmax or err_norm > BOUND_ULPS * EPS32 * norm:
            bad.append((i, err / gmax, err_max / gmax, err_norm / norm))
    assert not bad, bad


def test_classifier_gradients_against_float64_golden(res_grads):
    out, gold = res_grads
    want_b = gold["res_cls_bias"].astype(np.float64)
    assert np.abs(out["classifier.bias"].numpy() - want_b).max() <= _bound(want_b)
    idx = torch.from_numpy(gold["res_cls_w_idx"].astype(np.int64))
    want_w = gold["res_cls_w_val"].astype(np.float64)
    assert np.abs(out["classifier.weight"].reshape(-1)[idx].numpy() - want_w).max() <= _bound(want_w)
