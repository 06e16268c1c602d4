"""Checkpoint round trip (reference src/train.py:147-152 -> src/inference.py:59-69): tests/golden/ckpt_trained_nano.npz holds the tensors of
a checkpoint file that `Trainer.fit_epochs` WROTE on an MI355X after training (tools/make_ckpt_fixture.py) and the logits the package
computed from it there.  The oracle (pinned to the reference) reproduces those logits from the same tensors, and so did the reference's own
`Stlt` loaded with strict=True (its schemas and logits are stored beside the checkpoint, tests/golden/ckpt_trained_nano_reference.*,
recorded by tools/check_ckpt_roundtrip.py --write-golden); on a GPU the package's module does."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from oracle import stlt_oracle as O


def _load(pkg):
    z = np.load(os.path.join(GOLDEN, "ckpt_trained_nano.npz"))
    sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
    val = [pkg.synth.fit_batch("val", 0, i) for i in range(pkg.synth.FIT_TASK["val_batches"])]
    return z, sd, val


def test_written_checkpoint_has_the_reference_schema_and_the_oracle_reproduces_its_logits(pkg):
    z, sd, val = _load(pkg)
    model = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs("nano")))
    want = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want  # names and shapes: what load_state_dict(strict=True) checks
    assert sd["backbone.frames_embeddings.position_ids"].dtype == torch.int64
    H = pkg.synth.CONFIGS["nano"]["num_attention_heads"]
    with torch.no_grad():
        got = torch.cat([O.stlt_forward(sd, b, H)["stlt"] for b in val]).numpy()
    assert np.abs(got - z["__logits__"]).max() <= 1e-4
    # it is a TRAINED checkpoint: the weights moved away from the seeded initialisation and the saved epoch's accuracy is the recorded one
    init = pkg.synth.make_state_dict(want, seed=pkg.synth.FIT_TASK["weight_seed"])
    assert float((sd["prediction_head.fc1.weight"] - init["prediction_head.fc1.weight"]).abs().max()) > 1e-3
    labels = torch.cat([b["labels"] for b in val]).numpy()
    assert float((got.argmax(1) == labels).mean()) == float(z["__top1__"][z["__saved_epochs__"]][-1])


def test_written_checkpoint_loads_strictly_into_the_reference_model(pkg):
    """load_state_dict(strict=True) into the reference's Stlt, and into its StltBackbone for the backbone file the trainer writes beside
    it (src/train.py:152 -> models.py:130-134), compares names and shapes: the checkpoint's must be the recorded ones.  The reference's CPU
    forward from these very tensors (same digest) gave the logits the package computed on the GPU and the accuracy of the saved epoch."""
    z, sd, val = _load(pkg)
    ref = np.load(os.path.join(GOLDEN, "ckpt_trained_nano_reference.npz"))
    with open(os.path.join(GOLDEN, "ckpt_trained_nano_reference_schema.json")) as f:
        meta = json.load(f)
    spec = importlib.util.spec_from_file_location("check_ckpt_roundtrip", os.path.join(ROOT, "tools", "check_ckpt_roundtrip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.checkpoint_digest(sd) == meta["checkpoint_digest"]
    schema = lambda tensors: {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in tensors.items()}
    assert schema(sd) == meta["stlt"]
    assert schema({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}) == meta["backbone"]
    assert np.abs(ref["logits"] - z["__logits__"]).max() <= 1e-4
    labels = torch.cat([b["labels"] for b in val]).numpy()
    top1 = float((ref["logits"].argmax(1) == labels).mean())
    assert top1 == meta["top1_reference_forward"] == float(z["__top1__"][z["__saved_epochs__"]][-1])


@pytest.mark.gpu
def test_written_checkpoint_round_trips_through_the_package_module(pkg):
    z, sd, val = _load(pkg)
    model = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs("nano")))
    model.load_state_dict(sd, strict=True)
    model.train(False).to("cuda")
    with torch.no_grad():
        got = torch.cat([model({k: v.to("cuda") for k, v in b.items()})["stlt"] for b in val]).cpu().numpy()
    assert np.abs(got - z["__logits__"]).max() <= 1e-5
