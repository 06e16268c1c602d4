#!/usr/bin/env python3
"""BUILD CONTAINER ONLY (imports /root/reference): the checkpoint this package's `Trainer.fit_epochs` wrote on the GPU box
(tests/golden/ckpt_trained_nano.npz, made by tools/make_ckpt_fixture.py) loads into the REFERENCE's `Stlt` with strict=True
(src/inference.py:59-61) and the reference's CPU forward reproduces the logits the package computed from it on the GPU."""
import argparse, hashlib, importlib, json, os, sys, warnings
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
synth = importlib.import_module("revisiting-spatial-temporal-layouts_amd.synth")


def check(reference="/root/reference", path=None, config="nano", tol=1e-4):
    sys.path.insert(0, os.path.join(reference, "src"))
    sys.dont_write_bytecode = True
    warnings.filterwarnings("ignore")
    from modelling.configs import StltModelConfig
    from modelling.models import Stlt, StltBackbone

    z = np.load(path or os.path.join(ROOT, "tests", "golden", f"ckpt_trained_{config}.npz"))
    sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
    model = Stlt(StltModelConfig(**synth.model_kwargs(config)))
    model.load_state_dict(sd, strict=True)  # raises on any missing / unexpected key or shape
    model.train(False)
    val = [synth.fit_batch("val", 0, i) for i in range(synth.FIT_TASK["val_batches"])]
    with torch.no_grad():
        got = torch.cat([model(b)["stlt"] for b in val]).numpy()
    err = float(np.abs(got - z["__logits__"]).max())
    # the backbone file the trainer writes next to it = the same tensors without the prefix (src/train.py:152 -> models.py:130-134)
    bb = StltBackbone(StltModelConfig(**synth.model_kwargs(config)))
    bb.load_state_dict({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, strict=True)
    labels = torch.cat([b["labels"] for b in val]).numpy()
    top1 = float((got.argmax(1) == labels).mean())
    return {"keys": len(sd), "max_abs_logit_diff": err, "top1_reference_forward": top1, "top1_recorded_last_saved": float(z["__top1__"][z["__saved_epochs__"]][-1]),
            "ok": err <= tol and abs(top1 - float(z["__top1__"][z["__saved_epochs__"]][-1])) < 1e-9,
            "logits": got, "checkpoint_digest": checkpoint_digest(sd), "schema": {"stlt": _schema(model), "backbone": _schema(bb)}}


def _schema(module):
    """{name: [shape, dtype]} of a module's state dict: what load_state_dict(strict=True) compares, plus the dtypes."""
    return {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in module.state_dict().items()}


def checkpoint_digest(sd):
    """sha1 over the checkpoint's tensors in name order (ties a recorded reference result to one checkpoint)."""
    h = hashlib.sha1()
    for k in sorted(sd):
        v = sd[k].contiguous()
        h.update(k.encode())
        h.update(str(v.dtype).encode())
        h.update(v.numpy().tobytes())
    return h.hexdigest()


def write_golden(r, config="nano"):
    """What the reference's own model reported for the checkpoint, stored as a data fixture for the suite (no reference needed there):
    tests/golden/ckpt_trained_<config>_reference.npz (its logits) and ..._reference_schema.json (its state-dict schemas, the digest)."""
    base = os.path.join(ROOT, "tests", "golden", f"ckpt_trained_{config}_reference")
    np.savez_compressed(base + ".npz", logits=r["logits"].astype(np.float32))
    with open(base + "_schema.json", "w") as f:
        json.dump({"made_by": "tools/check_ckpt_roundtrip.py --write-golden", "checkpoint": f"tests/golden/ckpt_trained_{config}.npz",
                   "checkpoint_digest": r["checkpoint_digest"], "top1_reference_forward": r["top1_reference_forward"], **r["schema"]}, f, indent=1, sort_keys=True)
        f.write("\n")
    return base


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--path", default=None)
    ap.add_argument("--config", default="nano")
    ap.add_argument("--write-golden", action="store_true", help="also store the reference's result as tests/golden/ckpt_trained_<config>_reference.*")
    a = ap.parse_args()
    r = check(a.reference, a.path, a.config)
    if a.write_golden and r["ok"]:
        print("wrote", write_golden(r, a.config))
    print({k: v for k, v in r.items() if k not in ("logits", "schema")})
    sys.exit(0 if r["ok"] else 1)
