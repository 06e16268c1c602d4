"""The end-to-end cases of the integrated-gradients tests (tests/test_integrated_gradients_cpu.py, tests/test_integrated_gradients_gpu.py):
the two seeded layouts of test_forward_saliency_equals_the_autograd_gradient_of_the_selected_logit — cfg1 at B = 4 with its short clip,
refdef at B = 2 —, steps = 4, the zero baseline, and their fp64 oracle IG, computed once per (case, target) and never modified."""
import functools
import importlib

import torch

import ig_restated as R
from conftest import PKG_NAME

CASES = [("cfg1", 4), ("refdef", 2)]
STEPS = 4
CAP = 2e-4        # the bar tests/test_layout_gradients_gpu.py holds every gradient of the path to; the weights sum to 1
LOGIT_BAR = 1e-4  # the bar the logits of every explanation call are held to against the plain forward


@functools.lru_cache(maxsize=None)
def layout_case(name, B):
    synth = importlib.import_module(PKG_NAME + ".synth")
    pkg = importlib.import_module(PKG_NAME)
    c = synth.CONFIGS[name]
    if name == "cfg1":  # the seeded batch whose clip 4 is short, as clips 1..4: B = 4 with padded frames
        batch = synth.make_batch(B + 1, c["T"], c["N"], dataset=c["dataset"], seed=77, with_scores=True)
        batch = {k: v[1:].contiguous() for k, v in batch.items()}
    else:
        batch = synth.make_batch(B, c["T"], c["N"], dataset=c["dataset"], seed=77, with_scores=False)
    shapes = {k: tuple(v.shape) for k, v in pkg.Stlt(pkg.StltModelConfig(**synth.model_kwargs(name))).state_dict().items()}
    sd = synth.make_state_dict(shapes, seed=31, gain=1.5)
    return c, sd, batch


@functools.lru_cache(maxsize=None)
def oracle_top1(name, B):
    from oracle import stlt_oracle as O
    c, sd, batch = layout_case(name, B)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
    with torch.no_grad():
        return tuple(O.stlt_forward(sd64, b64, c["num_attention_heads"], dtype=torch.float64)["stlt"].argmax(dim=1).tolist())


@functools.lru_cache(maxsize=None)
def oracle_ig(name, B, target, dtype=torch.float64):
    """target: a tuple of B classes -> ig_restated.stlt_ig's dict for the one-hot seed, plus "seed" """
    c, sd, batch = layout_case(name, B)
    seed = torch.nn.functional.one_hot(torch.tensor(target), c["num_classes"]).double()
    out = R.stlt_ig(sd, batch, c["num_attention_heads"], seed, STEPS, dtype=dtype)
    out["seed"] = seed
    return out


def bounds(ref):
    """-> ({key: CAP * max|x - x0| * max_s max|g_s^ref|}, the delta bound (B,)).  Every attribution entry is held to its key's bound; delta
    is held to the sum of the keys' bounds plus LOGIT_BAR * sum|seed| for the two logit rows — tighter than the n-fold sum the entries'
    bounds would allow a sum of n entries."""
    per = {k: CAP * ref["diff_max"][k] * ref["grad_max"][k] for k in ref["attr"]}
    return per, sum(per.values()) + LOGIT_BAR * ref["seed"].abs().sum(dim=1)
