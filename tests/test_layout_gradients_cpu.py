"""Layout gradients, the host side: the three new C-ABI entries are declared, exported and bound alike, stlt_train_backward keeps its
signature, Stlt.forward_saliency documents what it returns, and the fp64 oracle — the yardstick of tests/test_layout_gradients_gpu.py — has
the property those tests assert: its gradient wrt the boxes / scores is exactly 0 at every padded object slot and in every padded frame."""
import ctypes as C
import os
import re
import subprocess

import torch
import torch.nn.functional as F

from oracle import stlt_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("stlt_train_backward_inputs", "stlt_embed_bwd_inputs", "stlt_saliency_seed")


def _header():
    return open(os.path.join(ROOT, "include", "stlt_hip.h")).read()


def _prototype(header, name):
    m = re.search(rf"\bint\s+{name}\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in include/stlt_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_new_entries_agree_between_header_exports_and_bindings(pkg):
    header = _header()
    lib = pkg._lib.load()
    vmap = open(os.path.join(ROOT, pkg.__name__, "csrc", "exports.map")).read()
    assert re.search(r"global:\s*stlt_\*;", vmap), "exports.map no longer exports the stlt_* C-ABI"
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        args = _prototype(header, name)
        res, argtypes = pkg._lib.SIGNATURES[name]
        assert res is C.c_int
        assert len(argtypes) == len(args), (name, args)
        assert name in exported, f"{name} is not a dynamic symbol of the library"
        assert getattr(lib, name).argtypes == argtypes
    # the sweep's new form is the old one plus the two outputs in front of the stream
    old, new = _prototype(header, "stlt_train_backward"), _prototype(header, "stlt_train_backward_inputs")
    assert new[:len(old) - 1] == old[:-1] and new[-1] == old[-1]
    assert new[len(old) - 1:-1] == ["float* d_boxes", "float* d_scores"]
    assert pkg._lib.SIGNATURES["stlt_train_backward_inputs"][1][:12] == pkg._lib.SIGNATURES["stlt_train_backward"][1][:12]
    assert _prototype(header, "stlt_embed_bwd_inputs") == ["const float* d_pre", "const float* box_w", "const float* score_w", "int64_t n_tokens", "int64_t d",
                                                           "float* d_boxes", "float* d_scores", "stlt_stream_t stream"]
    assert _prototype(header, "stlt_saliency_seed") == ["const float* logits", "const int64_t* target", "int64_t B", "int64_t K", "float* dlogits",
                                                        "stlt_stream_t stream"]
    assert lib.stlt_version() == 111


def test_train_backward_signature_is_unchanged(pkg):
    assert _prototype(_header(), "stlt_train_backward") == [
        "const stlt_params* p", "const stlt_params* grads", "const stlt_inputs* in", "const void* tape", "size_t tape_bytes", "void* scratch",
        "size_t scratch_bytes", "const float* dlogits", "float dropout_p", "uint64_t dropout_seed", "int flags", "stlt_ctx* ctx", "stlt_stream_t stream"]
    L = pkg._lib
    assert L.SIGNATURES["stlt_train_backward"] == (C.c_int, [C.POINTER(L.Params), C.POINTER(L.Params), C.POINTER(L.Inputs), C.c_void_p, C.c_size_t, C.c_void_p,
                                                             C.c_size_t, C.c_void_p, C.c_float, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p])


def test_host_refusals_need_no_gpu(pkg):
    """The argument checks of the two op-level entries run before anything touches a device."""
    lib = pkg._lib.load()
    a = 4096  # a 16-byte aligned stand-in address: refused calls never dereference it
    assert lib.stlt_embed_bwd_inputs(a, a, None, 8, 6, a, None, None) == -1      # d % 4
    assert lib.stlt_embed_bwd_inputs(a, a, None, -1, 8, a, None, None) == -1     # n_tokens < 0
    assert lib.stlt_embed_bwd_inputs(None, a, None, 8, 8, a, None, None) == -1   # null d_pre
    assert lib.stlt_embed_bwd_inputs(a, a, None, 8, 8, a, a, None) == -1         # d_scores without score_w
    assert lib.stlt_embed_bwd_inputs(a, a, a, 8, 8, a, None, None) == -1         # score_w without d_scores
    assert lib.stlt_embed_bwd_inputs(a, a + 4, None, 8, 8, a, None, None) == -1  # box_w off a 16-byte boundary
    assert b"box_w" in lib.stlt_last_error()
    assert lib.stlt_saliency_seed(None, None, 2, 4, a, None) == -1
    assert lib.stlt_saliency_seed(a, None, 2, 0, a, None) == -1


def test_forward_saliency_exists_and_documents_its_outputs(pkg):
    doc = pkg.Stlt.forward_saliency.__doc__
    for word in ('"stlt"', '"target"', '"boxes_grad"', '"scores_grad"', "(B, T, N, 4)", "(B, T, N)", "exactly 0", "skip_padding"):
        assert word in doc, word


def test_oracle_layout_gradient_is_exactly_zero_under_the_padding_masks(pkg):
    name, B = "cfg1", 5  # clip 4 of this seeded batch has 11 of 16 frames
    c = dict(pkg.synth.CONFIGS[name], num_spatial_layers=2, num_temporal_layers=2)  # the property does not depend on the depth
    kw = dict(pkg.synth.model_kwargs(name), num_spatial_layers=2, num_temporal_layers=2)
    m = pkg.Stlt(pkg.StltModelConfig(**kw))
    sd = pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=31, gain=1.5)
    batch = pkg.synth.make_batch(B, c["T"], c["N"], dataset=c["dataset"], seed=77, with_scores=True)
    labels = torch.randint(0, c["num_classes"], (B,), generator=torch.Generator().manual_seed(5))
    b = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
    b["boxes"].requires_grad_(True)
    b["scores"].requires_grad_(True)
    logits = O.stlt_forward({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, b, c["num_attention_heads"], dtype=torch.float64)["stlt"]
    F.cross_entropy(logits, labels).backward()
    pad_obj = batch["src_key_padding_mask_boxes"].bool()
    pad_frm = batch["src_key_padding_mask_frames"].bool()
    assert pad_obj.any() and pad_frm.any(), "the case must have padded slots and padded frames"
    for g in (b["boxes"].grad.abs().sum(-1), b["scores"].grad.abs()):
        assert g[pad_obj].max().item() == 0.0
        assert g[pad_frm].max().item() == 0.0
        assert g[~pad_obj].max().item() > 0.0
