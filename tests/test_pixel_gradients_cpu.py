"""Pixel gradients, the host side: the new C-ABI entries (the thin-input data gradient, its repack, the trunk sweep that reaches the video) are
declared, exported and bound alike; the sweep's workspace query is host arithmetic; the thin copy has the documented number of floats; the
launchers refuse what they document before anything touches a device; stlt_r3d_backward keeps its signature; and every model documents its
forward_saliency."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("stlt_conv3d_repack_dgrad_thin_floats", "stlt_conv3d_repack_dgrad_thin", "stlt_conv3d_bwd_data_thin", "stlt_r3d_backward_inputs_workspace_bytes",
       "stlt_r3d_backward_inputs")
EINVAL = -1


def _header():
    return open(os.path.join(ROOT, "include", "stlt_hip.h")).read()


def _prototype(header, name):
    m = re.search(rf"\b(?:int|size_t)\s+{name}\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in include/stlt_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _stem(pkg, B=1, T=4, H=8, W=8, c_in=3, c_out=64, k=(7, 7, 7), s=(1, 2, 2), p=(3, 3, 3)):
    return pkg._lib.Conv3dDesc(B, T, H, W, c_in, c_out, *k, *s, *p)


def test_new_entries_agree_between_header_exports_and_bindings(pkg):
    header = _header()
    lib = pkg._lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        args = _prototype(header, name)
        res, argtypes = pkg._lib.SIGNATURES[name]
        assert res is (C.c_size_t if name.endswith(("_floats", "_bytes")) else C.c_int)
        assert len(argtypes) == len(args), (name, args)
        assert name in exported, f"{name} is not a dynamic symbol of the library"
        assert getattr(lib, name).argtypes == argtypes
    # the sweep's new form is stlt_r3d_backward's plus dvideo in front of the workspace
    old, new = _prototype(header, "stlt_r3d_backward"), _prototype(header, "stlt_r3d_backward_inputs")
    assert new[:12] == old[:12] and new[12] == "float* dvideo" and new[13:] == old[12:]
    assert re.search(r"#define STLT_K_CONV_DGRAD_THIN\s+16\b", header) and pkg._lib.K_NAMES[16] == "conv_dgrad_thin"
    assert re.search(r"#define STLT_K_COUNT\s+17\b", header) and len(pkg._lib.K_NAMES) == 17
    assert re.search(r"#define STLT_DX_NDHWC\s+0\b", header) and re.search(r"#define STLT_DX_NCDHW\s+1\b", header)
    assert (pkg._lib.DX_NDHWC, pkg._lib.DX_NCDHW) == (0, 1)


def test_r3d_backward_signature_is_unchanged(pkg):
    assert _prototype(_header(), "stlt_r3d_backward") == [
        "const stlt_r3d_params* p", "const float* const* dgrad_w", "const void* tape", "size_t tape_bytes", "int64_t B", "int64_t T", "int64_t H", "int64_t W",
        "const float* dfeatures", "const float* dpooled", "float* const* dweight", "int accumulate", "void* workspace", "size_t workspace_bytes",
        "stlt_stream_t stream"]


def test_sweep_workspace_is_host_arithmetic(pkg):
    lib = pkg._lib.load()
    for shape in ((1, 8, 64, 64), (16, 32, 112, 112)):
        need, base = int(lib.stlt_r3d_backward_inputs_workspace_bytes(*shape)), int(lib.stlt_r3d_backward_workspace_bytes(*shape))
        assert base > 0 and need >= base, (shape, need, base)
    assert lib.stlt_r3d_backward_inputs_workspace_bytes(0, 8, 64, 64) == 0
    assert lib.stlt_r3d_backward_inputs_workspace_bytes(-3, 8, 64, 64) == 0


def test_thin_copy_float_count_matches_the_documented_layout(pkg):
    """[jt 7][jh 4][jw 4][c_out / 4][column 16][4]: 7·4·4 window taps x c_out x (4 classes x 4 channels) = 1792 · c_out floats, whatever
    the extents and the real channel count; 0 for a descriptor the entry points refuse."""
    lib = pkg._lib.load()
    for c_out in (4, 24, 64, 128):
        for c_in in (1, 3, 4):
            d = _stem(pkg, B=2, T=3, H=9, W=11, c_in=c_in, c_out=c_out)
            assert int(lib.stlt_conv3d_repack_dgrad_thin_floats(C.byref(d))) == 7 * 4 * 4 * c_out * 16 == 1792 * c_out
    assert 1792 * 64 * 4 == 458752  # the stem's copy: the 458 KB that stream through LDS by (temporal tap, row tap)
    assert pkg.modelling.resnet3d.THIN_FLOATS == 1792 * 64
    assert lib.stlt_conv3d_repack_dgrad_thin_floats(C.byref(_stem(pkg, c_in=8))) == 0
    assert lib.stlt_conv3d_repack_dgrad_thin_floats(C.byref(_stem(pkg, s=(1, 3, 3)))) == 0
    assert lib.stlt_conv3d_repack_dgrad_thin_floats(C.byref(_stem(pkg, c_out=6))) == 0
    assert lib.stlt_conv3d_repack_dgrad_thin_floats(None) == 0


def test_host_refusals_need_no_gpu(pkg):
    """The launchers check their arguments before anything touches a device."""
    lib = pkg._lib.load()
    err = lambda: lib.stlt_last_error().decode()  # noqa: E731
    a = 4096  # a 16-byte aligned stand-in address: refused calls never dereference it
    ok = _stem(pkg)
    # the thin data gradient: c_in > 4, stride 3 (and every stride but (1, 2, 2)), another kernel, c_out % 4, null and unaligned pointers, the layout
    assert lib.stlt_conv3d_bwd_data_thin(C.byref(_stem(pkg, c_in=8)), a, a, a, 0, None) == EINVAL and "at most 4 input channels" in err()
    assert lib.stlt_conv3d_bwd_data_thin(C.byref(_stem(pkg, s=(1, 3, 3))), a, a, a, 0, None) == EINVAL and "stride (1, 2, 2)" in err()
    assert lib.stlt_conv3d_bwd_data_thin(C.byref(_stem(pkg, s=(3, 2, 2))), a, a, a, 0, None) == EINVAL and "stride (1, 2, 2)" in err()
    assert lib.stlt_conv3d_bwd_data_thin(C.byref(_stem(pkg, s=(2, 2, 2))), a, a, a, 0, None) == EINVAL and "stride (1, 2, 2)" in err()
    assert lib.stlt_conv3d_bwd_data_thin(C.byref(_stem(pkg, k=(3, 3, 3), p=(1, 1, 1))), a, a, a, 0, None) == EINVAL and "7x7x7" in err()
    assert lib.stlt_conv3d_bwd_data_thin(C.byref(_stem(pkg, c_out=6)), a, a, a, 0, None) == EINVAL and "multiple of 4" in err()
    assert lib.stlt_conv3d_bwd_data_thin(C.byref(ok), None, a, a, 0, None) == EINVAL and "null" in err()
    assert lib.stlt_conv3d_bwd_data_thin(C.byref(ok), a, a, None, 0, None) == EINVAL
    assert lib.stlt_conv3d_bwd_data_thin(C.byref(ok), a + 4, a, a, 0, None) == EINVAL and "dy" in err() and "aligned" in err()
    assert lib.stlt_conv3d_bwd_data_thin(C.byref(ok), a, a + 8, a, 1, None) == EINVAL and "w_dgrad_thin" in err()
    assert lib.stlt_conv3d_bwd_data_thin(C.byref(ok), a, a, a, 2, None) == EINVAL and "dx_layout" in err()
    assert lib.stlt_conv3d_bwd_data_thin(None, a, a, a, 0, None) == EINVAL
    assert lib.stlt_conv3d_repack_dgrad_thin(a, C.byref(_stem(pkg, c_in=5)), None, a, None) == EINVAL and "at most 4 input channels" in err()
    assert lib.stlt_conv3d_repack_dgrad_thin(a, C.byref(_stem(pkg, s=(1, 3, 3))), None, a, None) == EINVAL
    assert lib.stlt_conv3d_repack_dgrad_thin(None, C.byref(ok), None, a, None) == EINVAL
    # the sweep: both outputs NULL is refused before the parameters are looked at
    p = pkg._lib.R3dParams()
    ptrs = pkg._lib.R3dPointers(*([a] * pkg._lib.R3D_CONVS))
    assert lib.stlt_r3d_backward_inputs(C.byref(p), ptrs, a, 1 << 20, 1, 8, 64, 64, None, a, None, 0, None, a, 1 << 20, None) == EINVAL
    assert "both null" in err()
    assert lib.stlt_r3d_backward_inputs(C.byref(p), ptrs, a, 1 << 20, 1, 8, 64, 64, None, a, None, 0, a, a, 1 << 20, None) == EINVAL  # null BN buffers
    assert "stlt_r3d_backward_inputs" in err()
    # stlt_r3d_backward keeps its refusal of a null gradient table
    for i in range(pkg._lib.R3D_CONVS):
        p.conv[i] = pkg._lib.R3dConv(a, a, a, a, a)
    assert lib.stlt_r3d_backward(C.byref(p), ptrs, a, 1 << 20, 1, 8, 64, 64, None, a, None, 0, a, 1 << 20, None) == EINVAL
    assert err() == "stlt_r3d_backward: null pointer"
    # ... and the sweep with a video wants the stem's thin copy aligned
    ptrs[0] = a + 4
    assert lib.stlt_r3d_backward_inputs(C.byref(p), ptrs, a, 1 << 20, 1, 8, 64, 64, None, a, None, 0, a, a, 1 << 20, None) == EINVAL
    assert "thin" in err() and "aligned" in err()


def test_every_video_model_documents_forward_saliency(pkg):
    for cls in (pkg.Resnet3D, pkg.TransformerResnet):
        doc = cls.forward_saliency.__doc__
        assert "video_frames_grad" in doc and "input-only" in doc, cls
    f = pkg.models_factory
    doc = f["caf"].forward_saliency.__doc__
    for word in ('"target"', '"boxes_grad"', '"scores_grad"', '"video_frames_grad"', '"appearance_features_grad"', "head"):
        assert word in doc, word
    assert f["cacnf"].forward_saliency.__doc__ and f["lcf"].forward_saliency.__doc__
    for text in (_header(), open(os.path.join(ROOT, "INTEGRATION.md")).read(), pkg.modelling.resnet3d.R3dTrunkFn.__doc__):
        assert "gets no gradient" not in text and "video gets no" not in text.lower()
