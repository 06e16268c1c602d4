"""The op-level Conv3d C-ABI off the trunk's shapes: anisotropic kernels and paddings, even kernels under stride 2, data-gradient parity
classes whose stride-1 sub-convolution has negative padding, input planes no window reads, mixed strides and stride 3 (forward and weight
gradient), c_out off the multiple of 4 (forward).  Every case runs the forward, the data gradient and the weight gradient it is
eligible for against a float64 CPU convolution (torch.autograd for the gradients) under the bars of tests/test_r3d_gpu.py and
tests/test_r3d_train_gpu.py, and once more on small integers, where the fp32 result must equal the float64 one bit for bit: that pins
every tap to its place independent of any tolerance.  The three extents of kernel, padding and input differ wherever a case allows, so
no exchange of two dimensions maps a case onto itself.  What each case reaches is asserted on the host in tests/test_r3d_plans_cpu.py."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from test_r3d_gpu import _conv, _repack, _to_ndhwc
from test_r3d_train_gpu import _grads64, _ndhwc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = 2.0 ** -24
EINVAL = -1

# (B, Cin, T, H, W, Cout, kernel, stride, pad, n_split)
CASES = {
    "k135_p012": (2, 8, 4, 7, 9, 24, (1, 3, 5), (1, 1, 1), (0, 1, 2), 1),            # anisotropic kernel and pad, stride 1
    "k531_p210": (1, 8, 7, 6, 5, 20, (5, 3, 1), (1, 1, 1), (2, 1, 0), 1),            # the mirror image
    "k333_p000_valid": (2, 12, 4, 5, 6, 28, (3, 3, 3), (1, 1, 1), (0, 0, 0), 1),     # no padding: the data gradient pads by 2
    "k333_p222_grow": (1, 4, 2, 3, 4, 8, (3, 3, 3), (1, 1, 1), (2, 2, 2), 1),        # output larger than input (dgrad pads by 0), T < kt
    # even kernels under stride 2: every parity class has taps, 1·1·2 or 1·2·2 of them (2 or 3 k-slabs of the data gradient)
    "k234_s2_p011": (2, 16, 6, 7, 9, 24, (2, 3, 4), (2, 2, 2), (0, 1, 1), 1),
    "k234_s2_p011_split3": (2, 16, 6, 7, 9, 24, (2, 3, 4), (2, 2, 2), (0, 1, 1), 3),  # ... one request of 3: 2 and 3 splits per class
    "k345_s2_p234_negpad": (1, 8, 5, 6, 8, 16, (3, 4, 5), (2, 2, 2), (2, 3, 4), 1),  # sub-convolution padding -1 in t, h and w
    "k322_s2_p211_negpad": (2, 8, 5, 4, 7, 12, (3, 2, 2), (2, 2, 2), (2, 1, 1), 1),  # one-tap classes with padding -1
    "k222_s2_p000_unread": (1, 8, 5, 7, 9, 16, (2, 2, 2), (2, 2, 2), (0, 0, 0), 1),  # the last plane of t, h and w is read by no window
    "k133_s122_p011": (2, 8, 3, 7, 9, 16, (1, 3, 3), (1, 2, 2), (0, 1, 1), 1),       # mixed strides: forward and wgrad only
    "k151_s213_p040": (1, 8, 6, 5, 10, 12, (1, 5, 1), (2, 1, 3), (0, 4, 0), 1),      # three different strides, p = k - 1
    "k222_s3_p011": (1, 8, 7, 8, 10, 12, (2, 2, 2), (3, 3, 3), (0, 1, 1), 1),        # stride above the kernel: forward and wgrad only
    "k212_cout5": (2, 4, 3, 4, 5, 5, (2, 1, 2), (1, 1, 1), (1, 0, 0), 1),            # c_out % 4 != 0: forward only
}
ALL = sorted(CASES)
WGRAD = [c for c in ALL if CASES[c][5] % 4 == 0]
DGRAD = [c for c in WGRAD if CASES[c][7] in ((1, 1, 1), (2, 2, 2))]
# the weight gradient of k234_s2_p011 under n_split 1 and 3 is the table's two rows; 0 (the library's plan) comes on top
WGRAD_RUNS = [(c, CASES[c][9]) for c in WGRAD] + [("k234_s2_p011", 0)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def unread_planes(n, k, s, p):
    """input positions of one dimension that no window of the forward reads, by enumeration"""
    read = {o * s - p + d for o in range(_out(n, k, s, p)) for d in range(k)}
    return [i for i in range(n) if i not in read]


@functools.lru_cache(maxsize=None)
def inputs(case, integer=False):
    """x (B, Cin, T, H, W), w (Cout, Cin, kt, kh, kw), dy (B, Cout, To, Ho, Wo) on the CPU; integer: whole numbers in [-2, 2]"""
    B, Ci, T, H, W, Co, k, s, p, _ = CASES[case]
    g = torch.Generator().manual_seed(3000 + ALL.index(case) + (100 if integer else 0))
    To, Ho, Wo = [_out(n, kk, ss, pp) for n, kk, ss, pp in zip((T, H, W), k, s, p)]
    if integer:
        draw = lambda *shape: torch.randint(-2, 3, shape, generator=g).float()
        return draw(B, Ci, T, H, W), draw(Co, Ci, *k), draw(B, Co, To, Ho, Wo)
    x = torch.randn(B, Ci, T, H, W, generator=g)
    w = torch.randn(Co, Ci, *k, generator=g) * (2.0 / (Ci * k[0] * k[1] * k[2])) ** 0.5
    return x, w, torch.randn(B, Co, To, Ho, Wo, generator=g)


@functools.lru_cache(maxsize=None)
def references(case, integer=False):
    """float64 on the CPU, computed once per case and shared: y, dx, dw and the same three of |x|, |w|, |dy| (the bars' magnitudes)"""
    x, w, dy = inputs(case, integer)
    _, _, _, _, _, _, _, s, p, _ = CASES[case]
    y = F.conv3d(x.double(), w.double(), stride=s, padding=p)
    y_mag = F.conv3d(x.double().abs(), w.double().abs(), stride=s, padding=p)
    dx, dw = _grads64(x, w, dy, s, p)
    dx_mag, dw_mag = _grads64(x, w, dy, s, p, absval=True)
    return {"y": y, "y_mag": y_mag, "dx": dx, "dx_mag": dx_mag, "dw": dw, "dw_mag": dw_mag}


def _desc(pkg, case):
    B, Ci, T, H, W, Co, k, s, p, _ = CASES[case]
    return pkg._lib.Conv3dDesc(B, T, H, W, (Ci + 3) // 4 * 4, Co, *k, *s, *p)


def _forward(pkg, case, x, w, bn=None, res=None, relu=False):
    B, Ci, T, H, W, Co, k, s, p, n_split = CASES[case]
    c_pad = (Ci + 3) // 4 * 4
    y = _conv(pkg, _to_ndhwc(pkg, x, c_pad), _repack(pkg, w, c_pad), Co, k, s, p, bn=bn, res=res, relu=relu, n_split=n_split)
    return y.permute(0, 4, 1, 2, 3)


def _dgrad(pkg, case, w, dy_d, scale_co=None, epilogue=None, dx=None):
    """stlt_conv3d_repack_dgrad + stlt_conv3d_bwd_data into a dx that starts as NaN (a position no class writes shows); epilogue:
    (scale, mask, add) device tensors; dx given: the launch's add source and destination (add == dx)"""
    B, Ci, T, H, W, Co, k, s, p, n_split = CASES[case]
    lib = pkg._lib.load()
    d = _desc(pkg, case)
    w_d = w.to(DEV)
    sc_d = None if scale_co is None else scale_co.to(DEV)
    wd = torch.empty(w.numel(), device=DEV)
    pkg._lib.check(lib.stlt_conv3d_repack_dgrad(w_d.data_ptr(), ctypes.byref(d), None if sc_d is None else sc_d.data_ptr(), wd.data_ptr(), _stream()),
                   "stlt_conv3d_repack_dgrad")
    nbytes = int(lib.stlt_conv3d_bwd_data_workspace_bytes(ctypes.byref(d), n_split))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
    args = [None, None, None] if epilogue is None else [t.data_ptr() for t in epilogue]
    if dx is None:
        dx = torch.full((B, T, H, W, Ci), float("nan"), device=DEV)
    else:
        args[2] = dx.data_ptr()
    pkg._lib.check(lib.stlt_conv3d_bwd_data(ctypes.byref(d), dy_d.data_ptr(), wd.data_ptr(), *args, n_split, ws.data_ptr(), nbytes, dx.data_ptr(),
                                            _stream()), "stlt_conv3d_bwd_data")
    return dx.permute(0, 4, 1, 2, 3).cpu().double()


def _wgrad(pkg, case, x_d, dy_d, n_split, scale=None, init=None):
    B, Ci, T, H, W, Co, k, s, p, _ = CASES[case]
    lib = pkg._lib.load()
    d = _desc(pkg, case)
    nbytes = int(lib.stlt_conv3d_bwd_weight_workspace_bytes(ctypes.byref(d), n_split))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dw = torch.full((Co, Ci, *k), float("nan"), device=DEV) if init is None else init.to(DEV)
    pkg._lib.check(lib.stlt_conv3d_bwd_weight(ctypes.byref(d), x_d.data_ptr(), dy_d.data_ptr(), None if scale is None else scale.data_ptr(), Ci,
                                              int(init is not None), n_split, ws.data_ptr(), nbytes, dw.data_ptr(), _stream()), "stlt_conv3d_bwd_weight")
    return dw.cpu().double()


@pytest.mark.parametrize("epilogue", [False, True], ids=["plain", "bn_res_relu"])
@pytest.mark.parametrize("case", ALL)
def test_forward_against_float64(pkg, case, epilogue):
    B, Ci, T, H, W, Co, k, s, p, _ = CASES[case]
    x, w, _ = inputs(case)
    R = references(case)
    ref, scale = R["y"], torch.ones(Co, dtype=torch.float64)
    bn = res_dev = None
    if epilogue:
        g = torch.Generator().manual_seed(3500 + ALL.index(case))
        bn = [1 + 0.2 * torch.randn(Co, generator=g), 0.1 * torch.randn(Co, generator=g), 0.1 * torch.randn(Co, generator=g),
              0.5 + torch.rand(Co, generator=g)]
        scale = bn[0].double() / torch.sqrt(bn[3].double() + 1e-5)
        res = torch.randn(ref.shape, generator=g)
        ref = (ref * scale.view(1, -1, 1, 1, 1) + (bn[1].double() - bn[2].double() * scale).view(1, -1, 1, 1, 1) + res.double()).relu()
        bn, res_dev = [t.to(DEV) for t in bn], _ndhwc(res)
    y = _forward(pkg, case, x, w, bn=bn, res=res_dev, relu=epilogue)
    assert y.shape == ref.shape
    K = Ci * k[0] * k[1] * k[2]
    tol = 4 * EPS32 * K ** 0.5 * (R["y_mag"] * scale.abs().view(1, -1, 1, 1, 1)).max().item() + 4 * EPS32 * ref.abs().max().item()
    err = (y.cpu().double() - ref).abs().max().item()
    print(f"forward {case} {'epilogue' if epilogue else 'plain'}: err {err:.3e} bar {tol:.3e}")
    assert err <= tol, (case, err, tol)
    assert torch.equal(y, _forward(pkg, case, x, w, bn=bn, res=res_dev, relu=epilogue))  # a second launch is bit-identical


@pytest.mark.parametrize("case", DGRAD)
def test_dgrad_against_float64(pkg, case):
    B, Ci, T, H, W, Co, k, s, p, _ = CASES[case]
    x, w, dy = inputs(case)
    g = torch.Generator().manual_seed(3600 + ALL.index(case))
    scale_co = 0.5 + torch.rand(Co, generator=g)   # folded into the dgrad copy
    scale_ci = 0.5 + torch.rand(Ci, generator=g)   # epilogue scale
    add = torch.randn(B, Ci, T, H, W, generator=g)
    mask = torch.randn(B, Ci, T, H, W, generator=g)
    dy_d, add_d, mask_d, sc_d = _ndhwc(dy), _ndhwc(add), _ndhwc(mask), scale_ci.to(DEV)
    ws_ = w * scale_co.view(-1, 1, 1, 1, 1)
    ref = _grads64(x, ws_, dy, s, p)[0]
    mag = _grads64(x, ws_, dy, s, p, absval=True)[0]
    tol = 4 * EPS32 * (Co * k[0] * k[1] * k[2]) ** 0.5 * mag.max().item()
    got = _dgrad(pkg, case, w, dy_d, scale_co)
    err = (got - ref).abs().max().item()  # NaN (a position left unwritten) fails the comparison below
    print(f"dgrad {case} plain: err {err:.3e} bar {tol:.3e}")
    assert err <= tol, (case, err, tol)
    masked_add = torch.where(mask.double() > 0, add.double(), torch.zeros_like(ref))
    ref_e = torch.where(mask.double() > 0, ref * scale_ci.double().view(1, -1, 1, 1, 1) + add.double(), torch.zeros_like(ref))
    got_e = _dgrad(pkg, case, w, dy_d, scale_co, epilogue=(sc_d, mask_d, add_d))
    tol_e = tol * scale_ci.max().item() + 4 * EPS32 * add.abs().max().item()
    err_e = (got_e - ref_e).abs().max().item()
    print(f"dgrad {case} epilogue: err {err_e:.3e} bar {tol_e:.3e}")
    assert err_e <= tol_e, (case, err_e, tol_e)
    assert torch.equal(got_e, _dgrad(pkg, case, w, dy_d, scale_co, epilogue=(sc_d, mask_d, add_d)))  # bit-identical again
    # add == dx: each element is read, then written, by one thread — bit for bit the out-of-place result
    assert torch.equal(_dgrad(pkg, case, w, dy_d, scale_co, epilogue=(sc_d, mask_d, add_d), dx=add_d.clone()), got_e), case
    # planes no window reads: no gradient reaches them, so they hold the epilogue of exactly zero
    planes = [unread_planes(n, kk, ss, pp) for n, kk, ss, pp in zip((T, H, W), k, s, p)]
    if case == "k222_s2_p000_unread":
        assert planes == [[4], [6], [8]]
    for dim, idx in enumerate(planes):
        for i in idx:
            assert torch.equal(got.select(2 + dim, i), torch.zeros_like(got.select(2 + dim, i))), (case, dim, i)
            assert torch.equal(got_e.select(2 + dim, i), masked_add.select(2 + dim, i)), (case, dim, i)


@pytest.mark.parametrize("case,n_split", WGRAD_RUNS, ids=[f"{c}-n{n}" for c, n in WGRAD_RUNS])
def test_wgrad_against_float64(pkg, case, n_split):
    B, Ci, T, H, W, Co, k, s, p, _ = CASES[case]
    x, w, dy = inputs(case)
    R = references(case)
    g = torch.Generator().manual_seed(3700 + ALL.index(case))
    scale = 0.5 + torch.rand(Co, generator=g)
    init = torch.randn(Co, Ci, *k, generator=g)
    x_d, dy_d, sc_d = _ndhwc(x, (Ci + 3) // 4 * 4), _ndhwc(dy), scale.to(DEV)
    sc = scale.double().view(-1, 1, 1, 1, 1)
    ref, mag = R["dw"] * sc, R["dw_mag"] * sc
    M = dy[0, 0].numel() * B
    tol = 4 * EPS32 * M ** 0.5 * mag.max().item()
    got = _wgrad(pkg, case, x_d, dy_d, n_split, scale=sc_d)
    err = (got - ref).abs().max().item()
    print(f"wgrad {case} n_split {n_split}: err {err:.3e} bar {tol:.3e}")
    assert err <= tol, (case, err, tol)
    got_acc = _wgrad(pkg, case, x_d, dy_d, n_split, scale=sc_d, init=init)
    err_acc = (got_acc - (ref + init.double())).abs().max().item()
    assert err_acc <= tol + 4 * EPS32 * init.abs().max().item(), (case, err_acc)
    assert torch.equal(got_acc, _wgrad(pkg, case, x_d, dy_d, n_split, scale=sc_d, init=init))


# ---- integers in [-2, 2], no BatchNorm and no scale: every product and partial sum is a whole number below 2^24 (checked on the
# reference of magnitudes, which bounds every partial sum in any order), so fp32 is exact and must equal float64 bit for bit ----
def _exact(case, key):
    R = references(case, integer=True)
    assert R[key + "_mag"].max().item() < 2 ** 24, (case, key)
    return R[key]


@pytest.mark.parametrize("case", ALL)
def test_forward_exact_on_integers(pkg, case):
    x, w, _ = inputs(case, integer=True)
    ref = _exact(case, "y")
    y = _forward(pkg, case, x, w)
    assert y.shape == ref.shape
    assert torch.equal(y.cpu().double(), ref), (case, (y.cpu().double() - ref).abs().max().item())


@pytest.mark.parametrize("case", DGRAD)
def test_dgrad_exact_on_integers(pkg, case):
    _, w, dy = inputs(case, integer=True)
    ref = _exact(case, "dx")
    got = _dgrad(pkg, case, w, _ndhwc(dy))
    assert torch.equal(got, ref), (case, (got - ref).abs().max().item())


@pytest.mark.parametrize("case,n_split", WGRAD_RUNS, ids=[f"{c}-n{n}" for c, n in WGRAD_RUNS])
def test_wgrad_exact_on_integers(pkg, case, n_split):
    Ci = CASES[case][1]
    x, _, dy = inputs(case, integer=True)
    ref = _exact(case, "dw")
    got = _wgrad(pkg, case, _ndhwc(x, (Ci + 3) // 4 * 4), _ndhwc(dy), n_split)
    assert torch.equal(got, ref), (case, (got - ref).abs().max().item())


# ---- refusals: STLT_EINVAL before anything is launched, and the message names the rule ----
def _buffers(B, Ci, T, H, W, Co, k, s, p):
    """device buffers of the described shapes (outputs sized for the larger of the padded and unpadded geometry), so that a call which
    wrongly launched would still stay inside them"""
    To, Ho, Wo = [max(_out(n, kk, ss, pp), 1) for n, kk, ss, pp in zip((T, H, W), k, s, p)]
    z = lambda *shape: torch.zeros(*shape, device=DEV)
    taps = k[0] * k[1] * k[2]
    return {"x": z(B, T, H, W, Ci), "y": z(B, To, Ho, Wo, Co + 3), "w": z((Co + 3) * taps * Ci), "dw": z((Co + 3) * taps * Ci),
            "ws": torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)}


def _calls(pkg, shape):
    """the four descriptor-taking entry points on one shape, each returning (code, message)"""
    lib = pkg._lib.load()
    B, Ci, T, H, W, Co, k, s, p = shape
    d = pkg._lib.Conv3dDesc(B, T, H, W, Ci, Co, *k, *s, *p)
    b = _buffers(*shape)
    ptr = {n: t.data_ptr() for n, t in b.items()}
    nws = b["ws"].numel()

    def run(fn, *args):
        code = fn(*args)
        return code, lib.stlt_last_error().decode()

    return {
        "fwd": lambda: run(lib.stlt_conv3d_fwd, ctypes.byref(d), ptr["x"], ptr["w"], None, None, None, None, 1e-5, None, 0, 1, ptr["ws"], nws, ptr["y"],
                           _stream()),
        "repack_dgrad": lambda: run(lib.stlt_conv3d_repack_dgrad, ptr["w"], ctypes.byref(d), None, ptr["dw"], _stream()),
        "bwd_data": lambda: run(lib.stlt_conv3d_bwd_data, ctypes.byref(d), ptr["y"], ptr["w"], None, None, None, 1, ptr["ws"], nws, ptr["x"], _stream()),
        "bwd_weight": lambda: run(lib.stlt_conv3d_bwd_weight, ctypes.byref(d), ptr["x"], ptr["y"], None, Ci, 0, 1, ptr["ws"], nws, ptr["dw"], _stream()),
    }, b


def _shape(case):
    return CASES[case][:9]


def test_refusals(pkg):
    # data gradient: mixed strides, stride 3, c_out = 5
    for case in ("k133_s122_p011", "k151_s213_p040", "k222_s3_p011"):
        calls, _keep = _calls(pkg, _shape(case))
        code, msg = calls["bwd_data"]()
        assert code == EINVAL and "strides must be equal and at most 2" in msg, (case, code, msg)
    calls, _keep = _calls(pkg, _shape("k212_cout5"))
    code, msg = calls["bwd_data"]()
    assert code == EINVAL and "c_out must be a multiple of 4" in msg, (code, msg)
    # weight gradient: c_out = 5
    code, msg = calls["bwd_weight"]()
    assert code == EINVAL and "c_out must be a multiple of 4" in msg, (code, msg)
    # the dgrad weight copy: stride 3 (and a stride of 3 in one dimension only)
    for case in ("k222_s3_p011", "k151_s213_p040"):
        calls, _keep = _calls(pkg, _shape(case))
        code, msg = calls["repack_dgrad"]()
        assert code == EINVAL and "strides above 2" in msg, (case, code, msg)
    # padding equal to the kernel extent in one dimension only, t, h and w in turn, at every entry point that takes a descriptor
    B, Ci, T, H, W, Co, k, s, _, _ = CASES["k135_p012"]
    k = (2, 3, 5)
    for dim in range(3):
        p = tuple(k[i] if i == dim else 0 for i in range(3))
        calls, _keep = _calls(pkg, (B, Ci, T, H, W, Co, k, s, p))
        for name, call in calls.items():
            code, msg = call()
            assert code == EINVAL and "padding must lie in [0, kernel)" in msg, (dim, name, code, msg)
