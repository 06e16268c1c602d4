"""Class activation maps restated in NumPy float64 (test infrastructure only): the three kernels of csrc/gradcam.hip as include/stlt_hip.h
words them, and Grad-CAM / HiResCAM themselves.  Layouts as in the header: "ndhwc" — a, g (B, ..., C); "ncdhw" — (B, C, ...)."""
import numpy as np

U = 2.0 ** -24  # the unit roundoff of float32


def _bpc(x, layout):
    """-> the tensor as float64 (B, P, C)"""
    x = np.asarray(x, dtype=np.float64)
    if layout == "ndhwc":
        return x.reshape(x.shape[0], -1, x.shape[-1])
    return np.moveaxis(x.reshape(x.shape[0], x.shape[1], -1), 1, 2)


def weights(g, layout):
    """alpha (B, C) = the mean of g over the positions, and the bound of a float32 sum of P terms plus the division's rounding"""
    g = _bpc(g, layout)
    P = g.shape[1]
    mag = np.abs(g).sum(axis=1)
    alpha = g.sum(axis=1) / P
    return alpha, P * U * mag / P + U * np.abs(alpha)


def cam_map(a, w, layout, relu):
    """cam (B, P) = sum_c w a (w (B, C), or of a's shape), the positive part with relu, and the bound (C + 1) 2^-24 sum_c|w a|"""
    a = _bpc(a, layout)
    w = np.asarray(w, dtype=np.float64)
    w = w[:, None, :] if w.ndim == 2 else _bpc(w, layout)
    terms = w * a
    cam = terms.sum(axis=2)
    return (np.maximum(cam, 0.0) if relu else cam), (a.shape[2] + 1) * U * np.abs(terms).sum(axis=2)


def gradcam(a, g, layout, variant="gradcam", relu=True):
    """Grad-CAM (alpha = mean_p g) or HiResCAM (element-wise) of activations a and gradient g -> cam (B, P)"""
    w = weights(g, layout)[0] if variant == "gradcam" else g
    return cam_map(a, w, layout, relu)[0]


def _source(out_n, in_n):
    """per output index: (i0, i1, l0, l1) of F.interpolate(align_corners=False)"""
    s = np.maximum((np.arange(out_n) + 0.5) * (in_n / out_n) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), in_n - 1)
    i1 = np.minimum(i0 + 1, in_n - 1)
    l1 = s - i0
    return i0, i1, 1.0 - l1, l1


def upsample(cam, size):
    """cam (B, gt, gh, gw) -> (B, T, H, W): the trilinear resize, w innermost, then h, then t"""
    cam = np.asarray(cam, dtype=np.float64)
    T, H, W = size
    w0, w1, lw0, lw1 = _source(W, cam.shape[3])
    x = cam[:, :, :, w0] * lw0 + cam[:, :, :, w1] * lw1
    h0, h1, lh0, lh1 = _source(H, cam.shape[2])
    x = x[:, :, h0, :] * lh0[:, None] + x[:, :, h1, :] * lh1[:, None]
    t0, t1, lt0, lt1 = _source(T, cam.shape[1])
    return x[:, t0] * lt0[:, None, None] + x[:, t1] * lt1[:, None, None]


def upsample_bound(cam, grid):
    """The float32 kernel against `upsample`: per axis the source coordinate (in / out) (d + 0.5) - 0.5 carries three roundings of numbers
    up to `in` (the quotient, the product, the difference), the fraction l1 is exact and l0 = 1 - l1 adds one: each weight is off by at most
    (3 in + 1) u.  The blend is piecewise linear and continuous in the coordinate, so a weight error d moves a blend of values bounded by
    M = max|cam| by at most (2 d + u) M, also across a cell border; three axes: 3 (2 (3 in + 1) + 1) u M.  The arithmetic adds two
    products and a sum per axis, 9 u M over the three levels.  Together (18 in + 18) u M with in = the largest grid extent."""
    return (18 * max(grid) + 18) * U * float(np.abs(np.asarray(cam, dtype=np.float64)).max())


def pool_cells(cam, cell):
    """cam (B, gt, gh, gw) -> (B, cells): the sum over cubes of `cell` positions (ops.cell_pool_sum on one channel)"""
    cam = np.asarray(cam, dtype=np.float64)
    B, gt, gh, gw = cam.shape
    ct, ch, cw = cell
    Gt, Gh, Gw = -(-gt // ct), -(-gh // ch), -(-gw // cw)
    pad = np.zeros((B, Gt * ct, Gh * ch, Gw * cw))
    pad[:, :gt, :gh, :gw] = cam
    return pad.reshape(B, Gt, ct, Gh, ch, Gw, cw).sum(axis=(2, 4, 6)).reshape(B, -1)
