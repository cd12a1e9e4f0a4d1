"""Tensor-level wrappers over the C ABI (include/dl3p.h).

PyTorch is only the allocator / stream provider here: every function takes CUDA(=HIP) float32
tensors in NHWC memory (a channel slice of a wider buffer is fine: row stride `ld` is taken from the
tensor's strides), hands raw device pointers to libdl3p.so and returns.  There is no CPU or torch
fallback: a missing library raises at import, a non-HIP tensor raises here.
"""
import ctypes
import torch

from ._lib import lib, Dl3pError  # noqa: F401

ACT_NONE, ACT_RELU, ACT_RELU6, ACT_HSWISH, ACT_HSIGMOID = 0, 1, 2, 3, 4
MAX_STAT_ROWS = 2048


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pl(t):
    """(device pointer, row stride in floats) of an NHWC / [M,C] tensor or channel-slice view"""
    if t is None:
        return None, 0
    if not t.is_cuda or t.dtype != torch.float32:
        raise Dl3pError('dl3p ops need float32 tensors on the HIP device (got %s on %s)' % (t.dtype, t.device))
    if t.stride(-1) != 1:
        raise Dl3pError('channel dim must be contiguous')
    ld = t.stride(-2) if t.dim() >= 2 else t.shape[-1]
    # rows must be evenly spaced: stride of each leading dim == size*stride of the next
    for d in range(t.dim() - 2):
        if t.shape[d + 1] > 0 and t.stride(d) != t.stride(d + 1) * t.shape[d + 1]:
            raise Dl3pError('rows are not evenly strided: %s %s' % (tuple(t.shape), t.stride()))
    return t.data_ptr(), ld


def _p(t):
    return None if t is None else t.data_ptr()


def same_pad(in_size, k, stride, rate):
    """TF SAME: (out, pad_begin) -- the odd unit of padding goes to the end"""
    k_eff = k + (k - 1) * (rate - 1)
    out = -(-in_size // stride)
    total = max((out - 1) * stride + k_eff - in_size, 0)
    return out, total // 2


def conv_geometry(H, W, k, stride, rate, padding):
    """padding 'same' | 'valid' | (pt, pb, pl, pr) -> Ho, Wo, pad_t, pad_l"""
    if padding == 'same':
        Ho, pt = same_pad(H, k, stride, rate)
        Wo, pl = same_pad(W, k, stride, rate)
        return Ho, Wo, pt, pl
    if padding == 'valid':
        padding = (0, 0, 0, 0)
    pt, pb, pl, pr = padding
    k_eff = k + (k - 1) * (rate - 1)
    return (H + pt + pb - k_eff) // stride + 1, (W + pl + pr - k_eff) // stride + 1, pt, pl


def new_partials(C, device, rows=MAX_STAT_ROWS):
    return torch.empty(rows * 2 * C, dtype=torch.float32, device=device)


# ------------------------------------------------------------------------------------- depthwise
def _arm_upsampled(up):
    """up (N,h,w,C1): the NEXT depthwise launch forms channels [0, C1) of its input from it (dl3p_dw_upsampled_input)"""
    if up is not None:
        upp, upld = _pl(up)
        lib().dw_upsampled_input(upp, upld, up.shape[1], up.shape[2], up.shape[3], _stream())


def dwconv2d_fwd(x, w, stride=1, rate=1, padding='same', in_scale=None, in_shift=None, in_act=ACT_NONE,
                 out=None, partials=None, upsampled=None):
    """x (N,H,W,C); w (k,k,C) or (k,k,C,1) -> y (N,Ho,Wo,C) [, rows]"""
    _arm_upsampled(upsampled)
    N, H, W, C = x.shape
    k = w.shape[0]
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    y = out if out is not None else torch.empty((N, Ho, Wo, C), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    rows = ctypes.c_int(0)
    lib().dwconv2d_fwd(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(w), yp, ldy, _p(partials), ctypes.byref(rows),
                       N, H, W, C, k, stride, rate, pt, pl, Ho, Wo, _stream())
    return (y, rows.value) if partials is not None else y


def dwconv2d_bwd_data(dy, w, x_shape, stride=1, rate=1, padding='same', out=None, accumulate=False):
    N, H, W, C = x_shape
    k = w.shape[0]
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    gx = out if out is not None else torch.empty(x_shape, dtype=torch.float32, device=dy.device)
    dp, ldd = _pl(dy)
    gp, ldg = _pl(gx)
    lib().dwconv2d_bwd_data(dp, ldd, _p(w), gp, ldg, int(accumulate), N, H, W, C, k, stride, rate, pt, pl, Ho, Wo,
                            _stream())
    return gx


def dwconv2d_bwd_data_bn(dy, w, x_shape, z, scale, shift, act, mean, invstd, partials, stride=1, rate=1, padding='same',
                          out=None, accumulate=False):
    """dwconv2d_bwd_data + the BatchNorm-backward partial sums of act(BN(z)) of the finished gradient; -> (gx, rows)"""
    N, H, W, C = x_shape
    k = w.shape[0]
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    gx = out if out is not None else torch.empty((N, H, W, C), dtype=torch.float32, device=dy.device)
    dp, lddy = _pl(dy)
    gp, ldg = _pl(gx)
    zp, ldz = _pl(z)
    rows = ctypes.c_int(0)
    lib().dwconv2d_bwd_data_bn(dp, lddy, _p(w), gp, ldg, int(accumulate), N, H, W, C, k, stride, rate, pt, pl, Ho, Wo,
                               zp, ldz, _p(scale), _p(shift), act, _p(mean), _p(invstd), _p(partials),
                               ctypes.byref(rows), _stream())
    return gx, rows.value


def dwconv2d_bwd_weight(x, dy, k, stride=1, rate=1, padding='same', in_scale=None, in_shift=None, in_act=ACT_NONE,
                        workspace=None, upsampled=None):
    _arm_upsampled(upsampled)
    N, H, W, C = x.shape
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    need = lib().dwconv2d_bwd_weight_workspace(N, Ho, Wo, C, k)
    ws = workspace if workspace is not None else torch.empty(need // 4, dtype=torch.float32, device=x.device)
    gw = torch.empty((k, k, C), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    dp, ldd = _pl(dy)
    lib().dwconv2d_bwd_weight(xp, ldx, _p(in_scale), _p(in_shift), in_act, dp, ldd, _p(gw), _p(ws), ws.numel() * 4,
                              N, H, W, C, k, stride, rate, pt, pl, Ho, Wo, _stream())
    return gw


def dwconv2d_bwd_weight_bn(x, g, z, bn, act, k, stride=1, rate=1, padding='same', in_scale=None, in_shift=None,
                           in_act=ACT_NONE, want_dz=True, upsampled=None):
    """depthwise weight gradient with the BatchNorm-backward apply of the conv's output folded in
    (dl3p_dwconv2d_bwd_weight_slabs_bn + the slab reduction) -> (gw, dz)"""
    _arm_upsampled(upsampled)
    N, H, W, C = x.shape
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    need = lib().dwconv2d_bwd_weight_workspace(N, Ho, Wo, C, k)
    ws = torch.empty(need // 4, dtype=torch.float32, device=x.device)
    gw = torch.empty((k, k, C), dtype=torch.float32, device=x.device)
    dz = torch.empty(g.shape, dtype=torch.float32, device=x.device) if want_dz else None
    xp, ldx = _pl(x)
    gp, ldg = _pl(g)
    zp, ldz = _pl(z)
    dp, ldd = _pl(dz)
    rows = ctypes.c_int(0)
    lib().dwconv2d_bwd_weight_slabs_bn(xp, ldx, _p(in_scale), _p(in_shift), in_act, gp, ldg, zp, ldz, _p(bn.scale),
                                       _p(bn.shift), act, _p(bn.mean), _p(bn.invstd), _p(bn.coef), dp, ldd or 0, _p(ws),
                                       ws.numel() * 4, ctypes.byref(rows), N, H, W, C, k, stride, rate, pt, pl, Ho, Wo,
                                       _stream())
    lib().reduce_rows(_p(ws), rows.value, k * k * C, _p(gw), 0, _stream())
    return gw, dz


# ------------------------------------------------------------------------------------- pointwise
def _rows(t):
    return t.numel() // t.shape[-1]


def pwconv_fwd(x, w, bias=None, in_scale=None, in_shift=None, in_act=ACT_NONE, out=None, partials=None):
    """x (..., K); w (K,N) -> y (..., N)"""
    K, Nn = w.shape[-2], w.shape[-1]
    M = _rows(x)
    y = out if out is not None else torch.empty(tuple(x.shape[:-1]) + (Nn,), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    rows = ctypes.c_int(0)
    lib().pwconv_fwd(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(w), _p(bias), yp, ldy, _p(partials),
                     ctypes.byref(rows), M, K, Nn, _stream())
    return (y, rows.value) if partials is not None else y


def pwconv_fwd_wt(x, wt, bias=None, in_scale=None, in_shift=None, in_act=ACT_NONE, out=None, partials=None):
    """pwconv_fwd with the kernel given transposed, wt (N, K)"""
    M, K = _rows(x), x.shape[-1]
    N = wt.shape[0]
    y = out if out is not None else torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    rows = ctypes.c_int(0)
    lib().pwconv_fwd_wt(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(wt), _p(bias), yp, ldy, _p(partials),
                        ctypes.byref(rows), M, K, N, _stream())
    return (y, rows.value) if partials is not None else y


def pwconv_fwd_wt_splitk(x, wt, bias=None, in_scale=None, in_shift=None, in_act=ACT_NONE, out=None, partials=None):
    """pwconv_fwd_wt through the split-K form (few rows, long reduction); raises Dl3pError where dl3p_pwconv_fwd_splitk_plan says 0"""
    M, K = _rows(x), x.shape[-1]
    N = wt.shape[0]
    y = out if out is not None else torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    rows = ctypes.c_int(0)
    wsb = lib().pwconv_fwd_splitk_workspace(M, K, N)
    ws = torch.empty(max(wsb, 16) // 4, dtype=torch.float32, device=x.device)
    lib().pwconv_fwd_wt_splitk(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(wt), _p(bias), yp, ldy, _p(partials),
                               ctypes.byref(rows), _p(ws), wsb, M, K, N, _stream())
    return (y, rows.value) if partials is not None else y


def transpose_batch(src, dst, table):
    lib().transpose_batch(_p(src), _p(dst), _p(table), int(table.shape[0]), _stream())


def pwconv_bwd_data(dy, w, out=None, accumulate=False):
    K, Nn = w.shape[-2], w.shape[-1]
    M = _rows(dy)
    gx = out if out is not None else torch.empty(tuple(dy.shape[:-1]) + (K,), dtype=torch.float32, device=dy.device)
    dp, ldd = _pl(dy)
    gp, ldg = _pl(gx)
    lib().pwconv_bwd_data(dp, ldd, _p(w), gp, ldg, int(accumulate), M, K, Nn, _stream())
    return gx


def pwconv_bwd_data_bn(dy, w, z, scale, shift, act, mean, invstd, partials, out=None, accumulate=False):
    """pwconv_bwd_data + the BatchNorm-backward partial sums of act(BN(z)) from the finished gradient; -> (gx, rows)"""
    M, N = _rows(dy), dy.shape[-1]
    K = w.shape[0]
    gx = out if out is not None else torch.empty(dy.shape[:-1] + (K,), dtype=torch.float32, device=dy.device)
    dp, lddy = _pl(dy)
    gp, ldg = _pl(gx)
    zp, ldz = _pl(z)
    rows = ctypes.c_int(0)
    lib().pwconv_bwd_data_bn(dp, lddy, _p(w), gp, ldg, int(accumulate), M, K, N, zp, ldz, _p(scale), _p(shift), act,
                             _p(mean), _p(invstd), _p(partials), ctypes.byref(rows), _stream())
    return gx, rows.value


def pwconv_bwd_weight(x, dy, in_scale=None, in_shift=None, in_act=ACT_NONE, with_bias=False, workspace=None):
    K, Nn = x.shape[-1], dy.shape[-1]
    M = _rows(x)
    need = lib().pwconv_bwd_weight_workspace(M, K, Nn)
    ws = workspace if workspace is not None else torch.empty(need // 4, dtype=torch.float32, device=x.device)
    gw = torch.empty((K, Nn), dtype=torch.float32, device=x.device)
    gb = torch.empty((Nn,), dtype=torch.float32, device=x.device) if with_bias else None
    xp, ldx = _pl(x)
    dp, ldd = _pl(dy)
    lib().pwconv_bwd_weight(xp, ldx, _p(in_scale), _p(in_shift), in_act, dp, ldd, _p(gw), _p(gb), _p(ws),
                            ws.numel() * 4, M, K, Nn, _stream())
    return (gw, gb) if with_bias else gw


def pwconv_bwd_weight_bn(x, g, z, bn, act, in_scale=None, in_shift=None, in_act=ACT_NONE, want_dz=True):
    """weight gradient with the BatchNorm-backward apply of the conv's output folded in (dl3p_pwconv_bwd_weight_slabs_bn
    + the slab reduction): g = gradient of act(bn(z)), bn.coef from bn_bwd_finalize -> (gw, dz)"""
    K, Nn = x.shape[-1], g.shape[-1]
    M = _rows(x)
    need = lib().pwconv_bwd_weight_workspace(M, K, Nn)
    ws = torch.empty(need // 4, dtype=torch.float32, device=x.device)
    gw = torch.empty((K, Nn), dtype=torch.float32, device=x.device)
    dz = torch.empty(g.shape, dtype=torch.float32, device=x.device) if want_dz else None
    xp, ldx = _pl(x)
    gp, ldg = _pl(g)
    zp, ldz = _pl(z)
    dp, ldd = _pl(dz)
    rows = ctypes.c_int(0)
    lib().pwconv_bwd_weight_slabs_bn(xp, ldx, _p(in_scale), _p(in_shift), in_act, gp, ldg, zp, ldz, _p(bn.scale), _p(bn.shift),
                                     act, _p(bn.mean), _p(bn.invstd), _p(bn.coef), dp, ldd or 0, _p(ws), ws.numel() * 4,
                                     ctypes.byref(rows), M, K, Nn, _stream())
    lib().reduce_rows(_p(ws), rows.value, K * Nn, _p(gw), 0, _stream())
    return gw, dz


# ------------------------------------------------------------------------------------- dense conv
def conv2d_fwd(x, w, stride=1, rate=1, padding='same', in_scale=None, in_shift=None, in_act=ACT_NONE, out=None,
               partials=None):
    N, H, W, Cin = x.shape
    k, _, _, Cout = w.shape
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    y = out if out is not None else torch.empty((N, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    rows = ctypes.c_int(0)
    lib().conv2d_fwd(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(w), yp, ldy, _p(partials), ctypes.byref(rows),
                     N, H, W, Cin, Cout, k, stride, rate, pt, pl, Ho, Wo, _stream())
    return (y, rows.value) if partials is not None else y


def conv2d_bwd_weight(x, dy, k, stride=1, rate=1, padding='same', in_scale=None, in_shift=None, in_act=ACT_NONE):
    N, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    need = lib().conv2d_bwd_weight_workspace(N, Ho, Wo, Cin, Cout, k)
    ws = torch.empty(need // 4, dtype=torch.float32, device=x.device)
    gw = torch.empty((k, k, Cin, Cout), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    dp, ldd = _pl(dy)
    lib().conv2d_bwd_weight(xp, ldx, _p(in_scale), _p(in_shift), in_act, dp, ldd, _p(gw), _p(ws), ws.numel() * 4,
                            N, H, W, Cin, Cout, k, stride, rate, pt, pl, Ho, Wo, _stream())
    return gw


def conv2d_bwd_data(dy, w, x_shape, stride=1, rate=1, padding='same', out=None, accumulate=False):
    N, H, W, Cin = x_shape
    k, _, _, Cout = w.shape
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    gx = out if out is not None else torch.empty(x_shape, dtype=torch.float32, device=dy.device)
    dp, ldd = _pl(dy)
    gp, ldg = _pl(gx)
    lib().conv2d_bwd_data(dp, ldd, _p(w), gp, ldg, int(accumulate), N, H, W, Cin, Cout, k, stride, rate, pt, pl,
                          Ho, Wo, _stream())
    return gx


# ------------------------------------------------------------------------------------- batch norm
class BNState:
    """device-side state of one BatchNormalization layer (all float32 [C])"""

    def __init__(self, C, device, eps=1e-3, momentum=0.99):
        f = dict(dtype=torch.float32, device=device)
        self.C, self.eps, self.momentum = C, eps, momentum
        self.gamma = torch.ones(C, **f)
        self.beta = torch.zeros(C, **f)
        self.moving_mean = torch.zeros(C, **f)
        self.moving_var = torch.ones(C, **f)
        self.scale = torch.empty(C, **f)
        self.shift = torch.empty(C, **f)
        self.mean = torch.empty(C, **f)
        self.invstd = torch.empty(C, **f)
        self.coef = torch.empty(3 * C, **f)
        self.dgamma = torch.empty(C, **f)
        self.dbeta = torch.empty(C, **f)


def bn_finalize(bn, partials, rows, count, update_moving=True, sums=None):
    lib().bn_finalize(_p(partials), rows, _p(sums), bn.C, float(count), _p(bn.gamma), _p(bn.beta), bn.eps,
                      bn.momentum, _p(bn.moving_mean), _p(bn.moving_var), int(update_moving), _p(bn.scale),
                      _p(bn.shift), _p(bn.mean), _p(bn.invstd), _stream())


def bn_reduce_partials(partials, rows, C2):
    sums = torch.empty(C2, dtype=torch.float64, device=partials.device)
    lib().bn_reduce_partials(_p(partials), rows, C2, _p(sums), _stream())
    return sums


def bn_infer_coeffs(bn):
    lib().bn_infer_coeffs(_p(bn.gamma), _p(bn.beta), _p(bn.moving_mean), _p(bn.moving_var), bn.eps, _p(bn.scale),
                          _p(bn.shift), _p(bn.mean), _p(bn.invstd), bn.C, _stream())


def bn_backward(bn, g, z, act, partials, frozen=False, out=None, sums=None):
    """g: gradient w.r.t. act(bn(z)); returns dz (in place in g unless out is given)"""
    M = _rows(z)
    gp, ldg = _pl(g)
    zp, ldz = _pl(z)
    rows = ctypes.c_int(0)
    if not frozen and sums is None:
        lib().bn_bwd_reduce(gp, ldg, zp, ldz, _p(bn.scale), _p(bn.shift), act, _p(bn.mean), _p(bn.invstd),
                            _p(partials), ctypes.byref(rows), M, bn.C, _stream())
    lib().bn_bwd_finalize(_p(partials), rows.value, _p(sums), bn.C, float(M), _p(bn.gamma), _p(bn.invstd),
                          _p(bn.scale), int(frozen), _p(bn.dgamma), _p(bn.dbeta), _p(bn.coef), _stream())
    dz = out if out is not None else g
    dp, ldd = _pl(dz)
    lib().bn_bwd_apply(gp, ldg, zp, ldz, _p(bn.scale), _p(bn.shift), act, _p(bn.mean), _p(bn.invstd), _p(bn.coef),
                       dp, ldd, 0, M, bn.C, _stream())
    return dz


# ------------------------------------------------------------------------------------- elementwise
def affine_act(x, scale=None, shift=None, act=ACT_NONE, residual=None, rscale=None, rshift=None, ract=ACT_NONE,
               dropout_rate=0.0, seed=0, step_counter=None, out=None):
    C = x.shape[-1]
    y = out if out is not None else torch.empty(x.shape, dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    rp, ldr = _pl(residual)
    yp, ldy = _pl(y)
    lib().affine_act(xp, ldx, _p(scale), _p(shift), act, rp, ldr, _p(rscale), _p(rshift), ract, float(dropout_rate),
                     int(seed), _p(step_counter), yp, ldy, _rows(x), C, _stream())
    return y


def scale_mask_bwd(gy, dropout_rate=0.0, seed=0, step_counter=None, out=None, accumulate=False):
    C = gy.shape[-1]
    gx = out if out is not None else torch.empty(gy.shape, dtype=torch.float32, device=gy.device)
    gp, ldg = _pl(gy)
    xp, ldx = _pl(gx)
    lib().scale_mask_bwd(gp, ldg, float(dropout_rate), int(seed), _p(step_counter), xp, ldx, int(accumulate),
                         _rows(gy), C, _stream())
    return gx


def dropout_mask(shape, rate, seed, step_counter, device):
    C = shape[-1]
    m = torch.empty(shape, dtype=torch.float32, device=device)
    lib().dropout_mask(float(rate), int(seed), _p(step_counter), _p(m), m.numel() // C, C, _stream())
    return m


def _pool_ws(N, HW, C, device, chunked):
    """zeroed ticket + partial-row workspace of the chunked per-image reductions (None: one workgroup per image)"""
    if not chunked:
        return None, 0
    nbytes = lib().pool_workspace(N, HW, C)
    return torch.zeros(nbytes // 4, dtype=torch.float32, device=device), nbytes


def global_avgpool_fwd(x, in_scale=None, in_shift=None, in_act=ACT_NONE, out_scale=1.0, out=None, chunked=True):
    N, H, W, C = x.shape
    y = out if out is not None else torch.empty((N, 1, 1, C), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    ws, wsb = _pool_ws(N, H * W, C, x.device, chunked)
    lib().global_avgpool_fwd(xp, ldx, _p(in_scale), _p(in_shift), in_act, yp, ldy, float(out_scale), N, H * W, C,
                             _p(ws), wsb, _stream())
    return y


def global_avgpool_bwd(gy, H, W, out=None, accumulate=False):
    N, C = gy.shape[0], gy.shape[-1]
    gx = out if out is not None else torch.empty((N, H, W, C), dtype=torch.float32, device=gy.device)
    gp, ldg = _pl(gy)
    xp, ldx = _pl(gx)
    lib().global_avgpool_bwd(gp, ldg, xp, ldx, int(accumulate), N, H * W, C, _stream())
    return gx


def maxpool2d_fwd(x, k, stride, pad, in_scale=None, in_shift=None, in_act=ACT_NONE, argmax=None):
    """x (N,H,W,C), explicit zero padding pad = (top, bottom, left, right) then VALID max pooling"""
    N, H, W, C = x.shape
    pt, pb, pl, pr = pad
    Ho, Wo = (H + pt + pb - k) // stride + 1, (W + pl + pr - k) // stride + 1
    y = torch.empty((N, Ho, Wo, C), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    lib().maxpool2d_fwd(xp, ldx, _p(in_scale), _p(in_shift), in_act, yp, ldy, _p(argmax), N, H, W, C, k, stride, pt, pl, Ho, Wo,
                        _stream())
    return y


def maxpool2d_bwd(x, dy, k, stride, pad, in_scale=None, in_shift=None, in_act=ACT_NONE, out=None, accumulate=False,
                  argmax=None):
    N, H, W, C = x.shape
    pt, pb, pl, pr = pad
    Ho, Wo = dy.shape[1], dy.shape[2]
    gx = out if out is not None else torch.empty(x.shape, dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    dp, ldd = _pl(dy)
    gp, ldg = _pl(gx)
    lib().maxpool2d_bwd(xp, ldx, _p(in_scale), _p(in_shift), in_act, dp, ldd, _p(argmax), gp, ldg, int(accumulate), N, H, W, C,
                        k, stride, pt, pl, Ho, Wo, _stream())
    return gx


def conv_narrow_fwd(x, w, in_scale=None, in_shift=None, in_act=ACT_NONE, out=None, stats=False):
    """3x3 stride-1 'same' conv, Cout <= 32 (csrc/conv_narrow.hip): x (N,H,W,Cin), w (3,3,Cin,Cout) -> y (N,H,W,Cout)
    [, the statistics partial rows (rows, 2, Cout) when stats]"""
    N, H, W, Cin = x.shape
    Cout = w.shape[-1]
    y = out if out is not None else torch.empty((N, H, W, Cout), dtype=torch.float32, device=x.device)
    part = torch.zeros((1024, 2, Cout), dtype=torch.float32, device=x.device) if stats else None
    rows = ctypes.c_int(0)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    lib().conv_narrow_fwd(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(w.contiguous()), yp, ldy, _p(part),
                          ctypes.byref(rows), N, H, W, Cin, Cout, _stream())
    return (y, part[:rows.value]) if stats else y


def conv_narrow_bwd_data(dy, w, out=None, accumulate=False):
    """d/d(act(x)) of conv_narrow_fwd"""
    N, H, W, Cout = dy.shape
    Cin = w.shape[2]
    gx = out if out is not None else torch.empty((N, H, W, Cin), dtype=torch.float32, device=dy.device)
    dp, ldd = _pl(dy)
    gp, ldg = _pl(gx)
    lib().conv_narrow_bwd_data(dp, ldd, _p(w.contiguous()), gp, ldg, int(accumulate), N, H, W, Cin, Cout, _stream())
    return gx


def conv_narrow_bwd_weight(x, dy, in_scale=None, in_shift=None, in_act=ACT_NONE):
    """gw (3,3,Cin,Cout) of conv_narrow_fwd (slabs + the deterministic row reduction)"""
    N, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    gw = torch.empty((3, 3, Cin, Cout), dtype=torch.float32, device=x.device)
    nbytes = lib().conv_narrow_bwd_weight_workspace(N, H, W, Cin, Cout)
    ws = torch.empty(nbytes // 4 + 4, dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    dp, ldd = _pl(dy)
    lib().conv_narrow_bwd_weight(xp, ldx, _p(in_scale), _p(in_shift), in_act, dp, ldd, _p(gw), _p(ws), nbytes, N, H, W, Cin,
                                 Cout, _stream())
    return gw


def avgpool2d_fwd(x, k, stride, in_scale=None, in_shift=None, in_act=ACT_NONE, out=None):
    """x (N,H,W,C) -> AveragePooling2D((k,k), strides, 'valid'); `out` may be a channel slice of a wider buffer"""
    N, H, W, C = x.shape
    Ho, Wo = (H - k) // stride + 1, (W - k) // stride + 1
    y = out if out is not None else torch.empty((N, Ho, Wo, C), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    lib().avgpool2d_fwd(xp, ldx, _p(in_scale), _p(in_shift), in_act, yp, ldy, N, H, W, C, k, stride, Ho, Wo, _stream())
    return y


def avgpool2d_bwd(dy, x_shape, k, stride, out=None, accumulate=False):
    """d/d(activated input) of AveragePooling2D; `out` (+)= it"""
    N, H, W, C = x_shape
    Ho, Wo = dy.shape[1], dy.shape[2]
    gx = out if out is not None else torch.empty(x_shape, dtype=torch.float32, device=dy.device)
    dp, ldd = _pl(dy)
    gp, ldg = _pl(gx)
    lib().avgpool2d_bwd(dp, ldd, gp, ldg, int(accumulate), N, H, W, C, k, stride, Ho, Wo, _stream())
    return gx


def resize_bilinear_fwd(x, H, W, out=None):
    N, h, w, C = x.shape
    y = out if out is not None else torch.empty((N, H, W, C), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    lib().resize_bilinear_fwd(xp, ldx, yp, ldy, N, h, w, C, H, W, _stream())
    return y


def resize_bilinear_bwd(gy, h, w, out=None, accumulate=False):
    N, H, W, C = gy.shape
    gx = out if out is not None else torch.empty((N, h, w, C), dtype=torch.float32, device=gy.device)
    gp, ldg = _pl(gy)
    xp, ldx = _pl(gx)
    lib().resize_bilinear_bwd(gp, ldg, xp, ldx, int(accumulate), N, h, w, C, H, W, _stream())
    return gx


# ------------------------------------------------------------------------------------- head / loss
def upsample_softmax_ce(z, C, H, W, labels=None, ignore_index=255, want_probs=False, want_logits=False,
                        want_grad=False, ld_big=None, loss=('ce',), pixel_weights=None):
    """z (N,h,w,Cpad) small logits -> dict(loss, probs (N,H,W,C), logits (N,H,W,ld_big), dlogits)"""
    N, h, w, _ = z.shape
    dev = z.device
    ld_big = ld_big or ((C + 3) // 4) * 4
    zp, ldz = _pl(z)
    out = {}
    probs = torch.empty((N, H, W, C), dtype=torch.float32, device=dev) if want_probs else None
    logits = torch.zeros((N, H, W, ld_big), dtype=torch.float32, device=dev) if want_logits else None
    dlog = torch.zeros((N, H, W, ld_big), dtype=torch.float32, device=dev) if want_grad else None
    partial = torch.zeros(MAX_STAT_ROWS, dtype=torch.float32, device=dev) if labels is not None else None
    rows = ctypes.c_int(0)
    inv = 1.0 / float(N * H * W)
    # loss: ('ce',) | ('weighted', weight tensor [C]) | ('focal', gamma, alpha)
    kind = {'ce': 0, 'weighted': 1, 'focal': 2}[loss[0]]
    cw = loss[1] if kind == 1 else None
    gamma, alpha = (float(loss[1]), float(loss[2])) if kind == 2 else (0.0, 0.0)
    lib().upsample_softmax_loss(zp, ldz, _p(labels), int(ignore_index or 0), inv, kind, _p(cw), gamma, alpha,
                                _p(pixel_weights), _p(logits), _p(probs), _p(dlog), ld_big, _p(partial), ctypes.byref(rows),
                                N, h, w, C, H, W, _stream())
    if labels is not None:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        lib().reduce_rows(_p(partial), rows.value, 1, _p(loss), 0, _stream())
        out['loss'] = loss
    out['probs'], out['logits'], out['dlogits'] = probs, logits, dlog
    return out


def argmax_confusion(z, C, H, W, labels=None, confusion=None, want_mask=False):
    """z (N,h,w,Cpad) small logits -> (pred mask (N,H,W) int32 or None, confusion (C,C) int64 or None); an existing
    `confusion` tensor is accumulated into (eval.py:443)"""
    N, h, w, _ = z.shape
    zp, ldz = _pl(z)
    pred = torch.empty((N, H, W), dtype=torch.int32, device=z.device) if want_mask else None
    if labels is not None and confusion is None:
        confusion = torch.zeros((C, C), dtype=torch.int64, device=z.device)
    lib().argmax_confusion(zp, ldz, _p(labels), _p(pred), _p(confusion) if labels is not None else None, N, h, w, C, H, W,
                           _stream())
    return pred, (confusion if labels is not None else None)


def tta_accumulate(z, z_mirror, C, H, W, weight, acc=None, write=True, labels=None, confusion=None, want_mask=False):
    """one scale of the multi-scale / mirrored evaluation: acc (N,H,W,Cpad) = (acc + weight * softmax(upsample(z))) + weight *
    mirror_x(softmax(upsample(z_mirror))); z / z_mirror (N,h,w,Cpad) small logits, either may be None.  acc None starts from 0;
    write=False leaves the sum unwritten (the last pass: only the mask and / or the counters are wanted).
    -> (acc or None, pred mask (N,H,W) int32 or None, confusion (C,C) int64 or None) of the sum after this call"""
    ref = z if z is not None else z_mirror
    N, h, w, _ = ref.shape
    zp, ldz = _pl(z)
    mp, ldm = _pl(z_mirror)
    cpad = ((C + 3) // 4) * 4
    out = None
    if write:
        out = acc if acc is not None else torch.empty((N, H, W, cpad), dtype=torch.float32, device=ref.device)
    ap, lda = _pl(acc)
    op, ldo = _pl(out)
    if acc is not None and out is not None and lda != ldo:
        raise Dl3pError('tta_accumulate: one row stride for the sum read and written')
    pred = torch.empty((N, H, W), dtype=torch.int32, device=ref.device) if want_mask else None
    if labels is not None and confusion is None:
        confusion = torch.zeros((C, C), dtype=torch.int64, device=ref.device)
    lib().tta_accumulate(zp, ldz, mp, ldm, h, w, float(weight), ap, op, lda or ldo, _p(labels), _p(pred),
                         _p(confusion) if labels is not None else None, N, C, H, W, _stream())
    return out, pred, (confusion if labels is not None else None)


def label_prepare(labels_u8, num_classes, ignore_index=255, adaptive=False, labels_out=None, weights_out=None):
    """uint8 labels (N, P) on the device -> (float32 labels with values above num_classes-1 set to ignore_index,
    float32 'balanced' pixel weights or None): deeplabv3p/data.py:116-145"""
    N, P = labels_u8.shape
    assert labels_u8.dtype == torch.uint8 and labels_u8.is_contiguous()
    if labels_out is None:
        labels_out = torch.empty((N, P), dtype=torch.float32, device=labels_u8.device)
    hist = None
    if adaptive:
        if weights_out is None:
            weights_out = torch.empty((N, P), dtype=torch.float32, device=labels_u8.device)
        hist = torch.empty(N * 256, dtype=torch.int32, device=labels_u8.device)
    lib().label_prepare(labels_u8.data_ptr(), labels_out.data_ptr(), _p(weights_out) if adaptive else None, _p(hist), N, P,
                        num_classes, ignore_index, _stream())
    return labels_out, (weights_out if adaptive else None)


def head_train_supported(h, w, C, H, W):
    return bool(lib().head_train_supported(h, w, C, H, W))


def head_train_rows_supported(h, w, C, H, W):
    return bool(lib().head_train_rows_supported(h, w, C, H, W))


def head_train(z, C, H, W, labels, ignore_index=255, rows_form=False):
    """fused training head: z (N,h,w,Cpad) -> (loss [1], d loss / d z (N,h,w,Cpad)) without the (N,H,W,C) gradient;
    rows_form: dl3p_head_train_rows (the row-walking kernel) instead of dl3p_head_train (the tile kernel)"""
    N, h, w, cp = z.shape
    dev = z.device
    zp, ldz = _pl(z)
    gz = torch.zeros((N, h, w, cp), dtype=torch.float32, device=dev)
    partial = torch.zeros(MAX_STAT_ROWS, dtype=torch.float32, device=dev)
    rows = ctypes.c_int(0)
    if rows_form:
        wsb = lib().head_train_rows_workspace(N, h, w, C, H, W)
        ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
        lib().head_train_rows(zp, ldz, _p(labels), int(ignore_index or 0), 1.0 / float(N * H * W), _p(gz), cp, 0, _p(partial),
                              ctypes.byref(rows), _p(ws), wsb, N, h, w, C, H, W, _stream())
    else:
        lib().head_train(zp, ldz, _p(labels), int(ignore_index or 0), 1.0 / float(N * H * W), _p(gz), cp, 0, _p(partial),
                         ctypes.byref(rows), N, h, w, C, H, W, _stream())
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    lib().reduce_rows(_p(partial), rows.value, 1, _p(loss), 0, _stream())
    return loss, gz


def sgd_momentum(w, v, g, lr_dev, momentum=0.9, l2=0.0, grad_scale=1.0, l2_elem=None, lr_scale_elem=None):
    lib().sgd_momentum(_p(w), _p(v), _p(g), w.numel(), _p(lr_dev), float(momentum), float(l2), float(grad_scale),
                       _p(l2_elem), _p(lr_scale_elem), _stream())


class GradClipMap:
    """the tables of the dl3p_grad_clip_* calls for variables (offset, length) of one flat buffer, in floats and both multiples
    of 4: `vars` [nvars][3] = {offset, length, first block} and `blockmap` [nblocks][2] = {variable, block within it}, on `device`
    and (the copies the library checks before it launches) on the host; plus the buffers the three calls share: partials
    (float64, one per block), scale (float32, one per variable), norm (float64, per variable and, last, the global norm)"""

    def __init__(self, variables, device):
        import numpy as np
        per = lib().grad_clip_block_elements()
        rows, blocks = [], []
        for v, (off, n) in enumerate(variables):
            nb = (int(n) + per - 1) // per
            rows.append((int(off), int(n), len(blocks)))
            blocks += [(v, b) for b in range(nb)]
        self.vars_host = np.ascontiguousarray(np.array(rows, dtype=np.int64).reshape(-1, 3))
        self.blockmap_host = np.ascontiguousarray(np.array(blocks, dtype=np.int32).reshape(-1, 2))
        self.nvars, self.nblocks = len(rows), len(blocks)
        self.vars = torch.from_numpy(self.vars_host).to(device)
        self.blockmap = torch.from_numpy(self.blockmap_host).to(device)
        self.partials = torch.zeros(max(self.nblocks, 1), dtype=torch.float64, device=device)
        self.scale = torch.ones(max(self.nvars, 1), dtype=torch.float32, device=device)
        self.norm = torch.zeros(self.nvars + 1, dtype=torch.float64, device=device)

    def var_args(self):
        return self.vars.data_ptr(), self.vars_host.ctypes.data, self.nvars

    def block_args(self):
        return self.blockmap.data_ptr(), self.blockmap_host.ctypes.data, self.nblocks


def grad_clip_sumsq(g, w, cmap, grad_scale=1.0, clip_value=0.0, l2_elem=None, lr_scale_elem=None):
    """cmap.partials[b] = sum of clamp(g * grad_scale + 2 * l2_elem * w)^2 over the trainable elements of block b"""
    lib().grad_clip_sumsq(_p(g), _p(w), _p(l2_elem), _p(lr_scale_elem), g.numel(), float(grad_scale), float(clip_value),
                          *cmap.var_args(), *cmap.block_args(), _p(cmap.partials), _stream())


def grad_clip_finalize(cmap, mode, threshold):
    """cmap.partials -> cmap.norm, cmap.scale; mode 1: threshold / max(norm_v, threshold) per variable, 2: one scale from the
    global norm"""
    lib().grad_clip_finalize(_p(cmap.partials), *cmap.var_args(), cmap.nblocks, int(mode), float(threshold), _p(cmap.scale),
                             _p(cmap.norm), _stream())


def grad_clip_apply(g, w, cmap, grad_scale=1.0, clip_value=0.0, l2_elem=None, lr_scale_elem=None, scaled=True, partials=False):
    """g <- clamp(g * grad_scale + 2 * l2_elem * w) * cmap.scale[variable] in place on the trainable elements (scaled=False: the
    clamp alone; partials=True: also leave the sums of squares of the clamped gradient in cmap.partials)"""
    lib().grad_clip_apply(_p(g), _p(w), _p(l2_elem), _p(lr_scale_elem), g.numel(), float(grad_scale), float(clip_value),
                          _p(cmap.scale) if scaled else None, *cmap.var_args(), *cmap.block_args(),
                          _p(cmap.partials) if partials else None, _stream())


def act_bwd(g, z, act, out, accumulate=False):
    """out (+)= g * act'(z): backward of a bare activation on a materialised tensor"""
    gp, ldg = _pl(g)
    zp, ldz = _pl(z)
    op, ldo = _pl(out)
    lib().bn_bwd_apply(gp, ldg, zp, ldz, None, None, act, None, None, None, op, ldo, int(accumulate), _rows(z),
                       z.shape[-1], _stream())
    return out


def im2col(x, k, stride=1, rate=1, padding='same', in_scale=None, in_shift=None, in_act=ACT_NONE):
    N, H, W, Cin = x.shape
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    kp = (k * k * Cin + 3) // 4 * 4
    col = torch.empty((N, Ho, Wo, kp), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    lib().im2col(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(col), kp, N, H, W, Cin, k, stride, rate, pt, pl, Ho, Wo,
                 _stream())
    return col


def conv2d_gemm_supported(Cin, Cout, k, stride):
    return bool(lib().conv2d_gemm_supported(Cin, Cout, k, stride))


def conv2d_gemm_plan_query(role, M, K, N):
    """the plan of a dense-conv implicit GEMM without launching it (include/dl3p.h: dl3p_conv2d_gemm_plan_query) -> the six ints"""
    out = (ctypes.c_int * 6)()
    lib().conv2d_gemm_plan_query(role, M, K, N, out)
    return tuple(out)


def conv2d_gemm_fwd(x, w, stride=1, rate=1, padding='same', in_scale=None, in_shift=None, in_act=ACT_NONE, bias=None,
                    partials=None, out=None):
    """dense conv as an implicit GEMM (no im2col matrix): x (N,H,W,Cin), w (k,k,Cin,Cout) -> y (N,Ho,Wo,Cout) [, rows];
    `out` may be a channel slice of a wider buffer"""
    N, H, W, Cin = x.shape
    k, Cout = w.shape[0], w.shape[-1]
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    wt = w.reshape(k * k * Cin, Cout).t().contiguous()
    y = out if out is not None else torch.empty((N, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    rows = ctypes.c_int(0)
    lib().conv2d_gemm_fwd(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(wt), _p(bias), yp, ldy, _p(partials),
                          ctypes.byref(rows), N, H, W, Cin, Cout, k, stride, rate, pt, pl, Ho, Wo, _stream())
    return (y, rows.value) if partials is not None else y


def conv2d_gemm_bwd_data(dy, w, x_shape, stride=1, rate=1, padding='same', out=None, accumulate=False):
    N, H, W, Cin = x_shape
    k, Cout = w.shape[0], w.shape[-1]
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    wd = torch.empty(Cin * k * k * Cout, dtype=torch.float32, device=dy.device)
    lib().conv2d_gemm_dgrad_weights(_p(w.contiguous()), _p(wd), k, Cin, Cout, _stream())
    gx = out if out is not None else torch.empty(x_shape, dtype=torch.float32, device=dy.device)
    dp, ldd = _pl(dy)
    gp, ldg = _pl(gx)
    lib().conv2d_gemm_bwd_data(dp, ldd, _p(wd), gp, ldg, int(accumulate), N, H, W, Cin, Cout, k, stride, rate, pt, pl, Ho,
                               Wo, _stream())
    return gx


def conv2d_gemm_bwd_weight(x, dy, k, stride=1, rate=1, padding='same', in_scale=None, in_shift=None, in_act=ACT_NONE,
                           with_bias=False):
    N, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    need = lib().conv2d_gemm_bwd_weight_workspace(N, Ho, Wo, Cin, Cout, k)
    ws = torch.empty(need // 4 + 4, dtype=torch.float32, device=x.device)
    gw = torch.empty((k, k, Cin, Cout), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    dp, ldd = _pl(dy)
    gb = torch.empty(Cout, dtype=torch.float32, device=x.device) if with_bias else None
    lib().conv2d_gemm_bwd_weight(xp, ldx, _p(in_scale), _p(in_shift), in_act, dp, ldd, _p(gw), _p(gb), _p(ws), need, N, H, W,
                                 Cin, Cout, k, stride, rate, pt, pl, Ho, Wo, _stream())
    return (gw, gb) if with_bias else gw


def conv2d_gemm_fwd_sb(x, w, stride=1, rate=1, padding='same', in_scale=None, in_shift=None, in_act=ACT_NONE, bias=None,
                       partials=None, out=None):
    """conv2d_gemm_fwd on the split-bf16 kernel (the kernel operand pre-split here: [3][Cout][pitch >= k k Cin])"""
    N, H, W, Cin = x.shape
    k, Cout = w.shape[0], w.shape[-1]
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    wsp = split_bf16x3(w.reshape(k * k * Cin, Cout).t().contiguous())
    y = out if out is not None else torch.empty((N, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    rows = ctypes.c_int(0)
    lib().conv2d_gemm_fwd_sb(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(wsp), wsp.shape[2], _p(bias), yp, ldy, _p(partials),
                             ctypes.byref(rows), N, H, W, Cin, Cout, k, stride, rate, pt, pl, Ho, Wo, _stream())
    return (y, rows.value) if partials is not None else y


def conv2d_gemm_bwd_data_sb(dy, w, x_shape, stride=1, rate=1, padding='same', out=None, accumulate=False):
    """conv2d_gemm_bwd_data on the split-bf16 kernel (wd = conv2d_gemm_dgrad_weights(w) pre-split: [3][Cin][pitch >= k k Cout])"""
    N, H, W, Cin = x_shape
    k, Cout = w.shape[0], w.shape[-1]
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    wd = torch.empty((Cin, k * k * Cout), dtype=torch.float32, device=dy.device)
    lib().conv2d_gemm_dgrad_weights(_p(w.contiguous()), _p(wd), k, Cin, Cout, _stream())
    wdsp = split_bf16x3(wd)
    gx = out if out is not None else torch.empty(x_shape, dtype=torch.float32, device=dy.device)
    dp, ldd = _pl(dy)
    gp, ldg = _pl(gx)
    lib().conv2d_gemm_bwd_data_sb(dp, ldd, _p(wdsp), wdsp.shape[2], gp, ldg, int(accumulate), N, H, W, Cin, Cout, k, stride, rate,
                                  pt, pl, Ho, Wo, _stream())
    return gx


def stem_conv_supported(Cin, Cout, k, stride, rate):
    return bool(lib().stem_conv_supported(Cin, Cout, k, stride, rate))


def stem_conv_fwd(x, w, padding='same', partials=None):
    """the RGB stem (3x3 stride 2) without an im2col matrix: x (N,H,W,3); w (3,3,3,Cout) -> y (N,Ho,Wo,Cout) [, rows]"""
    N, H, W, Cin = x.shape
    Cout = w.shape[-1]
    assert stem_conv_supported(Cin, Cout, w.shape[0], 2, 1)
    Ho, Wo, pt, pl = conv_geometry(H, W, 3, 2, 1, padding)
    wk = torch.zeros((28, Cout), dtype=torch.float32, device=x.device)
    wk[:27] = w.reshape(27, Cout)
    y = torch.empty((N, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    rows = ctypes.c_int(0)
    lib().stem_conv_fwd(xp, ldx, _p(wk), _p(y), Cout, _p(partials), ctypes.byref(rows), N, H, W, Cout, pt, pl, Ho, Wo,
                        _stream())
    return (y, rows.value) if partials is not None else y


def stem_conv_bwd_weight(x, dy, padding='same'):
    """-> gw (3,3,3,Cout)"""
    N, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    Ho, Wo, pt, pl = conv_geometry(H, W, 3, 2, 1, padding)
    need = lib().stem_conv_bwd_weight_workspace(N, Ho, Wo, Cout)
    ws = torch.empty(need // 4, dtype=torch.float32, device=x.device)
    gw = torch.full((28, Cout), float('nan'), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    dp, ldd = _pl(dy)
    lib().stem_conv_bwd_weight(xp, ldx, dp, ldd, _p(gw), _p(ws), need, N, H, W, Cout, pt, pl, Ho, Wo, _stream())
    assert float(gw[27].abs().max()) == 0.0
    return gw[:27].reshape(3, 3, 3, Cout)


def stem_conv_bwd_weight_bn(x, g, z, bn, act, padding='same'):
    """stem weight gradient with the BatchNorm-backward apply of (g, z) folded in (bn: BNState after bn_backward's finalize) -> gw"""
    N, H, W, Cin = x.shape
    Cout = g.shape[-1]
    Ho, Wo, pt, pl = conv_geometry(H, W, 3, 2, 1, padding)
    need = lib().stem_conv_bwd_weight_workspace(N, Ho, Wo, Cout)
    ws = torch.empty(need // 4, dtype=torch.float32, device=x.device)
    gw = torch.empty((28, Cout), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    gp, ldg = _pl(g)
    zp, ldz = _pl(z)
    rows = ctypes.c_int(0)
    lib().stem_conv_bwd_weight_slabs_bn(xp, ldx, gp, ldg, zp, ldz, _p(bn.scale), _p(bn.shift), act, _p(bn.mean), _p(bn.invstd),
                                        _p(bn.coef), _p(ws), need, ctypes.byref(rows), N, H, W, Cout, pt, pl, Ho, Wo, _stream())
    lib().reduce_rows(_p(ws), rows.value, 28 * Cout, _p(gw), 0, _stream())
    return gw[:27].reshape(3, 3, 3, Cout)


def col2im(gcol, x_shape, k, stride=1, rate=1, padding='same', out=None, accumulate=False):
    N, H, W, Cin = x_shape
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    gx = out if out is not None else torch.empty(x_shape, dtype=torch.float32, device=gcol.device)
    gp, ldg = _pl(gx)
    lib().col2im(_p(gcol), gcol.shape[-1], gp, ldg, int(accumulate), N, H, W, Cin, k, stride, rate, pt, pl, Ho, Wo,
                 _stream())
    return gx


def scale_bcast_fwd(x, s, scale=None, shift=None, act=ACT_NONE, s_act=ACT_NONE, out=None):
    """y = act(x*scale+shift) * s_act(s)[n]  with s (N,1,1,C): the SE-block Multiply"""
    N, H, W, C = x.shape
    y = out if out is not None else torch.empty(x.shape, dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    sp, lds = _pl(s)
    yp, ldy = _pl(y)
    lib().scale_bcast_fwd(xp, ldx, _p(scale), _p(shift), act, sp, lds, s_act, yp, ldy, N, H * W, C, _stream())
    return y


def scale_bcast_bwd(gy, x, s, scale=None, shift=None, act=ACT_NONE, s_act=ACT_NONE, chunked=True):
    N, H, W, C = x.shape
    gx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    gs = torch.empty((N, 1, 1, C), dtype=torch.float32, device=x.device)
    gp, ldg = _pl(gy)
    xp, ldx = _pl(x)
    sp, lds = _pl(s)
    ws, wsb = _pool_ws(N, H * W, C, x.device, chunked)
    lib().scale_bcast_bwd(gp, ldg, xp, ldx, _p(scale), _p(shift), act, sp, lds, s_act, _p(gx), C, 0, _p(gs), C, N, H * W, C,
                          _p(ws), wsb, _stream())
    return gx, gs


# ------------------------------------------------------------------------------------- mixed precision (bf16 storage)
# wrappers over the *_bf16 entry points: activation tensors are torch.bfloat16 (or float32 where the C ABI takes an
# `*_is_f32` flag), BatchNorm coefficients / partial rows / weight gradients float32
def _plb(t):
    """(device pointer, row stride in ELEMENTS, is_f32) of a bf16 (or f32) activation tensor or channel-slice view"""
    if t is None:
        return None, 0, 0
    if not t.is_cuda or t.dtype not in (torch.bfloat16, torch.float32):
        raise Dl3pError('bf16 ops need bfloat16 / float32 tensors on the HIP device (got %s on %s)' % (t.dtype, t.device))
    if t.stride(-1) != 1:
        raise Dl3pError('channel dim must be contiguous')
    ld = t.stride(-2) if t.dim() >= 2 else t.shape[-1]
    return t.data_ptr(), ld, int(t.dtype == torch.float32)


def _bf(t):
    return t if t.dtype == torch.bfloat16 else t.to(torch.bfloat16)


def pwconv_fwd_bf16(x, w, bias=None, in_scale=None, in_shift=None, in_act=ACT_NONE, partials=None, out_f32=False):
    """x (.., K) bf16 / f32, w (K, N) float32 master kernel -> y (.., N) bf16 (f32 with out_f32); (y, rows) with partials"""
    K, Nn = w.shape
    M = _rows(x)
    wt = _bf(w.t().contiguous())
    y = torch.empty(tuple(x.shape[:-1]) + (Nn,), dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    xp, ldx, xf = _plb(x)
    yp, ldy, yf = _plb(y)
    rows = ctypes.c_int(0)
    lib().pwconv_fwd_bf16(xp, ldx, xf, _p(in_scale), _p(in_shift), in_act, _p(wt), _p(bias), yp, ldy, yf, _p(partials),
                          ctypes.byref(rows), M, K, Nn, _stream())
    return (y, rows.value) if partials is not None else y


def pwconv_bwd_data_bf16(dy, w, out=None, accumulate=False):
    K, Nn = w.shape
    M = _rows(dy)
    gx = out if out is not None else torch.empty(tuple(dy.shape[:-1]) + (K,), dtype=torch.bfloat16, device=dy.device)
    dp, ldd, df = _plb(dy)
    gp, ldg, _ = _plb(gx)
    lib().pwconv_bwd_data_bf16(dp, ldd, df, _p(_bf(w.contiguous())), gp, ldg, int(accumulate), M, K, Nn, _stream())
    return gx


def pwconv_bwd_data_bn_bf16(dy, w, z, scale, shift, act, mean, invstd, partials, out=None, accumulate=False):
    """bf16 data gradient + the BatchNorm-backward partial sums of the BatchNorm behind it -> (gx, rows)"""
    K, Nn = w.shape
    M = _rows(dy)
    gx = out if out is not None else torch.empty(tuple(dy.shape[:-1]) + (K,), dtype=torch.bfloat16, device=dy.device)
    dp, ldd, _ = _plb(dy)
    gp, ldg, _ = _plb(gx)
    zp, ldz, _ = _plb(z)
    rows = ctypes.c_int(0)
    lib().pwconv_bwd_data_bn_bf16(dp, ldd, _p(_bf(w.contiguous())), gp, ldg, int(accumulate), M, K, Nn, zp, ldz, _p(scale),
                                  _p(shift), act, _p(mean), _p(invstd), _p(partials), ctypes.byref(rows), _stream())
    return gx, rows.value


def pwconv_bwd_weight_bf16(x, dy, in_scale=None, in_shift=None, in_act=ACT_NONE, with_bias=False):
    K, Nn = x.shape[-1], dy.shape[-1]
    M = _rows(x)
    need = lib().pwconv_bwd_weight_workspace_bf16(M, K, Nn)
    ws = torch.empty(need // 4 + 4, dtype=torch.float32, device=x.device)
    gw = torch.empty((K, Nn), dtype=torch.float32, device=x.device)
    gb = torch.empty((Nn,), dtype=torch.float32, device=x.device) if with_bias else None
    xp, ldx, _ = _plb(x)
    dp, ldd, df = _plb(dy)
    lib().pwconv_bwd_weight_bf16(xp, ldx, _p(in_scale), _p(in_shift), in_act, dp, ldd, df, _p(gw), _p(gb), _p(ws),
                                 ws.numel() * 4, M, K, Nn, _stream())
    return (gw, gb) if with_bias else gw


def dwconv2d_fwd_bf16(x, w, stride=1, rate=1, padding='same', in_scale=None, in_shift=None, in_act=ACT_NONE, partials=None):
    N, H, W, C = x.shape
    k = w.shape[0]
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    y = torch.empty((N, Ho, Wo, C), dtype=torch.bfloat16, device=x.device)
    xp, ldx, _ = _plb(x)
    yp, ldy, _ = _plb(y)
    rows = ctypes.c_int(0)
    lib().dwconv2d_fwd_bf16(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(_bf(w.contiguous())), yp, ldy, _p(partials),
                            ctypes.byref(rows), N, H, W, C, k, stride, rate, pt, pl, Ho, Wo, _stream())
    return (y, rows.value) if partials is not None else y


def dwconv2d_bwd_data_bf16(dy, w, x_shape, stride=1, rate=1, padding='same', out=None, accumulate=False):
    N, H, W, C = x_shape
    k = w.shape[0]
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    gx = out if out is not None else torch.empty((N, H, W, C), dtype=torch.bfloat16, device=dy.device)
    dp, ldd, _ = _plb(dy)
    gp, ldg, _ = _plb(gx)
    lib().dwconv2d_bwd_data_bf16(dp, ldd, _p(_bf(w.contiguous())), gp, ldg, int(accumulate), N, H, W, C, k, stride, rate,
                                 pt, pl, Ho, Wo, _stream())
    return gx


def dwconv2d_bwd_weight_bf16(x, dy, k, stride=1, rate=1, padding='same', in_scale=None, in_shift=None, in_act=ACT_NONE):
    N, H, W, C = x.shape
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    need = lib().dwconv2d_bwd_weight_workspace_bf16(N, Ho, Wo, C, k)
    ws = torch.empty(need // 4 + 4, dtype=torch.float32, device=x.device)
    gw = torch.empty((k, k, C), dtype=torch.float32, device=x.device)
    xp, ldx, _ = _plb(x)
    dp, ldd, _ = _plb(dy)
    lib().dwconv2d_bwd_weight_bf16(xp, ldx, _p(in_scale), _p(in_shift), in_act, dp, ldd, _p(gw), _p(ws), ws.numel() * 4,
                                   N, H, W, C, k, stride, rate, pt, pl, Ho, Wo, _stream())
    return gw


def bn_backward_bf16(bn, g, z, act, partials):
    """in-place BatchNorm backward on bf16 tensors (reduce + finalize + apply); bn: BNState with scale/shift/mean/invstd"""
    M = _rows(z)
    gp, ldg, _ = _plb(g)
    zp, ldz, _ = _plb(z)
    rows = ctypes.c_int(0)
    lib().bn_bwd_reduce_bf16(gp, ldg, zp, ldz, _p(bn.scale), _p(bn.shift), act, _p(bn.mean), _p(bn.invstd), _p(partials),
                             ctypes.byref(rows), M, bn.C, _stream())
    lib().bn_bwd_finalize(_p(partials), rows.value, None, bn.C, float(M), _p(bn.gamma), _p(bn.invstd), _p(bn.scale), 0,
                          _p(bn.dgamma), _p(bn.dbeta), _p(bn.coef), _stream())
    lib().bn_bwd_apply_bf16(gp, ldg, zp, ldz, _p(bn.scale), _p(bn.shift), act, _p(bn.mean), _p(bn.invstd), _p(bn.coef),
                            gp, ldg, 0, M, bn.C, _stream())
    return g


def affine_act_bf16(x, scale=None, shift=None, act=ACT_NONE, residual=None, rscale=None, rshift=None, ract=ACT_NONE):
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    xp, ldx, _ = _plb(x)
    rp, ldr, _ = _plb(residual)
    yp, ldy, _ = _plb(y)
    lib().affine_act_bf16(xp, ldx, _p(scale), _p(shift), act, rp, ldr, _p(rscale), _p(rshift), ract, 0.0, 0, None, yp, ldy,
                          _rows(x), x.shape[-1], _stream())
    return y


def global_avgpool_fwd_bf16(x, in_scale=None, in_shift=None, in_act=ACT_NONE, out_scale=1.0):
    N, H, W, C = x.shape
    y = torch.empty((N, 1, 1, C), dtype=torch.bfloat16, device=x.device)
    ws = torch.zeros(lib().pool_workspace_bf16(N, H * W, C) // 4 + 4, dtype=torch.float32, device=x.device)
    xp, ldx, _ = _plb(x)
    lib().global_avgpool_fwd_bf16(xp, ldx, _p(in_scale), _p(in_shift), in_act, y.data_ptr(), C, float(out_scale), N, H * W, C,
                                  _p(ws), ws.numel() * 4, _stream())
    return y


def scale_bcast_fwd_bf16(x, s, scale=None, shift=None, act=ACT_NONE, s_act=ACT_NONE):
    N, H, W, C = x.shape
    y = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=x.device)
    xp, ldx, _ = _plb(x)
    lib().scale_bcast_fwd_bf16(xp, ldx, _p(scale), _p(shift), act, s.data_ptr(), C, s_act, y.data_ptr(), C, N, H * W, C, _stream())
    return y


def scale_bcast_bwd_bf16(gy, x, s, scale=None, shift=None, act=ACT_NONE, s_act=ACT_NONE):
    N, H, W, C = x.shape
    gx = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=x.device)
    gs = torch.empty((N, 1, 1, C), dtype=torch.bfloat16, device=x.device)
    ws = torch.zeros(lib().pool_workspace_bf16(N, H * W, C) // 4 + 4, dtype=torch.float32, device=x.device)
    gp, ldg, _ = _plb(gy)
    xp, ldx, _ = _plb(x)
    lib().scale_bcast_bwd_bf16(gp, ldg, xp, ldx, _p(scale), _p(shift), act, s.data_ptr(), C, s_act, gx.data_ptr(), C, 0,
                               gs.data_ptr(), C, N, H * W, C, _p(ws), ws.numel() * 4, _stream())
    return gx, gs


def resize_bilinear_fwd_bf16(x, H, W):
    N, h, w, C = x.shape
    y = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=x.device)
    xp, ldx, _ = _plb(x)
    lib().resize_bilinear_fwd_bf16(xp, ldx, y.data_ptr(), C, N, h, w, C, H, W, _stream())
    return y


def resize_bilinear_bwd_bf16(gy, h, w):
    N, H, W, C = gy.shape
    gx = torch.empty((N, h, w, C), dtype=torch.bfloat16, device=gy.device)
    gp, ldg, _ = _plb(gy)
    lib().resize_bilinear_bwd_bf16(gp, ldg, gx.data_ptr(), C, 0, N, h, w, C, H, W, _stream())
    return gx


# ------------------------------------------------------------------------------------- split-bf16 GEMMs (fp32-accurate)
def split_bf16x3(mat):
    """mat (rows, cols) float32 -> (3, rows, pitch) int16: the exact 3-way bf16 split of every element (planes hi, mid, lo),
    pitch = cols rounded up to 32, zero padded -- the pre-split B operand of the *_sb entry points"""
    rows, cols = mat.shape
    assert mat.is_contiguous() and mat.dtype == torch.float32
    pitch = (cols + 31) // 32 * 32
    out = torch.empty((3, rows, pitch), dtype=torch.int16, device=mat.device)
    table = torch.tensor([[0, rows, cols, cols, 0, pitch]], dtype=torch.int64, device=mat.device)
    lib().split_bf16x3_batch(_p(mat), _p(out), _p(table), 1, _stream())
    return out


def pwconv_fwd_sb(x, wt_sp, K, bias=None, in_scale=None, in_shift=None, in_act=ACT_NONE, out=None, partials=None):
    """pwconv_fwd_wt on the bf16 matrix pipe; wt_sp = split_bf16x3(wt) with wt (N, K)"""
    M = _rows(x)
    N, pitch = wt_sp.shape[1], wt_sp.shape[2]
    y = out if out is not None else torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    rows = ctypes.c_int(0)
    lib().pwconv_fwd_sb(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(wt_sp), pitch, _p(bias), yp, ldy, _p(partials),
                        ctypes.byref(rows), M, K, N, _stream())
    return (y, rows.value) if partials is not None else y


def pwconv_bwd_data_sb(dy, w_sp, N, out=None, accumulate=False, z=None, scale=None, shift=None, act=ACT_NONE, mean=None,
                       invstd=None, partials=None):
    """pwconv_bwd_data (z is None) / pwconv_bwd_data_bn on the bf16 matrix pipe; w_sp = split_bf16x3(w) with w (K, N)"""
    M = _rows(dy)
    K, pitch = w_sp.shape[1], w_sp.shape[2]
    gx = out if out is not None else torch.empty(tuple(dy.shape[:-1]) + (K,), dtype=torch.float32, device=dy.device)
    dp, ldd = _pl(dy)
    gp, ldg = _pl(gx)
    zp, ldz = _pl(z)
    rows = ctypes.c_int(0)
    lib().pwconv_bwd_data_sb(dp, ldd, _p(w_sp), pitch, gp, ldg, int(accumulate), M, K, N, zp, ldz or 0, _p(scale), _p(shift), act,
                             _p(mean), _p(invstd), _p(partials), ctypes.byref(rows), _stream())
    return (gx, rows.value) if z is not None else gx


def pwconv_bwd_data_sb_apply(g, z_out, bn_scale, bn_shift, bn_act, bn_mean, bn_invstd, bn_coef, w_sp, N, dz=None, out=None,
                             accumulate=False, z=None, scale=None, shift=None, act=ACT_NONE, mean=None, invstd=None, partials=None):
    """pwconv_bwd_data_sb with the BatchNorm-backward apply of (g, z_out) folded into its staged operand; -> (dz, gx[, rows]):
    dz = bn_coef[0] * (g * act'(z_out * bn_scale + bn_shift) - bn_coef[1] - xhat * bn_coef[2]) is written to `dz` (default: over g)"""
    M = _rows(g)
    K, pitch = w_sp.shape[1], w_sp.shape[2]
    gx = out if out is not None else torch.empty(tuple(g.shape[:-1]) + (K,), dtype=torch.float32, device=g.device)
    dzt = dz if dz is not None else g
    gp_, ldg_ = _pl(g)
    zo, ldzo = _pl(z_out)
    dzp, lddz = _pl(dzt)
    gxp, ldgx = _pl(gx)
    zp, ldz = _pl(z)
    rows = ctypes.c_int(0)
    lib().pwconv_bwd_data_sb_apply(gp_, ldg_, zo, ldzo, _p(bn_scale), _p(bn_shift), bn_act, _p(bn_mean), _p(bn_invstd), _p(bn_coef),
                                   dzp, lddz, _p(w_sp), pitch, gxp, ldgx, int(accumulate), M, K, N, zp, ldz or 0, _p(scale), _p(shift),
                                   act, _p(mean), _p(invstd), _p(partials), ctypes.byref(rows), _stream())
    return (dzt, gx, rows.value) if z is not None else (dzt, gx)


def col2im_bf16(gcol, x_shape, k, stride=1, rate=1, padding='same', out=None, accumulate=False):
    """bf16 twin of col2im: gcol (N,Ho,Wo,kp) bf16 -> gx (N,H,W,Cin) bf16"""
    N, H, W, Cin = x_shape
    Ho, Wo, pt, pl = conv_geometry(H, W, k, stride, rate, padding)
    gx = out if out is not None else torch.empty(x_shape, dtype=torch.bfloat16, device=gcol.device)
    gp, ldg, _ = _plb(gx)
    lib().col2im_bf16(_p(gcol), gcol.shape[-1], gp, ldg, int(accumulate), N, H, W, Cin, k, stride, rate, pt, pl, Ho, Wo, _stream())
    return gx


def maxpool2d_fwd_bf16(x, k, stride, pad, in_scale=None, in_shift=None, in_act=ACT_NONE, argmax=None):
    N, H, W, C = x.shape
    pt, pb, pl, pr = pad
    Ho, Wo = (H + pt + pb - k) // stride + 1, (W + pl + pr - k) // stride + 1
    y = torch.empty((N, Ho, Wo, C), dtype=torch.bfloat16, device=x.device)
    xp, ldx, _ = _plb(x)
    yp, ldy, _ = _plb(y)
    lib().maxpool2d_fwd_bf16(xp, ldx, _p(in_scale), _p(in_shift), in_act, yp, ldy, _p(argmax), N, H, W, C, k, stride, pt, pl, Ho,
                             Wo, _stream())
    return y


def maxpool2d_bwd_bf16(dy, argmax, x_shape, k, stride, pad, out=None, accumulate=False):
    N, H, W, C = x_shape
    pt, pb, pl, pr = pad
    Ho, Wo = dy.shape[1], dy.shape[2]
    gx = out if out is not None else torch.empty(x_shape, dtype=torch.bfloat16, device=dy.device)
    dp, ldd, _ = _plb(dy)
    gp, ldg, _ = _plb(gx)
    lib().maxpool2d_bwd_bf16(dp, ldd, _p(argmax), gp, ldg, int(accumulate), N, H, W, C, k, stride, pt, pl, Ho, Wo, _stream())
    return gx


def avgpool2d_fwd_bf16(x, k, stride, in_scale=None, in_shift=None, in_act=ACT_NONE, out=None):
    N, H, W, C = x.shape
    Ho, Wo = (H - k) // stride + 1, (W - k) // stride + 1
    y = out if out is not None else torch.empty((N, Ho, Wo, C), dtype=torch.bfloat16, device=x.device)
    xp, ldx, _ = _plb(x)
    yp, ldy, _ = _plb(y)
    lib().avgpool2d_fwd_bf16(xp, ldx, _p(in_scale), _p(in_shift), in_act, yp, ldy, N, H, W, C, k, stride, Ho, Wo, _stream())
    return y


def avgpool2d_bwd_bf16(dy, x_shape, k, stride, out=None, accumulate=False):
    N, H, W, C = x_shape
    Ho, Wo = dy.shape[1], dy.shape[2]
    gx = out if out is not None else torch.empty(x_shape, dtype=torch.bfloat16, device=dy.device)
    dp, ldd, _ = _plb(dy)
    gp, ldg, _ = _plb(gx)
    lib().avgpool2d_bwd_bf16(dp, ldd, gp, ldg, int(accumulate), N, H, W, C, k, stride, Ho, Wo, _stream())
    return gx


# ------------------------------------------------------------------------------------- fused inverted-residual block
def irb_supported(x_shape, C, stride=1, padding='same', backward=False):
    N, H, W, K = x_shape
    Ho, Wo, pt, pl = conv_geometry(H, W, 3, stride, 1, padding)
    fn = lib().irb_bwd_supported if backward else lib().irb_supported
    return bool(fn(N, H, W, K, C, 3, stride, 1, pt, pl, Ho, Wo))


def irb_cov_sums(x, in_scale=None, in_shift=None, in_act=ACT_NONE):
    """float64 [K + K*K]: sum over pixels of the (prologue-applied) input and of its outer product"""
    K = x.shape[-1]
    M = _rows(x)
    xp, ldx = _pl(x)
    cap = lib().irb_cov_rows_max()
    rows_buf = torch.empty(cap * (K + K * K), dtype=torch.float64, device=x.device)
    rows = ctypes.c_int(0)
    lib().irb_cov_stats(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(rows_buf), cap, ctypes.byref(rows), M, K, _stream())
    sums = torch.empty(K + K * K, dtype=torch.float64, device=x.device)
    lib().irb_cov_reduce(_p(rows_buf), rows.value, K, _p(sums), _stream())
    return sums


def irb_bn_finalize_cov(bn, sums, w1, count, update_moving=True):
    """the expand BatchNorm's coefficients from the covariance sums of the expand conv's INPUT; w1 (K, C)"""
    K, C = w1.shape[-2], w1.shape[-1]
    lib().irb_bn_finalize_cov(_p(sums), _p(w1), K, C, float(count), _p(bn.gamma), _p(bn.beta), bn.eps, bn.momentum,
                              _p(bn.moving_mean), _p(bn.moving_var), int(update_moving), _p(bn.scale), _p(bn.shift),
                              _p(bn.mean), _p(bn.invstd), _stream())


def irb_fwd(x, w1, bn_scale, bn_shift, bn_act, wdw, stride=1, padding='same', in_scale=None, in_shift=None,
            in_act=ACT_NONE, out=None, partials=None):
    """x (N,H,W,K); w1 (K,C); wdw (3,3,C) -> raw depthwise output (N,Ho,Wo,C) [, rows]"""
    N, H, W, K = x.shape
    C = w1.shape[-1]
    Ho, Wo, pt, pl = conv_geometry(H, W, 3, stride, 1, padding)
    y = out if out is not None else torch.empty((N, Ho, Wo, C), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    rows = ctypes.c_int(0)
    lib().irb_fwd(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(w1), _p(bn_scale), _p(bn_shift), bn_act, _p(wdw), yp, ldy,
                  _p(partials), ctypes.byref(rows), N, H, W, K, C, stride, pt, pl, Ho, Wo, _stream())
    return (y, rows.value) if partials is not None else y


def ghost_fwd_supported(x_shape, C):
    N, H, W, K = x_shape
    return bool(lib().ghost_fwd_supported(N, H, W, K, C))


def ghost_fwd(x, w1, s1, h1, act1, wdw, in_scale=None, in_shift=None, in_act=ACT_NONE, out=None):
    """fused ghost module: x (N,H,W,K); w1 (K,C); s1, h1 (C,); wdw (3,3,C) -> y (N,H,W,2C): the raw primary conv output in
    [0, C), the raw 3x3 depthwise output of act1(z1 * s1 + h1) in [C, 2C); `out`: a (view of a) buffer to write into"""
    N, H, W, K = x.shape
    C = w1.shape[-1]
    y = out if out is not None else torch.empty((N, H, W, 2 * C), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    lib().ghost_fwd(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(w1), _p(s1), _p(h1), act1, _p(wdw), yp, ldy, N, H, W, K, C,
                    _stream())
    return y


def irb_bwd_sums(x, w1, bn, bn_act, wdw, dy, stride=1, padding='same', in_scale=None, in_shift=None, in_act=ACT_NONE):
    """pass A -> (depthwise kernel gradient (3,3,C), BatchNorm-backward sums float64 [2][C])"""
    N, H, W, K = x.shape
    C = w1.shape[-1]
    Ho, Wo, pt, pl = conv_geometry(H, W, 3, stride, 1, padding)
    nbytes = lib().irb_bwd_workspace(0, N, H, W, K, C, stride, pt, pl)
    slabs = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    part = torch.empty(MAX_STAT_ROWS * 2 * C, dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    dp, ldd = _pl(dy)
    rows = ctypes.c_int(0)
    lib().irb_bwd_sums(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(w1), _p(bn.scale), _p(bn.shift), bn_act, _p(bn.mean),
                       _p(bn.invstd), _p(wdw), dp, ldd, _p(slabs), nbytes, ctypes.byref(rows), _p(part), N, H, W, K, C, stride,
                       pt, pl, Ho, Wo, _stream())
    r = rows.value
    gw = slabs[:r * 9 * C].view(r, 9 * C).double().sum(0).float().view(3, 3, C)
    return gw, part, r


def irb_bwd_data(x, w1, bn, bn_act, wdw, dy, stride=1, padding='same', in_scale=None, in_shift=None, in_act=ACT_NONE,
                 out=None, accumulate=False, want_gx=True, front=None):
    """pass B -> (expand kernel gradient (K,C), gx, [front BatchNorm partial rows, rows]); bn.coef must hold the triple;
    front = (z0, scale0, shift0, act0, mean0, invstd0)"""
    N, H, W, K = x.shape
    C = w1.shape[-1]
    Ho, Wo, pt, pl = conv_geometry(H, W, 3, stride, 1, padding)
    nbytes = lib().irb_bwd_workspace(1, N, H, W, K, C, stride, pt, pl)
    slabs = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    gx = None
    if want_gx:
        gx = out if out is not None else torch.empty((N, H, W, K), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    dp, ldd = _pl(dy)
    gp, ldg = _pl(gx)
    rows = ctypes.c_int(0)
    part0 = None
    fz = (None, 0, None, None, ACT_NONE, None, None)
    if front is not None:
        z0, s0, h0, a0, m0, i0 = front
        zp, ldz = _pl(z0)
        fz = (zp, ldz, _p(s0), _p(h0), a0, _p(m0), _p(i0))
        part0 = torch.empty(MAX_STAT_ROWS * 2 * K, dtype=torch.float32, device=x.device)
    lib().irb_bwd_data(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(w1), _p(bn.scale), _p(bn.shift), bn_act, _p(bn.mean),
                       _p(bn.invstd), _p(bn.coef), _p(wdw), dp, ldd, _p(slabs), nbytes, ctypes.byref(rows), gp, ldg,
                       int(accumulate), *fz, _p(part0), N, H, W, K, C, stride, pt, pl, Ho, Wo, _stream())
    r = rows.value
    gw = slabs[:r * K * C].view(r, K * C).double().sum(0).float().view(K, C)
    return gw, gx, part0, r


# ------------------------------------------------------------------------------------- 2x2 stride-2 transposed conv
def deconv2x2_supported(Cin, Cout):
    return bool(lib().deconv2x2_supported(Cin, Cout))


def deconv2x2_fwd(x, w, bias=None, in_scale=None, in_shift=None, in_act=ACT_NONE, out=None):
    """x (N,H,W,Cin); w the Keras Conv2DTranspose kernel as stored, (2,2,Cout,Cin) -> y (N,2H,2W,Cout)"""
    N, H, W, Cin = x.shape
    Cout = w.shape[2]
    y = out if out is not None else torch.empty((N, 2 * H, 2 * W, Cout), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    lib().deconv2x2_fwd(xp, ldx, _p(in_scale), _p(in_shift), in_act, _p(w), _p(bias), yp, ldy, N, H, W, Cin, Cout,
                        _stream())
    return y


def deconv2x2_bwd_data(dy, w, out=None, accumulate=False):
    """dy (N,2H,2W,Cout) -> gx (N,H,W,Cin), the gradient w.r.t. the (activated) input of deconv2x2_fwd"""
    N, H2, W2, Cout = dy.shape
    Cin = w.shape[3]
    gx = out if out is not None else torch.empty((N, H2 // 2, W2 // 2, Cin), dtype=torch.float32, device=dy.device)
    dp, ldd = _pl(dy)
    gp, ldg = _pl(gx)
    lib().deconv2x2_bwd_data(dp, ldd, _p(w), gp, ldg, int(accumulate), N, H2 // 2, W2 // 2, Cin, Cout, _stream())
    return gx


def deconv2x2_bwd_weight(x, dy, in_scale=None, in_shift=None, in_act=ACT_NONE, with_bias=False, workspace=None):
    """-> gw (2,2,Cout,Cin) [, gb (Cout,)]"""
    N, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    need = lib().deconv2x2_bwd_weight_workspace(N, H, W, Cin, Cout)
    ws = workspace if workspace is not None else torch.empty(max(need, 16) // 4, dtype=torch.float32, device=x.device)
    gw = torch.empty((2, 2, Cout, Cin), dtype=torch.float32, device=x.device)
    gb = torch.empty((Cout,), dtype=torch.float32, device=x.device) if with_bias else None
    xp, ldx = _pl(x)
    dp, ldd = _pl(dy)
    lib().deconv2x2_bwd_weight(xp, ldx, _p(in_scale), _p(in_shift), in_act, dp, ldd, _p(gw), _p(gb), _p(ws),
                               ws.numel() * 4, N, H, W, Cin, Cout, _stream())
    return (gw, gb) if with_bias else gw


# ------------------------------------------------------------------------------------- nearest upsampling (Fast-SCNN)
def upsample_add_fwd(a, b, r, a_scale=None, a_shift=None, a_act=ACT_NONE, b_scale=None, b_shift=None, b_act=ACT_NONE, out=None,
                     partials=None):
    """a (N,r h,r w,C) + UpSampling2D(r)(b), b (N,h,w,C), each behind its own prologue -> out [, rows of `partials` written: the
    sum / sum of squares of `out` for the BatchNorm that follows]"""
    N, H, W, C = a.shape
    h, w = b.shape[1], b.shape[2]
    y = out if out is not None else torch.empty((N, H, W, C), dtype=torch.float32, device=a.device)
    ap, lda = _pl(a)
    bp, ldb = _pl(b)
    yp, ldy = _pl(y)
    rows = ctypes.c_int(0)
    lib().upsample_add_fwd(ap, lda, _p(a_scale), _p(a_shift), a_act, bp, ldb, _p(b_scale), _p(b_shift), b_act, yp, ldy,
                           _p(partials), ctypes.byref(rows), N, h, w, C, H, W, r, _stream())
    return (y, rows.value) if partials is not None else y


def block_sum_bwd(g, r, out=None, accumulate=False):
    """g (N,r h,r w,C) -> (N,h,w,C): the sum over every r x r block (the transpose of UpSampling2D(r)); `out` (+)= it"""
    N, H, W, C = g.shape
    h, w = (out.shape[1], out.shape[2]) if out is not None else (H // r, W // r)
    gl = out if out is not None else torch.empty((N, h, w, C), dtype=torch.float32, device=g.device)
    gp, ldg = _pl(g)
    lp, ldl = _pl(gl)
    lib().block_sum_bwd(gp, ldg, lp, ldl, int(accumulate), N, h, w, C, H, W, r, _stream())
    return gl


def winpool2d_fwd(x, kh, kw, in_scale=None, in_shift=None, in_act=ACT_NONE, out=None):
    """x (N,H,W,C) -> AveragePooling2D((kh,kw), strides=(kh,kw), 'valid'): (N, H // kh, W // kw, C); `out` may be a channel slice"""
    N, H, W, C = x.shape
    Ho, Wo = H // kh, W // kw
    y = out if out is not None else torch.empty((N, Ho, Wo, C), dtype=torch.float32, device=x.device)
    xp, ldx = _pl(x)
    yp, ldy = _pl(y)
    lib().winpool2d_fwd(xp, ldx, _p(in_scale), _p(in_shift), in_act, yp, ldy, N, H, W, C, kh, kw, Ho, Wo, _stream())
    return y


def winpool2d_bwd(dy, x_shape, kh, kw, out=None, accumulate=False):
    """d/d(activated input) of winpool2d_fwd; `out` (+)= it, uncovered rows and columns get 0"""
    N, H, W, C = x_shape
    gx = out if out is not None else torch.empty(x_shape, dtype=torch.float32, device=dy.device)
    dp, ldd = _pl(dy)
    gp, ldg = _pl(gx)
    lib().winpool2d_bwd(dp, ldd, gp, ldg, int(accumulate), N, H, W, C, kh, kw, dy.shape[1], dy.shape[2], _stream())
    return gx


def nearest_softmax_probs(z, C, H, W):
    """z (N,h,w,Cpad) logits -> Softmax(UpSampling2D(H / h)(z)) as (N,H,W,C): one softmax per logit pixel"""
    N, h, w, _ = z.shape
    zp, ldz = _pl(z)
    probs = torch.empty((N, H, W, C), dtype=torch.float32, device=z.device)
    lib().nearest_softmax_probs(zp, ldz, _p(probs), N, h, w, C, H, W, _stream())
    return probs


def nearest_head_train(z, C, H, W, labels, ignore_index=255, loss=('ce',), pixel_weights=None, want_grad=True, out=None,
                       accumulate=False):
    """training head behind a nearest upsampling: z (N,h,w,Cpad), labels [N*H*W] -> (loss [1], d loss / d z (N,h,w,Cpad) or None);
    loss: ('ce',) | ('weighted', weight tensor [C]) | ('focal', gamma, alpha), as upsample_softmax_ce"""
    N, h, w, cp = z.shape
    dev = z.device
    zp, ldz = _pl(z)
    gz = out
    if want_grad and gz is None:
        gz = torch.zeros((N, h, w, cp), dtype=torch.float32, device=dev)
    gp, ldg = _pl(gz if want_grad else None)
    partial = torch.zeros(MAX_STAT_ROWS, dtype=torch.float32, device=dev)
    rows = ctypes.c_int(0)
    kind = {'ce': 0, 'weighted': 1, 'focal': 2}[loss[0]]
    cw = loss[1] if kind == 1 else None
    gamma, alpha = (float(loss[1]), float(loss[2])) if kind == 2 else (0.0, 0.0)
    lib().nearest_head_train(zp, ldz, _p(labels), int(ignore_index or 0), 1.0 / float(N * H * W), kind, _p(cw), gamma, alpha,
                             _p(pixel_weights), gp, ldg, int(accumulate), _p(partial), ctypes.byref(rows), N, h, w, C, H, W,
                             _stream())
    total = torch.empty(1, dtype=torch.float32, device=dev)
    lib().reduce_rows(_p(partial), rows.value, 1, _p(total), 0, _stream())
    return total, (gz if want_grad else None)


def nearest_argmax_confusion(z, C, H, W, labels=None, confusion=None, want_mask=False):
    """argmax_confusion behind a nearest upsampling: (pred mask (N,H,W) int32 or None, confusion (C,C) int64 or None)"""
    N, h, w, _ = z.shape
    zp, ldz = _pl(z)
    pred = torch.empty((N, H, W), dtype=torch.int32, device=z.device) if want_mask else None
    if labels is not None and confusion is None:
        confusion = torch.zeros((C, C), dtype=torch.int64, device=z.device)
    lib().nearest_argmax_confusion(zp, ldz, _p(labels), _p(pred), _p(confusion) if labels is not None else None, N, h, w, C, H,
                                   W, _stream())
    return pred, (confusion if labels is not None else None)


def nearest_class_counts(z, C, H, W, labels):
    """-> counts (N,3,C) int32: |label == c and pred == c|, |label == c|, |pred == c| per image (dl3p_class_counts)"""
    N, h, w, _ = z.shape
    zp, ldz = _pl(z)
    counts = torch.zeros((N, 3, C), dtype=torch.int32, device=z.device)
    lib().nearest_class_counts(zp, ldz, _p(labels), _p(counts), N, h, w, C, H, W, _stream())
    return counts


# ---------------------------------------------------------------- hard-example mining (csrc/mining.hip)
def mining_workspace(device):
    """the select's workspace: zero once, every pixel_loss_map + topk_threshold pair leaves it zero again"""
    return torch.zeros(lib().mining_workspace() // 4, dtype=torch.int32, device=device)


def pixel_loss_map(z, C, H, W, labels, ignore_index=255, loss=('ce',), pixel_weights=None, nearest=False, out=None, workspace=None):
    """z (N,h,w,Cpad) logits, labels [N*H*W] -> (per-pixel loss map [N*H*W] as the weighted head defines it, before the mean; the
    workspace, now holding the first radix histogram of the map).  nearest: the head behind UpSampling2D (dl3p_nearest_head_train),
    else the bilinear one (dl3p_upsample_softmax_loss); loss as upsample_softmax_ce"""
    N, h, w, _ = z.shape
    zp, ldz = _pl(z)
    if out is None:
        out = torch.empty(N * H * W, dtype=torch.float32, device=z.device)
    if workspace is None:
        workspace = mining_workspace(z.device)
    kind = {'ce': 0, 'weighted': 1, 'focal': 2}[loss[0]]
    cw = loss[1] if kind == 1 else None
    gamma, alpha = (float(loss[1]), float(loss[2])) if kind == 2 else (0.0, 0.0)
    fn = lib().nearest_pixel_loss_map if nearest else lib().pixel_loss_map
    fn(zp, ldz, _p(labels), int(ignore_index or 0), kind, _p(cw), gamma, alpha, _p(pixel_weights), _p(out), _p(workspace), N, h, w,
       C, H, W, _stream())
    return out, workspace


def topk_threshold(loss_map, top_k_percent_pixels, hard_example_mining_step=0, step_counter=None, step_bias=0, workspace=None,
                   record=None):
    """exact k-th largest of loss_map [P] -> record, int32 [8] on the device: {k, threshold bits, kept, nonzero, scale bits, 0, 0, 0}.
    workspace: the one pixel_loss_map returned (its first histogram is used), or None for a map from elsewhere;
    step_counter: int64 [1] on the device (None: step 0)"""
    first_ready = workspace is not None
    if workspace is None:
        workspace = mining_workspace(loss_map.device)
    if record is None:
        record = torch.zeros(8, dtype=torch.int32, device=loss_map.device)
    lib().topk_threshold(_p(loss_map), loss_map.numel(), float(top_k_percent_pixels), int(hard_example_mining_step),
                         _p(step_counter), int(step_bias), int(first_ready), _p(workspace), _p(record), _stream())
    return record


def mining_weights(loss_map, record, base=None, out=None):
    """-> w [P] = (loss_map >= threshold) ? base * scale : 0 (base None: ones): the pixel weights of the head launch that follows"""
    if out is None:
        out = torch.empty_like(loss_map)
    lib().mining_weights(_p(loss_map), _p(base), _p(record), _p(out), loss_map.numel(), _stream())
    return out


# ---------------------------------------------------------------- region losses (csrc/region_loss.hip)
REGION_BASE_NONE = -1
REGION_RECORD_HEAD = 4          # {rho R, |S|, 0, 0} in front of T[Cpad], A[Cpad], B[Cpad]


def region_workspace(C, device):
    """room for the partial rows [3][Cpad] of region_sums (never needs clearing)"""
    return torch.empty(lib().region_workspace(int(C)) // 4, dtype=torch.float32, device=device)


def region_record(C, device):
    """the device record region_finalize fills: 4 + 3 Cpad words"""
    return torch.zeros(REGION_RECORD_HEAD + 3 * ((int(C) + 3) // 4 * 4), dtype=torch.float32, device=device)


def region_sums(z, C, H, W, labels, ignore_index=255, workspace=None):
    """z (N,h,w,Cpad) logits, labels [N*H*W] -> (workspace, rows): rows partial rows [3][Cpad] = float I_c, float P_c, int32 Y_c over
    the valid pixels of one workgroup each (I_c = sum p_ic [y_i == c], P_c = sum p_ic, Y_c = |y_i == c|)"""
    N, h, w, _ = z.shape
    zp, ldz = _pl(z)
    if workspace is None:
        workspace = region_workspace(C, z.device)
    rows = ctypes.c_int(0)
    lib().region_sums(zp, ldz, _p(labels), int(ignore_index or 0), _p(workspace), ctypes.byref(rows), N, h, w, C, H, W, _stream())
    return workspace, rows.value


def region_finalize(workspace, rows, C, alpha, beta, smooth=1.0, region_weight=1.0, record=None):
    """-> record, float32 [4 + 3 Cpad] on the device: {region_weight * R, |S| (int32 bits), 0, 0, T[Cpad], A[Cpad], B[Cpad]}"""
    if record is None:
        record = region_record(C, workspace.device)
    lib().region_finalize(_p(workspace), int(rows), C, float(alpha), float(beta), float(smooth), float(region_weight), _p(record),
                          _stream())
    return record


def region_head_grad(z, C, H, W, labels, record, ignore_index=255, base=None, base_weight=1.0, pixel_weights=None, want_grad=True,
                     out=None, ld_big=None):
    """the head of base_weight * base + region_weight * R -> (loss [1], dlogits (N,H,W,ld_big) or None); base: None | ('ce',) |
    ('weighted', weight tensor [C]) | ('focal', gamma, alpha); record: region_finalize's"""
    N, h, w, _ = z.shape
    dev = z.device
    zp, ldz = _pl(z)
    if ld_big is None:
        ld_big = out.shape[-1] if out is not None else (C + 3) // 4 * 4
    if want_grad and out is None:
        out = torch.empty((N, H, W, ld_big), dtype=torch.float32, device=dev)
    kind = REGION_BASE_NONE if base is None else {'ce': 0, 'weighted': 1, 'focal': 2}[base[0]]
    cw = base[1] if kind == 1 else None
    gamma, alpha = (float(base[1]), float(base[2])) if kind == 2 else (0.0, 0.0)
    partial = torch.zeros(MAX_STAT_ROWS, dtype=torch.float32, device=dev)
    rows = ctypes.c_int(0)
    lib().region_head_grad(zp, ldz, _p(labels), int(ignore_index or 0), 1.0 / float(N * H * W), kind, _p(cw), gamma, alpha,
                           _p(pixel_weights), float(base_weight), _p(record), _p(out) if want_grad else None, ld_big, _p(partial),
                           ctypes.byref(rows), N, h, w, C, H, W, _stream())
    total = torch.empty(1, dtype=torch.float32, device=dev)
    lib().reduce_rows(_p(partial), rows.value, 1, _p(total), 0, _stream())
    return total, (out if want_grad else None)


def region_loss(z, C, H, W, labels, alpha=0.5, beta=0.5, smooth=1.0, region_weight=1.0, ignore_index=255, base=None, base_weight=1.0,
                pixel_weights=None, want_grad=True, ld_big=None):
    """sums -> finalize -> head gradient in one call -> dict(loss [1] tensor: base_weight * base + region_weight * R; sums: (3, C)
    float64 on the host, the partial rows added up, [I, P, Y]; record: the device record; dlogits (N,H,W,ld_big) or None)"""
    ws, rows = region_sums(z, C, H, W, labels, ignore_index)
    record = region_finalize(ws, rows, C, alpha, beta, smooth, region_weight)
    loss, dlogits = region_head_grad(z, C, H, W, labels, record, ignore_index, base, base_weight, pixel_weights, want_grad,
                                     ld_big=ld_big)
    return dict(loss=loss, sums=region_partial_sums(ws, rows, C), record=record, dlogits=dlogits)


def region_partial_sums(workspace, rows, C):
    """the partial rows of region_sums added up in float64 on the host -> (3, C): I_c, P_c, Y_c (inspection; the device's own sum is
    region_finalize's)"""
    import numpy as np
    cp = (C + 3) // 4 * 4
    part = workspace[:rows * 3 * cp].cpu().numpy().reshape(rows, 3, cp)
    sums = part[:, :2].astype(np.float64).sum(axis=0)
    counts = np.ascontiguousarray(part[:, 2]).view(np.int32).astype(np.float64).sum(axis=0)
    return np.concatenate([sums, counts[None]], axis=0)[:, :C]


def region_record_fields(record, C):
    """the record on the host -> dict(loss, present, score [C], A [C], B [C])"""
    cp = (C + 3) // 4 * 4
    h = record.cpu().numpy()
    return dict(loss=float(h[0]), present=int(h[1:2].view('int32')[0]), score=h[4:4 + C].copy(), A=h[4 + cp:4 + cp + C].copy(),
                B=h[4 + 2 * cp:4 + 2 * cp + C].copy())


# ---- dense CRF post-processing (csrc/crf.hip) ----------------------------------------------------------------
CRF_LP = 32                 # columns of a class-vector row: the column count of v_mfma_f32_32x32x2_f32
CRF_MAX_CLASSES = 32
_crf_ws = {}                # (device index, N, H, W) -> the buffers of dense_crf, reused by the next call at that size


def crf_check_classes(num_classes):
    """ValueError where the CRF is asked for with more classes than a class-vector row holds"""
    if not 1 <= int(num_classes) <= CRF_MAX_CLASSES:
        raise ValueError('the dense CRF is built for at most %d classes (C <= %d: one MFMA tile of label columns); got %d'
                         % (CRF_MAX_CLASSES, CRF_MAX_CLASSES, int(num_classes)))
    return int(num_classes)


CRF_KEYS = ('iterations', 'gt_prob', 'sxy_gaussian', 'compat_gaussian', 'sxy_bilateral', 'srgb', 'compat_bilateral')


def crf_params(dense_crf, num_classes):
    """the `dense_crf` switch of the front ends (False, True or a dict of dense_crf's keyword arguments) -> None without the CRF,
    else the keyword arguments; ValueError for an unknown key or more classes than the CRF serves"""
    if not dense_crf:
        return None
    params = {} if dense_crf is True else dict(dense_crf)
    unknown = sorted(set(params) - set(CRF_KEYS))
    if unknown:
        raise ValueError('dense_crf takes the keys %s (got %s)' % (', '.join(CRF_KEYS), ', '.join(unknown)))
    crf_check_classes(num_classes)
    return params


def _crf_images(images_u8):
    if not (isinstance(images_u8, torch.Tensor) and images_u8.is_cuda and images_u8.dtype == torch.uint8 and images_u8.dim() == 4
            and images_u8.shape[3] == 3):
        raise Dl3pError('the dense CRF takes (N, H, W, 3) uint8 images on the HIP device')
    return images_u8.contiguous()


def _sxy(s):
    """pydensecrf's sxy: one number or an (sx, sy) pair"""
    return (float(s[0]), float(s[1])) if isinstance(s, (tuple, list)) else (float(s), float(s))


def crf_messages(images_u8, V, *, sxy_gaussian=(3, 3), sxy_bilateral=80, srgb=13, out=None):
    """the two raw message sums of the dense CRF, before normalisation and weighting: images (N,H,W,3) uint8, V (N,H,W,ld) or
    (N,H*W,ld) float32 rows (a channel-slice view of a wider buffer may be passed: the first 32 columns are read)
    -> (gaussian, bilateral), each (N, H*W, 32): out_i = sum over ALL pixels j of k(i, j) V_j, j == i included.
    out: a pair of (N, H*W, >= 32) buffers to write into"""
    img = _crf_images(images_u8)
    N, H, W, _ = img.shape
    n = H * W
    V = V.view(N, n, V.shape[-1])
    vp, ldv = _pl(V)
    if V.shape[-1] < CRF_LP:
        raise Dl3pError('crf_messages: V rows hold %d columns (got %d)' % (CRF_LP, V.shape[-1]))
    g, b = out if out is not None else (torch.empty((N, n, CRF_LP), dtype=torch.float32, device=img.device) for _ in range(2))
    gp, ldg = _pl(g)
    bp, ldb = _pl(b)
    tmp = torch.empty((N, n, CRF_LP), dtype=torch.float32, device=img.device)
    sx, sy = _sxy(sxy_gaussian)
    lib().crf_gauss_message(vp, ldv, None, _p(tmp), gp, ldg, N, H, W, sx, sy, _stream())
    lib().crf_bilateral_message(_p(img), vp, ldv, None, bp, ldb, None, N, H, W, float(sxy_bilateral), float(srgb), _stream())
    return g, b


def dense_crf(images_u8, masks_i32, num_classes, *, iterations=5, gt_prob=0.7, sxy_gaussian=(3, 3), compat_gaussian=3,
              sxy_bilateral=80, srgb=13, compat_bilateral=10, want_q=False):
    """fully connected CRF refinement of hard class masks (the reference's deeplabv3p/postprocess_np.py crf_postprocess with
    zero_unsure=False, every filter exact instead of pydensecrf's lattice): images (N,H,W,3) uint8 and masks (N,H,W) int32 on the
    device -> refined masks (N,H,W) int32, and Q (N,H,W,C) float32 with want_q.  A mask with a single class comes back unchanged.
    A class id outside [0, C) (an ignore label such as 255, say) is neither refused nor a class: it is not counted among the present
    classes and carries no evidence -- the pixel's unary term is that of "another class" for every present class -- while the pixel
    takes part in the messages like any other and leaves with a class in [0, C).  An image with fewer than two present classes comes
    back unchanged, such ids included.  iterations=0 returns the argmax of the unary term: a pixel's own class where
    gt_prob > 1 / n_labels, the lowest present id for an id outside [0, C).
    Runs on the current stream and does not synchronise; the buffers are kept per (device, N, H, W)"""
    C = crf_check_classes(num_classes)
    img = _crf_images(images_u8)
    N, H, W, _ = img.shape
    n = H * W
    if not (isinstance(masks_i32, torch.Tensor) and masks_i32.is_cuda and masks_i32.dtype == torch.int32
            and tuple(masks_i32.shape) == (N, H, W)):
        raise Dl3pError('dense_crf takes (N, H, W) int32 masks on the HIP device that match the images')
    if int(iterations) < 0:
        raise ValueError('iterations must not be negative (got %r)' % (iterations,))
    mask = masks_i32.contiguous()
    dev = img.device
    key = (dev.index, N, H, W)
    ws = _crf_ws.get(key)
    if ws is None:
        f32 = dict(dtype=torch.float32, device=dev)
        ws = _crf_ws[key] = {'census': torch.zeros((N, 2), dtype=torch.int32, device=dev),
                             'q': torch.empty((N, n, CRF_LP), **f32), 'fg': torch.empty((N, n, CRF_LP), **f32),
                             'fb': torch.empty((N, n, CRF_LP), **f32), 'tmp': torch.empty((N, n, CRF_LP), **f32),
                             'ng': torch.empty(n, **f32), 'nb': torch.empty((N, n), **f32)}
    L, st = lib(), _stream()
    q, fg, fb = ws['q'], ws['fg'], ws['fb']
    sx, sy = _sxy(sxy_gaussian)
    gt = float(gt_prob)
    out = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    L.crf_unary(_p(mask), _p(ws['census']), _p(q), CRF_LP, gt, N, n, C, st)
    if int(iterations) == 0:
        L.crf_update(_p(mask), _p(ws['census']), None, None, None, None, 0.0, 0.0, gt, None, CRF_LP, _p(out), N, n, C, st)
    else:
        L.crf_gauss_norm(_p(ws['ng']), H, W, sx, sy, st)
        L.crf_bilateral_message(_p(img), None, 0, None, None, 0, _p(ws['nb']), N, H, W, float(sxy_bilateral), float(srgb), st)
    for t in range(int(iterations)):
        last = t == int(iterations) - 1
        L.crf_gauss_message(_p(q), CRF_LP, _p(ws['ng']), _p(ws['tmp']), _p(fg), CRF_LP, N, H, W, sx, sy, st)
        L.crf_bilateral_message(_p(img), _p(q), CRF_LP, _p(ws['nb']), _p(fb), CRF_LP, None, N, H, W, float(sxy_bilateral),
                                float(srgb), st)
        L.crf_update(_p(mask), _p(ws['census']), _p(fg), _p(ws['ng']), _p(fb), _p(ws['nb']), float(compat_gaussian),
                     float(compat_bilateral), gt, _p(q) if (not last or want_q) else None, CRF_LP, _p(out) if last else None, N, n, C,
                     st)
    if want_q:
        return out, q.view(N, H, W, CRF_LP)[..., :C].clone()
    return out


def mask_confusion(pred_mask, labels, num_classes, confusion=None):
    """confusion[label, mask] += 1 over every pixel whose label is a class: pred_mask int32 and labels float32 of the same number of
    pixels, confusion (C, C) int64 on the device (made here when None) -> confusion"""
    if confusion is None:
        confusion = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=pred_mask.device)
    assert pred_mask.dtype == torch.int32 and labels.dtype == torch.float32 and pred_mask.numel() == labels.numel()
    lib().mask_confusion(_p(pred_mask.contiguous()), _p(labels.contiguous()), _p(confusion), pred_mask.numel(), int(num_classes),
                         _stream())
    return confusion


def denormalize_u8(x):
    """the reference's denormalize_image on the device: float32 in [-1, 1] -> uint8, (x * 127.5 + 127.5) truncated"""
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    lib().denormalize_u8(_p(x), _p(out), x.numel(), _stream())
    return out
