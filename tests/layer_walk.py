"""float64 restatements shared by the every-layer walks (tests/test_bf16_gpu.py, tests/test_peleenet_full_size_gpu.py,
tests/test_production_shapes_gpu.py): a layer recomputed on the device from the device's own input view."""
import torch

from conftest import load_pkg


def _act64(u, act):
    O_ = load_pkg('ops')
    if act == O_.ACT_NONE:
        return u
    if act == O_.ACT_RELU:
        return u.clamp_min(0)
    if act == O_.ACT_RELU6:
        return u.clamp(0, 6)
    hs = (u + 3).clamp(0, 6) / 6
    return hs if act == O_.ACT_HSIGMOID else u * hs


def _taps(a, k, stride, rate, pad_t, pad_l, Ho, Wo):
    """the k x k shifted, strided views of a zero-padded (N, H, W, C) tensor: [(ky, kx, view (N, Ho, Wo, C))]"""
    N, H, W, C = a.shape
    need_h, need_w = (Ho - 1) * stride + (k - 1) * rate + 1, (Wo - 1) * stride + (k - 1) * rate + 1
    ap = torch.nn.functional.pad(a, (0, 0, pad_l, max(0, need_w - W - pad_l), pad_t, max(0, need_h - H - pad_t)))
    for ky in range(k):
        for kx in range(k):
            yield ky, kx, ap[:, ky * rate: ky * rate + (Ho - 1) * stride + 1: stride, kx * rate: kx * rate + (Wo - 1) * stride + 1: stride, :]
