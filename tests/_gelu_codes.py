"""Shared arithmetic of the one-byte gelu' tests (test_gelu_aux8_gpu.py, test_headline_sizes_gpu.py): the exact derivative, the byte
offset of an element in gemm_nt4w_kernel's fragment-ordered code buffer (include/wft.h, WFT_EPI_GELU_GRAD8) and the decoding
code -> (code - 26) / 200."""
import torch


def _dgelu(x):
    x = x.double()
    return 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-x * x / 2) / (2 * torch.pi) ** 0.5


def _code_index(M, N, rows=None, device="cuda:0"):
    """byte offset of element (m, n) in the fragment-ordered buffer (wft.h / gemm_nt4w.hip): int64 [M, N], or with rows = (r0, r1)
    the rows r0 <= m < r1 of that grid only ([r1 - r0, N]: the full grid of a headline-size product is 5.9 GB of int64)"""
    r0, r1 = (0, M) if rows is None else rows
    assert 0 <= r0 <= r1 <= M
    m = torch.arange(r0, r1, device=device).view(-1, 1)
    n = torch.arange(N, device=device).view(1, -1)
    tiles_n = N // 256
    tm, r = m // 256, m % 256
    tn, c = n // 256, n % 256
    wave = (r // 128) * 2 + c // 128
    fx, mr = (r % 128) // 16, r % 16
    cc = c % 128
    u, q, e = cc // 32, (cc % 32) // 8, cc % 8
    up, hh = u // 2, u % 2
    lane = q * 16 + mr
    return ((tm * tiles_n + tn) * 4 + wave) * 16384 + (up * 8 + fx) * 1024 + lane * 16 + hh * 8 + e


def _decode(codes, M, N, rows=None):
    return (codes[_code_index(M, N, rows, codes.device)].float() - 26.0) / 200.0
