"""wft_embed_fwd / wft_embed_bwd (csrc/embed.hip) and wft_embed_fwd_f32 / wft_embed_bwd_f32 (csrc/f32.hip), bit for bit.

The backward kernels exist for run-to-run determinism: every embedding row is summed over the positions that hold its id in
position order, without atomics, so the reference is that sum — a float32 loop over the positions on the CPU, not sum() or
index_add_ (their order is not the kernel's) — and the comparison is torch.equal.  The token lists make the bf16 kernel's
chunk loop (256 positions per chunk, 16 vocabulary rows per workgroup) meet what it can get wrong: B * S of 51 (one partial
chunk), 256 (one full chunk) and 600 (three chunks, the last partial); the same four ids at the start of every clip; an id
repeated inside one chunk; an id in every chunk; ids 15 | 16 and 31 on the 16-row ownership boundaries, 992 and 1002 in the last
workgroup of V = 1003 (not a multiple of 16: rows 1003..1007 of that workgroup do not exist); d = 64 (192 idle threads per row)
and d = 384; non-zero demb / dpos to accumulate into.  Out-of-range ids (-100 and V) go to the bf16 kernels only: the forward
clamps them, the backward skips them in demb and still counts them in dpos.  The fp32 kernels index with the id as it is (wft.h),
so they get the same lists without those two.
"""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402
from whisper_finetune.engine import ops32  # noqa: E402

DEV = "cuda:0"
V, N_CTX = 1003, 448
SHAPES = [(3, 17), (4, 64), (3, 200)]   # B * S = 51, 256, 600
DIMS = [64, 384]
CLIP_START = (1001, 1000, 7, 500)
EDGE_IDS = (15, 16, 31, 992, 1002)


def _p(t):
    return C.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def _inputs(B, S, d):
    g = torch.Generator().manual_seed(B * S + d)
    n = B * S
    tok = torch.randint(0, V, (n,), generator=g)
    tok.view(B, S)[:, :4] = torch.tensor(CLIP_START)
    free = [j for j in range(n) if j % S >= 4]
    tok[free[1:11:2]] = torch.tensor(EDGE_IDS)
    tok[free[2:12:2]] = torch.tensor(EDGE_IDS[::-1])          # every edge id twice
    tok[[free[12], free[14], free[16]]] = 77    # one id three times inside the first chunk
    for j in (free[13], n // 2 + 5, n - 2):                      # one id in every chunk there is (B * S = 600: chunks 0, 1, 2)
        tok[j] = 123
    assert n // 2 + 5 in free and n - 2 in free and n - 3 in free
    oob = tok.clone()
    oob[free[15]], oob[n - 3] = -100, V
    emb, pos = torch.randn(V, d, generator=g), torch.randn(N_CTX, d, generator=g)
    dout = torch.randn(n, d, generator=g).to(torch.bfloat16)
    demb0, dpos0 = torch.randn(V, d, generator=g), torch.randn(N_CTX, d, generator=g)
    return tok.view(B, S), oob.view(B, S), emb, pos, dout.view(B, S, d), demb0, dpos0


def _bwd_reference(tok, dout, demb0, dpos0):
    """float32, position order: demb[tok[j]] += dout[j] for j = 0, 1, ... (ids outside [0, V) skipped); dpos[s] += the sum over
    the clips b = 0, 1, ... of dout[b, s], that sum started from zero."""
    B, S = tok.shape
    demb, dpos = demb0.clone(), dpos0.clone()
    flat, dflat = tok.reshape(-1).tolist(), dout.float().reshape(B * S, -1)
    for j, t in enumerate(flat):
        if 0 <= t < V:
            demb[t] = demb[t] + dflat[j]
    s = torch.zeros(S, dout.shape[-1])
    for b in range(B):
        s = s + dout[b].float()
    dpos[:S] = dpos[:S] + s
    return demb, dpos


def test_the_token_lists_hold_what_the_docstring_says():
    for B, S in SHAPES:
        tok, oob, *_ = _inputs(B, S, 64)
        flat = tok.reshape(-1)
        assert (tok[:, :4] == torch.tensor(CLIP_START)).all() and all((flat == e).sum() >= 2 for e in EDGE_IDS)
        assert ((flat[:256] == 77).sum() >= 3) and {int(j) // 256 for j in (flat == 123).nonzero()} == set(range((B * S + 255) // 256))
        assert (oob == -100).sum() == 1 and (oob == V).sum() == 1 and ((oob != tok).sum() == 2)
        assert flat.min() >= 0 and flat.max() < V


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("B,S", SHAPES)
def test_bf16_embedding_bit_for_bit(B, S, d):
    tok, oob, emb, pos, dout, demb0, dpos0 = _inputs(B, S, d)
    for t in (tok, oob):
        td, doutd = t.to(DEV), dout.to(DEV)
        out = K.embed_fwd(td, emb.to(DEV), pos.to(DEV))
        assert torch.equal(out.cpu(), (emb[t.clamp(0, V - 1)] + pos[:S]).to(torch.bfloat16)), "forward"
        want_demb, want_dpos = _bwd_reference(t, dout, demb0, dpos0)
        runs = []
        for _ in range(2):
            demb, dpos = demb0.to(DEV), dpos0.to(DEV)
            K.embed_bwd(td, doutd, demb, dpos)
            runs.append((demb.cpu(), dpos.cpu()))
        assert torch.equal(runs[0][0], want_demb), "demb"
        assert torch.equal(runs[0][1], want_dpos), "dpos"
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "a second run gives other bits"
    # the two out-of-range positions: skipped in demb, counted in dpos
    demb_in, _ = _bwd_reference(tok, dout, demb0, dpos0)
    hit = (tok != oob).reshape(-1).nonzero().reshape(-1).tolist()
    assert len(hit) == 2 and not torch.equal(demb_in, want_demb)
    assert torch.equal(_bwd_reference(oob, dout, demb0, dpos0)[1], _bwd_reference(tok, dout, demb0, dpos0)[1])


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("B,S", SHAPES)
def test_f32_embedding_bit_for_bit(B, S, d):
    tok, _, emb, pos, dout, _, _ = _inputs(B, S, d)
    h = L.load()
    g = torch.Generator().manual_seed(1)
    dout = dout.float() + torch.randn(B, S, d, generator=g) * 2.0 ** -10   # not bf16-representable
    td, doutd, embd, posd = tok.to(DEV), dout.to(DEV), emb.to(DEV), pos.to(DEV)
    out = torch.empty(B, S, d, device=DEV)
    L.check(h.wft_embed_fwd_f32(_p(td), _p(embd), _p(posd), _p(out), B, S, d, L.stream_ptr()), "wft_embed_fwd_f32")
    assert torch.equal(out.cpu(), emb[tok] + pos[:S]), "forward"
    want_demb, want_dpos = _bwd_reference(tok, dout, torch.zeros(V, d), torch.zeros(N_CTX, d))
    runs = []
    for _ in range(2):
        demb, dpos = torch.zeros(V, d, device=DEV), torch.zeros(N_CTX, d, device=DEV)   # zero-filled: the kernel's contract
        L.check(h.wft_embed_bwd_f32(_p(td), _p(doutd), _p(demb), _p(dpos), B, S, d, L.stream_ptr()), "wft_embed_bwd_f32")
        runs.append((demb.cpu(), dpos.cpu()))
    assert torch.equal(runs[0][0], want_demb), "demb"
    assert torch.equal(runs[0][1], want_dpos), "dpos"
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "a second run gives other bits"


def test_f32_embed_fn_takes_a_strided_tokens_view():
    B, S, d = 3, 17, 64
    tok, _, emb, pos, dout, _, _ = _inputs(B, S, d)
    tv = torch.stack([tok, torch.ones_like(tok)], 2).to(DEV)[:, :, 0]   # stride 2: every other element is not a token
    assert not tv.is_contiguous()
    embd, posd = emb.to(DEV).requires_grad_(True), pos.to(DEV).requires_grad_(True)
    out = ops32.EmbedFn.apply(tv, embd, posd)
    assert torch.equal(out.detach().cpu(), emb[tok] + pos[:S])
    out.backward(dout.float().to(DEV))
    want_demb, want_dpos = _bwd_reference(tok, dout, torch.zeros(V, d), torch.zeros(N_CTX, d))
    assert torch.equal(embd.grad.cpu(), want_demb) and torch.equal(posd.grad.cpu(), want_dpos)
