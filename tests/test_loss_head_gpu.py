"""The loss-head kernels under the per-element bounds of tests/_loss_head_cases.py (whose docstring has the cases, the float64
reference, the bound forms and how their constants were measured; tests/test_loss_head_host.py proves on the CPU that the same
checker rejects every listed mutant of the kernels' arithmetic): wft_ce_fwd, wft_ce_bwd (in place and out of place: same bits)
and wft_token_stats on bf16 logits, wft_ce_fwd_f32 / wft_ce_bwd_f32 through the C ABI with ld > V on fp32 and on bf16-valued
logits, and once more through ops32.CrossEntropyFn on a [rows, V] view of the padded buffer with a strided targets view.
Each test prints the worst |err| / bound it saw per output; above 1 it fails."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _loss_head_cases as H  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402
from whisper_finetune.engine import ops32  # noqa: E402

DEV = "cuda:0"
CASES = H.cases()
IDS = [c.name for c in CASES]


def _p(t):
    return C.c_void_p(t.data_ptr())


def _show(what, c, r):
    print(f"{what} {c.name}: worst |err| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))


def _bf16_outputs(c):
    x = c.x.to(torch.bfloat16).to(DEV)
    tg = c.targets.to(DEV)
    row_loss, row_lse, stats, am = K.ce_fwd(x, tg, c.V, c.eps, want_argmax=True)
    gs = torch.tensor([c.gscale], device=DEV)
    dl = K.ce_bwd(x, tg, c.V, c.eps, row_lse, stats, gs, inplace=False)
    assert dl.data_ptr() != x.data_ptr() and torch.equal(x.cpu().float(), c.x), "the out-of-place backward wrote to the logits"
    ts, tam = K.token_stats(x, tg, c.V)
    ts0, tam0 = K.token_stats(x, None, c.V)   # targets NULL: column 3 is 0, the rest the same bits
    assert torch.equal(ts0[:, :3], ts[:, :3]) and torch.equal(tam0, tam) and (ts0[:, 3] == 0).all()
    x2 = x.clone()
    dl2 = K.ce_bwd(x2, tg, c.V, c.eps, row_lse, stats, gs, inplace=True)
    assert dl2.data_ptr() == x2.data_ptr()
    assert torch.equal(dl2.view(torch.int16), dl.view(torch.int16)), "in-place and out-of-place wft_ce_bwd differ"
    return {"row_loss": row_loss, "row_lse": row_lse, "stats": stats, "argmax": am, "dlogits": dl.float(), "tstats": ts, "targmax": tam}


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_ce_fwd_bwd_and_token_stats_within_the_element_bounds(i):
    c = CASES[i]
    _show("bf16 mode", c, H.check(c, _bf16_outputs(c), what="bf16 mode"))


def test_all_ignored_batch():
    c = H.all_ignored_case()
    out = _bf16_outputs(c)
    H.check(c, out, what="bf16 mode")
    assert out["stats"].tolist() == [0.0, 0.0] and (out["dlogits"] == 0).all() and (out["row_loss"] == 0).all()


def _f32_abi(c, x):
    h = L.load()
    x = x.to(DEV)
    tg = c.targets.to(DEV)
    row_loss, row_lse = torch.empty(c.rows, device=DEV), torch.empty(c.rows, device=DEV)
    stats = torch.empty(2, device=DEV)
    L.check(h.wft_ce_fwd_f32(_p(x), c.ld, _p(tg), c.rows, c.V, c.eps, _p(row_loss), _p(row_lse), _p(stats), L.stream_ptr()), "wft_ce_fwd_f32")
    gs = torch.tensor([c.gscale], device=DEV)
    L.check(h.wft_ce_bwd_f32(_p(x), c.ld, _p(tg), c.rows, c.V, c.eps, _p(row_lse), _p(stats), _p(gs), L.stream_ptr()), "wft_ce_bwd_f32")
    return {"row_loss": row_loss, "row_lse": row_lse, "stats": stats, "dlogits": x}


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_f32_twins_through_the_abi_with_padded_rows(i):
    c = CASES[i]
    _show("fp32 mode, fp32 values", c, H.check(c, _f32_abi(c, c.x32), fp32_mode=True, fp32_values=True, what="fp32 mode, fp32 values"))
    _show("fp32 mode, bf16 values", c, H.check(c, _f32_abi(c, c.x), fp32_mode=True, what="fp32 mode, bf16 values"))


@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if c.rows == 50 or c.V == 51866], ids=lambda i: IDS[i])
def test_f32_cross_entropy_fn_on_a_padded_view_with_strided_targets(i):
    c = CASES[i]
    ref = H.case_reference(c, True)
    buf = c.x32.to(DEV).requires_grad_(True)
    tg = torch.stack([c.targets, torch.ones_like(c.targets)], 1).to(DEV)[:, 0]   # stride 2: every other element is not a target
    assert not tg.is_contiguous()
    loss = ops32.CrossEntropyFn.apply(buf[:, :c.V], tg, c.eps)
    (loss * c.gscale).backward()
    want = ref["stats0"] / ref["n_valid"]
    r = {"loss": H.ratio(loss.detach(), want, (H.K["stats0"] * ref["F"]["stats0"] + H.U * ref["stats0"].abs()) / ref["n_valid"])}
    assert (buf.grad[:, c.V:] == 0).all()
    # the gradient autograd hands back, and the logits buffer the backward wrote it over (padding untouched)
    grad = torch.full_like(c.x32, H.POISON)
    grad[:, :c.V] = buf.grad[:, :c.V].cpu()
    r.update(H.check(c, {"dlogits": grad}, fp32_mode=True, fp32_values=True, what="CrossEntropyFn gradient"))
    assert torch.equal(buf.detach().cpu(), grad)
    _show("ops32.CrossEntropyFn", c, r)
    assert r["loss"] <= 1.0, r
