"""Every single-token attention kernel of csrc/decode_attn.hip, at every split regime, on the probe operands of tests/_decode_probe.py:
each (row, head) puts its softmax mass in equal halves on two keys at the edges of the kernels' dealing and is aligned just as
strongly with decoys where a wrong kernel would read (the row behind the n keys, the stale cache row at len - 1, the row's own slot
under an ancestry table), so one lost, leaked or double-counted key moves that (row, head) by O(1) of its own size.  Outputs are
compared with the fp64 oracle per (row, head) at 2^-7 of the head's own largest value (close_per_head);
tests/test_decode_probe_host.py shows on the CPU that this bound passes correct fp32 -> bf16 attention and fails every mutant.

The cases (tests/_decode_probe.py SPECS; each with q_prescaled False and True, case 7 False only):
  1  attn_decode self   H = 6, cap 448, lengths 1 .. 448 around every block of 32, each repeated for edge coverage      1 split
  2  attn_decode self   H = 20, cap 448, lengths 129, 417, 448                                                          1
  3  attn_decode self   H = 2, cap 1100, calls of <= 42 rows, lengths 1 .. 1100 (rows inside split 0: empty partials)   3
  4  attn_decode self   H = 20, B = 7, cap 1100, lengths 129, 600, 1100                                                 2
  5  attn_decode cross  H = 6, B = 4, Tk = 1, 31, 32, 33, 500 (the cache bits unchanged)                                1
  6  attn_decode cross  (H = 6, B = 8), (H = 20, B = 7), Tk = 1500                                                      3, 2
  7  attn_decode cross  H = 2, B = 1, Tk = 7700, reduced edges                                                          16
  8  attn_decode_beam cross  H = 2, one audio, group 8, Tk = 7700, reduced edges, four calls                            16
  9  attn_decode_beam cross  two audios, H = 6, every group 1 .. 8, Tk = 500 and 1500                                   1, 3
  10 attn_decode_beam self   R = 10, H = 6, cap 448 at lengths 417 and 448; R = 4, H = 2, cap 1100 at length 1100       1, 3
The split of every call is asserted through the workspace-bytes query (R * H * nsplit * 66 * 4, or 0), so a later change of the
split rule cannot quietly move a case out of its regime.

Measured on an MI355X when this file was added: every case passes, worst (row, head) ratio 3.859e-3 (cases 1 and 5), the same as
the CPU emulation's — one bf16 rounding of the output.  No kernel fault was found.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _decode_probe as P  # noqa: E402
from tests.test_decode_kernels_gpu import PER_HEAD_TOL, close_per_head  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = "cuda:0"


def bits(t):
    return t.detach().cpu().view(torch.int16)


def _run(c, lens=None):
    """One call of the entry point the form belongs to -> (o, the whole cache buffer afterwards, the workspace bytes asked for)"""
    D = c.D
    qkv, buf = c.qkv.to(DEV), c.buf.to(DEV)
    cache = buf[:, :c.cap]
    kw = dict(q_prescaled=c.prescaled)
    if c.self_form:
        lens = c.lens if lens is None else lens
        kw.update(new_kv=(qkv[:, D:2 * D], qkv[:, 2 * D:]), lens=torch.tensor(lens, dtype=torch.int32, device=DEV))
    if c.form in ("self", "cross"):
        fn, query = K.attn_decode, L.load().wft_attn_decode_workspace_bytes
    else:
        fn, query = K.attn_decode_beam, L.load().wft_attn_decode_beam_workspace_bytes
        kw.update(group=c.group)
        if c.form == "beam_self":
            kw.update(anc=c.anc.to(DEV))
    args, _ = fn(qkv[:, :D], cache, c.H, P.SCALE, _args_only=True, **kw)
    ws = query(args)
    o = fn(qkv[:, :D], cache, c.H, P.SCALE, **kw)
    torch.cuda.synchronize()
    return o, buf, ws


@pytest.mark.parametrize("case", P.CASES, ids=P.IDS)
def test_decode_attention_on_probe_operands(case):
    case_id, pre = case
    spec = P.SPEC[case_id]
    worst = 0.0
    for i, c in enumerate(P.calls(case_id, pre)):
        ref = P.oracle(c)
        o, buf, ws = _run(c)
        assert c.nsplit == spec["nsplit"] and ws == c.workspace_bytes(), f"{case_id} call {i}: not the {spec['nsplit']}-split regime ({ws} bytes)"
        if case_id.startswith("3-"):
            assert ws > 0
        ratio = close_per_head(o, ref, PER_HEAD_TOL, f"{case_id} pre={pre} call {i} ({c.R} rows, {c.nsplit} split(s))")
        worst = max(worst, ratio.max().item())
        # the self forms append at len - 1 of the row's own slot; no other byte changes, guard rows and decoys included
        assert torch.equal(bits(buf), bits(c.cache_after())), f"{case_id} call {i}: the cache"
    print(f"{case_id} pre={pre}: worst (row, head) ratio {worst:.3e}")


def test_len_is_clamped_to_1_and_tk():
    """The documented "len clamped to 1..Tk": H = 2, cap 64 with 8 guard rows.  Row 1 is given len = 0 and must behave as length 1,
    writing row 0; row 2 is given len = cap + 5 and must behave as length cap; row 0 (len 33) is ordinary.  The probe operands are
    built for the clamped lengths, so a missing clamp meets the decoy behind the row or writes outside row len - 1; every byte
    outside the three written rows is unchanged.  Row 1 is not the first and the guard rows outnumber the overshoot, so even a
    missing clamp would stay inside the allocation."""
    for pre in (False, True):
        c = P.clamp_case(pre)
        assert (c.H, c.cap, c.lens) == (2, 64, [33, 1, 64]) and P.CLAMP_LENS[1] == [33, 0, 69]
        o, buf, ws = _run(c, lens=P.CLAMP_LENS[1])
        assert ws == 0
        ratio = close_per_head(o, P.oracle(c), PER_HEAD_TOL, f"len clamped, pre={pre}")
        assert torch.equal(bits(buf), bits(c.cache_after()))
        print(f"clamp pre={pre}: worst (row, head) ratio {ratio.max().item():.3e}")
