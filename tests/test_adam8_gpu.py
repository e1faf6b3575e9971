"""wft_mt_adamw8 (csrc/optim.hip, block-wise 8-bit AdamW) under the per-element checks of tests/_adam8_cases.py, whose docstring has
the stages, the float64 reference, the bound forms and how their constants were measured; tests/test_adam8_host.py proves on the CPU
that the same checker rejects every listed mutant of the kernel's arithmetic.  The kernel is called through K.mt_adamw8 on views
carved from guarded buffers of the test's own (p, g, state1, state2, absmax1, absmax2: at least 64 sentinels on every side, the byte
0xA5 in the code arrays), a good part of them off the 16-byte (p, g) or 8-byte (codes) boundary the vector path needs.  Stage 1 (the
encoder), 2 (the decoder) and 3 (the whole update on dyadic maps) hold codes and absmax to torch.equal; stage 4 holds absmax and p to
K F per element and every code to the float64 code unless a midpoint lies within K F_x.  tests/test_adam8bit.py keeps the multi-step
trajectory against the oracle.

Every test prints the worst |err| / bound for absmax (n1, n2) and p, the share of elements near a midpoint (near1, near2) and the
number of codes that differ from the float64 code (diff1, diff2).

Measured on an MI355X (the bound with the K = 4 in force): stages 1 to 3 hold every exact assertion, p at most 0.184 of its bound.
Stage 4, worst over the cases of a table: table A absmax1 0.117, absmax2 0.107, p 0.249, at most 4.9e-5 of the elements near a
midpoint, at most 1 code of 345 100 off the float64 code (state2; state1 none); table B absmax1 0.150, absmax2 0.169, p 0.241, no
element near a midpoint, no code off.  No output reaches its bound: the kernel needed no fix.  The ratios land where the CPU
restatement does (p 0.249 x 4 = 0.995 F, restated 0.995 F).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _adam8_cases as A  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402

DEV = "cuda:0"


def _launch(case):
    """-> the buffers after one launch (CPU), with q1, q2 and sumsq as the kernel left them, and what those were"""
    lay = case.lay
    buf = {a: b.to(DEV) for a, b in case.buffers().items()}
    assert all(b.data_ptr() % 16 == 0 for b in buf.values())
    v = {a: [buf[a][s:s + n] for s, n in zip(lay[a].starts, lay[a].numels)] for a in A.ARRAYS}
    for a in ("p", "g", "s1", "s2"):   # the layouts' misalignment is the pointers' misalignment
        size, bound = (4, 16) if a in "pg" else (1, 8)
        assert [x.data_ptr() % bound for x in v[a]] == [m * size for m in lay[a].mis], a
    q1, q2 = (q.to(DEV) for q in case.maps)
    ss = None if case.clip is None else torch.tensor([case.clip[0]], dtype=torch.float32, device=DEV)
    const = {"q1": q1.clone(), "q2": q2.clone()}
    if ss is not None:
        const["sumsq"] = ss.clone()
    table = K.TensorTable(v["p"])
    assert table.total_chunks == A.chunk_starts(case.numels)[-1]
    K.mt_adamw8(table, v["p"], v["g"], v["s1"], v["s2"], v["a1"], v["a2"], q1, q2, *case.scalars, ss, case.clip[1] if case.clip else 0.0)
    torch.cuda.synchronize()
    out = {a: b.cpu() for a, b in buf.items()}
    out.update(q1=q1.cpu(), q2=q2.cpu())
    if ss is not None:
        out["sumsq"] = ss.cpu()
    return out, const


def _run(case):
    out, const = _launch(case)
    st = A.check_adam8(case, out, inputs=const)
    print(f"{case.name}: " + ", ".join(f"{k} {v:.3g}" for k, v in st.items()))
    return out, st


def test_stage_1_the_encoder_on_every_entry_midpoint_and_neighbour():
    """b1 = b2 = 0, g = 1 planted in every block: all 256 entries of qmap1, its 255 midpoints (the lower code) and their float32
    neighbours; the reachable fl32(g g) on either side of, and on, every midpoint of qmap2; alone, as the second block of a chunk, as
    a last partial block and through the unaligned path.  Codes and absmax by torch.equal"""
    out, st = _run(A.stage1_case())
    assert st["diff1"] == st["diff2"] == 0
    again, _ = _launch(A.stage1_case())
    assert all(torch.equal(out[a].view(torch.uint8), again[a].view(torch.uint8)) for a in A.ARRAYS), "a second launch from the same state differs"


def test_stage_2_the_decoder_on_all_codes_of_both_maps():
    """g = 0, b1 = b2 = 1: every block holds all 256 codes under an absmax in {2^-20, 1, 2^10} that differs between the states, between
    neighbouring blocks and between block b and b + 32 (the chunk offset); a block whose extreme is negative writes fl(|q1[0]| a1); an
    all-zero block between two others writes absmax 0 and the codes of 0.  Codes and absmax come back bit for bit"""
    _run(A.stage2_case())


@pytest.mark.parametrize("table", "AB")
def test_stage_3_the_whole_update_in_exact_arithmetic(table):
    """dyadic maps, b1 = 0.5, b2 = 0.75, power-of-two absmax, g a small integer times a power of two: every product and sum is exact,
    a quarter of the values of state1 sit on a midpoint, every lane holds the code of a ramp.  Codes and absmax against integer
    arithmetic by torch.equal"""
    case = A.stage3_case(table)
    out, st = _run(case)
    got = {a: case.lay[a].gather(out[a]) for a in ("s1", "s2", "a1", "a2")}
    assert all(torch.equal(got[a], case.want[a]) for a in got)


@pytest.mark.parametrize("k", range(len(A.STAGE4)), ids=[A.stage4_case(k).name[9:] for k in range(len(A.STAGE4))])
def test_stage_4_general_values_within_the_element_bounds(k):
    """one step from a random state (and the first step from all-zero codes with absmax 0), the real maps: absmax within K F_n, p
    within K F_p, every code the float64 code unless a midpoint lies within K F_x of the normalised value (at most 1e-3 of the elements)"""
    _run(A.stage4_case(k))
