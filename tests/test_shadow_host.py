"""CPU twin of tests/test_shadow_gpu.py: no kernel runs here.  It proves what tests/_shadow_cases.py claims about its inputs — the
f32 chain of every family-(a) and (b) case, restated in the kernel's order, equals the float64 value; every (a) case holds at least
16 rounding ties per direction; every (b) output is a bf16 value; the restated chain of every (c) case stays inside the derived
bound — that torch's `.to(bfloat16)` is round-to-nearest-even on the special values and on random bit patterns, and that the
references reject every mutant of MUTANTS on every case that can show it (the `where` of each mutant says which those are)."""
import pytest
import torch

from tests import _shadow_cases as S

BF16, F32 = torch.bfloat16, torch.float32
CASES = S.merge_cases()
BY_FAMILY = {f: tuple(c for c in CASES if c.family == f) for f in "abc"}
ids = lambda cs: [c.name for c in cs]   # noqa: E731


def _accepts_f32(case, cand):
    """the check test_shadow_gpu.py applies to the f32 output: equality on (a) and (b), the derived bound on (c)"""
    op = S.operands(case)
    ref = S.effective64(op)
    if case.family in "ab":
        return torch.equal(cand.double(), ref)
    return bool(((cand.double() - ref).abs() <= S.merge_bound(op)).all())


def _accepts_images(got, want):
    return all(S.same_bf16(g, w) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ the rounding itself
def test_torch_rounding_is_nearest_even_on_the_special_values():
    v = S.special_values()
    want = S.rne_bits(v)
    got = S.bf16_bits(v.to(BF16))
    nan = torch.isnan(v)
    assert torch.equal(got[~nan], want[~nan]) and bool(torch.isnan(v.to(BF16).float())[nan].all())
    assert int(nan.sum()) == 4   # the signalling and the quiet NaN, both signs
    by = {int(b): int(g) for b, g in zip(S.f32_bits(v), got)}
    assert by[0x00000001] == 0 and by[0x00008000] == 0 and by[0x00008001] == 1 and by[0x00018000] == 2     # bf16 subnormals
    assert by[0x007f8000] == 0x0080 and by[0x007fffff] == 0x0080                                           # up into the normals
    assert by[0x3f807fff] == 0x3f80 and by[0x3f808000] == 0x3f80 and by[0x3f808001] == 0x3f81 and by[0x3f818000] == 0x3f82
    assert by[0x7f7f7fff] == 0x7f7f and by[0x7f7f8000] == 0x7f80 and by[0x7f7fffff] == 0x7f80              # the largest f32 -> inf
    assert by[0x80000000 | 0x7f7fffff] == 0xff80 and by[0x7f800000] == 0x7f80
    assert S.same_bf16(S.bf16_from_bits(want), v.to(BF16))


def test_torch_rounding_is_nearest_even_on_random_bits():
    gen = torch.Generator().manual_seed(0)
    v = torch.randint(-2 ** 31, 2 ** 31, (1 << 20,), generator=gen, dtype=torch.int64).to(torch.int32).view(F32)
    nan = torch.isnan(v)
    assert torch.equal(S.bf16_bits(v.to(BF16))[~nan], S.rne_bits(v)[~nan])
    assert bool(torch.isnan(v.to(BF16).float())[nan].all())


def test_special_matrix_holds_every_pattern():
    want = set(S.f32_bits(S.special_values()).tolist())
    for rows, cols in ((8, 20), (10, 17)):
        assert set(S.f32_bits(S.special_matrix(rows, cols)).view(-1).tolist()) == want


# ------------------------------------------------------------------------------------------------ the input families
@pytest.mark.parametrize("case", BY_FAMILY["a"], ids=ids(BY_FAMILY["a"]))
def test_dense_exact_cases_are_exact_and_hold_ties(case):
    op = S.operands(case)
    ref = S.effective64(op)
    f32 = S.restate_f32(op)
    assert torch.equal(f32.double(), ref), "the f32 chain in kernel order is not the float64 value"
    assert torch.equal(ref.float().double(), ref) and torch.equal(ref * 16, (ref * 16).round()) and float(ref.abs().max()) < 2 ** 14
    as64 = (op["scaling"] * op["A"].double()) * (1.0 if op["mask"] is None else op["mask"].double())
    prod = op["B"].double()[:, :, None] * as64[None]
    assert torch.equal(prod * 2, (prod * 2).round()) and float(prod.abs().max()) <= 160
    even, odd = S.tie_counts(f32)
    print(f"{case.name}: {even} ties with an even kept bit, {odd} with an odd one")
    assert even >= 16 and odd >= 16
    assert _accepts_f32(case, f32)


@pytest.mark.parametrize("case", BY_FAMILY["b"], ids=ids(BY_FAMILY["b"]))
def test_probe_cases_are_bf16_values(case):
    op = S.operands(case)
    ref = S.effective64(op)
    i = torch.arange(case.rows)
    hot = torch.zeros(case.rows, case.r, dtype=torch.bool)
    hot[i, i % case.r] = True
    assert bool((op["B"][hot] != 0).all()) and bool((op["B"][~hot] == 0).all())
    assert torch.equal(S.restate_f32(op).double(), ref)
    assert torch.equal(ref.float().to(BF16).double(), ref) and float(ref.abs().max()) <= 119
    assert _accepts_f32(case, S.restate_f32(op))


@pytest.mark.parametrize("case", BY_FAMILY["c"], ids=ids(BY_FAMILY["c"]))
def test_realistic_restatement_is_inside_the_derived_bound(case):
    op = S.operands(case)
    f32 = S.restate_f32(op)
    worst = ((f32.double() - S.effective64(op)).abs() / S.merge_bound(op)).max().item()
    print(f"{case.name}: worst |restatement - reference| / bound = {worst:.3f}")
    assert _accepts_f32(case, f32)


# ------------------------------------------------------------------------------------------------ mutants
def _merge_applies(mut, case):
    if mut in ("mask ignored", "mask shifted by one column"):
        return case.masked
    if mut == "B row taken without the tile's row offset":
        return case.rows > 64
    return True


MERGE_MUTANTS = tuple(m for m, (entry, _) in S.MUTANTS.items() if entry == "merge")


@pytest.mark.parametrize("mut", MERGE_MUTANTS)
def test_merge_mutants_are_rejected(mut):
    seen = {f: 0 for f in "abc"}
    for case in CASES:
        if not _merge_applies(mut, case):
            continue
        op = S.operands(case)
        assert not _accepts_f32(case, S.effective64(op, mut).float()), f"{mut}: accepted as the f32 output of {case.name}"
        if case.family in "ab":   # and in the bf16 images alone, which is all the refresh kernel writes
            rp, cp = case.pads
            got = S.images(S.effective64(op, mut).float(), rp, cp)
            assert not _accepts_images(got, S.images(S.effective64(op).float(), rp, cp)), f"{mut}: accepted in the images of {case.name}"
        seen[case.family] += 1
    assert all(seen.values()), f"{mut}: no case of some family shows it: {seen}"


def _image_applies(mut, case, fs):
    rp, cp = case.pads
    if mut in ("fwd_scale applied to dst_t", "dst_t built from the scaled image"):
        return fs != 1.0
    if mut == "padding left unwritten":
        return (rp, cp) != (case.rows, case.cols)
    if mut == "round-half-up instead of ties-to-even":
        return case.family == "a" and fs == 1.0
    if mut == "truncation instead of rounding":
        return case.family in "ac" and fs == 1.0
    return False   # NaN -> infinity: family (d) alone


IMAGE_MUTANTS = tuple(m for m, (entry, _) in S.MUTANTS.items() if entry == "images")


@pytest.mark.parametrize("mut", IMAGE_MUTANTS)
def test_image_mutants_are_rejected(mut):
    seen = 0
    for case in CASES:
        w32 = S.restate_f32(S.operands(case))
        rp, cp = case.pads
        for fs in (1.0, S.ALPHA):
            if _image_applies(mut, case, fs):
                assert not _accepts_images(S.images(w32, rp, cp, fs, mut), S.images(w32, rp, cp, fs)), f"{mut}: accepted on {case.name}, fs {fs}"
                seen += 1
    if mut in S.ROUND_MUTANTS:   # family (d), as every path of test_round_to_bf16_special_values compares it
        v = S.special_values()
        assert not S.same_bf16(S.round_bf16(v, mut), v.to(BF16)), f"{mut}: accepted on the special values"
        m = S.special_matrix(8, 20)
        assert not _accepts_images(S.images(m, 64, 64, 1.0, mut), S.images(m, 64, 64)), f"{mut}: accepted on the special matrix"
        seen += 1
    assert seen, f"{mut}: nothing shows it"


def test_images_reference_layout():
    """the reference itself, on a matrix small enough to state by hand"""
    w = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    img, img_t = S.images(w, 4, 4, fs=0.5)
    assert img.tolist() == [[0.5, 1.0, 1.5, 0], [2.0, 2.5, 3.0, 0], [0] * 4, [0] * 4]
    assert img_t.tolist() == [[1.0, 4.0, 0, 0], [2.0, 5.0, 0, 0], [3.0, 6.0, 0, 0], [0] * 4]
    buf = S.sentinel(1 + 4 * 6)
    S.view2d(buf, 1, 4, 4, 6).copy_(img)
    assert buf[0] == S.SENT and buf[1:].view(4, 6)[:, 4:].eq(S.SENT).all() and torch.equal(buf[1:].view(4, 6)[:, :4], img)


PACK_MUTANTS = tuple(m for m, (entry, _) in S.MUTANTS.items() if entry == "pack")


@pytest.mark.parametrize("mut", PACK_MUTANTS)
def test_pack_mutants_are_rejected(mut):
    seen = 0
    for sc in S.pack_scenarios():
        if mut == "pack: AmT pitch K instead of rpad" and sc.K == sc.rpad:
            continue
        want, got = S.ref_pack_scenario(sc), S.ref_pack_scenario(sc, mut)
        assert not all(torch.equal(g, w) for g, w in zip(got, want)), f"{mut}: accepted on {sc.name}"
        seen += 1
    assert seen


def test_pack_reference_layout():
    A = torch.tensor([[1.0, 2.0, 3.0]])
    B = torch.tensor([[1.0], [-1.0]])
    Am, AmT, Bb, BbT = (torch.full(s, S.SENT, dtype=BF16) for s in ((4, 3), (3, 4), (5, 4), (4, 5)))
    S.ref_pack(A, torch.tensor([1.0, 0.0, 0.5]), B, 2.0, Am, AmT, Bb, BbT, ro=2, no=1)
    s = S.SENT
    assert Am.tolist() == [[s] * 3, [s] * 3, [2.0, 0.0, 3.0], [s] * 3] and torch.equal(AmT, Am.t())
    assert Bb.tolist() == [[s] * 4, [s, s, 2.0, s], [s, s, -2.0, s], [s] * 4, [s] * 4] and torch.equal(BbT, Bb.t())


@pytest.mark.parametrize("mut", tuple(m for m, (entry, _) in S.MUTANTS.items() if entry == "mt_copy"))
def test_mt_copy_mutants_are_rejected(mut):
    rows = S.copy_rows()
    want, got = S.ref_mt_copy(rows), S.ref_mt_copy(rows, mut)
    for (src, n, scale), w, g in zip(rows, want, got):
        assert torch.equal(w[n:], S.sentinel(S.COPY_TAIL, F32))
        assert torch.equal(w, g) == (scale is None), f"{mut}: count {n}, scale {scale}"


def test_every_listed_mutant_has_a_test():
    entries = {entry for entry, _ in S.MUTANTS.values()}
    assert entries == {"merge", "images", "pack", "mt_copy"} and len(S.MUTANTS) == 20
    assert set(S.ROUND_MUTANTS) <= set(IMAGE_MUTANTS)


def test_refresh_reference_is_the_per_adapter_references():
    """ref_refresh places images and pack blocks exactly where the per-entry references do, and leaves the rest alone"""
    op = S.family_operands("a", 64, 128, 3, True)
    w32 = S.effective64(op).float()
    bufs = {k: S.sentinel(n) for k, n in (("d", 64 * 192), ("t", 128 * 64 + 2), ("Am", 8 * 128), ("AmT", 128 * 8), ("Bb", 64 * 8), ("BbT", 8 * 64))}
    e = {"w32": w32, "fs": S.ALPHA, "dst": ("d", 64, 192), "dst_t": ("t", 2, 64),
         "pack": {"A": op["A"], "mask": op["mask"], "B": op["B"], "scaling": 2.0, "Am": "Am", "AmT": "AmT", "Bb": "Bb", "BbT": "BbT",
                  "rpad": 8, "npad": 64, "ro": 4, "no": 0}}
    S.ref_refresh([e], bufs)
    img, img_t = S.images(w32, 64, 128, S.ALPHA)
    d = bufs["d"].view(64, 192)
    assert torch.equal(d[:, 64:], img) and bool(d[:, :64].eq(S.SENT).all())
    assert torch.equal(bufs["t"][2:].view(128, 64), img_t) and bool(bufs["t"][:2].eq(S.SENT).all())
    Am = bufs["Am"].view(8, 128)
    assert torch.equal(Am[4:7], ((2.0 * op["A"]) * op["mask"]).to(BF16)) and bool(Am[:4].eq(S.SENT).all()) and bool(Am[7:].eq(S.SENT).all())
    assert torch.equal(bufs["BbT"].view(8, 64)[4:7], (2.0 * op["B"]).to(BF16).t())
