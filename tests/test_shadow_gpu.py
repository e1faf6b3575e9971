"""The weight-shadow kernels of csrc/shadow.hip against the references of tests/_shadow_cases.py (whose docstring has the input
families, the references and the mutants; tests/test_shadow_host.py proves on the CPU that the inputs are what they claim to be and
that the references reject every listed mutant): K.cast_bf16, K.weight_shadow, K.lora_merge, K.lora_pack, K.lora_refresh_mt on a
table written by hand from the text of wft.h, and K.mt_copy_f32.  Every output buffer is flat, filled with a sentinel before the
launch and compared whole and bitwise; the one bound is the derived one of family (c)'s f32 output, whose worst |err| / bound each
case prints before it asserts.

Measured on an MI355X: every bitwise comparison holds, the packed and the scalar bf16 conversion agree with each other and with
torch on every special value, and family (c)'s f32 output uses at most 0.39 of its bound (rank 1; 0.36 at rank 5, 0.19 at rank 16,
0.06 at rank 64): the kernels needed no fix.
"""
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _shadow_cases as S  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402
from whisper_finetune.engine import ops  # noqa: E402

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
ALPHA = ops.QK_ALPHA
CASES = S.merge_cases()
SCENARIOS = S.pack_scenarios()


def _dev(t):
    return None if t is None else t.to(DEV)


def _bitwise(got, want, what):
    """whole buffers, bit for bit (torch.equal on floats would take -0 for 0 and no NaN for itself)"""
    got, want = got.cpu().contiguous(), want.cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    v = torch.int16 if got.dtype == BF16 else torch.int32
    if not torch.equal(got.view(v), want.view(v)):
        bad = (got.view(v) != want.view(v)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ, first at {i}: got {got[i].item()!r}, want {want[i].item()!r}")


def _offset_copy(t, off=1):
    """a copy of the tensor whose first element sits `off` elements into its allocation: contiguous, misaligned by off elements"""
    flat = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    flat[off:].copy_(t.reshape(-1))
    v = flat[off:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() == flat.data_ptr() + off * t.element_size()
    return v


class Target:
    """one flat sentinel-filled device buffer with a [rows, cols] view at (off, ld) for a kernel to write, and its expectation"""

    def __init__(self, rows, cols, off=0, ld=None, tail=8, dtype=BF16):
        self.rows, self.cols, self.off, self.ld = rows, cols, off, cols if ld is None else ld
        self.n = off + (rows - 1) * self.ld + cols + tail
        self.dtype = dtype
        self.buf = S.sentinel(self.n, dtype, DEV)
        self.view = S.view2d(self.buf, off, rows, cols, self.ld)

    def expect(self, img, what):
        want = S.sentinel(self.n, self.dtype)
        S.view2d(want, self.off, self.rows, self.cols, self.ld).copy_(img)
        _bitwise(self.buf, want, what)

    def untouched(self, what):
        _bitwise(self.buf, S.sentinel(self.n, self.dtype), what)


def test_alpha_is_the_projects():
    assert S.ALPHA == ALPHA


# ------------------------------------------------------------------------------------------------ the rounding itself
def test_round_to_bf16_special_values():
    v = S.special_values()
    nv = v.numel()
    # K.cast_bf16: n = 7 (the tail alone), n = 8 (one vector, no tail), n = 8 * 4 + 5 (rotated, so every pattern meets both)
    for n, shifts in ((7, range(0, nv, 7)), (8, range(0, nv, 8)), (37, range(nv))):
        for s in shifts:
            src = torch.roll(v, -s).repeat(2)[:n].clone()
            got = K.cast_bf16(src.to(DEV))
            assert S.same_bf16(got, src.to(BF16)), f"cast_bf16 n = {n}, shift {s}: {S.bf16_bits(got.cpu()).tolist()} != {S.bf16_bits(src.to(BF16)).tolist()}"
    # K.weight_shadow: the 4-wide path, the element-wise path by its width and by a source at a 1-element storage offset
    results = {}
    for name, (rows, cols), off in (("fast", (8, 20), 0), ("cols % 4 != 0", (10, 17), 0), ("source offset", (8, 20), 1)):
        m = S.special_matrix(rows, cols)
        src = _offset_copy(m.to(DEV), off) if off else m.to(DEV)
        d, t = Target(64, 64), Target(64, 64)
        K.weight_shadow(src, 64, 64, True, out=d.view, out_t=t.view, fwd_scale=1.0)
        img, img_t = S.images(m, 64, 64)
        for tg, want, side in ((d, img, "dst"), (t, img_t, "dst_t")):
            got = tg.buf.cpu()
            assert S.same_bf16(got[:64 * 64].view(64, 64), want), f"weight_shadow {name}: {side} is not torch's rounding"
            assert bool(got[64 * 64:].eq(S.SENT).all())
        results[name] = (d.buf.cpu(), t.buf.cpu())
    for a, b in zip(results["fast"], results["source offset"]):   # the same matrix through both conversions
        assert S.same_bf16(a, b), "the packed and the scalar conversion disagree"


# ------------------------------------------------------------------------------------------------ wft_cast_pad_transpose_f32_bf16
def _cast_source(family, rows, cols):
    op = S.family_operands(family, rows, cols, 3, True)
    return S.restate_f32(op)   # family (a): exact, with ties; any f32 matrix has an exact expectation here


@pytest.mark.parametrize("family", "ac")
@pytest.mark.parametrize("layout", S.CAST_LAYOUTS, ids=[f"{r}x{c}-to-{rp}x{cp}" for (r, c), (rp, cp) in S.CAST_LAYOUTS])
def test_cast_pad_transpose_layouts(layout, family):
    (rows, cols), (rp, cp) = layout
    w = _cast_source(family, rows, cols)
    wd = w.to(DEV)
    wd_off = _offset_copy(wd)
    for fs in (1.0, ALPHA):
        img, img_t = S.images(w, rp, cp, fs)
        for want_t in (True, False):
            runs = {
                "plain": (wd, Target(rp, cp), Target(cp, rp)),
                "inside wider buffers": (wd, Target(rp, cp, off=2 * (cp + 64), ld=cp + 64, tail=3 * (cp + 64)),
                                         Target(cp, rp, off=rp, ld=3 * rp)),   # the middle third of [cols_pad, 3 * rows_pad]
                "source misaligned by 4 bytes": (wd_off, Target(rp, cp), Target(cp, rp)),
                "destinations misaligned by 2 bytes": (wd, Target(rp, cp, off=1), Target(cp, rp, off=1)),
            }
            for name, (src, d, t) in runs.items():
                what = f"{rows}x{cols} -> {rp}x{cp}, family ({family}), fs {fs}, want_t {want_t}, {name}"
                K.weight_shadow(src, rp, cp, want_t, out=d.view, out_t=t.view if want_t else None, fwd_scale=fs)
                d.expect(img, what + ": dst")
                if want_t:
                    t.expect(img_t, what + ": dst_t")
                else:
                    t.untouched(what + ": dst_t")


# ------------------------------------------------------------------------------------------------ wft_lora_merge
def _check_f32(case, op, got, what):
    """(a), (b): the float64 value exactly; (c): the derived bound of _shadow_cases.py"""
    ref = S.effective64(op)
    got = got.cpu()
    if case.family in "ab":
        _bitwise(got, ref.float(), what)
        return
    ratio = ((got.double() - ref).abs() / S.merge_bound(op)).max().item()
    print(f"{what}: worst |f32 - float64 reference| / ((r + 3) u (|W| + sum|s B A mask|)) = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: {ratio:.3f} of the derived bound"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_lora_merge_per_element(case):
    op = S.operands(case)
    rows, cols = case.rows, case.cols
    rp, cp = case.pads
    W, B, A, mask = _dev(op["W"]), _dev(op["B"]), _dev(op["A"]), _dev(op["mask"])
    s = op["scaling"]

    # the f32 output alone, then in place over a copy of W
    f = Target(rows, cols, dtype=F32)
    K.lora_merge(W, B, A, mask, s, out_f32=f.view)
    w32 = f.buf.cpu()[:rows * cols].view(rows, cols).clone()
    _check_f32(case, op, w32, f"{case.name}: out_f32 alone")
    f.expect(w32, f"{case.name}: out_f32 alone")
    Wc = W.clone()
    K.lora_merge(Wc, B, A, mask, s, out_f32=Wc)
    _bitwise(Wc, w32, f"{case.name}: out_f32 aliasing W")
    f = Target(rows, cols, dtype=F32)
    K.lora_merge(_offset_copy(W), B, A, mask, s, out_f32=f.view)
    f.expect(w32, f"{case.name}: W misaligned by 4 bytes")
    f = Target(rows, cols, off=1, dtype=F32)
    K.lora_merge(W, B, A, mask, s, out_f32=f.view)
    f.expect(w32, f"{case.name}: out_f32 misaligned by 4 bytes")

    for fs in (1.0, ALPHA):
        img, img_t = S.images(w32, rp, cp, fs)   # (a), (b): w32 is the float64 value; (c): the roundings of what the kernel wrote
        what = f"{case.name}, fs {fs}"
        d, t = Target(rp, cp), Target(cp, rp)
        K.lora_merge(W, B, A, mask, s, out=d.view, out_t=t.view, rows_pad=rp, cols_pad=cp, fwd_scale=fs)
        d.expect(img, what + ", bf16 only: dst")
        t.expect(img_t, what + ", bf16 only: dst_t")
        d, t, f = Target(rp, cp), Target(cp, rp), Target(rows, cols, dtype=F32)
        K.lora_merge(W, B, A, mask, s, out=d.view, out_t=t.view, rows_pad=rp, cols_pad=cp, out_f32=f.view, fwd_scale=fs)
        d.expect(img, what + ", all three: dst")
        t.expect(img_t, what + ", all three: dst_t")
        f.expect(w32, what + ", all three: dst_f32")
        d = Target(rp, cp, off=2 * (cp + 64), ld=cp + 64, tail=3 * (cp + 64))
        K.lora_merge(W, B, A, mask, s, out=d.view, rows_pad=rp, cols_pad=cp, fwd_scale=fs)
        d.expect(img, what + ", dst without dst_t, ld_dst = cols_pad + 64")
        d, t = Target(rp, cp, off=1), Target(cp, rp, off=1, ld=rp + 4)
        K.lora_merge(W, B, A, mask, s, out=d.view, out_t=t.view, rows_pad=rp, cols_pad=cp, fwd_scale=fs)
        d.expect(img, what + ", destinations misaligned by 2 bytes: dst")
        t.expect(img_t, what + ", destinations misaligned by 2 bytes: dst_t")


@pytest.mark.parametrize("rank", (0, 65))
def test_lora_merge_refuses_rank_0_and_65(rank):
    rows, cols = 64, 64
    W = torch.zeros(rows, cols, device=DEV)
    B, A = torch.ones(rows, max(rank, 1), device=DEV), torch.ones(max(rank, 1), cols, device=DEV)   # valid pointers at rank 0 too
    d, t, f = Target(rows, cols), Target(cols, rows), Target(rows, cols, dtype=F32)
    p = K._p
    with pytest.raises(L.WftError):
        L.check(L.load().wft_lora_merge(p(W), rows, cols, p(B), p(A), p(None), rank, 2.0, p(d.view), p(t.view), rows, cols, cols, rows,
                                        p(f.view), 1.0, L.stream_ptr()), "wft_lora_merge")
    if rank:
        with pytest.raises(L.WftError):
            K.lora_merge(W, B, A, None, 2.0, out=d.view, out_t=t.view, out_f32=f.view)
    torch.cuda.synchronize()
    for tg in (d, t, f):
        tg.untouched(f"rank {rank}")


# ------------------------------------------------------------------------------------------------ wft_lora_pack
@pytest.mark.parametrize("sc", SCENARIOS, ids=[s.name for s in SCENARIOS])
def test_lora_pack_blocks(sc):
    bufs = S.pack_buffers(sc, DEV)
    for (A, mask, B), (_, _, ro, no) in zip(S.pack_operands(sc), sc.adapters):
        K.lora_pack(_dev(A), _dev(mask), _dev(B), S.SCALING, *bufs, ro, no)
    for name, got, want in zip(("Am", "AmT", "Bb", "BbT"), bufs, S.ref_pack_scenario(sc)):
        _bitwise(got, want, f"{sc.name}: {name}")


# ------------------------------------------------------------------------------------------------ wft_lora_refresh_mt
def _f32_field(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _table_row(W, rows, cols, B, A, mask, rank, scaling, fs, dst, dst_t, ld_dst, ld_dst_t, pack):
    """one row of the table as wft.h lays it out: 20 little-endian int64.  pack: (Am, AmT, Bb, BbT, rpad, npad, ro, no) or None"""
    f7 = _f32_field(scaling) | ((0 if fs is None else _f32_field(fs)) << 32)
    return struct.pack("<20q", W, rows, cols, B, A, mask, rank, f7, dst, dst_t, ld_dst, ld_dst_t, *(pack or (0,) * 8))


def _upload(raw, dtype):
    return torch.frombuffer(bytearray(raw), dtype=dtype).to(DEV)


def _ptr(buf, off=0):
    return buf.data_ptr() + off * buf.element_size()


# (rows, cols, rank, masked, fs, group): three adapters of one fused k = 192 group, a 64x64 one without pack or dst_t, a plain cast
REFRESH_ROWS = ((64, 192, 3, True, ALPHA, 1), (128, 192, 5, False, None, 1), (64, 192, 64, True, None, 1),
                (64, 64, 1, False, None, 2), (128, 128, 0, False, ALPHA, 3))
G1 = {"k": 192, "n": 256, "rpad": 128, "ro": (0, 3, 8), "no": (0, 64, 192)}
REFRESH_SIZES = {"d1": 256 * 192, "t1": 192 * 256, "Am": 128 * 192, "AmT": 192 * 128, "Bb": 256 * 128, "BbT": 128 * 256,
                 "d2": 64 * 128, "d3": 128 * 128, "t3": 128 * 128}


def _refresh_entries(family):
    """the five rows: CPU operands and where each output goes (name, element offset, leading dimension)"""
    out = []
    for i, (rows, cols, r, masked, fs, group) in enumerate(REFRESH_ROWS):
        op = S.family_operands(family, rows, cols, max(r, 1), masked, salt=10 + i)
        e = {"op": op, "rows": rows, "cols": cols, "r": r, "fs": 1.0 if fs is None else fs, "fs_field": fs, "pack": None}
        if group == 1:
            no, ro = G1["no"][i], G1["ro"][i]
            e.update(dst=("d1", no * 192, 192), dst_t=("t1", no, 256),
                     pack={"A": op["A"], "mask": op["mask"], "B": op["B"], "scaling": S.SCALING, "Am": "Am", "AmT": "AmT", "Bb": "Bb",
                           "BbT": "BbT", "rpad": G1["rpad"], "npad": G1["n"], "ro": ro, "no": no})
        elif group == 2:
            e.update(dst=("d2", 64, 128), dst_t=None)     # the right half of a [64, 128] buffer
        else:
            e.update(dst=("d3", 0, 128), dst_t=("t3", 0, 128))
        out.append(e)
    return out


@pytest.mark.parametrize("family", "abc")
def test_refresh_mt_hand_built_table(family):
    entries = _refresh_entries(family)
    mt = {k: S.sentinel(n, BF16, DEV) for k, n in REFRESH_SIZES.items()}     # what the one launch writes
    per = {k: S.sentinel(n, BF16, DEV) for k, n in REFRESH_SIZES.items()}    # what the per-adapter entry points write
    keep, raw, tile_start = [], b"", [0]
    for e in entries:
        op, rows, cols, r = e["op"], e["rows"], e["cols"], e["r"]
        W, B, A, mask = _dev(op["W"]), _dev(op["B"]), _dev(op["A"]), _dev(op["mask"])
        keep += [W, B, A, mask]
        views = {}
        for side, (h, w) in (("dst", (rows, cols)), ("dst_t", (cols, rows))):
            if e[side] is not None:
                name, off, ld = e[side]
                views[side] = (S.view2d(per[name], off, h, w, ld), _ptr(mt[name], off), ld)
        # the per-adapter kernels on the same operands; family (c) takes its f32 effective weight from them
        if r == 0:
            K.weight_shadow(W, rows, cols, True, out=views["dst"][0], out_t=views["dst_t"][0], fwd_scale=e["fs"])
            e["w32"] = op["W"]
        else:
            f = torch.empty(rows, cols, device=DEV)
            K.lora_merge(W, B, A, mask, S.SCALING, out=views["dst"][0], out_t=views["dst_t"][0] if "dst_t" in views else None,
                         rows_pad=rows, cols_pad=cols, out_f32=f, fwd_scale=e["fs"])
            e["w32"] = f.cpu() if family == "c" else S.effective64(op).float()
        pack = None
        if e["pack"] is not None:
            p = e["pack"]
            K.lora_pack(A, mask, B, S.SCALING, per["Am"].view(p["rpad"], cols), per["AmT"].view(cols, p["rpad"]),
                        per["Bb"].view(p["npad"], p["rpad"]), per["BbT"].view(p["rpad"], p["npad"]), p["ro"], p["no"])
            pack = (_ptr(mt["Am"]), _ptr(mt["AmT"]), _ptr(mt["Bb"]), _ptr(mt["BbT"]), p["rpad"], p["npad"], p["ro"], p["no"])
        raw += _table_row(_ptr(W), rows, cols, _ptr(B) if r else 0, _ptr(A) if r else 0, 0 if mask is None or not r else _ptr(mask), r,
                          S.SCALING, e["fs_field"], views["dst"][1], views["dst_t"][1] if "dst_t" in views else 0, views["dst"][2],
                          views["dst_t"][2] if "dst_t" in views else 0, pack)
        tile_start.append(tile_start[-1] + (rows // 64) * (cols // 64))
    assert tile_start == [0, 3, 9, 12, 13, 17]
    table, ts = _upload(raw, torch.int64).view(len(entries), 20), _upload(struct.pack(f"<{len(tile_start)}i", *tile_start), torch.int32)
    K.lora_refresh_mt(table, ts, len(entries), tile_start[-1])
    torch.cuda.synchronize()

    want = {k: S.sentinel(n) for k, n in REFRESH_SIZES.items()}
    S.ref_refresh(entries, want)
    for k in REFRESH_SIZES:
        _bitwise(mt[k], want[k], f"family ({family}): {k} against the reference")
        _bitwise(mt[k], per[k], f"family ({family}): {k} against the per-adapter kernels")


def test_refresh_mt_single_tile_and_empty_table():
    op = S.family_operands("a", 64, 64, 3, True, salt=30)
    W, B, A, mask = _dev(op["W"]), _dev(op["B"]), _dev(op["A"]), _dev(op["mask"])
    d, t = Target(64, 64), Target(64, 64)
    packs = [Target(64, 64), Target(64, 64), Target(64, 64), Target(64, 64)]
    raw = _table_row(_ptr(W), 64, 64, _ptr(B), _ptr(A), _ptr(mask), 3, S.SCALING, None, _ptr(d.buf), _ptr(t.buf), 64, 64,
                     tuple(_ptr(p.buf) for p in packs) + (64, 64, 61, 0))
    table, ts = _upload(raw, torch.int64).view(1, 20), _upload(struct.pack("<2i", 0, 1), torch.int32)
    K.lora_refresh_mt(table, ts, 0, 0)
    K.lora_refresh_mt(table, ts, 1, 0)
    torch.cuda.synchronize()
    for tg in [d, t] + packs:
        tg.untouched("n = 0 / total_tiles = 0")
    K.lora_refresh_mt(table, ts, 1, 1)
    torch.cuda.synchronize()
    img, img_t = S.images(S.effective64(op).float(), 64, 64)
    d.expect(img, "single tile: dst")
    t.expect(img_t, "single tile: dst_t")
    want = S.pack_buffers(S.PackScenario("a", 64, 64, 64, (), True))
    S.ref_pack(op["A"], op["mask"], op["B"], S.SCALING, *want, 61, 0)
    for p, w, name in zip(packs, want, ("Am", "AmT", "Bb", "BbT")):
        p.expect(w, f"single tile: {name}")


# ------------------------------------------------------------------------------------------------ wft_mt_copy_f32
def test_mt_copy_rows():
    rows = S.copy_rows()
    srcs = [src.to(DEV) for src, _, _ in rows]
    dsts = [S.sentinel(n + S.COPY_TAIL, F32, DEV) for _, n, _ in rows]
    raw = b"".join(struct.pack("<3q", _ptr(s), _ptr(d), S.copy_count_field(n, scale)) for s, d, (_, n, scale) in zip(srcs, dsts, rows))
    K.mt_copy_f32(_upload(raw, torch.int64).view(len(rows), 3))
    torch.cuda.synchronize()
    for (_, n, scale), got, want in zip(rows, dsts, S.ref_mt_copy(rows)):
        _bitwise(got, want, f"count {n}, scale {scale}")
