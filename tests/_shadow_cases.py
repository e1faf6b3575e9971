"""Cases, references and mutants for the weight-shadow kernels of csrc/shadow.hip: wft_cast_f32_bf16,
wft_cast_pad_transpose_f32_bf16, wft_lora_merge, wft_lora_pack, wft_lora_refresh_mt and wft_mt_copy_f32 (wft_quantize_rows_i8 has
tests/_q8_cases.py).  Shared by tests/test_shadow_host.py (CPU: the inputs have the properties claimed below and the references
reject every listed mutant) and tests/test_shadow_gpu.py (the kernels against the same references, bit for bit).

Input families (`operands(case)`), W f32 [rows, cols], B f32 [rows, r], A f32 [r, cols], mask f32 [cols] or None, scaling 2:
  (a) dense-exact   W = integer in [-64, 64] / 16; B, A nonzero integers in +-[1, 8]; mask in {0, 1.25}, about 20 % zeros.
                    (2 A) mask is exact, every product B (2 A mask) is a multiple of 0.5 no larger than 160, and every partial sum
                    of W + sum_q B as is a multiple of 1/16 below 2^14: 18 bits at most, so the f32 chain is exact in any order,
                    with or without fma, the f32 output equals the float64 value and each bf16 image is its single rounding to
                    nearest even.  Multiples of 1/16 above 16 are ties of that rounding half of the time.
  (b) probe         B[i, q] = +-4 at q = i % r only, A integers in +-[1, 7], mask in {0, 2}, W integers in [-7, 7]: every output is
                    W + 16 k with |k| <= 7, an integer of at most 7 bits, which bf16 holds exactly.  A lost W, a lost or
                    mis-indexed (row, q, col) term or a shifted mask column changes the bf16 image by at least 1.
  (c) realistic     W ~ 0.05 randn, A, B ~ 0.1 randn, mask in {0, 1 / 0.8}.  Float64 reference; per element, with u = 2^-24,
                    |f32 output - reference| <= (r + 3) u (|W| + sum_q |s B A mask|): two roundings form as = (s A) mask, r fma
                    roundings act on partial sums that this sum bounds, one u is slack for the second-order terms.  The bf16
                    images must be the roundings of the f32 output the kernel wrote.
  (d) special       `special_values()`: the f32 bit patterns around the ties, the bf16 subnormals, the largest finite f32 and the
                    NaNs, each with both signs.  Expected is torch's CPU `.to(bfloat16)` ("what `W.to(x.dtype)` does", wft.h):
                    bitwise for every result that is not a NaN, a NaN for a NaN (`same_bf16`).

References, from the text of wft.h alone: `effective64` (W + s B (A mask) in float64), `images` (the padded bf16 image and its
transpose of an f32 matrix; the forward-scaled image is bf16(f32(w) * f32(fs)), one f32 multiply and one rounding; the transposed
image is never scaled), `ref_pack`, `ref_mt_copy`, `ref_refresh` (images + ref_pack per table row).  Buffers are flat and filled
with SENT (bf16 7.0 / f32 7.0) before a reference or a kernel writes into them; `view2d` places a matrix at an element offset and
a leading dimension inside one, so a whole-buffer comparison sees every element the contract leaves alone: beyond cols_pad inside
a wider ld, other adapters' blocks of Am / AmT / Bb / BbT, the elements after a copy's count.

Mutants (`MUTANTS`: name -> what a case needs to show it); test_shadow_host.py asserts that every applicable case rejects each.
"""
import dataclasses
import functools

import torch

BF16 = torch.bfloat16
F32 = torch.float32
U = 2.0 ** -24
SENT = 7.0
SCALING = 2.0
# softmax scale of a 64-wide head times log2(e), both as f32: what ops.QK_ALPHA folds into the forward shadow of a q projection
ALPHA = float(torch.tensor(64 ** -0.5, dtype=F32) * torch.tensor(1.4426950408889634, dtype=F32))

# (rows, cols, rank) of families (a), (b), (c) and the padded image each is written into
SHAPES = ((64, 64, 1), (64, 64, 3), (37, 198, 5), (128, 192, 16), (100, 200, 64))
PADS = {(64, 64): (64, 64), (37, 198): (128, 256), (128, 192): (128, 192), (100, 200): (128, 256)}
# (rows, cols) -> (rows_pad, cols_pad) of the plain cast; (10, 64) -> (256, 128) has whole tiles of padding
CAST_LAYOUTS = (((1, 1), (128, 128)), ((64, 64), (64, 64)), ((100, 200), (128, 256)), ((37, 198), (128, 256)), ((10, 64), (256, 128)))

SPECIAL_BITS = (0x00000000, 0x00000001, 0x00008000, 0x00008001, 0x00018000, 0x007f8000, 0x007fffff,
                0x3f807fff, 0x3f808000, 0x3f808001, 0x3f818000,
                0x7f7f7fff, 0x7f7f8000, 0x7f7fffff, 0x7f800000, 0x7f800001, 0x7fc00000)

ROUND_MUTANTS = ("round-half-up instead of ties-to-even", "truncation instead of rounding", "NaN turned to infinity by the rounding add")
# name -> (entry point, which cases can show it)
MUTANTS = {
    "term q = 0 dropped": ("merge", "every case of (a), (b), (c)"),
    "term q = r - 1 dropped": ("merge", "every case of (a), (b), (c)"),
    "W dropped": ("merge", "every case of (a), (b), (c)"),
    "mask ignored": ("merge", "the masked cases of (a), (b), (c)"),
    "mask shifted by one column": ("merge", "the masked cases of (a), (b), (c)"),
    "scaling also applied to W": ("merge", "every case of (a), (b), (c)"),
    "B row taken without the tile's row offset": ("merge", "the cases of (a), (b), (c) with more than 64 rows"),
    "fwd_scale applied to dst_t": ("images", "(a), (b), (c) with fwd_scale = ALPHA"),
    "dst_t built from the scaled image": ("images", "(a), (b), (c) with fwd_scale = ALPHA"),
    "padding left unwritten": ("images", "the cases of (a), (b), (c) whose padded image is larger than the weight"),
    "round-half-up instead of ties-to-even": ("images", "every case of (a): its ties with an even kept bit; (d)"),
    "truncation instead of rounding": ("images", "every case of (a) and (c); (d)"),
    "NaN turned to infinity by the rounding add": ("images", "(d)"),
    "pack: ro ignored": ("pack", "every pack scenario (each has an adapter at ro > 0)"),
    "pack: no ignored": ("pack", "every pack scenario (each has an adapter at no > 0)"),
    "pack: AmT pitch K instead of rpad": ("pack", "the pack scenarios with K != rpad"),
    "pack: Bb / BbT swapped": ("pack", "every pack scenario"),
    "pack: scaling missing from Bb": ("pack", "every pack scenario"),
    "mt_copy: scale ignored": ("mt_copy", "the table of copy_rows(): its scaled rows"),
    "mt_copy: count taken from all 64 bits": ("mt_copy", "the table of copy_rows(): its scaled rows"),
}


# ------------------------------------------------------------------------------------------------ bits and rounding
def f32_bits(t):
    """f32 tensor -> its bit patterns as int64 in [0, 2^32)"""
    return t.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff


def bf16_from_bits(b):
    """int64 bit patterns (the low 16 bits count) -> bf16 tensor"""
    b = b & 0xffff
    return torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16).view(BF16)


def bf16_bits(t):
    return t.contiguous().view(torch.int16).to(torch.int64) & 0xffff


def rne_bits(t):
    """round-to-nearest-even of f32 to bf16 written out on the bits (NaN -> the quiet NaN of its sign's magnitude 0x7fc0, as torch
    does): the independent statement test_shadow_host.py holds torch's `.to(bfloat16)` against"""
    b = f32_bits(t)
    out = ((b + 0x7fff + ((b >> 16) & 1)) >> 16) & 0xffff
    return torch.where(torch.isnan(t), torch.full_like(b, 0x7fc0), out)


def round_bf16(t, mut=None):
    """f32 -> bf16 as the contract has it (torch CPU), or as one of ROUND_MUTANTS has it"""
    if mut is None:
        return t.to(BF16)
    b = f32_bits(t)
    nan = torch.isnan(t)
    if mut == "round-half-up instead of ties-to-even":
        out = torch.where(nan, torch.full_like(b, 0x7fc0), (b + 0x8000) >> 16)
    elif mut == "truncation instead of rounding":
        out = torch.where(nan, torch.full_like(b, 0x7fc0), b >> 16)
    elif mut == "NaN turned to infinity by the rounding add":
        out = (b + 0x7fff + ((b >> 16) & 1)) >> 16
    else:
        raise KeyError(mut)
    return bf16_from_bits(out).view(t.shape)


def same_bf16(got, want):
    """bitwise equal where `want` is no NaN, a NaN where it is one"""
    got, want = got.cpu(), want.cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = torch.isnan(want.float())
    if not torch.equal(torch.isnan(got.float()), nan):
        return False
    return torch.equal(bf16_bits(got)[~nan], bf16_bits(want)[~nan])


def special_values():
    """family (d): f32 [34], every pattern of SPECIAL_BITS and its sign flip"""
    b = torch.tensor([p | s for p in SPECIAL_BITS for s in (0, 0x80000000)], dtype=torch.int64)
    return torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32).view(F32)


def special_matrix(rows, cols):
    """family (d) repeated over a [rows, cols] matrix (rows * cols need not be a multiple of 34: the patterns land in every lane)"""
    v = special_values()
    return v.repeat(-(-rows * cols // v.numel()))[:rows * cols].view(rows, cols).clone()


def tie_counts(w32):
    """(ties whose kept bit is even, ties whose kept bit is odd) of the bf16 rounding of an f32 tensor: low half exactly 0x8000"""
    b = f32_bits(w32)
    tie = (b & 0xffff) == 0x8000
    odd = ((b >> 16) & 1) == 1
    return int((tie & ~odd).sum()), int((tie & odd).sum())


# ------------------------------------------------------------------------------------------------ cases and operands
@dataclasses.dataclass(frozen=True)
class Case:
    family: str      # "a", "b", "c"
    rows: int
    cols: int
    r: int
    masked: bool

    @property
    def name(self):
        return f"{self.family}-{self.rows}x{self.cols}-r{self.r}-{'mask' if self.masked else 'nomask'}"

    @property
    def pads(self):
        return PADS[(self.rows, self.cols)]

    @property
    def seed(self):
        return (self.rows * 1000003 + self.cols * 1009 + self.r * 17 + "abc".index(self.family)) & 0x7fffffff


@functools.lru_cache(maxsize=None)
def merge_cases():
    return tuple(Case(f, rows, cols, r, m) for f in "abc" for rows, cols, r in SHAPES for m in (True, False))


def _signed(gen, shape, hi):
    """nonzero integers in +-[1, hi] as f32"""
    mag = torch.randint(1, hi + 1, shape, generator=gen)
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (mag * sign).to(F32)


@functools.lru_cache(maxsize=None)
def _operands(family, rows, cols, r, seed):
    gen = torch.Generator().manual_seed(seed)
    if family == "a":
        W = torch.randint(-64, 65, (rows, cols), generator=gen).to(F32) / 16
        B, A = _signed(gen, (rows, r), 8), _signed(gen, (r, cols), 8)
        mask = torch.where(torch.rand(cols, generator=gen) < 0.2, 0.0, 1.25).to(F32)
    elif family == "b":
        W = torch.randint(-7, 8, (rows, cols), generator=gen).to(F32)
        B = torch.zeros(rows, r)
        i = torch.arange(rows)
        B[i, i % r] = _signed(gen, (rows,), 1) * 4
        A = _signed(gen, (r, cols), 7)
        mask = torch.where(torch.rand(cols, generator=gen) < 0.2, 0.0, 2.0).to(F32)
    elif family == "c":
        W = 0.05 * torch.randn(rows, cols, generator=gen)
        B, A = 0.1 * torch.randn(rows, r, generator=gen), 0.1 * torch.randn(r, cols, generator=gen)
        mask = torch.where(torch.rand(cols, generator=gen) < 0.2, 0.0, 1 / 0.8).to(F32)
    else:
        raise KeyError(family)
    if cols > 1:
        mask[0], mask[1] = 0.0, mask.max()   # a zero next to a kept column: a shift of the mask shows in every case
    return {"W": W, "B": B, "A": A, "mask": mask}


def operands(case):
    """{"W", "B", "A", "mask" (None if the case is not masked), "scaling"}: shared f32 CPU tensors, nobody writes to them"""
    op = dict(_operands(case.family, case.rows, case.cols, case.r, case.seed))
    if not case.masked:
        op["mask"] = None
    op["scaling"] = SCALING
    return op


def family_operands(family, rows, cols, r, masked, salt=0):
    """operands of a shape outside SHAPES (the rows of the refresh table, the pack scenarios)"""
    op = dict(_operands(family, rows, cols, r, (rows * 1000003 + cols * 1009 + r * 17 + 7919 * salt + "abc".index(family)) & 0x7fffffff))
    if not masked:
        op["mask"] = None
    op["scaling"] = SCALING
    return op


# ------------------------------------------------------------------------------------------------ wft_lora_merge
def effective64(op, mut=None):
    """W + scaling * B @ (A * mask) in float64 [rows, cols]"""
    W, B, A, mask, s = op["W"].double(), op["B"].double(), op["A"].double(), op["mask"], op["scaling"]
    rows, r = B.shape
    m = torch.ones(A.shape[1], dtype=torch.float64) if mask is None or mut == "mask ignored" else mask.double()
    if mut == "mask shifted by one column":
        m = torch.roll(m, 1)
    if mut == "B row taken without the tile's row offset":
        B = B[torch.arange(rows) % 64]
    if mut in ("term q = 0 dropped", "term q = r - 1 dropped"):
        B = B.clone()
        B[:, 0 if mut == "term q = 0 dropped" else r - 1] = 0
    if mut == "W dropped":
        W = torch.zeros_like(W)
    if mut == "scaling also applied to W":
        W = s * W
    return W + B @ ((s * A) * m)


def merge_bound(op):
    """(r + 3) u (|W| + sum_q |s B A mask|) in float64 [rows, cols]: see the top"""
    W, B, A, mask, s = op["W"].double(), op["B"].double(), op["A"].double(), op["mask"], op["scaling"]
    m = torch.ones(A.shape[1], dtype=torch.float64) if mask is None else mask.double()
    return (A.shape[0] + 3) * U * (W.abs() + B.abs() @ ((s * A) * m).abs())


def restate_f32(op):
    """lora_merge_kernel's arithmetic in CPU float32, in its order: as = (s * A) * mask, two f32 multiplies; acc = W, then
    acc = fmaf(B[:, q], as[q], acc) for q = 0 .. r - 1 (the product is exact in float64; one rounding to f32)"""
    s = torch.tensor(op["scaling"], dtype=F32)
    as_ = s * op["A"]
    if op["mask"] is not None:
        as_ = as_ * op["mask"]
    acc = op["W"].clone()
    for q in range(op["A"].shape[0]):
        acc = (op["B"][:, q:q + 1].double() * as_[q:q + 1].double() + acc.double()).float()
    return acc


def images(w32, rows_pad, cols_pad, fs=1.0, mut=None):
    """f32 [rows, cols] -> (bf16 [rows_pad, cols_pad] = bf16(f32(w) * f32(fs)), bf16 [cols_pad, rows_pad] = bf16(w) transposed),
    both zero padded"""
    rows, cols = w32.shape
    rmut = mut if mut in ROUND_MUTANTS else None
    fill = SENT if mut == "padding left unwritten" else 0.0
    fs32 = torch.tensor(fs, dtype=F32)
    plain = round_bf16(w32, rmut)
    scaled = plain if fs == 1.0 else round_bf16(w32 * fs32, rmut)
    img = torch.full((rows_pad, cols_pad), fill, dtype=BF16)
    img_t = torch.full((cols_pad, rows_pad), fill, dtype=BF16)
    img[:rows, :cols] = scaled
    t = plain
    if mut == "fwd_scale applied to dst_t":
        t = round_bf16(plain.float() * fs32)
    if mut == "dst_t built from the scaled image":
        t = scaled
    img_t[:cols, :rows] = t.t()
    return img, img_t


# ------------------------------------------------------------------------------------------------ flat sentinel buffers
def sentinel(n, dtype=BF16, device="cpu"):
    return torch.full((n,), SENT, dtype=dtype, device=device)


def view2d(buf, off, rows, cols, ld):
    """[rows, cols] with row stride ld at element offset off inside the flat buffer"""
    assert buf.dim() == 1 and off >= 0 and (rows - 1) * ld + cols + off <= buf.numel()
    return torch.as_strided(buf, (rows, cols), (ld, 1), buf.storage_offset() + off)


# ------------------------------------------------------------------------------------------------ wft_lora_pack
def ref_pack(A, mask, B, scaling, Am, AmT, Bb, BbT, ro, no, mut=None):
    """writes one adapter's blocks into the CPU bf16 buffers Am [rpad, K], AmT [K, rpad], Bb [npad, rpad], BbT [rpad, npad]:
    Am rows ro .. ro + r = bf16((s A) mask), Bb block (no .. no + n, ro .. ro + r) = bf16(s B), and their transposes"""
    r, K = A.shape
    n = B.shape[0]
    rpad, npad = Am.shape[0], Bb.shape[0]
    assert Am.shape == (rpad, K) and AmT.shape == (K, rpad) and Bb.shape == (npad, rpad) and BbT.shape == (rpad, npad)
    assert ro + r <= rpad and no + n <= npad
    s = torch.tensor(scaling, dtype=F32)
    am = s * A
    if mask is not None:
        am = am * mask.reshape(1, K)
    am = am.to(BF16)
    bb = (B if mut == "pack: scaling missing from Bb" else s * B).to(BF16)
    if mut == "pack: ro ignored":
        ro = 0
    if mut == "pack: no ignored":
        no = 0
    q, c, row = torch.arange(r), torch.arange(K), torch.arange(n)
    Am[ro:ro + r] = am
    if mut == "pack: AmT pitch K instead of rpad":
        idx = (c[None, :] * K + ro + q[:, None]).reshape(-1)
        ok = idx < AmT.numel()
        AmT.view(-1)[idx[ok]] = am.reshape(-1)[ok]
    else:
        AmT[:, ro:ro + r] = am.t()
    if mut == "pack: Bb / BbT swapped":
        Bb.view(-1)[((ro + q[None, :]) * npad + no + row[:, None]).reshape(-1)] = bb.reshape(-1)
        BbT.view(-1)[((no + row[:, None]) * rpad + ro + q[None, :]).reshape(-1)] = bb.reshape(-1)
    else:
        Bb[no:no + n, ro:ro + r] = bb
        BbT[ro:ro + r, no:no + n] = bb.t()


@dataclasses.dataclass(frozen=True)
class PackScenario:
    family: str
    K: int
    rpad: int
    npad: int
    adapters: tuple    # (rank, n, ro, no)
    masked: bool

    @property
    def name(self):
        return f"{self.family}-K{self.K}-" + "+".join(f"r{r}n{n}" for r, n, _, _ in self.adapters) + ("-mask" if self.masked else "-nomask")


@functools.lru_cache(maxsize=None)
def pack_scenarios():
    """three adapters of ranks 1, 5, 24 with n = 1, 100, 128 (rpad 64) and two of rank 64 (rpad 128), at K = 64, 77, 384"""
    out = []
    for fam in "ac":
        for K in (64, 77, 384):
            for masked in (True, False):
                out.append(PackScenario(fam, K, 64, 256, ((1, 1, 0, 0), (5, 100, 1, 1), (24, 128, 6, 101)), masked))
                out.append(PackScenario(fam, K, 128, 256, ((64, 128, 0, 0), (64, 100, 64, 128)), masked))
    return tuple(out)


def pack_operands(sc):
    """[(A, mask, B)] per adapter of the scenario"""
    out = []
    for i, (r, n, _, _) in enumerate(sc.adapters):
        op = family_operands(sc.family, n, sc.K, r, sc.masked, salt=i + 1)
        out.append((op["A"], op["mask"], op["B"]))
    return out


def pack_buffers(sc, device="cpu"):
    """sentinel-filled Am, AmT, Bb, BbT"""
    mk = lambda a, b: torch.full((a, b), SENT, dtype=BF16, device=device)   # noqa: E731
    return mk(sc.rpad, sc.K), mk(sc.K, sc.rpad), mk(sc.npad, sc.rpad), mk(sc.rpad, sc.npad)


def ref_pack_scenario(sc, mut=None):
    bufs = pack_buffers(sc)
    for (A, mask, B), (_, _, ro, no) in zip(pack_operands(sc), sc.adapters):
        ref_pack(A, mask, B, SCALING, *bufs, ro, no, mut=mut)
    return bufs


# ------------------------------------------------------------------------------------------------ wft_lora_refresh_mt
def ref_refresh(entries, bufs, mut=None):
    """every row of a refresh table into the flat CPU sentinel buffers `bufs` (name -> tensor).  An entry: {"w32": the f32
    effective weight [rows, cols] (W itself at rank 0), "fs", "dst": (name, offset, ld), "dst_t": (name, offset, ld) or None,
    "pack": None or {"A", "mask", "B", "scaling", "Am", "AmT", "Bb", "BbT" (names of whole buffers), "rpad", "npad", "ro", "no"}}"""
    for e in entries:
        rows, cols = e["w32"].shape
        img, img_t = images(e["w32"], rows, cols, e["fs"], mut=mut)
        name, off, ld = e["dst"]
        view2d(bufs[name], off, rows, cols, ld).copy_(img)
        if e["dst_t"] is not None:
            name, off, ld = e["dst_t"]
            view2d(bufs[name], off, cols, rows, ld).copy_(img_t)
        p = e["pack"]
        if p is not None:
            K, rpad, npad = p["A"].shape[1], p["rpad"], p["npad"]
            ref_pack(p["A"], p["mask"], p["B"], p["scaling"], bufs[p["Am"]].view(rpad, K), bufs[p["AmT"]].view(K, rpad),
                     bufs[p["Bb"]].view(npad, rpad), bufs[p["BbT"]].view(rpad, npad), p["ro"], p["no"], mut=mut)


# ------------------------------------------------------------------------------------------------ wft_mt_copy_f32
COPY_COUNTS = (1, 255, 256, 257, 1000)
COPY_TAIL = 3   # elements after each source's count and after each destination, which a copy must leave alone


@functools.lru_cache(maxsize=None)
def copy_rows():
    """[(src f32 [count + COPY_TAIL], count, scale or None)]: every count plain and scaled, in one table"""
    gen = torch.Generator().manual_seed(20)
    out = []
    for i, n in enumerate(COPY_COUNTS):
        out.append((torch.randn(n + COPY_TAIL, generator=gen), n, None))
        out.append((torch.randn(n + COPY_TAIL, generator=gen), n, ALPHA if i % 2 == 0 else 0.3))
    return tuple(out)


def copy_count_field(count, scale):
    """field 2 of a table row: the count in bits 0..31, the scale's f32 bits in bits 32..63 (0: a plain copy)"""
    return count | (0 if scale is None else int(f32_bits(torch.tensor([scale], dtype=F32))[0]) << 32)


def ref_mt_copy(rows, mut=None):
    """-> one flat f32 destination per row, count + COPY_TAIL long: src[:count] (* f32(scale), one f32 multiply), then SENT"""
    out = []
    for src, count, scale in rows:
        dst = sentinel(count + COPY_TAIL, F32)
        n = count
        if mut == "mt_copy: count taken from all 64 bits":
            n = min(copy_count_field(count, scale), src.numel(), dst.numel())
        v = src[:n]
        if scale is not None and mut != "mt_copy: scale ignored":
            v = v * torch.tensor(scale, dtype=F32)
        dst[:n] = v
        out.append(dst)
    return out
