"""Cases, float64 reference, per-element bounds and float32 restatements for the LayerNorm kernels: wft_layernorm_fwd / _bwd and
their _dspan forms (csrc/norm.hip: ln_fwd_kernel<NQ, VAR, DSPAN>, ln_bwd_kernel<DXSUM, NQ, VAR, DSPAN>, ln_bwd_reduce_kernel) and the
fp32-mode twins wft_layernorm_fwd_f32 / wft_layernorm_bwd_f32 (csrc/f32.hip).  Shared by tests/test_layernorm_host.py (CPU: the
bounds accept the kernels' arithmetic and reject every listed mutant of it) and tests/test_layernorm_gpu.py (the kernels themselves
under the same checker).

Cases (`bf16_cases()`): every width of WIDTHS (every NQ = 1..8, each with a full last pass and with a last pass of 2 to 62 pieces
where the width allows) at 5 and 1029 rows; widths 264, 1280 and 2040 also at 1, 3, 1024, 2051 and 8197 rows (partial workgroups;
the last one-level fold, 256 partial rows; the first two-level fold, 258 partial rows, 17 per chunk, a short last chunk; the capped
backward grid, where three waves take a second row through the prefetch; more rows than the forward's largest grid has waves) and,
at 1029 (rows_per_batch 7: row % rows_per_batch wraps 147 times), 2051 and 8197 rows (rows_per_batch 1500: a short last batch),
under the spans of `spans()`.  Row r of a case is of kind
KINDS[(r + offset) % 8], so that neighbouring rows differ by orders of magnitude; gamma = 1 + 0.5 randn, beta = randn (fp32), the
residual gradient randn (bf16).  `f32_cases()`: cols 1, 13, 128, 1000, 1283 at rows 1, 5, 50, 1029, spans (a), (b), (e) on the
three wider ones at 50 and 1029 rows; each on the values before the bf16 rounding and on the bf16-representable copy.

Reference (`reference()`): float64 closed forms, not autograd.  mean, var (biased), rstd = (var + eps)^-1/2, xh = (x - mean) rstd,
y = xh gamma + beta (masked positions 0); g = dy gamma with dy zeroed where masked, s1 = mean_c g, s2 = mean_c g xh,
dx = rstd (g - s1 - xh s2) + dres; dgamma = sum_r dy xh, dbeta = sum_r dy; dxsum = the float64 column sum of the dx the kernel wrote.

Bounds (`check()`): per element, from the reference alone.  With u = 2^-24, d = x - mean:
  F_mean   = u (|mean| + mean_c|x|)
  rho      = 3u + (mean_c|d| F_mean + u var) / (var + eps)
  F_rstd   = rstd rho
  F_xh     = |xh| (rho + 2u) + rstd F_mean
  F_y      = |gamma| F_xh + u (|y| + |beta|)                                                   (masked positions: exactly 0)
  F_s1     = u mean_c|g|
  F_s2     = u mean_c|g xh| + mean_c(|g| F_xh)
  F_dx     = rstd (u (|g| + |s1| + |xh s2|) + F_s1 + |xh| F_s2 + |s2| F_xh) + |dx - dres| rho + u (|dx| + |dres|)
  F_dgamma = (u sum_r|dy xh| + sum_r |dy| F_xh) sqrt(depth)
  F_dbeta  = u sum_r|dy| sqrt(depth)
  F_dxsum  = u sum_r|dx| sqrt(depth)
and the bound of an output is K[output] * F; y and dx of the bf16 kernels get half an ulp of bf16 at the reference value on top.
depth is the number of sequential adds on a column's longest path to the total (`depth_bf16`: rows per wave, the 4 waves of a
workgroup, the partial rows per reduce wave, one per level; fp32 twin: the rows, ln_bwd_dgb_f32_kernel adds them in order).

The constants K are not chosen: test_layernorm_host.py restates both kernels' arithmetic in torch CPU float32, in the kernels' order
(64 lanes, lane l owning the 4-column pieces l, l + 64, ...; xor-butterfly wave sums; the fmas where the source has them and where the
compiler contracts a * b + c; rows of a wave in order, four waves in order, the one- or two-level partial fold; fp32 twin: lane l
owning columns l, l + 64, ..., rows in order), measures max |restatement - reference| / F over all cases of both lists, and K is
4 x that (the GPU's rsqrtf and division are looser than the CPU's), rounded up to a power of two.  Measured (seed = case index):

  output   worst ratio bf16-kernel restatement   worst ratio fp32-twin restatement   4 x worst   K
  y        0.989                                 1.127                               4.51        8
  mean     0.996                                 1.135                               4.54        8
  rstd     0.995                                 0.817                               3.98        4
  dx       0.991                                 0.976                               3.96        4
  dgamma   0.302                                 0.443                               1.77        2
  dbeta    0.080                                 0.972                               3.89        4
  dxsum    0.370                                 -                                   1.48        2
"""
import dataclasses
import functools
import math

import torch

U = 2.0 ** -24
EPS = 1e-5
WIDTHS = (8, 64, 256, 264, 384, 512, 768, 1000, 1024, 1280, 1536, 1792, 2040, 2048)
SPAN_WIDTHS = (264, 1280, 2040)
ROWS_ALL, ROWS_MORE = (5, 1029), (1, 3, 1024, 2051, 8197)
SPAN_ROWS = ((1029, 7), (2051, 1500), (8197, 1500))            # (rows, rows_per_batch)
F32_COLS, F32_ROWS = (1, 13, 128, 1000, 1283), (1, 5, 50, 1029)
KINDS = ("randn", "randn x 3 + 0.5", "constant 2.5", "256 + 4 randn", "randn x 2^-10", "outlier 200 in the last column",
         "dy = |randn|", "dy = 2 (x - mean x)")
K = {"y": 8.0, "mean": 8.0, "rstd": 4.0, "dx": 4.0, "dgamma": 2.0, "dbeta": 4.0, "dxsum": 2.0}
FWD_WAVES_MAX = 8 * 256 * 4   # the forward's largest grid: 8 workgroups on each of 256 CUs, 4 waves each

MUTANTS = {
    "dx terms": ("s1 term dropped", "s2 term dropped", "dres dropped"),
    "lost contributions": ("s1 and s2 sums miss the last piece", "row mean misses the last piece", "dgamma fold loses the last row",
                           "dbeta fold loses row 0", "dxsum summed before the bf16 rounding"),
    "variance": ("variance over cols - 1", "eps outside the square root", "one-pass variance"),
    "stale data": ("gamma of piece ch - 64 in the last pass", "stale prefetch"),
    "masked positions and reduce": ("masked dy not zeroed in s1 and s2", "masked columns contribute to dgamma", "t = row / rpb",
                                    "span end inclusive", "short last reduce chunk skipped"),
}
ALL_MUTANTS = tuple(m for fam in MUTANTS.values() for m in fam)


def spans(rpb, cols):
    """the deep-SpecAugment spans (rows_per_batch, t0, t1, c0, c1) of the issue, by letter"""
    return {"a": (rpb, 0, 3, 0, 5), "b": (rpb, rpb - 2, rpb, cols - 3, cols), "c": (rpb, 0, 0, 250, 262), "d": (rpb, 0, 0, 0, 0),
            "e": (rpb, 0, 0, 0, cols)}


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    rows: int
    cols: int
    offset: int
    seed: int
    mask: tuple = None    # (rows_per_batch, t0, t1, c0, c1) or None
    span: str = ""        # its letter

    @property
    def family(self):
        return f"span ({self.span})" if self.span else "plain"


@functools.lru_cache(maxsize=None)
def bf16_cases():
    shapes = [(r, c) for c in WIDTHS for r in ROWS_ALL] + [(r, c) for c in SPAN_WIDTHS for r in ROWS_MORE]
    out = [Case(f"{r}x{c}", r, c, (3 * i) % 8 if r > 1 else i % 8, i) for i, (r, c) in enumerate(shapes)]
    seed = {(c.rows, c.cols): (c.seed, c.offset) for c in out}
    for c in SPAN_WIDTHS:
        for r, rpb in SPAN_ROWS:
            for letter, m in spans(rpb, c).items():
                if letter == "c" and c < 262:
                    continue
                s, off = seed[(r, c)]
                out.append(Case(f"{r}x{c}-span-{letter}-rpb{rpb}", r, c, off, s, m, letter))   # the inputs of the plain case
    return tuple(out)


@functools.lru_cache(maxsize=None)
def f32_cases():
    out = []
    for c in F32_COLS:
        for r in F32_ROWS:
            i = len(out)
            out.append(Case(f"f32-{r}x{c}", r, c, (3 * i) % 8 if r > 1 else i % 8, 100 + i))
            if c >= 13 and c != 128 and r >= 50:
                sp = spans(7, c)
                out += [Case(f"f32-{r}x{c}-span-{k}-rpb7", r, c, (3 * i) % 8, 100 + i, sp[k], k) for k in "abe"]
    return tuple(out)


def _bfq(t):
    return t.to(torch.bfloat16).float()


def make_rows(rows, cols, offset, gen, device="cpu", q=_bfq):
    """x, dy, dres f32 [rows, cols] of the row kinds, row r of kind KINDS[(r + offset) % 8]; q rounds them (bf16 by default)"""
    kind = ((torch.arange(rows, device=device) + offset) % len(KINDS))[:, None]
    rx = torch.randn(rows, cols, generator=gen, device=device)
    x = rx.clone()
    x = torch.where(kind == 1, rx * 3 + 0.5, x)
    x = torch.where(kind == 2, torch.full_like(rx, 2.5), x)
    x = torch.where(kind == 3, 256 + 4 * rx, x)
    x = torch.where(kind == 4, rx * 2.0 ** -10, x)
    last = torch.arange(cols, device=device)[None, :] == cols - 1
    x = q(torch.where((kind == 5) & last, torch.full_like(rx, 200.0), x))
    del rx
    dy = torch.randn(rows, cols, generator=gen, device=device)
    dy = torch.where(kind == 6, dy.abs(), dy)
    dy = q(torch.where(kind == 7, 2 * (x - x.mean(1, keepdim=True)), dy))
    dres = q(torch.randn(rows, cols, generator=gen, device=device))
    return x, dy, dres


@functools.lru_cache(maxsize=2)
def _inputs(rows, cols, offset, seed, exact):
    gen = torch.Generator().manual_seed(seed)
    gamma = 1 + 0.5 * torch.randn(cols, generator=gen)
    beta = torch.randn(cols, generator=gen)
    x, dy, dres = make_rows(rows, cols, offset, gen, q=(lambda t: t) if exact else _bfq)
    return {"x": x, "dy": dy, "dres": dres, "gamma": gamma, "beta": beta}


def inputs(case, fp32_values=False):
    """the case's operands (f32 CPU tensors, bf16-representable unless fp32_values); shared, nobody writes to them.  The span
    cases of a shape share the plain case's operands."""
    return _inputs(case.rows, case.cols, case.offset, case.seed, fp32_values)


def masked(rows, cols, mask, device="cpu", r0=0, mut=None):
    """bool [rows, cols] of the positions the span zeroes (rows r0 .. r0 + rows of the tensor), or None"""
    if mask is None or mask[0] <= 0:
        return None
    rpb, t0, t1, c0, c1 = mask
    r = torch.arange(r0, r0 + rows, device=device)
    t = torch.div(r, rpb, rounding_mode="floor") if mut == "t = row / rpb" else r % rpb
    c = torch.arange(cols, device=device)
    if mut == "span end inclusive":
        return ((t >= t0) & (t <= t1))[:, None] | ((c >= c0) & (c <= c1))[None, :]
    return ((t >= t0) & (t < t1))[:, None] | ((c >= c0) & (c < c1))[None, :]


# ------------------------------------------------------------------------------------------------ dispatch of norm.hip, restated
def bwd_grid(rows):
    return max(1, min((rows + 3) // 4, 512))


def fold_levels(rows):
    """partial rows each level of ln_bwd_reduce_kernel folds: one level up to 256 partial rows, else 16 chunks and then the 16"""
    g = bwd_grid(rows)
    return (g,) if g <= 256 else ((g + 15) // 16, 16)


def depth_bf16(rows):
    g = bwd_grid(rows)
    lv = fold_levels(rows)
    return -(-rows // (4 * g)) + 4 + sum(-(-n // 4) for n in lv) + len(lv)


# ------------------------------------------------------------------------------------------------ float64 reference and bounds
@functools.lru_cache(maxsize=1)
def _x_part(x, eps):
    """what the reference takes from x alone; the span cases of a shape share it (the key is the tensor itself).  F_xh is kept
    as |xh| a + b with the per-row a = rho + 2u, b = rstd F_mean."""
    x = x.double()
    mean = x.mean(1)
    d = x - mean[:, None]
    var = (d * d).mean(1)
    rstd = (var + eps) ** -0.5
    xh = d * rstd[:, None]
    f_mean = U * (mean.abs() + x.abs().mean(1))
    rho = 3 * U + (d.abs().mean(1) * f_mean + U * var) / (var + eps)
    return mean, rstd, xh, xh.abs(), f_mean, rho, rho + 2 * U, rstd * f_mean


@functools.lru_cache(maxsize=1)
def _y_part(x, gamma, beta, eps):
    _, _, xh, axh, _, _, a, b = _x_part(x, eps)
    gamma, beta = gamma.double(), beta.double()
    y = xh * gamma + beta
    return y, gamma.abs() * (axh * a[:, None] + b[:, None]) + U * (y.abs() + beta.abs())


def reference(inp, mask=None, r0=0, r1=None, eps=EPS, per_row=True):
    """float64 closed forms on rows [r0, r1) of the operands (any device) -> dict: the per-row references and bound forms F (left
    out with per_row=False) and the column sums over these rows, which add up over row chunks: dgamma, dbeta, and A_dgamma, A_dbeta
    with F_dgamma = A_dgamma sqrt(depth), F_dbeta = A_dbeta sqrt(depth).  The sums over a row or a column of a product with a
    per-column or per-row factor are written as matrix-vector products."""
    whole = r0 == 0 and (r1 is None or r1 == inp["x"].shape[0])
    r1 = inp["x"].shape[0] if r1 is None else r1
    dy, gamma = inp["dy"][r0:r1].double(), inp["gamma"].double()
    mean, rstd, xh, axh, f_mean, rho, a, b = _x_part(inp["x"], eps) if whole else _x_part.__wrapped__(inp["x"][r0:r1], eps)
    rows, cols = xh.shape
    m = masked(rows, cols, mask, xh.device, r0)
    if m is not None:
        dy = dy.masked_fill(m, 0.0)
    ady, dyxh = dy.abs(), dy * xh
    adyxh = dyxh.abs()
    out = {"dgamma": dyxh.sum(0), "dbeta": dy.sum(0), "A_dgamma": (U + a) @ adyxh + b @ ady, "A_dbeta": U * ady.sum(0), "masked": m}
    if not per_row:
        return out
    if whole:
        y, f_y = _y_part(inp["x"], inp["gamma"], inp["beta"], eps)
    else:
        y, f_y = _y_part.__wrapped__(inp["x"][r0:r1], inp["gamma"], inp["beta"], eps)
    if m is not None:
        y, f_y = y.masked_fill(m, 0.0), f_y.masked_fill(m, 0.0)
    ag = gamma.abs()
    s1, s2 = (dy @ gamma) / cols, (dyxh @ gamma) / cols          # mean_c g, mean_c g xh with g = dy gamma
    f_s1 = U * (ady @ ag) / cols
    f_s2 = ((U + a) * (adyxh @ ag) + b * (ady @ ag)) / cols      # u mean_c|g xh| + mean_c(|g| F_xh)
    del dyxh, adyxh
    core = dy * gamma
    core -= s1[:, None]
    core.addcmul_(xh, s2[:, None], value=-1.0)
    core *= rstd[:, None]
    # rstd (u (|g| + |s1| + |xh s2|) + F_s1 + |xh| F_s2 + |s2| F_xh) + |dx - dres| rho, the |xh| terms and the per-row terms collected
    f_dx = ady * (U * ag)
    f_dx.addcmul_(axh, (U * s2.abs() + f_s2 + s2.abs() * a)[:, None])
    f_dx += (U * s1.abs() + f_s1 + s2.abs() * b)[:, None]
    f_dx *= rstd[:, None]
    f_dx.addcmul_(core.abs(), rho[:, None])
    if "dres" in inp and inp["dres"] is not None:
        dres = inp["dres"][r0:r1].double()
        dx = core + dres
        f_dx += U * (dx.abs() + dres.abs())
    else:
        dx = core
        f_dx += U * dx.abs()
    out.update({"y": y, "mean": mean, "rstd": rstd, "dx": dx, "F": {"y": f_y, "mean": f_mean, "rstd": rstd * rho, "dx": f_dx}})
    return out


def bf16_half_ulp(ref):
    """what bf16 round-to-nearest of ref may be off by: 2^-9 times the power of two above |ref|"""
    _, e = torch.frexp(ref.abs())
    return torch.where(ref != 0, torch.ldexp(torch.ones_like(ref), e - 9), torch.zeros_like(ref))


def ratio(got, ref, bound):
    """worst |got - ref| / bound over the elements, on ref's device; where the bound is 0 the element has to be exact (inf
    otherwise); NaN -> inf."""
    got = torch.as_tensor(got).to(ref.device).double()
    err = (got - ref).abs()
    if not err.numel():
        return 0.0
    worst = torch.where(err == 0, err, err / bound).max().item()   # x / 0 = inf; a NaN anywhere makes the maximum NaN
    return math.inf if math.isnan(worst) else worst


def check(name, ref, out, depth, *, fp32_mode=False, k=None, limit=1.0, what="", rows=None, skip=()):
    """Every output present in `out` against `ref` (of `reference`), per element against K * F (see the top) -> {output: worst
    ratio}.  Raises AssertionError naming everything that is wrong.  Keys of out: y, dx [rows, cols] (bf16 values as f32, or fp32
    with fp32_mode); y_f32, dx_f32 (a bf16-mode restatement before its rounding: against K F alone); mean, rstd [rows]; dgamma,
    dbeta, dxsum [cols] (dxsum needs dx: its reference is the float64 column sum of that dx).  rows: a slice of the per-row outputs
    that ref covers; skip: outputs not to judge."""
    k = K if k is None else k
    F = ref.get("F")
    sl = slice(None) if rows is None else rows
    worst, wrong = {}, []

    def within(key, got, want, bound):
        worst[key] = ratio(got, want, bound)
        if not worst[key] <= limit:
            wrong.append(f"{key}: worst |err| / bound = {worst[key]:.3e} > {limit}")

    for key in ("y", "dx"):
        if key in out and key not in skip:
            within(key, out[key][sl], ref[key], (0.0 if fp32_mode else 1.0) * bf16_half_ulp(ref[key]) + k[key] * F[key])
        if key + "_f32" in out:
            within(key + "_f32", out[key + "_f32"][sl], ref[key], k[key] * F[key])
    for key in ("mean", "rstd"):
        if key in out:
            within(key, out[key][sl], ref[key], k[key] * F[key])
    for key in ("dgamma", "dbeta"):
        if key in out and out[key] is not None:
            within(key, out[key], ref[key], k[key] * ref["A_" + key] * math.sqrt(depth))
    if out.get("dxsum") is not None:
        dx64 = ref["dx_written"] if "dx_written" in ref else torch.as_tensor(out["dx"]).to(ref["dgamma"].device).double()
        within("dxsum", out["dxsum"], dx64.sum(0), k["dxsum"] * U * dx64.abs().sum(0) * math.sqrt(depth))
    assert not wrong, f"{what} {name}: " + "; ".join(wrong)
    return worst


# ------------------------------------------------------------------------------------------------ float32 restatements (CPU)
_F = torch.float32


def _fma(a, b, c):
    """fmaf: the product is exact in float64; one rounding to float32 (the double rounding through float64 is below 2^-29 relative)"""
    return (a.double() * b.double() + c.double()).float()


def _wave_sum(s):
    """wave_sum of common.h on lane states [rows, 64]: v += __shfl_xor(v, o) for o = 32 .. 1; every lane ends with the same bits"""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return s[:, 0]


def _pieces(t, cols):
    """[rows, cols] -> [rows, NQ, 64, 4] zero-padded: pass c, lane l, element e is column 4 (l + 64 c) + e"""
    nq = (cols + 255) // 256
    p = torch.zeros(t.shape[0], nq * 256, dtype=_F)
    p[:, :cols] = t
    return p.view(t.shape[0], nq, 64, 4)


def _lane_sum(v, fm=None):
    """per-lane sequential sum over the passes and the 4 elements: s += v, or s = fma(v, fm, s)"""
    s = torch.zeros(v.shape[0], 64, dtype=_F)
    for c in range(v.shape[1]):
        for e in range(4):
            s = s + v[:, c, :, e] if fm is None else _fma(v[:, c, :, e], fm[:, c, :, e], s)
    return s


def _drop_last_piece(v, cols):
    nch = cols >> 2
    v = v.clone()
    v[:, (nch - 1) // 64, (nch - 1) % 64, :] = 0
    return v


def _fold(partial, nchunks):
    """ln_bwd_reduce_kernel on partial [nblocks, cols] with gridDim.y = nchunks -> [nchunks, cols]: wave w of a chunk adds its rows
    b0 + w, b0 + w + 4, ... in order, then ((w0 + w1) + w2) + w3"""
    nb = partial.shape[0]
    per = (nb + nchunks - 1) // nchunks
    out = []
    for y in range(nchunks):
        b0, b1 = y * per, min(y * per + per, nb)
        acc = [torch.zeros(partial.shape[1], dtype=_F) for _ in range(4)]
        for b in range(b0, b1):
            acc[(b - b0) % 4] = acc[(b - b0) % 4] + partial[b]
        out.append(((acc[0] + acc[1]) + acc[2]) + acc[3])
    return torch.stack(out)


def _column_sums(rows, addend, factor=None, mut=None):
    """dgamma / dbeta / dx sums of ln_bwd_kernel + the reduce from the per-row addends [rows, cols]: a wave adds its rows w,
    w + nwaves, ... in order (acc += addend, or acc = fma(addend, factor, acc)), the 4 waves of a workgroup are added in order,
    then the fold"""
    grid = bwd_grid(rows)
    nw, cols = 4 * grid, addend.shape[1]

    def of_waves(t, it):
        p = torch.zeros(nw, cols, dtype=_F)
        p[:min(nw, rows - it * nw)] = t[it * nw:it * nw + nw]
        return p

    acc = torch.zeros(nw, cols, dtype=_F)
    for it in range(-(-rows // nw)):
        acc = acc + of_waves(addend, it) if factor is None else _fma(of_waves(addend, it), of_waves(factor, it), acc)
    part = acc.view(grid, 4, -1)
    part = ((part[:, 0] + part[:, 1]) + part[:, 2]) + part[:, 3]
    if grid <= 256:
        return _fold(part, 1)[0]
    mid = _fold(part, 16)
    if mut == "short last reduce chunk skipped":
        per = (grid + 15) // 16
        for y in range(16):
            if min(y * per + per, grid) - y * per < per:
                mid[y] = 0
    return _fold(mid, 1)[0]


_FWD_MUTANTS = ("row mean misses the last piece", "variance over cols - 1", "eps outside the square root", "one-pass variance",
                "gamma of piece ch - 64 in the last pass", "stale prefetch")


@functools.lru_cache(maxsize=1)
def _restate_fwd(rows, cols, offset, seed, mut, eps):
    """ln_fwd_kernel before the span: mean, rstd, xh = (x - mean) rstd as the kernel's lanes hold it ([rows, NQ, 64, 4], zero in
    the unused lanes) and y; the span cases of a shape share it"""
    inp = _inputs(rows, cols, offset, seed, False)
    nch, nq = cols >> 2, (cols + 255) // 256
    act = (torch.arange(64)[None, :] + 64 * torch.arange(nq)[:, None] < nch)[None, :, :, None]   # [1, NQ, 64, 1]
    x = inp["x"]
    if mut == "stale prefetch":   # the second row of a wave computed from the registers of its first
        x = x.clone()
        x[FWD_WAVES_MAX:] = inp["x"][:max(rows - FWD_WAVES_MAX, 0)]
    v = _pieces(x, cols)
    gm = _pieces(inp["gamma"][None], cols)
    if mut == "gamma of piece ch - 64 in the last pass" and nq >= 2:
        gm = gm.clone()
        gm[:, nq - 1] = gm[:, nq - 2]
    inv = torch.tensor(1.0, dtype=_F) / torch.tensor(float(cols), dtype=_F)
    s = _lane_sum(_drop_last_piece(v, cols) if mut == "row mean misses the last piece" else v)
    mu = _wave_sum(s) * inv
    d = torch.where(act, v - mu[:, None, None, None], torch.zeros((), dtype=_F))
    eps32 = torch.tensor(eps, dtype=_F)
    if mut == "one-pass variance":
        rs = torch.rsqrt(_fma(_wave_sum(_lane_sum(v, v)), inv, -(mu * mu)).clamp_min(0.0) + eps32)
    elif mut == "eps outside the square root":
        rs = 1 / ((_wave_sum(_lane_sum(d, d)) * inv).sqrt() + eps32)
    else:
        over = 1 / torch.tensor(float(cols - 1), dtype=_F) if mut == "variance over cols - 1" else inv
        rs = torch.rsqrt(_fma(_wave_sum(_lane_sum(d, d)), over, eps32))
    xh = d * rs[:, None, None, None]
    return mu, rs, xh, _fma(xh, gm, _pieces(inp["beta"][None], cols)), gm, act, inv


def restate_bf16(case, mut=None, eps=EPS):
    """wft_layernorm_fwd + wft_layernorm_bwd (dx column sums wanted) in CPU float32, in the kernels' order; mut: one of ALL_MUTANTS"""
    assert mut is None or mut in ALL_MUTANTS
    inp = inputs(case)
    rows, cols = case.rows, case.cols
    mu, rs, xh, y, gm, act, inv = _restate_fwd(rows, cols, case.offset, case.seed, mut if mut in _FWD_MUTANTS else None, eps)
    m = masked(rows, cols, case.mask, mut=mut)
    mp = None if m is None else _pieces(m.float(), cols) > 0
    if mp is not None:
        y = torch.where(mp, torch.zeros((), dtype=_F), y)
    y = y.reshape(rows, -1)[:, :cols]
    if mut == "stale prefetch":
        xb = inp["x"].clone()
        xb[4 * bwd_grid(rows):] = inp["x"][:max(rows - 4 * bwd_grid(rows), 0)]
        xh = torch.where(act, (_pieces(xb, cols) - mu[:, None, None, None]) * rs[:, None, None, None], torch.zeros((), dtype=_F))

    # ---- backward (mean and rstd as the forward wrote them)
    dyp = _pieces(inp["dy"], cols)
    dz = dyp if mp is None else torch.where(mp, torch.zeros((), dtype=_F), dyp)
    g = dz * gm
    gs = dyp * gm if mut == "masked dy not zeroed in s1 and s2" else g
    if mut == "s1 and s2 sums miss the last piece":
        gs = _drop_last_piece(gs, cols)
    s1 = (_wave_sum(_lane_sum(gs)) * inv)[:, None, None, None]
    s2 = (_wave_sum(_lane_sum(gs, xh)) * inv)[:, None, None, None]
    if mut == "s1 term dropped":
        s1 = torch.zeros_like(s1)
    if mut == "s2 term dropped":
        s2 = torch.zeros_like(s2)
    rv = torch.zeros_like(dyp) if mut == "dres dropped" else _pieces(inp["dres"], cols)
    dx32 = _fma(rs[:, None, None, None].expand_as(g), _fma(-xh, s2, g - s1), rv).reshape(rows, -1)[:, :cols]
    dx = _bfq(dx32)
    dgd = dz
    if mut == "masked columns contribute to dgamma" and case.mask is not None:
        rpb, t0, t1, _, _ = case.mask
        trow = _pieces(masked(rows, cols, (rpb, t0, t1, 0, 0)).float(), cols) > 0
        dgd = torch.where(trow, torch.zeros((), dtype=_F), dyp)
    dgd, dbd = dgd.reshape(rows, -1)[:, :cols].clone(), dz.reshape(rows, -1)[:, :cols].clone()
    if mut == "dgamma fold loses the last row":
        dgd[rows - 1] = 0
    if mut == "dbeta fold loses row 0":
        dbd[0] = 0
    xh2 = xh.reshape(rows, -1)[:, :cols]
    dsrc = dx32 if mut == "dxsum summed before the bf16 rounding" else dx

    dgamma = _column_sums(rows, dgd, xh2, mut=mut)
    dbeta = _column_sums(rows, dbd, mut=mut)
    dxsum = _column_sums(rows, dsrc, mut=mut)
    return {"y": _bfq(y), "y_f32": y, "mean": mu, "rstd": rs, "dx": dx, "dx_f32": dx32, "dgamma": dgamma, "dbeta": dbeta, "dxsum": dxsum}


def restate_f32(case, fp32_values=True, eps=EPS):
    """wft_layernorm_fwd_f32 + wft_layernorm_bwd_f32 in CPU float32: lane l owns columns l, l + 64, ...; butterfly sums, true
    divisions by cols, 1 / sqrtf; dgamma / dbeta one thread per column, rows in order"""
    inp = inputs(case, fp32_values)
    rows, cols = case.rows, case.cols
    P = (cols + 63) // 64

    def lanes(t):
        p = torch.zeros(t.shape[0], P * 64, dtype=_F)
        p[:, :cols] = t
        return p.view(t.shape[0], P, 64)

    def lane_sum(a, b=None):
        s = torch.zeros(a.shape[0], 64, dtype=_F)
        for p in range(P):
            s = s + a[:, p] if b is None else _fma(a[:, p], b[:, p], s)
        return s

    act = lanes(torch.ones(1, cols)) > 0
    fc = torch.tensor(float(cols), dtype=_F)
    x, gm, bt = lanes(inp["x"]), lanes(inp["gamma"][None]), lanes(inp["beta"][None])
    mu = _wave_sum(lane_sum(x)) / fc
    d = torch.where(act, x - mu[:, None, None], torch.zeros((), dtype=_F))
    rs = 1 / torch.sqrt(_wave_sum(lane_sum(d, d)) / fc + torch.tensor(eps, dtype=_F))
    m = masked(rows, cols, case.mask)
    mp = None if m is None else lanes(m.float()) > 0
    xh = d * rs[:, None, None]
    y = _fma(xh, gm, bt)
    dy = lanes(inp["dy"])
    g = dy * gm
    if mp is not None:
        y, g = torch.where(mp, torch.zeros((), dtype=_F), y), torch.where(mp, torch.zeros((), dtype=_F), g)
    s1 = (_wave_sum(lane_sum(g)) / fc)[:, None, None]
    s2 = (_wave_sum(lane_sum(g, xh)) / fc)[:, None, None]
    dx = rs[:, None, None] * _fma(-xh, s2, g - s1)
    flat = lambda t: t.reshape(rows, -1)[:, :cols]   # noqa: E731
    dg, db = torch.zeros(cols, dtype=_F), torch.zeros(cols, dtype=_F)
    dyf, df = inp["dy"], flat(d)
    for r in range(rows):
        keep = torch.ones(cols, dtype=torch.bool) if m is None else ~m[r]
        dg = torch.where(keep, _fma(dyf[r] * df[r], rs[r].expand(cols), dg), dg)
        db = torch.where(keep, db + dyf[r], db)
    return {"y": flat(y), "mean": mu, "rstd": rs, "dx": flat(dx), "dgamma": dg, "dbeta": db}
