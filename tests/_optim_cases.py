"""Cases, float64 references, per-element bounds and float32 restatements for the optimizer kernels of csrc/optim.hip:
wft_mt_adamw / wft_adamw_step, wft_mt_sumsq_f32 / wft_sumsq_f32, wft_muon_momentum_mt, wft_muon_prepare, wft_muon_apply_mt.  Shared
by tests/test_optim_host.py (CPU: the bounds accept the kernels' arithmetic and reject every listed mutant of it) and
tests/test_optim_gpu.py (the kernels themselves, through the C ABI, under the same checkers).

Conventions.  Scalars: the ABI takes floats, so every reference uses the float32-rounded lr, betas, eps, weight decay, bias
corrections, max_norm and scale (and the float32 1e-6 / 1e-7 of the source), promoted to float64; 1 - beta is formed from the
rounded beta.  Buffers: every array a kernel reads or writes is carved from a flat buffer (`Layout`) with at least 64 sentinel
elements (-12345.0f; bf16: the bits 0xC2F7) in front of, between and behind the tensors; outputs are pre-filled with the sentinel;
the checkers ask that every sentinel is unchanged (a bound of 0) and the tests that every const input keeps its bits.  Values:
element i of a tensor is of kind i % 8 (the 300 tiny tensors of table B: (i + 3 t) % 8, so that tensors of 1 to 7 elements see
every kind), so that neighbours differ by orders of magnitude; no NaN or Inf goes in.

AdamW (`adam_cases()`): table A = 7 tensors of 3, 8, 1001, 65536, 65537, 70001, 2 x 65536 + 5 elements (11 chunks), tensors 0, 1,
2 and 4 with exactly one of p, g, m, v starting 4 or 8 bytes off a 16-byte boundary; table B = 300 tensors of 1 + t % 7 elements,
all four arrays of tensor t starting 4 (t % 4) bytes off; x ADAM_HP (five hyper-parameter sets) x CLIPS (five).  Kinds:
0 ordinary, 1 g = 0, 2 g = m = v = 0, 3 g ~ 1e-7 with m = v = 0 (eps rules the denominator), 4 g ~ 1e3, 5 v ~ 1e4 with m small,
6 p = 0, 7 p ~ 1e3 with tiny g and m (the update is below half an ulp of p).  Reference, with gs = min(1, max_norm / (sqrt(sumsq)
+ 1e-6)), g' = g gs, decay = 1 - lr wd: m' = b1 m + (1 - b1) g', v' = b2 v + (1 - b2) g'^2,
p' = p decay - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps).  Bound forms, u = 2^-24, rg = 3u where gs < 1 came from sumsq, else 0:
  F_g'  = |g'| (rg + u)                       (u alone for wft_adamw_step's gscale; 0 when the gradient is not scaled)
  F_m   = u (|b1 m| + 2 |(1 - b1) g'| + |m'|) + (1 - b1) F_g'
  F_v   = u (|b2 v| + 3 (1 - b2) g'^2 + v') + 2 (1 - b2) |g'| F_g'
  F_den = (u sqrt(v') + F_v / (2 sqrt(v'))) / sqrt(bc2) + 3u sqrt(v' / bc2) + u den            (F_v / sqrt(v') = 0 where v' = 0)
  F_p   = |p| u (lr wd + decay) + u |p decay| + |t| (3u + F_den / den) + (lr / bc1) F_m / den + u |p'|,   t = (lr / bc1) m' / den
Sums of squares: partial[c] against the float64 sum of its chunk, F = u sum sqrt(depth), depth = ceil(cnt / 256) + 6 + 4 (the
per-thread strided adds, six butterfly levels, four waves); the total against the float64 sum of the partials the kernel wrote,
F = u sum|partial| sqrt(ceil(total / 256) + 10); wft_sumsq_f32 adds its grid size to the depth (one atomic per workgroup).
Momentum: b' = beta b + (1 - beta) g', u = nesterov ? beta b' + (1 - beta) g' : b' (real numbers); F is the larger of the bounds
of torch's two lerp forms s + w (e - s) and e - (e - s)(1 - w), with d = g' - b, d2 = b' - g':
  F_b' = max(w F_g' + 2u w |d| + u |b'|,  F_g' + beta (F_g' + 2u |d|) + u |b'|),   w = 1 - beta
  F_u  = max(F_g' + beta (F_d2 + u |d2|) + u |u|,  F_b' + w (F_d2 + u |d2|) + u |u|),   F_d2 = F_b' + F_g' + u |d2|
Prepare: q = U / (bf16(sqrt(s)) + 1e-7) in float64; inside [R, C] half an ulp of bf16 at q plus 4u |q| (derived: one fp32 division of
at most 2.5 ulp, one bf16 rounding); the pad exactly 0; Xt = X^T bit for bit.  Apply: F = u (|p decay| + |a o|), a = lr scale.

The constants K are not chosen: the restatements below redo each kernel's arithmetic in torch CPU float32, in the kernels' order
(chunks found by mt_find, vector part and tail, thread t owning elements t, t + 256, ..., xor-butterfly wave sums, four waves in
order), once with every product rounded (form 0) and with a * b + c contracted to an fma either way round (forms 1, 2);
tests/test_optim_host.py measures max |restatement - reference| / F over all cases and forms, and K is 4 x that (the GPU's sqrtf,
rsqrtf and division are looser than the CPU's), rounded up to a power of two.  Measured (seeds fixed per table):

  output    worst ratio of the restatement   4 x worst   K
  m         0.951                            3.80        4
  v         0.987                            3.95        4
  p         0.717                            2.87        4
  partial   0.622                            2.49        4
  total     0.362                            1.45        2
  buf       0.351                            1.40        2
  u         0.487                            1.95        2
  apply     2.453                            9.81        16
"""
import dataclasses
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
CHUNK = 65536          # include/wft.h WFT_MT_CHUNK
GUARD = 64
SENT = -12345.0
SENT_BF16_BITS = 0xC2F7 - 0x10000   # as int16
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
K = {"m": 4.0, "v": 4.0, "p": 4.0, "partial": 4.0, "total": 2.0, "buf": 2.0, "u": 2.0, "apply": 16.0}
FORMS = (0, 1, 2)

MUTANTS = {
    "adamw": ("eps scaled by the bias correction", "bias_corr2 applied without the square root", "decay applied after the update",
              "decay as 1 - wd", "v updated with (1 - b2) g", "coefficient not capped at 1", "coefficient from sumsq", "+ 1e-6 dropped",
              "v taking the unscaled g", "vector tail skipped", "last chunk at the full MT_CHUNK count", "mt_find with < for <="),
    "sumsq": ("tail lost", "unaligned branch starts one element late", "final sum over the first 256 partials",
              "NULL row's partial left unwritten"),
    "momentum": ("lerp weight beta for 1 - beta", "nesterov lerp with the ends swapped", "buf written with u", "g not overwritten",
                 "clip applied to U but not to buf", "partial from the fp32 u"),
    "prepare": ("norm not rounded to bf16", "+ 1e-7 dropped", "pad not written", "Xt not transposed for a tall parameter",
                "square treated as tall", "partial indexed without t chunks"),
    "apply": ("ldo ignored", "stride_o taken as rows cols", "decay missing", "scale folded into the decay"),
}


def f32(x):
    """the float32-rounded value of a Python number, as a Python float (exact in float64)"""
    return float(np.float32(x))


def sentinel(n, dtype=F32):
    if dtype == BF16:
        return torch.full((n,), SENT_BF16_BITS, dtype=torch.int16).view(BF16)
    return torch.full((n,), SENT, dtype=dtype)


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


class Layout:
    """tensors of `numels` elements carved from one flat buffer: tensor t starts `mis[t]` elements past a multiple of `align`
    elements (the buffer itself starts on one), with at least GUARD sentinel elements on each side of every tensor"""

    def __init__(self, numels, mis=None, align=4, order=None):
        self.numels = tuple(int(n) for n in numels)
        mis = (0,) * len(self.numels) if mis is None else tuple(mis)
        order = range(len(self.numels)) if order is None else order
        starts, pos = [0] * len(self.numels), 0
        for t in order:
            pos = -(-(pos + GUARD) // align) * align + mis[t]
            starts[t] = pos
            pos += self.numels[t]
        self.starts, self.mis, self.align = tuple(starts), mis, align
        self.length = -(-(pos + GUARD) // align) * align
        self.total = sum(self.numels)

    @functools.cached_property
    def index(self):
        return torch.cat([torch.arange(s, s + n) for s, n in zip(self.starts, self.numels)])

    @functools.cached_property
    def offsets(self):
        return tuple(np.cumsum((0,) + self.numels).tolist())

    def fill(self, values=None, dtype=F32):
        """a buffer of sentinels with `values` (the tensors' elements, concatenated) in place"""
        buf = sentinel(self.length, dtype)
        if values is not None:
            buf[self.index] = values.to(dtype)
        return buf

    def gather(self, buf):
        return buf[self.index.to(buf.device)]

    def guards_intact(self, buf):
        keep = torch.ones(self.length, dtype=torch.bool)
        keep[self.index] = False
        b = bits(buf.cpu())
        return bool((b[keep] == bits(sentinel(1, buf.dtype))).all())


def element_kinds(numels, per_tensor_shift=0):
    ei = torch.cat([torch.arange(n) for n in numels])
    ti = torch.cat([torch.full((n,), t) for t, n in enumerate(numels)])
    return (ei + per_tensor_shift * ti) % 8


def bf16_half_ulp(ref):
    _, e = torch.frexp(ref.abs())
    return torch.where(ref != 0, torch.ldexp(torch.ones_like(ref), e - 9), torch.zeros_like(ref))


def ratio(got, ref, bound):
    """worst |got - ref| / bound; where the bound is 0 the element has to be exact (inf otherwise); NaN -> inf"""
    got = torch.as_tensor(got).to(ref.device).double()
    err = (got - ref).abs()
    if not err.numel():
        return 0.0
    worst = torch.where(err == 0, err, err / bound).max().item()
    return math.inf if math.isnan(worst) else worst


class Checker:
    """collects the worst |err| / bound per output and everything that is wrong; `done()` raises naming all of it"""

    def __init__(self, name, k=None, limit=1.0):
        self.name, self.k, self.limit = name, K if k is None else k, limit
        self.worst, self.wrong = {}, []

    def within(self, key, got, ref, F, kname=None):
        r = ratio(got, ref, self.k[kname or key] * F if (kname or key) in self.k else F)
        self.worst[key] = max(self.worst.get(key, 0.0), r)
        if not r <= self.limit:
            self.wrong.append(f"{key}: worst |err| / bound = {r:.3e} > {self.limit}")

    def true(self, cond, what):
        if not cond:
            self.wrong.append(what)

    def done(self):
        assert not self.wrong, f"{self.name}: " + "; ".join(self.wrong)
        return self.worst


def fma(a, b, c):
    """fmaf: the product is exact in float64; one rounding to float32 (the double rounding through float64 is below 2^-29 relative)"""
    a, b, c = (x if torch.is_tensor(x) else torch.tensor(x, dtype=F64) for x in (a, b, c))
    return (a.double() * b.double() + c.double()).float()


def wave_sum(s):
    """wave_sum of common.h on lane states [..., 64]"""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ o]
    return s[..., 0]


def block_sum_256(s):
    """block_sum_256 on thread states [..., 256] (float32): four wave sums, ((w0 + w1) + w2) + w3"""
    w = wave_sum(s.reshape(*s.shape[:-1], 4, 64))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def mt_find(chunk_start, n, chunk, strict=False):
    lo, hi = 0, n
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if (chunk_start[mid] < chunk) if strict else (chunk_start[mid] <= chunk):
            lo = mid
        else:
            hi = mid
    return lo


def chunk_starts(numels):
    out, tot = [], 0
    for ne in numels:
        out.append(tot)
        tot += -(-ne // CHUNK)
    return out + [tot]


def depth(cnt, extra=0):
    return -(-cnt // 256) + 6 + 4 + extra


# ================================================================================================ AdamW
A_NUMELS = (3, 8, 1001, 65536, 65537, 70001, 2 * 65536 + 5)
A_MIS = {"p": (1, 0, 0, 0, 0, 0, 0), "g": (0, 2, 0, 0, 0, 0, 0), "m": (0, 0, 1, 0, 0, 0, 0), "v": (0, 0, 0, 0, 2, 0, 0)}
B_NUMELS = tuple(1 + i % 7 for i in range(300))
B_MIS = tuple(t % 4 for t in range(300))
# (lr, beta1, beta2, eps, weight_decay, step)
ADAM_HP = ((1e-2, 0.9, 0.98, 1e-6, 0.1, 1), (1e-2, 0.9, 0.98, 1e-6, 0.1, 1000), (1e-2, 0.9, 0.98, 1e-6, 0.0, 1),
           (1e-2, 0.9, 0.98, 1e-6, 0.0, 1000), (3e-4, 0.9, 0.95, 1e-10, 0.0, 7))
# (sumsq, max_norm) or None: no clip; coefficient 0.370; 2 (capped); sumsq = 0 (capped); sumsq 1e-10 (+ 1e-6 is 10 % of the norm: 0.5)
CLIPS = (None, (7.3, 1.0), (0.25, 1.0), (0.0, 1.0), (1e-10, 5.5e-6))


@dataclasses.dataclass(frozen=True)
class AdamCase:
    table: str
    hp: int
    clip: int

    @property
    def name(self):
        return f"table {self.table}, hp {self.hp}, clip {self.clip}"


@functools.lru_cache(maxsize=None)
def adam_cases():
    return tuple(AdamCase(t, h, c) for t in "AB" for h in range(len(ADAM_HP)) for c in range(len(CLIPS)))


@functools.lru_cache(maxsize=None)
def adam_table(table):
    """-> (numels, {array: Layout})"""
    if table == "A":
        return A_NUMELS, {a: Layout(A_NUMELS, A_MIS[a]) for a in "pgmv"}
    return B_NUMELS, {a: Layout(B_NUMELS, B_MIS) for a in "pgmv"}


def adam_values(kind, gen):
    """p, g, m, v (float32, one element per entry of `kind`) of the kinds of the top"""
    n = kind.numel()
    rn = lambda: torch.randn(n, generator=gen)   # noqa: E731
    p, g, m, v = rn(), rn(), rn(), 0.01 * torch.rand(n, generator=gen)
    zero = torch.zeros(n)
    g = torch.where(kind == 1, zero, g)
    g = torch.where(kind == 2, zero, g)
    g = torch.where(kind == 3, 1e-7 * rn(), g)
    g = torch.where(kind == 4, 1e3 * rn(), g)
    g = torch.where(kind == 7, 1e-6 * rn(), g)
    m = torch.where((kind == 2) | (kind == 3), zero, m)
    m = torch.where(kind == 5, 1e-3 * rn(), m)
    m = torch.where(kind == 7, 1e-6 * rn(), m)
    v = torch.where((kind == 2) | (kind == 3), zero, v)
    v = torch.where(kind == 5, 1e4 * (0.5 + torch.rand(n, generator=gen)), v)
    v = torch.where(kind == 7, 0.005 + 0.005 * torch.rand(n, generator=gen), v)
    p = torch.where(kind == 6, zero, p)
    p = torch.where(kind == 7, 1e3 * (1 + torch.rand(n, generator=gen)) * torch.sign(rn()), p)
    return {"p": p, "g": g, "m": m, "v": v}


@functools.lru_cache(maxsize=None)
def adam_inputs(table):
    """the table's operands, concatenated over its tensors (float32); shared, nobody writes to them"""
    numels, _ = adam_table(table)
    kind = element_kinds(numels, 3 if table == "B" else 0)
    d = adam_values(kind, torch.Generator().manual_seed(11 if table == "A" else 12))
    d["kind"] = kind
    return d


def adam_scalars(hp):
    """float32-rounded (lr, b1, b2, eps, wd, bc1, bc2) of a hyper-parameter set, as Python floats"""
    lr, b1, b2, eps, wd, step = hp
    return tuple(f32(x) for x in (lr, b1, b2, eps, wd, 1 - b1 ** step, 1 - b2 ** step))


def clip_coefficient(clip):
    """-> (gs, rg) of the reference: the float64 coefficient from the float32-rounded sumsq and max_norm, capped at 1, and the
    relative error 3u allowed to it (sqrtf, the add, the division) where it is below 1"""
    if clip is None:
        return 1.0, 0.0
    coef = f32(clip[1]) / (math.sqrt(f32(clip[0])) + f32(1e-6))
    return (coef, 3 * U) if coef < 1 else (1.0, 0.0)


def adam_reference(inp, scalars, gs=1.0, rg=0.0, scaled=None):
    """float64 closed forms and bound forms F of one AdamW step on concatenated operands; scaled: whether the kernel multiplies the
    gradient at all (mt_adamw always does: gs is 1.f without a clip)"""
    lr, b1, b2, eps, wd, bc1, bc2 = scalars
    p, g, m, v = (inp[k].double() for k in "pgmv")
    gg = g * gs
    f_g = gg.abs() * (rg + (U if (scaled if scaled is not None else gs != 1.0) else 0.0))
    decay = 1 - lr * wd
    m2 = b1 * m + (1 - b1) * gg
    v2 = b2 * v + (1 - b2) * gg * gg
    sq = v2.sqrt()
    den = sq / math.sqrt(bc2) + eps
    step = lr / bc1
    t = step * m2 / den
    p2 = p * decay - t
    f_m = U * ((b1 * m).abs() + 2 * ((1 - b1) * gg).abs() + m2.abs()) + (1 - b1) * f_g
    f_v = U * (b2 * v + 3 * (1 - b2) * gg * gg + v2) + 2 * (1 - b2) * gg.abs() * f_g
    f_sq = U * sq + torch.where(v2 > 0, f_v / (2 * sq), torch.zeros_like(sq))
    f_den = f_sq / math.sqrt(bc2) + 3 * U * sq / math.sqrt(bc2) + U * den
    f_p = p.abs() * U * (lr * wd + decay) + U * (p * decay).abs() + t.abs() * (3 * U + f_den / den) + step * f_m / den + U * p2.abs()
    return {"m": m2, "v": v2, "p": p2, "F": {"m": f_m, "v": f_v, "p": f_p}}


def adam_update(p, g, m, v, scalars, gs, form=0, mut=None, gs_raw=None):
    """the `upd` lambda of mt_adamw_kernel (and the loop body of adamw_kernel) on float32 tensors -> p, m, v"""
    lr, b1, b2, eps, wd, bc1, bc2 = (np.float32(x) for x in scalars)
    one = np.float32(1)
    step, rbc2 = float(lr / bc1), float(one / np.sqrt(bc2))
    decay = float(one - lr * wd) if form == 0 else f32(1 - float(lr) * float(wd))
    if mut == "decay as 1 - wd":
        decay = float(one - wd)
    omb1, omb2 = float(one - b1), float(one - b2)
    b1, b2, eps = float(b1), float(b2), float(eps)
    gg = g * gs
    gv = g if mut == "v taking the unscaled g" else gg
    if mut != "decay applied after the update":
        p = p * decay
    m = b1 * m + omb1 * gg if form == 0 else fma(b1, m, omb1 * gg) if form == 1 else fma(omb1, gg, b1 * m)
    if mut == "v updated with (1 - b2) g":
        v = b2 * v + omb2 * gv
    else:
        v = b2 * v + omb2 * gv * gv if form == 0 else fma(b2, v, omb2 * gv * gv) if form == 1 else fma(omb2 * gv, gv, b2 * v)
    if mut == "eps scaled by the bias correction":
        den = (v.sqrt() + eps) * rbc2
    elif mut == "bias_corr2 applied without the square root":
        den = v.sqrt() * (rbc2 * rbc2) + eps
    else:
        den = v.sqrt() * rbc2 + eps
    p = p - step * m / den
    if mut == "decay applied after the update":
        p = p * decay
    return p, m, v


def clip_gs(clip, mut=None):
    """gs of the kernels in float32 from (sumsq, max_norm)"""
    if clip is None:
        return 1.0
    s, mx = np.float32(clip[0]), np.float32(clip[1])
    root = s if mut == "coefficient from sumsq" else np.sqrt(s)
    with np.errstate(divide="ignore"):
        coef = mx / (root if mut == "+ 1e-6 dropped" else root + np.float32(1e-6))
    return float(coef) if (coef < 1 or mut == "coefficient not capped at 1") else 1.0


def restate_mt_adamw(case, form=0, mut=None):
    """wft_mt_adamw in CPU float32 on guarded buffers, chunk by chunk -> {p, g, m, v: the buffers after the launch}"""
    numels, lay = adam_table(case.table)
    inp = adam_inputs(case.table)
    buf = {a: lay[a].fill(inp[a]) for a in "pgmv"}
    scalars = adam_scalars(ADAM_HP[case.hp])
    gs = clip_gs(CLIPS[case.clip], mut)
    cs = chunk_starts(numels)
    n = len(numels)
    for c in range(cs[-1]):
        t = mt_find(cs, n, c, strict=mut == "mt_find with < for <=")
        off = (c - cs[t]) * CHUNK
        cnt = min(numels[t] - off, CHUNK)
        if mut == "last chunk at the full MT_CHUNK count":
            cnt = CHUNK
        if cnt <= 0:
            continue
        st = {a: lay[a].starts[t] + off for a in "pgmv"}
        al = all(s % 4 == 0 for s in st.values())
        if mut == "vector tail skipped" and al:
            cnt = cnt & ~3
        cnt = min(cnt, *(lay[a].length - st[a] for a in "pgmv"))   # (a mutant past the tensor: no further than the buffers reach)
        sl = {a: slice(st[a], st[a] + cnt) for a in "pgmv"}
        buf["p"][sl["p"]], buf["m"][sl["m"]], buf["v"][sl["v"]] = adam_update(
            buf["p"][sl["p"]], buf["g"][sl["g"]], buf["m"][sl["m"]], buf["v"][sl["v"]], scalars, gs, form, mut)
    return buf


def decay_candidates(scalars):
    """fl32(1 - fl32(lr wd)) and fl32(1 - lr wd): the compiler may or may not contract"""
    lr, wd = np.float32(scalars[0]), np.float32(scalars[4])
    return float(np.float32(1) - lr * wd), f32(1 - float(lr) * float(wd))


def check_adamw(name, lay, inp, ref, out, scalars, k=None, limit=1.0):
    """p, m, v buffers of `out` per element against K F; the sentinels and the const gradient unchanged; kind 2 exactly"""
    ck = Checker(name, k, limit)
    got = {}
    for a in "pmv":
        got[a] = lay[a].gather(out[a].cpu())
        ck.within(a, got[a], ref[a], ref["F"][a])
        ck.true(lay[a].guards_intact(out[a]), f"{a}: a sentinel was overwritten")
    ck.true(torch.equal(bits(out["g"].cpu()), bits(lay["g"].fill(inp["g"]))), "g: the const gradient buffer changed")
    k2 = inp["kind"] == 2
    if k2.any():
        ck.true(bool((bits(got["m"])[k2] == 0).all() and (bits(got["v"])[k2] == 0).all()), "kind 2: m or v is not +0")
        cands = [(inp["p"][k2].double() * d).float() for d in decay_candidates(scalars)]
        ck.true(any(torch.equal(bits(got["p"][k2]), bits(c)) for c in cands), "kind 2: p is not fl32(p decay)")
        if scalars[4] == 0:
            ck.true(torch.equal(bits(got["p"][k2]), bits(inp["p"][k2])), "kind 2, weight_decay 0: p changed")
    return ck.done()


def check_adam_case(case, out, k=None, limit=1.0):
    _, lay = adam_table(case.table)
    return check_adamw(case.name, lay, adam_inputs(case.table), _adam_ref(case.table, case.hp, case.clip), out,
                       adam_scalars(ADAM_HP[case.hp]), k, limit)


@functools.lru_cache(maxsize=4)
def _adam_ref(table, hp, clip):
    gs, rg = clip_coefficient(CLIPS[clip])
    return adam_reference(adam_inputs(table), adam_scalars(ADAM_HP[hp]), gs, rg)


# ================================================================================================ sums of squares
SUMSQ_NULL = {"A": (3, 5), "B": ()}                 # tensors without a gradient (address 0)
SUMSQ_MIS = {"A": (0, 2, 1, 0, 0, 0, 0), "B": B_MIS}
SPIKE = (6, 1)                                      # table A: chunk 1 of tensor 6 holds a single 1e4 among values of 1e-4


@functools.lru_cache(maxsize=None)
def sumsq_table(table):
    numels = A_NUMELS if table == "A" else B_NUMELS
    return numels, Layout(numels, SUMSQ_MIS[table])


@functools.lru_cache(maxsize=None)
def sumsq_inputs(table):
    numels, lay = sumsq_table(table)
    g = adam_inputs(table)["g"].clone()
    if table == "A":
        t, c = SPIKE
        o = lay.offsets[t] + c * CHUNK
        g[o:o + CHUNK] = 1e-4
        g[o + 4099] = 1e4
    return g


def chunk_list(numels):
    """(tensor, offset, count) of every chunk, in launch order"""
    return [(t, o, min(CHUNK, n - o)) for t, n in enumerate(numels) for o in range(0, n, CHUNK)]


def sumsq_reference(table):
    """-> (float64 sum of squares per chunk, 0 for the NULL rows; the bound forms F)"""
    numels, lay = sumsq_table(table)
    g = sumsq_inputs(table).double()
    s, f = [], []
    for t, o, cnt in chunk_list(numels):
        x = g[lay.offsets[t] + o:lay.offsets[t] + o + cnt]
        v = 0.0 if t in SUMSQ_NULL[table] else float((x * x).sum())
        s.append(v)
        f.append(U * v * math.sqrt(depth(cnt)))
    return torch.tensor(s, dtype=F64), torch.tensor(f, dtype=F64)


def _thread_sums(x, vec, form, late=False):
    """the per-thread accumulators [256] of one chunk x (float32): vec -> the f32x4 loop over cnt >> 2 vectors and the scalar tail;
    else the scalar loop"""
    cnt = x.numel()
    s = torch.zeros(256)

    def scalar(vals, s, first=0):
        n = vals.numel()
        pad = torch.zeros(-(-max(n, 1) // 256) * 256)
        pad[:n] = vals
        if first:
            pad[:first] = 0
        for row in pad.view(-1, 256):
            s = fma(row, row, s) if form else s + row * row
        return s

    if not vec:
        return scalar(x, s, 1 if late else 0)
    nv = cnt >> 2
    pad = torch.zeros(-(-max(nv, 1) // 256) * 256, 4)
    pad[:nv] = x[:nv * 4].view(nv, 4)
    for it in pad.view(-1, 256, 4):
        if form:
            q = fma(it[:, 3], it[:, 3], fma(it[:, 2], it[:, 2], fma(it[:, 1], it[:, 1], it[:, 0] * it[:, 0])))
        else:
            q = ((it[:, 0] * it[:, 0] + it[:, 1] * it[:, 1]) + it[:, 2] * it[:, 2]) + it[:, 3] * it[:, 3]
        s = s + q
    return scalar(x[nv * 4:], s)


def final_sum(partial, count=None):
    n = partial.numel() if count is None else min(count, partial.numel())
    pad = torch.zeros(-(-n // 256) * 256)
    pad[:n] = partial[:n]
    s = torch.zeros(256)
    for row in pad.view(-1, 256):
        s = s + row
    return block_sum_256(s)


def restate_mt_sumsq(table, form=0, mut=None):
    """wft_mt_sumsq_f32 in CPU float32 -> {partial: guarded buffer, total: [1]}"""
    numels, lay = sumsq_table(table)
    g = sumsq_inputs(table)
    chunks = chunk_list(numels)
    play = Layout((len(chunks),))
    partial = play.fill()
    for c, (t, o, cnt) in enumerate(chunks):
        if t in SUMSQ_NULL[table]:
            if mut != "NULL row's partial left unwritten":
                partial[play.starts[0] + c] = 0.0
            continue
        x = g[lay.offsets[t] + o:lay.offsets[t] + o + cnt]
        vec = (lay.starts[t] + o) % 4 == 0
        if mut == "tail lost" and vec:
            x = x[:cnt & ~3]
        s = _thread_sums(x, vec, form, late=mut == "unaligned branch starts one element late")
        partial[play.starts[0] + c] = block_sum_256(s)
    written = play.gather(partial)
    total = final_sum(written, 256 if mut == "final sum over the first 256 partials" else None)
    return {"partial": partial, "total": total.reshape(1)}


def check_mt_sumsq(table, out, k=None, limit=1.0):
    numels, _ = sumsq_table(table)
    chunks = chunk_list(numels)
    play = Layout((len(chunks),))
    ref, f = sumsq_reference(table)
    ck = Checker(f"sums of squares, table {table}", k, limit)
    got = play.gather(out["partial"].cpu())
    ck.within("partial", got, ref, f)
    null = torch.tensor([t in SUMSQ_NULL[table] for t, _, _ in chunks])
    ck.true(bool((bits(got)[null] == 0).all()), "the partial of a NULL row is not +0")
    ck.true(play.guards_intact(out["partial"]), "partial: a sentinel was overwritten")
    g64 = got.double()
    ck.within("total", out["total"].cpu(), g64.sum().reshape(1), U * g64.abs().sum().reshape(1) * math.sqrt(depth(len(chunks))))
    return ck.done()


# ================================================================================================ Muon: momentum
MOM_SHAPES = ((16, 320), (257, 255), (256, 256), (300, 300))
MOM_BETA = 0.95
MOM_CLIP = (7.3, 1.0)


@dataclasses.dataclass(frozen=True)
class MomCase:
    rows: int
    cols: int
    nesterov: int
    clip: bool

    @property
    def name(self):
        return f"{self.rows}x{self.cols}, nesterov {self.nesterov}, clip {'on' if self.clip else 'off'}"

    @property
    def numel(self):
        return self.rows * self.cols

    @property
    def chunks(self):
        return -(-self.numel // CHUNK)


@functools.lru_cache(maxsize=None)
def mom_cases():
    return tuple(MomCase(r, c, n, cl) for r, c in MOM_SHAPES for n in (0, 1) for cl in (False, True))


@functools.lru_cache(maxsize=None)
def mom_layouts(numel, chunks):
    """g and buf: three matrices at 0, 4 and 8 bytes off; U [3 numel] bf16 and partial [3 chunks] as one tensor each"""
    return {"g": Layout((numel,) * 3, (0, 1, 2)), "buf": Layout((numel,) * 3, (2, 0, 1)), "U": Layout((3 * numel,), align=8),
            "partial": Layout((3 * chunks,))}


@functools.lru_cache(maxsize=None)
def mom_inputs(numel):
    """g, buf [3 numel] float32; matrix 1 has no gradient (its g is all zero: what a NULL row stands for)"""
    gen = torch.Generator().manual_seed(numel)
    kind = element_kinds((numel,) * 3)
    n = kind.numel()
    rn = lambda: torch.randn(n, generator=gen)   # noqa: E731
    zero = torch.zeros(n)
    g, b = rn(), rn()
    g = torch.where((kind == 1) | (kind == 2), zero, g)
    g = torch.where(kind == 3, 1e-7 * rn(), g)
    g = torch.where(kind == 4, 1e3 * rn(), g)
    g = torch.where(kind == 5, 1e-3 * rn(), g)
    b = torch.where((kind == 2) | (kind == 3) | (kind == 6), zero, b)
    b = torch.where(kind == 5, 1e2 * rn(), b)
    b = torch.where(kind == 7, g * (1 + 1e-3 * rn()), b)
    g[numel:2 * numel] = 0
    return {"g": g, "buf": b}


def mom_reference(case):
    inp = mom_inputs(case.numel)
    beta = f32(MOM_BETA)
    w = 1 - beta
    gs, rg = clip_coefficient(MOM_CLIP if case.clip else None)
    g, b = inp["g"].double(), inp["buf"].double()
    gg = g * gs
    f_g = gg.abs() * (rg + U)
    f_g[case.numel:2 * case.numel] = 0
    d = gg - b
    b2 = beta * b + w * gg
    f_b = torch.maximum(w * f_g + 2 * U * w * d.abs() + U * b2.abs(), f_g + beta * (f_g + 2 * U * d.abs()) + U * b2.abs())
    if case.nesterov:
        uu = beta * b2 + w * gg
        d2 = b2 - gg
        f_d2 = f_b + f_g + U * d2.abs()
        f_u = torch.maximum(f_g + beta * (f_d2 + U * d2.abs()) + U * uu.abs(), f_b + w * (f_d2 + U * d2.abs()) + U * uu.abs())
    else:
        uu, f_u = b2, f_b
    return {"buf": b2, "u": uu, "F": {"buf": f_b, "u": f_u}}


def mom_partial(u_bf16_as_f32, numel, chunks, form=0):
    """partial [3 chunks] of muon_momentum_kernel from the values squared (float32 [3 numel])"""
    pad = torch.zeros(3, chunks * CHUNK)
    pad[:, :numel] = u_bf16_as_f32.view(3, numel)
    x = pad.view(3, chunks, CHUNK // 256, 256)
    s = torch.zeros(3, chunks, 256)
    for i in range(CHUNK // 256):
        s = fma(x[:, :, i], x[:, :, i], s) if form else s + x[:, :, i] * x[:, :, i]
    return block_sum_256(s).reshape(-1)


def restate_momentum(case, form=0, mut=None, null=True):
    """wft_muon_momentum_mt in CPU float32 -> {g, buf, U, partial: guarded buffers}; null: matrix 1's gradient row is address 0
    (its g buffer stays as it is), else it points at the all-zero gradient"""
    inp = mom_inputs(case.numel)
    lay = mom_layouts(case.numel, case.chunks)
    beta = f32(MOM_BETA)
    omb = float(np.float32(1) - np.float32(beta))
    gs = clip_gs(MOM_CLIP) if case.clip else 1.0
    g, b = inp["g"], inp["buf"]
    gg = g * gs
    w = beta if mut == "lerp weight beta for 1 - beta" else omb
    gb = g if mut == "clip applied to U but not to buf" else gg
    bb = fma(w, gb - b, b) if form else b + w * (gb - b)
    b_for_u = bb if gb is gg else (b + w * (gg - b))
    if not case.nesterov:
        uu = b_for_u
    elif mut == "nesterov lerp with the ends swapped":
        uu = b_for_u + beta * (gg - b_for_u)
    else:
        uu = fma(beta, b_for_u - gg, gg) if form else gg + beta * (b_for_u - gg)
    ub = uu.to(BF16)
    g_out = g.clone() if mut == "g not overwritten" else uu.clone()
    if null:
        g_out[case.numel:2 * case.numel] = 0   # nothing is written through address 0: the buffer keeps its zeros
    part = mom_partial(uu if mut == "partial from the fp32 u" else ub.float(), case.numel, case.chunks, form)
    return {"g": lay["g"].fill(g_out), "buf": lay["buf"].fill(uu if mut == "buf written with u" else bb), "U": lay["U"].fill(ub, BF16),
            "partial": lay["partial"].fill(part)}


def check_momentum(case, out, null=True, k=None, limit=1.0):
    lay = mom_layouts(case.numel, case.chunks)
    ref = mom_reference(case)
    ck = Checker("momentum " + case.name, k, limit)
    got = {a: lay[a].gather(out[a].cpu()) for a in lay}
    for a in lay:
        ck.true(lay[a].guards_intact(out[a]), f"{a}: a sentinel was overwritten")
    ck.within("buf", got["buf"], ref["buf"], ref["F"]["buf"])
    ne = case.numel
    live = torch.ones(3 * ne, dtype=torch.bool)
    if null:
        live[ne:2 * ne] = False
        ck.true(bool((bits(got["g"])[~live] == 0).all()), "the gradient buffer of the NULL row changed")
    ck.within("u", got["g"][live], ref["u"][live], ref["F"]["u"][live])
    # U is bf16 round-to-nearest-even of the u the kernel wrote (NULL row: of the u nobody wrote, so against the reference)
    ck.true(torch.equal(bits(got["U"])[live], bits(got["g"].to(BF16))[live]), "U is not RNE bf16 of the written g")
    if null:
        ck.within("U of the NULL row", got["U"].float()[~live], ref["u"][~live], bf16_half_ulp(ref["u"][~live]) + K["u"] * ref["F"]["u"][~live],
                  kname="none")
    sq = got["U"].double().view(3, -1) ** 2
    pad = torch.zeros(3, case.chunks * CHUNK, dtype=F64)
    pad[:, :ne] = sq
    s = pad.view(3, case.chunks, CHUNK).sum(-1).reshape(-1)
    cnt = torch.tensor([min(CHUNK, ne - c * CHUNK) for c in range(case.chunks)] * 3)
    dep = (-(-cnt // 256) + 10).double().sqrt()
    ck.within("partial", got["partial"], s, U * s * dep)
    return ck.done()


# ================================================================================================ Muon: prepare
# (rows, cols, rows_pad, cols_pad): the pads are for the orientation with rows <= cols
PREP_SHAPES = ((16, 320, 128, 384), (320, 16, 128, 384), (70, 130, 128, 256), (70, 130, 70, 130), (70, 130, 100, 200), (130, 70, 128, 256),
               (64, 64, 128, 128), (1, 65, 128, 128))
PREP_S = ((2.25, 2.0), (2.0, 2.0 ** -40), (2.0 ** -40, 0.0), (0.0, 2.25))   # sum of the partials of matrix 0, of matrix 1
PREP_CHUNKS = (1, 2, 300)


@dataclasses.dataclass(frozen=True)
class PrepCase:
    rows: int
    cols: int
    rp: int
    cp: int
    s: tuple
    chunks: int

    @property
    def name(self):
        return f"{self.rows}x{self.cols} -> {self.rp}x{self.cp}, s {self.s[0]:g} / {self.s[1]:g}, {self.chunks} chunks"

    @property
    def tall(self):
        return self.rows > self.cols


@functools.lru_cache(maxsize=None)
def prep_cases():
    return tuple(PrepCase(*sh, PREP_S[j], PREP_CHUNKS[(i + j) % 3]) for i, sh in enumerate(PREP_SHAPES) for j in range(len(PREP_S)))


def prep_partial(s, chunks):
    """`chunks` float32 entries, small integer multiples of a power of two, whose sum is s exactly in any order"""
    if s == 0:
        return torch.zeros(chunks)
    unit = 2.0 ** (math.frexp(s)[1] - 1 - 8)   # s = T units with 256 <= T < 512 ... 576
    T = int(round(s / unit))
    assert T * unit == s and T < 1024
    e = torch.full((chunks,), T // chunks, dtype=F64) + (torch.arange(chunks) < T % chunks)
    return (e * unit).float()


def prep_layouts(c):
    ne = c.rows * c.cols
    return {"U": Layout((2 * ne,), align=8), "partial": Layout((2 * c.chunks,)), "X": Layout((2 * c.rp * c.cp,), align=8),
            "Xt": Layout((2 * c.rp * c.cp,), align=8)}


@functools.lru_cache(maxsize=None)
def prep_inputs(c):
    """U bf16 [2, rows, cols] (scaled with the norm its matrix's partials give; all zero where they sum to 0) and partial [2, chunks]"""
    gen = torch.Generator().manual_seed(c.rows * 1000 + c.cols)
    ne = c.rows * c.cols
    scale = torch.tensor((1.0, 0.0, 1e-3, 1e2, 1.0, 2.0 ** -10, 1.0, 10.0))[element_kinds((ne, ne))]
    u = torch.randn(2 * ne, generator=gen) * scale
    for t in (0, 1):
        u[t * ne:(t + 1) * ne] *= math.sqrt(c.s[t])
    return {"U": u.to(BF16).view(2, c.rows, c.cols), "partial": torch.stack([prep_partial(s, c.chunks) for s in c.s])}


def restate_prepare(c, mut=None):
    """wft_muon_prepare in CPU float32 -> {X, Xt: guarded buffers, pre-filled with the sentinel}"""
    inp = prep_inputs(c)
    lay = prep_layouts(c)
    tall = c.rows >= c.cols if mut == "square treated as tall" else c.tall
    R, C = (c.cols, c.rows) if tall else (c.rows, c.cols)
    X = sentinel(2 * c.rp * c.cp, BF16).view(2, c.rp, c.cp).clone()
    Xt = sentinel(2 * c.rp * c.cp, BF16).view(2, c.cp, c.rp).clone()
    for t in (0, 1):
        s = final_sum(inp["partial"][0 if mut == "partial indexed without t chunks" else t])
        root = s.sqrt()
        nrm = (root if mut == "norm not rounded to bf16" else root.to(BF16).float()) + (0.0 if mut == "+ 1e-7 dropped" else f32(1e-7))
        u = inp["U"][t].float()
        q = ((u.t() if tall else u) / nrm).to(BF16)
        if mut != "pad not written":
            X[t], Xt[t] = 0, 0
        X[t, :R, :C] = q
        if mut == "Xt not transposed for a tall parameter" and tall:
            Xt[t] = X[t].reshape(c.cp, c.rp)
        else:
            Xt[t, :C, :R] = q.t()
    return {"X": lay["X"].fill(X.reshape(-1), BF16), "Xt": lay["Xt"].fill(Xt.reshape(-1), BF16)}


def check_prepare(c, out, limit=1.0):
    inp = prep_inputs(c)
    lay = prep_layouts(c)
    ck = Checker("prepare " + c.name, {}, limit)
    R, C = (c.cols, c.rows) if c.tall else (c.rows, c.cols)
    X = lay["X"].gather(out["X"].cpu()).view(2, c.rp, c.cp)
    Xt = lay["Xt"].gather(out["Xt"].cpu()).view(2, c.cp, c.rp)
    for a in ("X", "Xt"):
        ck.true(lay[a].guards_intact(out[a]), f"{a}: a sentinel was overwritten")
    for t in (0, 1):
        nrm = float(torch.tensor(math.sqrt(c.s[t]), dtype=F64).to(BF16)) + f32(1e-7)
        u = inp["U"][t].double()
        q = (u.t() if c.tall else u) / nrm
        ck.within("X", X[t, :R, :C].float(), q, bf16_half_ulp(q) + 4 * U * q.abs())
    frame = torch.ones(c.rp, c.cp, dtype=torch.bool)
    frame[:R, :C] = False
    ck.true(bool((bits(X)[:, frame] == 0).all()), "X: the pad is not +0")
    ck.true(bool((bits(Xt)[:, frame.t()] == 0).all()), "Xt: the pad is not +0")
    ck.true(torch.equal(bits(Xt), bits(X.transpose(1, 2).contiguous())), "Xt is not the transpose of X bit for bit")
    return ck.done()


# ================================================================================================ Muon: apply
APPLY_SHAPES = ((300, 300), (16, 320), (320, 16))
APPLY_LR = 0.02
APPLY_ORDER = (2, 0, 1)   # the order of the three p allocations in memory


@dataclasses.dataclass(frozen=True)
class ApplyCase:
    rows: int
    cols: int
    scale: float
    wd: float

    @property
    def name(self):
        return f"{self.rows}x{self.cols}, scale {self.scale:.3f}, weight_decay {self.wd:g}"

    @property
    def frame(self):
        """(frame rows, ldo) of O as muon_group_step lays it out: the 128-padded frame in p's orientation"""
        r128 = lambda x: -(-x // 128) * 128   # noqa: E731
        return r128(self.rows), r128(self.cols)


@functools.lru_cache(maxsize=None)
def apply_cases():
    return tuple(ApplyCase(r, c, s, wd) for r, c in APPLY_SHAPES for s in (1.0, math.sqrt(20.0)) for wd in (0.0, 0.01))


def apply_layouts(c):
    fr, ldo = c.frame
    return {"p": Layout((c.rows * c.cols,) * 3, (0, 1, 3), order=APPLY_ORDER), "O": Layout((3 * fr * ldo,), align=8)}


@functools.lru_cache(maxsize=None)
def apply_inputs(rows, cols):
    """p [3 numel] float32 and o [3, rows, cols] bf16; kinds: 1 o = 0, 2 p = 0, 3 p ~ 1e3 with tiny o, 4 o ~ 1e2, 5 p = o = 0"""
    gen = torch.Generator().manual_seed(rows * 7 + cols)
    ne = rows * cols
    kind = element_kinds((ne,) * 3)
    n = 3 * ne
    p, o = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    zero = torch.zeros(n)
    o = torch.where((kind == 1) | (kind == 5), zero, o)
    p = torch.where((kind == 2) | (kind == 5), zero, p)
    p = torch.where(kind == 3, 1e3 * (1 + torch.rand(n, generator=gen)), p)
    o = torch.where(kind == 3, 1e-4 * o, o)
    o = torch.where(kind == 4, 1e2 * o, o)
    return {"p": p, "o": o.to(BF16).view(3, rows, cols), "kind": kind}


def apply_frame(c):
    """O [3, frame rows, ldo] bf16: o inside [rows, cols], 1e30 everywhere else"""
    fr, ldo = c.frame
    O = torch.full((3, fr, ldo), 1e30, dtype=BF16)
    O[:, :c.rows, :c.cols] = apply_inputs(c.rows, c.cols)["o"]
    return O


def restate_apply(c, form=0, mut=None):
    inp = apply_inputs(c.rows, c.cols)
    lay = apply_layouts(c)
    fr, ldo = c.frame
    lr, wd, scale = np.float32(APPLY_LR), np.float32(c.wd), np.float32(c.scale)
    one = np.float32(1)
    decay = float(one - lr * wd) if form == 0 else f32(1 - float(lr) * float(wd))
    a = float(lr * scale)
    if mut == "decay missing":
        decay = 1.0
    if mut == "scale folded into the decay":
        decay, a = float(one - lr * wd * scale), float(lr)
    O = apply_frame(c).reshape(-1).float()
    i = torch.arange(c.rows * c.cols)
    r, col = i // c.cols, i % c.cols
    ld = c.cols if mut == "ldo ignored" else ldo
    so = c.rows * c.cols if mut == "stride_o taken as rows cols" else fr * ldo
    o = torch.stack([O[(t * so + r * ld + col) % O.numel()] for t in range(3)]).reshape(-1)
    p = inp["p"]
    new = p * decay - a * o if form == 0 else fma(p, decay, -(a * o)) if form == 1 else fma(-a, o, p * decay)
    return {"p": lay["p"].fill(new)}


def check_apply(c, out, k=None, limit=1.0):
    inp = apply_inputs(c.rows, c.cols)
    lay = apply_layouts(c)
    ck = Checker("apply " + c.name, k, limit)
    got = lay["p"].gather(out["p"].cpu())
    ck.true(lay["p"].guards_intact(out["p"]), "p: a sentinel was overwritten")
    p, o = inp["p"].double(), inp["o"].double().reshape(-1)
    decay, a = 1 - f32(APPLY_LR) * f32(c.wd), f32(APPLY_LR) * f32(c.scale)
    ck.within("apply", got, p * decay - a * o, U * ((p * decay).abs() + (a * o).abs()))
    if c.wd == 0:
        still = o == 0
        ck.true(bool(still.any()) and torch.equal(bits(got)[still], bits(inp["p"])[still]), "weight_decay 0, o = 0: p changed")
    return ck.done()
