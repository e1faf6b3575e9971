"""Cases, float64 reference, per-element bounds, float32 restatement and mutants for wft_mt_adamw8 of csrc/optim.hip (block-wise 8-bit
AdamW).  Shared by tests/test_adam8_host.py (CPU: the checkers accept the kernel's arithmetic in every contraction form and reject
every listed mutant of it) and tests/test_adam8_gpu.py (the kernel itself, through K.mt_adamw8, under the same checkers).  The scheme
is stated by oracle/adam8bit_oracle.py; the conventions are those of tests/_optim_cases.py, whose Layout, Checker, fma, mt_find,
chunk_starts and clip_gs are used here: the float32-rounded scalars promoted to float64, guarded buffers, bounds whose constants are
measured on a restatement and not chosen.

Buffers.  p, g (float32), state1, state2 (uint8), absmax1, absmax2 (float32) are views into flat buffers with at least GUARD = 64
sentinel elements before and after every tensor: -12345.0f for the float arrays, the byte 0xA5 for the code arrays (a valid code, so
that a kernel which decodes a sentinel does not leave the map).  Every array but g is read and written in place, so a buffer is its
input between sentinels.  Every checker asks that all sentinels are unchanged and that g, both maps and sumsq keep their bits.

Reference (float64, per element; q a = the decoded old moment, n the block's new absmax, taken over the block's own elements):
  gs = min(1, max_norm / (sqrt(sumsq) + 1e-6f)), g' = g gs;   m' = (q1[c1] a1) b1 + (1 - b1) g';   v' = (q2[c2] a2) b2 + (1 - b2) g'^2
  n1 = max |m'|, n2 = max v';   x = m' / n (0 where n = 0);   code = number of midpoints fl32((q[i] + q[i+1]) 0.5f) strictly below x
  step_size = -lr sqrt(bc2) / bc1, eps2 = sqrt(bc2) eps;   p' = p + step_size m' / (sqrt(v') + eps2), then times 1 - lr wd where wd > 0
Bound forms, u = 2^-24, rg = 3u where gs < 1 came from sumsq, else 0 (F_m and F_v of _optim_cases.py with q a in the place of m, and
one more u |b (q a)| for the rounding of the product q a itself):
  F_g'  = |g'| (rg + u) where gs < 1, else 0
  F_m   = u (2 |b1 q1 a1| + 2 |(1 - b1) g'| + |m'|) + (1 - b1) F_g'
  F_v   = u (2 b2 q2 a2 + 3 (1 - b2) g'^2 + v') + 2 (1 - b2) |g'| F_g'
  F_n   = F_m (F_v) of the element that attains the block's maximum
  F_x   = F_m / n + |x| (F_n / n + 2u)                   (1 / n rounded, the product rounded)
  F_den = u sqrt(v') + F_v / (2 sqrt(v')) + 2u eps2 + u den,   den = sqrt(v') + eps2            (F_v / sqrt(v') = 0 where v' = 0)
  F_t   = |t| (6u + F_den / den) + |step_size| F_m / den,   t = step_size m' / den   (sqrtf, two products and a division in step_size;
                                                                                      the quotient; the product)
  F_p   = F_t + u |p + t|  without decay;  with it  decay (F_t + u |p + t|) + u |p + t| (lr wd + decay) + u |p'|
Codes: where no midpoint lies within K F_x of x the code must be the float64 code; where one does, the code may be either of the two
codes next to it.  Two conditions keep that honest in stage 4: at most 1e-3 of a case's elements are that near a midpoint (asserted
for the reference inputs by the host test and again by the checker), and the number of codes that differ at all from the float64
code is printed per case.

Stages (the issue's): 1 the encoder alone (b1 = b2 = 0, g = 1 planted in every block, the real maps): all 256 entries of qmap1, its
255 float32 midpoints and their float32 neighbours both ways; for qmap2 the reachable fl32(g g) nearest below and above every midpoint,
the midpoint itself and every map entry where some g reaches it (stage1_probes() counts what no g reaches: 108 midpoints, 135 entries); each probe set as
a tensor's only block, as the second block of a chunk, as a last partial block and through the unaligned path.  2 the decoder (g = 0,
b1 = b2 = 1): every block holds all 256 codes, absmax in {2^-20, 1, 2^10}, different for the two states and for neighbouring blocks
and for block b and b + 32; a block whose extreme is negative; an all-zero block.  3 the whole update in exact arithmetic on dyadic
maps (qs[c] = (c - 127) / 128; qu[c] = c / 256, qu[255] = 1; b1 = 0.5, b2 = 0.75): with a1 = 2^A, a2 = 2^(2A - 6), g = j 2^(A - 7),
m' = (c1 - 127 + j) 2^(A - 8) = s 2^(A - 8) and v' = (3 c2' + j^2) 2^(2A - 16) = w 2^(2A - 16) are integers below 2^24 times a power of
two; one planted lane per block has s = +-512 and w = 2^18, so n1 = 2^(A + 1), n2 = 2^(2A + 2), x1 = s / 512 (a midpoint where s = 2
mod 4) and x2 = w / 2^18 (a midpoint where w = 512 mod 1024: a third of the lanes are given such a c2 where one exists); s is a ramp over
the block, of another step, sign and planted lane in the next block.  In stages 1 to 3 codes and absmax are bit for bit those of the
reference (but for the codes of state1 in the block with the negative extreme, whose 1 / n is not exact).  4 general values, one step
from a random state and the optimizer's first step (all-zero codes, absmax 0): element kinds 0 ordinary, 1 g = 0, 2 g = 0 with the
codes of 0, 3 g ~ 1e-7 with the codes of 0 (eps rules the denominator), 4 g ~ 1e3, 5 code 255 in state2 and a small old m, 6 p = 0,
7 p ~ 1e3 with tiny g and old m (the update is below half an ulp of p); three hyper-parameter sets x the bias corrections of steps 1, 2,
1000 x three clips as a Latin square.  A block whose absmax is subnormal overflows 1 / n (the kernel would normalise by Inf): every
case stays inside the normal range and that input is left out.

Tables (stages 3 and 4): A = 12 tensors of 1, 7, 8, 9, 2047, 2048, 2049, 5096, 65536, 65537, 65536 + 3 x 2048 + 5 and 2 x 65536 + 5
elements, six of them with exactly one array off its boundary (p 4 bytes, g 8 bytes, state1 1, 4 and 7 bytes, state2 3 bytes); B =
300 tensors of 1 + t % 7 elements, mixed misalignment.

The constants K are 4 x the worst |restatement - reference| / F over all cases and the three contraction forms (form 0: every
product rounded; 1, 2: a b + c contracted either way round), rounded up to a power of two.  Measured (seeds fixed per case):

  output    worst ratio of the restatement   4 x worst   K
  n1        0.724                            2.90        4
  n2        0.677                            2.71        4
  p         0.995                            3.98        4
  x1        0.575                            2.30        4
  x2        0.555                            2.22        4
"""
import dataclasses
import functools
import math

import numpy as np
import torch

from tests._optim_cases import (CHUNK, F64, GUARD, U, Checker, Layout, bits, chunk_starts, clip_coefficient, clip_gs, f32, fma, mt_find, ratio,  # noqa: F401
                                sentinel)
from whisper_finetune.model import optimizer as wopt

BLOCK = 2048           # include/wft.h WFT_Q8_BLOCK
SENT_U8 = 0xA5
U8 = torch.uint8
K = {"n1": 4.0, "n2": 4.0, "p": 4.0, "x1": 4.0, "x2": 4.0}
FORMS = (0, 1, 2)
NEAR_CAP = 1e-3
ARRAYS = ("p", "g", "s1", "s2", "a1", "a2")

MUTANTS = (
    "absmax over the first 2 047 elements of a block", "absmax left from the previous block", "absmax index without the chunk offset",
    "padding lanes of a partial block taking part in the max", "ties to the upper code", "bisection without its last step",
    "bisection that cannot return 255", "state2 decoded through qmap1", "encoding against the old absmax", "decoding with the new absmax",
    "v from the unscaled g", "coefficient not capped at 1", "+ 1e-6 dropped", "eps not scaled by sqrt(bc2)", "decay before the update",
    "decay applied when wd = 0 as 1 - lr", "scalar tail skipped", "unaligned path one element late", "last chunk at the full count",
    "mt_find with < for <=",
)


# ================================================================================================ maps
@functools.lru_cache(maxsize=None)
def real_maps():
    return wopt.create_dynamic_map(True).float().contiguous(), wopt.create_dynamic_map(False).float().contiguous()


@functools.lru_cache(maxsize=None)
def dyadic_maps():
    c = torch.arange(256, dtype=F64)
    qu = c / 256
    qu[255] = 1.0
    return ((c - 127) / 128).float(), qu.float()


def midpoints(q):
    """the kernel's 255 midpoints (q[i] + q[i + 1]) * 0.5f, in float32"""
    return (q[:-1] + q[1:]) * 0.5


# ================================================================================================ cases
@dataclasses.dataclass(eq=False)
class Case:
    name: str
    stage: int
    numels: tuple
    mis: dict        # array -> elements off the boundary, per tensor (p, g: of 4 floats; s1, s2: of 8 bytes)
    maps: tuple      # (q1, q2) float32 [256]
    scalars: tuple   # float32-rounded (lr, b1, b2, eps, wd, bc1, bc2)
    clip: object     # None or (sumsq, max_norm)
    inp: dict        # p, g float32 [total]; s1, s2 uint8 [total]; a1, a2 float32 [blocks]; all concatenated over the tensors
    exact: dict = None   # stages 1 to 3: s1, s2 [total], a1, a2 [blocks] bool: bit for bit the reference

    @functools.cached_property
    def nblocks(self):
        return tuple(-(-n // BLOCK) for n in self.numels)

    @functools.cached_property
    def lay(self):
        z = (0,) * len(self.numels)
        return {"p": Layout(self.numels, self.mis.get("p", z)), "g": Layout(self.numels, self.mis.get("g", z)),
                "s1": Layout(self.numels, self.mis.get("s1", z), align=8), "s2": Layout(self.numels, self.mis.get("s2", z), align=8),
                "a1": Layout(self.nblocks), "a2": Layout(self.nblocks)}

    @functools.cached_property
    def block_of(self):
        """the global block index of every element (concatenated order)"""
        boff = np.cumsum((0,) + self.nblocks)
        return torch.cat([boff[t] + torch.arange(n) // BLOCK for t, n in enumerate(self.numels)])

    def buffers(self):
        """fresh guarded buffers holding the inputs"""
        return {a: fill(self.lay[a], self.inp[a]) for a in ARRAYS}


def fill(lay, values):
    if values.dtype != U8:
        return lay.fill(values)
    buf = torch.full((lay.length,), SENT_U8, dtype=U8)
    buf[lay.index] = values
    return buf


def guards_intact(lay, buf):
    if buf.dtype != U8:
        return lay.guards_intact(buf)
    keep = torch.ones(lay.length, dtype=torch.bool)
    keep[lay.index] = False
    return bool((buf.cpu()[keep] == SENT_U8).all())


def block_coords(numels):
    """per element (concatenated): tensor, block within the tensor, lane within the block, length of that block"""
    t = torch.cat([torch.full((n,), i) for i, n in enumerate(numels)])
    e = torch.cat([torch.arange(n) for n in numels])
    n = torch.cat([torch.full((n,), n) for n in numels])
    b = e // BLOCK
    return t, b, e % BLOCK, torch.clamp(n - b * BLOCK, max=BLOCK)


def _random_state(total, blocks, gen):
    return {"s1": torch.randint(0, 256, (total,), generator=gen).to(U8), "s2": torch.randint(0, 256, (total,), generator=gen).to(U8),
            "a1": 10.0 ** (torch.rand(blocks, generator=gen) * 4 - 3), "a2": 10.0 ** (torch.rand(blocks, generator=gen) * 6 - 4)}


# ------------------------------------------------------------------------------------------------ stage 1
def _f32_neighbours(x, k):
    """float32 [len(x), 2k + 1]: x and its k float32 neighbours either way"""
    cols = {0: np.asarray(x, np.float32)}
    for d in range(1, k + 1):
        cols[d] = np.nextafter(cols[d - 1], np.float32(np.inf))
        cols[-d] = np.nextafter(cols[-d + 1], np.float32(-np.inf))
    return np.stack([cols[d] for d in range(-k, k + 1)], 1)


@functools.lru_cache(maxsize=None)
def stage1_probes():
    """-> {1: (g, want1), 2: (g, want2), "unreachable": (midpoints, entries of qmap2 no fl32(g g) equals)}: the probe values of either
    state with the code each must get, by construction (g[0] = 1 is the plant)"""
    q1, q2 = (q.numpy() for q in real_maps())
    m1, m2 = (midpoints(q).numpy() for q in real_maps())
    up, dn = np.nextafter(m1, np.float32(np.inf)), np.nextafter(m1, np.float32(-np.inf))
    g1 = np.concatenate([[1.0], q1, m1, up, dn]).astype(np.float32)
    w1 = np.concatenate([[255], np.arange(256), np.arange(255), np.arange(255) + 1, np.arange(255)])
    g2, w2, miss_mid, miss_ent = [1.0], [255], 0, 0
    for i, m in enumerate(m2):
        cand = _f32_neighbours([np.float32(math.sqrt(float(m)))], 8)[0]
        sq = cand * cand
        g2 += [cand[sq < m].max(), cand[sq > m].min()]
        w2 += [i, i + 1]
        if (sq == m).any():
            g2.append(cand[sq == m][0])
            w2.append(i)
        else:
            miss_mid += 1
    for c, q in enumerate(q2):
        cand = _f32_neighbours([np.float32(math.sqrt(float(q)))], 8)[0]
        hit = cand[cand * cand == q]
        if hit.size:
            g2.append(hit[0])
            w2.append(c)
        else:
            miss_ent += 1
    if len(g2) % 8 == 0:
        g2.append(1.0)
        w2.append(255)
    return {1: (torch.tensor(g1), torch.tensor(w1)), 2: (torch.tensor(np.asarray(g2, np.float32)), torch.tensor(w2)),
            "unreachable": (miss_mid, miss_ent)}


# (probe set, blocks of filler in front, partial, misaligned array, elements off)
STAGE1_TENSORS = ((1, 0, False, None, 0), (2, 0, False, None, 0), (1, 1, False, None, 0), (2, 1, False, None, 0), (1, 1, True, None, 0),
                  (2, 1, True, None, 0), (1, 0, False, "p", 1), (2, 0, False, "s2", 3), (1, 1, True, "s1", 1), (2, 0, True, "g", 2))


@functools.lru_cache(maxsize=None)
def stage1_case():
    gen = torch.Generator().manual_seed(101)
    pr = stage1_probes()
    gs, numels, mis = [], [], {a: [] for a in ("p", "g", "s1", "s2")}
    for which, filler, partial, arr, off in STAGE1_TENSORS:
        g = pr[which][0]
        parts = []
        for _ in range(filler):
            f = torch.rand(BLOCK, generator=gen) * 2 - 1
            f[777] = 1.0
            parts.append(f)
        parts.append(g if partial else g.repeat(-(-BLOCK // g.numel()))[:BLOCK])
        gs.append(torch.cat(parts))
        numels.append(gs[-1].numel())
        for a in mis:
            mis[a].append(off if a == arr else 0)
    g = torch.cat(gs)
    c = Case("stage 1", 1, tuple(numels), {a: tuple(v) for a, v in mis.items()}, real_maps(),
             tuple(f32(x) for x in (1e-2, 0.0, 0.0, 1e-6, 0.1, 0.1, 0.02)), None, {})
    c.inp = {"p": torch.randn(g.numel(), generator=gen), "g": g, **_random_state(g.numel(), sum(c.nblocks), gen)}
    c.exact = {"s1": torch.ones(g.numel(), dtype=torch.bool), "s2": torch.ones(g.numel(), dtype=torch.bool),
               "a1": torch.ones(sum(c.nblocks), dtype=torch.bool), "a2": torch.ones(sum(c.nblocks), dtype=torch.bool)}
    return c


def stage1_probe_slices(c):
    """(probe set, slice of the concatenated elements holding it from its first value on, its length) per tensor"""
    out, o = [], 0
    for (which, filler, partial, _, _), n in zip(STAGE1_TENSORS, c.numels):
        out.append((which, o + filler * BLOCK, n - filler * BLOCK))
        o += n
    return out


# ------------------------------------------------------------------------------------------------ stage 2
STAGE2_NUMELS = (CHUNK + 3 * BLOCK + 5, 4 * BLOCK, 2049, 7)
STAGE2_POW = (2.0 ** -20, 1.0, 2.0 ** 10)
STAGE2_ZERO, STAGE2_NEG = (1, 1), (1, 2)     # (tensor, block): all-zero; extreme negative (code 0 present, code 255 absent)


@functools.lru_cache(maxsize=None)
def stage2_case():
    gen = torch.Generator().manual_seed(102)
    t, b, i, _ = block_coords(STAGE2_NUMELS)
    c1 = (255 - i * (2 * (b % 4) + 1)) % 256       # an odd multiplier: every 256 lanes hold all 256 codes; lane 0 holds 255
    c2 = (255 + i * (2 * (b % 3) + 3)) % 256
    zero = (t == STAGE2_ZERO[0]) & (b == STAGE2_ZERO[1])
    neg = (t == STAGE2_NEG[0]) & (b == STAGE2_NEG[1])
    c1 = torch.where(zero, torch.full_like(c1, 127), torch.where(neg, (i * 7) % 255, c1))
    c2 = torch.where(zero, torch.zeros_like(c2), c2)
    nb = tuple(-(-n // BLOCK) for n in STAGE2_NUMELS)
    tb = torch.cat([torch.full((n,), k) for k, n in enumerate(nb)])
    bb = torch.cat([torch.arange(n) for n in nb])
    pw = torch.tensor(STAGE2_POW)
    total = sum(STAGE2_NUMELS)
    c = Case("stage 2", 2, STAGE2_NUMELS, {"s2": (0, 0, 3, 0)}, real_maps(), tuple(f32(x) for x in (1e-2, 1.0, 1.0, 1e-6, 0.1, 0.1, 0.02)), None,
             {"p": torch.randn(total, generator=gen), "g": torch.zeros(total), "s1": c1.to(U8), "s2": c2.to(U8), "a1": pw[(bb + tb) % 3],
              "a2": pw[(bb + tb + 1) % 3]})
    c.exact = {"s1": ~neg, "s2": torch.ones(total, dtype=torch.bool), "a1": torch.ones(sum(nb), dtype=torch.bool),
               "a2": torch.ones(sum(nb), dtype=torch.bool)}
    return c


# ------------------------------------------------------------------------------------------------ tables A and B
A_NUMELS = (1, 7, 8, 9, 2047, 2048, 2049, 5096, CHUNK, CHUNK + 1, CHUNK + 3 * BLOCK + 5, 2 * CHUNK + 5)
A_MIS = {"p": (0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), "g": (0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0), "s1": (0, 0, 0, 1, 0, 0, 0, 4, 0, 7, 0, 0),
         "s2": (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0)}
B_NUMELS = tuple(1 + t % 7 for t in range(300))
B_MIS = {"p": tuple(t % 4 for t in range(300)), "g": tuple((t // 4) % 4 for t in range(300)), "s1": tuple(t % 8 for t in range(300)),
         "s2": tuple((3 * t) % 8 for t in range(300))}
TABLES = {"A": (A_NUMELS, A_MIS), "B": (B_NUMELS, B_MIS)}


# ------------------------------------------------------------------------------------------------ stage 3
S3_PLANT = (0, 2047, 1023, 8)                    # the planted lane of block b is S3_PLANT[b % 4] % (length of the block)
S3_STEP = (1, 2, 4, 5, 7, 8, 10, 13)             # coprime to 1023
S3_A = (-3, 0, 4)
S3_MID2 = torch.tensor([(2 * c + 1) * 512 for c in range(254)] + [510 * 512])   # the midpoints of qu in units of 2^-18


@functools.lru_cache(maxsize=None)
def stage3_case(table):
    """-> the case; its `want` holds s, w and codes and absmax in integer arithmetic"""
    numels, mis = TABLES[table]
    gen = torch.Generator().manual_seed(301 if table == "A" else 302)
    t, b, i, ln = block_coords(numels)
    n = t.numel()
    plant = torch.tensor(S3_PLANT)[b % 4] % ln
    planted = i == plant
    r = torch.where(planted, torch.zeros_like(i), 1 + ((i - plant) * torch.tensor(S3_STEP)[b % 8]) % 1023)
    sign = 1 - 2 * (b % 2)
    s = sign * (512 - r)                           # the plant alone has |s| = 512: it is the block's only maximum
    lo, hi = torch.clamp(s - 128, min=-511), torch.clamp(s + 127, max=511)
    j = lo + torch.randint(0, 1 << 30, (n,), generator=gen) % (hi - lo + 1)
    c1 = s + 127 - j
    c2p = torch.randint(0, 256, (n,), generator=gen)
    c2p = torch.where(c2p == 255, torch.full_like(c2p, 256), c2p)
    tie = ((512 - j * j) * 683) % 1024             # 3 x 683 = 1 mod 1024: 3 tie + j^2 = 512 mod 1024, a midpoint of qu
    c2p = torch.where((i % 3 == 0) & ((tie <= 254) | (tie == 256)), tie, c2p)
    j = torch.where(planted, 512 * sign, j)
    c1 = torch.where(planted, torch.full_like(c1, 127), c1)
    c2p = torch.where(planted, torch.zeros_like(c2p), c2p)
    w = 3 * c2p + j * j
    A = torch.tensor(S3_A)[(b + t) % 3]
    nb = tuple(-(-x // BLOCK) for x in numels)
    tb = torch.cat([torch.full((x,), k) for k, x in enumerate(nb)])
    bb = torch.cat([torch.arange(x) for x in nb])
    Ab = torch.tensor(S3_A)[(bb + tb) % 3].double()
    one = torch.ones(n, dtype=F64)
    c = Case(f"stage 3, table {table}", 3, numels, mis, dyadic_maps(), tuple(f32(x) for x in (1e-2, 0.5, 0.75, 1e-6, 0.1, 0.5, 0.25)),
             (0.25, 1.0) if table == "A" else None,
             {"p": torch.randn(n, generator=gen), "g": (j.double() * torch.ldexp(one, A - 7)).float(), "s1": c1.to(U8),
              "s2": torch.where(c2p == 256, torch.full_like(c2p, 255), c2p).to(U8), "a1": torch.ldexp(torch.ones_like(Ab), Ab.long()).float(),
              "a2": torch.ldexp(torch.ones_like(Ab), (2 * Ab - 6).long()).float()})
    c.exact = {"s1": torch.ones(n, dtype=torch.bool), "s2": torch.ones(n, dtype=torch.bool), "a1": torch.ones(sum(nb), dtype=torch.bool),
               "a2": torch.ones(sum(nb), dtype=torch.bool)}
    c.want = {"s": s, "w": w, "s1": torch.clamp((s + 506 + 3) // 4, 0, 255).to(U8), "s2": torch.searchsorted(S3_MID2, w).to(U8),
              "a1": torch.ldexp(torch.ones_like(Ab), (Ab + 1).long()).float(), "a2": torch.ldexp(torch.ones_like(Ab), (2 * Ab + 2).long()).float()}
    return c


# ------------------------------------------------------------------------------------------------ stage 4
# (lr, beta1, beta2, eps, weight_decay)
HP = ((1e-2, 0.9, 0.98, 1e-6, 0.1), (1e-3, 0.9, 0.999, 1e-8, 0.0), (3e-4, 0.95, 0.95, 1e-10, 0.01))
STEPS = (1, 2, 1000)
# no clip; coefficient 2, capped: gs = 1 from sumsq; sumsq 1e-10 (the + 1e-6 is a tenth of the norm): gs ~ 0.5
CLIPS = (None, (0.25, 1.0), (1e-10, 5.5e-6))
# (table, hp, step, clip, first step): a Latin square of hp x step x clip per table, and the optimizer's own first step
STAGE4 = tuple((tb, h, s, (h + s) % 3, False) for tb in "AB" for h in range(3) for s in range(3)) + (("A", 0, 0, 2, True), ("B", 1, 0, 0, True))


def adam8_values(kind, gen, q1, q2):
    """p, g, s1, s2 per element of the kinds of the top (the codes of 0: 127 in the signed map, 0 in the unsigned one)"""
    n = kind.numel()
    rn = lambda: torch.randn(n, generator=gen)   # noqa: E731
    ri = lambda lo, hi: torch.randint(lo, hi, (n,), generator=gen)   # noqa: E731
    zero1 = int((q1 == 0).nonzero()[0])
    p, g, s1, s2 = rn(), rn(), ri(0, 256), ri(0, 256)
    zero = torch.zeros(n)
    g = torch.where((kind == 1) | (kind == 2), zero, g)
    g = torch.where(kind == 3, 1e-7 * rn(), g)
    g = torch.where(kind == 4, 1e3 * rn(), g)
    g = torch.where(kind == 7, 1e-6 * rn(), g)
    s1 = torch.where((kind == 2) | (kind == 3), torch.full_like(s1, zero1), s1)
    s2 = torch.where((kind == 2) | (kind == 3), torch.zeros_like(s2), s2)
    s1 = torch.where(kind == 5, zero1 - 12 + ri(0, 25), s1)    # |q1| below 1e-3
    s1 = torch.where(kind == 7, zero1 - 1 + ri(0, 3), s1)      # |q1| at most 5.5e-7
    s2 = torch.where(kind == 5, torch.full_like(s2, 255), s2)
    s2 = torch.where(kind == 7, 200 + ri(0, 56), s2)
    p = torch.where(kind == 6, zero, p)
    p = torch.where(kind == 7, 1e3 * (1 + torch.rand(n, generator=gen)) * torch.sign(rn()), p)
    return {"p": p, "g": g, "s1": s1.to(U8), "s2": s2.to(U8)}


@functools.lru_cache(maxsize=None)
def stage4_inputs(table, first):
    numels, _ = TABLES[table]
    gen = torch.Generator().manual_seed({"A": 41, "B": 42}[table] + (100 if first else 0))
    t, b, i, _ = block_coords(numels)
    kind = (i + (3 * t if table == "B" else b)) % 8
    q1, q2 = real_maps()
    d = adam8_values(kind, gen, q1, q2)
    nb = sum(-(-x // BLOCK) for x in numels)
    d.update({k: v for k, v in _random_state(t.numel(), nb, gen).items() if k in ("a1", "a2")})
    if first:
        d.update({"s1": torch.zeros_like(d["s1"]), "s2": torch.zeros_like(d["s2"]), "a1": torch.zeros(nb), "a2": torch.zeros(nb)})
    d["kind"] = kind
    return d


@functools.lru_cache(maxsize=None)
def stage4_case(k):
    table, h, s, cl, first = STAGE4[k]
    numels, mis = TABLES[table]
    lr, b1, b2, eps, wd = HP[h]
    step = STEPS[s]
    return Case(f"stage 4, table {table}, hp {h}, step {step}, clip {cl}" + (", first step" if first else ""), 4, numels, mis, real_maps(),
                tuple(f32(x) for x in (lr, b1, b2, eps, wd, 1 - b1 ** step, 1 - b2 ** step)), CLIPS[cl], stage4_inputs(table, first))


def exact_cases():
    return (stage1_case(), stage2_case(), stage3_case("A"), stage3_case("B"))


def all_cases():
    return exact_cases() + tuple(stage4_case(k) for k in range(len(STAGE4)))


# ================================================================================================ reference
def _block_max(c, x):
    return torch.zeros(sum(c.nblocks), dtype=F64).scatter_reduce(0, c.block_of, x, "amax", include_self=True)


def reference(c):
    """float64 closed forms of one launch and the bound forms F (docstring); the code band [lo, hi] at the K in force is taken by
    check_adam8.  Not cached: table A is 3 MB per array"""
    lr, b1, b2, eps, wd, bc1, bc2 = c.scalars
    q1, q2 = (q.double() for q in c.maps)
    blk = c.block_of
    gs, rg = clip_coefficient(c.clip)
    p, g = c.inp["p"].double(), c.inp["g"].double()
    d1 = q1[c.inp["s1"].long()] * c.inp["a1"].double()[blk]
    d2 = q2[c.inp["s2"].long()] * c.inp["a2"].double()[blk]
    gg = g * gs
    f_g = gg.abs() * (rg + U) if gs != 1.0 else torch.zeros_like(gg)
    m = d1 * b1 + (1 - b1) * gg
    v = d2 * b2 + (1 - b2) * gg * gg
    if c.stage == 1:   # b1 = b2 = 0: v' is the single float32 product fl32(g g) under any contraction, and the probes are built on it
        v = v.float().double()
    f_m = U * (2 * (b1 * d1).abs() + 2 * ((1 - b1) * gg).abs() + m.abs()) + (1 - b1) * f_g
    f_v = U * (2 * b2 * d2 + 3 * (1 - b2) * gg * gg + v) + 2 * (1 - b2) * gg.abs() * f_g
    out = {"m": m, "v": v, "F": {}}
    for key, val, f_val in (("1", m.abs(), f_m), ("2", v, f_v)):
        n = _block_max(c, val)
        f_n = _block_max(c, torch.where(val == n[blk], f_val, torch.zeros_like(f_val)))
        nn, fnn = n[blk], f_n[blk]
        safe = torch.where(nn > 0, nn, torch.ones_like(nn))
        x = torch.where(nn > 0, (m if key == "1" else v) / safe, torch.zeros_like(nn))
        f_x = torch.where(nn > 0, f_val / safe + x.abs() * (fnn / safe + 2 * U), torch.zeros_like(nn))
        mid = midpoints(c.maps[int(key) - 1]).double()
        out.update({"n" + key: n, "x" + key: x, "code" + key: torch.searchsorted(mid, x), "mid" + key: mid})
        out["F"].update({"n" + key: f_n, "x" + key: f_x})
    c2 = math.sqrt(bc2)
    step, eps2 = -lr * c2 / bc1, c2 * eps
    sq = v.sqrt()
    den = sq + eps2
    t = step * m / den
    f_den = U * sq + torch.where(v > 0, f_v / (2 * torch.where(v > 0, sq, torch.ones_like(sq))), torch.zeros_like(sq)) + 2 * U * eps2 + U * den
    f_t = t.abs() * (6 * U + f_den / den) + abs(step) * f_m / den
    pre = p + t
    f_pre = f_t + U * pre.abs()
    if wd > 0:
        decay = 1 - lr * wd
        out["p"] = pre * decay
        out["F"]["p"] = decay * f_pre + U * pre.abs() * (lr * wd + decay) + U * out["p"].abs()
    else:
        out["p"], out["F"]["p"] = pre, f_pre
    return out


def code_band(ref, key, k):
    """-> (lo, hi, near): the codes of x - k F_x and x + k F_x, and where they differ (a midpoint lies within k F_x of x)"""
    x, f, mid = ref["x" + key], ref["F"]["x" + key], ref["mid" + key]
    lo, hi = torch.searchsorted(mid, x - k * f), torch.searchsorted(mid, x + k * f, right=True)
    return lo, hi, lo != hi


# ================================================================================================ restatement
def q8_encode(mid, x, mut=None):
    """q8_encode of optim.hip on a float32 tensor: the 8-step bisection over the 255 midpoints"""
    lo = torch.zeros(x.shape, dtype=torch.long)
    top = 254 if mut == "bisection that cannot return 255" else 255
    for step in (128, 64, 32, 16, 8, 4, 2, 1)[:7 if mut == "bisection without its last step" else 8]:
        probe = lo + step
        at = mid[torch.clamp(probe - 1, max=254)]
        ok = (probe <= top) & ((at <= x) if mut == "ties to the upper code" else (at < x))
        lo = torch.where(ok, probe, lo)
    return lo.to(U8)


def _scalars32(c, form, mut):
    lr, b1, b2, eps, wd, bc1, bc2 = (np.float32(x) for x in c.scalars)
    one = np.float32(1)
    c2 = np.sqrt(bc2)
    decay = float(one - lr * wd) if form == 0 else f32(1 - float(lr) * float(wd))
    if mut == "decay applied when wd = 0 as 1 - lr" and wd == 0:
        decay = float(one - lr)
    return {"b1": float(b1), "b2": float(b2), "omb1": float(one - b1), "omb2": float(one - b2), "step": float(-lr * c2 / bc1),
            "eps2": float(eps) if mut == "eps not scaled by sqrt(bc2)" else float(c2 * eps), "decay": decay,
            "decays": bool(wd > 0) or mut == "decay applied when wd = 0 as 1 - lr"}


def _moments(q1, q2, c1, c2, a1, a2, gv, gs, sc, form, mut):
    gg = gv * gs
    gq = gv if mut == "v from the unscaled g" else gg
    d1 = q1[c1] * a1
    d2 = (q1 if mut == "state2 decoded through qmap1" else q2)[c2] * a2
    b1, b2, omb1, omb2 = sc["b1"], sc["b2"], sc["omb1"], sc["omb2"]
    m = d1 * b1 + omb1 * gg if form == 0 else fma(d1, b1, omb1 * gg) if form == 1 else fma(omb1, gg, d1 * b1)
    v = d2 * b2 + (omb2 * gq) * gq if form == 0 else fma(d2, b2, (omb2 * gq) * gq) if form == 1 else fma(omb2 * gq, gq, d2 * b2)
    return m, v


def restate_mt_adamw8(case, form=0, mut=None):
    """wft_mt_adamw8 in CPU float32 on guarded buffers -> {p, g, s1, s2, a1, a2: the buffers after the launch; x1, x2: the normalised
    values it encoded, concatenated over the tensors (float32; for measuring K)}.  In the kernel's order: a workgroup per chunk finds
    its tensor by mt_find and walks the chunk's blocks in sequence ([block, thread, 8 consecutive elements] below; no block reads what
    another wrote, so the walk is one tensor operation); the block maximum runs over all 256 threads, the padding lanes of a partial
    block holding 0"""
    lay, numels = case.lay, case.numels
    buf = case.buffers()
    q1, q2 = case.maps
    mid1, mid2 = midpoints(q1), midpoints(q2)
    sc = _scalars32(case, form, mut)
    gs = clip_gs(case.clip, mut)
    cs = chunk_starts(numels)
    xs = {"x1": torch.zeros(sum(numels)), "x2": torch.zeros(sum(numels))}
    offs = np.cumsum((0,) + tuple(numels))
    for ch in range(cs[-1]):
        t = mt_find(cs, len(numels), ch, strict=mut == "mt_find with < for <=")
        off = (ch - cs[t]) * CHUNK
        cnt = min(numels[t] - off, CHUNK)
        if mut == "last chunk at the full count":
            cnt = CHUNK
        st = {a: lay[a].starts[t] + off for a in ("p", "g", "s1", "s2")}
        sa = {a: lay[a].starts[t] + (0 if mut == "absmax index without the chunk offset" else off // BLOCK) for a in ("a1", "a2")}
        # (a mutant past the tensor: no further than the buffers reach)
        cnt = min(cnt, *(lay[a].length - st[a] for a in st), *((lay[a].length - sa[a]) * BLOCK for a in sa))
        if cnt <= 0:
            continue
        al = st["p"] % 4 == 0 and st["g"] % 4 == 0 and st["s1"] % 8 == 0 and st["s2"] % 8 == 0
        nblk = -(-cnt // BLOCK)
        # (of the threads wholly past the end of a chunk's only block, which all hold the same padding, the first alone is kept)
        threads = 256 if nblk > 1 else min(256, -(-cnt // 8) + 1)
        idx = torch.arange(nblk * threads * 8)
        valid = idx < cnt
        if mut == "scalar tail skipped" and al:
            valid = idx < (cnt & ~7)
        if mut == "unaligned path one element late" and not al:
            valid &= idx >= 1
        at = torch.clamp(idx, max=cnt - 1)
        shape = (nblk, threads, 8)
        ld = lambda a, pad: torch.where(valid, buf[a][st[a] + at], torch.full((), pad, dtype=buf[a].dtype)).view(shape)   # noqa: E731
        pv, gv, c1, c2 = ld("p", 0.0), ld("g", 0.0), ld("s1", 0).long(), ld("s2", 0).long()
        a1 = buf["a1"][sa["a1"]:sa["a1"] + nblk].clone().view(nblk, 1, 1)
        a2 = buf["a2"][sa["a2"]:sa["a2"] + nblk].clone().view(nblk, 1, 1)
        vv = valid.view(shape)
        live = torch.ones_like(vv) if mut == "padding lanes of a partial block taking part in the max" else vv
        if mut == "absmax over the first 2 047 elements of a block" and threads == 256:
            live = live.clone()
            live[:, 255, 7] = False

        def moments(a1, a2):
            m, v = _moments(q1, q2, c1, c2, a1, a2, gv, gs, sc, form, mut)
            zero = torch.zeros(())
            m, v = torch.where(live, m, zero), torch.where(live, v, zero)
            n1 = m.abs().amax((1, 2))
            n2 = torch.clamp(v.amax((1, 2)), min=0.0)
            if mut == "absmax over the first 2 047 elements of a block":   # (the lane is left out of the max alone)
                m, v = _moments(q1, q2, c1, c2, a1, a2, gv, gs, sc, form, mut)
                m, v = torch.where(vv, m, zero), torch.where(vv, v, zero)
            return m, v, n1, n2

        m, v, n1, n2 = moments(a1, a2)
        if mut == "decoding with the new absmax":
            m, v, n1, n2 = moments(n1.view(nblk, 1, 1), n2.view(nblk, 1, 1))
        if mut == "absmax left from the previous block":
            n1, n2 = torch.cat([n1[:1], n1[:-1]]), torch.cat([n2[:1], n2[:-1]])
        e1, e2 = (a1.view(-1), a2.view(-1)) if mut == "encoding against the old absmax" else (n1, n2)
        i1 = torch.where(e1 > 0, 1.0 / torch.where(e1 > 0, e1, torch.ones_like(e1)), torch.zeros_like(e1)).view(nblk, 1, 1)
        i2 = torch.where(e2 > 0, 1.0 / torch.where(e2 > 0, e2, torch.ones_like(e2)), torch.zeros_like(e2)).view(nblk, 1, 1)
        quot = m / (v.sqrt() + sc["eps2"])
        if mut == "decay before the update":
            pn = pv * sc["decay"] + sc["step"] * quot
        else:
            pn = pv + sc["step"] * quot if form == 0 else fma(sc["step"], quot, pv)
            if sc["decays"]:
                pn = pn * sc["decay"]
        x1, x2 = m * i1, v * i2
        k1, k2 = q8_encode(mid1, x1, mut), q8_encode(mid2, x2, mut)
        w = idx[valid]
        for a, val in (("p", pn), ("s1", k1), ("s2", k2)):
            buf[a][st[a] + w] = val.reshape(-1)[valid]
        buf["a1"][sa["a1"]:sa["a1"] + nblk] = n1
        buf["a2"][sa["a2"]:sa["a2"] + nblk] = n2
        own = valid & (idx < numels[t] - off)
        xs["x1"][offs[t] + off + idx[own]] = x1.reshape(-1)[own]
        xs["x2"][offs[t] + off + idx[own]] = x2.reshape(-1)[own]
    buf.update(xs)
    return buf


# ================================================================================================ checker
def check_adam8(case, out, k=None, limit=1.0, inputs=None, ref=None):
    """the buffers p, s1, s2, a1, a2 of `out` per element: absmax and p within K F, every code inside its band (and none but the
    float64 code where no midpoint is near), bit for bit where the case is exact; every sentinel unchanged; g (and, where `out` or
    `inputs` holds them, q1, q2, sumsq) keeping its bits.  -> the worst ratios, the near-midpoint shares and the counts of codes that
    differ from the float64 code"""
    k = K if k is None else k
    lay = case.lay
    ref = reference(case) if ref is None else ref
    ck = Checker(case.name, k, limit)
    for a in ARRAYS:
        ck.true(guards_intact(lay[a], out[a]), f"{a}: a sentinel was overwritten")
    ck.true(torch.equal(bits(out["g"].cpu()), bits(fill(lay["g"], case.inp["g"]))), "g: the const gradient buffer changed")
    for a, was in (inputs or {}).items():
        ck.true(torch.equal(bits(out[a].cpu()), bits(was.cpu())), f"{a}: a const input changed")
    got = {a: lay[a].gather(out[a].cpu()) for a in ARRAYS}
    for key in ("1", "2"):
        ck.within("n" + key, got["a" + key], ref["n" + key], ref["F"]["n" + key])
        lo, hi, near = code_band(ref, key, k["x" + key])
        code = got["s" + key].long()
        bad = (code < lo) | (code > hi)
        ck.true(not bad.any(), f"state{key}: {int(bad.sum())} codes outside their band, the first at element {int(bad.nonzero()[0]) if bad.any() else -1}"
                f" (got {int(code[bad][0]) if bad.any() else -1}, float64 code {int(ref['code' + key][bad][0]) if bad.any() else -1})")
        ck.worst["near" + key] = float(near.double().mean())
        ck.worst["diff" + key] = float((code != ref["code" + key]).sum())
        if case.stage == 4:
            ck.true(bool((hi - lo <= 1).all()), f"state{key}: a band holds more than one midpoint")
            ck.true(ck.worst["near" + key] <= NEAR_CAP, f"state{key}: {ck.worst['near' + key]:.2e} of the elements are near a midpoint")
        if case.exact is not None:
            ex = case.exact["s" + key]
            ck.true(torch.equal(got["s" + key][ex], ref["code" + key][ex].to(U8)), f"state{key}: the codes are not bit for bit the reference's"
                    f" ({int((code != ref['code' + key])[ex].sum())} differ)")
            ex = case.exact["a" + key]
            ck.true(torch.equal(bits(got["a" + key][ex]), bits(ref["n" + key].float()[ex])), f"absmax{key} is not bit for bit the reference's")
    ck.within("p", got["p"], ref["p"], ref["F"]["p"])
    return ck.done()


def measure_x(case, out, ref):
    """worst |x - reference| / F_x of a restatement's normalised values (K = 1)"""
    return {"x" + key: ratio(out["x" + key], ref["x" + key], ref["F"]["x" + key]) for key in ("1", "2")}
