"""Probe operands for the training attention kernels (csrc/attn*.hip), their fp64 oracle, an fp32 -> bf16 emulation of the
kernels' arithmetic, the ways a tiled kernel loses or leaks one key restated as wrong masks ("mutants"), and the per-(row, head)
bound.  CPU only, plain torch; shared by tests/test_attn_probe_host.py (which proves on the CPU that the bound passes the correct
emulation and fails every mutant) and tests/test_attn_probe_gpu.py (which holds every kernel of the dispatch plan to it).

Why structured operands: with randn operands one key carries 1 / Tk of a row's softmax mass, so a key lost or leaked at a tile seam
moves one row by 1/65 .. 1/1500 of |v| — below any bound a bf16 kernel can be held to.  Here every query row puts nearly all of its
mass, in equal halves, on two chosen allowed keys that sit at tile edges, and is aligned just as strongly with a decoy key it must
not see (causal: key i + 1; non-causal: the guard row behind the last key, which for all but the last batch entry is exactly where a
kernel that runs one key over reads).  Losing a target key or admitting the decoy then moves o, lse, dq, dk and dv of that row by
O(1) of their own size.

Construction (per batch entry and head): keys are 8 u_j with u_j random unit vectors, rounded to bf16.  For a row with target keys
a, b and decoy d the query is the minimum-norm vector with scale * q . k_t = 16 for t in {a, b, d}, solved on the bf16 bits of the
keys, so the three scores are equal BY CONSTRUCTION up to q's own bf16 rounding and not by luck of the random cross terms; plus
a random part of its own, projected off the constrained keys, so that the rows that share a target do not all hand dK the same
vector.  Every other key of norm 8 scores ~N(0, 3.7^2), whose tail over a few hundred keys and a few thousand rows reaches the
targets' 16: each row's highest 16 background keys therefore join its constraints, capped at a score of 8, and in the non-causal
cases (up to 1500 keys) only the edge keys and the guard rows have norm 8, the keys in between 2.  The builder asserts in fp64,
for every row and head, that the two targets hold 95 % of the mass, each of them (and the decoy, were it admitted) at least 0.1;
as built (seed 0) they hold 97.9 % or more and the decoy would take 0.32.  v and do are randn.
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch

BF = torch.bfloat16
HD = 64
SCALE = 0.125
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
ALPHA = SCALE * LOG2E      # what a prescaled q carries (ops.QK_ALPHA)
GUARD = 8                  # rows behind every batch entry's Tk keys that the call's Tk excludes
TARGET_SCORE = 16.0        # scale * q . k of the two targets and of the decoy
FLOOR = 2.0 ** -6          # close_rows: a row's scale is never taken below FLOOR * the tensor's max|ref|
TOL = 2.0 ** -5            # derived and asserted by tests/test_attn_probe_host.py (see its docstring); never from a kernel
LSE_TOL = 1e-4             # |lse err| <= LSE_TOL * max|lse ref| per row (tests/test_kernels_gpu.py test_attention_fwd_bwd)
NOISE, NOISE_CAUSAL = 2.5, 1.0   # per-element standard deviation of each row's own random part of q (see probe_case)
INTERIOR_NORM = 2.0        # |k| of the non-causal cases' keys that are no edge (edge keys, guard rows and all causal keys: 8)
PIN_ROUNDS, PIN_PER_ROUND, PIN_CAP = 4, 4, 8.0   # probe_case: a row's highest background keys are capped at a score of 8
MIN_TARGET_MASS = 0.95     # the two targets together, of the row's softmax
MIN_EACH_MASS = 0.1        # each target alone; and the decoy, were it admitted


def heads(t, H):
    """[B, T, H * 64] (any strides) -> [B, H, T, 64]"""
    B, T, _ = t.shape
    return t.reshape(B, T, H, HD).permute(0, 2, 1, 3)


def merge(t):
    """[B, H, T, 64] -> [B, T, H * 64]"""
    B, H, T, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, T, H * HD)


@dataclass
class Probe:
    B: int
    H: int
    Tq: int
    Tk: int
    causal: bool
    q_prescaled: bool
    q: torch.Tensor        # bf16 [B, Tq, D] view inside [B, Tq, 3D]
    k: torch.Tensor        # bf16 [B, Tk, D] view inside [B, Tk + GUARD, 2D]
    v: torch.Tensor
    do: torch.Tensor       # bf16 [B, Tq, D]
    qkv: torch.Tensor      # the buffers the views live in
    kv: torch.Tensor
    tgt: Optional[torch.Tensor]    # long [B, H, Tq, 2]: the two heavy keys of every row (equal where a row has one allowed key)
    decoy: Optional[torch.Tensor]  # long [Tq]: the key each row must not see (index into the guarded buffer)
    mass: dict

    @property
    def kbuf(self):
        return self.kv[..., :self.H * HD]

    @property
    def vbuf(self):
        return self.kv[..., self.H * HD:]

    @property
    def kappa(self):
        """natural-log score = kappa * (q as given) . k"""
        return LN2 if self.q_prescaled else SCALE

    def to(self, dev):
        qkv, kv, D = self.qkv.to(dev), self.kv.to(dev), self.H * HD
        return qkv[..., :D], kv[:, :self.Tk, :D], kv[:, :self.Tk, D:], self.do.to(dev)


# ------------------------------------------------------------------------------------------------ which keys carry the mass
def edge_keys(Tk):
    """non-causal: key 0, key Tk - 1, every multiple of 32 (hence of 64, 128, 256) below Tk and the key before each."""
    e = {0, Tk - 1}
    for t in range(0, Tk, 32):
        e.add(t)
        if t:
            e.add(t - 1)
    return sorted(e)


def causal_edge_candidates(i):
    """the last key at or before i that is a 32-, 64-, 128- or 256-multiple, or one less than such a multiple; without i itself"""
    c = set()
    for m in (32, 64, 128, 256):
        c.add(i // m * m)
        if (i + 1) // m:
            c.add((i + 1) // m * m - 1)
    c.discard(i)
    return sorted(c)


def _targets(B, H, Tq, Tk, causal):
    tgt = torch.zeros(B, H, Tq, 2, dtype=torch.long)
    if causal:
        used = {}
        for i in range(Tq):
            cand = causal_edge_candidates(i)
            b = min(cand, key=lambda e: (used.get(e, 0), -e)) if cand else i   # least used so far, then the latest
            used[b] = used.get(b, 0) + 1
            tgt[:, :, i, 0], tgt[:, :, i, 1] = i, b
        for i in range(Tq - 1):   # every edge key below the last row is some later row's second target
            for e in causal_edge_candidates(i + 1):
                assert used.get(e, 0) > 0 or e > Tq - 2, f"edge key {e} is no row's heavy key"
        decoy = torch.arange(1, Tq + 1)
    else:
        E = edge_keys(Tk)
        n = len(E)
        assert 2 * Tq >= n, f"{Tq} rows cannot cover {n} edge keys"
        Et = torch.tensor(E)
        for b in range(B):
            for h in range(H):
                off = 3 * (b * H + h)
                i = torch.arange(Tq)
                tgt[b, h, :, 0], tgt[b, h, :, 1] = Et[(2 * i + off) % n], Et[(2 * i + 1 + off) % n]
                assert set(tgt[b, h].flatten().tolist()) == set(E)
        decoy = torch.full((Tq,), Tk)
    return tgt, decoy


# ------------------------------------------------------------------------------------------------ operands
def _pack(B, H, Tq, Tk, q, k, v, do):
    """bf16 [B, H, T, 64] operands -> the model's packed layout (q inside [B, Tq, 3D], k / v inside [B, Tk + GUARD, 2D])"""
    D = H * HD
    g = torch.Generator().manual_seed(12345)
    qkv = torch.randn(B, Tq, 3 * D, generator=g).to(BF)
    qkv[..., :D] = merge(q)
    kv = torch.cat([merge(k), merge(v)], -1).contiguous()
    return qkv, kv, merge(do).contiguous()


def probe_case(B, H, Tq, Tk, causal, q_prescaled=False, seed=0):
    assert not causal or Tq == Tk
    g = torch.Generator().manual_seed(seed * 1000003 + Tq * 1009 + Tk * 31 + B * 7 + H + (500 if causal else 0))
    Tkg = Tk + GUARD
    u = torch.randn(B, H, Tkg, HD, generator=g, dtype=torch.float64)
    norm = torch.full((Tkg,), 8.0, dtype=torch.float64)
    if not causal:   # keys that are nobody's target or decoy stay in the background (causal: every key is its own row's target)
        norm[:Tk] = INTERIOR_NORM
        norm[edge_keys(Tk)] = 8.0
    k = (norm[:, None] * u / u.norm(dim=-1, keepdim=True)).to(BF)
    v = torch.randn(B, H, Tkg, HD, generator=g).to(BF)
    do = torch.randn(B, H, Tq, HD, generator=g).to(BF)
    tgt, decoy = _targets(B, H, Tq, Tk, causal)
    cols = torch.cat([tgt, decoy.view(1, 1, Tq, 1).expand(B, H, Tq, 1)], -1)                      # [B, H, Tq, 3]
    k64 = k.double()

    def rows_of(idx):   # the keys idx [B, H, Tq, n] names -> [B, H, Tq, n, 64]
        return torch.gather(k64[:, :, None].expand(B, H, Tq, Tkg, HD), 3, idx[..., None].expand(*idx.shape, HD))

    def solve(idx, want):   # minimum norm with q . k = want for the keys idx names
        kt = rows_of(idx)
        pinv = torch.linalg.pinv(kt)             # duplicate keys in idx make a consistent system: pinv solves it
        return (pinv @ want[..., None]).squeeze(-1), kt, pinv

    # Background keys score ~N(0, 3.6^2); over up to 1500 keys and a few thousand rows the tail reaches the targets' 16 in some
    # row.  So that the mass condition holds by construction, each row's highest background keys are capped: in PIN_ROUNDS
    # rounds the PIN_PER_ROUND highest allowed background keys join the row's constraints with min(their score, PIN_CAP).
    aligned = torch.full((B, H, Tq, 3), TARGET_SCORE / SCALE, dtype=torch.float64)
    idx, want = cols, aligned
    allowed = _allowed(Tq, Tk, causal)
    per_round = PIN_PER_ROUND
    for _ in range(PIN_ROUNDS + 1):
        q0, kt, pinv = solve(idx, want)
        if idx.shape[-1] + per_round > min(3 + PIN_ROUNDS * per_round, Tkg):
            break
        s1 = (q0 @ k64.transpose(-1, -2)).masked_fill(~allowed, -math.inf)
        s1.scatter_(3, idx, -math.inf)
        top = s1.topk(per_round, -1)
        keep = torch.isfinite(top.values)        # fewer allowed background keys than slots: repeat the row's first target
        idx = torch.cat([idx, torch.where(keep, top.indices, cols[..., :1])], -1)
        want = torch.cat([want, torch.where(keep, top.values.clamp(max=PIN_CAP / SCALE), aligned[..., :1])], -1)
    noise = torch.randn(B, H, Tq, HD, generator=g, dtype=torch.float64)
    q0 = q0 + (NOISE_CAUSAL if causal else NOISE) * (noise - (pinv @ (kt @ noise[..., None])).squeeze(-1))
    q = (q0 * ALPHA if q_prescaled else q0).to(BF)
    qkv, kv, dop = _pack(B, H, Tq, Tk, q, k, v, do)
    D = H * HD
    c = Probe(B, H, Tq, Tk, bool(causal), bool(q_prescaled), qkv[..., :D], kv[:, :Tk, :D], kv[:, :Tk, D:], dop, qkv, kv, tgt, decoy, {})
    _check_mass(c)
    return c


def randn_case(B, H, Tq, Tk, causal, seed=0):
    """the operands of the older tests (scores of standard deviation ~1, a nearly flat softmax) in the same container"""
    g = torch.Generator().manual_seed(seed * 7 + Tq + Tk)
    q, do = (torch.randn(B, H, Tq, HD, generator=g).to(BF) for _ in range(2))
    k, v = (torch.randn(B, H, Tk + GUARD, HD, generator=g).to(BF) for _ in range(2))
    qkv, kv, dop = _pack(B, H, Tq, Tk, q, k, v, do)
    D = H * HD
    return Probe(B, H, Tq, Tk, bool(causal), False, qkv[..., :D], kv[:, :Tk, :D], kv[:, :Tk, D:], dop, qkv, kv, None, None, {})


def _allowed(Tq, Tk, causal):
    j = torch.arange(Tk + GUARD)[None, :]
    m = (j < Tk).expand(Tq, -1).clone()
    if causal:
        m &= j <= torch.arange(Tq)[:, None]
    return m


def good_mask(c):
    """[Tq, Tk + GUARD] bool: what a row may see"""
    return _allowed(c.Tq, c.Tk, c.causal)


def _scores64(c):
    """natural-log scores over the guarded buffer, fp64, from the bits the kernel is handed"""
    return (heads(c.q, c.H).double() @ heads(c.kbuf, c.H).double().transpose(-1, -2)) * c.kappa


def _check_mass(c):
    s = _scores64(c)
    p = torch.softmax(s.masked_fill(~good_mask(c), -math.inf), -1)
    pt = torch.gather(p, 3, c.tgt)
    two = c.tgt[..., 0] != c.tgt[..., 1]
    both = torch.where(two, pt.sum(-1), pt[..., 0])
    each = torch.where(two, pt.amin(-1), pt[..., 0])
    leak = good_mask(c).clone()
    leak[torch.arange(c.Tq), c.decoy] = True
    pd = torch.softmax(s.masked_fill(~leak, -math.inf), -1)[:, :, torch.arange(c.Tq), c.decoy]
    c.mass = {"targets": both.min().item(), "each": each.min().item(), "decoy": pd.min().item()}
    assert c.mass["targets"] >= MIN_TARGET_MASS, f"a row's targets hold only {c.mass['targets']:.3f} of its mass"
    assert c.mass["each"] >= MIN_EACH_MASS, f"a target holds only {c.mass['each']:.3f} of its row's mass"
    assert c.mass["decoy"] >= MIN_EACH_MASS, f"a decoy would take only {c.mass['decoy']:.3f} of its row's mass"


# ------------------------------------------------------------------------------------------------ fp64 oracle
def oracle_fwd(c, dtype=torch.float64):
    """-> o [B, Tq, D], lse [B, H, Tq] (natural log).  Prescaled q: base 2 from the bits (q already carries scale * log2 e)."""
    q, k, v = (heads(t, c.H).to(dtype) for t in (c.q, c.k, c.v))
    s2 = (q @ k.transpose(-1, -2)) * (1.0 if c.q_prescaled else ALPHA)
    s2 = s2.masked_fill(~good_mask(c)[:, :c.Tk], -math.inf)
    m = s2.amax(-1, keepdim=True)
    p = torch.exp2(s2 - m)
    l = p.sum(-1, keepdim=True)
    return merge((p @ v) / l), ((m + torch.log2(l)) * LN2).squeeze(-1)


def oracle_bwd(c, o, lse, dtype=torch.float64):
    """The backward as a function of exactly what wft_attn_bwd_bf16 is given: P = exp(s - lse) with the SUPPLIED lse and
    delta = rowsum(o * do) with the SUPPLIED o.  dq is the gradient w.r.t. the unscaled projection (K.attn_bwd's docstring)."""
    q, k, v, do = (heads(t, c.H).to(dtype) for t in (c.q, c.k, c.v, c.do))
    s2 = (q @ k.transpose(-1, -2)) * (1.0 if c.q_prescaled else ALPHA)
    p = torch.exp2(s2 - lse.to(dtype).cpu()[..., None] * LOG2E).masked_fill(~good_mask(c)[:, :c.Tk], 0.0)
    delta = (heads(o.cpu(), c.H).to(dtype) * do).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(-1, -2) - delta)
    return merge(ds @ k) * SCALE, merge(ds.transpose(-1, -2) @ q) * c.kappa, merge(p.transpose(-1, -2) @ do)


# ------------------------------------------------------------------------------------------------ fp32 -> bf16 emulation
def _r(x):
    return x.to(BF).float()


def emulate_fwd(c, mask=None):
    """fp32 with the kernels' roundings (P to bf16 before P V, o to bf16; the row sum from the unrounded P), under `mask`
    [Tq, Tk + GUARD] over the guarded buffer (default: the correct one).  -> o bf16 [B, Tq, D], lse fp32 [B, H, Tq]"""
    mask = good_mask(c) if mask is None else mask
    q, k, v = (heads(t, c.H).float() for t in (c.q, c.kbuf, c.vbuf))
    s2 = q @ k.transpose(-1, -2)
    if not c.q_prescaled:
        s2 = s2 * torch.tensor(ALPHA, dtype=torch.float32)
    s2 = s2.masked_fill(~mask, -math.inf)
    m = s2.amax(-1, keepdim=True)
    p = torch.exp2(s2 - m)
    l = p.sum(-1, keepdim=True)
    return merge((_r(p) @ v) / l).to(BF), ((m + torch.log2(l)) * torch.tensor(LN2, dtype=torch.float32)).squeeze(-1)


def emulate_bwd(c, o, lse, mask=None, drop_q=None):
    """fp32 with the kernels' roundings (P and dS to bf16 before the MFMAs that consume them, outputs to bf16) on the supplied
    o / lse.  drop_q: query rows that contribute nothing to dK / dV.  -> dq [B, Tq, D], dk, dv [B, Tk, D] bf16"""
    mask = good_mask(c) if mask is None else mask
    q, k, v, do = (heads(t, c.H).float() for t in (c.q, c.kbuf, c.vbuf, c.do))
    s2 = q @ k.transpose(-1, -2)
    if not c.q_prescaled:
        s2 = s2 * torch.tensor(ALPHA, dtype=torch.float32)
    p = torch.exp2(s2 - lse.float()[..., None] * torch.tensor(LOG2E, dtype=torch.float32)).masked_fill(~mask, 0.0)
    delta = (heads(o, c.H).float() * do).sum(-1, keepdim=True)
    ds = _r(p * (do @ v.transpose(-1, -2) - delta))
    pb = _r(p)
    dq = merge(ds @ k) * SCALE
    if drop_q is not None:
        ds, pb = ds.clone(), pb.clone()
        ds[:, :, drop_q], pb[:, :, drop_q] = 0.0, 0.0
    dk = merge(ds.transpose(-1, -2) @ q) * torch.tensor(c.kappa, dtype=torch.float32)
    dv = merge(pb.transpose(-1, -2) @ do)
    return dq.to(BF), dk[:, :c.Tk].to(BF), dv[:, :c.Tk].to(BF)


# ------------------------------------------------------------------------------------------------ mutants
def mutants(c):
    """name -> (mask or None, dropped query rows or None): the kernels' tiling restated with one fault each — 128 queries per
    workgroup (forward, 8-wave backward), 256-row items (one-wave-per-SIMD backward), 32- / 64-key steps, 32-query dK/dV steps.
    A mutation never empties a row (such a row keeps the correct mask); a mutant that then changes nothing is left out."""
    good = good_mask(c)
    Tq, Tk = c.Tq, c.Tk
    i = torch.arange(Tq)
    out = {}

    def add(name, m):
        empty = ~m.any(-1)
        m[empty] = good[empty]
        if not torch.equal(m, good):
            out[name] = (m, None)

    if c.causal:
        m = good.clone(); m[i, i] = False
        add("diagonal dropped on all rows", m)
        m = good.clone(); r = i[i % 64 == 0]; m[r, r] = False
        add("diagonal dropped on rows that are multiples of 64", m)
        m = good.clone(); m[i, i + 1] = True
        add("key i+1 admitted on all rows", m)
        m = good.clone(); r = i[(i + 1) % 64 == 0]; m[r, r + 1] = True
        add("key i+1 admitted across 64-seams", m)
    else:
        m = good.clone(); m[:, Tk - 1] = False
        add("key Tk-1 dropped", m)
        m = good.clone(); m[:, Tk] = True
        add("key Tk admitted", m)
    m = good.clone(); m[:, torch.arange(0, Tk, 64)] = False
    add("first key of every 64-tile dropped", m)
    if Tk > 64:
        m = good.clone(); m[:, 64] = False
        add("key 64 dropped", m)
    b32 = max(0, (Tk - 1) // 32 - 1)
    m = good.clone(); m[:, 32 * b32:min(32 * b32 + 32, Tk)] = False
    add(f"32-key block {b32} dropped", m)
    s32 = max(0, (Tq - 1) // 32 - 1)
    out[f"32-query step {s32} dropped from dK/dV"] = (None, torch.arange(32 * s32, min(32 * s32 + 32, Tq)))
    return out


def probed(c, mask=None, drop_q=None):
    """-> (rows [B, H, Tq] bool, keys [B, H, Tk] bool): the query rows whose own target or decoy key the mutation touches, and the
    keys (inside the call's Tk) that are such a row's touched target or decoy."""
    cols = torch.cat([c.tgt, c.decoy.view(1, 1, c.Tq, 1).expand(c.B, c.H, c.Tq, 1)], -1)
    if mask is not None:
        diff = mask ^ good_mask(c)
        hit = diff[torch.arange(c.Tq)[None, None, :, None], cols]              # [B, H, Tq, 3]
    else:
        hit = torch.zeros_like(cols, dtype=torch.bool)
        hit[:, :, drop_q, :2] = True
    keys = torch.zeros(c.B, c.H, c.Tk + GUARD, dtype=torch.long).scatter_add_(2, cols.flatten(2), hit.flatten(2).long()) > 0
    rows = hit.any(-1) if mask is not None else torch.zeros(c.B, c.H, c.Tq, dtype=torch.bool)
    return rows, keys[..., :c.Tk]


# ------------------------------------------------------------------------------------------------ the bound
def row_ratios(got, ref, floor=FLOOR, atol=0.0):
    """got / ref [B, T, H * 64] -> [B, T, H]: max|err| over the 64 dims of each (row, head) / max(that row's own max|ref|,
    floor * the tensor's max|ref|); an error of at most atol counts as none."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    B, T, D = ref.shape
    err = (got - ref).abs().view(B, T, -1, HD).amax(-1)
    own = ref.abs().view(B, T, -1, HD).amax(-1)
    err = torch.where(err <= atol, torch.zeros_like(err), err)
    return err / torch.clamp(own, min=floor * ref.abs().max().item()).clamp_min(1e-300), err


def close_rows(got, ref, tol=TOL, floor=FLOOR, what="", atol=0.0):
    """Per (row, head), over the 64 dims: max|err| <= tol * max(own max|ref|, floor * tensor max|ref|).  A row cannot borrow the
    scale of another beyond the floor, which exists because some rows are exactly or nearly zero (causal row 0's dq, the dK / dV
    rows of keys that nobody targets).  atol: only for a tensor that is exactly zero as a whole (one key: dq = dk = 0, and fp32
    summation order leaves ~1e-8 — the atol tests/test_kernels_gpu.py test_attention_fwd_bwd uses there)."""
    ratio, err = row_ratios(got, ref, floor, atol)
    bad = ratio > tol
    print(f"{what}: worst (row, head) max|err| / max(own max|ref|, 2^{math.log2(floor):.0f} tensor max|ref|) = {ratio.max().item():.3e} "
          f"(tol {tol:.3e}), {int(bad.sum())} of {ratio.numel()} (row, head) pairs above it")
    assert torch.isfinite(got.detach().float()).all() and not bad.any(), \
        f"{what}: worst (row, head) {ratio.max().item():.3e} tol={tol:.3e}, first at (b, row, head) {bad.nonzero()[:4].tolist()}"
    return ratio


def close_lse(got, ref, what="lse"):
    """per row: |err| <= 1e-4 * max|lse ref|"""
    err = (got.detach().double().cpu() - ref.double()).abs()
    lim = LSE_TOL * ref.abs().max().item()
    print(f"{what}: worst row |err| = {err.max().item():.3e} (limit {lim:.3e}), {int((err > lim).sum())} of {err.numel()} rows above it")
    assert torch.isfinite(err).all() and (err <= lim).all(), f"{what}: worst row |err| {err.max().item():.3e} limit {lim:.3e}"
    return err


# ------------------------------------------------------------------------------------------------ the cases
# (Tq, Tk, causal) -> the kernels that serve it (forward: 1 plain / 2 pipelined; dQ, dK/dV: 8 waves / 4 = one wave per SIMD)
TABLE = [
    ((1, 1, 1), (1, 8, 8)), ((37, 37, 1), (1, 8, 8)), ((130, 130, 1), (1, 8, 8)), ((257, 257, 1), (1, 8, 8)), ((448, 448, 1), (1, 8, 8)),
    ((50, 333, 0), (1, 8, 8)), ((127, 77, 0), (1, 8, 8)),
    ((128, 70, 0), (1, 8, 4)), ((321, 257, 0), (1, 8, 4)),
    ((50, 1500, 0), (2, 8, 8)), ((33, 513, 0), (2, 8, 8)),
    ((129, 512, 0), (2, 8, 4)),
    ((513, 70, 0), (1, 4, 4)), ((512, 511, 0), (1, 4, 4)),
    ((640, 1500, 0), (2, 4, 4)),
]
GROUPS = ((1, 8), (3, 2))    # B * H a multiple of 8 (the XCD-aware item walk) and not
FORCED = [(129, 512, 0), (513, 70, 0), (640, 1500, 0)]                 # run again on the 8-wave / non-pipelined twins
PRESCALED = [(130, 130, 1), (50, 333, 0)] + [s for s, kern in TABLE if 4 in kern]
PRESCALED_CASES = [(*GROUPS[n % 2], *s) for n, s in enumerate(PRESCALED)]


def operand_cases():
    """every distinct (B, H, Tq, Tk, causal, q_prescaled) the GPU file builds operands for"""
    return [(B, H, *s, False) for s, _ in TABLE for B, H in GROUPS] + [(*c, True) for c in PRESCALED_CASES]
