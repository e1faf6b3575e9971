"""Probe operands for the single-token attention kernels (csrc/decode_attn.hip: attn_decode_kernel, attn_decode_beam_kernel<1, true>,
attn_decode_beam_kernel<W, false>, attn_decode_merge_kernel), their fp64 oracle, an fp32-softmax -> bf16 emulation that attends over
an explicit list of keys, and the ways such a kernel loses, leaks or double-counts one key restated as wrong lists ("mutants").
CPU only, plain torch; shared by tests/test_decode_probe_host.py (which proves on the CPU that the 2^-7 per-(row, head) bound passes
the correct emulation and fails every mutant) and tests/test_decode_probe_gpu.py (which holds every kernel and split regime to it).

Why structured operands: with randn operands one key of n carries 1 / n of a row's softmax mass, 1 / 448 .. 1 / 7700 here, below any
bound a bf16 output can be held to (tests/test_attn_bounds_host.py test_one_dropped_key_of_448_is_reported).  Here every (query row,
head) puts nearly all of its mass, in equal halves, on two keys at the edges of the kernels' dealing (key 0, n - 2, n - 1, every
multiple of 32 below n and the key before it: block seams, the 128-key wave seams, the split seams), and is aligned just as
strongly with decoys at the places a wrong kernel would read.  Losing a target, admitting a decoy or counting a target twice moves
that (row, head) by O(1) of its own size.

Construction, per (query row, head): q, the background keys and all values are randn rounded to bf16.  The two targets and every
decoy carry the SAME bf16 key bits k = bf16(gamma q) with gamma = 16 / (kappa |q|^2) computed on the bits of q as the kernel is handed
them (kappa = 0.125, or ln 2 for a prescaled q), so the natural-log score of each is 16 up to one rounding and — identical bits — the
scores are equal EXACTLY in whatever order a kernel sums the dot product.  Background keys score ~N(0, 1).  A correct kernel's output
is then (v_a + v_b) / 2 to about 1e-3.  Decoys (same key bits, a randn value row of their own):
  - position n of the row's own slot: the first row behind its n keys.  Caches are allocated [rows, cap + GUARD, 2D] and the call is
    given the [:, :cap] view, so the row of length cap has one too.  Grouped cross form: the first guard row of head h holds the
    decoy of query h % group of the audio.
  - self forms: the stale cache row at n - 1 (the true key n - 1 is the step's k_new / v_new row, a target in some (row, head) of
    every length).
  - beam self form: the row's OWN slot at each target position below n - 1 (the target itself sits in slot anc[r, position]).
The builder asserts in fp64, for every (row, head): the two targets hold >= 0.99 of the mass, each >= 0.45, and each decoy, were it
admitted, would hold >= 0.3; and over the calls of a case: every edge key of every length is a target somewhere.

A key is named by its index into the call's key pool: at(slot, position) for a cache row (guard rows included), new(r) for the
step's own row of query r.  The lists of the emulation and of the mutants hold such indices and may contain repeats.
"""
import functools
import math
from dataclasses import dataclass, field
from typing import Optional

import torch

from tests._attn_probe import GUARD, HD, LOG2E, SCALE, TARGET_SCORE
from tests.test_decode_kernels_gpu import _ref_decode

BF = torch.bfloat16
LN2 = math.log(2.0)
ALPHA = SCALE * LOG2E          # what a prescaled q carries; the kernels' qk_alpha for an unscaled one
BLOCK = 32                     # keys per block (DEC_BLOCK_KEYS)
WAVES = 4                      # block j belongs to wave j % 4 of split (j / 4) % nsplit
MIN_TARGET_MASS = 0.99         # the two targets together, of the (row, head)'s softmax
MIN_EACH_MASS = 0.45           # each target alone
MIN_DECOY_MASS = 0.3           # each decoy, were it admitted
MUTANT_MIN = 4 * 2.0 ** -7     # every (row, head) a mutant touches lies at least this far off (tests/test_decode_probe_host.py)


def expected_nsplit(rows, H, Tk):
    """The split rule include/wft.h states; rows: sequences (self forms) or audios (cross forms)."""
    return max(1, min(-(-256 // (rows * H)), -(-Tk // 512), 16))


# ------------------------------------------------------------------------------------------------ which keys carry the mass
def edge_keys(n, seam=BLOCK):
    """key 0, n - 2, n - 1, every multiple of `seam` below n and the key before it"""
    e = {0, n - 1, max(n - 2, 0)}
    for m in range(seam, n, seam):
        e |= {m, m - 1}
    return sorted(e)


def _pairs(E):
    """The edge keys in pairs, the i-th of the lower half with the i-th of the upper half: the two targets of a (row, head) then lie
    about n / 2 keys apart, in different blocks and mostly in different waves and splits, so a partial counted twice (which a
    pair inside one split would not notice: both halves double) moves the row.  An odd one out is paired with key 0."""
    h = len(E) // 2
    p = [(E[i], E[i + h]) for i in range(h)]
    if len(E) % 2:
        p.append((E[-1], E[0]))
    return p


class _Dealer:
    """Deals the pairs of every length in turn; `used`: positions already taken in the cache the (row, head) shares with others."""

    def __init__(self, seam):
        self.seam, self.next, self.seen = seam, {}, {}

    def pairs(self, n):
        return _pairs(edge_keys(n, self.seam))

    def take(self, n, used=()):
        ps = self.pairs(n)
        for _ in range(len(ps)):
            p = ps[self.next.get(n, 0) % len(ps)]
            self.next[n] = self.next.get(n, 0) + 1
            if not set(p) & set(used):
                self.seen.setdefault(n, set()).update(p)
                return p
        raise AssertionError(f"no pair of length {n} is free of the positions {sorted(used)}")

    def covered(self, n):
        return self.seen.get(n, set()) == set(edge_keys(n, self.seam))


# ------------------------------------------------------------------------------------------------ one call
@dataclass
class DecodeProbe:
    form: str              # "self" | "cross" | "beam_self" | "beam_cross"
    H: int
    cap: int               # the call's Tk
    R: int                 # query rows
    S: int                 # cache slots: R (self forms, greedy cross) or the audios (grouped cross)
    group: int
    lens: list             # keys per query row (cross forms: cap)
    nsplit: int
    prescaled: bool
    qkv: torch.Tensor      # bf16 [R, 3D]: q | k_new | v_new (the cross forms use q alone)
    buf: torch.Tensor      # bf16 [S, cap + GUARD, 2D]: k | v; the call is given buf[:, :cap]
    anc: Optional[torch.Tensor]   # beam self form: i32 [R, cap + GUARD]
    tgt: torch.Tensor      # long [R, H, 2]: the two target positions (equal where the row has one key)
    decoys: list = field(default_factory=list)   # [r][h] -> pool indices of the (row, head)'s decoys
    mass: dict = field(default_factory=dict)
    _cache: dict = field(default_factory=dict)

    @property
    def D(self):
        return self.H * HD

    @property
    def self_form(self):
        return self.form in ("self", "beam_self")

    @property
    def kappa(self):
        """natural-log score = kappa * (q as given) . k"""
        return LN2 if self.prescaled else SCALE

    @property
    def q(self):
        return self.qkv[:, :self.D]

    def at(self, slot, pos):
        return slot * (self.cap + GUARD) + pos

    def new(self, r):
        return self.S * (self.cap + GUARD) + r

    def own_slot(self, r):
        return r // self.group

    def anc_ok(self):
        """the ancestry table as the kernel uses it: an out-of-range entry names the row's own slot"""
        if "anc" not in self._cache:
            rows = torch.arange(self.R)[:, None].expand_as(self.anc)
            self._cache["anc"] = torch.where((self.anc >= 0) & (self.anc < self.R), self.anc.long(), rows)
        return self._cache["anc"]

    def keys(self, r, pos, slots=None):
        """pool indices of the logical keys `pos` (long tensor) of query row r: the cache row of the slot the form reads (`slots`
        overrides it), the step's own row at n - 1 in the self forms; a position behind n - 1 is read in the row's own slot."""
        n = self.lens[r]
        if slots is None:
            slots = torch.full_like(pos, self.own_slot(r))
            if self.form == "beam_self":
                slots = torch.where(pos < n - 1, self.anc_ok()[r, pos], slots)
        idx = self.at(slots, pos)
        return torch.where(pos == n - 1, torch.full_like(pos, self.new(r)), idx) if self.self_form else idx

    def lists(self):
        """[r] -> the keys a correct kernel attends over"""
        if "lists" not in self._cache:
            self._cache["lists"] = [self.keys(r, torch.arange(self.lens[r])) for r in range(self.R)]
        return self._cache["lists"]

    def pools(self, dtype):
        """k, v [pool, H, 64] in `dtype`: every cache row of every slot, then the step's own rows"""
        if ("pool", dtype) not in self._cache:
            D, H = self.D, self.H
            k, v = self.buf[..., :D].reshape(-1, H, HD), self.buf[..., D:].reshape(-1, H, HD)
            if self.self_form:
                k = torch.cat([k, self.qkv[:, D:2 * D].reshape(-1, H, HD)])
                v = torch.cat([v, self.qkv[:, 2 * D:].reshape(-1, H, HD)])
            self._cache["pool", dtype] = (k.to(dtype), v.to(dtype))
        return self._cache["pool", dtype]

    def scores(self, dtype):
        """[R, H, pool]: base-2 scores of every query row against the whole pool, as the kernels form them (dot * qk_alpha)"""
        if ("s", dtype) not in self._cache:
            k, _ = self.pools(dtype)
            s = torch.einsum("rhd,phd->rhp", self.q.reshape(self.R, self.H, HD).to(dtype), k)
            self._cache["s", dtype] = s if self.prescaled else s * torch.tensor(ALPHA, dtype=dtype)
        return self._cache["s", dtype]

    def heavy(self, r, h):
        """pool indices of the (row, head)'s targets and decoys"""
        return torch.cat([self.keys(r, self.tgt[r, h]), torch.tensor(self.decoys[r][h], dtype=torch.long)]).unique()

    def logical_cache(self):
        """bf16 [R, cap, 2D]: per query row, the keys a correct kernel reads, gathered (the step's own row in place)"""
        full = self.buf[:, :self.cap]
        if self.form == "beam_self":
            full = self.buf[self.anc_ok()[:, :self.cap], torch.arange(self.cap)[None, :]]
        elif self.form == "beam_cross":
            full = full.repeat_interleave(self.group, 0)
        full = full.clone()
        if self.self_form:
            for r, n in enumerate(self.lens):
                full[r, n - 1] = self.qkv[r, self.D:]
        return full

    def cache_after(self):
        """the whole buffer, guard rows and decoys included, as a correct call leaves it: the self forms write row n - 1 of slot r"""
        after = self.buf.clone()
        if self.self_form:
            for r, n in enumerate(self.lens):
                after[r, n - 1] = self.qkv[r, self.D:]
        return after

    def workspace_bytes(self):
        return 0 if self.nsplit == 1 else self.R * self.H * self.nsplit * 66 * 4


def _derangements(R, cols, g):
    """i32 [R, cols]: every column a permutation of the rows without a fixed point, so each slot position is read by one row"""
    out = torch.empty(R, cols, dtype=torch.int32)
    ar = torch.arange(R)
    for t in range(cols):
        while True:
            p = torch.randperm(R, generator=g)
            if not (p == ar).any():
                break
        out[:, t] = p
    return out


def _build_call(spec, lens, dealer, prescaled, seed, call):
    form, H, cap, group = spec["form"], spec["H"], spec["cap"], spec.get("group", 1)
    R, D = len(lens), H * HD
    S = R // group
    self_form = form in ("self", "beam_self")
    rows_of_split = R if self_form else S
    g = torch.Generator().manual_seed(seed * 1000003 + H * 7919 + cap * 31 + R * 977 + call * 101 + len(form) + 17 * group + (5 if prescaled else 0))
    qkv = torch.randn(R, 3 * D, generator=g).to(BF)
    if prescaled:
        qkv[:, :D] = (qkv[:, :D].float() * ALPHA).to(BF)
    buf = torch.randn(S, cap + GUARD, 2 * D, generator=g).to(BF)
    anc = None
    if form == "beam_self":
        n = lens[0]
        assert all(m == n for m in lens), "the rows of a beam self case share one length"
        anc = _derangements(R, cap + GUARD, g)
        anc[:, n - 1:] = torch.tensor([10 ** 6, -3, R] * (cap + GUARD))[:cap + GUARD - n + 1]
    c = DecodeProbe(form, H, cap, R, S, group, list(lens), expected_nsplit(rows_of_split, H, cap), bool(prescaled), qkv, buf, anc,
                    torch.zeros(R, H, 2, dtype=torch.long))
    assert c.nsplit == spec["nsplit"], f"{spec['id']}: the shape runs with {c.nsplit} splits, the table says {spec['nsplit']}"
    assert all(1 <= n <= cap for n in lens) and (self_form or all(n == cap for n in lens))

    # the targets: positions shared by the (row, head) pairs that read one cache must differ
    if form == "beam_self":
        units = [[(r, h) for r in range(R)] for h in range(H)]
    elif form == "beam_cross":
        units = [[(a * group + j, h) for j in range(group)] for a in range(S) for h in range(H)]
    else:
        units = [[(r, h)] for r in range(R) for h in range(H)]
    for unit in units:
        used = set()
        for r, h in unit:
            p = dealer.take(lens[r], used)
            used.update(p)
            c.tgt[r, h] = torch.tensor(p)

    # the aligned key bits of every (row, head), from the bits of q the kernel is handed
    qh = qkv[:, :D].reshape(R, H, HD).double()
    kt = (TARGET_SCORE / (c.kappa * (qh * qh).sum(-1)))[..., None] * qh
    kt = kt.to(BF)
    ar = anc is not None and c.anc_ok()
    c.decoys = [[[] for _ in range(H)] for _ in range(R)]
    for r in range(R):
        n, own = lens[r], c.own_slot(r)
        for h in range(H):
            hs = slice(h * HD, (h + 1) * HD)
            for t in set(c.tgt[r, h].tolist()):
                if self_form and t == n - 1:
                    qkv[r, D + h * HD:D + (h + 1) * HD] = kt[r, h]
                    continue
                slot = int(ar[r, t]) if form == "beam_self" else own
                buf[slot, t, hs] = kt[r, h]
                if form == "beam_self":    # the row's own slot at the target's position
                    buf[r, t, hs] = kt[r, h]
                    c.decoys[r][h].append(c.at(r, t))
            if form != "beam_cross" or r % group == h % group:    # the first row behind the n keys
                buf[own, n, hs] = kt[r, h]
                c.decoys[r][h].append(c.at(own, n))
            if self_form:    # the stale cache row at n - 1
                buf[r, n - 1, hs] = kt[r, h]
                c.decoys[r][h].append(c.at(r, n - 1))
    _check_mass(c)
    return c


def _check_mass(c):
    s = c.scores(torch.float64) * LN2
    both, each, decoy = [], [], []
    for r in range(c.R):
        good = c.lists()[r]
        lse = torch.logsumexp(s[r][:, good], -1)              # [H]
        for h in range(c.H):
            pt = torch.exp(s[r, h, c.keys(r, c.tgt[r, h])] - lse[h])
            one = c.tgt[r, h, 0] == c.tgt[r, h, 1]
            both.append(pt[0].item() if one else pt.sum().item())
            each.append(pt[0].item() if one else pt.min().item())
            for d in c.decoys[r][h]:
                decoy.append(1.0 / (1.0 + math.exp(lse[h].item() - s[r, h, d].item())))
    c.mass = {"targets": min(both), "each": min(each), "decoy": min(decoy)}
    assert c.mass["targets"] >= MIN_TARGET_MASS, f"a (row, head)'s targets hold only {c.mass['targets']:.4f} of its mass"
    assert c.mass["each"] >= MIN_EACH_MASS, f"a target holds only {c.mass['each']:.4f} of its (row, head)'s mass"
    assert c.mass["decoy"] >= MIN_DECOY_MASS, f"a decoy would take only {c.mass['decoy']:.4f} of its (row, head)'s mass"


# ------------------------------------------------------------------------------------------------ fp64 oracle, fp32 -> bf16 emulation
def oracle(c):
    """fp64 [R, D] from the bits the kernel is handed"""
    full = c.logical_cache()
    return _ref_decode(c.q, full[..., :c.D], full[..., c.D:], c.lens, c.H, c.kappa, dtype=torch.float64)


def emulate(c, lists=None, vlists=None, qrow=None, dtype=torch.float32):
    """Single-token attention over explicit key lists.  lists[r]: a long tensor of pool indices (repeats allowed) for all heads of
    query row r, or a list of H such tensors; vlists: where the VALUES are read if not at the same indices; qrow[r]: the row whose
    q query row r attends with.  fp32 softmax (base 2, as the kernels), the output rounded once to bf16 -> bf16 [R, D]; with
    dtype = float64 the unrounded result."""
    lists = c.lists() if lists is None else lists
    s_all, (_, vp) = c.scores(dtype), c.pools(dtype)
    out = torch.zeros(c.R, c.H, HD, dtype=dtype)
    for r in range(c.R):
        s_r = s_all[r if qrow is None else qrow[r]]
        kl, vl = lists[r], (lists if vlists is None else vlists)[r]
        per_head = [(h, kl[h], vl[h]) for h in range(c.H)] if isinstance(kl, list) else [(slice(None), kl, vl)]
        for h, ki, vi in per_head:
            s = s_r[h][..., ki]
            p = torch.exp2(s - s.amax(-1, keepdim=True))
            l = p.sum(-1, keepdim=True)
            v = vp[vi][:, h]
            out[r, h] = (torch.einsum("hn,nhd->hd", p, v) if p.dim() == 2 else p @ v) / l
    out = out.reshape(c.R, c.D)
    return out.to(BF) if dtype == torch.float32 else out


# ------------------------------------------------------------------------------------------------ mutants
def _block(t):
    return t // BLOCK


def mutants(c):
    """name -> dict(lists=, vlists=, qrow=): decode_attn.hip's dealing restated with one fault each.  A mutation never empties a
    row's list (such a row keeps the correct one); a mutant that changes no list is left out."""
    good = c.lists()
    R, H, ns = c.R, c.H, c.nsplit
    out = {}

    def add(name, lists=None, vlists=None, qrow=None):
        if lists is not None:
            for r in range(R):
                if isinstance(lists[r], list):
                    lists[r] = [x if x.numel() else good[r] for x in lists[r]]
                elif not lists[r].numel():
                    lists[r] = good[r]
        same = lists is None or all(torch.is_tensor(lists[r]) and torch.equal(lists[r], good[r]) for r in range(R))
        if same and vlists is None and qrow is None:
            return
        out[name] = dict(lists=good if lists is None else lists, vlists=vlists, qrow=qrow)

    def by_pos(keep):   # keep(r, n, t) -> bool tensor over the positions t, or a long tensor of positions
        res = []
        for r in range(R):
            n = c.lens[r]
            k = keep(r, n, torch.arange(n))
            res.append(c.keys(r, torch.arange(n)[k] if k.dtype == torch.bool else k))
        return res

    for i, which in enumerate("ab"):
        add(f"target {which} lost", [[good[r][good[r] != c.keys(r, c.tgt[r, h, i:i + 1])] for h in range(H)] for r in range(R)])
    add("n + 1: the guard decoy admitted", by_pos(lambda r, n, t: torch.arange(n + 1)))
    add("n - 1", by_pos(lambda r, n, t: t < n - 1))
    if c.self_form:
        stale = [torch.where(good[r] == c.new(r), torch.full_like(good[r], c.at(r, c.lens[r] - 1)), good[r]) for r in range(R)]
        add("stale cache row at len - 1, k and v", stale)
        add("stale cache row at len - 1, v only", None, vlists=stale)
    add("the clamped tail counted", by_pos(lambda r, n, t: torch.cat([t, torch.full((-n % BLOCK,), n - 1)])))
    for w in range(WAVES):
        add(f"wave {w}'s blocks dropped", by_pos(lambda r, n, t: _block(t) % WAVES != w))
    if ns > 1:
        for s in range(ns):
            add(f"split {s}'s partial dropped", by_pos(lambda r, n, t: _block(t) // WAVES % ns != s))
            add(f"split {s}'s partial merged twice", by_pos(lambda r, n, t: torch.cat([t, t[_block(t) // WAVES % ns == s]])))
    if c.form == "beam_self":
        add("anc ignored: own slot read", [c.keys(r, torch.arange(c.lens[r]), torch.full((c.lens[r],), r)) for r in range(R)])
        ahead = BLOCK * WAVES * ns
        shifted = []
        for r in range(R):
            n = c.lens[r]
            t = torch.arange(n)
            ta = t + ahead
            slots = torch.where(ta < n - 1, c.anc_ok()[r, ta.clamp(max=n - 1)], torch.full_like(t, r))
            shifted.append(c.keys(r, t, slots))
        add("the indices of block j + stride used for block j", shifted)
    if c.form == "beam_cross":
        add("the next audio's cache read", [c.keys(r, torch.arange(c.cap), torch.full((c.cap,), (c.own_slot(r) + 1) % c.S)) for r in range(R)])
        if c.group > 1:
            add("a group's queries all attend with row 0's q", qrow=[r // c.group * c.group for r in range(R)])
    return out


def _heavy_counts(kl, vl, hv, big):
    m = torch.isin(kl, hv)   # (the key decides the weight: a value read elsewhere matters only under a heavy key)
    u, n = torch.unique(kl[m] * big + vl[m], return_counts=True)
    return dict(zip(u.tolist(), n.tolist()))


def touched(c, lists, vlists=None, qrow=None):
    """bool [R, H]: the (row, head) pairs whose own targets or decoys the mutation concerns — the counts of its heavy (key, value)
    pairs are no multiple of the correct list's (counting every heavy key twice changes nothing), or it attends with another q."""
    good = c.lists()
    big = c.new(c.R) + 1
    out = torch.zeros(c.R, c.H, dtype=torch.bool)
    for r in range(c.R):
        for h in range(c.H):
            if qrow is not None and qrow[r] != r:
                out[r, h] = True
                continue
            kl = lists[r][h] if isinstance(lists[r], list) else lists[r]
            vl = kl if vlists is None else (vlists[r][h] if isinstance(vlists[r], list) else vlists[r])
            hv = c.heavy(r, h)
            a, b = _heavy_counts(good[r], good[r], hv, big), _heavy_counts(kl, vl, hv, big)
            if a.keys() != b.keys():
                out[r, h] = True
            else:
                k0 = next(iter(a))
                out[r, h] = any(b[k] * a[k0] != a[k] * b[k0] for k in a)
    return out


# ------------------------------------------------------------------------------------------------ the cases
ALL_448 = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 225, 256, 257, 416, 417, 447, 448]
ALL_1100 = [1, 33, 127, 128, 129, 511, 512, 513, 600, 1024, 1099, 1100]


def _spec(id, form, H, cap, nsplit, **kw):
    return dict(id=id, form=form, H=H, cap=cap, nsplit=nsplit, **kw)


# lens: the lengths of a greedy self case, each repeated over as many rows as its edge keys need; rows: a fixed number of rows per
# call (the split rule depends on it); max_rows: the rows are cut into calls of at most so many; seam: 128 = the reduced edge set
# of the 16-split cases (0, n - 2, n - 1, every multiple of 128 and the key before it)
SPECS = [
    _spec("1-self-H6-cap448", "self", 6, 448, 1, lens=ALL_448),
    _spec("2-self-H20-cap448", "self", 20, 448, 1, lens=[129, 417, 448]),
    _spec("3-self-H2-cap1100-split3", "self", 2, 1100, 3, lens=ALL_1100, max_rows=42),
    _spec("4-self-H20-B7-cap1100-split2", "self", 20, 1100, 2, lens=[129, 600, 1100], rows=7),
    *[_spec(f"5-cross-H6-B4-Tk{Tk}", "cross", 6, Tk, 1, rows=4) for Tk in (1, 31, 32, 33, 500)],
    _spec("6-cross-H6-B8-Tk1500-split3", "cross", 6, 1500, 3, rows=8),
    _spec("6-cross-H20-B7-Tk1500-split2", "cross", 20, 1500, 2, rows=7),
    _spec("7-cross-H2-B1-Tk7700-split16", "cross", 2, 7700, 16, rows=1, seam=128, prescaled=(False,)),
    _spec("8-beamcross-H2-A1-g8-Tk7700-split16", "beam_cross", 2, 7700, 16, rows=8, group=8, seam=128),
    *[_spec(f"9-beamcross-A2-H6-g{gr}-Tk{Tk}-split{ns}", "beam_cross", 6, Tk, ns, rows=2 * gr, group=gr)
      for gr in range(1, 9) for Tk, ns in ((500, 1), (1500, 3))],
    _spec("10-beamself-R10-H6-cap448-len417", "beam_self", 6, 448, 1, rows=10, n=417),
    _spec("10-beamself-R10-H6-cap448-len448", "beam_self", 6, 448, 1, rows=10, n=448),
    _spec("10-beamself-R4-H2-cap1100-len1100-split3", "beam_self", 2, 1100, 3, rows=4, n=1100),
]
SPEC = {s["id"]: s for s in SPECS}
CASES = [(s["id"], pre) for s in SPECS for pre in s.get("prescaled", (False, True))]
IDS = [f"{i}-pre{int(pre)}" for i, pre in CASES]
MAX_CALLS = 40


CLAMP_LENS = ([33, 1, 64], [33, 0, 64 + 5])   # what the rows must behave as, and the `len` the kernel is given


def clamp_case(prescaled, seed=0):
    """The documented "len clamped to 1..Tk" (H = 2, cap 64): operands built for the lengths the rows must BEHAVE as.  Row 1 is not
    the first and the GUARD rows outnumber the overshoot of row 2, so even a missing clamp stays inside the allocation."""
    assert GUARD > CLAMP_LENS[1][2] - 64
    return _build_call(dict(id="clamp", form="self", H=2, cap=64, nsplit=1), CLAMP_LENS[0], _Dealer(BLOCK), prescaled, seed, 0)


def _row_plan(spec):
    """-> the lengths of the rows of every call, or None where calls are added until every edge key is a target"""
    if spec["form"] != "self":
        return None
    H, rows = spec["H"], []
    for n in spec["lens"]:
        rows += [(i, n) for i in range(-(-len(_pairs(edge_keys(n))) // H))]
    lens = [n for _, n in sorted(rows)]   # repeat-major: a call mixes short and long rows
    per = spec.get("rows") or spec.get("max_rows") or len(lens)
    i = 0
    while spec.get("rows") and len(lens) % per:   # a fixed batch is filled up with further rows of the case's lengths
        lens.append(spec["lens"][i % len(spec["lens"])])
        i += 1
    return [lens[i:i + per] for i in range(0, len(lens), per)]


@functools.lru_cache(maxsize=4)
def calls(case_id, prescaled, seed=0):
    """The calls of a case (list of DecodeProbe): together they make every edge key of every length a target somewhere."""
    spec = SPEC[case_id]
    dealer = _Dealer(spec.get("seam", BLOCK))
    plan = _row_plan(spec)
    out = []
    if plan is not None:
        out = [_build_call(spec, lens, dealer, prescaled, seed, i) for i, lens in enumerate(plan)]
        lengths = spec["lens"]
    else:
        n = spec.get("n", spec["cap"])
        lengths = [n]
        while not dealer.covered(n):
            assert len(out) < MAX_CALLS, f"{case_id}: {MAX_CALLS} calls do not cover the edge keys"
            out.append(_build_call(spec, [n] * spec["rows"], dealer, prescaled, seed, len(out)))
    for n in lengths:
        assert dealer.covered(n), f"{case_id}: edge keys {sorted(set(edge_keys(n, dealer.seam)) - dealer.seen.get(n, set()))} of length {n} are no target"
    return out
