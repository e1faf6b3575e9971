"""Cases, float64 reference, per-element bounds and float32 restatements for the loss-head kernels: wft_ce_fwd, wft_ce_bwd and
wft_token_stats (csrc/loss.hip) and their fp32-mode twins wft_ce_fwd_f32 / wft_ce_bwd_f32 (csrc/f32.hip).  Shared by
tests/test_loss_head_host.py (CPU: the bound accepts the kernels' arithmetic and rejects every listed mutant of it) and
tests/test_loss_head_gpu.py (the kernels themselves under the same checker).

Cases (`cases()`): V in 13, 1000, 2051, 51865, 51866 with ld = round_up(V, 128); rows 1, 50 and 600 (600 at V = 1000 and 2051 only,
8 at the two production sizes).  Row r of a case is of kind kinds[(r + offset) % len(kinds)]: the value kinds of VALUE_KINDS and one
planted tie of the maximum per entry of `tie_pairs(V)`; every row's padding columns [V, ld) hold POISON, a finite value above
every real logit, so a padding column that leaks into the max, the sum-exp, sum x or the argmax moves the result by much more
than 1 / V.  Every 7th row (r % 7 == 6) is ignored (-100); the others aim at column 0, column V - 1, the row's special column
(the dominant one, the lower tied one) or a fixed other column in turn.  Each case exists twice: `x` holds bf16-representable
values (both modes), `x32` the same rows without the rounding (fp32 mode only).

Reference (`reference()`): float64 closed forms — logsumexp, softmax, loss, gradient — not autograd.

Bounds (`check()`): per element, from the reference alone.  With u = 2^-24, p = softmax, mx = the row maximum, t the target:
  F_lse     = u (|lse| + |mx| + 1 + sum_c p_c |x_c - mx|)
  F_loss    = F_lse + u (|lse| + |x_t|) + eps u (|lse| + mean_c|x_c| sqrt(V / 256 + 8))      (valid rows; ignored rows: exactly 0)
              the last term is sum x / V: every column's path to the total is V / 256 adds in its thread plus 8 tree steps, each
              rounded at the magnitude of the partial sum (mean|x| per summand after the division by V); roundings add up as the
              square root of their number.  It is what the rows shifted by +-300 need.
  F_stats0  = sum_valid F_loss + u sum_valid |loss|
  F_dlogits = coef (p (1 + |x - lse|) + eps / V + onehot) u,  coef = gscale / n_valid
  F_ex      = u (sum_c p_c |x_c| (2 + |x_c - mx|) + |E_p[x]|)                                 (token_stats column 2)
and the bound of an output is K[output] * F (dlogits of the bf16 mode: bf16 round-to-nearest of the reference, that is half an ulp
of bf16 at ref = 2^-9 times the power of two above |ref|, plus K F).  Exact, no tolerance: argmax, stats[1], token_stats columns 1 (the maximum is a selection) and 3, row_loss and
dlogits of ignored rows (zero), the padding columns of dlogits (zero in bf16 mode whatever the input held, untouched in fp32 mode).

The constants K are not chosen: test_loss_head_host.py restates both kernels' arithmetic in torch CPU float32, in the kernels'
order of operations (256 threads, 8-wide vectors, online max / sum-exp, xor-butterfly per wave, four waves in order; fp32 twin:
two passes, butterfly sums), measures max |restatement - reference| / F over all cases and both restatements, and K is 4 x that
(the GPU's __expf / __logf are looser than the CPU's expf), rounded up to a power of two.  Measured (seed 0, all cases):

  output     worst ratio bf16-kernel restatement   worst ratio fp32-twin restatement   4 x worst   K
  lse        0.889                                 0.889                               3.56        4
  loss       0.679                                 0.773                               3.09        4
  stats0     0.144                                 0.332                               1.33        2
  dlogits    109.6                                 109.6                               438.5       512
  ex         2.277                                 -                                   9.11        16

(dlogits is large because F_dlogits, as given, has no term for the rounding of lse itself: on the rows shifted by +-300
half an ulp of lse is 1.5e-5 = 256 u, which enters every p_c as p_c * 256 u where p_c (1 + |x_c - lse|) u offers (1 + 7..12) u.)
"""
import dataclasses
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
POISON = 9984.0   # bf16(1e4)
IGNORE = -100
VOCABS = (13, 1000, 2051, 51865, 51866)
EPS_GSCALE = ((0.0, 1.0), (0.05, 0.25), (0.1, 1.0), (0.1, 0.25), (0.05, 1.0), (0.0, 0.25))
VALUE_KINDS = ("randn x 3", "randn", "constant", "dominant at the target", "dominant elsewhere", "shifted +300", "shifted -300",
               "maximum in column V - 1")
K = {"lse": 4.0, "loss": 4.0, "stats0": 2.0, "dlogits": 512.0, "ex": 16.0}

MUTANTS = ("smoothing term dropped from the gradient", "smoothing divided by ld", "sum x of the loss over ld columns",
           "a padding column admitted to the max", "coef from the total row count", "ignored rows in stats[0]",
           "highest index on ties", "ties by wave order, not by index", "tail columns dropped from the sum-exp",
           "tail columns dropped from the argmax", "one-hot at t + 1", "1 - eps replaced by 1")


def round_up(v, m):
    return (v + m - 1) // m * m


def owner(c, V):
    """thread of the 256 that reads column c in ce_fwd_kernel / token_stats_kernel: vector i = c // 8 goes to thread i % 256, the
    tail column c >= (V // 8) * 8 to thread c - (V // 8) * 8."""
    t0 = (V >> 3) << 3
    return (c >> 3) % 256 if c < t0 else c - t0


def tie_pairs(V):
    """(name, lower column, higher column) of the planted ties that fit V.  'crossed': the lower column sits in the later lane /
    wave, so a merge that lets the first (or the last) lane or wave win regardless of the index picks the higher column."""
    nv, t0 = V >> 3, (V >> 3) << 3
    tail = V - t0
    out = [("columns i, i + 1 of one 8-vector", 2, 3)]
    if nv >= 2:
        out.append(("one in-vector position, two lanes of a wave", 5, 13))
    if nv > 67:
        out.append(("two waves", 8 * 3 + 1, 8 * 67 + 1))
    if tail:
        out.append(("vector part and tail, one thread", 4, t0))
    if tail and nv > 70:
        out.append(("vector part (wave 1) and tail (wave 0), crossed", 8 * 70 + 6, V - 1))
    if tail >= 2:
        out.append(("two tail columns", t0, V - 1))
    if nv > 261:
        out.append(("two lanes, crossed", 8 * 7, 8 * 261))
    if nv > 300:
        out.append(("two waves, crossed", 8 * 100 + 7, 8 * 300 + 7))
    for _, a, b in out:
        assert 0 <= a < b < V
    return out


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    V: int
    ld: int
    rows: int
    eps: float
    gscale: float
    kinds: tuple          # kind of every row
    x: torch.Tensor       # f32 [rows, ld], every value bf16-representable, padding = POISON
    x32: torch.Tensor     # f32 [rows, ld], the same rows without the rounding to bf16
    targets: torch.Tensor  # i64 [rows]


def _rows(V, ld, rows, kinds, off, seed, q, top, dom_v, const_v, shift):
    raw = torch.randn(rows, V, generator=torch.Generator().manual_seed(seed))
    x = torch.full((rows, ld), POISON)
    ties = {f"tie: {n}": (a, b) for n, a, b in tie_pairs(V)}
    tg = torch.empty(rows, dtype=torch.int64)
    names = []
    for r in range(rows):
        kind = kinds[(r + off) % len(kinds)]
        names.append(kind)
        row = q(raw[r])
        special = (11 * r + 3) % V
        dom = (37 * r + 5) % V
        if kind == "randn x 3":
            row = q(raw[r] * 3)
        elif kind == "constant":
            row = torch.full((V,), const_v)
        elif kind.startswith("dominant"):
            row[dom] = dom_v
            special = dom
        elif kind == "shifted +300":
            row = q(raw[r] + shift)
        elif kind == "shifted -300":
            row = q(raw[r] - shift)
        elif kind == "maximum in column V - 1":
            row[V - 1] = q(row.max() + 2)
        elif kind in ties:
            a, b = ties[kind]
            row[a] = row[b] = top
            special = a
        elif kind != "randn":
            raise KeyError(kind)
        x[r, :V] = row
        t = (0, V - 1, special, (5 * r + 1) % V)[r % 4]
        if kind == "dominant at the target":
            t = dom
        elif kind == "dominant elsewhere" and t == dom:
            t = (dom + 1) % V
        tg[r] = IGNORE if r % 7 == 6 else t
    return x, tg, tuple(names)


def _bfq(t):
    return t.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for V in VOCABS:
        ld = round_up(V, 128)
        ties = tuple(f"tie: {n}" for n, _, _ in tie_pairs(V))
        if V >= 51865:   # at most 8 rows each: the value kinds, then the ties
            plan = [(8, VALUE_KINDS, "values"), (len(ties), ties, "ties")]
        else:
            plan = [(n, VALUE_KINDS + ties, "all kinds") for n in {13: (1, 50), 1000: (1, 50, 600), 2051: (50, 600)}[V]]
        for rows, kinds, what in plan:
            i = len(out)
            eps, gscale = EPS_GSCALE[i % len(EPS_GSCALE)]
            off = 3 * (i % 5) if rows > 1 else 0
            x, tg, names = _rows(V, ld, rows, kinds, off, i, _bfq, 8.0, 40.0, 1.5, 300.0)
            x32, tg32, _ = _rows(V, ld, rows, kinds, off, i, lambda t: t.clone(), 8.1, 40.3, 1.1, 300.123)
            assert torch.equal(tg, tg32) and torch.equal(_bfq(x), x) and rows <= (8 if V >= 51865 else 600)
            out.append(Case(f"V{V}-r{rows}-{what}-eps{eps}-g{gscale}", V, ld, rows, eps, gscale, names, x, x32, tg))
    return tuple(out)


def all_ignored_case():
    """the all-ignored batch: stats = {0, 0}, every gradient zero (coef = gscale / max(n_valid, 1) times valid = 0)."""
    c = cases()[3]
    return dataclasses.replace(c, name=c.name + "-all-ignored", targets=torch.full_like(c.targets, IGNORE))


# ------------------------------------------------------------------------------------------------ float64 reference and bounds
def reference(x, targets, V, eps, gscale):
    """float64 closed forms on the V real columns of x [rows, ld] -> dict of references and of the bound forms F (see the top)."""
    x64 = x[:, :V].double()
    rows = x64.shape[0]
    mx = x64.max(1).values
    lse = torch.logsumexp(x64, 1)
    p = (x64 - lse[:, None]).exp()
    valid = (targets >= 0) & (targets < V)
    n_valid = int(valid.sum())
    tc = targets.clamp(0, V - 1)
    xt = x64.gather(1, tc[:, None])[:, 0]
    zero = torch.zeros((), dtype=torch.float64)
    loss = torch.where(valid, (1 - eps) * (lse - xt) + eps * (lse - x64.sum(1) / V), zero)
    onehot = torch.zeros_like(x64)
    onehot[torch.arange(rows)[valid], targets[valid]] = 1.0
    coef = gscale / max(n_valid, 1)
    dl = coef * (p - eps / V - (1 - eps) * onehot) * valid[:, None]
    col = torch.arange(V).expand(rows, V)
    argmax = torch.where(x64 == mx[:, None], col, torch.full_like(col, V)).min(1).values   # lowest index on ties
    ex = (p * x64).sum(1)
    f_lse = U * (lse.abs() + mx.abs() + 1 + (p * (x64 - mx[:, None]).abs()).sum(1))
    f_loss = torch.where(valid, f_lse + U * (lse.abs() + xt.abs()) + eps * U * (lse.abs() + x64.abs().mean(1) * math.sqrt(V / 256 + 8)), zero)
    return {
        "lse": lse, "loss": loss, "stats0": loss.sum(), "n_valid": n_valid, "dlogits": dl, "argmax": argmax, "valid": valid,
        "max": mx, "ex": ex, "xt": torch.where(valid, xt, zero),
        "F": {"lse": f_lse, "loss": f_loss, "stats0": f_loss.sum() + U * loss.abs().sum(),
              "dlogits": coef * (p * (1 + (x64 - lse[:, None]).abs()) + eps / V + onehot) * U * valid[:, None],
              "ex": U * ((p * x64.abs() * (2 + (x64 - mx[:, None]).abs())).sum(1) + ex.abs())},
    }


@functools.lru_cache(maxsize=None)
def case_reference(case, fp32_values=False):
    """computed once per (case, operand variant) and shared; nobody writes to it."""
    return reference(case.x32 if fp32_values else case.x, case.targets, case.V, case.eps, case.gscale)


def bf16_half_ulp(ref):
    """what bf16 round-to-nearest of ref may be off by: 2^-9 times the power of two above |ref| (2^-9 |ref| .. 2^-8 |ref|; as a
    plain factor on |ref|, 2^-9 would refuse correct rounding just above a power of two, where the relative error reaches 2^-8)."""
    _, e = torch.frexp(ref.abs())   # |ref| = m 2^e, 0.5 <= m < 1
    return torch.where(ref != 0, torch.ldexp(torch.ones_like(ref), e - 9), torch.zeros_like(ref))


def ratio(got, ref, bound):
    """worst |got - ref| / bound over the elements; where the bound is 0 the element has to be exact (inf otherwise); NaN -> inf."""
    got, ref, bound = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double(), torch.as_tensor(bound).double()
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return r.max().item() if r.numel() else 0.0


def check(case, out, *, fp32_mode=False, fp32_values=False, k=None, limit=1.0, what=""):
    """Every output present in `out` against the reference of `case`: the exact ones exactly, the others per element against
    K * F (see the top).  -> {output: worst ratio}.  Raises AssertionError naming everything that is wrong.
    Keys of out: row_loss, row_lse [rows]; stats [2]; argmax [rows]; dlogits [rows, ld] (bf16 values, or fp32 with fp32_mode);
    dlogits_f32 [rows, ld] (a bf16-mode restatement before its rounding: against K F alone); tstats [rows, 4]; targmax [rows]."""
    k = K if k is None else k
    ref = case_reference(case, fp32_values)
    F, V, valid = ref["F"], case.V, ref["valid"]
    worst, wrong = {}, []

    def exact(name, got, want):
        if not torch.equal(torch.as_tensor(got).cpu().double(), torch.as_tensor(want).double()):
            g, w = torch.as_tensor(got).cpu().double().reshape(-1), torch.as_tensor(want).double().reshape(-1)
            i = int((g != w).nonzero()[0]) if g.shape == w.shape else -1
            wrong.append(f"{name} is not exact (first at flat index {i}: got {g[i].item() if i >= 0 else g.shape}, want {w[i].item() if i >= 0 else w.shape})")

    def within(name, got, want, bound):
        worst[name] = ratio(got, want, bound)
        if not worst[name] <= limit:
            wrong.append(f"{name}: worst |err| / bound = {worst[name]:.3e} > {limit}")

    if "row_lse" in out:
        within("row_lse", out["row_lse"], ref["lse"], k["lse"] * F["lse"])
    if "row_loss" in out:
        within("row_loss", out["row_loss"], ref["loss"], k["loss"] * F["loss"])
        exact("row_loss of ignored rows", torch.as_tensor(out["row_loss"]).cpu()[~valid], torch.zeros(int((~valid).sum())))
    if "stats" in out:
        within("stats[0]", out["stats"][0], ref["stats0"], k["stats0"] * F["stats0"])
        exact("stats[1]", out["stats"][1], torch.tensor(float(ref["n_valid"])))
    if "argmax" in out:
        exact("argmax", out["argmax"], ref["argmax"])
    for name in ("dlogits", "dlogits_f32"):
        if name in out:
            dl = torch.as_tensor(out[name]).cpu().double()
            rn = 0.0 if (fp32_mode or name == "dlogits_f32") else 1.0
            within(name, dl[:, :V], ref["dlogits"], rn * bf16_half_ulp(ref["dlogits"]) + k["dlogits"] * F["dlogits"])
            exact(f"{name} of ignored rows", dl[:, :V][~valid], torch.zeros(int((~valid).sum()), V))
            exact(f"{name} padding columns", dl[:, V:], torch.full((case.rows, case.ld - V), POISON if fp32_mode else 0.0))
    if "tstats" in out:
        ts = torch.as_tensor(out["tstats"]).cpu()
        within("tstats lse", ts[:, 0], ref["lse"], k["lse"] * F["lse"])
        exact("tstats max", ts[:, 1], ref["max"])
        within("tstats E_p[x]", ts[:, 2], ref["ex"], k["ex"] * F["ex"])
        exact("tstats x_target", ts[:, 3], ref["xt"])
    if "targmax" in out:
        exact("token_stats argmax", out["targmax"], ref["argmax"])
    assert not wrong, f"{what} {case.name}: " + "; ".join(wrong)
    return worst


# ------------------------------------------------------------------------------------------------ float32 restatements (CPU)
_NEG = -3.0e38
_F = torch.float32


def _f32(v):
    return float(np.float32(v))


def _butterfly(state, merge):
    """the 6 __shfl_xor steps of a wave reduction on [rows, 256] thread states (xor below 64 stays inside a wave)."""
    lane = torch.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        state = merge(state, tuple(a[:, lane ^ o] for a in state))
    return state


def _argmax_rule(x, V, mut):
    rows = x.shape[0]
    n = V
    if mut == "tail columns dropped from the argmax":
        n = (V >> 3) << 3
    if mut == "a padding column admitted to the max":
        n = V + 1
    xs = x[:, :n]
    col = torch.arange(n).expand(rows, n)
    mx = xs.max(1, keepdim=True).values
    if mut == "highest index on ties":
        return torch.where(xs == mx, col, torch.full_like(col, -1)).max(1).values, mx[:, 0]
    if mut == "ties by wave order, not by index":   # lowest index inside a wave; across the waves the first one with the maximum
        wave = torch.tensor([owner(c, V) >> 6 for c in range(n)])
        best_v, best_i = torch.full((rows,), _NEG), torch.full((rows,), 0x7fffffff)
        for w in range(4):
            vals = torch.where(wave == w, xs, torch.full_like(xs, _NEG))
            wv = vals.max(1, keepdim=True).values
            wi = torch.where(vals == wv, col, torch.full_like(col, 0x7fffffff)).min(1).values
            take = wv[:, 0] > best_v
            best_v, best_i = torch.where(take, wv[:, 0], best_v), torch.where(take, wi, best_i)
        return best_i, best_v
    return torch.where(xs == mx, col, torch.full_like(col, n)).min(1).values, mx[:, 0]


def _threads_online(x, V, per_element, mut):
    """the per-thread loops of ce_fwd_kernel (per_element False: the vector's max first, then its 8 exps) or token_stats_kernel
    (True: one online step per element, carrying w = sum exp(x - m) x) -> m, s, sumx, w as [rows, 256]."""
    rows = x.shape[0]
    nv = V >> 3
    t0 = nv << 3
    P = (nv + 255) // 256
    m = torch.full((rows, 256), _NEG, dtype=_F)
    s = torch.zeros(rows, 256, dtype=_F)
    sumx, w = s.clone(), s.clone()
    xp = torch.zeros(rows, P * 256 * 8, dtype=_F)
    xp[:, :t0] = x[:, :t0]
    xp = xp.view(rows, P, 256, 8)
    vec = torch.arange(256)

    def push(v, act):
        nonlocal m, s, w
        up = act & (v > m)
        f = torch.exp(m - v)
        s, w, m = torch.where(up, s * f, s), torch.where(up, w * f, w), torch.where(up, v, m)
        e = torch.exp(v - m)
        s, w = torch.where(act, s + e, s), torch.where(act, w + e * v, w)

    for p in range(P):
        act = (p * 256 + vec < nv).expand(rows, 256)
        v = xp[:, p]
        if not per_element:
            cm = v.max(-1).values
            up = act & (cm > m)
            s, m = torch.where(up, s * torch.exp(m - cm), s), torch.where(up, cm, m)
        for e in range(8):
            sumx = torch.where(act, sumx + v[..., e], sumx)
            if per_element:
                push(v[..., e], act)
            else:
                s = torch.where(act, s + torch.exp(v[..., e] - m), s)
    if V > t0:
        v = torch.zeros(rows, 256, dtype=_F)
        v[:, :V - t0] = x[:, t0:V]
        act = (vec < V - t0).expand(rows, 256)
        sumx = torch.where(act, sumx + v, sumx)
        if mut != "tail columns dropped from the sum-exp":
            push(v, act)
    return m, s, sumx, w


def _merge_msxw(a, b):
    m, s, sumx, w = a
    om, os_, osx, ow = b
    nm = torch.maximum(m, om)
    f0, f1 = torch.exp(m - nm), torch.exp(om - nm)
    return nm, s * f0 + os_ * f1, sumx + osx, w * f0 + ow * f1


def _block_online(x, V, per_element, mut):
    st = _butterfly(_threads_online(x, V, per_element, mut), _merge_msxw)
    acc = tuple(a[:, 0:1] for a in st)
    for wv in (64, 128, 192):
        acc = _merge_msxw(acc, tuple(a[:, wv:wv + 1] for a in st))
    return tuple(a[:, 0] for a in acc)


def _reduce(row_loss, take):
    """ce_reduce_kernel: thread t adds rows t, t + 256, ... in order, then a 128..1 tree over the 256 partial sums."""
    rows = row_loss.shape[0]
    P = (rows + 255) // 256
    lp = torch.zeros(P * 256, dtype=_F)
    lp[:rows] = torch.where(take, row_loss, torch.zeros((), dtype=_F))
    cp = torch.zeros(P * 256, dtype=_F)
    cp[:rows] = take.float()
    sl, sc = torch.zeros(256, dtype=_F), torch.zeros(256, dtype=_F)
    for p in range(P):
        sl, sc = sl + lp[p * 256:(p + 1) * 256], sc + cp[p * 256:(p + 1) * 256]
    o = 128
    while o:
        sl, sc = sl.clone(), sc.clone()
        sl[:o] += sl[o:2 * o]
        sc[:o] += sc[o:2 * o]
        o >>= 1
    return sl[0], sc[0]


def _loss_and_grad(x, lse, X, targets, V, ld, eps, gscale, mut, exp_cols):
    """the tail of the forward (row loss, reduction) and the whole backward, shared by both restatements; exp_cols = ld: bf16 kernel
    (writes zeros to the padding), V: fp32 twin (leaves the padding alone)."""
    rows = x.shape[0]
    valid = (targets >= 0) & (targets < V)
    xt = x.gather(1, targets.clamp(0, V - 1)[:, None])[:, 0]
    ome = 1.0 if mut == "1 - eps replaced by 1" else _f32(np.float32(1) - np.float32(eps))
    eps32 = _f32(eps)
    full = ome * (lse - xt) + eps32 * (lse - X / _f32(V))
    zero = torch.zeros((), dtype=_F)
    row_loss = torch.where(valid, full, zero)
    s0, s1 = _reduce(full if mut == "ignored rows in stats[0]" else row_loss, torch.ones_like(valid) if mut == "ignored rows in stats[0]" else valid)
    if mut == "ignored rows in stats[0]":
        s1 = valid.float().sum()
    n = float(rows) if mut == "coef from the total row count" else max(float(s1), 1.0)
    coef = torch.where(valid, torch.tensor(_f32(np.float32(gscale) / np.float32(n))), zero)
    sm = 0.0 if mut == "smoothing term dropped from the gradient" else _f32(np.float32(eps) / np.float32(ld if mut == "smoothing divided by ld" else V))
    g = torch.exp(x[:, :V] - lse[:, None]) - sm
    hot = targets + 1 if mut == "one-hot at t + 1" else targets
    sel = valid & (hot < V)
    g[torch.arange(rows)[sel], hot[sel]] -= ome
    g = g * coef[:, None]
    dl = x.clone() if exp_cols == V else torch.zeros(rows, ld, dtype=_F)
    dl[:, :V] = g
    return row_loss, torch.stack([s0, s1]), dl


def restate_bf16(case, mut=None):
    """wft_ce_fwd + wft_ce_bwd + wft_token_stats in CPU float32, in the kernels' order; mut: one of MUTANTS, or None."""
    assert mut is None or mut in MUTANTS
    x, V, ld = case.x, case.V, case.ld
    m, s, X, _ = _block_online(x, V, False, mut)
    tm, ts, _, tw = _block_online(x, V, True, mut)
    if mut == "a padding column admitted to the max":
        nm = torch.maximum(m, x[:, V])
        s, m = s * torch.exp(m - nm), nm
        ts, tw, tm = ts * torch.exp(tm - nm), tw * torch.exp(tm - nm), nm
    if mut == "sum x of the loss over ld columns":
        X = X + x[:, V:].sum(1)
    lse = m + torch.log(s)
    am, bv = _argmax_rule(x, V, mut)
    row_loss, stats, g = _loss_and_grad(x, lse, X, case.targets, V, ld, case.eps, case.gscale, mut, ld)
    valid = (case.targets >= 0) & (case.targets < V)
    xt = torch.where(valid, x.gather(1, case.targets.clamp(0, V - 1)[:, None])[:, 0], torch.zeros((), dtype=_F))
    return {"row_loss": row_loss, "row_lse": lse, "stats": stats, "argmax": am, "dlogits_f32": g, "dlogits": _bfq(g),
            "tstats": torch.stack([tm + torch.log(ts), bv, tw / ts, xt], 1), "targmax": am}


def restate_f32(case, fp32_values=True):
    """wft_ce_fwd_f32 + wft_ce_bwd_f32 in CPU float32: the max first, then per-thread sums of exp(x - max) and of x over columns
    t, t + 256, ..., butterfly sums per wave, (w0 + w1) + (w2 + w3)."""
    x, V, ld = (case.x32 if fp32_values else case.x), case.V, case.ld
    rows = x.shape[0]
    m = x[:, :V].max(1).values
    P = (V + 255) // 256
    xp = torch.zeros(rows, P * 256, dtype=_F)
    xp[:, :V] = x[:, :V]
    act = (torch.arange(P * 256) < V).view(P, 256)
    xp = xp.view(rows, P, 256)
    s, sx = torch.zeros(rows, 256, dtype=_F), torch.zeros(rows, 256, dtype=_F)
    for p in range(P):
        s = torch.where(act[p], s + torch.exp(xp[:, p] - m[:, None]), s)
        sx = torch.where(act[p], sx + xp[:, p], sx)
    s, sx = _butterfly((s, sx), lambda a, b: (a[0] + b[0], a[1] + b[1]))
    S = (s[:, 0] + s[:, 64]) + (s[:, 128] + s[:, 192])
    X = (sx[:, 0] + sx[:, 64]) + (sx[:, 128] + sx[:, 192])
    lse = m + torch.log(S)
    row_loss, stats, g = _loss_and_grad(x, lse, X, case.targets, V, ld, case.eps, case.gscale, None, V)
    return {"row_loss": row_loss, "row_lse": lse, "stats": stats, "dlogits": g}
