"""Shared by test_mix_host.py (CPU) and test_mix_gpu.py: float64 references of wft_loudness_f32 and wft_bg_mix_f32 (scipy's lfilter,
numpy sums; optionally with one planted defect), the derived bounds, and the case tables.

BOUNDS (derived, not tuned).  u = 2^-53, the unit roundoff of fp64.

Loudness.  The device filters a row as filter.hip does, cut into chunks of 512 samples; its documented reordering bound is
|y_dev - y_seq| <= DELTA * Y with DELTA = 2^-30 and Y the row's largest |y| (include/wft.h "IIR filter"; lfilter IS the sequential
direct-form-II-transposed recurrence, and the rounding of its own fp64 steps is inside the same DELTA).  For block j with energy
z_j = sum y^2 / block over N_j samples:
    |sum y_dev^2 - sum y^2| <= 2 DELTA Y sum |y| + N_j DELTA^2 Y^2 <= (2 rho_j + rho_j^2) * sum y^2,  rho_j = DELTA * Y / sqrt(z_j)
(Cauchy-Schwarz: sum |y| <= sqrt(N_j sum y^2), and N_j <= block).  The sums of non-negative terms add a relative (number of additions
on the longest path) * u each: on the device 512 per chunk, hop / 512 + 2 chunk partials per slot, 4 slots, one square and one
division; for the reference any order of a block's terms, block - 1.  So
    eps_z(j) = 2 rho_j + rho_j^2 + (512 + hop / 512 + 8 + 4 hop) * u.
A gated mean of n_g blocks has the largest eps_z of its members plus 2 n_g u (both means); 10 log10 turns a relative eps into
(10 / ln 10) * eps / (1 - eps) dB; log10, the product, the sums and the division cost at most 8 ulps of max(|L|, 1) together
(2 ulps for each library's log10, one for each of the four other roundings):
    |dL| <= (10 / ln 10) * E / (1 - E) + 8 * 2^-52 * max(|L|, 1),   E = max eps_z over the gate + 2 n_g u.
The gate sets must be the same on both sides, so every case used on the GPU keeps every finite l_j at least 1e-3 dB (and at least
its own bound) away from -70 and from Gr (test_mix_host.py checks it).  The gain: 10^((target - L) / 20) moves by a relative
ln(10) / 20 * |dL| < 1e-8 — far inside half an f32 ulp (6e-8) — so gain_dev is the reference's f32 or its neighbour: one f32 ulp.
out must be x * gain_dev in f32, bit for bit.

Background.  A sum of squares of n non-negative terms: device 16 additions per thread, 8 halvings, ceil(n / 4096) chunks, one square
-> (25 + ceil(n / 4096)) u; reference, any order, n u.  eps_sum(n) = (n + 25 + ceil(n / 4096)) * u.  An RMS halves that and adds a
division and a square root: eps_rms(n) = eps_sum(n) / 2 + 2 u.  scale = desired / noise: eps_scale = eps_rms(n) + eps_rms(cnt) + 8 u
(exp10 at 2 ulps on each side, the two divisions).  An element: with t = scale * s in fp64,
    |out - (x + t)| <= ulp32(x + t) / 2  [the one rounding]  +  |t| * eps_scale + 2 u (|x| + |t|)  [the fp64 product and sum].
A copied row (kind none, a silent entry) is compared bit for bit, and so are the zeros behind n[b].
"""
import math

import numpy as np
from scipy.signal import lfilter

from whisper_finetune.data import mix_fx as MF

U = 2.0 ** -53
DELTA = 2.0 ** -30  # wft_sos_filter_f32's documented bound on the chunked recurrence, relative to the row's largest output
CHUNK = 512
SENTINEL = np.float32(-7.25)
PAD = 5             # columns behind n_max of a row's buffer (poisoned on input, sentinel on output)
GATE_MARGIN_DB = 1e-3
SINE_16K_LUFS = -3.083227497136298  # the restatement's reading of 5 s of a full-scale 997 Hz sine at 16 kHz (pinned to 1e-9)

LOUD_MUTANTS = ("hop_off_by_one", "block_of_three_hops", "offset_dropped", "first_gate_strict", "gamma_from_all_blocks",
                "minus_ten_dropped", "second_gate_without_absolute", "one_section_skipped", "state_reset_at_seam", "behind_n_counted",
                "last_block_dropped", "divisor_cut_length")
BG_MUTANTS = ("noise_rms_over_n", "mod_without_offset", "snr_sign_flipped", "db_over_10", "absolute_uses_clean_rms",
              "silent_rule_missing", "bank_offsets_off_by_one")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ loudness: reference
def k_filter(x64, sos, mutant=None):
    secs = sos[:1] if mutant == "one_section_skipped" else sos
    if mutant == "state_reset_at_seam":
        parts = []
        for c in range(0, len(x64), CHUNK):
            y = x64[c:c + CHUNK]
            for s in secs:
                y = lfilter(s[:3], s[3:], y)
            parts.append(y)
        return np.concatenate(parts) if parts else x64
    y = x64
    for s in secs:
        y = lfilter(s[:3], s[3:], y)
    return y


def block_energies(row, n, rate, mutant=None):
    """row: the f32 buffer (poison behind n) -> (z f64 [nb], the largest |y| of the row)."""
    hop = rate // 10
    block = 4 * hop
    m = len(row) if mutant == "behind_n_counted" else n
    y = k_filter(np.asarray(row[:m], dtype=np.float64), MF.k_weighting(rate), mutant)
    ymax = float(np.max(np.abs(y[:n]))) if n else 0.0
    nb = MF.block_count(n, hop)
    if mutant == "last_block_dropped" and n >= block:
        nb = (n - block) // hop + 1
    h = hop + 1 if mutant == "hop_off_by_one" else hop
    blk = 3 * hop if mutant == "block_of_three_hops" else block
    z = np.zeros(nb, dtype=np.float64)
    for j in range(nb):
        seg = y[j * h:j * h + blk]  # the slice cuts the rounded-up last block at the row's end, as upstream's does
        z[j] = np.sum(seg * seg) / (len(seg) if mutant == "divisor_cut_length" else blk)
    return z, ymax


def gates(z, mutant=None):
    """z -> dict(L, gamma, over, l, J1, J2): steps 4 to 7 of include/wft.h."""
    ninf = -math.inf
    off = 0.0 if mutant == "offset_dropped" else -0.691
    with np.errstate(divide="ignore", invalid="ignore"):
        l = off + 10.0 * np.log10(z)
        J1 = l > -70.0 if mutant == "first_gate_strict" else l >= -70.0
        none = np.zeros(len(z), dtype=bool)
        if not J1.any():
            return dict(L=ninf, gamma=ninf, over=0, l=l, J1=J1, J2=none)
        gamma = off + 10.0 * np.log10(np.mean(z if mutant == "gamma_from_all_blocks" else z[J1])) - (0.0 if mutant == "minus_ten_dropped" else 10.0)
        J2 = (l > gamma) if mutant == "second_gate_without_absolute" else (l > gamma) & (l > -70.0)
        if not J2.any():
            return dict(L=ninf, gamma=float(gamma), over=0, l=l, J1=J1, J2=J2)
        return dict(L=float(off + 10.0 * np.log10(np.mean(z[J2]))), gamma=float(gamma), over=int(J2.sum()), l=l, J1=J1, J2=J2)


def loud_ref(row, n, rate, target=None, mutant=None):
    """The float64 reference of one row: dict(L, gamma, over, gain f32, active, z, l, J1, J2, ymax, nb)."""
    z, ymax = block_energies(row, n, rate, mutant)
    g = gates(z, mutant)
    g.update(z=z, ymax=ymax, nb=len(z), gain=np.float32(1.0), active=False)
    if target is not None and g["over"] > 0 and math.isfinite(g["L"]):
        g["gain"], g["active"] = np.float32(10.0 ** ((target - g["L"]) / 20.0)), True
    return g


def eps_z(ref, hop):
    """The relative bound on every block energy of a reference row (module docstring); inf for an empty block."""
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = DELTA * ref["ymax"] * (1.0 + DELTA) / np.sqrt(ref["z"])
    rho = np.where(np.isfinite(rho), rho, np.inf)
    return 2.0 * rho + rho * rho + (CHUNK + hop // CHUNK + 8 + 4 * hop) * U


def _db(eps):
    return (10.0 / math.log(10.0)) * eps / (1.0 - eps) if eps < 1.0 else math.inf


def level_bound(ref, hop, which):
    """The bound on |dL| (which = "J2", level = L) or |dGr| (which = "J1", level = gamma) in dB."""
    sel = ref[which]
    if not sel.any():
        return 0.0
    level = ref["L"] if which == "J2" else ref["gamma"]
    E = float(np.max(eps_z(ref, hop)[sel])) + 2.0 * int(sel.sum()) * U
    return _db(E) + 8.0 * 2.0 ** -52 * max(abs(level), 1.0)


def gate_margin(ref, hop):
    """(The smallest distance in dB of a finite l_j from -70 or from Gr, the smallest distance that is left once every l_j and Gr have
    moved by their bounds).  The second one positive = no block can change sides legitimately.  A block's energy can move up by the
    relative eps_z and down by the same (all the way to zero when eps_z >= 1: such a block lies far below both gates)."""
    l = ref["l"]
    fin = np.isfinite(l)
    if not fin.any():
        return math.inf, math.inf
    eps = eps_z(ref, hop)[fin]
    with np.errstate(divide="ignore"):
        hi = l[fin] + 10.0 * np.log10(1.0 + eps)
        lo = l[fin] + 10.0 * np.log10(np.maximum(1.0 - eps, 0.0))
    gates_ = [(-70.0, -70.0)]
    if math.isfinite(ref["gamma"]):
        bg = level_bound(ref, hop, "J1")
        gates_.append((ref["gamma"] - bg, ref["gamma"] + bg))
    plain = min(float(np.min(np.abs(l[fin] - 0.5 * (a + b)))) for a, b in gates_)
    left = min(float(np.min(np.maximum(a - hi, lo - b))) for a, b in gates_)
    return plain, left


def loud_check(got, ref, hop):
    """got: dict(L, gamma, over, gain) of the code under test -> (ok, complaint)."""
    if int(got["over"]) != ref["over"]:
        return False, f"blocks over both gates {got['over']} != {ref['over']}"
    for key, which in (("L", "J2"), ("gamma", "J1")):
        a, b = float(got[key]), ref[key]
        if math.isinf(b):
            if a != b:
                return False, f"{key} {a} != {b}"
        elif not abs(a - b) <= level_bound(ref, hop, which):  # (NaN fails)
            return False, f"{key} {a!r} against {b!r}: off by {abs(a - b):.3e} dB, bound {level_bound(ref, hop, which):.3e}"
    ga, gb = np.float32(got["gain"]), ref["gain"]
    if not abs(float(ga) - float(gb)) <= float(np.spacing(gb)):
        return False, f"gain {ga!r} against {gb!r}: more than one f32 ulp"
    return True, ""


# ------------------------------------------------------------------------------------------------------------ loudness: cases
def _rng(seed):
    return np.random.default_rng(seed)


def three_level_row():
    """3 s at 16 kHz: 1 s of Gaussian noise at sigma = 0.3, 1 s 30 dB down, 0.5 s at 1e-5, 0.5 s of zeros."""
    g = _rng(31)
    return np.concatenate([0.3 * g.standard_normal(16000), 0.3 * 10.0 ** -1.5 * g.standard_normal(16000), 1e-5 * g.standard_normal(8000),
                           np.zeros(8000)]).astype(np.float32)


def quiet_two_level_row():
    """2 s at 16 kHz around the absolute gate: 1 s at sigma = 5e-4 (about -63 LUFS), 1 s at 2e-4 (about -71: under -70, over Gr)."""
    g = _rng(32)
    return np.concatenate([5e-4 * g.standard_normal(16000), 2e-4 * g.standard_normal(16000)]).astype(np.float32)


LOUD_N = (6399, 6400, 7199, 7200, 7201, 8800, 32767, 32768, 32769, 65537)


def _loud_rows():
    rows = [(f"noise_n{n}", (0.1 * _rng(100 + i).standard_normal(n)).astype(np.float32)) for i, n in enumerate(LOUD_N)]
    rows.append(("three_level", three_level_row()))
    rows.append(("quiet_two_level", quiet_two_level_row()))
    rows.append(("zeros", np.zeros(16000, dtype=np.float32)))
    rows.append(("amplitude_1e-5", (1e-5 * _rng(120).standard_normal(16000)).astype(np.float32)))
    return rows


def _loud_case(rate, rows):
    """rows [(name, samples)] -> one ragged batch: X f32 [B, n_max + PAD] with NaN behind n[b], ns, targets, the references."""
    n_max = max(len(s) for _, s in rows)
    X = np.full((len(rows), n_max + PAD), np.nan, dtype=np.float32)
    ns, names = [], []
    for b, (name, s) in enumerate(rows):
        X[b, :len(s)] = s
        ns.append(len(s))
        names.append(name)
    targets = [-31.0 + 18.0 * ((7 * b) % len(rows)) / len(rows) for b in range(len(rows))]  # spread over audiomentations' range
    refs = [loud_ref(X[b], ns[b], rate, targets[b]) for b in range(len(rows))]
    return dict(rate=rate, hop=rate // 10, X=X, ns=ns, n_max=n_max, names=names, targets=targets, refs=refs)


_CACHE = {}


def loud_case(rate=16000):
    """The reference is computed once and shared."""
    if rate not in _CACHE:
        if rate == 16000:
            _CACHE[rate] = _loud_case(rate, _loud_rows())
        else:
            _CACHE[rate] = _loud_case(rate, [(f"noise_2s_{rate}", (0.1 * _rng(rate).standard_normal(2 * rate)).astype(np.float32))])
    return _CACHE[rate]


def z_at_the_gate():
    """A block energy whose l_j is exactly -70.0 in float64 (for the `>` against `>=` defect; never used on the GPU)."""
    z = 10.0 ** ((-70.0 + 0.691) / 10.0)
    for _ in range(4096):
        with np.errstate(all="ignore"):
            l = -0.691 + 10.0 * np.log10(z)
        if l == -70.0:
            return z
        z = np.nextafter(z, math.inf if l < -70.0 else -math.inf)
    raise AssertionError("no float64 z with l == -70 found")


def loud_mutant_rejected(mutant):
    """Whether the comparisons reject the planted defect on at least one row (or on the gate-level case)."""
    hits = []
    for rate in (16000, 8000):
        case = loud_case(rate)
        for b, ref in enumerate(case["refs"]):
            got = loud_ref(case["X"][b], case["ns"][b], rate, case["targets"][b], mutant)
            if not loud_check(got, ref, case["hop"])[0]:
                hits.append(case["names"][b])
    z = np.array([z_at_the_gate(), 1e-3, 1e-3])
    a, b = gates(z), gates(z, mutant)
    if a["over"] != b["over"] or a["gamma"] != b["gamma"] or a["L"] != b["L"]:
        hits.append("z_at_the_gate")
    return hits


# ------------------------------------------------------------------------------------------------------------ background: reference
def eps_sum(n):
    return (n + 25 + -(-n // 4096)) * U


def eps_rms(n):
    return eps_sum(n) / 2.0 + 2.0 * U


def bg_ref(row, n, bank, off, rec, mutant=None):
    """The float64 reference of one row.  rec = (kind, entry, offset, db).  -> dict(out64 f64 [n] or None for a copy, clean, noise,
    scale, cnt, t = |scale * s|)."""
    kind, entry, offset, db = rec
    x = np.asarray(row[:n], dtype=np.float64)
    if kind == 0 or n == 0:
        return dict(out64=None, clean=0.0, noise=0.0, scale=0.0, cnt=0)
    a, b = int(off[entry]), int(off[entry + 1])
    if mutant == "bank_offsets_off_by_one":
        a, b = a + 1, b + 1
    e = np.asarray(bank[a:b], dtype=np.float64)
    m = len(e)
    o = min(int(offset), m - n) if m > n else 0
    cnt = min(m, n)
    idx = (np.arange(n) if mutant == "mod_without_offset" else o + np.arange(n)) % m
    s = e[idx]
    noise = float(np.sqrt(np.sum(s[:n if mutant == "noise_rms_over_n" else cnt] ** 2) / (n if mutant == "noise_rms_over_n" else cnt)))
    clean = float(np.sqrt(np.sum(x * x) / n))
    if noise < MF.SILENT_RMS and mutant != "silent_rule_missing":
        return dict(out64=None, clean=clean, noise=noise, scale=0.0, cnt=cnt)
    r = db / 10.0 if mutant == "db_over_10" else db / 20.0
    if kind == MF.KIND_ID["snr"]:
        desired = clean * 10.0 ** r if mutant == "snr_sign_flipped" else clean / 10.0 ** r
    else:
        desired = clean / 10.0 ** r if mutant == "absolute_uses_clean_rms" else 10.0 ** r
    scale = desired / noise
    return dict(out64=x + scale * s, clean=clean, noise=noise, scale=scale, cnt=cnt, t=np.abs(scale * s), x=np.abs(x))


def bg_check(got_out, got_stats, row, n, ref):
    """got_out f32 [n], got_stats (clean, noise, scale) of the code under test against the reference -> (ok, complaint)."""
    es = eps_rms(n) + eps_rms(max(ref["cnt"], 1)) + 8.0 * U
    for k, (name, eps) in enumerate((("clean", eps_rms(n) + U), ("noise", eps_rms(max(ref["cnt"], 1)) + U), ("scale", es))):
        a, b = float(got_stats[k]), ref[name]
        if not abs(a - b) <= eps * abs(b):  # (NaN fails; a zero must be a zero)
            return False, f"{name} {a!r} against {b!r}"
    if ref["out64"] is None:
        same = np.array_equal(bits(got_out), bits(row[:n]))
        return same, "" if same else "a copied row must keep its bits"
    want = ref["out64"]
    got = np.asarray(got_out, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mag = np.maximum(np.abs(got), np.abs(want)).astype(np.float32)
        lim = 0.5 * np.spacing(mag).astype(np.float64) + ref["t"] * es + 2.0 * U * (ref["x"] + ref["t"])
        bad = ~(np.abs(got - want) <= lim)
    if bad.any():
        i = int(np.argmax(bad))
        return False, f"element {i}: {got[i]!r} against {want[i]!r}, bound {lim[i]:.3e}"
    return True, ""


# ------------------------------------------------------------------------------------------------------------ background: cases
BG_N = (1, 4095, 4096, 4097, 12289)
GUARD_VALUE = 1e6


def bg_lengths(n):
    return (1, 7, 1023, 1025, 4096, 4097, n, n + 1, 3 * n)


def bg_case():
    """One ragged batch over every n of BG_N, every entry length of bg_lengths(n), the offsets 0 and m - n, both kinds; a silent entry,
    a "none" row; around every entry in use the bank holds entries of +-1e6, so a read one sample outside is an O(1) error."""
    if "bg" in _CACHE:
        return _CACHE["bg"]
    g = _rng(2024)
    entries, rows = [], []  # rows: (n, entry index, offset, kind, db)
    silent = None
    for n in BG_N:
        for m in bg_lengths(n):
            entries.append(np.full(3, GUARD_VALUE, dtype=np.float32))
            entries.append((0.05 * g.standard_normal(m)).astype(np.float32))
            e = len(entries) - 1
            entries.append(np.full(3, -GUARD_VALUE, dtype=np.float32))
            for o in sorted({0, max(m - n, 0)}):
                rows.append((n, e, o, MF.KIND_ID["snr"], float(g.uniform(2.0, 4.0))))
                rows.append((n, e, o, MF.KIND_ID["absolute"], float(g.uniform(-30.0, -10.0))))
    entries.append(np.full(2000, 1e-10, dtype=np.float32))  # RMS 1e-10 < 1e-9: the row is copied
    silent = len(entries) - 1
    entries.append(np.full(3, GUARD_VALUE, dtype=np.float32))
    rows.append((4097, silent, 0, MF.KIND_ID["absolute"], -20.0))
    rows.append((4096, silent, 17, MF.KIND_ID["snr"], 3.0))
    rows.append((4097, 1, 0, 0, 0.0))  # a "none" row
    bank, off = MF.pack_bank(entries)
    n_max = max(BG_N)
    X = np.full((len(rows), n_max + PAD), np.nan, dtype=np.float32)
    for b, r in enumerate(rows):
        X[b, :r[0]] = (0.1 * g.standard_normal(r[0])).astype(np.float32)
    ns = [r[0] for r in rows]
    recs = [(r[3], r[1], r[2], r[4]) for r in rows]
    refs = [bg_ref(X[b], ns[b], bank, off, recs[b]) for b in range(len(rows))]
    _CACHE["bg"] = dict(X=X, ns=ns, n_max=n_max, bank=bank, off=off, recs=recs, refs=refs, lengths=np.diff(off).tolist(), silent=silent)
    return _CACHE["bg"]


def bg_records(recs):
    rec = np.zeros(len(recs), dtype=MF.RECORD_DTYPE)
    for b, (kind, entry, offset, db) in enumerate(recs):
        rec[b] = (kind, entry, offset, db)
    return rec


def bg_mutant_rejected(mutant):
    case = bg_case()
    hits = []
    for b, ref in enumerate(case["refs"]):
        n = case["ns"][b]
        got = bg_ref(case["X"][b], n, case["bank"], case["off"], case["recs"][b], mutant)
        with np.errstate(over="ignore", invalid="ignore"):
            out = case["X"][b, :n] if got["out64"] is None else got["out64"].astype(np.float32)
        if not bg_check(out, (got["clean"], got["noise"], got["scale"]), case["X"][b], n, ref)[0]:
            hits.append(b)
    return hits
