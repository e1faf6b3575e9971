"""Per-row rate conversion: float64 references, case tables, the per-element bound and planted defects (numpy only).

include/wft.h "Per-row rate conversion" is the contract; tests/test_rate_host.py proves the references here against numpy / scipy and
shows that the comparisons reject every mutant listed in SINC_MUTANTS and ALIAS_MUTANTS; tests/test_rate_gpu.py holds the kernels of
csrc/rate.hip against them.

SINC.  sinc_ref is the definition in float64, tap by tap in ascending j, t = j - t0 and a = c t formed exactly as the kernel forms
them (so WHICH taps count is decided by the same float64 comparison on both sides).  The kernel may differ from it by
    |got - ref| <= half an f32 ulp (of |ref| + E) + E,    E = EPS * sum_j |x_j| over the output's taps,
and EPS is derived by counting the fp64 operations of a tap's weight g = (c * (sinpi(a) / (pi * a))) * cospi(a / 12)^2, |g| <= 1:
  * a / 12, pi * a: one rounding each, 2^-53 relative; they move cospi by <= (pi / 2) 2^-53 and the quotient by <= 2^-52;
  * sinpi, cospi of the device's math library: taken as <= 4 ulp = 2^-51 absolute each (their values are <= 1); numpy's sin / cos of
    an argument pi * a that carries a rounding of up to 6 pi 2^-53 < 2^-48 absolute;
  * the division, c * snc, w * w, (c snc)(w w): four roundings, 2^-53 relative each;
  so |dg| <= 2^-48 + 2 * 2^-48 (the window enters squared) + 2^-51 < 2^-46 on either side, 2^-45 between kernel and reference;
  * the product x_j g: one rounding; the sum: at most 27 additions of partial sums bounded by sum |x_j| |g|, (27 + 1) 2^-53 < 2^-48
    relative on either side.
  EPS = 2^-44 covers the lot with a factor 2 to spare.  The issue's condition is EPS <= 2^-30: a t0 formed in f32 moves t by up to
  2^-24 * t0, i.e. the weight by ~1e-4 of |x| at t0 ~ 1000 — five orders above this bound.

ALIAS.  alias_numpy is audiomentations' Aliasing.apply in numpy, the reference; alias_emulation is the kernel's index rule written in
numpy (the direct index j = floor(t / step) corrected against the formed grid values, np.interp's value rule) and must be BIT-EQUAL to
it in float64 — that is the proof that the rule restates np.interp.  The kernel must give alias_numpy rounded once to f32, bit for bit.
"""
import numpy as np

EPS = 2.0 ** -44
SENTINEL = np.float32(-7.5e8)
RHOS = (0.5, 2.0 ** (-4.0 / 12.0), 1.0 - 2.0 ** -20, 1.0, 2.0 ** (4.0 / 12.0), 2.0)
SINC_MUTANTS = ("drop_first_tap", "drop_last_tap", "c_rho", "window_no_c", "t0_f32", "n_in_off", "fix_floor")
ALIAS_MUTANTS = ("d_trunc", "last_point", "no_eq_shortcut", "fma", "j_off_at_hit")
REACH = 14  # taps lie within floor(t0) - 13 .. floor(t0) + 13


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def signal(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ sinc resampler
def sinc_limit(N, rho, n_out, mutant=None):
    edge = np.floor(float(N) * rho) if mutant == "fix_floor" else np.ceil(float(N) * rho)
    return int(min(n_out, edge))


def sinc_ref(x, N, rho, n_out, mutant=None):
    """(out float64 [n_out], mag float64 [n_out]): the definition, and sum |x_j| over each output's taps (for the bound)."""
    x = np.asarray(x, dtype=np.float64)
    out, mag = np.zeros(n_out), np.zeros(n_out)
    if not (0.5 <= rho <= 2.0):  # (false for NaN)
        return out, mag
    N = int(min(max(N, 0), x.shape[0]))
    lim = sinc_limit(N, rho, n_out, mutant)
    if lim <= 0:
        return out, mag
    Nr = N - 1 if mutant == "n_in_off" else N
    c = 0.99 * rho if mutant == "c_rho" else 0.99 * min(1.0, rho)
    m = np.arange(lim, dtype=np.float64)
    t0 = (m.astype(np.float32) / np.float32(rho)).astype(np.float64) if mutant == "t0_f32" else m / rho
    i0 = np.floor(t0).astype(np.int64)
    acc, am = np.zeros(lim), np.zeros(lim)
    first = np.ones(lim, dtype=bool)
    last_j = np.full(lim, -(1 << 40), dtype=np.int64)
    for k in range(-REACH, REACH + 1):
        j = i0 + k
        t = j.astype(np.float64) - t0
        a = c * t
        on = np.abs(a) < 6.0
        if mutant == "drop_first_tap":
            on &= ~first
            first &= ~(np.abs(a) < 6.0)
        if mutant == "drop_last_tap":
            last_j = np.where(on, j, last_j)
        inside = (j >= 0) & (j < Nr)
        xs = np.where(inside, x[np.clip(j, 0, max(x.shape[0] - 1, 0))] if x.shape[0] else 0.0, 0.0)
        w = np.cos(np.pi * ((t if mutant == "window_no_c" else a) / 12.0))
        g = (c * np.sinc(a)) * (w * w)
        term = np.where(on, xs * g, 0.0)
        acc = acc + term
        am = am + np.where(on, np.abs(xs), 0.0)
    if mutant == "drop_last_tap":  # the same sum without each output's highest tap
        inside = (last_j >= 0) & (last_j < Nr)
        xs = np.where(inside, x[np.clip(last_j, 0, max(x.shape[0] - 1, 0))] if x.shape[0] else 0.0, 0.0)
        a = c * (last_j.astype(np.float64) - t0)
        w = np.cos(np.pi * (a / 12.0))
        acc = acc - xs * ((c * np.sinc(a)) * (w * w))
    out[:lim], mag[:lim] = acc, am
    return out, mag


def sinc_allow(ref, mag):
    e = EPS * mag
    return 0.5 * np.spacing((np.abs(ref) + e).astype(np.float32)).astype(np.float64) + e


def sinc_violations(got, ref, mag):
    """(number of elements outside the bound, largest |got - ref| / bound, share of elements that are not the rounded reference)."""
    got = np.asarray(got, dtype=np.float32)
    err = np.abs(got.astype(np.float64) - ref)
    allow = sinc_allow(ref, mag)
    finite = np.isfinite(got)
    bad = int(np.count_nonzero(~finite | (err > allow)))
    frac = float(np.max(np.where(allow > 0, err / np.where(allow > 0, allow, 1.0), 0.0))) if got.size else 0.0
    off = float(np.mean(bits(got) != bits(ref.astype(np.float32)))) if got.size else 0.0
    return bad, frac, off


def sinc_probe_rows(N, rho, tile, seed):
    """The probe inputs of one row of N samples: impulses at 0, N - 1 and around the staging seams (the first and last staged sample
    of the tiles), an all-ones row, a Gaussian row.  {name: f32 [N]}"""
    rows = {"ones": np.ones(N, dtype=np.float32), "gauss": signal(N, seed)}
    imp = np.zeros(N, dtype=np.float32)
    spots = [0, N - 1]
    for k in range(1, 10):  # every seam inside the row: the outputs k * tile start at the input floor(k * tile / rho)
        q = int(np.floor(k * tile / rho))
        if q - REACH >= N:
            break
        spots += [q - REACH, q - 1, q, q + REACH - 1]
    for i, s in enumerate(spots):
        if 0 <= s < N:
            imp[s] = 1.0 + 0.25 * (i % 3)
    rows["impulses"] = imp
    return rows


def sinc_batches(tile, rhos=RHOS):
    """Batches of three rows (N, rho).  Per ratio: every N of the issue's list with n_out between the rows' ceil(N rho), so that it
    lies below one and above another (mostly ONE workgroup per row); then a LONG batch, rows of 4 tile + 9, 2 tile + 5 and tile + 1
    samples with n_out = ceil((4 tile + 9) rho) + 7, above every row's own ceil(N rho): at least three workgroups per row at every
    ratio, full tiles (at rho = 0.5 and tile 784 the staged span of a full tile is 1597 of the 1600 floats), and every staging seam
    of the longest row inside the checked outputs.  Last, one batch of mixed ratios (sinc_mixed)."""
    ns = [0, 1, 2, 13, tile - 1, tile + 1, 2 * tile + 5]
    groups = [(0, 13, tile + 1), (1, 2, 2 * tile + 5), (tile - 1, 13, 2 * tile + 5)]
    assert sorted({n for g in groups for n in g}) == sorted(ns)
    out = []
    for rho in rhos:
        for g in groups:
            mid = sorted(int(np.ceil(n * rho)) for n in g)[1]
            out.append(([(n, rho) for n in g], max(mid + 3, 1)))
        long = (4 * tile + 9, 2 * tile + 5, tile + 1)
        out.append(([(n, rho) for n in long], int(np.ceil(long[0] * rho)) + 7))
    if len(rhos) >= 3:
        out.append(sinc_mixed(tile, rhos))
    return out


def sinc_mixed(tile, rhos=RHOS):
    """One batch of three ratios, rows of 4 tile + 9 samples and n_out = 3 * 1024 + 37: several workgroups per row, and workgroup
    boundaries at other outputs under a tile of 784 (a host bound of 0.5) than under one of 1024 (a host bound >= 0.66)."""
    n = 4 * tile + 9
    return [(n, rhos[0]), (n, rhos[-2]), (n - 2, rhos[1])], 3 * 1024 + 37


def peak_hz(y, sr=16000):
    """The frequency of the largest bin of the row's spectrum."""
    spec = np.abs(np.fft.rfft(np.asarray(y, dtype=np.float64)))
    return float(np.argmax(spec)) * sr / len(y)


# ------------------------------------------------------------------------------------------------------------ alias
def alias_numpy(samples, new_rate, sample_rate):
    """audiomentations' Aliasing.apply, float64 [n]."""
    n = len(samples)
    x = np.linspace(0, n, num=n)
    d = round(n * float(new_rate) / sample_rate)
    u = np.linspace(0, n, num=d)
    return np.interp(x, u, np.interp(u, x, samples))


def alias_d(n, new_rate, sample_rate, mutant=None):
    q = (float(n) * float(new_rate)) / float(sample_rate)
    return int(np.trunc(q)) if mutant == "d_trunc" else int(np.rint(q))


def _two_prod(a, b):
    p = a * b
    s = 134217729.0  # 2^27 + 1 (Veltkamp's split)
    ah = a * s - (a * s - a); al = a - ah
    bh = b * s - (b * s - b); bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _fma(a, b, c):
    """a * b + c with (nearly) one rounding: the exact product by Dekker, added with a compensated sum."""
    p, e = _two_prod(a, b)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    return s + (err + e)


def _grid(k, num, step, n_d, mutant):
    g = k.astype(np.float64) * step
    return g if mutant == "last_point" else np.where(k == num - 1, n_d, g)


def _locate(t, num, step, n_d, mutant):
    k = np.clip(np.floor(t / step).astype(np.int64), 0, num - 1)
    for _ in range(2):
        down = (k > 0) & (_grid(k, num, step, n_d, mutant) > t)
        up = ~down & (k < num - 1) & (_grid(np.minimum(k + 1, num - 1), num, step, n_d, mutant) <= t)
        k = k - down.astype(np.int64) + up.astype(np.int64)
    if mutant == "j_off_at_hit":
        k = np.where((k > 0) & (_grid(k, num, step, n_d, mutant) == t), k - 1, k)
    return k


def _interp(t, num, step, n_d, f, mutant):
    """np.interp(t, grid, f) by the direct index; f: callable index array -> float64 values."""
    j = _locate(t, num, step, n_d, mutant)
    f0, g0 = f(j), _grid(j, num, step, n_d, mutant)
    j1 = np.minimum(j + 1, num - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = (f(j1) - f0) / (_grid(j1, num, step, n_d, mutant) - g0)
        lin = _fma(slope, t - g0, f0) if mutant == "fma" else slope * (t - g0) + f0
    flat = (j == num - 1) if mutant == "no_eq_shortcut" else ((j == num - 1) | (g0 == t))
    return np.where(flat, f0, lin)


def alias_emulation(samples, new_rate, sample_rate, mutant=None):
    """The kernel's rule in numpy, float64 [n]; a "none" row (new_rate 0, n < 2, d < 2) is the samples themselves."""
    s = np.asarray(samples, dtype=np.float64)
    n = s.shape[0]
    d = alias_d(n, new_rate, sample_rate, mutant) if n >= 2 and new_rate != 0 else 0
    if d < 2:
        return s.copy()
    n_d = float(n)
    step_x, step_u = n_d / float(n - 1), n_d / float(d - 1)
    inner = lambda k: _interp(_grid(k, d, step_u, n_d, mutant), n, step_x, n_d, lambda j: s[j], mutant)  # noqa: E731
    t = _grid(np.arange(n, dtype=np.int64), n, step_x, n_d, mutant)
    return _interp(t, d, step_u, n_d, inner, mutant)


def alias_rates_for(n, sample_rate=16000.0):
    """New rates that give d in {2, n - 1, n, n + 1, ~n / 2, ~1.9 n} (where >= 2), two whose n * rate / sample_rate has a fraction
    above one half (truncation differs from rounding) and one exactly on a half (half to even)."""
    ds = sorted({d for d in (2, n - 1, n, n + 1, n // 2, int(1.9 * n)) if d >= 2})
    rates = [d * sample_rate / n for d in ds]
    rates += [(max(n // 2, 2) + 0.75) * sample_rate / n, (n + 0.625) * sample_rate / n, (2 * (n // 3) + 2.5) * sample_rate / n]
    return rates


def alias_inputs(n, tile, seed):
    """{name: f32 [n]}: impulses at 0, n - 1 and the tile seams; Gaussian rows; a row that starts with -0.0 in front of a positive sample
    (the one place where the `grid_j == t` shortcut shows: slope * 0 + (-0.0) is +0.0)."""
    imp = np.zeros(n, dtype=np.float32)
    for i, s in enumerate([0, n - 1] + [k * tile + o for k in (1, 2) for o in (-1, 0)]):
        if 0 <= s < n:
            imp[s] = 1.0 + 0.5 * (i % 2)
    g = signal(n, seed)
    z = np.abs(signal(n, seed + 1)) + np.float32(0.5)
    z[0] = np.float32(-0.0)
    return {"impulses": imp, "gauss": g, "negzero": z}


HOST_ALIAS_NS = (2, 3, 5, 7, 100, 1023, 1024, 1025, 2051, 4801)
LOADER_ALIAS_NS = (479999, 480000, 384000, 640000)  # the loader's rows: 30 s, and the ends of the default stretch range
