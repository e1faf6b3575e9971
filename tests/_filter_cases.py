"""Reference, emulation, per-element bound, cases and mutants for the IIR cascade (csrc/filter.hip, include/wft.h "IIR filter").
numpy float64 throughout.  Only the filter TABLE comes from the product (data/filters.py designs the extremes of its own ranges); the
reference, the emulation and the bound import nothing from it.  The chunk length L and the group size G are arguments: the tests read
them from the library (wft_sos_filter_chunk / wft_sos_filter_group, pure host functions).

THE REFERENCE (`reference`) is the sequential recurrence of the header, one sample after the other, every product and every sum its
own numpy operation (no FMA), vectorised over rows:
    y = b0 x + z0;   z0 = b1 x - a1 y + z1;   z1 = b2 x - a2 y        per section, sections in index order, zero initial state
Row r filters its first n[r] samples and is zero behind them.  It returns float64: the ONE rounding to float32 is the bound's first term.

THE EMULATION (`emulate`) restates the kernel's parallel form in float64: chunks of L samples from zero state -> z_c; the L-step
zero-input transition matrix M, column j = the state after L zero-input steps of the same step function from e_j; the scan
s_0 = 0, s_(c+1) = M s_c + z_c (products summed in ascending column order, then z_c); the chunks again from s_c.  `mutant=` breaks
one thing at a time (MUTANTS below); tests/test_filter_host.py asserts that the bound rejects them.

THE BOUND, per element, no element excluded:
    |y - ref| <= 2^-24 |ref| + DELTA max_row|ref| + 2^-149
  2^-24 |ref|        the one float32 rounding (half an ulp, relative)
  DELTA max_row|ref| the fp64 reordering of the chunked scheme and the FMA contraction of the device code
  2^-149             the smallest float32 subnormal: a reference value below it may round either way
DELTA was chosen on the CPU (`calibrate` below, run as `python -m tests._filter_cases 512`): the largest error of `emulate` against
the sequential recurrence over the whole table x the five probes at 480 000 samples, relative to the row's largest output, is
    1.03e-10 at L = 512 (the band-stop at 4000 Hz, fraction 1.99, order 4, on the DC step; 9.8e-11 on the noise probe; every other
    filter of the table stays under 5e-13)
The smallest power of two that is at least 8 times that (8.2e-10) is 2^-30 = 9.3e-10.  DELTA = 2^-30 meets the condition
DELTA <= 2^-30: it is 64 times under half a float32 ulp at full scale, so the bound still sees a one-ulp error of any element within
a factor of 64 of the row's maximum.  It is derived from the emulation alone, never from what the kernel gives.  (The band-stop is
the worst because its sections cannot all be well scaled: its zeros lie in the stopped band and its poles at the two edges, so the
signal between two sections carries a factor of about (4000 / 20)^2 at the lowest frequencies; data/filters.py alternates the sections
of the two edges to keep it at one such factor.  Outside the table, a band-stop at 200 Hz with fraction 1.99, whose lower edge is
1 Hz, reaches 2e-9 on the DC step.)
"""
import numpy as np

DELTA = 2.0 ** -30
U32 = 2.0 ** -24
TINY = 2.0 ** -149
IDENTITY = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])
N_FULL = 480000


# ------------------------------------------------------------------------------------------------------------ reference
def _step(c, z, x):
    """One sample through the cascade.  c [R, S, 6], z [R, S, 2] (updated in place), x [R] -> y [R]."""
    for s in range(c.shape[1]):
        y = c[:, s, 0] * x + z[:, s, 0]
        z[:, s, 0] = c[:, s, 1] * x - c[:, s, 4] * y + z[:, s, 1]
        z[:, s, 1] = c[:, s, 2] * x - c[:, s, 5] * y
        x = y
    return x


def reference(x, sos, n=None):
    """x [R, N] (float32 values in any float dtype), sos f64 [R, S, 6], n int [R] or None -> float64 [R, N]."""
    x = np.asarray(x, dtype=np.float64)
    sos = np.asarray(sos, dtype=np.float64)
    R, N = x.shape
    n = np.full(R, N) if n is None else np.clip(np.asarray(n), 0, N)
    xt = np.ascontiguousarray(np.where(np.arange(N)[None, :] < n[:, None], x, 0.0).T)  # what lies behind n[r] is never read
    z = np.zeros((R, sos.shape[1], 2))
    y = np.empty((N, R))
    for i in range(N):
        y[i] = _step(sos, z, xt[i])
    y = y.T
    return np.where(np.arange(N)[None, :] < n[:, None], y, 0.0)


# ------------------------------------------------------------------------------------------------------------ emulation
MUTANTS = ("zero_state",        # every chunk starts from zero state
           "scan_drops_z",      # s_(c+1) = M s_c
           "scan_drops_Ms",     # s_(c+1) = z_c
           "z1_not_carried",    # the second state of every section is not carried across a seam
           "row0_coeffs",       # every row reads row 0's coefficients
           "n_max_for_n",       # a row uses n_max for n[b]
           "f32_between_sections",  # the output of every section is rounded through float32
           "M_one_step_short",  # M from L - 1 steps
           "M_transposed")      # the scan multiplies by M^T
EQUIVALENT_MUTANT = "partial_state_at_L"  # the last partial chunk's state is taken at L instead of at its true length: in this scheme
#                                           the state a row's LAST chunk ends in feeds nothing, so the mutant changes no bit


def _step_f32(c, z, x):
    for s in range(c.shape[1]):
        y = c[:, s, 0] * x + z[:, s, 0]
        z[:, s, 0] = c[:, s, 1] * x - c[:, s, 4] * y + z[:, s, 1]
        z[:, s, 1] = c[:, s, 2] * x - c[:, s, 5] * y
        x = y.astype(np.float32).astype(np.float64)
    return x


def emulate(x, sos, n, L, mutant=None, rounded=True):
    """The chunked scheme.  x [R, N], sos [R, S, 6], n [R] or None -> float32 [R, N] (rounded once), or float64 with rounded=False."""
    assert mutant is None or mutant in MUTANTS or mutant == EQUIVALENT_MUTANT, mutant
    x = np.asarray(x, dtype=np.float64)
    sos = np.asarray(sos, dtype=np.float64)
    R, N = x.shape
    S = sos.shape[1]
    n = np.full(R, N) if n is None else np.clip(np.asarray(n), 0, N)
    if mutant == "n_max_for_n":
        n = np.full(R, N)
    if mutant == "row0_coeffs":
        sos = np.broadcast_to(sos[:1], sos.shape).copy()
    step = _step_f32 if mutant == "f32_between_sections" else _step
    C = -(-N // L)
    xp = np.zeros((R, C * L))
    xp[:, :N] = np.where(np.arange(N)[None, :] < n[:, None], x, 0.0)
    xc = np.ascontiguousarray(xp.reshape(R * C, L).T)          # [L, R C]: sample i of every chunk
    cc = np.repeat(sos, C, axis=0)                             # the chunk's row's coefficients
    # 1. every chunk from zero state; the state is kept at the chunk's TRUE length (a partial last chunk stops at n[r])
    length = np.clip(n[:, None] - np.arange(C)[None, :] * L, 0, L).reshape(R * C)
    z = np.zeros((R * C, S, 2))
    zc = np.zeros_like(z)
    for i in range(L):
        step(cc, z, xc[i])
        live = length == i + 1
        zc[live] = z[live]
    if mutant == EQUIVALENT_MUTANT:
        zc = z.copy()
        zc[length == 0] = 0.0
    zc = zc.reshape(R, C, 2 * S)
    # 2. M by the same step function: column j = the state after L zero-input steps from e_j
    M = np.zeros((R, 2 * S, 2 * S))
    for j in range(2 * S):
        e = np.zeros((R, 2 * S))
        e[:, j] = 1.0
        e = e.reshape(R, S, 2)
        for _ in range(L - 1 if mutant == "M_one_step_short" else L):
            step(sos, e, np.zeros(R))
        M[:, :, j] = e.reshape(R, 2 * S)
    if mutant == "M_transposed":
        M = M.transpose(0, 2, 1).copy()
    # 3. the scan
    s0 = np.zeros((R, C, 2 * S))
    s = np.zeros((R, 2 * S))
    for c in range(C):
        s0[:, c] = s
        acc = M[:, :, 0] * s[:, 0:1]
        for k in range(1, 2 * S):
            acc = acc + M[:, :, k] * s[:, k:k + 1]
        if mutant == "scan_drops_Ms":
            acc = np.zeros_like(acc)
        s = acc if mutant == "scan_drops_z" else acc + zc[:, c]
    if mutant == "zero_state":
        s0[:] = 0.0
    if mutant == "z1_not_carried":
        s0[:, :, 1::2] = 0.0
    # 4. every chunk again from its true state
    z = s0.reshape(R * C, S, 2).copy()
    y = np.empty((L, R * C))
    for i in range(L):
        y[i] = step(cc, z, xc[i])
    y = y.T.reshape(R, C * L)[:, :N]
    y = np.where(np.arange(N)[None, :] < n[:, None], y, 0.0)
    return y.astype(np.float32) if rounded else y


# ------------------------------------------------------------------------------------------------------------ bound
def allowance(ref):
    """ref float64 [R, N] -> the per-element allowance [R, N]."""
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    return U32 * ref + DELTA * ref.max(axis=1, keepdims=True) + TINY


def worst_ratio(got, ref):
    """max over the elements of |got - ref| / allowance; NaN or inf in `got` counts as infinite."""
    got = np.asarray(got, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        return float("inf")
    return float((np.abs(got - ref) / allowance(ref)).max())


# ------------------------------------------------------------------------------------------------------------ cases
def _sections(*rows):
    return np.asarray(rows, dtype=np.float64)


def table():
    """name -> (sos f64 [S, 6], exact).  The exact filters' outputs are exact in float64 and float32 on small-integer input; the others
    are the extremes of the default ranges of data/filters.py."""
    from whisper_finetune.data.filters import design

    d1 = [0.0, 1.0, 0.0, 1.0, 0.0, 0.0]
    t = {
        "identity": (_sections(IDENTITY), True),
        "delay1": (_sections(d1), True),
        "delay2": (_sections([0.0, 0.0, 1.0, 1.0, 0.0, 0.0]), True),
        "delay1x4": (_sections(d1, d1, d1, d1), True),
        "accumulator": (_sections([1.0, 0.0, 0.0, 1.0, -1.0, 0.0]), True),
        "hp20_o4": (design("high_pass", cutoff_freq=20.0, order=4), False),
        "lp150_o4": (design("low_pass", cutoff_freq=150.0, order=4), False),
        "lp7500_o2": (design("low_pass", cutoff_freq=7500.0, order=2), False),
        "bp200_f0.5_o4": (design("band_pass", center_freq=200.0, bandwidth_fraction=0.5, order=4), False),
        "bs4000_f1.99_o4": (design("band_stop", center_freq=4000.0, bandwidth_fraction=1.99, order=4), False),
        "peak50_q5_p24": (design("peaking", center_freq=50.0, gain_db=24.0, q=5.0), False),
        "peak50_q5_m24": (design("peaking", center_freq=50.0, gain_db=-24.0, q=5.0), False),
        "ls50_q0.1_p18": (design("low_shelf", center_freq=50.0, gain_db=18.0, q=0.1), False),
        "ls50_q0.999_m18": (design("low_shelf", center_freq=50.0, gain_db=-18.0, q=0.999), False),
        "hs7500_q0.1_p18": (design("high_shelf", center_freq=7500.0, gain_db=18.0, q=0.1), False),
    }
    return t


def padded(sos, S=4):
    """sos [s, 6] -> [S, 6] with identity sections behind it."""
    out = np.tile(IDENTITY, (S, 1))
    out[: sos.shape[0]] = sos
    return out


PROBES = ("impulse0", "impulse_chunk_end", "impulse_group_end", "dc_step", "noise_silent_tail")


def probe(name, n, L, G, exact=False, seed=0):
    """One probe signal of n samples, float32.  The impulses sit at sample 0, at the last sample of a chunk (L - 1) and at the last
    sample of a workgroup's group of chunks (G L - 1), or at the row's last sample where the row is shorter.  exact: small integers."""
    x = np.zeros(n, dtype=np.float32)
    if name == "impulse0":
        x[0] = 1.0
    elif name == "impulse_chunk_end":
        x[min(L - 1, n - 1)] = 1.0
    elif name == "impulse_group_end":
        x[min(G * L - 1, n - 1)] = 1.0
    elif name == "dc_step":
        x[n // 3:] = 1.0
    elif name == "noise_silent_tail":
        rng = np.random.default_rng(1000 + seed)
        k = max(1, (2 * n) // 3)
        # (+ 0.0: rint gives -0.0 for a small negative number; the sign of zero has its own test, an identity row with -0.0 in it,
        # and the reference's 1 * -0.0 + 0.0 = +0.0 is not what a bit copy gives)
        x[:k] = (np.rint(rng.uniform(-4, 4, k)) + 0.0) if exact else (0.3 * rng.standard_normal(k))
    else:
        raise KeyError(name)
    return x


def lengths(L, G):
    """The smallest shapes at which a chunk seam, a group seam or the scan can go wrong."""
    return (1, L - 1, L, L + 1, 2 * L + 3, G * L - 1, G * L + 1, 2 * G * L + 5)


def cases(L, G):
    """Every (filter, probe, length) of the table -> a list of dicts {name, x f32 [n], sos f64 [S, 6], exact, n}, in a fixed shuffled
    order so that consecutive triples (the batches of 3) mix filters, section counts and lengths."""
    out = []
    for fi, (fname, (sos, exact)) in enumerate(table().items()):
        for pi, pname in enumerate(PROBES):
            for n in lengths(L, G):
                out.append({"name": f"{fname}/{pname}/{n}", "x": probe(pname, n, L, G, exact, seed=fi * 16 + pi), "sos": sos, "exact": exact,
                            "n": n})
    order = np.random.default_rng(20240).permutation(len(out))
    return [out[i] for i in order]


_REF = {}


def references(L, G):
    """name -> float64 reference of every case, computed ONCE per (L, G): rows of one length share a vectorised run."""
    if (L, G) not in _REF:
        cs, ref = cases(L, G), {}
        for n in lengths(L, G):
            grp = [c for c in cs if c["n"] == n]
            y = reference(np.stack([c["x"] for c in grp]), np.stack([padded(c["sos"]) for c in grp]))
            ref.update({c["name"]: y[i] for i, c in enumerate(grp)})
        _REF[(L, G)] = ref
    return _REF[(L, G)]


def batches(L, G, B=3):
    """The cases in batches of B rows -> a list of lists; every row has its own sos, n and section count."""
    cs = cases(L, G)
    assert len(cs) % B == 0
    return [cs[i:i + B] for i in range(0, len(cs), B)]


# ------------------------------------------------------------------------------------------------------------ choosing DELTA
def calibrate(L, n=N_FULL):
    """The largest error of the emulation against the sequential reference over the table x the probes at n samples, relative to
    the row's largest output.  scipy.signal.sosfilt stands in for `reference` where it is installed (tests/test_filter_host.py holds
    the two bit-equal), because the Python loop over 480 000 samples is slow."""
    try:
        from scipy.signal import sosfilt

        def seq(x, sos):
            return np.stack([sosfilt(s, r) for s, r in zip(sos, x)])
    except ImportError:
        seq = reference
    worst = (0.0, None)
    for fi, (fname, (sos, exact)) in enumerate(table().items()):
        x = np.stack([probe(p, n, L, 64, exact, seed=fi * 16 + pi) for pi, p in enumerate(PROBES)]).astype(np.float64)
        c = np.stack([padded(sos)] * len(PROBES))
        want, got = seq(x, c), emulate(x, c, None, L, rounded=False)
        rel = np.abs(got - want).max(axis=1) / np.maximum(np.abs(want).max(axis=1), 1e-300)
        for p, r in zip(PROBES, rel):
            print(f"{fname:18s} {p:18s} {r:.3e}")
            if r > worst[0]:
                worst = (float(r), f"{fname}/{p}")
    return worst


if __name__ == "__main__":
    import sys

    w = calibrate(int(sys.argv[1]) if len(sys.argv) > 1 else 512)
    print("worst", w, "-> 8x =", 8 * w[0], "DELTA = 2^", int(np.ceil(np.log2(8 * w[0]))))
