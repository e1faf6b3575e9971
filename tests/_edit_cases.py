"""Edit counts (include/wft.h "Edit counts"): two restatements of the rule, the case sets of tests/test_edit_host.py and
tests/test_edit_gpu.py, and the mutants the comparison has to reject.

A case set is a *batch*: one int32 symbol buffer `sym` and an int64 table `rows` [P, 4] of (ref_off, hyp_off, ref_len, hyp_len) — the
kernel's own input.  `expected(batch)` is int64 [P, 4] of (H, S, D, I), computed once per batch and shared (never modified).

References: `counts_table` fills the whole (n + 1) x (m + 1) table in plain Python, row by row; `counts_diagonals` sweeps anti-diagonals
with numpy (four separate integer planes, no packing), for the pairs too long for Python.  They share no code with each other, with
eval/metrics.py or with the kernel's 64-bit cells."""
import functools
import itertools

import numpy as np

POISON = 0x5A5A5A5A  # between the rows of a buffer; the same value on both sides of every gap, so an over-read MATCHES and shows
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


# --------------------------------------------------------------------------- references
def counts_table(r, h):
    """(H, S, D, I) by the rule, whole table, plain Python."""
    r, h = [int(x) for x in r], [int(x) for x in h]
    n, m = len(r), len(h)
    T = [[None] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0:
                T[i][j] = (0, 0, j)
            elif j == 0:
                T[i][j] = (0, i, 0)
            else:
                s, d, k = T[i - 1][j - 1]
                best = (s + (r[i - 1] != h[j - 1]), d, k)
                s, d, k = T[i - 1][j]
                if s + d + k + 1 < sum(best):
                    best = (s, d + 1, k)
                s, d, k = T[i][j - 1]
                if s + d + k + 1 < sum(best):
                    best = (s, d, k + 1)
                T[i][j] = best
    S, D, I = T[n][m]
    return n - S - D, S, D, I


def counts_diagonals(r, h):
    """(H, S, D, I) by the rule, anti-diagonal by anti-diagonal with numpy: planes [cost, S, D, I] indexed by i."""
    r, h = np.asarray(r, dtype=np.int64).reshape(-1), np.asarray(h, dtype=np.int64).reshape(-1)
    n, m = r.shape[0], h.shape[0]
    p1 = p2 = np.zeros((4, n + 1), dtype=np.int64)
    for d in range(n + m + 1):
        lo, hi = max(0, d - m), min(n, d)
        cur = np.zeros((4, n + 1), dtype=np.int64)
        a, b = max(lo, 1), min(hi, d - 1)  # the cells with i >= 1 and j >= 1
        if a <= b:
            ii = np.arange(a, b + 1)
            sub = (r[ii - 1] != h[d - ii - 1]).astype(np.int64)
            best = p2[:, a - 1:b].copy()
            best[0] += sub
            best[1] += sub
            dele = p1[:, a - 1:b].copy()
            dele[0] += 1
            dele[2] += 1
            best = np.where(dele[0] < best[0], dele, best)
            ins = p1[:, a:b + 1].copy()
            ins[0] += 1
            ins[3] += 1
            best = np.where(ins[0] < best[0], ins, best)
            cur[:, a:b + 1] = best
        if lo == 0:
            cur[:, 0] = (d, 0, 0, d)
        if d <= n:
            cur[:, d] = (d, 0, d, 0) if d else (0, 0, 0, 0)
        p2, p1 = p1, cur
    _, S, D, I = (int(v) for v in p1[:, n])
    return n - S - D, S, D, I


def reference(r, h):
    return counts_table(r, h) if len(r) * len(h) <= 1024 else counts_diagonals(r, h)


# --------------------------------------------------------------------------- batches
class Batch:
    def __init__(self, name, sym, rows):
        self.name = name
        self.sym = np.ascontiguousarray(np.asarray(sym, dtype=np.int64).astype(np.int32))
        self.rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)

    def pair(self, p):
        ro, ho, n, m = (int(v) for v in self.rows[p])
        return self.sym[ro:ro + n], self.sym[ho:ho + m]

    def __len__(self):
        return self.rows.shape[0]


_EXPECTED = {}


def expected(batch):
    """int64 [P, 4], computed once per batch name (read-only)."""
    if batch.name not in _EXPECTED:
        want = np.array([reference(*batch.pair(p)) for p in range(len(batch))], dtype=np.int64).reshape(-1, 4)
        want.setflags(write=False)
        _EXPECTED[batch.name] = want
    return _EXPECTED[batch.name]


def _pack(name, pairs, gap=1):
    """Pairs of sequences -> one buffer: every sequence on its own, `gap` poison symbols in front of each and behind the last."""
    sym, rows = [], []
    for r, h in pairs:
        offs = []
        for s in (r, h):
            sym += [POISON] * gap
            offs.append(len(sym))
            sym += [int(x) for x in s]
        rows.append((offs[0], offs[1], len(r), len(h)))
    sym += [POISON] * max(gap, 1)
    return Batch(name, sym, rows)


@functools.lru_cache(maxsize=None)
def exhaustive():
    """Every pair of strings over {0, 1, 2} of length 0 .. 4: 121 strings stored once, 14 641 pairs."""
    strings = [s for k in range(5) for s in itertools.product((0, 1, 2), repeat=k)]
    sym, off = [POISON], []
    for s in strings:
        off.append(len(sym))
        sym += list(s) + [POISON]
    rows = [(off[a], off[b], len(strings[a]), len(strings[b])) for a in range(len(strings)) for b in range(len(strings))]
    return Batch("exhaustive", sym, rows)


def seam_lengths(T):
    return sorted({63, 64, 65, T - 1, T, T + 1, 2 * T + 1})


def _structured(rng, L):
    """The structured pairs of one seam length L (>= 3)."""
    base = rng.integers(0, 3, size=L).tolist()
    mid = L // 2
    return [
        (base, list(base)),                                   # identical
        (base, [x + 3 for x in base]),                        # no symbol in common
        (base, base[1:]), (base, base[:mid] + base[mid + 1:]), (base, base[:-1]),   # one deletion: first, middle, last
        (base, [7] + base), (base, base + [7]),               # one insertion: first, last
        (base, base[1:] + [rng.integers(0, 3).item()]),       # the reference shifted by one
    ]


@functools.lru_cache(maxsize=None)
def seams(T, sample=False):
    """n and m each over the seam lengths (both n < m and n > m), random over an alphabet of 3, then the structured pairs of every
    seam length.  sample=True: the lengths <= 65 only (what the plain-Python reference can afford)."""
    rng = np.random.default_rng(20)
    lengths = [L for L in seam_lengths(T) if not sample or L <= 65]
    pairs = [(rng.integers(0, 3, size=n).tolist(), rng.integers(0, 3, size=m).tolist()) for n in lengths for m in lengths]
    for L in lengths:
        pairs += _structured(rng, L)
    return _pack(f"seams_{T}_{int(sample)}", pairs)


@functools.lru_cache(maxsize=None)
def extremes(L):
    rng = np.random.default_rng(21)
    s = lambda k: rng.integers(0, 3, size=k).tolist()
    return _pack(f"extremes_{L}", [([], s(L)), (s(L), []), (s(1), s(L)), (s(L), s(1)), (s(L), s(L)), ([], [])])


@functools.lru_cache(maxsize=None)
def ragged(P=300):
    """Mixed lengths 0 .. 150 (a few empty sides), alphabets of 2 .. 5; one poison symbol between neighbours."""
    rng = np.random.default_rng(22)
    pairs = []
    for p in range(P):
        n, m = (int(v) for v in rng.integers(0, 151, size=2))
        if p % 37 == 0:
            n = 0
        if p % 41 == 0:
            m = 0
        k = 2 + p % 4
        r = rng.integers(0, k, size=n).tolist()
        # half of the hypotheses are noisy copies of the reference, as a transcript is
        h = [x for x in r if rng.random() > 0.1][:m] + rng.integers(0, k, size=3).tolist() if p % 2 else rng.integers(0, k, size=m).tolist()
        pairs.append((r, h[:150]))
    return _pack("ragged", pairs)


@functools.lru_cache(maxsize=None)
def symbol_values():
    hi = 1 << 16
    pairs = [
        ([-1, -2, -3, -1], [-1, -3, -2, -1, -1]),
        ([INT32_MIN, INT32_MAX, 0, INT32_MIN], [INT32_MAX, INT32_MIN, 0]),
        ([INT32_MIN, INT32_MIN + 1, INT32_MAX - 1], [INT32_MIN + 1, INT32_MIN, INT32_MAX]),
        ([5, 5 + hi, 5 + 2 * hi, 5], [5 + hi, 5, 5, 5 + 3 * hi]),           # differ only above bit 15
        ([1, 2, 3, 4], [1 + hi, 2 + hi, 3 + hi, 4 + hi]),
        ([-1, 0x7FFF0000, 9], [0xFFFF, 0, 9]),                                # -1 and 0xFFFF agree in their low 16 bits
    ]
    return _pack("symbol_values", pairs)


def host_case_set(T=256):
    """What the mutants are run on (and the two references against each other): the exhaustive set, the symbol values, the seam sample."""
    return [exhaustive(), symbol_values(), seams(T, sample=True)]


def mismatches(got, want):
    """Rows where two [P, >= 4] integer arrays differ in any of the four counts -> indices."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.flatnonzero((got != want).any(axis=1))


# --------------------------------------------------------------------------- mutants
def _mutant_table(sym, row, order=("diag", "del", "ins"), column_as_insertions=False, read_at_i=False, diag_from_prev_diagonal=False,
                  drop_last=False, bits16=False):
    """The rule with one fault switched on, on the kernel's own input (buffer + table row) so that offset faults can be modelled."""
    ro, ho, n, m = (int(v) for v in row)
    sym = [int(x) & 0xFFFF for x in sym] if bits16 else [int(x) for x in sym]
    shift = 1 if read_at_i else 0
    rsym = lambda i: sym[min(ro + i - 1 + shift, len(sym) - 1)]
    hsym = lambda j: sym[min(ho + j - 1 + shift, len(sym) - 1)]
    T = [[(0, 0, 0)] * (m + 1) for _ in range(n + 1)]
    for d in range(n + m + 1):
        lo, hi = max(0, d - m), min(n, d)
        for i in range(lo, hi + 1):
            j = d - i
            if drop_last and i == hi and hi > lo:
                continue  # the cell keeps its initial zeros
            if i == 0:
                T[i][j] = (0, 0, j)
            elif j == 0:
                T[i][j] = (0, 0, i) if column_as_insertions else (0, i, 0)
            else:
                cand = {}
                s, dd, k = T[i - 1][j] if diag_from_prev_diagonal else T[i - 1][j - 1]
                cand["diag"] = (s + (rsym(i) != hsym(j)), dd, k)
                s, dd, k = T[i - 1][j]
                cand["del"] = (s, dd + 1, k)
                s, dd, k = T[i][j - 1]
                cand["ins"] = (s, dd, k + 1)
                best = cand[order[0]]
                for name in order[1:]:
                    if sum(cand[name]) < sum(best):
                        best = cand[name]
                T[i][j] = best
    S, D, I = T[n][m]
    return n - S - D, S, D, I


def _transposed_without_priority(sym, row):
    """Index by the shorter side: when n > m solve (h, r) and swap D and I back — but keep deletion-before-insertion in the transposed
    problem, where it means insertion-before-deletion."""
    ro, ho, n, m = (int(v) for v in row)
    if n <= m:
        return _mutant_table(sym, row)
    H, S, D, I = _mutant_table(sym, (ho, ro, m, n))
    return n - S - I, S, I, D


def _lengths_swapped(sym, row):
    ro, ho, n, m = (int(v) for v in row)
    r = [int(x) for x in sym[ro:ro + m]]
    h = [int(x) for x in sym[ho:ho + n]]
    return counts_table(r, h)


MUTANTS = {
    "deletion_insertion_priority_swapped": lambda sym, row: _mutant_table(sym, row, order=("diag", "ins", "del")),
    "deletion_before_diagonal": lambda sym, row: _mutant_table(sym, row, order=("del", "diag", "ins")),
    "insertion_before_diagonal": lambda sym, row: _mutant_table(sym, row, order=("ins", "diag", "del")),
    "transposed_without_priority_swap": _transposed_without_priority,
    "boundary_column_as_insertions": lambda sym, row: _mutant_table(sym, row, column_as_insertions=True),
    "symbol_read_at_i": lambda sym, row: _mutant_table(sym, row, read_at_i=True),
    "diagonal_from_previous_diagonal": lambda sym, row: _mutant_table(sym, row, diag_from_prev_diagonal=True),
    "last_cell_of_a_diagonal_dropped": lambda sym, row: _mutant_table(sym, row, drop_last=True),
    "hyp_off_ignored": lambda sym, row: _mutant_table(sym, (row[0], 0, row[2], row[3])),
    "symbols_truncated_to_16_bits": lambda sym, row: _mutant_table(sym, row, bits16=True),
    "lengths_swapped": _lengths_swapped,
}


def run_mutant(name, batch, limit=None):
    """A mutant's counts for (the first `limit` rows of) a batch -> int64 [P, 4]."""
    rows = batch.rows if limit is None else batch.rows[:limit]
    sym = batch.sym.tolist()
    return np.array([MUTANTS[name](sym, row) for row in rows], dtype=np.int64).reshape(-1, 4)
