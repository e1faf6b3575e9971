"""The word-level alignment kernels (csrc/align.hip) through the C ABI against tests/_align_oracle.py: the alignment-head
probabilities and the standardise / median / head-mean stage inside the per-element bounds derived there (proved on the CPU by
tests/test_align_host.py: they pass a correct fp32 restatement and fail every mutant on these same inputs), dynamic time warping
path for path.  Shapes are the smallest that reach every edge: key counts at, one below and far below the 32-key tile edges and a
single key; one, a few and more than one tile of query rows, ragged; the filter skipped, the smallest reflecting width, one strip
and 47 strips of columns; DTW from one cell to the full 445 x 1500."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _align_oracle as AO  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = torch.device("cuda:0")
SENTINEL = -7.0


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _report(what, got, ref, bound):
    err = (got.cpu().to(AO.F64) - ref).abs()
    live = bound > 0
    worst = float((err[live] / bound[live]).max())
    print(f"{what}: worst |err| / bound {worst:.3f}, max |err| {float(err[live].max()):.3e}, largest bound {float(bound.max()):.3e}")
    return worst


# ------------------------------------------------------------------------------------------------ probabilities
def _run_probs(c):
    q, k = c["qbuf"].to(DEV), c["kv"].to(DEV)[..., :384]
    B, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    out = torch.full((B, len(c["heads"]), Tq, Tk), SENTINEL, dtype=torch.float32, device=DEV)
    K.attn_probs(q, k, _i32(c["heads"]), _i32(c["n_tok"]), _i32(c["n_key"]), c["H"], c["scale"], out, host_lens=(c["n_tok"], c["n_key"]))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", range(len(AO.PROBS_CASES)))
def test_attn_probs_within_the_bound_and_nothing_else_written(case):
    Tq, n_tok, n_key = AO.PROBS_CASES[case]
    c = AO.probs_case(Tq, n_tok, n_key, seed=case)
    ref = AO.probs_ref(c["q"], c["k"], c["heads"], c["n_tok"], c["n_key"], c["scale"])
    bound = AO.probs_bound(c["q"], c["k"], c["heads"], c["n_tok"], c["n_key"], c["scale"], ref)
    out = _run_probs(c).cpu()
    for b in range(3):
        nt, nk = n_tok[b], n_key[b]
        assert (out[b, :, nt:, :] == SENTINEL).all() and (out[b, :, :, nk:] == SENTINEL).all(), f"audio {b}: written outside [:n_tok, :n_key]"
        row_sum = out[b, :, :nt, :nk].double().sum(-1)
        assert (row_sum - 1).abs().max() < 1e-5
    got = torch.where(bound > 0, out.double(), torch.zeros((), dtype=AO.F64))
    worst = _report(f"probs Tq {Tq} n_tok {n_tok} n_key {n_key}", got, ref, bound)
    assert worst <= 1.0


def test_attn_probs_reruns_bit_identical_and_checks_its_arguments():
    c = AO.probs_case(33, (33, 17, 32), (1500, 1499, 750), seed=2)
    a, b = _run_probs(c), _run_probs(c)
    assert torch.equal(a, b)
    q, k = c["qbuf"].to(DEV), c["kv"].to(DEV)[..., :384]
    out = torch.empty((3, 3, 33, 1500), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):  # a host length beyond the extent is refused before any launch
        K.attn_probs(q, k, _i32(c["heads"]), _i32((34, 1, 1)), _i32(c["n_key"]), 6, 0.125, out, host_lens=((34, 1, 1), c["n_key"]))
    with pytest.raises(ValueError):
        K.attn_probs(q, k, _i32(c["heads"]), _i32(c["n_tok"]), _i32((1501, 1, 1)), 6, 0.125, out, host_lens=(c["n_tok"], (1501, 1, 1)))
    # the device copy alone being wrong cannot take the kernel out of bounds: it clamps to Tq / Tk
    out.fill_(SENTINEL)
    K.attn_probs(q, k, _i32(c["heads"]), _i32((1 << 20, -5, 32)), _i32((1 << 20, 1499, -1)), 6, 0.125, out, host_lens=((33, 0, 32), (1500, 1499, 0)))
    torch.cuda.synchronize()
    ref = AO.probs_ref(c["q"], c["k"], c["heads"], (33, 0, 32), (1500, 1499, 0), 0.125)
    bound = AO.probs_bound(c["q"], c["k"], c["heads"], (33, 0, 32), (1500, 1499, 0), 0.125, ref)
    o = out.cpu()
    assert (o[1] == SENTINEL).all() and (o[2] == SENTINEL).all()
    assert _report("probs, clamped lengths", torch.where(bound > 0, o.double(), torch.zeros((), dtype=AO.F64)), ref, bound) <= 1.0


# ------------------------------------------------------------------------------------------------ matrix
def _run_matrix(probs, n_tok, n_key, width=7):
    B, S, Tq, Tk = probs.shape
    out = torch.full((B, Tq, Tk), SENTINEL, dtype=torch.float32, device=DEV)
    K.align_matrix(probs, _i32(n_tok), _i32(n_key), width, out=out, host_lens=(n_tok, n_key))
    torch.cuda.synchronize()
    return out.cpu()


def _check_matrix(what, out, probs_cpu, n_tok, n_key, width=7):
    ref, bound = AO.matrix_ref(probs_cpu, n_tok, n_key, width)
    for b in range(out.shape[0]):
        assert (out[b, n_tok[b]:, :] == SENTINEL).all() and (out[b, :, n_key[b]:] == SENTINEL).all(), f"audio {b}: written outside [:n_tok, :n_key]"
    assert torch.isfinite(ref).all()
    got = torch.where(bound > 0, out.double(), torch.zeros((), dtype=AO.F64))
    assert _report(what, got, ref, bound) <= 1.0


@pytest.mark.parametrize("S", AO.MATRIX_SEL)
@pytest.mark.parametrize("keys", range(len(AO.MATRIX_KEYS)))
def test_align_matrix_on_crafted_probabilities(keys, S):
    n_key = AO.MATRIX_KEYS[keys]
    probs = AO.crafted_probs(3, S, 448, 1500, n_key, seed=keys)
    out = _run_matrix(probs.to(DEV), AO.MATRIX_TOK, n_key)
    _check_matrix(f"matrix n_sel {S} n_tok {AO.MATRIX_TOK} n_key {n_key}", out, probs, AO.MATRIX_TOK, n_key)


def test_align_matrix_on_the_kernels_own_probabilities_and_other_widths():
    c = AO.probs_case(33, (33, 17, 32), (1500, 1499, 750), seed=2)
    probs = _run_probs(c)
    out = _run_matrix(probs, c["n_tok"], c["n_key"])
    _check_matrix("matrix on device probabilities", out, probs.cpu(), c["n_tok"], c["n_key"])
    for width in (1, 3, 31):
        out = _run_matrix(probs, c["n_tok"], c["n_key"], width)
        _check_matrix(f"matrix, width {width}", out, probs.cpu(), c["n_tok"], c["n_key"], width)
    with pytest.raises(ValueError):
        K.align_matrix(probs, _i32(c["n_tok"]), _i32(c["n_key"]), 6, host_lens=(c["n_tok"], c["n_key"]))
    assert torch.equal(_run_matrix(probs, c["n_tok"], c["n_key"]), _run_matrix(probs, c["n_tok"], c["n_key"]))


# ------------------------------------------------------------------------------------------------ dynamic time warping
def _run_dtw(mats, row0=0, negate=True):
    """mats: list of float32 [N_b, M_b] costs x_b; the device matrix holds -x_b (negate) at rows row0.., junk elsewhere."""
    B = len(mats)
    R = row0 + max(m.shape[0] for m in mats)
    Cn = max(m.shape[1] for m in mats)
    g = torch.Generator().manual_seed(77)
    M = torch.randn(B, R, Cn, generator=g)
    for b, m in enumerate(mats):
        M[b, row0:row0 + m.shape[0], :m.shape[1]] = torch.from_numpy(-m if negate else m)
    n_rows, n_cols = [m.shape[0] for m in mats], [m.shape[1] for m in mats]
    ld = max(n_rows) + max(n_cols) - 1 + 3
    paths = (torch.full((B, ld), -9, dtype=torch.int32, device=DEV), torch.full((B, ld), -9, dtype=torch.int32, device=DEV),
             torch.full((B,), -9, dtype=torch.int32, device=DEV))
    K.dtw(M.to(DEV), row0, _i32(n_rows), _i32(n_cols), host_lens=(n_rows, n_cols), negate=negate, paths=paths)
    torch.cuda.synchronize()
    return [p.cpu() for p in paths]


def _check_paths(mats, paths):
    pt, pj, pl = paths
    for b, m in enumerate(mats):
        t, f = AO.dtw_ref(m)
        n = int(pl[b])
        assert n == len(t), (b, m.shape, n, len(t))
        assert np.array_equal(pt[b, :n].numpy(), t) and np.array_equal(pj[b, :n].numpy(), f), (b, m.shape)
        assert (pt[b, n:] == -9).all() and (pj[b, n:] == -9).all(), "the path buffer is written beyond path_len"


@pytest.mark.parametrize("shape", AO.DTW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("row0", [0, 4])
def test_dtw_path_equals_the_serial_loop(shape, row0):
    m = AO.dtw_matrix(*shape, "randn", seed=shape[0] + shape[1])
    _check_paths([m], _run_dtw([m], row0=row0))


def test_dtw_tie_laden_matrices():
    mats = [AO.dtw_matrix(N, M, kind, seed=i) for i, (N, M, kind) in enumerate(AO.DTW_TIE_CASES)]
    _check_paths(mats, _run_dtw(mats, row0=4))
    _check_paths(mats, _run_dtw(mats, row0=0, negate=False))
    big = [AO.dtw_matrix(130, 700, "ints", seed=50), AO.dtw_matrix(445, 1500, "equal")]
    _check_paths(big, _run_dtw(big))


def test_dtw_ragged_batch_equals_each_audio_alone():
    mats = [AO.dtw_matrix(65, 1500, "randn", seed=1), AO.dtw_matrix(1, 9, "randn", seed=2), AO.dtw_matrix(200, 130, "randn", seed=3)]
    batch = _run_dtw(mats, row0=4)
    _check_paths(mats, batch)
    for b, m in enumerate(mats):
        alone = _run_dtw([m], row0=4)
        n = int(alone[2][0])
        assert n == int(batch[2][b])
        assert torch.equal(alone[0][0, :n], batch[0][b, :n]) and torch.equal(alone[1][0, :n], batch[1][b, :n])


def test_dtw_checks_its_arguments_and_clamps_device_lengths():
    m = AO.dtw_matrix(9, 12, "randn", seed=9)
    M = torch.from_numpy(-m).to(DEV)[None]
    with pytest.raises(ValueError):  # more rows than the matrix holds behind row0
        K.dtw(M, 4, _i32([9]), _i32([12]), host_lens=([9], [12]))
    with pytest.raises(ValueError):
        K.dtw(M, 0, _i32([9]), _i32([13]), host_lens=([9], [13]))
    # device lengths beyond what the host declared are clamped to the launch's extents; a zero length gives an empty path
    pt, pj, pl = K.dtw(M, 0, _i32([1 << 20]), _i32([1 << 20]), host_lens=([9], [12]))
    torch.cuda.synchronize()
    t, f = AO.dtw_ref(m)
    n = int(pl[0])
    assert n == len(t) and np.array_equal(pt[0, :n].cpu().numpy(), t) and np.array_equal(pj[0, :n].cpu().numpy(), f)
    pt, pj, pl = K.dtw(M, 0, _i32([0]), _i32([-3]), host_lens=([9], [12]))
    torch.cuda.synchronize()
    assert int(pl[0]) == 0 and (pt == -1).all()
    assert L.load().wft_dtw_workspace_bytes(2, 448, 1500) >= 2 * 448 * 1947
