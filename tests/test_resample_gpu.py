"""wft_resample_f32 on the GPU (csrc/audio.hip; K.resample): every output under the derived per-element bound of
tests/_resample_cases.py against the float64 sum over the same f32 table, the impulse response bit for bit, poison behind the rows'
ends, batch independence, the 64-bit phase and the argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _resample_cases as RC  # noqa: E402
from whisper_finetune.data import gpu_frontend as G  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = torch.device("cuda:0")


def _tile(orig, new):
    o, n, _, width = RC.geometry(orig, new)
    return L.load().wft_resample_tile(o, n, width)


def _lengths(orig, new):
    """The issue's lengths, and one output below, at and above the kernel's output tile (and two tiles plus a ragged third)."""
    tile = _tile(orig, new)
    return sorted(set(RC.lengths(orig, new)) | set(RC.lengths_around(orig, new, tile)) | {RC.lengths_around(orig, new, 2 * tile + 3)[1]})


def _check(got, x, orig, new, what, ms=None):
    taps = G.resample_taps(orig, new)[0].numpy()
    ref, bound = RC.ref_on_table(x, taps, orig, new, ms)
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == ref.shape and got.dtype == np.float32, (what, got.shape, ref.shape)
    bad = RC.violations(got, ref, bound)
    ratio = RC.worst_ratio(got, ref, bound)
    assert bad == 0, f"{what}: {bad} of {ref.shape[0]} outputs miss the bound (worst |got - ref| / bound = {ratio:.3f})"
    return ratio


# ----------------------------------------------------------------------------- 1. random input under the bound
@pytest.mark.parametrize("orig,new", RC.PAIRS)
def test_random_input_under_the_bound(orig, new):
    o, n = RC.reduced(orig, new)
    tile = _tile(orig, new)
    worst, outs = 0.0, []
    for n_in in _lengths(orig, new):
        x = RC.signal(n_in, seed=n_in)
        got = K.resample(torch.from_numpy(x).to(DEV)[None], orig, new)
        assert tuple(got.shape) == (1, RC.n_out_of(n_in, o, n))
        outs.append(got.shape[1])
        worst = max(worst, _check(got[0], x, orig, new, f"{orig} -> {new}, n_in = {n_in}"))
    assert any(v < tile for v in outs) and any(tile <= v <= tile + 3 for v in outs) and any(v > 2 * tile for v in outs), (tile, outs)
    x = RC.signal(257, 0, kind="constant")
    worst = max(worst, _check(K.resample(torch.from_numpy(x).to(DEV)[None], orig, new)[0], x, orig, new, "constant"))
    print(f"{orig} -> {new}: tile {tile}, n_out {outs}, worst |got - ref| / bound = {worst:.3f}")


def test_identity_and_the_public_wrapper():
    x = torch.from_numpy(RC.signal(1000, 1)).to(DEV)
    assert K.resample(x[None], 16000, 16000).data_ptr() == x.data_ptr()          # orig == new: the input, unchanged
    assert G.resample(x, 16000).data_ptr() == x.data_ptr()
    one = G.resample(x.cpu().numpy(), 48000)                                      # a host array goes to the device; 1-D in, 1-D out
    assert one.is_cuda and tuple(one.shape) == (334,)
    two = G.resample(torch.stack([x, x]), 48000)
    assert tuple(two.shape) == (2, 334) and torch.equal(two[0], one) and torch.equal(two[1], one)
    assert torch.equal(one, K.resample(x[None], 3, 1)[0])                          # the reduced pair is the same launch


# ----------------------------------------------------------------------------- 2. the impulse response
@pytest.mark.parametrize("orig,new", [(48000, 16000), (44100, 16000), (8000, 16000), (16000, 44100)])
def test_impulse_response_bit_for_bit(orig, new):
    o, n, _, width = RC.geometry(orig, new)
    taps = G.resample_taps(orig, new)[0].numpy()
    n_in = 3 * o + 2 * width + 5
    for j_imp in (0, n_in - 1, n_in // 2 + 1):
        x = np.zeros(n_in, dtype=np.float32)
        x[j_imp] = 1.0
        got = K.resample(torch.from_numpy(x).to(DEV)[None], orig, new)[0].cpu().numpy()
        want = RC.impulse_expected(taps, orig, new, n_in, j_imp)
        assert np.count_nonzero(want) > 0
        hit = want != 0
        assert np.array_equal(got[hit].view(np.uint32), want[hit].view(np.uint32)) and (got[~hit] == 0).all(), (orig, new, j_imp)


# ----------------------------------------------------------------------------- 3. poison behind the rows' ends
@pytest.mark.parametrize("pad_in,pad_out", [(5, 3), (8, 8), (1, 0)])
def test_poison_behind_the_row_ends(pad_in, pad_out):
    orig, new, B = 44100, 16000, 2
    o, n = RC.reduced(orig, new)
    n_in = RC.lengths_around(orig, new, _tile(orig, new) + 7)[1]
    n_out = RC.n_out_of(n_in, o, n)
    ld_out = n_out + pad_out + (-(n_out + pad_out) % 4 if pad_out == 8 else 0)   # (8, 8): every row on the 16-byte grid
    xs = [RC.signal(n_in, seed=70 + b) for b in range(B)]
    buf = torch.full((B, n_in + pad_in), float("nan"), device=DEV)
    buf[:, :n_in] = torch.from_numpy(np.stack(xs)).to(DEV)
    canary = 12345.678
    out = torch.full((B, ld_out), canary, device=DEV)
    res = K.resample(buf[:, :n_in], orig, new, out=out[:, :n_out])
    assert res.data_ptr() == out.data_ptr()
    host = out.cpu()
    assert torch.isfinite(host).all()
    for b in range(B):
        _check(host[b, :n_out], xs[b], orig, new, f"row {b} with NaN behind n_in")
    assert (host[:, n_out:] == torch.tensor(canary)).all(), "the kernel wrote behind n_out"


# ----------------------------------------------------------------------------- 4. batch independence
@pytest.mark.parametrize("orig,new", [(48000, 16000), (44100, 16000)])
def test_rows_of_a_batch_equal_the_single_calls(orig, new):
    n_in = RC.lengths_around(orig, new, 2 * _tile(orig, new) + 3)[1] | 1     # odd: the rows sit differently on the 16-byte grid
    x = torch.from_numpy(np.stack([RC.signal(n_in, seed=90 + b) for b in range(3)])).to(DEV)
    both = K.resample(x, orig, new)
    for b in range(3):
        assert torch.equal(both[b], K.resample(x[b:b + 1].clone(), orig, new)[0]), b


# ----------------------------------------------------------------------------- 5. the 64-bit phase
def test_the_phase_is_formed_in_64_bits():
    orig, new, n_in = 44100, 16000, 14_000_000
    x = RC.signal(n_in, seed=5)
    n_out = RC.n_out_of(n_in, 441, 160)
    m_c = 2 ** 31 // 441
    ms = np.concatenate([np.arange(m_c - 750, m_c + 750), np.arange(n_out - 500, n_out)])
    assert ms.shape[0] == 2000 and (ms[:1500] * 441 < 2 ** 31).any() and (ms[:1500] * 441 >= 2 ** 31).any()
    got = K.resample(torch.from_numpy(x).to(DEV)[None], orig, new)
    assert tuple(got.shape) == (1, n_out)
    ratio = _check(got[0, torch.from_numpy(ms).to(DEV)], x, orig, new, "around m * 441 = 2^31 and at the end", ms)
    print(f"64-bit phase: worst |got - ref| / bound = {ratio:.3f} over {ms.shape[0]} sampled outputs")


# ----------------------------------------------------------------------------- 6. argument errors, before any launch
def test_argument_errors():
    lib = L.load()
    taps, o, n, width = G.resample_taps(48000, 16000)
    taps = taps.to(DEV)
    x = torch.zeros((2, 300), device=DEV)
    out = torch.full((2, 100), 7.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(ld_in=300, n_in=300, o_=3, n_=1, ld_out=100, n_out=100, B=2):
        return lib.wft_resample_f32(p(x), ld_in, n_in, p(taps), o_, n_, width, p(out), ld_out, n_out, B, L.stream_ptr())

    assert call() == 0
    torch.cuda.synchronize()
    assert (out == 0).all()
    out.fill_(7.0)
    for what, kw in (("not coprime", dict(o_=6, n_=2)), ("wrong n_out", dict(n_out=99)), ("wrong n_out", dict(n_out=101, ld_out=101)),
                     ("short ld_in", dict(ld_in=299)), ("short ld_out", dict(ld_out=99)), ("no rows", dict(B=0)), ("empty", dict(n_in=0, n_out=0))):
        assert call(**kw) != 0, what
        assert "wft_resample_f32" in L.last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all(), "a refused call must not launch"
    # the Python wrapper checks before it calls
    for bad in (dict(orig=0, new=1), dict(orig=3.0, new=1), dict(orig=True, new=1), dict(orig=3, new=-1)):
        with pytest.raises(ValueError):
            K.resample(x, **bad)
    with pytest.raises(ValueError):
        K.resample(x[0], 3, 1)                                     # 2-D only
    with pytest.raises(ValueError):
        K.resample(x, 3, 1, out=torch.empty((2, 99), device=DEV))  # wrong n_out
    with pytest.raises(TypeError):
        K.resample(x.double(), 3, 1)
    with pytest.raises(L.WftError):
        K.resample(x.cpu(), 3, 1)                                  # no CPU path
    with pytest.raises(ValueError):
        K.resample(x, 5000 * 7, 1)                                 # 2 * width taps do not fit the staging buffer
