"""The two kernels of csrc/transcribe.hip on the GPU, against the references and bounds of tests/_transcribe_cases.py (which
tests/test_transcribe_host.py proves to bite).

wft_lang_probs: every (V, ld, ids) case x B in {1, 3, 5} x every kind of structured logits (one dominant language, all equal, a
planted tie between the first and the last id, values near +-80, probabilities spread over many orders of magnitude); every column
that is not a language column, and every column >= V, holds +inf or NaN.  probs within the derived per-element bound of float64,
best exact, the same launch twice gives the same bits.
wft_mel_windows: n_mels in {80, 128}, three recordings packed at odd offsets whose padding region is NaN, rows in non-index order
at every edge seek — bit for bit against slicing plus zero fill."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _transcribe_cases as TC  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402

DEV = torch.device("cuda:0")


def _bf16(x: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(TC.bf16_bits(x).view(np.int16)).view(torch.bfloat16).reshape(x.shape).to(DEV)


@pytest.mark.parametrize("case", TC.lang_cases(), ids=lambda c: c[0])
def test_lang_probs(case):
    name, V, ld, ids = case
    worst = 0.0
    for B in TC.LANG_ROWS:
        for kind in TC.LANG_KINDS:
            x = TC.lang_logits(B, V, ld, ids, kind)
            logits = _bf16(x)
            probs, best = K.lang_probs(logits, V, ids)
            again = K.lang_probs(logits, V, ids)
            assert probs.dtype == torch.float32 and tuple(probs.shape) == (B, len(ids)) and best.dtype == torch.int64
            assert torch.equal(probs, again[0]) and torch.equal(best, again[1])
            worst = max(worst, TC.lang_check(probs.cpu().numpy(), best.cpu().numpy(), x, V, ids, f"{name} B={B} {kind}"))
    print(f"{name}: worst |p - ref| / bound {worst:.3f}")


def test_lang_probs_argument_errors():
    logits = torch.zeros((2, 384), dtype=torch.bfloat16, device=DEV)
    for ids in ([], [5, 5], [7, 3], [-1, 3], [3, 300], list(range(1025))):
        with pytest.raises(ValueError):
            K.lang_probs(logits, 300, ids)
    with pytest.raises(ValueError):
        K.lang_probs(logits, 385, [1])
    with pytest.raises(TypeError):
        K.lang_probs(logits.float(), 300, [1])


@pytest.fixture(scope="module", params=[80, 128])
def mel_case(request):
    case = TC.mel_case(request.param)
    dev = dict(mel=torch.from_numpy(case["mel"]).to(DEV), off=torch.tensor(case["off"], dtype=torch.int64, device=DEV),
               ld=torch.tensor(case["ld"], dtype=torch.int32, device=DEV), cf=torch.tensor(case["cf"], dtype=torch.int32, device=DEV))
    return case, dev, TC.mel_expected(case)


def _windows(case, dev, rows, seeks, **kw):
    return K.mel_windows(dev["mel"], dev["off"], dev["ld"], dev["cf"], rows, seeks, case["n_mels"], TC.N_WIN,
                         host=(case["off"], case["ld"], case["cf"]), **kw)


def test_mel_windows_bit_for_bit(mel_case):
    case, dev, want = mel_case
    out = _windows(case, dev, case["rows"], case["seeks"])
    assert out.dtype == torch.float32 and tuple(out.shape) == want.shape
    got = out.cpu().numpy()
    assert np.isfinite(got).all(), "a NaN of the source's padding region reached the output"
    for r, (a, s) in enumerate(zip(case["rows"], case["seeks"])):
        assert TC.same_bits(got[r], want[r]), f"row {r}: recording {a} at seek {s}"
    # a single row, written into a buffer that held something else
    buf = torch.full((1, case["n_mels"], TC.N_WIN), float("nan"), device=DEV)
    one = _windows(case, dev, [1], [2], out=buf)
    assert one is buf and TC.same_bits(one.cpu().numpy()[0], want[case["rows"].index(1, 5)])


def test_mel_windows_argument_errors(mel_case):
    case, dev, _ = mel_case
    for rows, seeks in (([0], [4700]), ([0], [-1]), ([3], [0]), ([2], [7]), ([0, 1], [0]), ([], [])):
        with pytest.raises(ValueError):
            _windows(case, dev, rows, seeks)
    with pytest.raises(ValueError):
        K.mel_windows(dev["mel"], dev["off"], dev["ld"], dev["cf"], [0], [0], case["n_mels"], TC.N_WIN, host=(case["off"], case["ld"], [c + 1 for c in case["cf"]]))
    with pytest.raises(ValueError):
        K.mel_windows(dev["mel"], dev["off"], dev["ld"], dev["cf"], [0], [0], case["n_mels"], 2998, host=(case["off"], case["ld"], case["cf"]))
