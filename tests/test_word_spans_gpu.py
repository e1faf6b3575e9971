"""wft_word_spans on the GPU (csrc/align.hip; K.word_spans): every case of tests/_word_cases.py against the float64 reference —
frames exactly, probabilities within n * 2^-23 * ref + 2^-149, the sentinels beyond n_words[b] and in the audio with the empty path
untouched — and a rerun is bit-identical.  tests/test_word_host.py shows on the CPU that this check rejects the listed mutants."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _word_cases as WC  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402

DEV = torch.device("cuda:0")
CASES = WC.cases()


def _launch(case):
    dev = lambda a: torch.from_numpy(a).to(DEV)
    out = tuple(dev(a) for a in WC.fresh_outputs(case))
    got = K.word_spans((dev(case["path_text"]), dev(case["path_time"]), dev(case["path_len"])), dev(case["bounds"]), dev(case["n_words"]),
                       dev(case["token_probs"]), dev(case["tok_off"]), case["n_rows_max"], host_lens=(case["n_words"].tolist(),), out=out)
    torch.cuda.synchronize()
    assert all(g is o for g, o in zip(got, out))
    return [g.cpu().numpy() for g in got]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_word_spans_against_the_reference(case):
    start, end, prob = _launch(case)
    worst = WC.check(case, start, end, prob)
    print(f"{case['name']}: worst |err| / bound {worst:.3f}")
    again = _launch(case)
    assert all((a == g).all() for a, g in zip(again, (start, end, prob))), "a rerun is not bit-identical"


def test_fresh_buffers_and_argument_errors():
    case = CASES[0]
    dev = lambda a: torch.from_numpy(a).to(DEV)
    paths = (dev(case["path_text"]), dev(case["path_time"]), dev(case["path_len"]))
    args = (dev(case["bounds"]), dev(case["n_words"]), dev(case["token_probs"]), dev(case["tok_off"]), case["n_rows_max"])
    start, end, prob = K.word_spans(paths, *args, host_lens=(case["n_words"].tolist(),))
    assert (start[2] == -1).all() and (end[2] == -1).all() and (prob[2] == 0).all()      # the empty path: what a fresh buffer holds
    assert tuple(start.shape) == (3, case["ld_words"]) and start.dtype == torch.int32 and prob.dtype == torch.float32
    with pytest.raises(ValueError):
        K.word_spans(paths, *args, host_lens=([1, 4, case["ld_words"] + 1],))            # more words than the bounds rows hold
    with pytest.raises(ValueError):
        K.word_spans(paths, *args[:4], 449, host_lens=(case["n_words"].tolist(),))       # one thread per path row: at most 448
    with pytest.raises(TypeError):
        K.word_spans(paths, args[0].float(), *args[1:], host_lens=(case["n_words"].tolist(),))
