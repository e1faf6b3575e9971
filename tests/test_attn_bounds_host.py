"""CPU proof that the per-(row, head) bound of the long-row attention tests bites (tests/test_decode_kernels_gpu.py close_per_head,
tol = 2^-7): the fp32 -> bf16 emulation of CORRECT single-token attention passes it, and the emulation of each way a kernel that
deals keys in blocks of 32 over 4 waves can go wrong fails it — on batches in which every row is long, where the batch-wide bound
(2e-2 of the largest value of the whole batch) has no short row to lean on.

Only arithmetic on the CPU: no kernel runs here, right or wrong.  The mutants restate csrc/decode_attn.hip's dealing (block j of 32 keys
belongs to wave j % 4; the key at p_new = n - 1 comes from the step's own k / v row, not from the cache)."""
import pytest
import torch

from tests.test_decode_kernels_gpu import ALL_LONG, PER_HEAD_TOL, _ref_decode, close, close_per_head

BF = torch.bfloat16
CAP = 449  # one row more than n_text_ctx, so that the "n + 1" mutant has a row to read behind a 448-key row


def _case(H, seed=0):
    lens = ALL_LONG
    B, D = len(lens), H * 64
    g = torch.Generator().manual_seed(seed * 7919 + H)
    cache = torch.randn(B, CAP, 2 * D, generator=g).to(BF)  # what the cache holds BEFORE the step: stale at p_new, garbage behind
    qkv = torch.randn(B, 3 * D, generator=g).to(BF)
    full = cache.clone()
    for b, n in enumerate(lens):
        full[b, n - 1] = qkv[b, D:]
    return lens, D, cache, qkv, full


def _attend(q, kv, keep, H, dtype):
    """Attention of row b over the keys keep[b] (a list of positions) of kv[b]; fp32 then rounded to bf16, or fp64 unrounded."""
    D = q.shape[1]
    out = []
    for b, idx in enumerate(keep):
        sub = kv[b, torch.tensor(idx)][None]
        out.append(_ref_decode(q[b:b + 1], sub[..., :D], sub[..., D:], [len(idx)], H, 0.125, dtype=dtype))
    o = torch.cat(out)
    return o.to(BF) if dtype == torch.float32 else o


def _mutants(lens, cache, full, D):
    """name -> (kv to read, the key positions each row attends over, the rows the mutation touches)."""
    every = [list(range(n)) for n in lens]
    rows = list(range(len(lens)))
    stale_v = full.clone()
    for b, n in enumerate(lens):
        stale_v[b, n - 1, D:] = cache[b, n - 1, D:]
    last_block = [list(range(32 * ((n - 1) // 32))) for n in lens]
    one_key = [[t for t in range(n) if t != 200] if n == 448 else list(range(n)) for n in lens]
    return {
        "wave 3's blocks dropped": (full, [[t for t in range(n) if (t // 32) % 4 != 3] for n in lens], rows),
        "stale cache row at p_new, k and v": (cache, every, rows),
        "stale cache row at p_new, v only": (stale_v, every, rows),
        "n - 1": (full, [list(range(n - 1)) for n in lens], rows),
        "n + 1": (full, [list(range(n + 1)) for n in lens], rows),
        "last block of 32 dropped": (full, last_block, rows),
        "one key of 448 dropped": (full, one_key, [b for b, n in enumerate(lens) if n == 448]),
    }


@pytest.mark.parametrize("H", [6, 20])
def test_the_per_head_bound_passes_correct_attention_and_fails_every_mutant(H):
    lens, D, cache, qkv, full = _case(H)
    q = qkv[:, :D]
    every = [list(range(n)) for n in lens]
    ref = _attend(q, full, every, H, torch.float64)
    good = _attend(q, full, every, H, torch.float32)
    ratio = close_per_head(good, ref, PER_HEAD_TOL, f"correct fp32 -> bf16, H={H}")
    assert ratio.max().item() <= 2.0 ** -8 * 1.01  # one rounding of the output: the bf16 half-ulp, which the bound doubles
    report = {}
    for name, (kv, keep, touched) in _mutants(lens, cache, full, D).items():
        bad = _attend(q, kv, keep, H, torch.float32)
        r = ((bad.double() - ref).abs().view(len(lens), H, 64).amax(-1) / ref.abs().view(len(lens), H, 64).amax(-1))[touched]
        report[name] = (r.min().item(), r.max().item(), (r > PER_HEAD_TOL).float().mean().item())
        print(f"H={H} {name}: per (row, head) error / own max|ref| min {r.min().item():.3e} max {r.max().item():.3e}, "
              f"{100 * report[name][2]:.0f} % of the touched (row, head) pairs above 2^-7")
        with pytest.raises(AssertionError):
            close_per_head(bad, ref, PER_HEAD_TOL, name)
        assert r.amax(-1).min().item() > PER_HEAD_TOL, f"{name}: a touched row passes in every head"
    # the batch-wide bound on the same all-long batch, for the record (it is kept as it is in the GPU tests)
    for name, (kv, keep, _) in _mutants(lens, cache, full, D).items():
        bad = _attend(q, kv, keep, H, torch.float32)
        try:
            close(bad, ref, 2e-2, f"batch-wide 2e-2, {name}")
            print(f"H={H} {name}: PASSES the batch-wide 2e-2 bound")
        except AssertionError:
            print(f"H={H} {name}: fails the batch-wide 2e-2 bound")


def test_one_dropped_key_of_448_is_reported():
    """A single key of a 448-key row carries about 1 / 448 of the softmax mass.  What the 2^-7 bound does with it is measured here
    and printed, not tuned for.  Found over 8 seeds x 20 heads (key 200 dropped): per head the error lies between 2.1e-3 and
    2.4e-1 of the head's own largest value, median 1.6e-2; 123 of 160 heads lie above 2^-7 and 37 below it.  So the bound does NOT
    separate a single lost key head by head, but a row of 20 heads (or 6) always has heads above it: the worst head of a row was
    never below 4.9e-2, six times the bound, and the row as a whole fails.  That, and that the mutant is never closer to the
    reference than correct attention, is what is asserted.
    Separating a single key head by head is not this file's job any more: on the probe operands of tests/_decode_probe.py one lost,
    leaked or double-counted key moves its (row, head) by at least 4 x 2^-7 (tests/test_decode_probe_host.py on the CPU,
    tests/test_decode_probe_gpu.py for every decode kernel and split regime)."""
    H = 20
    above = total = 0
    for seed in range(8):
        lens, D, cache, qkv, full = _case(H, seed)
        b = lens.index(448)
        q = qkv[b:b + 1, :D]
        ref = _attend(q, full[b:b + 1], [list(range(448))], H, torch.float64)
        good = _attend(q, full[b:b + 1], [list(range(448))], H, torch.float32)
        bad = _attend(q, full[b:b + 1], [[t for t in range(448) if t != 200]], H, torch.float32)
        scale = ref.abs().view(H, 64).amax(-1)
        rg = (good.double() - ref).abs().view(H, 64).amax(-1) / scale
        rb = (bad.double() - ref).abs().view(H, 64).amax(-1) / scale
        above += int((rb > PER_HEAD_TOL).sum()); total += H
        print(f"seed {seed}: one key of 448 dropped, per head error / own max|ref| min {rb.min().item():.3e} median {rb.median().item():.3e} "
              f"max {rb.max().item():.3e}; correct attention max {rg.max().item():.3e}")
        assert rb.max().item() > rg.max().item() and rb.max().item() > PER_HEAD_TOL
    print(f"one key of 448 dropped: {above} of {total} heads lie above 2^-7 = {PER_HEAD_TOL:.3e}")
    assert 0 < above <= total
