"""The fp32 compute mode (training.mixed_precision_training: False; engine/ops32.py + csrc/f32.hip) against the fp32 CPU
oracle: BASELINE.json's north star asks for loss / metric parity with the reference's fp32 path within 1e-3 relative.
Kernel checks compare with plain torch fp32 on the CPU (tolerance 2e-5 relative: fp32 products in a different summation
order); the model checks are loss <= 1e-4, logits <= 1e-3 (relative L2), every gradient <= 2e-3 relative L2."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import whisper_oracle as O  # noqa: E402
from whisper_finetune.engine import ops32  # noqa: E402
from whisper_finetune.engine.whisper_model import MODEL_DIMS, ModelDimensions, Whisper  # noqa: E402
from whisper_finetune.model import lora as lora_mod  # noqa: E402
from whisper_finetune.model import model_utils  # noqa: E402

DEV = torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


@pytest.mark.parametrize("M,N,K,batch", [(64, 64, 16, 1), (70, 130, 33, 1), (1500, 384, 240, 1), (37, 64, 1500, 3), (1, 1, 1, 1)])
def test_gemm_f32_strided_forms(M, N, K, batch):
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(batch, M, K, generator=g)
    b = torch.randn(batch, N, K, generator=g)
    bias = torch.randn(N, generator=g)
    ad, bd = a.to(DEV), b.to(DEV)
    # NT with bias
    got = ops32.gemm(ad, bd, M=M, N=N, K=K, a_strides=(K, 1, M * K), b_strides=(1, K, N * K), batch=batch, bias=bias.to(DEV))
    ref = a @ b.transpose(1, 2) + bias
    assert rel(got.view(batch, M, N), ref) < 2e-5
    # TN (weight-gradient form): A(m, k) = at[k, m]
    at = a.transpose(1, 2).contiguous().to(DEV)  # [batch, K, M]
    got = ops32.gemm(at, bd, M=M, N=N, K=K, a_strides=(1, M, M * K), b_strides=(1, K, N * K), batch=batch)
    assert rel(got.view(batch, M, N), a @ b.transpose(1, 2)) < 2e-5
    # accumulate into C with alpha / beta
    c0 = torch.randn(batch, M, N, generator=g)
    cd = c0.clone().to(DEV)
    ops32.gemm(ad, bd, M=M, N=N, K=K, a_strides=(K, 1, M * K), b_strides=(1, K, N * K), batch=batch, out=cd, ldc=N, c_bs=M * N,
               alpha=0.5, beta=2.0)
    assert rel(cd, 0.5 * (a @ b.transpose(1, 2)) + 2.0 * c0) < 2e-5
    # bitwise reproducible
    again = ops32.gemm(at, bd, M=M, N=N, K=K, a_strides=(1, M, M * K), b_strides=(1, K, N * K), batch=batch)
    assert torch.equal(got, again)


def test_f32_ops_match_torch():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 50, 128, generator=g).requires_grad_(True)
    gam = (1 + 0.1 * torch.randn(128, generator=g)).requires_grad_(True)
    bet = (0.1 * torch.randn(128, generator=g)).requires_grad_(True)
    w = torch.randn(2, 50, 128, generator=g)
    # LayerNorm with a deep-SpecAugment mask (rows 5..9 of every clip and channels 20..29 zeroed)
    xd, gd, bd = (t.detach().to(DEV).requires_grad_(True) for t in (x, gam, bet))
    y = ops32.LayerNormFn.apply(xd, gd, bd, 1e-5, (50, 5, 10, 20, 30))
    (y * w.to(DEV)).sum().backward()
    ref = torch.nn.functional.layer_norm(x, (128,), gam, bet, 1e-5).clone()
    mask = torch.ones_like(ref)
    mask[:, 5:10, :] = 0
    mask[:, :, 20:30] = 0
    ref = ref * mask
    (ref * w).sum().backward()
    assert rel(y, ref) < 1e-5 and rel(xd.grad, x.grad) < 1e-4 and rel(gd.grad, gam.grad) < 1e-4 and rel(bd.grad, bet.grad) < 1e-4
    # GELU
    xg = torch.randn(1000, generator=g).requires_grad_(True)
    xgd = xg.detach().to(DEV).requires_grad_(True)
    ops32.GeluFn.apply(xgd).sum().backward()
    torch.nn.functional.gelu(xg).sum().backward()
    assert rel(ops32.GeluFn.apply(xgd), torch.nn.functional.gelu(xg)) < 1e-6 and rel(xgd.grad, xg.grad) < 1e-5
    # attention: self (non-causal), causal, cross
    for Tq, Tk, causal in ((70, 70, False), (33, 33, True), (20, 70, False)):
        q = torch.randn(2, Tq, 128, generator=g).requires_grad_(True)
        k = torch.randn(2, Tk, 128, generator=g).requires_grad_(True)
        v = torch.randn(2, Tk, 128, generator=g).requires_grad_(True)
        wo = torch.randn(2, Tq, 128, generator=g)
        qd, kd, vd = (t.detach().to(DEV).requires_grad_(True) for t in (q, k, v))
        o = ops32.AttentionFn.apply(qd, kd, vd, 2, causal)
        (o * wo.to(DEV)).sum().backward()
        qh, kh, vh = (t.view(2, -1, 2, 64).transpose(1, 2) for t in (q, k, v))
        s = qh @ kh.transpose(-1, -2) * 0.125
        if causal:
            s = s + torch.full((Tq, Tk), float("-inf")).triu_(1)
        oref = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(2, Tq, 128)
        (oref * wo).sum().backward()
        assert rel(o, oref) < 1e-5, (Tq, Tk, causal)
        assert max(rel(qd.grad, q.grad), rel(kd.grad, k.grad), rel(vd.grad, v.grad)) < 1e-4, (Tq, Tk, causal)
    # cross entropy with label smoothing and ignored rows
    lg = torch.randn(12, 1000, generator=g).requires_grad_(True)
    tg = torch.randint(0, 1000, (12,), generator=g)
    tg[[1, 7]] = -100
    lgd = lg.detach().to(DEV).requires_grad_(True)
    loss = ops32.CrossEntropyFn.apply(lgd * 1.0, tg.to(DEV), 0.1)
    loss.backward()
    lref = torch.nn.functional.cross_entropy(lg, tg, label_smoothing=0.1)
    lref.backward()
    assert abs(loss.item() - lref.item()) < 1e-5 * lref.item() and rel(lgd.grad, lg.grad) < 1e-5


@pytest.mark.parametrize("Tq,Tk,causal", [(130, 130, True), (50, 333, False)])
def test_f32_attention_on_probe_operands(Tq, Tk, causal):
    """ops32.AttentionFn (wft_gemm_f32 + wft_softmax_fwd_f32 / _bwd_f32, the causal mask and the ld handling) on the probe operands of
    tests/_attn_probe.py: every row's softmax mass sits on two keys at tile edges, next to a decoy the row must not see (causal:
    key i + 1; non-causal: the guard row behind key Tk - 1 that the packed k / v views exclude).  Judged per (row, head) against the
    fp64 oracle of the same fp32 operands, with test_f32_ops_match_torch's figures (1e-5 forward, 1e-4 gradients) applied to each
    row's own scale and the probe tests' floor, where that test has three flat-softmax shapes under a tensor-wide L2."""
    from tests import _attn_probe as P

    B, H = 3, 2
    D = H * 64
    c = P.probe_case(B, H, Tq, Tk, causal, seed=0)
    qkv, kv = c.qkv.float().to(DEV), c.kv.float().to(DEV)   # bf16 values held in fp32: the oracle reads the same numbers
    q, k, v = (t.requires_grad_(True) for t in (qkv[..., :D], kv[:, :Tk, :D], kv[:, :Tk, D:]))
    assert q.stride(1) == 3 * D and k.stride(0) == (Tk + P.GUARD) * 2 * D
    o = ops32.AttentionFn.apply(q, k, v, H, causal)
    o.backward(c.do.float().to(DEV))
    o64, lse64 = P.oracle_fwd(c)
    rdq, rdk, rdv = P.oracle_bwd(c, o64, lse64)
    P.close_rows(o, o64, 1e-5, P.FLOOR, "fp32 o")
    for name, got, ref in (("dq", q.grad, rdq), ("dk", k.grad, rdk), ("dv", v.grad, rdv)):
        P.close_rows(got, ref, 1e-4, P.FLOOR, f"fp32 {name}")


def _tiny_case(B=2, S=24, seed=0):
    dims = O.DIMS["tiny"]
    params = O.init_params(dims, seed=seed)
    g = torch.Generator().manual_seed(5)
    for k, v in params.items():
        if k.endswith("bias"):
            params[k] = torch.randn(v.shape, generator=g) * 0.02
        elif "ln" in k and k.endswith("weight"):
            params[k] = 1 + torch.randn(v.shape, generator=g) * 0.05
    audio, y_in, y_out = O.synthetic_batch(dims, B, S)
    y_out[0, :3] = -100
    return dims, params, audio, y_in, y_out


def test_tiny_fp32_step_matches_the_fp32_oracle_to_1e3():
    """BASELINE configs[0] arithmetic (whisper-tiny, 2 synthetic clips, fp32): logits within 1e-3, loss within 1e-4, every
    gradient within 2e-3 (relative L2) of the CPU oracle; the teacher-forced argmax is bit-exact where the oracle's top-2
    margin exceeds 1e-4."""
    dims, params, audio, y_in, y_out = _tiny_case()
    p_req = {k: v.clone().requires_grad_(k != "encoder.positional_embedding") for k, v in params.items()}
    mel = O.log_mel_spectrogram(audio, dims.n_mels)
    logits_ref = O.Oracle(dims, p_req).forward(mel, y_in)
    loss_ref = O.cross_entropy(logits_ref, y_out, 0.1)
    loss_ref.backward()
    m = Whisper(ModelDimensions(**vars(dims)))
    m.load_state_dict(params)
    m.to(DEV).set_compute_dtype("fp32").train()
    loss = m(mel.to(DEV), y_in.to(DEV), targets=y_out.to(DEV), label_smoothing=0.1)
    loss.backward()
    assert abs(loss.item() - loss_ref.item()) < 1e-4 * loss_ref.item(), (loss.item(), loss_ref.item())
    errs = {n: rel(p.grad, p_req[n].grad) for n, p in m.named_parameters()}
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    assert worst[0][1] < 2e-3, worst
    m.eval()
    with torch.no_grad():
        logits = m(mel.to(DEV), y_in.to(DEV))
    assert logits.dtype == torch.float32 and rel(logits, logits_ref) < 1e-3
    top2 = logits_ref.detach().topk(2, -1).values
    decisive = (top2[..., 0] - top2[..., 1]) > 1e-4
    assert torch.equal(logits.cpu().argmax(-1)[decisive], logits_ref.argmax(-1)[decisive])


def test_fp32_mode_with_lora_stochastic_depth_and_deep_specaug():
    """The training-time extras in fp32 mode: LoRA with a fixed dropout mask (parametrization form), stochastic depth and the
    deep-SpecAugment mask with the host draws replayed — loss within 1e-4, adapter gradients within 2e-3 of the oracle."""
    dims, params, audio, y_in, y_out = _tiny_case()
    from whisper_finetune.model.model_utils import CheckpointedStochasticAudioEncoder, CheckpointedStochasticTextDecoder

    m = Whisper(MODEL_DIMS["tiny"])
    m.encoder = CheckpointedStochasticAudioEncoder(dims.n_mels, dims.n_audio_ctx, dims.n_audio_state, dims.n_audio_head, dims.n_audio_layer, 0.3)
    m.decoder = CheckpointedStochasticTextDecoder(dims.n_vocab, dims.n_text_ctx, dims.n_text_state, dims.n_text_head, dims.n_text_layer, 0.3)
    m.load_state_dict(params)
    torch.manual_seed(31)  # lora_A's kaiming init draws from the global generator: the same adapters in every run
    lora_mod.apply_lora(m, {"rank": 8, "lora_alpha": 16, "lora_dropout": 0.25})
    g = torch.Generator().manual_seed(9)
    cfg, adapters = {}, {}
    for n, mod in m.named_modules():
        if "parametrizations" in mod._modules:
            ad = mod.parametrizations.weight[0]
            with torch.no_grad():
                ad.lora_B.copy_(torch.randn(ad.lora_B.shape, generator=g) * 0.05)
            mask = (torch.rand(1, ad.lora_A.shape[1], generator=g) >= 0.25).float() / 0.75
            cfg[n] = (ad.lora_A.detach().clone().requires_grad_(True), ad.lora_B.detach().clone().requires_grad_(True), ad.scaling, mask)
            adapters[n] = (ad, mask)
    m.to(DEV).set_compute_dtype("fp32").train()
    for ad, mask in adapters.values():
        ad.draw_mask = (lambda mk: (lambda training: mk))(mask.to(DEV))
    model_utils.register_deep_spec_augment_hooks(m, time_mask_param=100, freq_mask_param=27, p=1.0)
    mel = O.log_mel_spectrogram(audio, dims.n_mels)
    torch.manual_seed(77)
    state = torch.get_rng_state()
    enc_skips, masks = [], {}
    for i in range(dims.n_audio_layer):
        s = torch.rand(1).item() < 0.3
        enc_skips.append(s)
        if not s and i < dims.n_audio_layer - 1:
            masks[i] = O.draw_mask_span(100, dims.n_audio_ctx) + O.draw_mask_span(27, dims.n_audio_state)
    dec_skips = [torch.rand(1).item() < 0.3 for _ in range(dims.n_text_layer)]
    ref_logits = O.Oracle(dims, params, lora=cfg).forward(mel, y_in, enc_sd_p=0.3, enc_training=True, enc_skips=enc_skips, enc_ln_masks=masks,
                                                          dec_sd_p=0.3, dec_training=True, dec_skips=dec_skips)
    ref_loss = O.cross_entropy(ref_logits, y_out, 0.1)
    ref_loss.backward()
    torch.set_rng_state(state)
    loss = m(mel.to(DEV), y_in.to(DEV), targets=y_out.to(DEV), label_smoothing=0.1)
    loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 1e-4 * ref_loss.item(), (loss.item(), ref_loss.item())
    errs = []
    for n, (A, Bm, _, _) in cfg.items():
        ad = adapters[n][0]
        if A.grad is None:
            assert ad.lora_A.grad is None
            continue
        errs += [rel(ad.lora_A.grad, A.grad), rel(ad.lora_B.grad, Bm.grad)]
    assert errs and max(errs) < 2e-3, max(errs)


def test_train_step_in_fp32_mode_reproduces_the_references_loss_sequence():
    """tests/golden/ref_train_step.npz (the REFERENCE'S OWN train_step, fp32, 4 optimizer steps x 2 micro-batches): the engine
    in fp32 mode under this package's train_step reproduces every loss within 1e-4 and the final parameter norms within 1e-4."""
    from pathlib import Path
    from tests.golden.gen_golden import ARCH_DIMS, TRAIN_STEP_CFG, TRAIN_STEP_OPT, arch_params, train_step_case
    from whisper_finetune.model.optimizer import WftAdamW
    from whisper_finetune.model.scheduler import get_scheduler

    ref = np.load(Path(__file__).parent / "golden" / "ref_train_step.npz")
    m = Whisper(ModelDimensions(**vars(ARCH_DIMS)))
    m.load_state_dict(arch_params(ARCH_DIMS, seed=3))
    m.to(DEV).set_compute_dtype("fp32")
    opt = WftAdamW(m.parameters(), **TRAIN_STEP_OPT)
    sched = get_scheduler(opt, {"type": "linear", "warmup_steps": 2}, 4)
    it = iter(train_step_case())
    losses = [model_utils.train_step(m, it, opt, sched, dict(TRAIN_STEP_CFG), step=s) for s in range(1, 5)]
    np.testing.assert_allclose(losses, ref["losses"], rtol=1e-4)
    for n, p in m.named_parameters():
        want = float(ref["final_norm/" + n])
        assert abs(p.detach().float().norm().item() - want) < 1e-4 * want + 1e-7, n


def test_finetune_entrypoint_runs_the_fp32_config(tmp_path):
    """mixed_precision_training: False in the YAML -> fp32 compute mode end to end (configs[0]-shaped plumbing run)."""
    from pathlib import Path
    import yaml
    import whisper_finetune.runtime as rt
    from whisper_finetune.scripts import finetune

    cfg = yaml.safe_load((Path(__file__).resolve().parents[1] / "configs" / "DEBUG_synthetic.yaml").read_text())
    cfg["save_dir"] = str(tmp_path)
    cfg["training"]["mixed_precision_training"] = False
    cfg["dataset"]["synthetic"] = {"train": 8, "val": 2}
    losses = finetune.main(cfg)
    assert len(losses) == 4 and all(np.isfinite(l) for l in losses)
    rt.cleanup()
