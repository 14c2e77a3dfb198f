"""Validation on the device: the per-clip reconstruction loss of a padded batch (ast_recon_loss_len through
ast_amd.reconstruction_losses) against the float64 reference of tests/recon_len_ref.py, its isolation from padded sections, and
Trainer.evaluate -- against an eval-mode oracle forward, against direct module calls, on a ragged batch, and for what it must
leave untouched (state digest, module modes, the following training steps)."""
import math

import numpy as np
import pytest
import torch

import recon_len_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import ast_amd
    from ast_amd import _lib, config, train
    from ast_amd.losses import RECON_KEYS

# ---- the error bound of the kernel tests -------------------------------------------------------------------------------------
# Worst |value - float64 reference| / |reference| of ast_recon_loss_total (grad = NULL), the batch kernel this one stands beside,
# over five runs on the equal-length version of each case (the same tensors, every clip full), for the eleven numbers
# [5 sums][total][5 means]: profiles/validation/measure.py errors.  The per-clip kernel is allowed 4 x that per quantity (its
# reduction order differs and each clip sums fewer terms), as a fraction of |reference|.
# One floor, from the number format: a figure below 2^-24 says where the exact value happens to lie between two neighbouring f32
# numbers, not how accurate a kernel is -- rounding the EXACT result to f32 already costs up to 2^-24 of it.  The batch kernel's
# figure is therefore taken as max(measured, 2^-24).  Without the floor, the small cases would ask for 4.0e-9 (total of
# small-ragged: the batch kernel measured 9.9e-10), 4.3e-8 and 7.4e-8 (mag, spectral means), and 1.7e-8, 8.8e-8, 3.6e-8 (spectral
# sum, total, mse mean of small-full), where this kernel measured 7.4e-8, 8.7e-8, 1.1e-7 and 1.1e-7, 1.5e-7, 8.5e-8: one to three
# f32 roundings.  On the two large cases it measured at most 1.2 x the batch kernel's own figure on any quantity.
PARENT_ERR = {
    "small-ragged": (2.737e-08, 2.099e-08, 7.606e-08, 3.83e-08, 2.21e-08, 9.896e-10, 4.392e-08, 1.083e-08, 9.985e-08, 5.38e-08, 1.847e-08),
    "small-full": (2.119e-08, 3.829e-08, 5.45e-08, 6.036e-08, 4.248e-09, 2.212e-08, 8.921e-09, 3.217e-08, 7.596e-08, 1.031e-07, 4.069e-08),
    "real-size": (8.365e-08, 1.775e-07, 8.748e-08, 1.278e-07, 1.763e-07, 1.357e-07, 8.24e-08, 1.679e-07, 4.684e-08, 1.235e-07, 2.157e-07),
    "strided-bins": (3.43e-07, 1.037e-07, 1.326e-07, 2.868e-07, 1.497e-07, 1.106e-07, 3.133e-07, 7.082e-08, 1.209e-07, 2.794e-07, 1.798e-07),
}
BOUND_FACTOR, F32_ROUNDING = 4.0, 2.0 ** -24


def _bound(case_name):
    return BOUND_FACTOR * np.maximum(np.asarray(PARENT_ERR[case_name]), F32_ROUNDING)


def _res11(parts):
    """the dict of reconstruction_losses -> (B, 11) float64 in the kernel's layout (the raw sums are not part of the dict: NaN)"""
    cols = [parts[k].double().cpu().numpy() for k in ("total_loss",) + tuple(RECON_KEYS)]
    return np.stack([np.full_like(cols[0], np.nan)] * 5 + cols, axis=1)


def _raw(out, tgt, ld, n, mse_weight=2.0):
    """ast_recon_loss_len through the C ABI -> (B, 11) float32 tensor (all eleven numbers)"""
    import ctypes
    B, S, _, T, F = out.shape
    lib = _lib.lib()
    need = int(lib.ast_recon_loss_len_ws_floats(B, S, T, F))
    ws = torch.full((need,), float("nan"), device="cuda")
    res = torch.full((B, 11), float("nan"), device="cuda")
    c5 = (ctypes.c_float * 5)(mse_weight, 0.5, 0.2, 0.3, 0.1)
    _lib.check(lib.ast_recon_loss_len(out.data_ptr(), tgt.data_ptr(), ld, B, S, T, F, None if n is None else n.data_ptr(), c5, ws.data_ptr(),
                                      need, res.data_ptr(), None), "ast_recon_loss_len")
    return res


def _case(name):
    _, B, S, T, F, ld, n = next(c for c in R.CASES if c[0] == name)
    out, x = R.make_case(B, S, T, F, ld, seed=len(name))
    return out, x, F, ld, n


def _dev_n(n):
    return None if n is None else torch.tensor(n, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_kernel_against_float64_reference(name):
    out, x, F, ld, n = _case(name)
    ref = R.recon_len_ref(out, x[..., :F], n)
    o, xd = torch.from_numpy(out).cuda(), torch.from_numpy(x).cuda()
    got = _raw(o, xd, ld, _dev_n(n)).double().cpu().numpy()
    via_op = _res11(ast_amd.reconstruction_losses(o, xd[..., :F], _dev_n(n)))
    assert np.array_equal(via_op[:, 5:], got[:, 5:])                       # the public op is the same call
    bound = _bound(name)
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
    print(name, "worst relative error per quantity:", " ".join(f"{e:.2e}" for e in err.max(axis=0)), "| bound:", " ".join(f"{b:.2e}" for b in bound))
    if n is not None:
        for b, nb in enumerate(n):
            if nb == 1:
                assert got[b, 3] == 0.0 and got[b, 9] == 0.0               # the temporal term of a one-section clip is exactly 0.0f
    assert np.isfinite(got).all()
    assert (np.abs(got - ref) <= bound[None, :] * np.abs(ref)).all(), (name, err.max(axis=0), bound)


def test_mse_weight_of_the_simple_decoder():
    out, x, F, ld, n = _case("small-ragged")
    ref = R.recon_len_ref(out, x[..., :F], n, mse_weight=1.0)
    got = _raw(torch.from_numpy(out).cuda(), torch.from_numpy(x).cuda(), ld, _dev_n(n), mse_weight=1.0).double().cpu().numpy()
    assert (np.abs(got - ref) <= _bound("small-ragged")[None, :] * np.abs(ref)).all()


@pytest.mark.parametrize("name", ["small-ragged", "real-size"])
def test_padded_sections_cannot_reach_a_result(name):
    out, x, F, ld, n = _case(name)
    B = out.shape[0]
    dn = _dev_n(n)

    def run(fill):
        o, xx = out.copy(), x.copy()
        for b, nb in enumerate(n):
            o[b, nb:], xx[b, nb:] = fill, fill
        return _raw(torch.from_numpy(o).cuda(), torch.from_numpy(xx).cuda(), ld, dn)

    zero = run(0.0)
    assert torch.equal(run(0.0), zero)                                     # two runs of the same call: bit-identical
    for fill in (float("nan"), 1e30):
        assert torch.equal(run(fill).view(torch.int32), zero.view(torch.int32)), fill
    # clip b alone (B = 1, S = n_b) against its row in the batch, within the kernel's bound (the grid per clip and the slot order
    # depend on T * F alone, so the two are in fact the same bits; the bound is what is asked)
    bound = _bound(name)
    for b, nb in enumerate(n):
        alone = _raw(torch.from_numpy(out[b:b + 1, :nb].copy()).cuda(), torch.from_numpy(x[b:b + 1, :nb].copy()).cuda(), ld, None)
        a, z = alone[0].double().cpu().numpy(), zero[b].double().cpu().numpy()
        print(name, "clip", b, "alone against its row, worst relative difference:", float((np.abs(a - z) / np.maximum(np.abs(z), 1e-300)).max()))
        assert (np.abs(a - z) <= bound * np.abs(z)).all(), (b, a, z)


def test_equal_length_mean_of_clips_is_the_batch_loss():
    out, x, F, ld, _ = _case("small-full")
    o, tgt = torch.from_numpy(out).cuda(), torch.from_numpy(x).cuda()[..., :F]
    per_clip = ast_amd.reconstruction_losses(o, tgt)
    batch = ast_amd.compute_comprehensive_loss(o, tgt)
    ref = R.recon_len_ref(out, x[..., :F], None)
    bound = _bound("small-full")
    for j, k in enumerate(("total_loss",) + tuple(RECON_KEYS)):
        m, bt, r = float(per_clip[k].double().mean()), float(batch[k]), float(ref[:, 5 + j].mean())
        print(k, "mean of clips against the reference:", abs(m - r) / abs(r), "against the batch kernel:", abs(m - bt) / abs(r), "bound:", bound[5 + j])
        assert abs(m - r) <= bound[5 + j] * abs(r) and abs(m - bt) <= bound[5 + j] * abs(r), (k, m, bt, r)


# ---- Trainer.evaluate ------------------------------------------------------------------------------------------------------------
REL, ABS = 2e-3, 2e-4              # what tests/test_gpu_trainer.py applies to the f32 training step's loss terms against the oracle


def _seeded_trainer(decoder="new", use_graph=False, deterministic=None, warm_x=None):
    """A Trainer on the oracle's seeded parameters whose BatchNorm running statistics are those of real activations (one training
    forward with momentum 1: the seeded ones let eval-mode activations explode)."""
    from oracle import seeded_params as sp
    ast_amd.set_compute_dtype(torch.float32)
    tr = train.Trainer(train.TrainConfig(use_graph=use_graph, dropout=False, decoder=decoder, deterministic=deterministic), seed=7)
    tags = (("style", tr.style), ("content", tr.content), ("simple_decoder" if decoder == "simple" else "decoder", tr.decoder), ("disc", tr.disc))
    for tag, m in tags:
        m.load_state_dict({k: v.to("cuda") for k, v in sp.seeded_state_dict(m.state_dict(), tag=tag).items()})
    x0 = sp.seeded_input(2, 2, seed=9).cuda() if warm_x is None else warm_x
    labels = sp.balanced_labels(x0.shape[0])
    bns = [m for _, mod in tags for m in mod.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for m in bns:
        m.momentum = 1.0
    with torch.no_grad():
        s, k = tr.style(x0, labels)
        c = tr.content(x0)
        tr.decoder(c, k[labels.cuda()].contiguous(), y=x0[..., :513])
    for m in bns:
        m.momentum = 0.1
    torch.cuda.synchronize()
    return tr, tags


@pytest.fixture(scope="module")
def eager():
    return _seeded_trainer()


def _floats(res):
    return {k: (v.double().cpu().numpy() if k != "rec_parts" else {p: q.double().cpu().numpy() for p, q in v.items()}) for k, v in res.items()}


def _oracle_eval(tags, x, labels, simple):
    """OracleTrainer.forward_losses without the discriminator step, in eval mode, with the teacher-forced decoder."""
    from oracle import ast_oracle as O
    sds = {tag.replace("simple_", ""): {k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for tag, m in tags}
    cfg = O.Cfg(training=False, p_drop=0.0)
    xc = x.cpu()
    y = xc[..., :513]
    B, S = xc.shape[:2]
    with torch.no_grad():
        style, cls = O.style_encoder_forward(sds["style"], xc, labels, cfg)
        content = O.content_encoder_forward(sds["content"], xc, cfg)
        sd = sds["decoder"]
        memory = O.decoder_prepare_memory(sd, content, cls[labels], cfg)
        d = memory.shape[-1]
        if simple:
            emb = O.linear(sd, "stft_to_embedding.", y.reshape(B * S, -1)).view(B, S, d)
        else:
            emb = O.decoder_encode_input(sd, y.reshape(B * S, *y.shape[2:]), cfg).view(B, S, d)
        tgt = torch.cat([sd["start_token"].expand(B, 1, -1), emb[:, :-1]], dim=1)
        tgt = O.layernorm(sd, "input_norm.", tgt + O.positional_encoding(S, d))
        tok = O._decoder_stack(sd, tgt, memory, 4, 4, cfg)
        if simple:
            out = O.linear(sd, "embedding_to_stft.", O.layernorm(sd, "output_norm.", tok)).reshape(B, S, 2, 287, 513)
        else:
            out = O.decoder_generate_output(sd, tok, cfg)
        w = 1.0 if simple else 2.0
        rec = [O.comprehensive_loss(out[b:b + 1], y[b:b + 1], mse_weight=w) for b in range(B)]
        d_loss, g_adv = O.adversarial_loss(sds["disc"], style, cls, content, labels, False)
        terms = {"rec": np.array([float(r["total_loss"]) for r in rec]), "nce": float(O.infonce_loss(style, labels)),
                 "margin": float(O.margin_loss(cls)), "hsic": float(O.disentanglement_loss(style, content.mean(1))),
                 "adv_g": float(g_adv), "adv_d": float(d_loss)}
        terms["rec_parts"] = {k: np.array([float(r[k]) for r in rec]) for k in ("total_loss",) + tuple(RECON_KEYS)}
        batch_total = float(O.comprehensive_loss(out, y, mse_weight=w)["total_loss"])
    total = terms["rec"].mean()
    for k in ("margin", "nce", "hsic", "adv_g"):
        total = total + terms[k]
    terms["total"] = float(total)
    return terms, batch_total


def _close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    print(what, got, ref)
    # math.isclose's rule, as tests/test_gpu_trainer.py applies it: the larger of the relative and the absolute allowance
    assert np.all(np.abs(got - ref) <= np.maximum(REL * np.maximum(np.abs(got), np.abs(ref)), ABS)), (what, got, ref)


@pytest.mark.parametrize("decoder", ["new", "simple"])
def test_evaluate_teacher_forced_against_the_oracle(decoder, eager):
    from oracle import seeded_params as sp
    tr, tags = eager if decoder == "new" else _seeded_trainer("simple")
    x, labels = sp.seeded_input(2, 2).cuda(), sp.balanced_labels(2)
    got = _floats(tr.evaluate(x, labels, decode="teacher_forced"))
    ref, batch_total = _oracle_eval(tags, x, labels, decoder == "simple")
    for k in ("rec", "nce", "margin", "hsic", "adv_d", "adv_g", "total"):
        _close(got[k], ref[k], k)
    for k, v in ref["rec_parts"].items():
        _close(got["rec_parts"][k], v, k)
    _close(got["rec"].mean(), batch_total, "mean of rec against the batch loss")      # equal lengths: up to rounding
    assert all(m.training for _, m in tags)


def test_simple_decoder_eval_teacher_forcing_against_the_reference_fixture(golden_dir):
    """tests/golden/simple_b2s2.npz records the real reference's teacher-forced SimpleDecoder output and its 1.0-MSE-weight loss for
    DECODER inputs (content, class rows, y: seeds 4101-4103, 513 bins).  `evaluate` takes x and forms content and class rows with
    the encoders, so those inputs do not fit it (the case above uses seeded_input for that reason); they do fit the two parts
    `evaluate` adds around the encoders: forward_teacher_forced in eval mode (no dropout in the fixture, no BatchNorm in this
    decoder, so eval equals the recorded training-mode pass) and reconstruction_losses, whose mean over the equal-length clips
    is the recorded batch loss.  Bounds: those of tests/test_gpu_models.py for the same fixture."""
    import os
    from ast_amd import SimpleDecoder_TransformerOnly as SD
    from oracle import seeded_params as sp
    g = np.load(os.path.join(golden_dir, "simple_b2s2.npz"), allow_pickle=False)
    ast_amd.set_compute_dtype(torch.float32)
    m = SD.Decoder()
    m.load_state_dict(sp.seeded_state_dict(m.state_dict(), tag="simple_decoder"))
    m = m.cuda().eval()
    content, cls = sp.seeded_normal((2, 2, 256), 4101).cuda(), sp.seeded_normal((2, 256), 4102).cuda()
    y = sp.seeded_input(2, 2, seed=4103, F=513).cuda()
    with torch.no_grad():
        out = m.forward_teacher_forced(content, cls, y)
        full = m.forward_teacher_forced(content, cls, y, lengths=torch.tensor([2, 2], dtype=torch.int32, device="cuda"))
        rec = ast_amd.reconstruction_losses(out, y, mse_weight=1.0)
    sub, ref = out[:, :, :, ::11, ::13].cpu(), torch.from_numpy(g["out_sub"])
    assert float((sub - ref).norm() / ref.norm()) < 1e-3
    assert float((full - out).norm() / out.norm()) < 1e-3                             # lengths that pad nothing: the same output, other kernels
    for k in ("total_loss",) + tuple(RECON_KEYS):
        assert math.isclose(float(rec[k].double().mean()), float(g["rec_" + k]), rel_tol=1e-3, abs_tol=1e-6), k


@pytest.mark.parametrize("mode", ["recompute", "kv_cache"])
def test_evaluate_autoregressive_is_the_eval_mode_forward(mode, eager):
    from oracle import seeded_params as sp
    tr, tags = eager
    x, labels = sp.seeded_input(4, 3, seed=21).cuda(), sp.balanced_labels(4)
    n = torch.tensor([3, 1, 2, 3], dtype=torch.int32, device="cuda")
    saved = (type(tr.decoder).decode_mode, config.deterministic)
    type(tr.decoder).decode_mode = mode
    config.set_deterministic(True)            # no f32 atomics in the forward pass either: the two runs can be compared bit for bit
    try:
        got = tr.evaluate(x, labels, n, decode="autoregressive")["rec"].clone()
        for _, m in tags:
            m.eval()
        with torch.no_grad():
            _, cls = tr.style(x, labels, n)
            content = tr.content(x, n)
            out = tr.decoder(content, cls[labels.cuda()].contiguous(), lengths=n)
            want = ast_amd.reconstruction_losses(out, x[..., :513], n)["total_loss"]
    finally:
        type(tr.decoder).decode_mode, config.deterministic = saved
        for _, m in tags:
            m.train()
    assert torch.equal(got, want), (got, want)


@pytest.mark.parametrize("decode", ["teacher_forced", "autoregressive"])
def test_evaluate_on_a_ragged_batch(decode, eager):
    """Eval-mode BatchNorm makes the models per-sample, so the full-length clips 0 and 3 of the ragged batch must give what they
    give as an equal-length batch of their own.  One thing still couples class-mates: the class prototype a clip is decoded with
    is the mean style embedding of its class, and `evaluate` on the sub-batch alone would form it from clip 0 (clip 3) only.  The
    sub-batch therefore goes through the same modules directly, decoded with the prototypes of the ragged batch.  NaN in the
    padded sections of x changes no output bit, and counts outside [1, S_max] clamp."""
    from oracle import seeded_params as sp
    tr, tags = eager
    x = sp.seeded_input(4, 3, seed=22).cuda()
    labels = torch.tensor([0, 0, 1, 1])
    n_host = [3, 1, 2, 3]
    n = torch.tensor(n_host, dtype=torch.int32, device="cuda")
    for b, nb in enumerate(n_host):
        x[b, nb:] = 0.0
    prev = config.deterministic
    config.set_deterministic(True)                # no f32 atomics in the forward pass either: runs can be compared bit for bit
    try:
        _ragged_checks(tr, tags, x, labels, n_host, n, decode)
    finally:
        config.deterministic = prev
        for _, m in tags:
            m.train()


def _ragged_checks(tr, tags, x, labels, n_host, n, decode):
    rag = tr.evaluate(x, labels, n, decode=decode)
    rag = {"rec": rag["rec"].clone(), "rec_parts": {k: v.clone() for k, v in rag["rec_parts"].items()},
           **{k: rag[k].clone() for k in ("nce", "margin", "hsic", "adv_d", "adv_g", "total")}}
    for _, m in tags:
        m.eval()
    with torch.no_grad():
        style4, cls = tr.style(x, labels, n)
        # the content embedding averaged over each clip's OWN sections, and the three terms it feeds
        content4 = tr.content(x, n)
        own_mean = torch.stack([content4[b, :nb].double().mean(dim=0) for b, nb in enumerate(n_host)])
        got_mean = tr._content_mean(content4, n).double()
        assert float((got_mean - own_mean).abs().max()) <= 1e-6 * float(own_mean.abs().max())
        assert float((content4.double().mean(dim=1) - own_mean)[1].abs().max()) > 1e-3 * float(own_mean.abs().max())   # / S_max would show
        from ast_amd.losses import embedding_loss_values
        emb = embedding_loss_values(style4, cls, own_mean.float(), tr.disc, labels)
        for k in ("hsic", "adv_d", "adv_g", "nce", "margin"):
            _close(float(rag[k]), float(emb[k]), k + " of the ragged batch")
        rows = cls[labels.cuda()][[0, 3]].contiguous()
        xs = x[[0, 3]].contiguous()
        content = tr.content(xs)
        out = tr.decoder.forward_teacher_forced(content, rows, xs[..., :513]) if decode == "teacher_forced" else tr.decoder(content, rows)
        sub = {k: v.double().cpu().numpy() for k, v in ast_amd.reconstruction_losses(out, xs[..., :513]).items()}
    for _, m in tags:
        m.train()
    _close(rag["rec"][[0, 3]].double().cpu().numpy(), sub["total_loss"], "rec of clips 0, 3")
    for k, v in sub.items():
        _close(rag["rec_parts"][k][[0, 3]].double().cpu().numpy(), v, k)
    assert float(rag["rec_parts"]["temporal_loss"][1]) == 0.0
    xn = x.clone()
    for b, nb in enumerate(n_host):
        xn[b, nb:] = float("nan")
    nan = tr.evaluate(xn, labels, n, decode=decode)
    for k in ("rec", "nce", "margin", "hsic", "adv_d", "adv_g", "total"):
        assert torch.equal(nan[k].view(torch.int32), rag[k].view(torch.int32)), k
    for k, v in rag["rec_parts"].items():
        assert torch.equal(nan["rec_parts"][k].view(torch.int32), v.view(torch.int32)), k
    # counts outside [1, S_max] clamp, as the front end's length kernels clamp
    wide = tr.evaluate(x, labels, torch.tensor([9, 0, 2, 3], dtype=torch.int32, device="cuda"), decode=decode)
    assert torch.equal(wide["rec"].view(torch.int32), rag["rec"].view(torch.int32))


def test_evaluate_leaves_state_and_modes_alone(eager):
    from oracle import seeded_params as sp
    tr, tags = eager
    x, labels = sp.seeded_input(2, 2).cuda(), sp.balanced_labels(2)
    before = tr.state_digest()
    for decode in train.Trainer.DECODE_MODES:
        out = tr.evaluate(x, labels, decode=decode)
        assert all(math.isfinite(float(out[k])) for k in ("total", "nce", "margin", "hsic", "adv_d", "adv_g"))
        assert tr.state_digest() == before, decode
        assert all(m.training for _, m in tags)
    with pytest.raises(ValueError, match="decode"):
        tr.evaluate(x, labels, decode="beam")
    with pytest.raises(ValueError, match="n_sections"):
        tr.evaluate(x, labels, torch.tensor([2, 2]))                      # int64, on the host: refused inside the pass's checks
    with pytest.raises(ValueError):
        tr.evaluate(x[:, :, :, :, :100], labels)
    assert all(m.training for _, m in tags) and tr.state_digest() == before
    tr2 = train.Trainer.__new__(train.Trainer)
    tr2.world = 2
    with pytest.raises(ValueError, match="per process"):
        tr2.evaluate(x, labels)


def test_steps_around_evaluate_are_bit_identical_in_deterministic_mode():
    """step, step, evaluate, step == step, step, step (losses and final digest), with an evaluate before the first capture, one
    after it, and a replay of the captured evaluation for a second mix of lengths without a new capture; the digest stays put
    across every evaluate, graphs on."""
    x, labels = train.synthetic_batch(4, 2, "cuda:0", seed=3)
    n1 = torch.tensor([2, 1, 2, 1], dtype=torch.int32, device="cuda")
    n2 = torch.tensor([1, 2, 1, 2], dtype=torch.int32, device="cuda")

    def run(with_eval):
        ast_amd.set_compute_dtype(torch.float32)
        tr = train.Trainer(train.TrainConfig(use_graph=True, dropout=True, deterministic=True), seed=7)
        hist, evals = [], []

        def ev(n, decode="teacher_forced"):
            if with_eval:
                d = tr.state_digest()
                out = tr.evaluate(x, labels, n, decode=decode)
                evals.append(out["rec"].clone())
                assert tr.state_digest() == d and tr.style.training and tr.decoder.training

        ev(n1)                                                              # before the first capture of the step
        for i in range(3):
            hist.append({k: v.clone() for k, v in tr.step(x, labels).items()})
            if i == 0:
                ev(n1, "autoregressive")                                    # between capture + first replay and the second replay
            if i == 1:
                ev(n1)
                ev(n2)                                                      # a second mix of lengths: the same captured evaluation
        torch.cuda.synchronize()
        return hist, tr.state_digest(), tr, evals

    ref_hist, ref_digest, _, _ = run(False)
    hist, digest, tr, evals = run(True)
    assert digest == ref_digest
    for a, b in zip(hist, ref_hist):
        for k in b:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert len(tr._eval_graphs) == 2 and len(tr._graphs) == 1                # teacher-forced (three calls, two mixes) + autoregressive
    assert not torch.equal(evals[0], evals[2])                              # the parameters moved in between ...
    assert not torch.equal(evals[2], evals[3])                              # ... and the replay read the new lengths
