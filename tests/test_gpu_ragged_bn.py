"""BatchNorm over the live images of a padded batch on the device: ops.BatchNormActLenFn and the two masked layout ops against the
float64 references of tests/ragged_bn_ref.py, and new_decoder.Decoder.forward_training_ragged_bn against the compaction reference
(oracle CNN halves on the concatenated live sections, transformer clip by clip) under autograd in float64.

Tolerances are taken over, not derived here.  Op level: tests/test_gpu_ops.py::test_batchnorm_relu -- y 1e-4 (f32) / 1e-2 (bf16) of
the tensor scale, dx, dgamma and dbeta three times that, running statistics 1e-4.  Decoder level: tests/test_gpu_models.py -- f32
output 1e-3 of scale, whole-model gradient 1e-2 in relative L2, worst single parameter 3e-2; bf16 output 3e-2 in relative L2 and the whole-model gradient of its smooth surrogate loss 0.15."""
import functools
import math

import numpy as np
import pytest
import torch

import ragged_bn_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import ast_amd
    from ast_amd import config, layers as AL, ops
from oracle import layout as OL
from oracle import seeded_params as sp

DEV = "cuda"
Y_TOL = {torch.float32: 1e-4, torch.bfloat16: 1e-2}          # test_gpu_ops.py::test_batchnorm_relu
RUN_TOL = 1e-4
DTYPES = [torch.float32, torch.bfloat16]


def rel_err(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-12))


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / max(b.norm().item(), 1e-12))


def _dev_n(n):
    return torch.tensor(list(n), dtype=torch.int32, device=DEV)


def to_nhwc(x, dtype):
    return ops.nchw_to_nhwc(x.to(DEV).contiguous(), dtype)


def from_nhwc(y, C):
    return y[..., :C].permute(0, 3, 1, 2).float().cpu()


def _bn(gamma, beta, rm, rv):
    bn = torch.nn.BatchNorm2d(gamma.numel()).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    return bn


def _masked_run(name, dtype, poison=False):
    """one forward + backward of BatchNormActLenFn on the case -> (y, dx NHWC on the device; dgamma, dbeta, rm, rv, nbt)"""
    B, S, H, W, C, Creal, n = R.bn_case(name)
    x, dy, gamma, beta, rm, rv = R.bn_inputs(name)
    bn = _bn(gamma, beta, rm, rv)
    xh, dyh = to_nhwc(x, dtype), to_nhwc(dy, dtype)
    if poison:
        dead = torch.from_numpy(~R.live_mask(B, S, n)).to(DEV)
        xh[dead] = float("nan")
        dyh[dead] = float("nan")
    xh.requires_grad_(True)
    y = AL.bn_act_len(xh, bn, (_dev_n(n), S), relu=True)
    assert getattr(y, "_bn_link", None) is None
    y.backward(dyh)
    torch.cuda.synchronize()
    return y.detach(), xh.grad, bn.weight.grad, bn.bias.grad, bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)


def _unmasked_check(dtype):
    """the unmasked op right after, on the statistics scratch the masked op handed back: against its own float64 reference"""
    ops.stat_arena_reset(DEV)
    x, dy, gamma, beta, rm, rv = R.bn_inputs("full", seed=3)
    bn = _bn(gamma, beta, rm, rv)
    xh = to_nhwc(x, dtype).requires_grad_(True)
    y = AL.bn_act(xh, bn, True, relu=True)
    y.backward(to_nhwc(dy, dtype))
    xq, dq = from_nhwc(xh.detach(), x.shape[1]), from_nhwc(to_nhwc(dy, dtype), x.shape[1])
    live = np.ones(x.shape[0], dtype=bool)
    yr, _, _, rmr, rvr = R.masked_bn_relu_fwd(xq, gamma, beta, rm, rv, live)
    dxr, dgr, dbr = R.masked_bn_relu_bwd(xq, dq, gamma, beta, live)
    tol = Y_TOL[dtype]
    assert rel_err(from_nhwc(y, x.shape[1]), yr) < tol and rel_err(from_nhwc(xh.grad, x.shape[1]), dxr) < 3 * tol
    assert rel_err(bn.weight.grad, dgr) < 3 * tol and rel_err(bn.bias.grad, dbr) < 3 * tol
    assert rel_err(bn.running_mean, rmr) < RUN_TOL and rel_err(bn.running_var, rvr) < RUN_TOL


@pytest.fixture(autouse=True)
def _restore_compute_dtype():
    old = config.compute_dtype
    yield
    config.set_compute_dtype(old)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", R.BN_NAMES)
def test_masked_batchnorm_against_float64(name, dtype):
    B, S, H, W, C, Creal, n = R.bn_case(name)
    x, dy, gamma, beta, rm, rv = R.bn_inputs(name)
    live = R.live_mask(B, S, n)
    ops.stat_arena_reset(DEV)
    y, dx, dg, db, nrm, nrv, nbt = _masked_run(name, dtype)
    xq, dq = from_nhwc(to_nhwc(x, dtype), Creal), from_nhwc(to_nhwc(dy, dtype), Creal)      # the values the kernels see
    yr, _, _, rmr, rvr = R.masked_bn_relu_fwd(xq, gamma, beta, rm, rv, live)
    dxr, dgr, dbr = R.masked_bn_relu_bwd(xq, dq, gamma, beta, live)
    tol = Y_TOL[dtype]
    errs = dict(y=rel_err(from_nhwc(y, Creal), yr), dx=rel_err(from_nhwc(dx, Creal), dxr), dgamma=rel_err(dg, dgr), dbeta=rel_err(db, dbr),
                running_mean=rel_err(nrm, rmr), running_var=rel_err(nrv, rvr))
    print(name, dtype, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["y"] < tol and errs["dx"] < 3 * tol and errs["dgamma"] < 3 * tol and errs["dbeta"] < 3 * tol
    assert errs["running_mean"] < RUN_TOL and errs["running_var"] < RUN_TOL and nbt == 1
    dead = torch.from_numpy(~live).to(DEV)
    assert int((y[dead].view(torch.int16 if dtype == torch.bfloat16 else torch.int32) != 0).sum()) == 0       # bitwise 0
    assert int((dx[dead].view(torch.int16 if dtype == torch.bfloat16 else torch.int32) != 0).sum()) == 0
    if Creal < C:                                                         # padded channels: scale 0, so y and dx are 0 there
        assert int((y[..., Creal:] != 0).sum()) == 0 and int((dx[..., Creal:] != 0).sum()) == 0
    if name == "full":                                                     # every image live: ops.BatchNormActFn on the same input
        ops.stat_arena_reset(DEV)
        bn = _bn(gamma, beta, rm, rv)
        xh = to_nhwc(x, dtype).requires_grad_(True)
        yu = AL.bn_act(xh, bn, True, relu=True)
        yu.backward(to_nhwc(dy, dtype))
        assert rel_err(y, yu) < tol and rel_err(dx, xh.grad) < 3 * tol
        assert rel_err(dg, bn.weight.grad) < 3 * tol and rel_err(db, bn.bias.grad) < 3 * tol
        assert rel_err(nrm, bn.running_mean) < RUN_TOL and rel_err(nrv, bn.running_var) < RUN_TOL


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["one-unit", "eight-units", "padded-channels", "130-images", "clamped"])
def test_nan_in_dead_images_reaches_nothing_and_the_scratch_comes_back_clean(name, dtype):
    """Bit for bit: at these sizes a table row receives at most two atomic adds (one or two workgroups per image), and two floats
    add to the same bits in either order; the rows are then summed by one wave in a fixed order."""
    ops.stat_arena_reset(DEV)
    clean = _masked_run(name, dtype)
    ops.stat_arena_reset(DEV)
    bad = _masked_run(name, dtype, poison=True)
    for a, c in zip(clean[:6], bad[:6]):
        assert bool(torch.isfinite(c.float()).all())
        assert torch.equal(a, c)
    assert clean[6] == bad[6] == 1
    _unmasked_check(dtype)


def test_layout_ops_on_a_padded_batch():
    B, S, n = 2, 2, (2, 1)
    live = torch.from_numpy(R.live_mask(B, S, n)).to(DEV)
    nd = _dev_n(n)
    g = torch.Generator().manual_seed(11)
    for dtype in DTYPES:
        # NCHW -> NHWC, 6 x 10
        x = torch.randn(B * S, 2, 6, 10, generator=g).to(DEV)
        plain = ops.nchw_to_nhwc(x, dtype)
        xp = x.clone()
        xp[~live] = float("nan")
        for src in (x, xp):
            got = ops.nchw_to_nhwc_len(src, dtype, nd, S)
            assert torch.equal(got[live], plain[live]) and int((got[~live].float() != 0).sum()) == 0
            assert int((got[~live].view(torch.int16 if dtype == torch.bfloat16 else torch.int32) != 0).sum()) == 0
        # bilinear 8 x 4 -> 5 x 7, forward and backward
        h = torch.randn(B * S, 8, 4, 8, generator=g).to(DEV).to(dtype)
        dy = torch.randn(B * S, 2, 5, 7, generator=g).to(DEV)
        hu = h.clone().requires_grad_(True)
        yu = ops.BilinearToNCHWFn.apply(hu, 2, 5, 7)
        yu.backward(dy)
        hp, dyp = h.clone(), dy.clone()
        hp[~live], dyp[~live] = float("nan"), float("nan")
        for src, gy in ((h, dy), (hp, dyp)):
            hm = src.clone().requires_grad_(True)
            ym = ops.BilinearToNCHWLenFn.apply(hm, 2, 5, 7, nd, S)
            ym.backward(gy)
            assert torch.equal(ym[live], yu[live]) and torch.equal(hm.grad[live], hu.grad[live])
            assert int((ym[~live].view(torch.int32) != 0).sum()) == 0
            assert int((hm.grad[~live].view(torch.int16 if dtype == torch.bfloat16 else torch.int32) != 0).sum()) == 0


# ---- the decoder ---------------------------------------------------------------------------------------------------------------------
def _set_dropout(m, p):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = p
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = p


def _decoder():
    m = ast_amd.Decoder()
    m.load_state_dict(sp.seeded_state_dict(m.state_dict(), tag="decoder"))
    _set_dropout(m, 0.0)
    return m.to(DEV).train()


def _surrogate_weights(B, S, n):
    """fixed random weights of the smooth surrogate loss of tests/test_gpu_models.py (sum(out * w) / 50), zero on padded sections: the
    loss must give rows s >= n_b no gradient"""
    w = torch.randn(B, S, 2, 287, 513, generator=torch.Generator().manual_seed(5))
    w[~torch.from_numpy(R.live_mask(B, S, n)).view(B, S)] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def _reference(B, S, n, surrogate=False):
    """the float64 compaction reference, computed once per case: output, loss, {parameter name: gradient}.  surrogate: the gradient of
    the smooth surrogate loss instead of the reconstruction loss."""
    content, cls, y = R.decoder_inputs(B, S)
    sd = R.double_state(OL.seeded_model_state("decoder"))
    out = R.compaction_decoder(sd, content.double(), cls.double(), y.double(), n)
    loss = (out * _surrogate_weights(B, S, n).double()).sum() / 50.0 if surrogate else R.ragged_loss(out, y.double(), n)
    loss.backward()
    return out.detach(), float(loss.detach()), {k: v.grad for k, v in sd.items() if v.is_floating_point() and v.grad is not None}


def _step(dec, content, cls, y, n, entry="ragged", surrogate=None):
    for p in dec.parameters():
        p.grad = None
    ops.stat_arena_reset(DEV)
    nd = n if torch.is_tensor(n) else _dev_n(n)
    out = dec.forward_training_ragged_bn(content, cls, y, nd) if entry == "ragged" else dec(content, cls, y=y)
    loss = (out * surrogate).sum() / 50.0 if surrogate is not None else ast_amd.ragged_reconstruction_loss(out, y, nd)[0]
    loss.backward()
    torch.cuda.synchronize()
    return out.detach(), loss.detach(), {k: p.grad.detach().clone() for k, p in dec.named_parameters() if p.grad is not None}


def _grad_check(grads, ref, whole, worst, what=""):
    """whole-model relative L2 and the worst single parameter (those whose reference norm is >= 1e-3, as tests/test_gpu_models.py);
    every such parameter must HAVE a gradient -- one that lost it in the new pass is a failure, not a skip.  Below that norm are
    the convolution biases in front of a BatchNorm: identically 0 on the device (no gradient is formed), rounding noise in float64."""
    rows, num, den = [], 0.0, 0.0
    missing = [k for k, r in ref.items() if float(r.norm()) >= 1e-3 and k not in grads]
    assert not missing, missing
    for k, r in ref.items():
        gk = grads.get(k)
        if gk is None:
            continue
        num += float((gk.double().cpu() - r.double().cpu()).pow(2).sum())
        den += float(r.double().pow(2).sum())
        if float(r.norm()) >= 1e-3:
            rows.append((rel_l2(gk, r), k))
    rows.sort(reverse=True)
    print(what, "whole-model gradient", math.sqrt(num / den), "worst", rows[:3])
    assert math.sqrt(num / den) < whole, math.sqrt(num / den)
    assert rows[0][0] < worst, rows[:4]


def test_decoder_on_a_padded_batch_against_the_compaction_reference():
    config.set_compute_dtype(torch.float32)
    B, S, n = 2, 3, (3, 1)
    content, cls, y = (t.to(DEV) for t in R.decoder_inputs(B, S))
    ref_out, ref_loss, ref_grads = _reference(B, S, n)
    dec = _decoder()
    out, loss, grads = _step(dec, content, cls, y, n)
    live = torch.from_numpy(R.live_mask(B, S, n)).view(B, S)
    print("output", rel_err(out.cpu()[live], ref_out[live]), "loss", float(loss), ref_loss)
    assert rel_err(out.cpu()[live], ref_out[live]) < 1e-3
    assert int((out.cpu()[~live].view(torch.int32) != 0).sum()) == 0
    assert math.isclose(float(loss), ref_loss, rel_tol=1e-3)
    _grad_check(grads, ref_grads, 1e-2, 3e-2, "against float64:")
    # NaN in the padded sections of y: loss and every gradient finite, and UNCHANGED from the clean run.  The two runs differ by the
    # arrival order of their f32 atomics (statistics, weight gradients), which is a part of the rounding error the bounds above allow
    # against float64; a tenth of each bound tells "the same run again" from "another result within tolerance" -- one padded section
    # leaking into the statistics of four live ones moves the output by percents, a NaN by everything.
    yn = y.clone()
    yn[1, 1:] = float("nan")
    out2, loss2, grads2 = _step(_decoder(), content, cls, yn, n)
    assert bool(torch.isfinite(loss2)) and all(bool(torch.isfinite(v).all()) for v in grads2.values())
    assert int((out2.cpu()[~live].view(torch.int32) != 0).sum()) == 0
    print("poisoned against clean: output", rel_err(out2, out), "loss", float(loss2), float(loss))
    assert rel_err(out2, out) < 1e-4 and math.isclose(float(loss2), float(loss), rel_tol=1e-4)
    assert set(grads2) == set(grads)
    _grad_check(grads2, grads, 1e-3, 3e-3, "poisoned against clean:")


def test_decoder_bf16_against_the_compaction_reference():
    """bf16 storage: the output in relative L2 and the whole-model gradient of the smooth surrogate loss, both with the bounds of
    tests/test_gpu_models.py::test_full_step_bf16_vs_oracle (3e-2, 0.15) -- the reconstruction loss's wrapped-phase term turns bf16
    forward rounding into gradient changes that say nothing about the backward kernels, as that test's docstring explains.
    Measured on an MI355X: output 9.4e-3, gradient 0.141."""
    config.set_compute_dtype(torch.bfloat16)
    B, S, n = 2, 3, (3, 1)
    content, cls, y = (t.to(DEV) for t in R.decoder_inputs(B, S))
    ref_out, _, ref_grads = _reference(B, S, n, True)
    out, loss, grads = _step(_decoder(), content, cls, y, n, surrogate=_surrogate_weights(B, S, n).to(DEV))
    live = torch.from_numpy(R.live_mask(B, S, n)).view(B, S)
    print("bf16 output rel l2", rel_l2(out.cpu()[live], ref_out[live]))
    assert rel_l2(out.cpu()[live], ref_out[live]) < 3e-2
    assert int((out.cpu()[~live].view(torch.int32) != 0).sum()) == 0
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v).all()) for v in grads.values())
    _grad_check(grads, ref_grads, 0.15, float("inf"), "bf16 surrogate against float64:")
    # and the reconstruction loss itself stays finite with NaN in the padded sections
    yn = y.clone()
    yn[1, 1:] = float("nan")
    _, loss2, grads2 = _step(_decoder(), content, cls, yn, n)
    assert bool(torch.isfinite(loss2)) and all(bool(torch.isfinite(v).all()) for v in grads2.values())


def test_full_lengths_give_the_unmasked_training_pass():
    config.set_compute_dtype(torch.float32)
    B, S = 2, 2
    content, cls, y = (t.to(DEV) for t in R.decoder_inputs(B, S))
    out_u, loss_u, grads_u = _step(_decoder(), content, cls, y, (S,) * B, entry="forward")
    out_m, loss_m, grads_m = _step(_decoder(), content, cls, y, (S,) * B)
    assert rel_err(out_m, out_u) < 1e-3 and math.isclose(float(loss_m), float(loss_u), rel_tol=1e-3)
    _grad_check(grads_m, grads_u, 1e-2, 3e-2)


def test_one_captured_graph_serves_every_mix_of_lengths():
    config.set_compute_dtype(torch.float32)
    B, S = 2, 3
    content, cls, y = (t.to(DEV) for t in R.decoder_inputs(B, S))
    dec = _decoder()
    lengths = _dev_n((3, 1))
    _step(dec, content, cls, y, lengths)                                  # warm-up: weight bank, scratch, gradient buffers

    def step():
        for p in dec.parameters():
            if p.grad is not None:
                p.grad.zero_()
        ops.stat_arena_reset(DEV)
        out = dec.forward_training_ragged_bn(content, cls, y, lengths)
        loss, _ = ast_amd.ragged_reconstruction_loss(out, y, lengths)
        loss.backward()
        return out.detach(), loss.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    seen = []
    for mix in ((3, 1), (1, 2)):
        lengths.copy_(_dev_n(mix))
        state = {k: v.clone() for k, v in dec.state_dict().items()}       # a step moves the spectral-norm vectors: the eager twin starts here
        graph.replay()
        torch.cuda.synchronize()
        r_out, r_loss = captured[0].clone(), captured[1].clone()
        r_grads = {k: p.grad.clone() for k, p in dec.named_parameters() if p.grad is not None}
        twin = _decoder()
        twin.load_state_dict(state)
        e_out, e_loss, e_grads = _step(twin, content, cls, y, mix)
        assert rel_err(r_out, e_out) < 1e-3 and math.isclose(float(r_loss), float(e_loss), rel_tol=1e-3), mix
        live = torch.from_numpy(R.live_mask(B, S, mix)).view(B, S)
        assert int((r_out.cpu()[~live].view(torch.int32) != 0).sum()) == 0
        _grad_check(r_grads, e_grads, 1e-2, 3e-2)
        seen.append(float(r_loss))
    assert seen[0] != seen[1]                                             # the replay read the new lengths


def test_decoder_refuses_sync_bn_deterministic_and_eval_mode():
    config.set_compute_dtype(torch.float32)
    B, S, n = 2, 2, (2, 1)
    content, cls, y = (t.to(DEV) for t in R.decoder_inputs(B, S))
    dec = _decoder()
    ops.set_sync_bn(1, None, force=True)
    try:
        with pytest.raises(ValueError, match="sync-BN"):
            dec.forward_training_ragged_bn(content, cls, y, _dev_n(n))
    finally:
        ops.set_sync_bn(1)
    with ast_amd.deterministic():
        with pytest.raises(ValueError, match="deterministic mode"):
            dec.forward_training_ragged_bn(content, cls, y, _dev_n(n))
    with pytest.raises(ValueError, match="train"):
        dec.eval().forward_training_ragged_bn(content, cls, y, _dev_n(n))
    bn = torch.nn.BatchNorm2d(8).to(DEV).eval()
    with pytest.raises(ValueError, match="eval mode"):
        AL.bn_act_len(torch.zeros(4, 4, 4, 8, device=DEV), bn, (_dev_n(n), S))
