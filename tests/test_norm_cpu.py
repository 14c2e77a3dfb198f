"""Host side of the normalisation kernel tests (no GPU): the float64 references of tests/norm_ref.py against float64 torch autograd
through nn.BatchNorm2d, nn.InstanceNorm2d and nn.LayerNorm; the conditions the seeded inputs of every GPU case must meet (the ReLU
margin with nothing excluded, values representable in the case's dtype, the constant channel); the plain float32 evaluation that sets
the bounds; and the launch arithmetic of csrc/norm.hip that says which path each named case enters."""
import pytest
import torch
import torch.nn as nn

import norm_ref as R

F64 = torch.float64
SMALL = [n for n in R.BN_CASES if n != "stride2"] + list(R.BN_CASES_EXTRA)


def _modules(i):
    Cr = i["Creal"]
    bn, inn = nn.BatchNorm2d(Cr, eps=R.EPS, momentum=R.MOMENTUM).double(), nn.InstanceNorm2d(Cr, eps=R.EPS, affine=True).double()
    with torch.no_grad():
        bn.weight.copy_(i["g1"]); bn.bias.copy_(i["b1"]); bn.running_mean.copy_(i["rm"]); bn.running_var.copy_(i["rv"])
        inn.weight.copy_(i["g2"]); inn.bias.copy_(i["b2"])
    return bn, inn


def _nchw(t, Cr):
    return t[..., :Cr].permute(0, 2, 1).unsqueeze(-1).contiguous()                         # (N, Creal, HW, 1)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("name", SMALL)
def test_bn_reference_matches_float64_autograd(name, relu):
    for with_r in R.variants(name):
        _reference_matches_autograd(name, relu, with_r)


def _reference_matches_autograd(name, relu, with_r):
    i = R.bn_inputs(name, torch.float32, relu, with_r)
    ref, _, _ = R.bn_reference(name, torch.float32, relu, with_r)
    Cr = i["Creal"]
    bn, inn = _modules(i)
    x = _nchw(i["x"], Cr).requires_grad_(True)
    out = bn(x)
    r = None
    if i["r"] is not None:
        r = _nchw(i["r"], Cr).requires_grad_(True)
        out = out + inn(r)
    y = torch.relu(out) if relu else out
    y.backward(_nchw(i["dy"], Cr))
    tol = 1e-12
    assert R.rel(ref["y"][..., :Cr], y.squeeze(-1).permute(0, 2, 1)) < tol
    assert R.rel(ref["dx"][..., :Cr], x.grad.squeeze(-1).permute(0, 2, 1)) < tol * max(1.0, ref["kappa1"])
    assert R.rel(ref["dgamma1"], bn.weight.grad) < tol * max(1.0, ref["kappa1"]) and R.rel(ref["dbeta1"], bn.bias.grad) < tol
    # the running statistics after one training step, and the counter
    assert R.rel(ref["running_mean"], bn.running_mean) < tol and R.rel(ref["running_var"], bn.running_var) < tol
    assert int(bn.num_batches_tracked) == 1
    if r is not None:
        assert R.rel(ref["dr"][..., :Cr], r.grad.squeeze(-1).permute(0, 2, 1)) < tol * max(1.0, ref["kappa2"])
        assert R.rel(ref["dgamma2"], inn.weight.grad) < tol * max(1.0, ref["kappa2"]) and R.rel(ref["dbeta2"], inn.bias.grad) < tol
    # padded channels: scale = shift = 0, so y, dx, dr and the k coefficients are exact zeros whatever the channel holds
    for k in ("scale1", "shift1", "y", "dx", "k1") + (("scale2", "shift2", "dr", "k2") if r is not None else ()):
        t = ref[k]
        pad = t[..., Cr:, :] if k in ("k1", "k2") else t[..., Cr:]
        assert pad.numel() == 0 or R.is_zero(pad), (name, k)
    # dx = k0 dz + k1 x + k2 is the same gradient written the way the apply kernels evaluate it
    xh = (i["x"] - ref["mean1"]) * ref["rstd1"]
    G1 = R.pad_params(i["g1"], i["C"])
    P = i["N"] * i["HW"]
    direct = G1 * ref["rstd1"] * (ref["relu_bwd"] - ref["relu_bwd"].sum((0, 1)) / P - xh * (ref["relu_bwd"] * xh).sum((0, 1)) / P)
    assert R.rel(ref["dx"], direct) < 1e-9 * max(1.0, ref["kappa1"])


def test_sums_finalize_and_slot_split_are_consistent():
    """The finalize from the float64 sums is the finalize from the data; a slot table's rows add up to the per-image sums."""
    i = R.bn_inputs("c24-r8", torch.float32)
    ref, _, _ = R.bn_reference("c24-r8", torch.float32)
    cnt = i["N"] * i["HW"]
    s = ref["sums1"].sum(0)
    m = s[:, 0] / cnt
    v = s[:, 1] / cnt - m * m
    assert R.rel(m, ref["mean1"]) < 1e-14 and R.rel(v, ref["var1"]) < 1e-11
    for rows in (1, 8, 16, 64):
        parts = R.slot_split(i["x"], rows)
        assert len(parts) == rows and sum(p.shape[0] for p in parts) == cnt
        tot = sum(p.sum(0) for p in parts)
        assert R.rel(tot, s[:, 0]) < 1e-13
    # the unbiased variance guards a single pixel: cnt - 1 -> max(cnt - 1, 1)
    rm, rv = R.running_update(torch.zeros(1, dtype=F64), torch.ones(1, dtype=F64), torch.tensor([2.0], dtype=F64), torch.tensor([0.0], dtype=F64), 1, 1)
    assert float(rm) == 0.2 and float(rv) == 0.9


def _adiff(a, b):
    """max |a - b| / max(1, max |b|): for gradients that the formula may give as an exact 0 (D = 1) where torch leaves 1e-16"""
    return float((a.detach() - b.detach()).abs().max()) / max(1.0, float(b.detach().abs().max()))


def test_layernorm_references_match_float64_autograd():
    for rows in R.LN_ROWS:
        for D in R.LN_D:
            i = R.ln_inputs(rows, D)
            ln = nn.LayerNorm(D, eps=R.EPS).double()
            with torch.no_grad():
                ln.weight.copy_(i["gamma"]); ln.bias.copy_(i["beta"])
            x = i["x"].clone().requires_grad_(True)
            y = ln(x)
            y.backward(i["dy"])
            yr, m, rs = R.layernorm(i["x"], i["gamma"], i["beta"])
            dx, dg, db = R.layernorm_bwd(i["dy"], i["x"], i["gamma"], m, rs)
            # D = 1: dx is exactly 0 in the formula (torch leaves 1e-16 of rounding), so the gradients are compared at the scale of dy
            assert R.rel(yr, y) < 1e-12 and _adiff(dx, x.grad) < 1e-12 and _adiff(dg, ln.weight.grad) < 1e-12 and R.rel(db, ln.bias.grad) < 1e-12
            # s = x + mask * sub; y = LN(s), with upstream gradients on both y and s
            mask = (torch.rand(rows, D, generator=torch.Generator().manual_seed(rows * D)) > 0.3).double() / 0.7
            xs, sub = i["x"].clone().requires_grad_(True), i["sub"].clone().requires_grad_(True)
            ln.zero_grad()
            s = xs + mask * sub
            y = ln(s)
            ((y * i["dy"]).sum() + (s * i["ds_ext"]).sum()).backward()
            sr, yr, m, rs = R.add_drop_ln(i["x"], i["sub"], mask, i["gamma"], i["beta"])
            dxr, dsub, dg, db = R.add_drop_ln_bwd(i["dy"], i["ds_ext"], sr, i["gamma"], m, rs, mask)
            assert R.rel(sr, s) < 1e-13 and R.rel(yr, y) < 1e-12
            assert _adiff(dxr, xs.grad) < 1e-12 and _adiff(dsub, sub.grad) < 1e-12 and _adiff(dg, ln.weight.grad) < 1e-12
    # absent operands
    i = R.ln_inputs(4, 64)
    s, y, m, rs = R.add_drop_ln(None, i["sub"], None, None, None)
    assert torch.equal(s, i["sub"]) and y is None
    dx, dsub, dg, db = R.add_drop_ln_bwd(None, i["ds_ext"], s, None, None, None, None)
    assert torch.equal(dx, i["ds_ext"]) and torch.equal(dsub, i["ds_ext"]) and dg is None


def test_gpu_variants_cover_what_the_gpu_file_runs():
    """every (case, dtype, with-InstanceNorm-input) the GPU file runs with ReLU on is in the list the next test walks"""
    v = set(R.gpu_variants())
    for n, d in R.BN_PARAMS:
        assert {(n, d, w) for w in R.variants(n)} <= v and (n, d, bool(R.case(n)[5])) in v      # _case(name, dtype): the case's own form
    for n in R.DET_CASES:
        assert all((n, d, bool(R.case(n)[5])) in v for d in R.BOTH)
    assert all((n, torch.float32, False) in v for _, n in R.SLOT_CASES) and (R.SLOT_REJECTED[1], torch.float32, False) in v
    assert all((n, d, w) in v for n in R.AUTOGRAD_CASES for d in R.BOTH for w in (False, True))
    assert all(w is False or R.case(n)[5] for n, d, w in v)
    # the two variants of one case are conditioned separately: different x, each with its own margin
    a, b = R.bn_inputs("c24", torch.float32, True, False), R.bn_inputs("c24", torch.float32, True, True)
    assert not torch.equal(a["x"], b["x"]) and torch.equal(a["dy"], b["dy"]) and a["r"] is None and b["r"] is not None


@pytest.mark.parametrize("name,dtype,with_r", R.gpu_variants(),
                         ids=[f"{n}-{'f32' if d == torch.float32 else 'bf16'}-{'bn+in' if w else 'bn'}" for n, d, w in R.gpu_variants()])
def test_bn_inputs_meet_their_conditions(name, dtype, with_r):
    N, HW, C, Creal, ratio, _, const, _ = R.case(name)
    i = R.bn_inputs(name, dtype, True, with_r)
    ref, plain, kappa = R.bn_reference(name, dtype, True, with_r)
    assert tuple(i["x"].shape) == (N, HW, C) and (i["r"] is not None) == with_r
    # the inputs were moved, not reseeded: how many elements, in how many passes
    frac = i["moved"] / (N * HW * Creal)
    print(f"{name} {dtype} with_r={with_r}: {i['moved']} of {N * HW * Creal} elements moved ({frac:.2%}) in {i['rounds']} passes")
    assert frac <= 0.02 and i["rounds"] <= 5
    for k in ("x", "dy") + (("r",) if with_r else ()):
        assert torch.equal(i[k], R.rounded(i[k], dtype)), f"{k} is not representable in {dtype}"
        assert i[k].numel() * (2 if dtype == torch.bfloat16 else 4) <= 20 * 2 ** 20
    # the ReLU margin: no pre-activation of a real channel within MARGIN of its scale of zero, nothing excluded
    margin = R.relu_margin(ref["pre"], Creal)
    print(f"{name} {dtype} with_r={with_r}: min |pre| / max |pre| = {margin:.2e}, kappa = {kappa:.1f}")
    assert margin >= R.MARGIN
    assert bool((plain["pre"][..., :Creal] > 0).eq(ref["pre"][..., :Creal] > 0).all())       # so float32 takes the same mask
    if Creal < C:
        assert R.is_zero(ref["pre"][..., Creal:]) and float(i["x"][..., Creal:].abs().max()) > 0
    if const is not None:
        assert bool((i["x"][..., const] == 0.5).all()) and float(ref["var1"][const]) == 0.0
        assert float(ref["rstd1"][const]) == R.EPS ** -0.5
        assert abs(float(ref["pre"][0, 0, const]) - float(i["b1"][const])) < 1e-12
    if ratio and N * HW >= 100:
        assert (0.8 * ratio) ** 2 < ref["kappa1"] - 1 < (1.25 * ratio) ** 2
    if ratio == 0 and N * HW >= 100:
        assert ref["kappa1"] < 1.2
    # the plain float32 evaluation is wired to the same quantities: it is within the kernels' own floor of the float64 reference
    for k, v in plain.items():
        e32, tol = R.bound(v, ref[k], R.kappa_for(k, ref))
        assert e32 <= R.FLOOR * max(1.0, R.kappa_for(k, ref) / 4) <= tol, (k, e32)
    if N * HW <= 8:                                         # a handful of pixels per channel: spread by construction, not by luck
        assert kappa < 8
    assert R.kappa_for("dbeta1", ref) == R.kappa_for("sums3", ref) == R.kappa_for("mean1", ref) == R.kappa_for("relu_bwd", ref) == 1.0
    assert R.kappa_for("dx", ref) == ref["kappa1"] and R.kappa_for("y", ref) == kappa and R.kappa_for("dr", ref) == ref.get("kappa2", 1.0)


def test_bound_is_the_loss_tail_rule_while_the_conditioning_is_small():
    """max(8 e32, 64 * 2^-24 * max(1, kappa / 4)): loss_tail_ref.bound while kappa / 4 <= 1, the floor scaled by kappa / 4 beyond"""
    import loss_tail_ref as LT
    ref = torch.tensor([1.0, -2.0, 4.0], dtype=F64)
    for err in (0.0, 1e-8, 1e-6, 3e-5):
        plain = ref + torch.tensor([0.0, 0.0, 4.0 * err], dtype=F64)
        for kappa in (1.0, 2.0, 4.0):
            assert R.bound(plain, ref, kappa) == LT.bound(plain, ref)
        assert R.bound(plain, ref, 5.0) == (LT.bound(plain, ref)[0], max(LT.bound(plain, ref)[1], 1.25 * LT.FLOOR))
    assert R.bound(ref, ref, 1025.0)[1] == R.FLOOR * 1025 / 4
    assert R.bound(ref, ref, 1.0, bf16_store=True)[1] == R.FLOOR + 2.0 ** -8


def test_launch_arithmetic_puts_every_case_on_its_path(monkeypatch):
    monkeypatch.delenv("AST_REDUCE_BLOCKS", raising=False)
    monkeypatch.delenv("AST_ELEM_BLOCKS", raising=False)
    assert R.reduce_blocks() == 512 and R.elem_blocks() == 2048
    assert set(R.PATH_CLAIMS) == set(R.PATH_TESTS)
    for path, names in R.PATH_CLAIMS.items():
        assert len(names) >= 1, f"no case enters {path}"
        for n in names:
            c = R.BN_CASES[n]                                 # a case removed from the table fails here
            assert R.PATH_TESTS[path](c, R.reduce_launch(c[0], c[1], c[2]), R.elem_launch(c[0], c[1], c[2])), (path, n)
    # the channel counts, pixel counts and image counts the table must hold
    assert {c[2] for c in R.BN_CASES.values()} >= {8, 24, 40, 64, 256, 512, 2048}
    assert {c[1] for c in R.BN_CASES.values()} >= {1, 3, 117} and {c[0] for c in R.BN_CASES.values()} >= {1, 3}
    assert any(c[0] > R.reduce_blocks() and c[2] == 8 for c in R.BN_CASES.values())
    # spelled out for the cases the docstring of the GPU test describes
    red = R.reduce_launch(3, 117, 24)
    assert (red["U"], red["PL"], red["idle_threads"], red["ppb"], red["grid"]) == (3, 85, 1, 59, (2, 3)) and red["ragged_last_block"]
    assert R.reduce_launch(3, 117, 8)["PL"] == 256 and R.reduce_launch(1, 3, 2048)["PL"] == 1 and R.reduce_launch(1, 3, 2048)["U"] == 256
    assert R.reduce_launch(600, 3, 8)["grid"] == (1, 600)
    el = R.elem_launch(256, 300, 64)
    assert el["grid"] == (8, 256) and el["trips"] == 2 and el["hoist"]
    assert all(R.elem_launch(c[0], c[1], c[2])["trips"] == 1 for n, c in R.BN_CASES.items() if n != "stride2")
    # deterministic forms: the grid is the slot count
    N, HW, C = R.case(R.DET_CASES[0])[:3]
    assert max(R.DET_SLOTS) > HW
    d = R.reduce_launch(N, HW, C, nslots=max(R.DET_SLOTS))
    assert d["empty_slots"] == max(R.DET_SLOTS) - HW and d["ppb"] == 1 and d["grid"] == (max(R.DET_SLOTS), N)
    assert R.reduce_launch(N, HW, C, nslots=1)["empty_slots"] == 0
    assert R.reduce_launch(*R.case("c24")[:3], nslots=3)["ppb"] == 39
    # the slot reduction inside ast_bn_apply_fwd / _bwd
    nparts = {(rows, R.BN_CASES[n][2]): R.apply_launch(rows, R.BN_CASES[n][2])["nparts"] for rows, n in R.SLOT_CASES}
    assert nparts == {(1, 64): 1, (8, 24): 8, (16, 24): 10, (64, 8): 32, (32, 2048): 1}
    assert {R.apply_launch(c[0], c[2])["nparts"] for c in R.BN_CASES.values()} >= {1, 3}      # rows = N: per-image tables
    assert {1, 8, 16, 64} <= {rows for rows, _ in R.SLOT_CASES}
    for rows, n in R.SLOT_CASES:
        for bwd in (False, True):
            a = R.apply_launch(rows, R.BN_CASES[n][2], bwd)
            assert a["accepted"] and a["lds"] <= 65536, (rows, n, bwd)
    Crej = R.BN_CASES[R.SLOT_REJECTED[1]][2]
    assert (32, "c2048") in R.SLOT_CASES and 32 * 2048 == 65536 and R.SLOT_REJECTED[0] * Crej == 65536 + Crej
    assert not R.apply_launch(R.SLOT_REJECTED[0], Crej)["accepted"]


def test_layernorm_case_tables():
    assert set(R.LN_D) == {1, 63, 64, 65, 256, 1000} and set(R.LN_ROWS) == {1, 4, 5, 67} and set(R.ADLN_ROWS) == {1, 5, 67}
    assert sorted(4 - r % 4 for r in R.ADLN_ROWS) == [1, 3, 3]                             # invalid waves of the last 4-row workgroup
    names = {c[0] for c in R.ADLN_COMBOS}
    assert names == {"full", "x-null", "gamma-null", "dy-only", "ds-only", "mask-null", "dx-null"}
    for name, x, gamma, p, dy, ds, dx in R.ADLN_COMBOS:
        assert dy or ds                                         # the entry refuses a backward with neither
        assert gamma or not dy                                  # no LayerNorm, no dy
        assert (p == 0.0) == (name == "mask-null")
    i = R.ln_inputs(5, 256)
    assert float(i["dgamma0"].abs().min()) > 0 and float(i["dbeta0"].abs().min()) > 0
