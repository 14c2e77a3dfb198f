"""Host side of the weight-bank tests (no GPU): the float64 reference of tests/weight_bank_ref.py against torch's own
spectral_norm in float64, branch coverage of csrc/weights.hip by the case table of tests/weight_bank_cases.py (through the restated
predicates), the conditions the seeded inputs must meet for the GPU comparison to mean something, the tolerance table, and the
tap limit of WeightBank.add."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import weight_bank_cases as WC
import weight_bank_ref as R


# ---- the reference against torch.nn.utils.spectral_norm, float64 ----------------------------------------------------------

def _torch_sn(kind, Co, Ci, k, W, u, v, G, training):
    """(weight, u, v, weight_orig.grad) of a spectral-normalised torch module in float64, in the logical (Co, Ci, KK) layout.
    The loss is sum(G * weight): its gradient with respect to the normalised weight is G."""
    if kind == "conv":
        m, dim = nn.Conv2d(Ci, Co, k, bias=False), 0
        to_master = lambda a: a.reshape(Co, Ci, k, k)
        to_logical = lambda t: t.reshape(Co, Ci, k * k)
        x = torch.zeros(1, Ci, k, k, dtype=torch.float64)
    elif kind == "convT":
        m, dim = nn.ConvTranspose2d(Ci, Co, k, bias=False), 1
        to_master = lambda a: a.reshape(Co, Ci, k, k).transpose(1, 0, 2, 3)
        to_logical = lambda t: t.permute(1, 0, 2, 3).reshape(Co, Ci, k * k)
        x = torch.zeros(1, Ci, 1, 1, dtype=torch.float64)
    else:
        m, dim = nn.Linear(Ci, Co, bias=False), 0
        to_master = lambda a: a.reshape(Co, Ci)
        to_logical = lambda t: t.reshape(Co, Ci, 1)
        x = torch.zeros(1, Ci, dtype=torch.float64)
    m = nn.utils.spectral_norm(m.double(), n_power_iterations=1, eps=1e-12, dim=dim)
    with torch.no_grad():
        m.weight_orig.copy_(torch.from_numpy(np.ascontiguousarray(to_master(W))))
        m.weight_u.copy_(torch.from_numpy(u))
        m.weight_v.copy_(torch.from_numpy(v))
    m.train(training)
    m(x)                                                   # the forward pre-hook: power iteration (training) and weight = W / sigma
    (m.weight * torch.from_numpy(np.ascontiguousarray(to_master(G)))).sum().backward()
    return (to_logical(m.weight.detach()).numpy(), m.weight_u.detach().numpy(), m.weight_v.detach().numpy(),
            to_logical(m.weight_orig.grad).numpy())


@pytest.mark.parametrize("kind,Co,Ci,k", [("conv", 5, 3, 3), ("conv", 7, 6, 2), ("convT", 4, 6, 3), ("convT", 3, 2, 1), ("linear", 9, 11, 1)])
@pytest.mark.parametrize("training", [True, False])
def test_reference_matches_torch_spectral_norm_float64(kind, Co, Ci, k, training):
    rng = np.random.default_rng(Co * 100 + Ci * 10 + k)
    KK = k * k
    W, G, grad0 = (rng.standard_normal((Co, Ci, KK)) for _ in range(3))
    u, v = rng.standard_normal(Co), rng.standard_normal(Ci * KK)
    u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
    parts = rng.standard_normal((3, Co, Ci, KK))
    parts[-1] = G - parts[:-1].sum(axis=0)
    tw, tu, tv, tg = _torch_sn(kind, Co, Ci, k, W, u, v, G, training)

    ru, rv, sigma = R.spectral(W, u, v, 1 if training else 0)
    Cop, Cip = R.pad8(Co), R.pad8(Ci)
    wf, wb = R.pack(W, sigma, Cop, Cip)
    # the replicas go through the staging layout of the kind and back, padding filled with NaN: it must be ignored
    from_wb = 1 if kind == "convT" else 0
    st = R.stage(parts.astype(np.float32), from_wb, Cop, Cip, pad_value=np.nan)
    np.testing.assert_array_equal(R.unstage(st, from_wb, 3, Co, Ci, KK, Cop, Cip), parts.astype(np.float32))
    grad, inner = R.flush(grad0, W, parts, ru, rv, sigma)

    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    assert rel(ru, tu) <= 1e-12 and rel(rv, tv) <= 1e-12
    if not training:
        np.testing.assert_array_equal(ru, u)
        np.testing.assert_array_equal(rv, v)
    assert rel(wf[:Co, :, :Ci].transpose(0, 2, 1), tw) <= 1e-12
    assert rel(wb[:Ci, :, :Co].transpose(2, 0, 1), tw) <= 1e-12
    assert rel(grad - grad0, tg) <= 1e-12
    # zeros in the padding of both images, and nowhere else by accident
    assert np.count_nonzero(wf) == Co * Ci * KK == np.count_nonzero(wb)
    assert abs(float(inner) - float((parts.sum(axis=0) * W).sum() / sigma)) <= 1e-12 * abs(float(inner))


def test_reference_without_u_is_the_identity_pack():
    rng = np.random.default_rng(5)
    W = rng.standard_normal((9, 11, 1)).astype(np.float32)
    for dt in (np.float64, np.float32):
        u, v, sigma = R.spectral(W, None, None, 1, dt)
        assert u is None and v is None and sigma == 1.0
        wf, wb = R.pack(W, sigma, 16, 16, dt)
        np.testing.assert_array_equal(wf[:9, 0, :11], W[:, :, 0])
        np.testing.assert_array_equal(wb[:11, 0, :9], W[:, :, 0].T)


def test_strided_master_views_round_trip():
    for c in WC.CASES:
        d = WC.inputs(c.id)
        W = R.logical(d["w"], c.Co, c.Ci, c.KK, c.s_co, c.s_ci, c.w_offset)
        np.testing.assert_array_equal(W, d["W"])
        if c.kind == "convT":                                # the master really is [ci][co][tap]
            np.testing.assert_array_equal(d["w"][c.w_offset:].reshape(c.Ci, c.Co, c.KK).transpose(1, 0, 2), d["W"])
        else:
            np.testing.assert_array_equal(d["w"][c.w_offset:].reshape(c.Co, c.Ci, c.KK), d["W"])


def test_sequential_float32_chain_is_float32_and_close():
    """The yardstick stays in float32 end to end (a silent promotion to float64 would make every e_seq 6e-8) and is the same
    computation as the reference (it agrees with it to float32 accuracy)."""
    for c in WC.CASES:
        ref, seq = WC.reference(c.id)
        for q, a in seq.items():
            if a is not None:
                assert np.asarray(a).dtype == np.float32, (c.id, q)
                assert np.asarray(ref[q]).dtype == np.float64, (c.id, q)
        for q, (e, b) in WC.tolerances(c.id).items():
            assert e <= 1e-4, (c.id, q, e)
            assert 16 * R.U24 <= b <= R.F32_CEILING


# ---- coverage of the kernels' branches by the case table -----------------------------------------------------------------

# what each case is in the table for (Case.note), as branch names
PROMISED = {
    "A": {"tile_full", "master_vector", "packed_vector", "sn_wt_u_vector", "sn_w_v_vector_train", "sn_w_v_vector_eval", "dwp_vector_eight",
          "kkc9", "co_outer", "dwp_from_wb0", "chunks_all"},
    "B": {"tile_partial", "master_scalar", "packed_scalar", "sn_wt_u_scalar", "sn_w_v_scalar_train", "sn_w_v_scalar_eval", "dwp_scalar_eight",
          "chunks_some_empty", "rows_per_many", "padding_ci"},
    "C": {"kkc1", "sn_w_v_last_block_partial", "chunks_some_empty", "dwp_vector_other", "dwp_scalar_other", "padding_co", "tile_full", "tile_partial"},
    "D": {"ci_outer", "dwp_from_wb1", "tile_full", "master_vector", "dwp_vector_other", "sn_wt_u_scalar"},
    "E": {"ci_outer", "dwp_from_wb1", "tile_partial", "master_scalar", "dwp_scalar_one", "padding_co"},
    "F": {"kkc0", "master_scalar", "packed_scalar", "dwp_scalar_one", "sn_wt_u_vector"},
    "G": {"no_u", "replicas_none", "kkc1", "tile_full", "master_vector", "packed_vector"},
    "H": {"tile_full", "master_scalar_on_full_tile", "packed_vector", "dwp_vector_eight", "sn_wt_u_scalar", "sn_w_v_scalar_train"},
    "I": {"sn_column_blocks_many", "rows_per_1", "chunks_some_empty", "sn_wt_u_vector", "tile_partial"},
    "J": {"sn_sigma_strided", "kkc1", "dwp_scalar_one", "tile_partial"},
    "K": {"tile_full", "kkc1", "dwp_vector_one", "master_vector"},
}


def test_every_promised_branch_is_taken():
    for c in WC.CASES:
        missing = PROMISED[c.id] - WC.branches(c)
        assert not missing, f"case {c.id} ({c.note}) does not take {sorted(missing)}"
    # the facts the table states in numbers
    assert WC.sn_chunks(WC.BY_ID["B"]) == (2, 20) and WC.sn_chunks(WC.BY_ID["C"]) == (2, 17)
    assert WC.sn_chunks(WC.BY_ID["I"]) == (1, 8) and WC.sn_chunks(WC.BY_ID["A"]) == (2, 32)
    assert WC.BY_ID["B"].ncols == 18 and WC.BY_ID["I"].ncols == 4608 and (WC.BY_ID["J"].Co + 3) // 4 == 66
    assert WC.MAX_CO == 264 and WC.MAX_COLS == 4608
    assert max(c.numel for c in WC.CASES) == 8 * 512 * 9 <= 37_000
    assert all(c.KK <= WC.MAX_KK for c in WC.CASES)


def test_every_branch_of_the_kernels_has_a_case_on_each_side():
    taken = set().union(*(WC.branches(c) for c in WC.CASES))
    both_sides = [("sn_wt_u_vector", "sn_wt_u_scalar"), ("sn_w_v_vector_train", "sn_w_v_scalar_train"), ("sn_w_v_vector_eval", "sn_w_v_scalar_eval"),
                  ("tile_full", "tile_partial"), ("master_vector", "master_scalar"), ("master_vector", "master_scalar_on_full_tile"),
                  ("packed_vector", "packed_scalar"), ("co_outer", "ci_outer"), ("dwp_from_wb0", "dwp_from_wb1"), ("has_u", "no_u"),
                  ("chunks_all", "chunks_some_empty"), ("rows_per_1", "rows_per_many"), ("padding_co", "padding_ci")]
    for pair in both_sides:
        for name in pair:
            assert name in taken, f"no case takes {name}"
    for name in ("kkc9", "kkc1", "kkc0", "sn_column_blocks_many", "sn_w_v_last_block_partial", "sn_sigma_strided"):
        assert name in taken, f"no case takes {name}"
    # replica counts 1, 8 (unrolled) and "other", each on the vector and on the scalar staging loader
    for path in ("vector", "scalar"):
        for rep in ("one", "eight", "other"):
            assert f"dwp_{path}_{rep}" in taken, f"no case sums {rep} replica(s) on the {path} staging path"
    # both layouts on both loaders, and the run-time-KK body with and without spectral norm's vector loops
    for name, pred in (("convT on the vector staging path", lambda c, t: c.from_wb and WC.packed_vector(c, *t)),
                       ("convT on the scalar staging path", lambda c, t: c.from_wb and not WC.packed_vector(c, *t)),
                       ("convT master along co, vector", lambda c, t: not WC.co_outer(c) and WC.master_vector(c, *t)),
                       ("convT master along co, scalar", lambda c, t: not WC.co_outer(c) and not WC.master_vector(c, *t))):
        assert any(pred(c, t) for c in WC.CASES for t in c.tiles()), name
    # the misaligned case is the ONLY reason H leaves the vector path: aligned, it would take it everywhere
    H = WC.BY_ID["H"]
    aligned = WC.Case("H0", H.kind, H.Co, H.Ci, H.k, H.replicas)
    assert WC.sn_wt_u_vector(aligned) and all(WC.master_vector(aligned, *t) for t in aligned.tiles())
    assert not WC.sn_wt_u_vector(H) and not any(WC.master_vector(H, *t) for t in H.tiles())


def test_tile_list_layout():
    tl = WC.tile_list().reshape(-1, 4)
    assert tl.dtype == np.int32 and (tl[:, 3] == 0).all()
    assert (np.diff(tl[:, 0]) >= 0).all()                    # tiles of a weight are consecutive (inner_sum_det_kernel relies on it)
    for wi, c in enumerate(WC.CASES):
        mine = tl[tl[:, 0] == wi]
        assert len(mine) == -(-c.Cop // 32) * -(-c.Cip // 32)
        cover = np.zeros((c.Cop, c.Cip), int)
        for _, co0, ci0, _ in mine:
            cover[co0:co0 + 32, ci0:ci0 + 32] += 1
        assert (cover == 1).all()                            # the padded extents, each channel pair exactly once


# ---- the inputs make the comparison mean something ------------------------------------------------------------------------

def test_input_conditions():
    for c in WC.CASES:
        d, ref = WC.inputs(c.id), WC.reference(c.id)[0]
        if not c.has_u:
            assert ref["sigma"] == 1.0
            continue
        dW = d["parts"].astype(np.float64).sum(axis=0)
        rank_one = float(ref["inner"]) * np.outer(ref["u"], ref["v"])
        ratio = float(np.max(np.abs(rank_one)) / np.max(np.abs(dW)))
        print(f"case {c.id}: sigma {float(ref['sigma']):6.2f}  sigma_eval {float(ref['sigma_eval']):8.4f}  max|inner u v^T| / max|dW| = {ratio:.2f}")
        assert ratio >= 0.1, (c.id, ratio)                   # the rank-one correction is no 1 % effect
        assert float(ref["sigma"]) > 1.0, (c.id, float(ref["sigma"]))
        assert abs(np.linalg.norm(d["u"]) - 1) < 1e-6 and abs(np.linalg.norm(d["v"]) - 1) < 1e-6
        # the replicas are really different from one another (a kernel that reads one of them eight times must fail)
        if c.replicas > 1:
            assert np.max(np.abs(d["parts"][0] - d["parts"][1])) > 1.0
        assert np.isfinite(ref["grad"]).all()


def test_tolerance_table():
    table = WC.tolerance_table()
    print("\ne_seq -> f32 bound, as fractions of the float64 tensor's max-abs (bf16 packed values: + 2^-8 |ref|)\n" + table)
    for c in WC.CASES:
        t = WC.tolerances(c.id)
        want = {"wf", "wf_eval", "sigma", "sigma_eval"} | ({"u", "v", "grad"} if c.has_u else set()) | \
               ({"unpack", "unpack_plain"} if c.id in WC.UNPACK_CASES else set())
        assert want <= set(t), (c.id, sorted(want - set(t)))
        for q, (e, b) in t.items():
            assert b == min(2e-4, max(4 * e, 16 * 2.0 ** -24))


# ---- the tap limit of the LDS tile ------------------------------------------------------------------------------------------

def test_weight_bank_refuses_more_than_nine_taps():
    from ast_amd.layers import WeightBank
    bank = WeightBank()
    f32 = lambda: torch.float32
    for kind, shape in (("conv", (4, 3, 5, 5)), ("convT", (3, 4, 5, 5)), ("conv", (4, 3, 2, 5)), ("convT", (4, 3, 4, 4))):
        with pytest.raises(ValueError, match="taps"):
            bank.add(torch.zeros(shape), kind, f32)
    assert bank.specs == [] and bank.entries == []
    for kind, shape in (("conv", (4, 3, 3, 3)), ("convT", (3, 4, 3, 3)), ("conv", (4, 3, 1, 1)), ("conv", (4, 3, 2, 2)), ("linear", (40, 30))):
        bank.add(torch.zeros(shape), kind, f32)
    assert len(bank.specs) == 5
