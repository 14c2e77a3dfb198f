"""CPU-only checks of tests/wgrad_cases.py: the float64 weight-gradient reference against autograd, every row's plan pinned
through ast_wgrad_plan (the library loads without a GPU), the exactness condition of every row's inputs, the table's coverage
of what wgrad_dispatch can name (derived from csrc/wgrad.hip), and that the exact comparison rejects broken results."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import igemm_cases as IC
import wgrad_cases as WC
from ast_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = {name: code for code, name in enumerate(WC.FAMILIES)}


def _P(g):
    return g.N * g.Hm * g.Wm


@pytest.mark.parametrize("N,H,W,Cs,Cd,k,stride,pad", [(2, 7, 9, 8, 16, 3, 1, 1), (2, 9, 12, 8, 8, 3, 2, 1), (2, 9, 13, 16, 8, 3, 2, 1),
                                                     (3, 5, 6, 16, 8, 1, 1, 0), (2, 9, 19, 8, 8, 1, 2, 0), (5, 1, 1, 24, 16, 1, 1, 0),
                                                     (1, 2, 2, 8, 8, 3, 1, 1)])
def test_wgrad_ref_matches_conv2d(N, H, W, Cs, Cd, k, stride, pad):
    """wgrad_ref on Conv2d geometries (the linear one, H = W = 1, among them) against autograd's weight gradient in float64, and
    its second output against the same gradient of absolute values."""
    gen = torch.Generator().manual_seed(3)
    g, (Ho, Wo) = ops.gather_direct(N, H, W, Cs, Cd, k, stride, pad)
    x = torch.randn(N, Cs, H, W, dtype=torch.float64, generator=gen)
    dy = torch.randn(N, Cd, Ho, Wo, dtype=torch.float64, generator=gen)
    outs = []
    for xx, dd in ((x, dy), (x.abs(), dy.abs())):
        w = torch.zeros(Cd, Cs, k, k, dtype=torch.float64, requires_grad=True)
        F.conv2d(xx, w, stride=stride, padding=pad).backward(dd)
        outs.append(w.grad.permute(0, 2, 3, 1).reshape(Cd, k * k, Cs))
    dW, A = WC.wgrad_ref(dy.permute(0, 2, 3, 1), x.permute(0, 2, 3, 1), g)
    assert float((dW - outs[0]).abs().max()) < 1e-11 and float((A - outs[1]).abs().max()) < 1e-11
    assert bool((A >= dW.abs() - 1e-11).all())


@pytest.mark.parametrize("Hs,Ws,Hd,Wd,k,stride,pad", [(5, 7, 10, 14, 3, 2, 1), (5, 7, 9, 13, 3, 2, 1), (4, 5, 8, 9, 1, 2, 0)])
def test_wgrad_ref_parity_classes_assemble_conv_transpose2d(Hs, Ws, Hd, Wd, k, stride, pad):
    """The parity classes of ops.gathers_transposed, as weight-gradient geometries (dy = the class's pixels of the output gradient),
    write disjoint tap slices that together are F.conv_transpose2d's weight gradient; a class leaves the other slices zero."""
    N, Cs, Cd = 2, 8, 16
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(N, Cs, Hs, Ws, dtype=torch.float64, generator=gen)
    dy = torch.randn(N, Cd, Hd, Wd, dtype=torch.float64, generator=gen)
    w = torch.zeros(Cs, Cd, k, k, dtype=torch.float64, requires_grad=True)
    oph, opw = Hd - ((Hs - 1) * stride - 2 * pad + k), Wd - ((Ws - 1) * stride - 2 * pad + k)
    F.conv_transpose2d(x, w, stride=stride, padding=pad, output_padding=(oph, opw)).backward(dy)
    ref = w.grad.permute(1, 2, 3, 0).reshape(Cd, k * k, Cs)
    total, seen = torch.zeros_like(ref), torch.zeros(k * k, dtype=torch.int32)
    for g in ops.gathers_transposed(N, Hs, Ws, Cs, Hd, Wd, Cd, k, stride, pad):
        dyc = dy.permute(0, 2, 3, 1)[:, g.doh::g.dsh, g.dow::g.dsw, :][:, :g.Hm, :g.Wm, :]
        dW, A = WC.wgrad_ref(dyc, x.permute(0, 2, 3, 1), g)
        m = WC.listed_taps(g)
        assert not bool(dW[:, ~m].any()) and not bool(A[:, ~m].any())
        total += dW
        seen += m.int()
    assert bool((seen == 1).all())
    assert float((total - ref).abs().max()) < 1e-11


def test_wgrad_case_table_plans_are_pinned():
    """Every row gets exactly the six integers of ast_wgrad_plan it records, under its own environment and under
    AST_WGRAD_FLUSH_LDS=1 where the row also runs that; every halo row is a halo plan with partial tiles on both axes, and the
    weight-gradient shapes of test_gpu_ops.py are not halo plans (that kernel was never launched by an op-level test)."""
    for c in WC.CASES:
        g = c.gather()
        with WC.case_env(c):
            plan = WC.plan_of(g, c.dtype)
            caps = [WC.plan_of(g, c.dtype, cap) for cap in WC.slab_caps(c.plan[4])]
        assert plan == c.plan, (c.name, plan)
        assert plan[0] == FAMILY[c.family], c.name
        assert c.plan[4] > 1, c.name                                          # so that one slab cap lies below the slice count
        lo, hi = WC.slab_caps(c.plan[4])
        assert caps[0][:4] == plan[:4] and caps[1][:4] == plan[:4], c.name   # the slab entry runs the same tile shape
        assert 1 <= caps[0][4] <= lo < plan[4] and caps[1][4] == plan[4], (c.name, caps)
        if c.flush_lds:
            with WC.case_env(c, AST_WGRAD_FLUSH_LDS=1):
                assert WC.plan_of(g, c.dtype) == c.plan, c.name
        if c.family == "halo":
            assert g.Hm % 8 and g.Wm % 16 and plan[5] >= 256 * plan[3] * (2 if plan[3] > 1 else 1), c.name
    with WC.case_env():
        for cin, cout, k, stride, H, W, N in [(32, 32, 3, 1, 40, 61, 4), (8, 32, 3, 2, 64, 97, 4), (64, 64, 3, 1, 30, 50, 4), (32, 64, 1, 2, 40, 60, 2),
                                              (64, 128, 3, 2, 36, 75, 3), (2, 16, 3, 1, 57, 83, 2), (128, 128, 3, 1, 9, 19, 3)]:
            g = ops.gather_direct(N, H, W, ops.pad8(cin), ops.pad8(cout), k, stride, 1 if k == 3 else 0)[0]
            for dt in ("f32", "bf16"):
                assert WC.plan_of(g, dt)[0] != FAMILY["halo"], (cin, cout, H, W, dt)


def test_wgrad_case_table_holds_what_it_is_there_for():
    """The edge conditions the rows exist for, read off the geometries and the pinned plans."""
    by = lambda fam, dt=None, pg=None: [c for c in WC.CASES if c.family == fam and dt in (None, c.dtype) and pg in (None, c.plan[3])]
    for dt in ("f32", "bf16"):
        for pg in (1, 2):
            rows = by("coop", dt, pg)
            gs = [(c, c.gather()) for c in rows]
            ncols = lambda g: g.ntaps * g.Cs
            assert all((pg == 2) == (dict(c.env).get("AST_WGRAD_PG_MINP") == "1") for c in rows)
            assert any(g.Cd % c.plan[1] for c, g in gs if c.plan[1] == 32) and any(g.Cd % 64 and g.Cd > 64 for c, g in gs)
            assert all(ncols(g) % (c.plan[2] * 16) for c, g in gs)                                   # every row: a partly empty last column tile
            assert any(ncols(g) > 320 for c, g in gs if c.plan[1] <= 32) and any(ncols(g) > 192 for c, g in gs if c.plan[1] == 64)    # gy > 1
            assert all(_P(g) % WC.BKP[dt] for c, g in gs)                                            # P no multiple of a K trip
            assert all(c.plan[4] > 1 and _P(g) % c.plan[5] for c, g in gs)                           # a shorter last slice
            assert all(g.N >= 2 and (g.Hm * g.Wm) % 2 for c, g in gs if g.Hm * g.Wm > 1)             # a K tile straddles the image boundary
            assert any(g.sh == 2 and g.Hs % 2 and g.Ws % 2 and g.ntaps == 9 for c, g in gs)
            assert any(g.ntaps == 1 and g.wtaps == 1 and g.Hm * g.Wm > 1 for c, g in gs)             # 1x1 kernel
            assert any(g.Hs == g.Ws == g.Hm == g.Wm == 1 and g.ntaps == 1 for c, g in gs)            # the linear geometry
            assert any(1 < g.ntaps < g.wtaps for c, g in gs)                                         # a parity class
            trips = lambda c, g: -(-(_P(g) - (c.plan[4] - 1) * c.plan[5]) // WC.BKP[dt])             # K trips of the last slice
            if pg == 2:
                assert any(trips(c, g) == 1 for c, g in gs), dt                                      # group 1 loads only zeros
                assert any(trips(c, g) % 2 and trips(c, g) > 1 for c, g in gs), dt                   # odd nk_all
                assert any((c.plan[5] // WC.BKP[dt]) % 2 == 0 for c, g in gs)
        for pg in (1, 2):
            gs = [(c, c.gather()) for c in by("halo", dt, pg)]
            assert {c.plan[1:3] for c, g in gs} == set(WC.HALO_TILES)
            assert any(1 < g.ntaps == 2 < g.wtaps for c, g in gs)                                    # the two-tap parity class
            E = 8 if dt == "bf16" else 4
            if pg == 1:
                effs = [g.Hm * g.Wm / (-(-g.Hm // 8) * 8 * -(-g.Wm // 16) * 16) for c, g in gs]
                assert any(0.6 <= e < 0.62 for e in effs), effs
                assert any(g.sh == 2 and g.ntaps == 9 for c, g in gs)                                # PH x PW = 17 x 33
                assert any(g.sh == 1 and g.ntaps == 9 and 10 * 18 * (g.Cs // E) <= 2560 < 10 * 18 * (g.Cs // E + 1) for c, g in gs)
        assert any(g.Cs == 8 for c, g in ((c, c.gather()) for c in by("halo", "bf16")))              # one 16-byte chunk per pixel
    rows = by("rows")
    assert any(not c.env for c in rows) and any(dict(c.env).get("AST_WGRAD_FLUSH_LDS") == "1" for c in rows)
    assert all(c.plan[3] == 4 for c in rows)                                                         # the default ring depth
    for fam in ("coop", "halo"):
        for pg in (1, 2):
            assert {c.dtype for c in by(fam, None, pg) if c.flush_lds} == {"f32", "bf16"}, (fam, pg)


def test_wgrad_case_inputs_meet_the_exactness_condition():
    """max A + max |old| < 2^24 for every row and draw, from the reference alone; one operand is full-width odd integers, the other
    -1 / 0 / 1; every pixel has a non-zero channel in both; the sentinel is no value a gradient can take unnoticed."""
    for c in WC.CASES:
        g = c.gather()
        for draw in (0, 1):
            d = WC.make_inputs(c, draw)
            dy, src = d["dy"].float(), d["src"].float()
            ref, A = WC.wgrad_ref(dy, src, g)
            assert float(A.max()) + float(d["old"].abs().max()) < WC.EXACT, (c.name, draw, float(A.max()))
            assert float(A.max()) >= 2 ** 10, (c.name, draw)                                        # sums, not a handful of products
            full, small = (dy, src) if draw == 0 else (src, dy)
            assert WC.FULL_MAX[c.dtype] // 2 < float(full.abs().max()) <= WC.FULL_MAX[c.dtype] and bool((full[full != 0] % 2 == 1).all()), (c.name, draw)
            assert set(small.unique().tolist()) == {-1.0, 0.0, 1.0}, (c.name, draw)
            assert bool((dy != 0).any(-1).all()) and bool((src != 0).any(-1).all()), (c.name, draw)
            assert bool((ref == ref.round()).all()) and float(ref.abs().max()) > 0
            assert bool(ref[:, WC.listed_taps(g)].abs().sum(dim=(0, 2)).gt(0).all()), (c.name, draw)


def _sources():
    return open(os.path.join(ROOT, "audio-style-transfer_amd", "csrc", "wgrad.hip")).read()


def test_wgrad_table_covers_every_instantiation_the_dispatcher_names():
    """The template-argument sets of wgrad_dispatch, read from the source: every (family, dtype, BMW, NCT, PG) they span is a row of
    the table or an entry of NOT_LAUNCHED, and neither lists anything else.  A new tile shape without a row fails here."""
    src = _sources()
    body = src[src.index("int wgrad_dispatch("):]
    body = body[:body.index("#undef AST_WG")]
    tiles = {(int(b), int(n)) for b, n in re.findall(r"AST_WG\((\d+), (\d+)\);", body)}
    halo_pg = {int(p) for p in re.findall(r"launch_wgrad_halo_pg<T, B_, N_, (\d+)>", body)}
    coop_pg = {int(p) for p in re.findall(r"launch_wgrad_pg<T, B_, N_, (\d+)>", body)}
    stages = {int(p) for p in re.findall(r"launch_wgrad_rows<(\d+)>", body)}
    assert "launch_wgrad_tap<T>" in body
    assert tiles == set(WC.COOP_TILES) and len(tiles) == 11 and halo_pg == {1, 2, 4} and coop_pg == {1, 2} and stages == {2, 3, 4}
    named = set()
    for dt in ("f32", "bf16"):
        named |= {("coop", dt, b, n, pg) for b, n in tiles for pg in coop_pg} | {("halo", dt, b, n, pg) for b, n in tiles for pg in halo_pg}
        named.add(("tap", dt, 64, 4, 1))
    named |= {("rows", "bf16", 64, 12, s) for s in stages}
    rows = {c.key for c in WC.CASES}
    assert not (rows & set(WC.NOT_LAUNCHED))
    assert rows | set(WC.NOT_LAUNCHED) == named, sorted(named ^ (rows | set(WC.NOT_LAUNCHED)))
    assert all(isinstance(r, str) and r for r in WC.NOT_LAUNCHED.values())
    # what NOT_LAUNCHED says about the knobs is true: each is reachable with its knob and not without
    g = IC.conv_gather(16, 61, 250, 8, 8, 3, 3, 1, 1, 1)          # 2048 tiles: enough for four pixel groups
    g64 = IC.conv_gather(2, 61, 250, 8, 40, 3, 3, 1, 1, 1)
    gr = IC.conv_gather(2, 17, 16, 64, 64, 3, 3, 1, 1, 1)
    with WC.case_env():
        assert WC.plan_of(g, "bf16")[:4] == (1, 16, 8, 2) and WC.plan_of(g64, "bf16")[0] == 0 and WC.plan_of(gr, "bf16")[:4] == (2, 64, 12, 4)
        for var, val, geo, want in (("AST_WGRAD_PG", "4", g, (1, 16, 8, 4)), ("AST_WGRAD_HALO_MAXCD", "64", g64, (1, 64, 8, 1)),
                                    ("AST_WGRAD_ROWS_STAGES", "3", gr, (2, 64, 12, 3)), ("AST_WGRAD_TAP", "1", gr, (3, 64, 4, 1))):
            os.environ[var] = val
            try:
                assert WC.plan_of(geo, "bf16")[:4] == want, (var, WC.plan_of(geo, "bf16"))
            finally:
                del os.environ[var]
        os.environ["AST_WGRAD_TAP"] = "1"
        try:
            assert WC.plan_of(gr, "bf16", 4)[0] == 2            # the tap kernel has no slab form
        finally:
            del os.environ["AST_WGRAD_TAP"]


def test_exact_comparison_rejects_broken_results():
    """The comparison the GPU test uses is not vacuous: it rejects the reference with one pixel dropped, one pixel doubled, the
    full-width operand rounded through bf16 (f32 rows), and a single element written into a guard band."""
    for name in ("c16x20-pg2-f32", "c64x12-pg1-bf16", "c32x8-pg1-f32", "h32x20-pg1-bf16", "h16x12-pg1-f32", "r-slab-bf16"):
        c = WC.BY_NAME[name]
        g = c.gather()
        for draw in (0, 1):
            d = WC.make_inputs(c, draw)
            dy, src = d["dy"].float(), d["src"].float()
            ref = WC.wgrad_ref(dy, src, g)[0]
            good = WC.Dw(g, fill=ref.float())
            assert WC.exact(good.dw[0], ref) and good.guards_intact()
            for n, h, w in ((0, 0, 0), (g.N - 1, g.Hm - 1, g.Wm - 1), (g.N // 2, g.Hm // 2, g.Wm // 3)):
                for factor in (0.0, 2.0):                                        # the pixel dropped / counted twice
                    dy2 = dy.clone()
                    dy2[n, h, w] *= factor
                    assert not WC.exact(WC.wgrad_ref(dy2, src, g)[0].float(), ref), (name, draw, n, h, w, factor)
            if c.dtype == "f32":
                full = "dy" if draw == 0 else "src"
                r = {"dy": dy, "src": src}
                r[full] = r[full].bfloat16().float()
                assert not WC.exact(WC.wgrad_ref(r["dy"], r["src"], g)[0].float(), ref), (name, draw)
            nan = ref.float().clone()
            nan[0, 0, 0] = float("nan")
            assert not WC.exact(nan, ref)
            for at in (WC.GUARD - 1, good.buf.numel() - WC.GUARD):
                bad = WC.Dw(g, fill=ref.float())
                bad.buf[at] = 0.0
                assert not bad.guards_intact()


def test_wgrad_plan_refuses_bad_arguments():
    L = _lib.lib()
    out = (ctypes.c_int32 * 6)()
    g = ops.gather_direct(2, 9, 19, 8, 16, 3, 1, 1)[0]
    assert L.ast_wgrad_plan(g, _lib.BF16, 0, ctypes.byref(out)) == 0 and tuple(out)[:4] == (0, 16, 8, 1)
    assert L.ast_wgrad_plan(g, _lib.BF16, 0, None) < 0 and b"null" in L.ast_last_error()
    assert L.ast_wgrad_plan(None, _lib.BF16, 0, ctypes.byref(out)) < 0
    assert L.ast_wgrad_plan(g, _lib.BF16, -1, ctypes.byref(out)) < 0 and b"slab cap" in L.ast_last_error()
    assert L.ast_wgrad_plan(g, _lib.BF16, 4097, ctypes.byref(out)) < 0
    assert L.ast_wgrad_plan(g, 7, 0, ctypes.byref(out)) < 0 and b"dtype" in L.ast_last_error()
    for cs, cd in ((4, 16), (8, 12)):
        bad = IC.conv_gather(2, 9, 19, cs, cd, 3, 3, 1, 1, 1)
        assert L.ast_wgrad_plan(bad, _lib.F32, 0, ctypes.byref(out)) < 0 and b"multiples of 8" in L.ast_last_error()
    # a geometry without taps launches nothing: family -1
    none = type(g).from_buffer_copy(g)
    none.ntaps = 0
    assert L.ast_wgrad_plan(none, _lib.F32, 0, ctypes.byref(out)) == 0 and tuple(out) == (-1, 0, 0, 0, 0, 0)
    # the knobs are read per call
    big = ops.gather_direct(2, 21, 27, 8, 16, 3, 1, 1)[0]
    with WC.case_env():
        one = WC.plan_of(big, "f32")
    with WC.case_env(AST_WGRAD_PG_MINP=1):
        two = WC.plan_of(big, "f32")
    assert one[3] == 1 and two[3] == 2 and one[:3] == two[:3]
