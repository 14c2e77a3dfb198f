"""Float64 reference of the gather-GEMM contract (include/ast_hip.h: ast_gather_t / ast_igemm), the derived per-element
error bound, seeded inputs, and the table of cases that tests/test_gpu_igemm_variants.py launches -- one row per kernel
variant the planner of csrc/igemm.hip can select.  Everything here runs on the CPU; tests/test_host_cpu.py checks the
reference against F.conv2d / F.conv_transpose2d and pins every row's plan without a GPU.

Geometry notes (the table's shapes follow from them):
  * a launch over N = 2 images has an even M = 2 * Hm * Wm, so "M = 2 BM + 5" and "M = 262144 k + 37" cannot be met exactly
    with two images; the rows take the nearest M above them that keeps Hm * Wm odd (a tile straddles the image boundary, the
    last tile is partial, the direct kernel's pixel walk crosses the boundary inside a wave's run);
  * the library takes channel counts in multiples of 8 only (check_gather; the host suite asserts that Cs = 4 is refused), and
    a 3x3 gather of 8 f32 channels has 18 sixteen-byte chunks, more than the direct kernel's 12: no 3x3 f32 geometry reaches
    the direct kernel.  The f32 direct rows use a 2x3 kernel (12 chunks) where the bf16 rows use 3x3 (9 chunks);
  * ast_igemm_plan reports a patch plan as (-TH, channel tile, -slab bytes, -(fragments) for row blocks else 1, 1), which does
    not tell WALL on from off or, for 2-D tiles, the fragment count: a patch row also records ast_pconv_variant's
    (SLB, TM, TN, WALL), the template arguments of the pconv_kernel instantiation the launch runs (TM x 4 fragments).

PATCH_SELECTABLE lists every pconv_kernel instantiation plan_pconv can select by itself and the table launches; the ones it
can select but the table leaves alone are in PATCH_NOT_LAUNCHED, with the reason.
"""
from __future__ import annotations

import ctypes
import functools
import os
import zlib
from dataclasses import dataclass

import torch

from ast_amd import _lib, ops

SENTINEL = -24576.0          # -1.5 * 2^14: exact in bf16 and f32, far outside every row's outputs (checked per row on the CPU)
GUARD = 1024                 # sentinel elements before and after dst: writes past either end of the tensor land here
U24 = 2.0 ** -24
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


# ---- geometry -------------------------------------------------------------------------------------------------------

def taps_of(g):
    return [((g.tap[i] & 255) - 64, ((g.tap[i] >> 8) & 255) - 64, g.tap[i] >> 16) for i in range(g.ntaps)]


@functools.lru_cache(maxsize=None)
def conv_gather(N, H, W, Cs, Cd, kh, kw, stride, ph, pw):
    """Conv2d forward geometry for a kh x kw kernel (ops.gather_direct itself for the square ones)."""
    if kh == kw and ph == pw:
        return ops.gather_direct(N, H, W, Cs, Cd, kh, stride, ph)[0]
    Ho, Wo = (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1
    taps = tuple((i, j, i * kw + j) for i in range(kh) for j in range(kw))
    return ops._mk(N, H, W, Cs, Ho, Wo, stride, stride, -ph, -pw, Ho, Wo, Cd, 1, 1, 0, 0, taps, kh * kw)


def grid_mask(g):
    """[Hd, Wd] bool: the destination pixels a launch writes."""
    m = torch.zeros(g.Hd, g.Wd, dtype=torch.bool)
    m[g.doh:g.doh + (g.Hm - 1) * g.dsh + 1:g.dsh, g.dow:g.dow + (g.Wm - 1) * g.dsw + 1:g.dsw] = True
    return m


# ---- the float64 reference ------------------------------------------------------------------------------------------

def _span(n_out, stride, off, n_src):
    """Logical indices i in [0, n_out) whose source coordinate i * stride + off lies in [0, n_src): (first, last) or None."""
    lo = max(0, -(off // stride))                 # ceil(-off / stride)
    hi = min(n_out - 1, (n_src - 1 - off) // stride)
    return (lo, hi) if hi >= lo else None


def gather_contract(src, wgt, g):
    """sum over taps and channels on the logical grid, and the same over absolute values: two [N, Hm, Wm, Cd] f64 tensors."""
    src, wgt = src.double(), wgt.double()
    assert tuple(src.shape) == (g.N, g.Hs, g.Ws, g.Cs) and tuple(wgt.shape) == (g.Cd, g.wtaps, g.Cs)
    asrc, awgt = src.abs(), wgt.abs()
    out = torch.zeros(g.N, g.Hm, g.Wm, g.Cd, dtype=torch.float64)
    A = torch.zeros_like(out)
    for dh, dw, wt in taps_of(g):
        hs, ws = _span(g.Hm, g.sh, g.oh + dh, g.Hs), _span(g.Wm, g.sw, g.ow + dw, g.Ws)
        if hs is None or ws is None:
            continue                              # the whole tap reads outside the image: zeros
        (h0, h1), (w0, w1) = hs, ws
        ys = slice(h0 * g.sh + g.oh + dh, h1 * g.sh + g.oh + dh + 1, g.sh)
        xs = slice(w0 * g.sw + g.ow + dw, w1 * g.sw + g.ow + dw + 1, g.sw)
        out[:, h0:h1 + 1, w0:w1 + 1, :] += src[:, ys, xs, :] @ wgt[:, wt, :].t()
        A[:, h0:h1 + 1, w0:w1 + 1, :] += asrc[:, ys, xs, :] @ awgt[:, wt, :].t()
    return out, A


def gather_gemm_ref(src, wgt, bias, g, old_dst=None, relu=False, core=None):
    """dst[n, hm*dsh+doh, wm*dsw+dow, :] = act(sum_{t,c} src[gather(pix,t)][c] * wgt[co][wtap[t]][c] + bias (+ old_dst)) in float64.
    Returns (dst, A), both [N, Hd, Wd, Cd]: destination pixels off the grid keep old_dst (zero without one) and have A = 0;
    A = sum |x| |w| + |bias| (+ |old|) is the magnitude the rounding-error bound scales with.  core: a gather_contract result to
    reuse (the contraction does not depend on bias / old_dst / relu)."""
    out, A = (t.clone() for t in (core if core is not None else gather_contract(src, wgt, g)))
    if bias is not None:
        out += bias.double()
        A += bias.double().abs()
    dst = old_dst.double().clone() if old_dst is not None else torch.zeros(g.N, g.Hd, g.Wd, g.Cd, dtype=torch.float64)
    assert tuple(dst.shape) == (g.N, g.Hd, g.Wd, g.Cd)
    Ad = torch.zeros_like(dst)
    view = dst[:, g.doh::g.dsh, g.dow::g.dsw, :][:, :g.Hm, :g.Wm, :]
    if old_dst is not None:
        out += view
        A += view.abs()
    if relu:
        out.clamp_(min=0)
    view.copy_(out)
    Ad[:, g.doh::g.dsh, g.dow::g.dsw, :][:, :g.Hm, :g.Wm, :].copy_(A)
    return dst, Ad


def out_bound(ref, A, g, bf16):
    """|y - ref| <= 2 K 2^-24 A + (bf16 outputs) 2^-8 |ref|.
    First term: f32 accumulation, in any order, of K = ntaps * Cs exact products, the bias and the old value: at most
    (K + 2) 2^-24 A to first order; 2 K covers the two extra terms and the higher orders for every K >= 8.
    Second term: the one rounding of the f32 result to bf16.  bf16 keeps 8 significant bits, so round-to-nearest is off by at
    most 2^-8 |y32| <= 2^-8 (|ref| + e): the term is that rounding with no margin of its own, and the slack of the first term
    (2 K against K + 2) absorbs the 2^-8 e."""
    K = max(1, g.ntaps * g.Cs)
    b = 2.0 * K * U24 * A
    return b + 2.0 ** -8 * ref.abs() if bf16 else b


def sum_bound(n, abs_sum):
    """The same form for a sum of n f32 values accumulated in f32 in any order."""
    return 2.0 * n * U24 * abs_sum


# ---- seeded inputs ----------------------------------------------------------------------------------------------------

MASK_MARGIN = 1e-3


def make_inputs(case):
    """CPU tensors, already rounded to the compute dtype: src, wgt (x 0.1), bias (f32, non-zero), old (a previous dst),
    bn_x / scale / shift with |fma(x, scale, shift)| > MASK_MARGIN everywhere (offending elements are redrawn)."""
    g, dt = case.gather(), DTYPES[case.dtype]
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    r = lambda *s: torch.randn(*s, generator=gen)
    d = {"src": r(g.N, g.Hs, g.Ws, g.Cs).to(dt), "wgt": (0.1 * r(g.Cd, g.wtaps, g.Cs)).to(dt)}
    bias = r(g.Cd)
    d["bias"] = torch.where(bias.abs() < 0.05, torch.full_like(bias, 0.25), bias)
    d["old"] = r(g.N, g.Hd, g.Wd, g.Cd).to(dt)
    d["scale"] = 0.5 + torch.rand(g.Cd, generator=gen)
    d["shift"] = 0.5 * r(g.Cd)
    x = r(g.N, g.Hd, g.Wd, g.Cd).to(dt)
    for _ in range(64):
        bad = bn_pre(x, d["scale"], d["shift"]).abs() <= 2 * MASK_MARGIN
        nbad = int(bad.sum())
        if nbad == 0:
            break
        x[bad] = r(nbad).to(dt)
    d["bn_x"] = x
    return d


def bn_pre(x, scale, shift):
    return x.double() * scale.double() + shift.double()


# ---- the case table ---------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Case:
    name: str
    family: str          # "gathered" | "direct" | "patch": the kernel family the row is meant to run
    dtype: str           # "f32" | "bf16"
    geom: tuple          # ("conv", N, H, W, Cs, Cd, kh, kw, stride, ph, pw) | ("convT", N, Hs, Ws, Cs, Hd, Wd, Cd, k, stride, pad, class)
    env: tuple           # ((variable, value), ...): AST_IGEMM_FORCE / AST_PCONV* only (read per call)
    plan: tuple          # ast_igemm_plan's five integers under env
    ws: int              # ast_igemm_ws_floats under env
    note: str = ""
    pc: tuple = ()       # patch rows: ast_pconv_variant's (SLB, TM, TN, WALL) under env

    def gather(self):
        if self.geom[0] == "conv":
            return conv_gather(*self.geom[1:])
        return ops.gathers_transposed(*self.geom[1:-1])[self.geom[-1]]


class case_env:
    """The row's environment for the duration of a block; the five planner variables a row does not set are removed, and the
    cached workspace needs (ops._ws_cache) are dropped on both edges, since the plan changes with the environment."""
    VARS = ("AST_IGEMM_FORCE", "AST_PCONV", "AST_PCONV_MIN_TILES", "AST_PCONV_NF", "AST_PCONV_WALL")

    def __init__(self, case):
        self.kv = dict(case.env)
        assert set(self.kv) <= set(self.VARS)

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in self.VARS}
        os.environ.update(self.kv)
        ops._ws_cache.clear()

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        ops._ws_cache.clear()
        return False


def plan_of(g, dtype):
    out = (ctypes.c_int32 * 5)()
    assert _lib.lib().ast_igemm_plan(g, _lib.dcode(DTYPES[dtype]), ctypes.byref(out)) == 0
    return tuple(out), int(_lib.lib().ast_igemm_ws_floats(g, _lib.dcode(DTYPES[dtype])))


def patch_variant_of(g, dtype):
    """(SLB, TM, TN, WALL) of the pconv_kernel instantiation the launch runs, () when the patch kernel does not take it."""
    out = (ctypes.c_int32 * 4)()
    rc = _lib.lib().ast_pconv_variant(g, _lib.dcode(DTYPES[dtype]), ctypes.byref(out))
    assert rc in (0, 1)
    return tuple(out) if rc else ()


def _rows():
    rows = []

    def add(name, family, dtype, geom, env, plan, ws, note="", pc=()):
        rows.append(Case(f"{name}-{dtype}", family, dtype, tuple(geom), tuple(sorted(env.items())), tuple(plan), ws, note, tuple(pc)))

    both = ("f32", "bf16")
    # Cs with a power-of-two chunk count per pixel (8: the shift path, uniform taps for kch 4 and 8) and without (6: the division
    # path, taps change inside a K tile, K tail inside the last tile)
    cs_shift, cs_div = {"f32": 32, "bf16": 64}, {"f32": 24, "bf16": 48}

    # -- gathered kernel: every tile the planner can pick, forced onto a 3x3 stride-1 pad-1 layer of two images of BM + 1 (64-row
    # tiles: 5 x 13) or BM + 5 (128-row tiles: 7 x 19) pixels with BN + 8 output channels.  Split-K only where plan_igemm splits
    # by itself (the 32- and 16-channel tiles).
    hw = {64: (5, 13), 128: (7, 19)}
    tiles = [(64, 64, 4, 1, (1,)), (64, 64, 8, 1, (1,)), (64, 64, 8, 4, (1,)), (64, 128, 4, 1, (1,)), (64, 128, 8, 1, (1,)),
             (64, 32, 4, 1, (1, 2, 4)), (128, 32, 4, 1, (1, 2, 4)), (64, 16, 4, 1, (1, 2, 4)), (128, 16, 4, 1, (1, 2, 4))]
    for bm, bn, kch, kg, splits in tiles:
        H, W = hw[bm]
        for ns in splits:
            for dt in both:
                for tag, cs in (("shift", cs_shift[dt]), ("div", cs_div[dt])):
                    force = f"{bm},{bn},{kch},{ns}" + (",4" if kg == 4 else "")
                    M, Cd = 2 * H * W, bn + 8
                    add(f"g{bm}x{bn}k{kch}" + ("kg4" if kg == 4 else "") + f"s{ns}-{tag}", "gathered", dt,
                        ("conv", 2, H, W, cs, Cd, 3, 3, 1, 1, 1), {"AST_IGEMM_FORCE": force, "AST_PCONV": "0"},
                        (bm, bn, kch, ns, kg), M * Cd if ns > 1 else 0)
    # three images (per-image statistics: Hm * Wm = BM + 1 / BM + 5 is no multiple of BM) on the tiles production uses them with
    for bm, bn, kch, kg in ((64, 64, 8, 1), (64, 64, 8, 4), (64, 128, 8, 1), (128, 32, 4, 1), (64, 32, 4, 1)):
        H, W = hw[bm]
        for dt in both:
            add(f"g{bm}x{bn}k{kch}" + ("kg4" if kg == 4 else "") + "-n3", "gathered", dt, ("conv", 3, H, W, cs_shift[dt], bn + 8, 3, 3, 1, 1, 1),
                {"AST_IGEMM_FORCE": f"{bm},{bn},{kch},1" + (",4" if kg == 4 else ""), "AST_PCONV": "0"}, (bm, bn, kch, 1, kg), 0)
    # stride 2, 1x1 and one parity class of a stride-2 data gradient (4 taps, destination stride 2, offset 1) on 64x64 and 64x32
    for bn in (64, 32):
        for dt in both:
            cs, Cd = cs_shift[dt], bn + 8
            k3 = 8 if bn == 64 else 4
            add(f"g64x{bn}-s2", "gathered", dt, ("conv", 2, 9, 25, cs, Cd, 3, 3, 2, 1, 1),
                {"AST_IGEMM_FORCE": f"64,{bn},{k3},1", "AST_PCONV": "0"}, (64, bn, k3, 1, 1), 0)
            add(f"g64x{bn}-1x1", "gathered", dt, ("conv", 2, 5, 13, cs, Cd, 1, 1, 1, 0, 0),
                {"AST_IGEMM_FORCE": f"64,{bn},4,1", "AST_PCONV": "0"}, (64, bn, 4, 1, 1), 0)
            add(f"g64x{bn}-parity", "gathered", dt, ("convT", 2, 5, 13, cs, 10, 26, Cd, 3, 2, 1, 3),
                {"AST_IGEMM_FORCE": f"64,{bn},{k3},1", "AST_PCONV": "0"}, (64, bn, k3, 1, 1), 0)

    # -- gathered kernel, unforced, on both sides of the production thresholds (8 source channels keep the tensors small)
    for dt in both:
        k = 8 if dt == "f32" else 4                   # 3x3 x 8 channels: 18 chunks in f32 (kch 8 for 64+-channel tiles), 9 in bf16
        add("thr-m4140-cd32", "gathered", dt, ("conv", 2, 45, 46, 8, 32, 3, 3, 1, 1, 1), {}, (128, 32, 4, 1, 1), 0, "M >= 4096: 128-row tiles")
        add("thr-m4050-cd32", "gathered", dt, ("conv", 2, 45, 45, 8, 32, 3, 3, 1, 1, 1), {}, (64, 32, 4, 1, 1), 0, "M < 4096")
        add("thr-m30012-cd136", "gathered", dt, ("conv", 2, 123, 122, 8, 136, 3, 3, 1, 1, 1), {}, (64, 128, k, 1, 1), 0, "M >= 30000: 64x128")
        add("thr-m29768-cd136", "gathered", dt, ("conv", 2, 122, 122, 8, 136, 3, 3, 1, 1, 1), {}, (64, 64, k, 1, 1), 0, "M < 30000")
        # the planner's own in-workgroup K groups (under-filled grid, >= 16 K tiles) and its own split-K (128x32, 151 tiles)
        add("nat-kg4", "gathered", dt, ("conv", 2, 5, 13, 2 * cs_shift[dt], 72, 3, 3, 1, 1, 1), {}, (64, 64, 8, 1, 4), 0)
        add("nat-split2", "gathered", dt, ("conv", 2, 97, 99, cs_shift[dt], 24, 3, 3, 1, 1, 1), {}, (128, 32, 4, 2, 1), 2 * 97 * 99 * 24)

    # -- direct kernel: Cd 8 / 16, 1..12 chunks (NKS 1, 2, 3), jt = 1 on two images of 7 x 19 pixels (M = 266: five workgroups)
    small = {"f32": [("nks1", 8, 1, 1, 1, 0, 0, 7), ("nks2-div", 24, 1, 1, 1, 0, 0, 7), ("nks3", 8, 2, 3, 1, 1, 1, 6), ("nks3-div", 40, 1, 1, 1, 0, 0, 7),
                     ("nks3-s2", 8, 2, 3, 2, 1, 1, 12)],
             "bf16": [("nks1", 8, 1, 1, 1, 0, 0, 7), ("nks2", 8, 2, 3, 1, 1, 1, 6), ("nks2-div", 48, 1, 1, 1, 0, 0, 7), ("nks3", 8, 3, 3, 1, 1, 1, 7),
                      ("nks3-s2", 8, 3, 3, 2, 1, 1, 13)]}
    for dt in both:
        for tag, cs, kh, kw, s, ph, pw, H in small[dt]:
            for Cd in (8, 16):
                W = 19 if s == 1 else 37
                add(f"d-cd{Cd}-{tag}", "direct", dt, ("conv", 2, H, W, cs, Cd, kh, kw, s, ph, pw), {}, (64, 16, 0, 1, 1), 0)
    # jt = 2, 4, 8: M just above 262144 x {1, 2, 4} over two images (331 x 397, 509 x 517, 723 x 727 output pixels each)
    for dt in both:
        kh, dH = (2, -1) if dt == "f32" else (3, 0)     # output rows: H + 2 - kh + 1
        add("d-jt2-s2", "direct", dt, ("conv", 2, 661 + dH, 793, 8, 8, kh, 3, 2, 1, 1), {}, (128, 16, 0, 1, 1), 0, "M = 262814")
        add("d-jt4", "direct", dt, ("conv", 2, 509 + dH, 517, 8, 8, kh, 3, 1, 1, 1), {}, (256, 16, 0, 1, 1), 0, "M = 526306")
        add("d-jt8", "direct", dt, ("conv", 2, 723 + dH, 727, 8, 8, kh, 3, 1, 1, 1), {}, (512, 16, 0, 1, 1), 0, "M = 1051242")

    # -- patch kernel as production selects it (AST_PCONV_NF never set).  min1 = AST_PCONV_MIN_TILES=1: the shape has fewer than
    # the default 192 tiles.  Hm, Wm are no multiples of the tile in any 2-D row; a row-block tile spans the image width, and the
    # planner gives the 12- and 4-fragment forms the whole image (9 x 19, 5 x 10), so there the overhang is the partial last fragment.
    min1 = {"AST_PCONV_MIN_TILES": "1"}
    for name, dt, geom, env, plan, pc, note in _PATCH_ROWS:
        add(name, "patch", dt, ("conv",) + geom, dict(min1) if env == "min1" else dict(env), plan, 0, note, pc)
    return rows


# (name, dtype, (N, H, W, Cs, Cd, kh, kw, stride, ph, pw), environment, plan, (SLB, TM, TN, WALL), what the row is)
def _patch_rows():
    rows = []
    g3 = lambda N, H, W, Cs, Cd: (N, H, W, Cs, Cd, 3, 3, 1, 1, 1)
    for dt, c64, c128 in (("f32", 16, 32), ("bf16", 32, 64)):      # source channels of one 64-byte / 128-byte slab
        rows += [
            ("p64-8f-tn2", dt, g3(2, 13, 70, c64, 32), "min1", (-8, 32, -64, 1, 1), (64, 2, 2, 0), "64-byte slabs, 8x16-pixel tiles (8 fragments: 16 need 1024 tiles), 20 tiles"),
            ("p64-16f", dt, g3(8, 175, 190, c64, 32), {}, (-16, 32, -64, 1, 1), (64, 4, 2, 0), "64-byte slabs, 16x16-pixel tiles (16 fragments), 1056 tiles"),
            ("p64-16f-tn4", dt, g3(32, 125, 49, c64, 64), {}, (-16, 64, -64, 1, 1), (64, 4, 4, 0), "the same with 64-channel tiles: 1024 tiles, the fewest that select 16 fragments"),
            ("p64-8f-tn4", dt, g3(5, 61, 67, c64, 64), {}, (-8, 64, -64, 1, 1), (64, 2, 4, 0), "64-byte slabs, 64-channel tiles, 200 tiles"),
            ("p128-8f-tn2", dt, g3(2, 61, 67, c128, 32), "min1", (-8, 32, -128, 1, 1), (128, 2, 2, 0), "128-byte slabs, 8 fragments, 32-channel tiles, 80 tiles"),
            ("p128-8f-tn4", dt, g3(5, 61, 67, c128, 64), {}, (-8, 64, -128, 1, 1), (128, 2, 4, 0), "128-byte slabs, 8 fragments (150 12-fragment tiles < 384), 200 tiles"),
            ("p128-12f-tn4", dt, g3(4, 90, 100, c128, 128), {}, (-12, 64, -128, 1, 1), (128, 3, 4, 0), "128-byte slabs, 12x16-pixel tiles (12 fragments), 448 tiles"),
            ("p128-rows8", dt, g3(2, 17, 38, c128, 64), "min1", (-3, 32, -128, -8, 1), (128, 2, 2, 0), "row blocks: 3 full rows of 38 pixels (17 rows: a partial last block), 8 fragments"),
            ("p128-rows12", dt, g3(3, 9, 19, c128, 64), "min1", (-9, 32, -128, -12, 1), (128, 3, 2, 0), "row blocks: the whole 9x19 image (171 of 192 fragment pixels), 12 fragments"),
            ("p64-rows8", dt, g3(3, 19, 23, c64, 32), "min1", (-5, 32, -64, -8, 1), (64, 2, 2, 0), "row blocks on 64-byte slabs: 5 rows of 23 pixels"),
            ("p64-rows12-tn2", dt, g3(3, 9, 19, c64, 32), "min1", (-9, 32, -64, -12, 1), (64, 3, 2, 0), "12-fragment row blocks on 64-byte slabs: the whole 9x19 image"),
            ("p64-rows12-tn4", dt, g3(50, 9, 19, c64, 256), {}, (-9, 64, -64, -12, 1), (64, 3, 4, 0), "the same with 64-channel tiles (50 images x 4 channel tiles = 200 tiles)"),
            ("p128-tiny4", dt, g3(2, 5, 10, c128, 64), "min1", (-5, 32, -128, -4, 1), (128, 1, 2, 0), "the 4-fragment tile of a 5x10 image (50 of 64 fragment pixels)"),
            ("p128-tiny4-tn4", dt, g3(50, 5, 10, c128, 256), {}, (-5, 64, -128, -4, 1), (128, 1, 4, 0), "the same with 64-channel tiles (50 images x 4 channel tiles = 200 tiles)"),
        ]
    # >= 4 channel slabs, 3x3: bf16 takes WALL (all taps' weights resident), which forces 32-channel tiles; AST_PCONV_WALL=0 and
    # f32 (never WALL) take the 64-channel tiles the tile count allows.  The deep layers WALL was built for are the 9x19 and 5x10
    # images of 512 channels: their tile forms (12-fragment row blocks, the 4-fragment tile) at 256 channels, the fewest with 4 slabs.
    off = {"AST_PCONV_WALL": "0"}
    rows += [
        ("p128-wall-rows", "bf16", g3(3, 33, 50, 256, 256), {}, (-2, 32, -128, -8, 1), (128, 2, 2, 1), "WALL on, row blocks, 4 slabs, 408 tiles"),
        ("p128-nowall-rows", "bf16", g3(3, 33, 50, 256, 256), off, (-2, 64, -128, -8, 1), (128, 2, 4, 0), "the same with WALL off"),
        ("p128-4slab-rows", "f32", g3(3, 33, 50, 128, 256), {}, (-2, 64, -128, -8, 1), (128, 2, 4, 0), "4 slabs in f32 (no WALL)"),
        ("p128-wall-2d", "bf16", g3(5, 61, 67, 256, 64), {}, (-8, 32, -128, 1, 1), (128, 2, 2, 1), "WALL on, 8x16-pixel tiles, 4 slabs, 400 tiles"),
        ("p128-nowall-2d", "bf16", g3(5, 61, 67, 256, 64), off, (-8, 64, -128, 1, 1), (128, 2, 4, 0), "the same with WALL off"),
        ("p128-wall-rows12", "bf16", g3(3, 9, 19, 256, 64), "min1", (-9, 32, -128, -12, 1), (128, 3, 2, 1), "WALL on, 12-fragment row blocks: the whole 9x19 image, 4 slabs"),
        ("p128-nowall-rows12", "bf16", g3(3, 9, 19, 256, 64), dict(off, AST_PCONV_MIN_TILES="1"), (-9, 32, -128, -12, 1), (128, 3, 2, 0), "the same with WALL off"),
        ("p128-wall-tiny4", "bf16", g3(2, 5, 10, 256, 64), "min1", (-5, 32, -128, -4, 1), (128, 1, 2, 1), "WALL on, the 4-fragment tile of a 5x10 image, 4 slabs"),
        ("p128-nowall-tiny4", "bf16", g3(2, 5, 10, 256, 64), dict(off, AST_PCONV_MIN_TILES="1"), (-5, 32, -128, -4, 1), (128, 1, 2, 0), "the same with WALL off"),
    ]
    return rows


# Every (SLB, TM, TN, WALL) plan_pconv selects without AST_PCONV_NF / AST_PCONV_WALL: TM 2, 3, 4 on 64-byte slabs (8, 12, 16
# fragments; 12 only as row blocks), TM 1, 2, 3 on 128-byte slabs, TN 2 and 4 for each; WALL in bf16 only, always with TN 2.
# The host suite asserts that the table reaches each of these in each dtype it exists for.
PATCH_SELECTABLE = {
    "f32": {(slb, tm, tn, 0) for slb, tms in ((64, (2, 3, 4)), (128, (1, 2, 3))) for tm in tms for tn in (2, 4)},
    "bf16": {(slb, tm, tn, 0) for slb, tms in ((64, (2, 3, 4)), (128, (1, 2, 3))) for tm in tms for tn in (2, 4)}
            | {(128, tm, 2, 1) for tm in (1, 2, 3)},
}
# Selectable, not launched: WALL on 64-byte slabs needs >= 4 slabs in a pixel row that is an odd multiple of 64 bytes, i.e.
# 160, 224, ... bf16 source channels.  No layer of the model has such a count, so these three instantiations have never run
# on hardware; the table does not launch them for the first time on a shared machine.
PATCH_NOT_LAUNCHED = {"bf16": {(64, tm, 2, 1) for tm in (2, 3, 4)}}


# (name, dtype, (N, H, W, Cs, Cd, kh, kw, stride, ph, pw), environment, plan, (SLB, TM, TN, WALL), what the row is)
_PATCH_ROWS = _patch_rows()

CASES = _rows()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
