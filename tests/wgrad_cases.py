"""Float64 reference of the weight-gradient contract (include/ast_hip.h: ast_wgrad), exact integer inputs, and the table of
cases that tests/test_gpu_wgrad_variants.py launches -- one row per kernel instantiation the dispatcher of csrc/wgrad.hip
selects by default.  Everything here runs on the CPU; tests/test_wgrad_cases_cpu.py checks the reference against the
F.conv2d / F.conv_transpose2d weight gradients and pins every row's plan (ast_wgrad_plan) without a GPU.

Exactness.  Every row's dy and src hold integers: one operand carries the full significand of the dtype under test (odd
integers up to +-255 in bf16, +-4095 in f32: 8 and 12 significant bits), the other is -1, 0 or 1.  Every product and every
partial sum, in any order and through any number of atomics, is then an integer of magnitude at most
A = sum_pix |dy| |src| (+ |old| in the accumulate form), and while A + |old| < 2^24 each of them is exact in f32: the result
must EQUAL the float64 reference.  That is a condition on the inputs (the CPU suite asserts it for every row and draw), not
a tolerance.  The number of non-zero channels per pixel is chosen from the pixel count so that the expected A stays below
2^22; every pixel keeps at least one non-zero channel in both operands, so no pixel can vanish unnoticed.  Each row is drawn
twice: draw 0 has dy full-width and src in {-1, 0, 1}, draw 1 the other way round.

What the dispatcher can select (read from wgrad_dispatch / plan_wgrad; the CPU suite re-derives the sets from the source):
  cooperative wgrad_kernel<T, BMW, NCT, PG, SLAB>: BMW from Cd (<= 16: 16, <= 32: 32, else 64), NCT from the 16-column tiles
    of ntaps * Cs (4, 8, 12, 20; 4, 8, 12 at BMW 64), PG = 2 from AST_WGRAD_PG_MINP (100000) pixels, else 1;
  wgrad_halo_kernel<T, BMW, NCT, PG, SLAB>: Cd <= 32 (BMW 16, 32), >= 2 taps, >= 256 8x16-pixel tiles at >= 60 % fill, patch of
    at most 2560 16-byte chunks; PG = 2 from 1024 tiles;
  wgrad_rows_kernel<NST, SLAB>: bf16 3x3 stride-1 "same" layers with channel counts multiples of 64, NST = 4 ring stages;
  SLAB is the entry point (ast_wgrad_slab), the atomic flush through LDS is AST_WGRAD_FLUSH_LDS=1: every row runs both.
NOT_LAUNCHED lists the instantiations that only a tuning knob reaches, with the reason the table leaves each alone.
"""
from __future__ import annotations

import ctypes
import os
import zlib
from dataclasses import dataclass

import torch

import igemm_cases as IC
from ast_amd import _lib, ops

SENTINEL = IC.SENTINEL        # -24576: exact in f32, no integer-valued gradient of the table comes near it unnoticed (a guard is compared bitwise)
GUARD = IC.GUARD
DTYPES = IC.DTYPES
EXACT = 2 ** 24               # integers of magnitude below this are exact in f32, and so are their sums while they stay below it
BUDGET = 2 ** 22              # the expected A the channel densities aim for
OLD_MAX = 1000                # |old| of the accumulate form
FULL_MAX = {"bf16": 255, "f32": 4095}
BKP = {"bf16": 64, "f32": 32}                      # pixels per K trip of the cooperative kernel (WgradCfg<T>::BKP)
FAMILIES = ("coop", "halo", "rows", "tap")         # ast_wgrad_plan's family codes 0..3


# ---- the float64 reference ------------------------------------------------------------------------------------------

def wgrad_ref(dy, src, g):
    """dW[cd][wtap[t]][c] = sum_pix dy[pix][cd] * src[gather(pix, t)][c] over the logical grid, zeros outside the source image,
    and A, the same sum over absolute values: two [Cd, wtaps, Cs] float64 tensors.  Slices of taps g does not list stay zero."""
    dy, src = dy.double(), src.double()
    assert tuple(dy.shape) == (g.N, g.Hm, g.Wm, g.Cd) and tuple(src.shape) == (g.N, g.Hs, g.Ws, g.Cs)
    ady, asrc = dy.abs(), src.abs()
    dW = torch.zeros(g.Cd, g.wtaps, g.Cs, dtype=torch.float64)
    A = torch.zeros_like(dW)
    for dh, dw, wt in IC.taps_of(g):
        hs, ws = IC._span(g.Hm, g.sh, g.oh + dh, g.Hs), IC._span(g.Wm, g.sw, g.ow + dw, g.Ws)
        if hs is None or ws is None:
            continue                              # the whole tap reads outside the image: zeros
        (h0, h1), (w0, w1) = hs, ws
        ys = slice(h0 * g.sh + g.oh + dh, h1 * g.sh + g.oh + dh + 1, g.sh)
        xs = slice(w0 * g.sw + g.ow + dw, w1 * g.sw + g.ow + dw + 1, g.sw)
        dW[:, wt, :] += dy[:, h0:h1 + 1, w0:w1 + 1, :].reshape(-1, g.Cd).t() @ src[:, ys, xs, :].reshape(-1, g.Cs)
        A[:, wt, :] += ady[:, h0:h1 + 1, w0:w1 + 1, :].reshape(-1, g.Cd).t() @ asrc[:, ys, xs, :].reshape(-1, g.Cs)
    return dW, A


def listed_taps(g):
    """[wtaps] bool: the weight slices the geometry writes."""
    m = torch.zeros(g.wtaps, dtype=torch.bool)
    for _, _, wt in IC.taps_of(g):
        m[wt] = True
    return m


# ---- exact inputs -----------------------------------------------------------------------------------------------------

def densities(case):
    """(non-zero channels per pixel of the full-width operand, of the {-1, 0, 1} operand) for each draw: the densest pair, halving
    the small operand first, whose expected A = P * mean|full| * (kf / Cf) * (ks / Cs) stays within BUDGET."""
    g = case.gather()
    P, mean = g.N * g.Hm * g.Wm, (FULL_MAX[case.dtype] + 1) / 2
    out = []
    for cf, cs in ((g.Cd, g.Cs), (g.Cs, g.Cd)):       # draw 0: dy full-width; draw 1: src full-width
        kf, ks = cf, max(1, cs // 2)
        while P * mean * kf * ks > BUDGET * cf * cs and (ks > 1 or kf > 1):
            if ks > 1:
                ks = max(1, ks // 2)
            else:
                kf = max(1, kf // 2)
        out.append((kf, ks))
    return out


def _operand(npix, C, k, maxv, gen):
    """[npix, C] f32: k non-zero channels per pixel (k >= 1), odd integers of magnitude <= maxv with random signs."""
    keep = torch.zeros(npix, C, dtype=torch.bool)
    keep.scatter_(1, torch.rand(npix, C, generator=gen).topk(k, dim=1).indices, True)
    mag = 2 * torch.randint(0, (maxv + 1) // 2, (npix, C), generator=gen) + 1
    sign = 2 * torch.randint(0, 2, (npix, C), generator=gen) - 1
    return (mag * sign * keep).float()


def make_inputs(case, draw):
    """CPU tensors in the compute dtype: dy [N, Hm, Wm, Cd], src [N, Hs, Ws, Cs]; old [Cd, wtaps, Cs] f32 integers."""
    g, dt = case.gather(), DTYPES[case.dtype]
    gen = torch.Generator().manual_seed(zlib.crc32(f"{case.name}/{draw}".encode()))
    kf, ks = densities(case)[draw]
    kdy, ksrc = (kf, ks) if draw == 0 else (ks, kf)
    mdy, msrc = (FULL_MAX[case.dtype], 1) if draw == 0 else (1, FULL_MAX[case.dtype])
    dy = _operand(g.N * g.Hm * g.Wm, g.Cd, kdy, mdy, gen).view(g.N, g.Hm, g.Wm, g.Cd)
    src = _operand(g.N * g.Hs * g.Ws, g.Cs, ksrc, msrc, gen).view(g.N, g.Hs, g.Ws, g.Cs)
    old = torch.randint(-OLD_MAX, OLD_MAX + 1, (g.Cd, g.wtaps, g.Cs), generator=gen).float()
    assert torch.equal(dy.to(dt).float(), dy) and torch.equal(src.to(dt).float(), src)       # representable as they are
    return {"dy": dy.to(dt), "src": src.to(dt), "old": old}


# ---- the destination and the comparison -------------------------------------------------------------------------------

class Dw:
    """`copies` copies of dW ([Cd, wtaps, Cs] f32 each, back to back) inside one allocation with GUARD sentinel elements on
    either side, every copy filled with `fill` (a number or a [Cd, wtaps, Cs] tensor)."""

    def __init__(self, g, copies=1, fill=0.0, device="cpu"):
        self.n = g.Cd * g.wtaps * g.Cs
        self.buf = torch.full((copies * self.n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=device)
        self.dw = self.buf[GUARD:GUARD + copies * self.n].view(copies, g.Cd, g.wtaps, g.Cs)
        if torch.is_tensor(fill):
            self.dw.copy_(fill.to(device).expand_as(self.dw))
        else:
            self.dw.fill_(fill)

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[-GUARD:] == SENTINEL).all())


def exact(got, want):
    """got (f32) equals want (f64, integer-valued below 2^24) element for element; NaN never equals."""
    return got.shape == want.shape and bool((got.double() == want.to(got.device)).all())


# ---- the case table ---------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Case:
    name: str
    family: str          # "coop" | "halo" | "rows": the kernel family the row is meant to run
    dtype: str           # "f32" | "bf16"
    geom: tuple          # ("conv", N, H, W, Cs, Cd, kh, kw, stride, ph, pw) | ("convT", N, Hs, Ws, Cs, Hd, Wd, Cd, k, stride, pad, class)
    env: tuple           # ((variable, value), ...): AST_WGRAD_PG_MINP / AST_WGRAD_FLUSH_LDS only (read per call)
    plan: tuple          # ast_wgrad_plan's six integers under env, slab_cap = 0
    flush_lds: bool = False      # also run the atomic forms under AST_WGRAD_FLUSH_LDS=1
    note: str = ""

    def gather(self):
        if self.geom[0] == "conv":
            return IC.conv_gather(*self.geom[1:])
        return ops.gathers_transposed(*self.geom[1:-1])[self.geom[-1]]

    @property
    def key(self):
        """The instantiation the row's plan names: (family, dtype, BMW, NCT, PG)."""
        return (self.family, self.dtype) + self.plan[1:4]


class case_env:
    """The row's environment (plus `extra`) for the duration of a block; every weight-gradient knob a row does not set is removed."""
    VARS = ("AST_WGRAD_PG_MINP", "AST_WGRAD_PG", "AST_WGRAD_FLUSH_LDS", "AST_WGRAD_TAP", "AST_WGRAD_TAP_WGS", "AST_WGRAD_ROWS",
            "AST_WGRAD_ROWS_STAGES", "AST_WGRAD_HALO_MAXCD", "AST_WGRAD_WG_TARGET")
    SETTABLE = ("AST_WGRAD_PG_MINP", "AST_WGRAD_FLUSH_LDS")

    def __init__(self, case=None, **extra):
        self.kv = dict(case.env if case is not None else ())
        self.kv.update({k: str(v) for k, v in extra.items()})
        assert set(self.kv) <= set(self.SETTABLE)

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in self.VARS}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        return False


def plan_of(g, dtype, slab_cap=0):
    """ast_wgrad_plan's six integers: (family, BMW, NCT, PG, pixel slices, pixels per slice)."""
    out = (ctypes.c_int32 * 6)()
    rc = _lib.lib().ast_wgrad_plan(g, _lib.dcode(DTYPES[dtype]), slab_cap, ctypes.byref(out))
    assert rc == 0, _lib.lib().ast_last_error()
    return tuple(out)


def slab_caps(slices):
    """The two slab caps a row runs: one below its uncapped slice count (half of it; every row of the table has more than one slice), one above it."""
    return (max(1, (slices + 1) // 2), slices + 2)


COOP_TILES = tuple((b, n) for b, ncts in ((16, (4, 8, 12, 20)), (32, (4, 8, 12, 20)), (64, (4, 8, 12))) for n in ncts)
HALO_TILES = tuple(t for t in COOP_TILES if t[0] <= 32)
# two images (a K tile straddles the image boundary where Hm * Wm is odd); pixel counts that are no multiple of a K trip and leave
# a short last pixel slice: 1134 (last slice 110 pixels), 1178 (154 bf16: three trips / 26 f32: one), 1054 (30: one trip),
# 1102 (78: two trips bf16 / three f32)
_HW = ((21, 27), (19, 31), (17, 31), (19, 29))

# (slices, pixels per slice) of every row's plan at slab_cap = 0
_SLICES = {
    "c16x4-pg1-f32": (9, 128), "c16x8-pg1-f32": (10, 128), "c16x12-pg1-f32": (9, 128), "c16x20-pg1-f32": (9, 128),
    "c32x4-pg1-f32": (9, 128), "c32x8-pg1-f32": (10, 128), "c32x12-pg1-f32": (9, 128), "c32x20-pg1-f32": (9, 128),
    "c64x4-pg1-f32": (9, 128), "c64x8-pg1-f32": (10, 128), "c64x12-pg1-f32": (9, 128), "c16x4-pg2-f32": (9, 128),
    "c16x8-pg2-f32": (9, 128), "c16x12-pg2-f32": (10, 128), "c16x20-pg2-f32": (9, 128), "c32x4-pg2-f32": (9, 128),
    "c32x8-pg2-f32": (9, 128), "c32x12-pg2-f32": (10, 128), "c32x20-pg2-f32": (9, 128), "c64x4-pg2-f32": (9, 128),
    "c64x8-pg2-f32": (9, 128), "c64x12-pg2-f32": (10, 128), "c16x4-pg1-bf16": (5, 256), "c16x8-pg1-bf16": (5, 256),
    "c16x12-pg1-bf16": (5, 256), "c16x20-pg1-bf16": (5, 256), "c32x4-pg1-bf16": (5, 256), "c32x8-pg1-bf16": (5, 256),
    "c32x12-pg1-bf16": (5, 256), "c32x20-pg1-bf16": (5, 256), "c64x4-pg1-bf16": (5, 256), "c64x8-pg1-bf16": (5, 256),
    "c64x12-pg1-bf16": (5, 256), "c16x4-pg2-bf16": (5, 256), "c16x8-pg2-bf16": (5, 256), "c16x12-pg2-bf16": (5, 256),
    "c16x20-pg2-bf16": (5, 256), "c32x4-pg2-bf16": (5, 256), "c32x8-pg2-bf16": (5, 256), "c32x12-pg2-bf16": (5, 256),
    "c32x20-pg2-bf16": (5, 256), "c64x4-pg2-bf16": (5, 256), "c64x8-pg2-bf16": (5, 256), "c64x12-pg2-bf16": (5, 256),
    "h16x4-pg1-f32": (256, 256), "h16x8-pg1-f32": (256, 256), "h16x12-pg1-f32": (256, 273), "h16x20-pg1-f32": (256, 256),
    "h32x4-pg1-f32": (256, 256), "h32x8-pg1-f32": (256, 256), "h32x12-pg1-f32": (256, 256), "h32x20-pg1-f32": (128, 256),
    "h16x4-pg2-f32": (256, 1024), "h16x8-pg2-f32": (256, 1024), "h16x12-pg2-f32": (256, 1024), "h16x20-pg2-f32": (256, 1024),
    "h32x4-pg2-f32": (256, 1024), "h32x8-pg2-f32": (256, 1024), "h32x12-pg2-f32": (256, 1024), "h32x20-pg2-f32": (256, 1024),
    "h16x4-pg1-bf16": (256, 256), "h16x8-pg1-bf16": (256, 256), "h16x12-pg1-bf16": (256, 273), "h16x20-pg1-bf16": (256, 256),
    "h32x4-pg1-bf16": (256, 256), "h32x8-pg1-bf16": (256, 256), "h32x12-pg1-bf16": (256, 256), "h32x20-pg1-bf16": (64, 256),
    "h16x4-pg2-bf16": (256, 1024), "h16x8-pg2-bf16": (256, 1024), "h16x12-pg2-bf16": (256, 1024), "h16x20-pg2-bf16": (256, 1024),
    "h32x4-pg2-bf16": (256, 1024), "h32x8-pg2-bf16": (256, 1024), "h32x12-pg2-bf16": (256, 1024), "h32x20-pg2-bf16": (256, 1024),
    "r-slab-bf16": (3, 192), "r-flush-lds-bf16": (3, 192),
}


def _coop_geom(bmw, nct, hw):
    """The smallest geometry of each cooperative tile, with what else the row is there for."""
    H, W = hw
    s2 = (2 * H - 1, 2 * W - 1)                       # odd source sizes whose stride-2 output is H x W
    if bmw == 16:
        return {4: (("conv", 2 * H * W, 1, 1, 40, 8, 1, 1, 1, 0, 0), "the linear geometry (H = W = 1, one tap); 40 of 64 columns, 8 of 16 rows"),
                8: (("conv", 2, H, W, 8, 8, 3, 3, 1, 1, 1), "72 of 128 columns"),
                12: (("conv", 2, *s2, 16, 16, 3, 3, 2, 1, 1), "stride 2, odd source sizes; 144 of 192 columns"),
                20: (("conv", 2, H, W, 40, 8, 3, 3, 1, 1, 1), "360 columns: gy = 2, the second tile holds 40")}[nct]
    if bmw == 32:
        return {4: (("conv", 2, H, W, 40, 24, 1, 1, 1, 0, 0), "1x1 kernel; 24 of 32 rows"),
                8: (("convT", 2, H, W, 24, 2 * H, 2 * W, 24, 3, 2, 1, 3), "parity class (1, 1) of a stride-2 data gradient: 4 of 9 taps, 96 of 128 columns"),
                12: (("conv", 2, H, W, 16, 24, 3, 3, 1, 1, 1), "144 of 192 columns"),
                20: (("conv", 2, H, W, 24, 24, 3, 3, 1, 1, 1), "216 of 320 columns")}[nct]
    return {4: (("conv", 2, *s2, 40, 40, 1, 1, 2, 0, 0), "1x1 kernel, stride 2; 40 of 64 rows and columns"),
            8: (("conv", 2, H, W, 8, 72, 3, 3, 1, 1, 1), "72 output channels: two row tiles, the second holds 8"),
            12: (("conv", 2, H, W, 24, 40, 3, 3, 1, 1, 1), "216 columns: gy = 2, the second tile holds 24")}[nct]


def _halo_geom(dt, bmw, nct, pg):
    """Halo rows: two (PG = 1: 256 tiles) or eight (PG = 2: 1024 tiles) images of 61 x 250 pixels unless the row says otherwise."""
    N, H, W = (2 if pg == 1 else 8), 61, 250
    cd = {16: 8, 32: 24}[bmw] if nct in (4, 12) else bmw
    bf = dt == "bf16"
    if nct == 4:
        return ("convT", N, H, W + 1, 8, 2 * H, 2 * W + 1, cd, 3, 2, 1, 1), "two-tap parity class (0, 1) of a stride-2 data gradient" + \
            ("; one 16-byte chunk per source pixel" if bf else "")
    if pg == 1:
        if (bmw, nct) == (32, 8):
            return ("conv", N, 2 * H - 1, 2 * W - 1, 8, cd, 3, 3, 2, 1, 1), "stride 2: a 17 x 33 patch"
        if (bmw, nct) == (32, 12):
            return ("conv", N, 2 * H - 1, 2 * W - 1, 16, cd, 3, 3, 2, 1, 1), "stride 2: a 17 x 33 patch, two (bf16) / four (f32) chunks per pixel"
        if (bmw, nct) == (16, 12):
            return ("conv", 13, 17, 97, 16, cd, 3, 3, 1, 1, 1), "273 tiles of 17 x 97 images: 61.3 % of the tiled area is image"
        if (bmw, nct) == (32, 20):
            cs = 112 if bf else 56
            return ("conv", N, H, W, cs, cd, 3, 3, 1, 1, 1), f"{cs} source channels: 2520 chunks in the 10 x 18 patch, the most the loader takes; gy = {4 if bf else 2}"
    cs = {8: 8, 12: 16, 20: 24}[nct]
    return ("conv", N, H, W, cs, cd, 3, 3, 1, 1, 1), ""


def _rows():
    rows = []

    def add(name, family, dtype, geom, env, plan4, flush_lds=False, note=""):
        name = f"{name}-{dtype}"
        rows.append(Case(name, family, dtype, tuple(geom), tuple(sorted(env.items())), tuple(plan4) + tuple(_SLICES.get(name, (0, 0))), flush_lds, note))

    i = 0
    for dt in ("f32", "bf16"):
        for pg in (1, 2):
            for bmw, nct in COOP_TILES:
                geom, note = _coop_geom(bmw, nct, _HW[i % len(_HW)])
                i += 1
                add(f"c{bmw}x{nct}-pg{pg}", "coop", dt, geom, {} if pg == 1 else {"AST_WGRAD_PG_MINP": "1"}, (0, bmw, nct, pg),
                    flush_lds=(bmw, nct) in ((16, 20), (64, 12)), note=note)
    for dt in ("f32", "bf16"):
        for pg in (1, 2):
            for bmw, nct in HALO_TILES:
                geom, note = _halo_geom(dt, bmw, nct, pg)
                add(f"h{bmw}x{nct}-pg{pg}", "halo", dt, geom, {}, (1, bmw, nct, pg), flush_lds=(bmw, nct) in ((16, 4), (32, 20)), note=note)
    # the rows kernel at its default ring depth: the slab form (every row runs it) and the atomic flush through LDS
    add("r-slab", "rows", "bf16", ("conv", 2, 17, 16, 64, 64, 3, 3, 1, 1, 1), {}, (2, 64, 12, 4), note="544 pixels in three slices, the last of 160")
    add("r-flush-lds", "rows", "bf16", ("conv", 3, 9, 19, 128, 64, 3, 3, 1, 1, 1), {"AST_WGRAD_FLUSH_LDS": "1"}, (2, 64, 12, 4),
        note="two source-channel chunks; every atomic form under AST_WGRAD_FLUSH_LDS=1")
    return rows


# Instantiations wgrad_dispatch can name that no default launch reaches, and why the table leaves them alone.
# Keys as Case.key: (family, dtype, BMW, NCT, PG) -- rows kernel: (.., 64, 12, ring stages), tap kernel: (.., 64, 4, 1).
NOT_LAUNCHED = {}
for _dt in ("f32", "bf16"):
    for _b, _n in COOP_TILES:
        if _b == 64:
            for _pg in (1, 2, 4):
                NOT_LAUNCHED[("halo", _dt, _b, _n, _pg)] = "needs AST_WGRAD_HALO_MAXCD > 32, a tuning knob production never sets (measured slower at 64 output channels)"
        else:
            NOT_LAUNCHED[("halo", _dt, _b, _n, 4)] = "needs AST_WGRAD_PG=4, a tuning knob production never sets (the kernel spills at four groups)"
    NOT_LAUNCHED[("tap", _dt, 64, 4, 1)] = "opt-in (AST_WGRAD_TAP=1); test_gpu_ops.py::test_wgrad_tap_kernel is its test"
for _nst in (2, 3):
    NOT_LAUNCHED[("rows", "bf16", 64, 12, _nst)] = "needs AST_WGRAD_ROWS_STAGES, a tuning knob production never sets"

CASES = _rows()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
