"""Every weight-gradient kernel instantiation the dispatcher of csrc/wgrad.hip selects by default, each EXACTLY equal to the
float64 reference of the contract (tests/wgrad_cases.py), through every entry point and flush form.

One test case per row of wgrad_cases.CASES, two draws of integer inputs each (the roles of dy and src swapped).  A row first
asserts that ast_wgrad_plan gives the plan the row records (the CPU suite pins the same), then, per draw:
  1. ast_wgrad into zeros equals the reference; 2. into `old` equals old + reference;
  3. ast_wgrad_rep with 2 and 8 copies: the copies sum to the reference, copies past the plan's slice count stay zero;
  4. ast_wgrad_slab into NaN-filled copies at a cap below and a cap above the uncapped slice count: *slices_out is what the plan
     query reports for the cap, every written copy is finite and integer-valued, the rest still NaN; after ast_slab_sum copy 0
     is the reference and the other copies are bitwise what they were;
  5. (rows marked flush_lds) 1 and 2 again under AST_WGRAD_FLUSH_LDS=1.
There is no tolerance: the inputs are integers whose every partial sum is exact in f32 (wgrad_cases: the exactness condition),
so any order of summation and any number of atomics give the same bits.  dW lives inside one allocation with sentinel guard
bands before the first and after the last copy.  A geometry that lists fewer taps than a weight row has (a parity class)
must leave the other taps' slices of dW bitwise alone in every form.  The reference is computed once per row and draw, on the CPU."""
import ctypes

import pytest
import torch

import wgrad_cases as WC

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ast_amd._lib import check, dcode, lib, ptr, stream

DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Draw:
    def __init__(self, case, draw):
        self.case, self.g, self.tag = case, case.gather(), f"{case.name} draw {draw}"
        self.dc = dcode(WC.DTYPES[case.dtype])
        cpu = WC.make_inputs(case, draw)
        self.ref = WC.wgrad_ref(cpu["dy"], cpu["src"], self.g)[0].to(DEV)
        self.dy, self.src, self.old = (cpu[k].to(DEV) for k in ("dy", "src", "old"))
        self.listed = WC.listed_taps(self.g).to(DEV)
        self.n = self.g.Cd * self.g.wtaps * self.g.Cs

    def dst(self, copies=1, fill=0.0):
        return WC.Dw(self.g, copies, fill, device=DEV)

    def atomic(self, what):
        """Steps 1 and 2."""
        d = self.dst()
        check(lib().ast_wgrad(ptr(self.dy), ptr(self.src), d.dw.data_ptr(), self.g, self.dc, stream()), "ast_wgrad")
        torch.cuda.synchronize()
        assert WC.exact(d.dw[0], self.ref), f"{self.tag} {what}: ast_wgrad into zeros differs from the reference"
        assert d.guards_intact(), f"{self.tag} {what}: wrote outside dW"
        d = self.dst(fill=self.old)
        check(lib().ast_wgrad(ptr(self.dy), ptr(self.src), d.dw.data_ptr(), self.g, self.dc, stream()), "ast_wgrad")
        torch.cuda.synchronize()
        assert WC.exact(d.dw[0], self.old.double() + self.ref), f"{self.tag} {what}: ast_wgrad into old differs from old + reference"
        assert torch.equal(_bits(d.dw[0][:, ~self.listed]), _bits(self.old[:, ~self.listed])), f"{self.tag} {what}: touched the slice of a tap it does not list"
        assert d.guards_intact(), f"{self.tag} {what}: wrote outside dW"

    def replicas(self):
        """Step 3."""
        slices = self.case.plan[4]
        for nrep in (2, 8):
            d = self.dst(copies=nrep)
            check(lib().ast_wgrad_rep(ptr(self.dy), ptr(self.src), d.dw.data_ptr(), self.g, self.dc, nrep, stream()), "ast_wgrad_rep")
            torch.cuda.synchronize()
            assert WC.exact(d.dw.double().sum(0).float(), self.ref), f"{self.tag}: {nrep} replicas do not sum to the reference"
            if slices < nrep:
                assert not bool(d.dw[slices:].any()), f"{self.tag}: a replica past the {slices} pixel slices was written"
            assert d.guards_intact(), f"{self.tag}: {nrep} replicas: wrote outside the copies"

    def slabs(self):
        """Step 4."""
        g, listed = self.g, self.listed
        for cap in WC.slab_caps(self.case.plan[4]):
            want = WC.plan_of(g, self.case.dtype, cap)[4]
            assert 1 <= want <= cap
            d = self.dst(copies=cap, fill=float("nan"))
            sl = ctypes.c_int32(-1)
            check(lib().ast_wgrad_slab(ptr(self.dy), ptr(self.src), d.dw.data_ptr(), g, self.dc, cap, ctypes.byref(sl), stream()), "ast_wgrad_slab")
            torch.cuda.synchronize()
            sl = int(sl.value)
            assert sl == want, f"{self.tag}: ast_wgrad_slab reports {sl} slices at cap {cap}, ast_wgrad_plan {want}"
            w = d.dw[:sl][:, :, listed]
            assert bool(torch.isfinite(w).all()) and bool((w == w.round()).all()), f"{self.tag}: cap {cap}: a written copy is not all integers"
            assert bool(torch.isnan(d.dw[:sl][:, :, ~listed]).all()), f"{self.tag}: cap {cap}: wrote the slice of a tap the geometry does not list"
            assert bool(torch.isnan(d.dw[sl:]).all()), f"{self.tag}: cap {cap}: wrote a copy past the {sl} slices"
            assert WC.exact(w.double().sum(0).float(), self.ref[:, listed]), f"{self.tag}: cap {cap}: the copies do not sum to the reference"
            assert d.guards_intact(), f"{self.tag}: cap {cap}: wrote outside the copies"
            before = d.dw.clone()
            bases, sizes, cnt = (ctypes.c_void_p * 1)(d.dw.data_ptr()), (ctypes.c_int64 * 1)(self.n), (ctypes.c_int32 * 1)(sl)
            check(lib().ast_slab_sum(bases, sizes, cnt, 1, stream()), "ast_slab_sum")
            torch.cuda.synchronize()
            assert WC.exact(d.dw[0][:, listed], self.ref[:, listed]), f"{self.tag}: cap {cap}: copy 0 after ast_slab_sum differs from the reference"
            assert bool(torch.isnan(d.dw[0][:, ~listed]).all())
            assert torch.equal(_bits(d.dw[1:]), _bits(before[1:])), f"{self.tag}: cap {cap}: ast_slab_sum changed a copy other than copy 0"
            assert d.guards_intact(), f"{self.tag}: cap {cap}: ast_slab_sum wrote outside the copies"


@pytest.mark.parametrize("case", WC.CASES, ids=[c.name for c in WC.CASES])
def test_wgrad_variant(case):
    draws = [_Draw(case, i) for i in (0, 1)]
    with WC.case_env(case):
        plan = WC.plan_of(case.gather(), case.dtype)
        assert plan == case.plan, f"{case.name}: the dispatcher would launch {plan}, the row is for {case.plan}"
        for d in draws:
            d.atomic("atomic")
            d.replicas()
            d.slabs()
    if case.flush_lds:
        with WC.case_env(case, AST_WGRAD_FLUSH_LDS=1):
            assert WC.plan_of(case.gather(), case.dtype) == case.plan
            for d in draws:
                d.atomic("atomic through LDS")


# ---- ast_slab_sum alone ---------------------------------------------------------------------------------------------------

SIZES = (4, 1020, 1024, 1028, 16 * 9 * 24)          # floats per copy: below / at / above one workgroup's 1024, and a real dW (16 x 9 taps x 24)
SLABS = (1, 2, 8, 9, 16, 17)                        # the single copy, the tail loop alone, the eight-wide loop exactly, with a tail, twice, twice with a tail


def _slab_sum_launch(recs, seed):
    """recs: [(floats per copy, copies)].  Every record sits between guard bands of its own; copy 0 must become the exact sum of the
    record's copies, every other copy and every guard must stay bitwise what it was."""
    gen = torch.Generator().manual_seed(seed)
    G = WC.GUARD
    offs, total = [], 0
    for n, s in recs:
        offs.append(total + G)
        total += 2 * G + n * s
    buf = torch.full((total,), WC.SENTINEL, dtype=torch.float32)
    for (n, s), o in zip(recs, offs):
        buf[o:o + n * s] = torch.randint(-1000, 1001, (n * s,), generator=gen).float()
    want = buf.double().clone()
    for (n, s), o in zip(recs, offs):
        want[o:o + n] = want[o:o + n * s].view(s, n).sum(0)
    dev = buf.to(DEV)
    k = len(recs)
    bases = (ctypes.c_void_p * k)(*[dev.data_ptr() + 4 * o for o in offs])
    sizes = (ctypes.c_int64 * k)(*[n for n, _ in recs])
    cnt = (ctypes.c_int32 * k)(*[s for _, s in recs])
    check(lib().ast_slab_sum(bases, sizes, cnt, k, stream()), "ast_slab_sum")
    torch.cuda.synchronize()
    got = dev.cpu().double()
    bad = (got != want).nonzero().flatten().tolist()
    assert not bad, f"records {recs}: {len(bad)} elements differ, the first at float {bad[0]} (record starts {offs})"


@pytest.mark.parametrize("nrec", [1, 3, 48])
def test_slab_sum_alone(nrec):
    """ast_slab_sum on integer data: one record of every size with every slab count; three and 48 records of different sizes and
    slab counts in one launch (the kernel finds a workgroup's record by searching first_block)."""
    if nrec == 1:
        for i, n in enumerate(SIZES):
            for j, s in enumerate(SLABS):
                _slab_sum_launch([(n, s)], 100 * i + j)
        return
    for shift in range(3 if nrec == 3 else 1):
        recs = [(SIZES[(r + shift) % len(SIZES)], SLABS[(2 * r + shift) % len(SLABS)]) for r in range(nrec)]
        if nrec == 48:                              # every slab count with every size: 5 and 6 are coprime
            recs = [(SIZES[r % len(SIZES)], SLABS[r % len(SLABS)]) for r in range(nrec)]
        _slab_sum_launch(recs, 7 + shift)
