"""Every conv GEMM kernel variant the planner of csrc/igemm.hip can select, each against the float64 reference of the
gather-GEMM contract (tests/igemm_cases.py), in every epilogue form the library accepts for it.

One test case per row of igemm_cases.CASES.  A row first asserts that ast_igemm_plan (and, for the patch kernel,
ast_pconv_variant) gives the plan the row records (the CPU suite pins the same), then launches through ops._igemm:
  plain store with / without bias, ReLU, accumulate, fused BatchNorm statistics (64 slots and ops.stat_slots(Cd) slots),
  per-image statistics, fused BatchNorm-backward sums (with and without the ReLU mask), and the deterministic form twice.
Combinations the library documents as refused (include/ast_hip.h; the argument checks of ast_igemm_bn) must return an
error code and leave dst untouched.

The bound is derived, not measured (igemm_cases.out_bound): |y - ref| <= 2 K 2^-24 A, plus 2^-8 |ref| for bf16 outputs (one
round-to-nearest to 8 significant bits), per element, with A the same contraction over absolute values.  Statistics are compared with float64 sums of the values the
kernel STORED -- epi_store_m / the patch kernel's epilogue add (float)(T)v, i.e. the value after the bf16 rounding --
within 2 n 2^-24 sum|.| for n summed values.  dst is pre-filled with a sentinel (and has sentinel guard bands before and
after it): pixels the launch must not write, e.g. the other parity classes of a stride-2 data gradient, must keep it
bitwise.  Comparisons run on the device in float64; the reference itself is computed on the CPU."""
import pytest
import torch

import igemm_cases as IC

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ast_amd import _lib, config, ops

DEV = "cuda"


class _Dst:
    """A destination tensor inside one allocation with GUARD sentinel elements on either side."""

    def __init__(self, g, dt, fill=None):
        n = g.N * g.Hd * g.Wd * g.Cd
        self.buf = torch.full((n + 2 * IC.GUARD,), IC.SENTINEL, dtype=dt, device=DEV)
        self.y = self.buf[IC.GUARD:IC.GUARD + n].view(g.N, g.Hd, g.Wd, g.Cd)
        if fill is not None:
            self.y.copy_(fill)

    def guards_intact(self):
        return bool((self.buf[:IC.GUARD] == IC.SENTINEL).all()) and bool((self.buf[-IC.GUARD:] == IC.SENTINEL).all())

    def untouched(self):
        return bool((self.buf == IC.SENTINEL).all())


class _Row:
    def __init__(self, case):
        self.case, self.g = case, case.gather()
        self.dt, self.bf = IC.DTYPES[case.dtype], case.dtype == "bf16"
        self.dc = _lib.dcode(self.dt)
        g = self.g
        self.M = g.N * g.Hm * g.Wm
        self.cpu = IC.make_inputs(case)
        self.dev = {k: v.to(DEV) for k, v in self.cpu.items()}
        self.core = IC.gather_contract(self.cpu["src"], self.cpu["wgt"], g)
        self.mask = IC.grid_mask(g).to(DEV)
        self.full = bool(self.mask.all())
        self.split = case.family == "gathered" and case.plan[3] > 1
        self._refs = {}

    def ref(self, bias=True, relu=False, acc=False):
        key = (bias, relu, acc)
        if key not in self._refs:
            c = self.cpu
            r, A = IC.gather_gemm_ref(c["src"], c["wgt"], c["bias"] if bias else None, self.g, old_dst=c["old"] if acc else None, relu=relu,
                                      core=self.core)
            self._refs[key] = (r.to(DEV), A.to(DEV))
        return self._refs[key]

    def launch(self, d, bias=True, **kw):
        v = self.dev
        ops._igemm(v["src"], v["wgt"], v["bias"] if bias else None, d.y, self.g, **kw)
        torch.cuda.synchronize()

    def check_output(self, tag, d, ref, A, untouched=None):
        """d.y within the bound of ref on the grid; bitwise `untouched` (the sentinel unless given) off it and in the guards."""
        y = d.y.double()
        err, bound = (y - ref).abs(), IC.out_bound(ref, A, self.g, self.bf)
        if not self.full:
            err, bound = err[:, self.mask], bound[:, self.mask]
        worst = float((err / bound.clamp(min=1e-300)).max())
        print(f"{self.case.name} {tag}: max |y - ref| / bound = {worst:.3g} (max err {float(err.max()):.3g})")
        nbad = int((~(err <= bound)).sum())                # (a NaN output compares false: it counts as outside)
        assert nbad == 0, f"{self.case.name} {tag}: {nbad} of {err.numel()} outputs outside the bound, worst {worst:.3g} x bound"
        assert d.guards_intact(), f"{self.case.name} {tag}: wrote outside the destination tensor"
        if not self.full:
            off = d.y[:, ~self.mask]
            want = torch.full_like(off, IC.SENTINEL) if untouched is None else untouched[:, ~self.mask]
            assert torch.equal(off, want), f"{self.case.name} {tag}: wrote a destination pixel off the grid"

    def stored(self, d):
        """The values the launch stored, [N, Hm * Wm, Cd] in float64."""
        g = self.g
        return d.y[:, g.doh::g.dsh, g.dow::g.dsw, :][:, :g.Hm, :g.Wm, :].double().reshape(g.N, g.Hm * g.Wm, g.Cd)

    def check_sums(self, tag, got, want, absum, n):
        bound = IC.sum_bound(n, absum)
        err = (got.double() - want).abs()
        worst = float((err / bound.clamp(min=1e-300)).max())
        print(f"{self.case.name} {tag}: max |sum - ref| / bound = {worst:.3g}")
        assert bool((err <= bound).all()), f"{self.case.name} {tag}: fused sums outside the bound, worst {worst:.3g} x bound"

    # ---- forms ---------------------------------------------------------------------------------------------------------
    def plain_relu_accumulate(self):
        for bias in (True, False):
            d = _Dst(self.g, self.dt)
            self.launch(d, bias=bias)
            self.check_output("plain" if bias else "plain, no bias", d, *self.ref(bias=bias))
        d = _Dst(self.g, self.dt)
        self.launch(d, flags=2)
        self.check_output("relu", d, *self.ref(relu=True))
        d = _Dst(self.g, self.dt, fill=self.dev["old"])
        self.launch(d, flags=1)
        self.check_output("accumulate", d, *self.ref(acc=True), untouched=self.dev["old"])
        d = _Dst(self.g, self.dt, fill=self.dev["old"])
        self.launch(d, flags=3)
        self.check_output("accumulate + relu", d, *self.ref(acc=True, relu=True), untouched=self.dev["old"])

    def forward_statistics(self):
        g = self.g
        for slots in sorted({64, ops.stat_slots(g.Cd)}):
            tab = torch.zeros(slots * g.Cd * 2, device=DEV)
            d = _Dst(g, self.dt)
            self.launch(d, stats=tab)
            self.check_output(f"statistics, {slots} slots", d, *self.ref())
            v = self.stored(d).reshape(-1, g.Cd)
            got = tab.view(slots, g.Cd, 2).double().sum(0)
            self.check_sums(f"statistics, {slots} slots: sum", got[:, 0], v.sum(0), v.abs().sum(0), self.M)
            self.check_sums(f"statistics, {slots} slots: sum of squares", got[:, 1], (v * v).sum(0), (v * v).sum(0), self.M)

    def per_image_statistics(self):
        g = self.g
        tab = torch.zeros(g.N * g.Cd * 2, device=DEV)
        d = _Dst(g, self.dt)
        self.launch(d, stats=tab, per_image=True)
        self.check_output("per-image statistics", d, *self.ref())           # image-aligned tiles: another tile layout
        v = self.stored(d)
        got = tab.view(g.N, g.Cd, 2).double()
        self.check_sums("per-image statistics: sum", got[..., 0], v.sum(1), v.abs().sum(1), g.Hm * g.Wm)
        self.check_sums("per-image statistics: sum of squares", got[..., 1], (v * v).sum(1), (v * v).sum(1), g.Hm * g.Wm)

    def backward_sums(self):
        g, v = self.g, self.dev
        pre = IC.bn_pre(v["bn_x"], v["scale"], v["shift"])                   # |pre| > 1e-3 by construction: the mask cannot flip
        for relu, slots in ((True, ops.stat_slots(g.Cd)), (False, 64)):
            link = ops.BNLink()
            link.x, link.scale, link.shift, link.relu, link.slots = v["bn_x"], v["scale"], v["shift"], relu, slots
            link.table = torch.zeros(slots * g.Cd * 3, device=DEV)
            d = _Dst(g, self.dt)
            self.launch(d, bn=link)
            tag = f"backward sums, {'ReLU mask' if relu else 'no mask'}, {slots} slots"
            self.check_output(tag, d, *self.ref())
            sel = lambda t: t[:, g.doh::g.dsh, g.dow::g.dsw, :][:, :g.Hm, :g.Wm, :].double().reshape(-1, g.Cd)
            dz = self.stored(d).reshape(-1, g.Cd)
            if relu:
                dz = dz * (sel(pre) > 0)
            x = sel(v["bn_x"])
            got = link.table.view(slots, g.Cd, 3).double().sum(0)
            self.check_sums(tag + ": sum dz", got[:, 0], dz.sum(0), dz.abs().sum(0), self.M)
            self.check_sums(tag + ": sum dz x", got[:, 1], (dz * x).sum(0), (dz * x).abs().sum(0), self.M)
            assert float(got[:, 2].abs().max()) == 0.0

    def deterministic(self):
        old = config.deterministic
        config.deterministic = True
        try:
            ops._ws_cache.clear()
            a, b = _Dst(self.g, self.dt), _Dst(self.g, self.dt)
            self.launch(a)
            self.launch(b)
        finally:
            config.deterministic = old
            ops._ws_cache.clear()
        self.check_output("deterministic", a, *self.ref())
        assert torch.equal(a.buf, b.buf), f"{self.case.name}: two deterministic launches differ"

    def refused(self, tag, flags, bn=False):
        """The library must return an error code before it launches anything: dst keeps the sentinel."""
        g, v, L = self.g, self.dev, _lib.lib()
        ws = torch.zeros(64 * g.Cd * 3 + (4 * self.M * g.Cd if self.split else 0), device=DEV)      # large enough for whatever the flags ask
        d = _Dst(g, self.dt)
        p = lambda t: t.data_ptr()
        if bn:
            rc = L.ast_igemm_bn(p(v["src"]), p(v["wgt"]), p(v["bias"]), p(d.y), g, self.dc, flags, p(ws), ws.numel(), p(v["bn_x"]), p(v["scale"]),
                                p(v["shift"]), _lib.stream())
        else:
            rc = L.ast_igemm(p(v["src"]), p(v["wgt"]), p(v["bias"]), p(d.y), g, self.dc, flags, p(ws), ws.numel(), _lib.stream())
        torch.cuda.synchronize()
        assert rc != 0, f"{self.case.name}: {tag} (flags {flags}) was accepted"
        assert d.untouched() and float(ws.abs().max()) == 0.0, f"{self.case.name}: {tag} was refused after a launch"


@pytest.mark.parametrize("case", IC.CASES, ids=[c.name for c in IC.CASES])
def test_igemm_variant(case):
    with IC.case_env(case):
        plan, ws = IC.plan_of(case.gather(), case.dtype)
        assert (plan, ws) == (case.plan, case.ws), f"{case.name}: the planner picked {plan} (workspace {ws}), the row is for {case.plan}"
        pc = IC.patch_variant_of(case.gather(), case.dtype)
        assert pc == case.pc, f"{case.name}: the launch would run pconv_kernel<SLB, TM, TN, WALL> = {pc}, the row is for {case.pc}"
        row = _Row(case)
        row.plain_relu_accumulate()
        row.deterministic()
        # the argument checks at the end of ast_igemm_bn: statistics need plain stores and have no deterministic form
        row.refused("statistics with accumulate", 8 | 1)
        row.refused("statistics with ReLU", 8 | 2)
        row.refused("backward sums with ReLU", 16 | 2, bn=True)
        row.refused("deterministic statistics", 4096 | 8)
        row.refused("deterministic backward sums", 4096 | 16, bn=True)
        if row.split:                                 # "Only for plans that do not split K"
            row.refused("statistics on a split-K plan", 8)
            row.refused("backward sums on a split-K plan", 16, bn=True)
            row.refused("per-image statistics on a split-K plan", 8 | 64)
        else:
            row.forward_statistics()
            row.backward_sums()
            if case.family == "direct":               # "gathered and patch kernels only"
                row.refused("per-image statistics on the direct kernel", 8 | 64)
            else:
                row.per_image_statistics()
