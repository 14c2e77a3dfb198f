"""csrc/weights.hip against the float64 reference of tests/weight_bank_ref.py, through the C ABI alone: hand-built ast_weight_desc_t
tables and a hand-built tile list for the eleven weights of tests/weight_bank_cases.py (no model, no WeightBank), all in ONE
ast_weights_prepare_t / ast_weight_grads_flush_t / ast_weight_grads_flush_det call, for f32 and bf16 packed images; and
ast_weight_grad_unpack, the per-weight form.

Before every call scratch, wf, wb, sigma, inner and every staging replica are filled with NaN, padding included: a value read
before it is written, or left unwritten, shows up.  Every buffer sits between two bands of a sentinel that must survive.

Tolerances are measured on the reference, never on the kernels (weight_bank_ref.bound_rel): per case and quantity,
e_seq = max |sequential-float32 chain - float64| / max |float64|, and the f32 bound is min(2e-4, max(4 e_seq, 16 * 2^-24)) of the
float64 tensor's max-abs; bf16 packed values get 2^-8 |ref| on top (one bf16 ulp).  u, v, sigma and the gradients are f32 in
both modes.  The table tests/test_weight_bank_cpu.py::test_tolerance_table prints (e_seq -> bound):

case                    u                    v                sigma                   wf           sigma_eval              wf_eval                 grad               unpack         unpack_plain
A      3.4e-07 -> 1.4e-06   2.4e-07 -> 9.6e-07   1.6e-07 -> 9.5e-07   1.6e-07 -> 9.5e-07   1.1e-06 -> 4.2e-06   1.0e-06 -> 4.2e-06   5.4e-07 -> 2.2e-06
B      1.7e-07 -> 9.5e-07   1.4e-07 -> 9.5e-07   2.6e-07 -> 1.0e-06   2.8e-07 -> 1.1e-06   2.7e-07 -> 1.1e-06   3.1e-07 -> 1.2e-06   1.6e-07 -> 9.5e-07   9.5e-08 -> 9.5e-07   3.4e-08 -> 9.5e-07
C      1.2e-07 -> 9.5e-07   2.3e-07 -> 9.5e-07   6.7e-08 -> 9.5e-07   1.0e-07 -> 9.5e-07   2.2e-06 -> 8.7e-06   2.1e-06 -> 8.5e-06   2.9e-07 -> 1.2e-06
D      3.8e-07 -> 1.5e-06   2.0e-07 -> 9.5e-07   6.3e-08 -> 9.5e-07   9.0e-08 -> 9.5e-07   5.5e-07 -> 2.2e-06   5.5e-07 -> 2.2e-06   2.6e-07 -> 1.0e-06   2.5e-07 -> 1.0e-06   3.6e-08 -> 9.5e-07
E      1.0e-07 -> 9.5e-07   8.1e-08 -> 9.5e-07   8.4e-08 -> 9.5e-07   9.6e-08 -> 9.5e-07   5.1e-07 -> 2.0e-06   5.5e-07 -> 2.2e-06   3.2e-08 -> 9.5e-07
F      2.0e-07 -> 9.5e-07   2.0e-07 -> 9.5e-07   3.9e-08 -> 9.5e-07   6.2e-08 -> 9.5e-07   1.6e-07 -> 9.5e-07   1.5e-07 -> 9.5e-07   1.3e-07 -> 9.5e-07   9.1e-08 -> 9.5e-07   5.3e-08 -> 9.5e-07
G                                                0.0e+00 -> 9.5e-07   0.0e+00 -> 9.5e-07   0.0e+00 -> 9.5e-07   0.0e+00 -> 9.5e-07
H      5.5e-07 -> 2.2e-06   1.9e-07 -> 9.5e-07   3.4e-08 -> 9.5e-07   5.3e-08 -> 9.5e-07   3.8e-06 -> 1.5e-05   3.8e-06 -> 1.5e-05   3.3e-07 -> 1.3e-06
I      9.0e-07 -> 3.6e-06   3.8e-07 -> 1.5e-06   7.8e-07 -> 3.1e-06   8.0e-07 -> 3.2e-06   9.2e-07 -> 3.7e-06   9.1e-07 -> 3.7e-06   4.7e-08 -> 9.5e-07
J      2.6e-07 -> 1.0e-06   1.2e-07 -> 9.5e-07   3.8e-07 -> 1.5e-06   4.1e-07 -> 1.6e-06   2.9e-07 -> 1.2e-06   2.9e-07 -> 1.2e-06   5.9e-08 -> 9.5e-07
K      2.1e-07 -> 9.5e-07   1.7e-07 -> 9.5e-07   1.5e-08 -> 9.5e-07   3.0e-08 -> 9.5e-07   1.8e-07 -> 9.5e-07   2.1e-07 -> 9.5e-07   2.7e-07 -> 1.1e-06

(G has no spectral norm: its sigma must be exactly 1 and its f32 wf exactly W, whatever the bound says.)"""
import numpy as np
import pytest
import torch

import weight_bank_cases as WC
import weight_bank_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ast_amd import _lib

DEV = "cuda"
GUARD = 64                   # sentinel elements on either side of every buffer (256 bytes of f32: the alignment stays)
SENTINEL = -24576.0          # exact in bf16 and f32
NAN = float("nan")


class _Buf:
    """n elements between two sentinel bands, in one allocation."""

    def __init__(self, n, dtype=torch.float32):
        self.all = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
        self.t = self.all[GUARD:GUARD + n]

    def guards_intact(self):
        return bool((self.all[:GUARD] == SENTINEL).all()) and bool((self.all[-GUARD:] == SENTINEL).all())

    def np(self):
        return self.t.float().cpu().numpy() if self.t.dtype != torch.float32 else self.t.cpu().numpy()


def _t(a):
    """a flat float32 host tensor holding a copy of a (the seeded inputs are read-only arrays)"""
    return torch.from_numpy(np.array(a, np.float32).reshape(-1))


def _bits(a):
    """bit pattern of a float32 array: NaN-filled buffers compare equal to themselves"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class _Table:
    """The device buffers of every case, the training and eval descriptor tables over them, the tile list."""

    def __init__(self, dt):
        self.dt, self.bf = dt, dt == torch.bfloat16
        L = _lib.lib()
        self.b = {}
        train, evald = [], []
        for c in WC.CASES:
            b = {"w": _Buf(c.w_offset + c.numel), "sigma": _Buf(1), "inner": _Buf(1), "wf": _Buf(c.packed, dt), "wb": _Buf(c.packed, dt),
                 "scratch": _Buf(int(L.ast_sn_scratch_floats(c.Co, c.ncols)))}
            if c.has_u:
                b.update(u=_Buf(c.Co), v=_Buf(c.ncols), grad=_Buf(c.w_offset + c.numel), dwp=_Buf(c.replicas * c.packed))
            self.b[c.id] = b
            p = lambda name, off=0: (b[name].t.data_ptr() + 4 * off) if name in b else None
            if c.aligned:
                assert p("w") % 16 == 0
            else:
                assert p("w", c.w_offset) % 16 == 4 and p("grad", c.w_offset) % 16 == 4
            for power_iter, out in ((1, train), (0, evald)):
                out.append(_lib.WeightDesc(w=p("w", c.w_offset), u=p("u"), v=p("v"), sigma=p("sigma"), scratch=p("scratch"), wf=p("wf"), wb=p("wb"),
                                           Co=c.Co, Ci=c.Ci, KK=c.KK, s_co=c.s_co, s_ci=c.s_ci, Cop=c.Cop, Cip=c.Cip, power_iter=power_iter,
                                           dwp=p("dwp"), grad=p("grad", c.w_offset), inner=p("inner"), dwp_from_wb=c.from_wb,
                                           dwp_replicas=max(1, c.replicas)))
        n = len(WC.CASES)
        dev_bytes = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
        self.d_train = dev_bytes(bytes((_lib.WeightDesc * n)(*train)))
        self.d_eval = dev_bytes(bytes((_lib.WeightDesc * n)(*evald)))
        self.d_dtypes = torch.full((n,), _lib.dcode(dt), dtype=torch.int32, device=DEV)
        tl = WC.tile_list()
        self.ntiles = len(tl) // 4
        self.d_tiles = torch.from_numpy(tl).to(DEV)
        self.det_ws = _Buf(self.ntiles)

    def reset(self):
        """The initial state: seeded w, u, v, grad; NaN everywhere the kernels are to write before they read."""
        for c in WC.CASES:
            b, d = self.b[c.id], WC.inputs(c.id)
            b["w"].t.copy_(_t(d["w"]))
            for name in ("sigma", "inner", "wf", "wb", "scratch"):
                b[name].t.fill_(NAN)
            if c.has_u:
                b["u"].t.copy_(_t(d["u"]))
                b["v"].t.copy_(_t(d["v"]))
                b["grad"].t.copy_(_t(d["grad"]))
                b["dwp"].t.fill_(NAN)
        self.det_ws.t.fill_(NAN)
        torch.cuda.synchronize()

    def prepare(self, training):
        d = self.d_train if training else self.d_eval
        _lib.check(_lib.lib().ast_weights_prepare_t(d.data_ptr(), self.d_dtypes.data_ptr(), len(WC.CASES), WC.MAX_CO, WC.MAX_COLS,
                                                    self.d_tiles.data_ptr(), self.ntiles, _lib.stream()), "ast_weights_prepare_t")
        torch.cuda.synchronize()

    def flush(self, det):
        L = _lib.lib()
        if det:
            _lib.check(L.ast_weight_grads_flush_det(self.d_train.data_ptr(), self.d_tiles.data_ptr(), self.ntiles, self.det_ws.t.data_ptr(),
                                                    self.ntiles, _lib.stream()), "ast_weight_grads_flush_det")
        else:
            _lib.check(L.ast_weight_grads_flush_t(self.d_train.data_ptr(), self.d_tiles.data_ptr(), self.ntiles, _lib.stream()),
                       "ast_weight_grads_flush_t")
        torch.cuda.synchronize()

    def stage(self):
        """The replica split into the valid part of every staging buffer, NaN in its padding."""
        for c in WC.CASES:
            if c.has_u:
                st = R.stage(WC.inputs(c.id)["parts"], c.from_wb, c.Cop, c.Cip, pad_value=np.nan)
                self.b[c.id]["dwp"].t.copy_(_t(st))
        torch.cuda.synchronize()

    def get(self, cid, name):
        return self.b[cid][name].np()

    def snapshot(self, names):
        return {(c.id, n): self.get(c.id, n) for c in WC.CASES for n in names if n in self.b[c.id]}

    def assert_guards(self, what):
        for cid, b in self.b.items():
            for name, buf in b.items():
                assert buf.guards_intact(), f"{what}: wrote outside {name} of case {cid}"
        assert self.det_ws.guards_intact(), f"{what}: wrote outside the deterministic workspace"


@pytest.fixture(scope="module", params=["f32", "bf16"])
def table(request):
    return _Table({"f32": torch.float32, "bf16": torch.bfloat16}[request.param])


def _close(what, cid, q, got, ref, bf16=False):
    e, rel = WC.tolerances(cid)[q]
    ok, worst, nbad = R.check(got, ref, rel, bf16)
    print(f"{what} {cid} {q:<10}: max |got - ref| / max|ref| = {worst:.2e}   bound {rel:.2e}{' + 2^-8 |ref|' if bf16 else ''}   (e_seq {e:.1e})")
    return [] if ok else [f"{what}, case {cid}, {q}: {nbad} of {np.size(ref)} outside the bound; worst {worst:.3g} of max|ref|, bound {rel:.3g}"]


def _check_packed(what, t, c, ref_wf, ref_wb, q):
    """wf / wb of case c: valid part within the bound, padding exactly zero, the two images bit-identical transposes."""
    bad = []
    wf = t.get(c.id, "wf").reshape(c.Cop, c.KK, c.Cip)
    wb = t.get(c.id, "wb").reshape(c.Cip, c.KK, c.Cop)
    bad += _close(what, c.id, q, wf[:c.Co, :, :c.Ci], ref_wf[:c.Co, :, :c.Ci], t.bf)
    pad = np.ones((c.Cop, c.KK, c.Cip), bool)
    pad[:c.Co, :, :c.Ci] = False
    if not (_bits(wf[pad]) == 0).all():
        bad.append(f"{what}, case {c.id}: {int((_bits(wf[pad]) != 0).sum())} of {int(pad.sum())} padding elements of wf are not +0")
    if not (_bits(wb.transpose(2, 1, 0)) == _bits(wf)).all():
        bad.append(f"{what}, case {c.id}: wf[co,tap,ci] and wb[ci,tap,co] differ in {int((_bits(wb.transpose(2, 1, 0)) != _bits(wf)).sum())} elements")
    return bad


def test_prepare_training(table):
    t = table
    t.reset()
    t.prepare(True)
    t.assert_guards("training prepare")
    first = t.snapshot(("u", "v", "sigma"))
    bad = []
    for c in WC.CASES:
        ref, d = WC.reference(c.id)[0], WC.inputs(c.id)
        sigma = t.get(c.id, "sigma")
        if c.has_u:
            bad += _close("train", c.id, "u", t.get(c.id, "u"), ref["u"])
            bad += _close("train", c.id, "v", t.get(c.id, "v"), ref["v"])
            bad += _close("train", c.id, "sigma", sigma, np.asarray([ref["sigma"]]))
            dwp = t.get(c.id, "dwp")
            if not (_bits(dwp) == 0).all():
                bad.append(f"case {c.id}: {int((_bits(dwp) != 0).sum())} of {dwp.size} staging elements (all replicas, padding included) are not +0")
        else:
            if sigma[0] != 1.0:
                bad.append(f"case {c.id}: sigma of a weight without spectral norm is {sigma[0]!r}, not 1")
            if not t.bf and not (_bits(t.get(c.id, "wf").reshape(c.Cop, c.KK, c.Cip)[:c.Co, 0, :c.Ci]) == _bits(d["W"][:, :, 0])).all():
                bad.append(f"case {c.id}: the f32 wf of a weight without spectral norm is not W bit for bit")
        if _bits(t.get(c.id, "inner"))[0] != 0:
            bad.append(f"case {c.id}: inner is {t.get(c.id, 'inner')[0]!r} after a training prepare, not +0")
        bad += _check_packed("train", t, c, ref["wf"], ref["wb"], "wf")
        if not (_bits(t.get(c.id, "w")) == _bits(d["w"])).all():
            bad.append(f"case {c.id}: prepare changed w")
    # a second run from the same initial buffers: the same bits
    t.reset()
    t.prepare(True)
    for key, a in t.snapshot(("u", "v", "sigma")).items():
        if not (_bits(a) == _bits(first[key])).all():
            bad.append(f"case {key[0]}: {key[1]} is not bit-reproducible between two runs from the same buffers")
    assert not bad, "\n".join(bad)


def test_prepare_eval(table):
    t = table
    t.reset()
    before = t.snapshot(("u", "v", "dwp", "inner", "w", "grad"))
    t.prepare(False)
    t.assert_guards("eval prepare")
    bad = []
    for key, a in t.snapshot(("u", "v", "dwp", "inner", "w", "grad")).items():
        if not (_bits(a) == _bits(before[key])).all():
            bad.append(f"case {key[0]}: an eval prepare changed {key[1]}")
    for c in WC.CASES:
        ref = WC.reference(c.id)[0]
        sigma = t.get(c.id, "sigma")
        if c.has_u:
            bad += _close("eval", c.id, "sigma_eval", sigma, np.asarray([ref["sigma_eval"]]))
        elif sigma[0] != 1.0:
            bad.append(f"case {c.id}: sigma of a weight without spectral norm is {sigma[0]!r}, not 1")
        bad += _check_packed("eval", t, c, ref["wf_eval"], ref["wb_eval"], "wf_eval")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
def test_flush(table, det):
    t = table
    t.reset()
    t.prepare(True)
    t.stage()
    keep = ("w", "u", "v", "sigma", "wf", "wb")
    before = t.snapshot(keep + ("scratch", "inner"))
    t.flush(det)
    t.assert_guards("flush")
    after = t.snapshot(keep + ("scratch", "inner"))
    bad = []
    for c in WC.CASES:
        names = keep if c.has_u else keep + ("scratch", "inner")          # G: every buffer it has
        for n in names:
            if (c.id, n) in before and not (_bits(after[(c.id, n)]) == _bits(before[(c.id, n)])).all():
                bad.append(f"case {c.id}: the flush changed {n}")
        if not c.has_u:
            continue
        ref, d = WC.reference(c.id)[0], WC.inputs(c.id)
        flat = t.get(c.id, "grad")
        if not np.isfinite(flat).all():
            bad.append(f"case {c.id}: {int((~np.isfinite(flat)).sum())} of {flat.size} gradient elements are not finite (staging padding read?)")
        bad += _close("flush", c.id, "grad", R.logical(flat, c.Co, c.Ci, c.KK, c.s_co, c.s_ci, c.w_offset), ref["grad"])
        if c.w_offset and not (_bits(flat[:c.w_offset]) == _bits(d["grad"][:c.w_offset])).all():
            bad.append(f"case {c.id}: the flush changed the float in front of the offset grad view")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("cid,with_u", [(cid, True) for cid in WC.UNPACK_CASES] + [("B", False)],
                         ids=[f"{cid}-u" for cid in WC.UNPACK_CASES] + ["B-plain"])
def test_weight_grad_unpack(cid, with_u):
    """ast_weight_grad_unpack (PackedWeight.add_weight_grad): one staging copy, a finished (u, v, sigma)."""
    c, d, s = WC.BY_ID[cid], WC.inputs(cid), WC.unpack_inputs(cid)
    q = "unpack" if with_u else "unpack_plain"
    ref = WC.unpack_reference(cid)[0][q]
    def up(a, n):
        b = _Buf(n)
        b.t.copy_(_t(a))
        return b

    bufs = {"dwp": up(R.stage(s["dW1"][None], c.from_wb, c.Cop, c.Cip, pad_value=np.nan), c.packed), "w": up(d["w"], c.w_offset + c.numel),
            "grad": up(d["grad"], c.w_offset + c.numel), "u": up(s["u"], c.Co), "v": up(s["v"], c.ncols), "sigma": up([s["sigma"]], 1),
            "scratch": _Buf(1)}
    bufs["scratch"].t.fill_(NAN)
    p = lambda name, off=0: bufs[name].t.data_ptr() + 4 * off
    on = lambda name: p(name) if with_u else None
    _lib.check(_lib.lib().ast_weight_grad_unpack(p("dwp"), c.from_wb, p("w", c.w_offset), on("u"), on("v"), on("sigma"), p("grad", c.w_offset),
                                                 c.Co, c.Ci, c.KK, c.s_co, c.s_ci, c.Cop, c.Cip, on("scratch"), _lib.stream()),
               "ast_weight_grad_unpack")
    torch.cuda.synchronize()
    bad = []
    for name, b in bufs.items():
        if not b.guards_intact():
            bad.append(f"wrote outside {name}")
    for name, a in (("w", d["w"]), ("u", s["u"]), ("v", s["v"]), ("sigma", [s["sigma"]])):
        if not (_bits(bufs[name].np()) == _bits(a).reshape(-1)).all():
            bad.append(f"the unpack changed {name}")
    flat = bufs["grad"].np()
    if not np.isfinite(flat).all():
        bad.append(f"{int((~np.isfinite(flat)).sum())} gradient elements are not finite (staging padding read?)")
    bad += _close("unpack", cid, q, R.logical(flat, c.Co, c.Ci, c.KK, c.s_co, c.s_ci, c.w_offset), ref)
    assert not bad, "\n".join(bad)
