"""The weights that tests/test_gpu_weight_bank.py puts into ONE descriptor table for csrc/weights.hip, their seeded inputs, their
float64 reference and tolerances (tests/weight_bank_ref.py), and a host restatement of every data-dependent branch predicate of the
kernels -- so tests/test_weight_bank_cpu.py can prove, without a GPU, that each branch is taken by some case and that each vector
path also has a case that falls off it.  Nothing here needs the library or a GPU.

All cases share one prepare / flush call on purpose: the grids are sized by max_co / max_cols over the table, and every smaller
weight relies on the kernels' early exits.

Layouts (include/ast_hip.h, ast_weight_desc_t; layers.WeightBank._build):
  conv    master [co][ci][tap]   s_co = Ci*KK, s_ci = KK      staging [Cop][KK][Cip]  (dwp_from_wb = 0)
  convT   master [ci][co][tap]   s_co = KK,    s_ci = Co*KK   staging [Cip][KK][Cop]  (dwp_from_wb = 1)
  linear  master [co][ci]        s_co = Ci,    s_ci = 1, KK = 1; here without u, staging and grad (the bank's linear weights
          take their gradients through ast_linear_wgrad)
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import numpy as np

import weight_bank_ref as R

TL = 32          # tile edge of pack / flush (channels)
RZ = 32          # row chunks of W^T u
MAX_KK = 9       # taps the LDS tile of pack / flush holds (float[9 * 32 * 33])


@dataclass(frozen=True)
class Case:
    id: str
    kind: str            # "conv" | "convT" | "linear"
    Co: int
    Ci: int
    k: int
    replicas: int        # copies of the gradient staging; 0: no u, no staging, no grad (the linear case)
    w_offset: int = 0    # floats between the start of the w / grad allocations and the master (1: 4 bytes past a 16-byte boundary)
    note: str = ""

    @property
    def has_u(self):
        return self.replicas > 0

    @property
    def KK(self):
        return self.k * self.k

    @property
    def s_co(self):
        return self.KK if self.kind == "convT" else self.Ci * self.KK

    @property
    def s_ci(self):
        return self.Co * self.KK if self.kind == "convT" else self.KK

    @property
    def from_wb(self):
        return 1 if self.kind == "convT" else 0

    @property
    def Cop(self):
        return R.pad8(self.Co)

    @property
    def Cip(self):
        return R.pad8(self.Ci)

    @property
    def ncols(self):
        return self.Ci * self.KK

    @property
    def numel(self):
        return self.Co * self.Ci * self.KK

    @property
    def packed(self):
        return self.Cop * self.KK * self.Cip

    @property
    def aligned(self):
        """w and grad start on a 16-byte boundary (the allocations themselves are at least that aligned)"""
        return self.w_offset % 4 == 0

    def tiles(self):
        """(co0, ci0) in the order WeightBank._build lists them"""
        return [(co0, ci0) for co0 in range(0, self.Cop, TL) for ci0 in range(0, self.Cip, TL)]


CASES = [
    Case("A", "conv", 64, 32, 3, 8, note="all-full tiles, every vector path, the unrolled 8-replica sum"),
    Case("B", "conv", 40, 2, 3, 8, note="partial tiles in both dimensions; ncols = 18: scalar spectral-norm loops; scalar 8-replica sum; "
                                        "rows_per = 2, 20 of 32 chunks used"),
    Case("C", "conv", 33, 64, 1, 3, note="KK = 1; Co no multiple of 4 (last sn_w_v block half empty); 17 chunks; 'other' replica count"),
    Case("D", "convT", 32, 64, 3, 3, note="co_outer false, dwp_from_wb = 1, full tiles, vector master path along co"),
    Case("E", "convT", 2, 8, 3, 1, note="the same layout, partial tiles"),
    Case("F", "conv", 16, 16, 2, 1, note="KK = 4: the run-time-KK bodies (KKC = 0)"),
    Case("G", "linear", 96, 256, 1, 0, note="no u, no dwp, no grad: sigma exactly 1, wf exactly W, untouched by the flush"),
    Case("H", "conv", 32, 32, 3, 8, w_offset=1, note="full tiles, w and grad 4 bytes past a 16-byte boundary: scalar master path"),
    Case("I", "conv", 8, 512, 3, 1, note="ncols = 4608: several column blocks, the longest reduction; rows_per = 1, 8 chunks"),
    Case("J", "conv", 264, 8, 1, 1, note="Co > 256: the strided loops of sn_sigma_kernel; 66 row blocks in sn_w_v"),
    # without K no case sums a SINGLE staging copy on the vector loader of tile_load_dwp, which is the form every large weight of
    # the models takes (WeightBank._build gives replicas to the small ones only)
    Case("K", "conv", 32, 32, 1, 1, note="one full tile, one staging copy: the vector staging loader without replicas"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
UNPACK_CASES = ("B", "D", "F")             # ast_weight_grad_unpack: with u, and B once more with u = NULL

MAX_CO = max(c.Co for c in CASES)
MAX_COLS = max(c.ncols for c in CASES)


def tile_list():
    """{w, co0, ci0, 0} for every 32x32 channel tile of every case (padded extents), flat int32, as WeightBank._build emits it."""
    tl = []
    for wi, c in enumerate(CASES):
        for co0, ci0 in c.tiles():
            tl += [wi, co0, ci0, 0]
    return np.asarray(tl, np.int32)


# ---- the branch predicates of csrc/weights.hip, restated ------------------------------------------------------------------

def sn_chunks(c):
    """(rows_per, chunks that hold rows) of sn_wt_u_kernel / sn_t_sum_kernel"""
    rows_per = (c.Co + RZ - 1) // RZ
    return rows_per, (c.Co + rows_per - 1) // rows_per


def sn_wt_u_vector(c):
    """sn_wt_u_kernel: 16-byte loads along the row (4 columns per thread)"""
    return c.s_ci == c.KK and c.ncols % 4 == 0 and c.s_co % 4 == 0 and c.aligned


def sn_w_v_vector(c, power_iter):
    """sn_w_v_kernel: the row AND the vector are 16-byte aligned; in training the vector is scratch + Co"""
    vec_aligned = c.Co % 4 == 0 if power_iter else True
    return c.s_ci == c.KK and c.ncols % 4 == 0 and c.s_co % 4 == 0 and c.aligned and vec_aligned


def sn_w_v_last_block_partial(c):
    return c.Co % 4 != 0


def sn_sigma_strided(c):
    """sn_sigma_kernel's loops over Co take more than one trip"""
    return c.Co > 256


def kkc(c):
    """the compile-time tap count of the pack / flush bodies: 9, 1, or 0 = run-time"""
    return c.KK if c.KK in (9, 1) else 0


def co_outer(c):
    return c.s_co >= c.s_ci


def tile_is_full(c, co0, ci0):
    return co0 + TL <= c.Co and ci0 + TL <= c.Ci


def master_vec_ok(c):
    inner, outer = min(c.s_co, c.s_ci), max(c.s_co, c.s_ci)
    return inner == c.KK and outer % 4 == 0 and c.aligned


def master_vector(c, co0, ci0):
    """tile_load_master / the master walks of both flush kernels: 16-byte accesses"""
    return kkc(c) > 0 and tile_is_full(c, co0, ci0) and master_vec_ok(c)


def packed_vector(c, co0, ci0):
    """tile_store_packed (8-element stores), the staging zeroing of pack_tile_body and tile_load_dwp (16-byte accesses)"""
    return kkc(c) > 0 and tile_is_full(c, co0, ci0) and c.Cip % 8 == 0 and c.Cop % 8 == 0


def replica_path(c):
    return "none" if c.replicas == 0 else "one" if c.replicas == 1 else "eight" if c.replicas == 8 else "other"


def branches(c):
    """Every branch the case takes, as a set of names (the coverage test's vocabulary)."""
    b = {f"kkc{kkc(c)}", "co_outer" if co_outer(c) else "ci_outer", f"dwp_from_wb{c.from_wb}", f"replicas_{replica_path(c)}",
         "has_u" if c.has_u else "no_u"}
    if c.has_u:
        rows_per, nz = sn_chunks(c)
        b.add("sn_wt_u_vector" if sn_wt_u_vector(c) else "sn_wt_u_scalar")
        for pi in (1, 0):
            b.add(("sn_w_v_vector" if sn_w_v_vector(c, pi) else "sn_w_v_scalar") + ("_train" if pi else "_eval"))
        b.add("chunks_all" if nz == RZ else "chunks_some_empty")
        b.add(f"rows_per_{'1' if rows_per == 1 else 'many'}")
        if (c.ncols // 4 if sn_wt_u_vector(c) else c.ncols) > 256:     # more than one 256-thread column block of sn_wt_u does work
            b.add("sn_column_blocks_many")
        if sn_w_v_last_block_partial(c):
            b.add("sn_w_v_last_block_partial")
        if sn_sigma_strided(c):
            b.add("sn_sigma_strided")
    for co0, ci0 in c.tiles():
        full = tile_is_full(c, co0, ci0)
        b.add("tile_full" if full else "tile_partial")
        b.add("master_vector" if master_vector(c, co0, ci0) else "master_scalar")
        b.add("packed_vector" if packed_vector(c, co0, ci0) else "packed_scalar")
        if full and not master_vector(c, co0, ci0) and kkc(c) > 0:
            b.add("master_scalar_on_full_tile")
        if c.has_u:
            b.add(f"dwp_{'vector' if packed_vector(c, co0, ci0) else 'scalar'}_{replica_path(c)}")
    if c.Cop > c.Co:
        b.add("padding_co")
    if c.Cip > c.Ci:
        b.add("padding_ci")
    return b


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------

def _unit(rng, n):
    x = rng.standard_normal(n)
    return (x / np.linalg.norm(x)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """Float32 host arrays of one case (read-only: shared by every test).
      w, grad : flat masters of w_offset + numel floats (the kernels get the view at w_offset; element 0 of case H is the guard)
      u, v    : random unit vectors (None without u)
      parts   : [replicas][co][ci][tap], random parts that sum to dW = G + 0.5 W up to the rounding of the last one: the rank-one
                term <dW, W/sigma> u v^T is then of the size of dW itself, not a 1 % effect
      W, G0   : the logical (Co, Ci, KK) views of w and grad"""
    c = BY_ID[cid]
    rng = np.random.default_rng(zlib.crc32(("weight-bank-" + cid).encode()))
    d = {}
    W = rng.standard_normal((c.Co, c.Ci, c.KK)).astype(np.float32)
    G0 = rng.standard_normal((c.Co, c.Ci, c.KK)).astype(np.float32)
    guard = rng.standard_normal(c.w_offset + c.numel).astype(np.float32)
    d["w"] = R.scatter(guard, W, c.s_co, c.s_ci, c.w_offset)
    d["grad"] = R.scatter(guard[::-1].copy(), G0, c.s_co, c.s_ci, c.w_offset)
    d["W"], d["G0"] = W, G0
    d["u"] = d["v"] = d["parts"] = None
    if c.has_u:
        d["u"], d["v"] = _unit(rng, c.Co), _unit(rng, c.ncols)
        dW = rng.standard_normal(W.shape) + 0.5 * W.astype(np.float64)
        parts = rng.standard_normal((c.replicas,) + W.shape).astype(np.float32)
        parts[-1] = (dW - parts[:-1].astype(np.float64).sum(axis=0)).astype(np.float32)
        d["parts"] = parts
    for a in d.values():
        if a is not None:
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(cid):
    """(float64 chain, sequential-float32 chain) of the case"""
    c, d = BY_ID[cid], inputs(cid)
    return tuple(R.chain(d["W"], d["u"], d["v"], d["G0"], d["parts"], c.Cop, c.Cip, dt) for dt in (np.float64, np.float32))


@functools.lru_cache(maxsize=None)
def unpack_inputs(cid):
    """ast_weight_grad_unpack takes one staging copy and a finished state: dW1 = the replicas' sum and (u, v, sigma) of the float64
    training prepare, all rounded to float32."""
    d, ref = inputs(cid), reference(cid)[0]
    out = {"dW1": d["parts"].astype(np.float64).sum(axis=0).astype(np.float32), "u": ref["u"].astype(np.float32),
           "v": ref["v"].astype(np.float32), "sigma": np.float32(ref["sigma"])}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def unpack_reference(cid):
    d, s = inputs(cid), unpack_inputs(cid)
    return tuple(R.unpack_chain(d["W"], s["u"], s["v"], s["sigma"], d["G0"], s["dW1"], dt) for dt in (np.float64, np.float32))


@functools.lru_cache(maxsize=None)
def tolerances(cid):
    """{quantity: (e_seq, f32 bound)}, both as fractions of the float64 tensor's max-abs"""
    e = R.e_seq(*reference(cid))
    if cid in UNPACK_CASES:
        e.update(R.e_seq(*unpack_reference(cid)))
    return {q: (v, R.bound_rel(v)) for q, v in e.items()}


def tolerance_table():
    """The table tests/test_weight_bank_cpu.py prints: e_seq -> bound per case and quantity."""
    qs = [q for q in R.QUANTITIES]
    lines = ["case  " + "  ".join(f"{q:>19}" for q in qs)]
    for c in CASES:
        t = tolerances(c.id)
        lines.append(f"{c.id:<4}  " + "  ".join(f"{t[q][0]:8.1e} -> {t[q][1]:7.1e}" if q in t else " " * 19 for q in qs))
    return "\n".join(lines)
