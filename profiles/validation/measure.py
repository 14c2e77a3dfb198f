#!/usr/bin/env python3
"""Figures of DESIGN 7 "Validation" (run from the repository root on the GPU: python profiles/validation/measure.py [errors|kernel|evaluate] ...).

errors    ast_recon_loss_total (grad = NULL) against the float64 reference of tests/recon_len_ref.py on the equal-length version of
          every case of the GPU test: worst relative error over five runs per quantity -> the PARENT_ERR table of
          tests/test_gpu_validation.py; and ast_recon_loss_len's own worst figures on the cases as the test runs them.
kernel    ast_recon_loss_len against ast_recon_loss_total (grad = NULL) on the same tensors at B=8, S=4, T=287, Fq=513, equal
          lengths: blocks of 100 back-to-back calls of one entry between two device events, the entries' blocks alternating:
          median, minimum and maximum of the per-call time over the blocks, GB/s of the bytes both read once.  Per-kernel times:
          run this mode under the profiler's kernel trace.
evaluate  Trainer.evaluate replay time per batch at bench.py's default configuration (bf16, B=8, S=2, one graph), both decode
          modes, next to the replayed training step."""
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "audio-style-transfer_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import ast_amd  # noqa: E402
from ast_amd import _lib, train  # noqa: E402
import recon_len_ref as R  # noqa: E402

C5 = (2.0, 0.5, 0.2, 0.3, 0.1)


def parent(out, x, ld, runs=1):
    """ast_recon_loss_total with grad = NULL -> list of (11,) float64"""
    B, S, _, T, F = out.shape
    n = B * S * T * F
    coef = (C5[0] / (2 * n), C5[1] / n, C5[2] / n, C5[3] / (2 * B * (S - 1) * T * F) if S > 1 else 0.0, C5[4] / (2 * B * S * (T - 1) * F) if T > 1 else 0.0)
    inv = (1 / (2 * n), 1 / n, 1 / n, 1 / (2 * B * (S - 1) * T * F) if S > 1 else 0.0, 1 / (2 * B * S * (T - 1) * F) if T > 1 else 0.0)
    c5, i5 = (ctypes.c_float * 5)(*coef), (ctypes.c_float * 5)(*inv)
    ws, res = torch.empty(64 * 5, device="cuda"), torch.empty(11, device="cuda")
    got = []
    for _ in range(runs):
        _lib.check(_lib.lib().ast_recon_loss_total(out.data_ptr(), x.data_ptr(), ld, B, S, T, F, c5, i5, ws.data_ptr(), res.data_ptr(), None, None),
                   "ast_recon_loss_total")
        got.append(res.double().cpu().numpy())
    return got


def batch_ref(out, tgt):
    """the batch value in float64, in res11's layout, from the per-clip reference (equal lengths)"""
    per = R.recon_len_ref(out, tgt, None)
    B, S, _, T, F = out.shape
    ref = np.zeros(11)
    ref[:5] = per[:, :5].sum(axis=0)
    counts = [2 * B * S * T * F, B * S * T * F, B * S * T * F, 2 * B * (S - 1) * T * F, 2 * B * S * (T - 1) * F]
    ref[6:] = [s / c if c else 0.0 for s, c in zip(ref[:5], counts)]
    ref[5] = sum(w * m for w, m in zip(C5, ref[6:]))
    return ref


def new_kernel(o, xd, ld, n):
    B, S, _, T, F = o.shape
    need = int(_lib.lib().ast_recon_loss_len_ws_floats(B, S, T, F))
    ws, res = torch.empty(need, device="cuda"), torch.empty((B, 11), device="cuda")
    c5 = (ctypes.c_float * 5)(*C5)
    nd = None if n is None else torch.tensor(n, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().ast_recon_loss_len(o.data_ptr(), xd.data_ptr(), ld, B, S, T, F, None if nd is None else nd.data_ptr(), c5, ws.data_ptr(), need,
                                             res.data_ptr(), None), "ast_recon_loss_len")
    return res.double().cpu().numpy()


def errors():
    table = {}
    for name, B, S, T, F, ld, n in R.CASES:
        out, x = R.make_case(B, S, T, F, ld, seed=len(name))
        o, xd = torch.from_numpy(out).cuda(), torch.from_numpy(x).cuda()
        ref = batch_ref(out, x[..., :F])
        errs = np.max([np.abs(g - ref) / np.maximum(np.abs(ref), 1e-300) for g in parent(o, xd, ld, runs=5)], axis=0)
        pref = R.recon_len_ref(out, x[..., :F], n)
        e_new = (np.abs(new_kernel(o, xd, ld, n) - pref) / np.maximum(np.abs(pref), 1e-300)).max(axis=0)
        table[name] = {"parent": [float(f"{e:.3e}") for e in errs], "new": [float(f"{e:.3e}") for e in e_new]}
        print(name, json.dumps(table[name]), flush=True)
    return table


def kernel(blocks=12, per_block=100):
    B, S, T, F, ld = 8, 4, 287, 513, 597
    out, x = R.make_case(B, S, T, F, ld, seed=1)
    o, xd = torch.from_numpy(out).cuda(), torch.from_numpy(x).cuda()
    n = B * S * T * F
    c5p = (ctypes.c_float * 5)(*[1.0 / n] * 5)
    c5 = (ctypes.c_float * 5)(*C5)
    lib = _lib.lib()
    need = int(lib.ast_recon_loss_len_ws_floats(B, S, T, F))
    ws, wsp, res, resp = torch.empty(need, device="cuda"), torch.empty(320, device="cuda"), torch.empty((B, 11), device="cuda"), torch.empty(11, device="cuda")
    calls = {"ast_recon_loss_total": lambda: lib.ast_recon_loss_total(o.data_ptr(), xd.data_ptr(), ld, B, S, T, F, c5p, c5p, wsp.data_ptr(), resp.data_ptr(), None, None),
             "ast_recon_loss_len": lambda: lib.ast_recon_loss_len(o.data_ptr(), xd.data_ptr(), ld, B, S, T, F, None, c5, ws.data_ptr(), need, res.data_ptr(), None)}
    # Blocks of per_block calls of ONE entry enqueued back to back between two events, the two entries' blocks alternating: the
    # queue stays full, so a block's time / per_block is the device time of one call (all its launches, no host gap inside).
    times = {k: [] for k in calls}
    for r in range(blocks + 2):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per_block):
                assert f() == 0
            e1.record()
            e1.synchronize()
            if r >= 2:
                times[k].append(e0.elapsed_time(e1) * 1e3 / per_block)
    nbytes = 2 * 4 * B * S * 2 * T * F
    rep = {}
    for k, v in times.items():
        med = statistics.median(v)
        rep[k] = {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "GBps": round(nbytes / med / 1e3, 1)}
    print("kernel", json.dumps(rep), flush=True)
    return rep


def evaluate(rounds=20):
    ast_amd.set_compute_dtype(torch.bfloat16)
    tr = train.Trainer(train.TrainConfig(use_graph=True))
    x, labels = train.synthetic_batch(8, 2, "cuda:0")
    rep = {}

    def timed(f):
        for _ in range(3):
            f()
        ts = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        return {"median_ms": round(statistics.median(ts), 3), "p10_ms": round(ts[len(ts) // 10], 3), "p90_ms": round(ts[9 * len(ts) // 10], 3)}

    rep["step"] = timed(lambda: tr.step(x, labels))
    for decode in train.Trainer.DECODE_MODES:
        rep["evaluate_" + decode] = timed(lambda: tr.evaluate(x, labels, decode=decode))
    print("evaluate", json.dumps(rep), flush=True)
    return rep


if __name__ == "__main__":
    what = sys.argv[1:] or ["errors", "kernel", "evaluate"]
    for w in what:
        {"errors": errors, "kernel": kernel, "evaluate": evaluate}[w]()
