#!/usr/bin/env python3
"""Drives the host glue of ast_amd/ops.py that the ops-glue refactor touched -- the dropout-bearing ops, both attention Functions,
the scalar losses, the reconstruction losses, the big linears, one token program, two train steps -- on seeded inputs and prints one line per case, to
compare two checkouts that share one libast_hip.so on one MI355X:

    timeout -k 10 600 python profiles/ops_glue/hash_ops.py [--root CHECKOUT] [--trace FILE] > hashes.txt

--root: the checkout whose ast_amd is imported (default: this one; set AST_HIP_LIB to the library both sides use).  A line holds
  calls A->B   ops._DropState.calls before and after the case;
  lib N <hex>  the number of library calls the case made and the SHA-256 (first 16 digits) of their sequence: entry names with every
               non-pointer argument (a pointer counts as null or not; a structure or array as its non-pointer fields), recorded by
               standing in for the loaded library object as _lib._ProfiledLib does.  --trace FILE writes the sequences themselves;
  out <hex>    SHA-256 over all outputs and gradients of the case."""
import ctypes
import hashlib
import os
import sys


def _opt(name):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None


HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.abspath(_opt("--root") or HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-style-transfer_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import ast_amd  # noqa: E402
from ast_amd import _lib, config, layers as AL, ops, train  # noqa: E402

DEV = "cuda"
TRACE = open(_opt("--trace"), "w") if _opt("--trace") else None
_line = [0]


# ---- the recording stand-in for the library -----------------------------------------------------------------------------------------
def _is_ptr(t):
    return t is ctypes.c_void_p or t is ctypes.c_char_p or hasattr(t, "contents") or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def _describe(v, t=None):
    if isinstance(v, ctypes.Structure):
        return "{" + ",".join(f"{n}={_describe(getattr(v, n), ft)}" for n, ft in v._fields_) + "}"
    if isinstance(v, ctypes.Array):
        if _is_ptr(v._type_):
            return "[" + ",".join("p" if e else "0" for e in v) + "]"
        return "[" + ",".join(_describe(e) for e in v) + "]"
    if t is not None and _is_ptr(t):
        return "p" if v else "0"
    if isinstance(v, (int, float)):
        return repr(v)
    return "p" if v is not None else "0"                      # byref() and the like


class Recorder:
    def __init__(self, raw):
        self._raw, self.calls = raw, []

    def __getattr__(self, name):
        fn = getattr(self._raw, name)
        types = getattr(fn, "argtypes", None)
        if name == "ast_last_error" or types is None:
            return fn

        def wrapped(*args):
            self.calls.append(f"{name}({', '.join(_describe(a, t) for a, t in zip(args, types))})")
            return fn(*args)
        return wrapped


REC = Recorder(_lib.lib())
_lib._lib = REC                                              # lib() hands out this object from here on


def case(label, fn, calls=None):
    """fn() -> the tensors of the case (None: a parameter without gradient); calls: what _DropState.calls is set to before it."""
    if calls is not None:
        ops._DropState.calls = calls
    REC.calls, before = [], ops._DropState.calls
    outs = fn()
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in outs:
        if isinstance(t, (int, float)):
            h.update(repr(t).encode())
        else:
            h.update(b"" if t is None else t.detach().float().cpu().contiguous().numpy().tobytes())
    seq = "\n".join(REC.calls)
    print(f"{_line[0]:03d} {label} | calls {before}->{ops._DropState.calls} | lib {len(REC.calls)} "
          f"{hashlib.sha256(seq.encode()).hexdigest()[:16]} | out {h.hexdigest()}", flush=True)
    if TRACE:
        TRACE.write(f"=== {_line[0]:03d} {label}\n{seq}\n")
    _line[0] += 1


def rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def grads(y, g, *leaves):
    y.backward(g)
    return [y] + [t.grad for t in leaves]


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def dropout_ops():
    rows = 24
    x, sub, g = rnd(rows, 256, seed=1), rnd(rows, 256, seed=2), rnd(rows, 256, seed=3)
    torch.manual_seed(5)
    ln = nn.LayerNorm(256).to(DEV)
    l1, l2 = nn.Linear(256, 1024).to(DEV), nn.Linear(1024, 256).to(DEV)
    config.set_compute_dtype(torch.float32)
    bank = AL.WeightBank()
    pw1, pw2 = (bank.add(m.weight, "linear", AL.tok_dtype, bias=m.bias) for m in (l1, l2))
    bank.prepare(True)
    for p in (0.0, 0.1):
        def f32():
            xh = x.clone().requires_grad_(True)
            return grads(ops.dropout(xh, p, True), g, xh)

        def dropout_fn():
            xh = x.clone().requires_grad_(True)
            return grads(ops.DropoutFn.apply(xh, p), g, xh)

        def bf16():
            xh = x.bfloat16().requires_grad_(True)
            return grads(ops.dropout(xh, p, True), g.bfloat16(), xh)

        def adln(with_ln):
            def run():
                for q in ln.parameters():
                    q.grad = None
                xh, sh = x.clone().requires_grad_(True), sub.clone().requires_grad_(True)
                s, y = ops.add_drop_ln(xh, sh, ln if with_ln else None, p, True)
                torch.autograd.backward([s] + ([y] if with_ln else []), [g] + ([g * 0.5] if with_ln else []))
                return [s, y, xh.grad, sh.grad, ln.weight.grad, ln.bias.grad]
            return run

        def ffn():
            for m in (l1, l2):
                m.zero_grad()
            xh = x.clone().requires_grad_(True)
            y = ops.ffn(xh, pw1, pw2, p, True)
            y.backward(g)
            bank._flush()
            return [y, xh.grad, l1.weight.grad, l1.bias.grad, l2.weight.grad, l2.bias.grad]

        case(f"dropout f32 p={p}", f32, 100)
        if p > 0:
            case(f"DropoutFn p={p}", dropout_fn, 110)
        case(f"dropout bf16 (dropout_mask, MulMaskFn) p={p}", bf16, 120)
        case(f"add_drop_ln with LayerNorm p={p}", adln(True), 130)
        case(f"add_drop_ln without LayerNorm p={p}", adln(False), 140)
        case(f"ffn (FFNFn) p={p}", ffn, 150)


def attention():
    B, H, dh = 3, 4, 64
    d = H * dh
    for Lq, Lk in ((5, 5), (16, 16), (17, 33)):
        q, kv, g = rnd(B * Lq, d, seed=10 + Lq), rnd(B * Lk, 2 * d, seed=20 + Lk), rnd(B * Lq, d, seed=30 + Lq)
        key_len = i32([1, max(2, Lk // 2), Lk])
        for causal in (False, True):
            for p in (0.0, 0.3):
                def core():
                    qh, kvh = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
                    return grads(ops.AttnCoreFn.apply(qh, kvh, B, H, Lq, Lk, dh, 0, d, causal, p), g, qh, kvh)

                def masked():
                    qh, kvh = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
                    return grads(ops.MaskedAttnFn.apply(qh, kvh, B, H, Lq, Lk, dh, 0, d, causal, p, key_len, Lk), g, qh, kvh)

                tag = f"Lq={Lq} Lk={Lk} causal={int(causal)} p={p}"
                case(f"AttnCoreFn {tag}", core, 2000)
                case(f"MaskedAttnFn {tag}", masked, 2100)

            def inference():
                with torch.no_grad():
                    return [ops.AttnCoreFn.apply(q, kv, B, H, Lq, Lk, dh, 0, d, causal, 0.0, key_len, Lk)]
            case(f"AttnCoreFn key_len no_grad Lq={Lq} Lk={Lk} causal={int(causal)}", inference, 2200)
        # self-attention on one packed tensor (q and kv share storage: one gradient tensor)
        if Lq == Lk:
            qkv = rnd(B * Lq, 3 * d, seed=40 + Lq)

            def packed(fn, *tail):
                def run():
                    t = qkv.clone().requires_grad_(True)
                    return grads(fn.apply(t, t, B, H, Lq, Lk, dh, d, 2 * d, False, 0.3, *tail), g, t)
                return run
            case(f"AttnCoreFn packed qkv Lq=Lk={Lq} p=0.3", packed(ops.AttnCoreFn), 2300)
            case(f"MaskedAttnFn packed qkv Lq=Lk={Lq} p=0.3", packed(ops.MaskedAttnFn, key_len, Lk), 2400)


def scalar_losses():
    D = 8
    for B in (2, 33):
        s, c = rnd(B, D, seed=50 + B), rnd(B, D, seed=60 + B)
        labels, target = i32([i % 2 for i in range(B)]), i32([(3 * i) % D for i in range(B)])
        g = torch.tensor(0.7, device=DEV)
        fns = (("InfoNCEFn", lambda a, b: ops.InfoNCEFn.apply(a, labels, 0.1), 1), ("MarginFn", lambda a, b: ops.MarginFn.apply(a, 2.0), 1),
               ("HSICFn", lambda a, b: ops.HSICFn.apply(a, b), 2), ("CrossCovFn", lambda a, b: ops.CrossCovFn.apply(a, b), 2),
               ("CrossEntropyFn", lambda a, b: ops.CrossEntropyFn.apply(a, target), 1),
               ("SoftmaxEntropyFn", lambda a, b: ops.SoftmaxEntropyFn.apply(a), 1))
        for name, fn, n in fns:
            def run():
                a, b = s.clone().requires_grad_(True), c.clone().requires_grad_(True)
                return grads(fn(a, b), g, *((a, b)[:n]))
            case(f"{name} B={B} D={D}", run)


def recon_losses():
    shape = (2, 3, 2, 4, 8)
    out, tgt, g = rnd(*shape, seed=70), rnd(*shape, seed=71), torch.tensor(1.3, device=DEV)
    for det in (False, True):
        with ast_amd.deterministic(det):
            def total():
                o = out.clone().requires_grad_(True)
                rec = ast_amd.compute_comprehensive_loss(o, tgt)
                return grads(rec["total_loss"], g, o) + [rec[k] for k in sorted(rec) if k != "total_loss"]

            def ragged(n):
                def run():
                    o = out.clone().requires_grad_(True)
                    loss, parts = ast_amd.ragged_reconstruction_loss(o, tgt, n)
                    return grads(loss, g, o) + [parts[k] for k in sorted(parts)]
                return run
            mode = "deterministic" if det else "default"
            case(f"ReconTotalFn (compute_comprehensive_loss) {mode}", total)
            case(f"ReconLenGradFn (ragged_reconstruction_loss) equal {mode}", ragged(None))
            case(f"ReconLenGradFn (ragged_reconstruction_loss) n=(3,1) {mode}", ragged(i32([3, 1])))


def big_linears():
    BIG = 2050
    torch.manual_seed(23)
    lin_in, lin_out = nn.Linear(BIG, 256).to(DEV), nn.Linear(256, BIG).to(DEV)
    with torch.no_grad():
        lin_in.bias.normal_(0, 0.1)
        lin_out.bias.normal_(0, 0.1)
    for rows, S in ((6, 3), (70, 7)):
        n = i32([1 + (2 * b) % S for b in range(rows // S)])
        x, h = rnd(rows, BIG, seed=80 + rows, scale=0.1), rnd(rows, 256, seed=81 + rows)
        gy_in, gy_out = rnd(rows, 256, seed=82 + rows), rnd(rows, BIG, seed=83 + rows, scale=0.1)
        for det in (False, True):
            with ast_amd.deterministic(det):
                def huge_in(lengths):
                    def run():
                        lin_in.zero_grad()
                        y = ops.BigLinearFn.apply(x, lin_in.weight, lin_in.bias, *((S, lengths) if lengths is not None else ()))
                        return grads(y, gy_in, lin_in.weight, lin_in.bias)
                    return run

                def huge_out():
                    lin_out.zero_grad()
                    hh = h.clone().requires_grad_(True)
                    return grads(ops.BigLinearFn.apply(hh, lin_out.weight, lin_out.bias), gy_out, hh, lin_out.weight, lin_out.bias)

                def huge_out_len(lengths):
                    def run():
                        lin_out.zero_grad()
                        hh = h.clone().requires_grad_(True)
                        y = ops.BigOutLinearLenFn.apply(hh, lin_out.weight, lin_out.bias, S, lengths)
                        return grads(y, gy_out, hh, lin_out.weight, lin_out.bias)
                    return run

                def inference(lengths):
                    def run():
                        with torch.no_grad():
                            return [ops.big_out_linear(h, lin_out.weight, lin_out.bias, S, lengths)]
                    return run
                tag = f"rows={rows} S={S} {'deterministic' if det else 'default'}"
                case(f"BigLinearFn huge input {tag}", huge_in(None))
                case(f"BigLinearFn huge input lengths {tag}", huge_in(n))
                case(f"BigLinearFn huge output {tag}", huge_out)
                case(f"BigOutLinearLenFn {tag}", huge_out_len(None))
                case(f"BigOutLinearLenFn lengths {tag}", huge_out_len(n))
                case(f"big_out_linear {tag}", inference(None))
                case(f"big_out_linear lengths {tag}", inference(n))


def token_programs():
    """The style encoder's TransformerEncoder stack as a token program (config.tok_programs = 1: one kernel per op), dropout 0.1:
    tokprog's seeds come from the same draw (tests/test_gpu_tokprog.py::test_stacks_with_dropout_match_per_operator_path)."""
    from ast_amd import tokprog
    from ast_amd.style_encoder import _module_bank
    from oracle import seeded_params as sp
    config.set_compute_dtype(torch.float32)
    m = ast_amd.StyleEncoder()
    m.load_state_dict(sp.seeded_state_dict(m.state_dict(), tag="style"))
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.1
        if isinstance(mod, nn.MultiheadAttention):
            mod.dropout = 0.1
    m = m.to(DEV).train()
    seq0, g = rnd(8, 3, 256, seed=90), rnd(8, 3, 256, seed=91)

    def run():
        for p in m.parameters():
            p.grad = None
        seq = seq0.clone().requires_grad_(True)
        _module_bank(m).prepare(True)
        out = tokprog.encoder_stack(seq, m._layers, True, 0)
        out.backward(g)
        torch.cuda.synchronize()
        return [out, seq.grad] + [p.grad for _, p in m.named_parameters() if p.grad is not None]
    old = config.tok_programs
    config.tok_programs = 1
    try:
        case("tokprog.encoder_stack (8, 3, 256) p=0.1", run, 3000)
    finally:
        config.tok_programs = old
    tokprog.check_status()


def train_steps():
    x, labels = train.synthetic_batch(2, 2, "cuda:0", seed=3)
    for use_graph in (False, True):
        def run():
            tr = train.Trainer(train.TrainConfig(use_graph=use_graph, dropout=True, deterministic=True), seed=7)
            out = []
            for _ in range(2):
                losses = tr.step(x, labels)
                out += [losses[k] for k in sorted(losses)]
            torch.cuda.synchronize()
            return out + [int(tr.state_digest()), int(tr._drop_calls)]
        case(f"Trainer.step x2 deterministic dropout {'graph' if use_graph else 'eager'}: losses, state_digest, _drop_calls", run, 0)
    config.set_deterministic(False)


if __name__ == "__main__":
    print(f"ast_amd from {os.path.dirname(ast_amd.__file__)}", file=sys.stderr, flush=True)
    dropout_ops()
    attention()
    scalar_losses()
    recon_losses()
    big_linears()
    token_programs()
    train_steps()
