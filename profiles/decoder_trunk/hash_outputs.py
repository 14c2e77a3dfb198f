#!/usr/bin/env python3
"""Runs what the decoder-trunk refactor touched -- both decoders, the two encoders' stacks, StyleTransferSession -- on seeded
parameters and inputs and prints one SHA-256 per call (over all its outputs), to compare two checkouts on one MI355X:

    timeout -k 10 600 python profiles/decoder_trunk/hash_outputs.py > hashes.txt

It calls only what both sides of the refactor have.  A line that a checkout does not reproduce against itself (two runs) is
compared numerically instead: `--dump DIR WORDS` also writes the tensors of the lines whose label contains WORDS to
DIR/<line number>_<output>.npy, for compare_dumps.py.  The last line is the number of graphs the graph sessions hold."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-style-transfer_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ast_amd  # noqa: E402
from ast_amd import SimpleDecoder_TransformerOnly as simple  # noqa: E402
from ast_amd import config, cqt, new_decoder  # noqa: E402
from ast_amd import utilityFunctions as U  # noqa: E402
from ast_amd.infer import StyleTransferSession  # noqa: E402
from oracle import seeded_params as sp  # noqa: E402
from test_ragged_cpu import N_SHORT, short_inputs  # noqa: E402

DEV = "cuda"
DUMP, MATCH = (sys.argv[sys.argv.index("--dump") + 1], sys.argv[sys.argv.index("--dump") + 2]) if "--dump" in sys.argv else (None, "")
DTYPES = (("f32", torch.float32), ("bf16", torch.bfloat16))
_line = [0]


def sha(label, *tensors):
    """one line per call: SHA-256 over all its outputs in order (None: a parameter without gradient)"""
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for j, t in enumerate(tensors):
        a = np.zeros(0, np.float32) if t is None else t.detach().float().cpu().contiguous().numpy()
        h.update(a.tobytes())
        if DUMP and MATCH in label:
            np.save(os.path.join(DUMP, f"{_line[0]:03d}_{j}.npy"), a)
    print(f"{_line[0]:03d} {label}: {len(tensors)} tensors, sha256 {h.hexdigest()}", flush=True)
    _line[0] += 1


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def seeded(tag, ctor, keep_dropout=False):
    m = ctor()
    m.load_state_dict(sp.seeded_state_dict(m.state_dict(), tag=tag))
    if not keep_dropout:
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
            if isinstance(mod, torch.nn.MultiheadAttention):
                mod.dropout = 0.0
    return m.to(DEV).eval()


DECODERS = (("new_decoder", "decoder", new_decoder), ("simple", "simple_decoder", simple))


def decoders_eval():
    _, cls, rows = short_inputs()
    cls, rows, n = cls.to(DEV), rows.to(DEV), i32(N_SHORT)
    for name, tag, mod in DECODERS:
        dec = seeded(tag, mod.Decoder)
        for dname, dt in DTYPES:
            config.set_compute_dtype(dt)
            with torch.no_grad():
                for lname, lengths in (("equal", None), ("lengths", n)):
                    sha(f"{name} {dname} eval forward {lname}", dec(rows, cls, target_length=3, lengths=lengths))
                    for mode in ("recompute", "kv_cache"):
                        dec.decode_mode = mode
                        mem = dec.prepare_memory(rows, cls, lengths=lengths)
                        sha(f"{name} {dname} eval prepare_memory+forward_inference {mode} {lname}", mem,
                            dec.forward_inference(mem, 3, lengths=lengths))
                    dec.decode_mode = "recompute"
        del dec
    config.set_compute_dtype(torch.float32)


def decoders_train():
    config.set_compute_dtype(torch.float32)
    config.set_deterministic(True)
    content, cls = sp.seeded_normal((2, 2, 256), 9100).to(DEV), sp.seeded_normal((2, 256), 9101).to(DEV)
    y = sp.seeded_input(2, 2, seed=9102)[..., :513].contiguous().to(DEV)
    for name, tag, mod in DECODERS:
        dec = seeded(tag, mod.Decoder, keep_dropout=True).train()
        forms = ("y",) + (("y_embeddings",) if mod is new_decoder else ())
        for form in forms:
            for p in dec.parameters():
                p.grad = None
            out = dec(content, cls, y=y) if form == "y" else dec(content, cls, y=y, y_embeddings=dec.encode_target(y))
            loss = mod.compute_comprehensive_loss(out, y)["total_loss"]
            loss.backward()
            sha(f"{name} train {form} output+loss", out, loss)
            sha(f"{name} train {form} every parameter gradient", *[p.grad for p in dec.parameters()])
        del dec
    config.set_deterministic(False)


def sessions():
    rate, targets = 48000, (85760, 36708)                    # tests/test_gpu_resample_len.py: the 2-section clip and a short one
    orig, new = rate // 150, 22050 // 150
    n_in = [t * orig // new for t in targets]
    gen = torch.Generator().manual_seed(77)
    clips = [(0.1 * torch.randn(2, nb, generator=gen)).to(DEV) for nb in n_in]
    cls = sp.seeded_normal((2, 256), 7710).to(DEV)
    graphs = []
    # The f32 session's waveforms and sections differ from run to run in the last bits (kernels that add partial sums with f32
    # atomics in arrival order).  Deterministic mode orders those sums, so the same f32 path also appears in a reproducible form.
    for dname, dt, det in (("f32", torch.float32, False), ("bf16", torch.bfloat16, False), ("f32-deterministic", torch.float32, True)):
        config.set_compute_dtype(dt)
        config.set_deterministic(det)
        enc, dec = seeded("content", ast_amd.ContentEncoder), seeded("decoder", ast_amd.Decoder)
        for use_graph in (False, True):
            sess = StyleTransferSession(enc, dec, use_graph=use_graph)
            tag = f"session {dname} {'graph' if use_graph else 'eager'}"
            for order in ([0, 1], [1, 0]):                   # the second call: clips swapped, so the copy-in path runs
                mono = [torch.mean(cqt.resample(clips[b], rate, 22050), dim=0) for b in order]
                w22, n22 = U.pad_waveforms(mono)
                x, n_sec, _ = U.frontend_sections(w22, n22)
                w48, n48 = U.pad_waveforms([clips[b] for b in order], channels=2)
                sha(f"{tag} {order} call equal", *sess(x, cls))
                sha(f"{tag} {order} call n_sections", *sess(x, cls, n_sections=n_sec))
                sha(f"{tag} {order} transfer n_samples", *sess.transfer(w22, cls, n_samples=n22))
                sha(f"{tag} {order} transfer 48 kHz stereo", *sess.transfer(w48, cls, n_samples=n48, sample_rate=rate))
            if use_graph:
                graphs.append(len(sess._graphs))
    config.set_compute_dtype(torch.float32)
    config.set_deterministic(False)
    return graphs


def encoders():
    clips, _, _ = short_inputs()
    x, n = U.pad_sections([c.to(DEV) for c in clips])
    models = (("style cls", "style", ast_amd.StyleEncoder), ("style mean", "style", lambda: ast_amd.StyleEncoder(use_cls=False)),
              ("content", "content", ast_amd.ContentEncoder))
    for name, tag, ctor in models:
        enc = seeded(tag, ctor)
        for dname, dt in DTYPES:
            config.set_compute_dtype(dt)
            with torch.no_grad():
                for lname, lengths in (("equal", None), ("lengths", n)):
                    out = enc(x, lengths=lengths)
                    sha(f"{name} {dname} {lname}", out[0] if isinstance(out, tuple) else out)
    config.set_compute_dtype(torch.float32)


if __name__ == "__main__":
    if DUMP:
        os.makedirs(DUMP, exist_ok=True)
    decoders_eval()
    encoders()
    graphs = sessions()
    decoders_train()
    print(f"graphs held by the graph sessions (f32, bf16, f32-deterministic): {graphs}", flush=True)
