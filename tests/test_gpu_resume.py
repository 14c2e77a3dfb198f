"""Resumable training (Trainer.save_state / load_state / state_digest; DESIGN 10, "Resuming").

A run that is saved after step 2 and continued by ANOTHER Trainer of the same process must compute steps 3-4 of the uninterrupted
run: bit for bit in deterministic mode (dropout on: the resumed Trainer has to draw the masks the uninterrupted one drew), within
the run-to-run spread in the default mode.  Graphs captured before a load replay over the loaded weights; files that do not fit
are refused and leave the Trainer untouched; the file still loads through load_checkpoint; and the digest kernel computes
tests/state_digest_ref.py.  Every run is B = 2, S = 2 synthetic batches and at most four steps."""
import contextlib
import ctypes
import gc

import pytest
import torch

import state_digest_ref as ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import ast_amd
    from ast_amd import _lib, checkpoint, config, train

DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


@contextlib.contextmanager
def _compute_dtype(name):
    prev = config.compute_dtype
    ast_amd.set_compute_dtype(DTYPES[name])
    try:
        yield
    finally:
        ast_amd.set_compute_dtype(prev)
        gc.collect()
        torch.cuda.empty_cache()


def _batches():
    return [train.synthetic_batch(2, 2, DEV, seed=100 + i) for i in range(4)]


def _trainer(decoder, det, seed, use_graph=True):
    return train.Trainer(train.TrainConfig(use_graph=use_graph, deterministic=det, decoder=decoder), seed=seed)


def _steps(tr, batches):
    out = []
    for x, labels in batches:
        losses = tr.step(x, labels)
        torch.cuda.synchronize()
        out.append({k: v.detach().clone() for k, v in losses.items()})
    return out


def _state(tr):
    return [t.detach().clone() for t in tr._mutable_state()]


_FILES = {}


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """saved(dtype, decoder, det) -> path of the file a seed-11 Trainer wrote after steps 1-2; made once per combination."""
    root = tmp_path_factory.mktemp("resume")

    def get(dtype, decoder, det):
        key = (dtype, decoder, det)
        if key not in _FILES:
            with _compute_dtype(dtype):
                tr = _trainer(decoder, det, seed=11)
                _steps(tr, _batches()[:2])
                path = str(root / f"{dtype}_{decoder}_{int(det)}.pth")
                tr.save_state(path, note="after step 2")
                _FILES[key] = path
        return _FILES[key]
    yield get
    _FILES.clear()


def _resume(dtype, decoder, det, saved):
    """(losses of steps 3-4, Trainer) of a seed-99 Trainer that loaded the seed-11 run's file."""
    path = saved(dtype, decoder, det)
    tr = _trainer(decoder, det, seed=99)
    tr.load_state(path)
    return _steps(tr, _batches()[2:]), tr


# ---- 1. bit-exact resume, deterministic mode --------------------------------------------------------------------------------
@pytest.mark.parametrize("decoder", ["new", "simple"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_resume_is_bit_exact_in_deterministic_mode(dtype, decoder, saved):
    with _compute_dtype(dtype):
        a = _trainer(decoder, True, seed=11)
        la = _steps(a, _batches())
        lc, c = _resume(dtype, decoder, True, saved)
        assert c.steps == a.steps == 4
        for i, (x, y) in enumerate(zip(la[2:], lc)):
            assert x.keys() == y.keys()
            for k in x:
                assert torch.equal(x[k], y[k]), (dtype, decoder, "step", 3 + i, k, float(x[k]), float(y[k]))
        sa, sc = _state(a), _state(c)
        assert len(sa) == len(sc)
        for i, (p, q) in enumerate(zip(sa, sc)):
            assert torch.equal(p, q), (dtype, decoder, "state tensor", i, tuple(p.shape))
        assert a.state_digest() == c.state_digest()
        # dropout is on (a test without it would say nothing about the dropout stream): the steps differ from a dropout-free run
        assert any(isinstance(m, torch.nn.Dropout) and m.p > 0 for m in a.decoder.modules())


# ---- 2. default (atomic) mode -----------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(a), abs(b), 1e-30)


# Measured on an MI355X (five uninterrupted runs, three resumed ones; maximum relative difference of a loss over all pairs):
#   f32   run to run  rec 1.5e-5  hsic 1.4e-3  adv_g 1.6e-6  adv_d 8.9e-5  total 3.4e-5  nce 0
#         resumed     rec 1.3e-5  hsic 1.6e-3  adv_g 1.8e-6  adv_d 6.1e-5  total 2.4e-5  nce 0
#   bf16  run to run  rec 1.0e-4  hsic 5.2e-3  adv_g 1.6e-5  adv_d 3.4e-4  total 1.5e-4  nce 0
#         resumed     rec 2.0e-4  hsic 4.9e-3  adv_g 8.3e-6  adv_d 4.9e-4  total 2.1e-4  nce 0
# The bound below is taken from the spread of THIS run's two uninterrupted runs, not from these figures.
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_resume_in_default_mode_stays_inside_the_run_to_run_spread(dtype, saved):
    """Resumed steps 3-4 against the uninterrupted run, each loss within 4x the difference of two uninterrupted runs (floor 1e-6).

    The resumed-vs-uninterrupted differences have the distribution of the run-to-run ones (figures above), but single pairs of one
    quantity scatter over two decades (f32 rec at step 4: 1.1e-7 ... 1.5e-5 among ten pairs).  Two fresh Trainers that run the same
    steps back to back are often much closer to each other than either is to any other execution of the same arithmetic (resumed
    runs are as close among themselves: rec <= 1.3e-6), presumably because they replay one graph over the same addresses and the
    atomics then arrive in nearly the same order; the resumed Trainer captures its own graph over other addresses.  In f32 the
    pair this bound comes from was therefore too close in both full runs so far, and the test FAILED there: rec 1.19e-5 against a
    pair at 1.08e-6 (bound 4.3e-6), then adv_d 4.00e-5 against a pair at 5.10e-6 (bound 2.0e-5), while bf16 passed both times.  No
    state is missing from the file: deterministic mode resumes bit for bit from the same code (test above)."""
    with _compute_dtype(dtype):
        l1 = _steps(_trainer("new", False, seed=11), _batches())
        l2 = _steps(_trainer("new", False, seed=11), _batches())
        spread = {k: max(_rel(p[k], q[k]) for p, q in zip(l1, l2)) for k in l1[0]}
        lc, _ = _resume(dtype, "new", False, saved)
        diff = {k: max(_rel(p[k], q[k]) for p, q in zip(l1[2:], lc)) for k in l1[0]}
        for k in spread:
            print(f"default-mode resume [{dtype}] {k}: run-to-run spread {spread[k]:.3e}, resumed vs uninterrupted {diff[k]:.3e}")
        for k in spread:
            assert diff[k] <= max(4.0 * spread[k], 1e-6), (dtype, k, diff[k], spread[k])


# ---- 3. graphs captured before a load -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_graph_captured_before_load_replays_the_loaded_weights(dtype, saved):
    with _compute_dtype(dtype):
        path = saved(dtype, "new", True)
        batches = _batches()
        g = _trainer("new", True, seed=5)
        _steps(g, batches[:2])                                   # captured over seed-5 weights
        graphs = dict(g._graphs)
        before = g.G.flat_p.clone()
        g.load_state(path)
        assert not torch.equal(before, g.G.flat_p)               # every weight came from the file
        assert g._graphs and all(g._graphs[k] is v for k, v in graphs.items()), "load_state dropped the captured graphs"
        e = _trainer("new", True, seed=6, use_graph=False)
        e.load_state(path)
        lg, le = _steps(g, batches[2:3])[0], _steps(e, batches[2:3])[0]
        assert len(g._graphs) == len(graphs)                     # ... and the step replayed one of them
        for k in lg:
            assert torch.equal(lg[k], le[k]), (dtype, k, float(lg[k]), float(le[k]))
        for i, (p, q) in enumerate(zip(_state(g), _state(e))):
            assert torch.equal(p, q), (dtype, "state tensor", i, tuple(p.shape))
        assert g.state_digest() == e.state_digest()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["decoder", "dtype", "deterministic", "digest"])
def test_load_state_refuses_and_leaves_the_trainer_untouched(case, saved, tmp_path):
    with _compute_dtype("f32"):
        if case == "decoder":
            path = saved("f32", "simple", True)
        elif case == "dtype":
            path = saved("bf16", "new", True)
        elif case == "deterministic":
            path = saved("f32", "new", False)
        else:
            ckpt = torch.load(saved("f32", "new", True), map_location="cpu")
            m = ckpt["trainer"]["optim"]["G"]["m"]
            raw = m.view(torch.uint8)
            raw[raw.numel() // 2] ^= 0x10                        # one bit of one byte of Adam's first moment
            path = str(tmp_path / "flipped.pth")
            torch.save(ckpt, path)
        tr = _trainer("new", True, seed=3)
        d0, steps0 = tr.state_digest(), tr.steps
        with pytest.raises(ValueError, match=case):
            tr.load_state(path)
        assert tr.state_digest() == d0 and tr.steps == steps0


# ---- 5. the file is still a reference checkpoint --------------------------------------------------------------------------------
def test_save_state_file_loads_through_load_checkpoint(saved):
    with _compute_dtype("f32"):
        path = saved("f32", "new", True)
        mods = [ast_amd.ContentEncoder().to(DEV), ast_amd.StyleEncoder().to(DEV), ast_amd.Decoder().to(DEV), ast_amd.Discriminator().to(DEV)]
        ckpt = checkpoint.load_checkpoint(path, *mods, map_location=DEV)
        assert tuple(ckpt)[:4] == checkpoint.KEYS and tuple(ckpt)[4] == "trainer" and ckpt["note"] == "after step 2"
        for key, mod in zip(checkpoint.KEYS, mods):
            sd = mod.state_dict()
            assert sd.keys() == ckpt[key].keys()
            assert all(torch.equal(sd[k], ckpt[key][k]) for k in sd), key
        entry = ckpt["trainer"]
        assert entry["version"] == checkpoint.STATE_VERSION and entry["step"] == 2 and entry["sampler"] is None
        assert set(entry["optim"]) == {"G", "D"} and int(entry["optim"]["G"]["step"]) == 2 and int(entry["dropout"]["counter"]) == 2


# ---- 6. the digest kernel against its Python statement --------------------------------------------------------------------------
def _bytes_tensor(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g).to(DEV)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 1023, 65537])
def test_digest_of_one_tensor(n):
    t = _bytes_tensor(n, n)
    assert checkpoint.state_digest([t]) == ref.digest_tensors([t])


def test_digest_of_a_mixed_list_with_an_empty_entry_and_an_offset_view():
    g = torch.Generator().manual_seed(7)
    f = torch.randn(1001, generator=g).to(DEV)
    b = torch.randn(333, generator=g).to(DEV).to(torch.bfloat16)
    i = torch.randint(-2 ** 62, 2 ** 62, (17,), generator=g).to(DEV)
    empty = torch.zeros(0, device=DEV)
    view = torch.randn(5001, generator=g).to(DEV)[1:]            # starts 4 bytes into its allocation
    odd = _bytes_tensor(4099, 9)[1:]                             # ... and one that is not even 4-byte aligned
    assert view.data_ptr() % 16 == 4 and odd.data_ptr() % 4 == 1
    ts = [f, b, empty, i, view, odd]
    assert checkpoint.state_digest(ts) == ref.digest_tensors(ts)
    assert checkpoint.state_digest([]) == ref.digest_bytes([])


def test_digest_properties():
    g = torch.Generator().manual_seed(8)
    a = torch.randn(70000, generator=g).to(DEV)
    b = torch.randn(300, generator=g).to(DEV)
    d = checkpoint.state_digest([a, b])
    assert checkpoint.state_digest([a, b]) == d                  # the same list twice
    assert checkpoint.state_digest([a.clone(), b.clone()]) == d  # other addresses, the same bytes
    s = a.clone()
    s[[123, 45678]] = s[[45678, 123]]                            # two words swapped: a plain sum or xor would not notice
    assert not torch.equal(s, a) and checkpoint.state_digest([s, b]) != d
    assert checkpoint.state_digest([b, a]) != d                  # list order
    for word, bit in ((0, 0), (34567, 31), (69999, 13)):
        f = a.clone()
        f.view(torch.int32)[word] ^= (1 << bit) if bit < 31 else -(1 << 31)
        assert checkpoint.state_digest([f, b]) != d, (word, bit)
    # where the list is cut counts too: the same bytes as one entry and as two
    assert checkpoint.state_digest([a[:100].clone(), a[100:].clone(), b]) != d


def test_digest_argument_errors_launch_nothing():
    lib = _lib.lib()
    out = torch.full((1,), 1234567, dtype=torch.int64, device=DEV)
    t = _bytes_tensor(64, 1)
    ptrs, sizes = (ctypes.c_void_p * 1)(t.data_ptr()), (ctypes.c_longlong * 1)(64)
    neg, null = (ctypes.c_longlong * 1)(-1), (ctypes.c_void_p * 1)(None)
    s = _lib.stream()
    assert lib.ast_state_digest(None, sizes, 1, out.data_ptr(), s) != 0
    assert lib.ast_state_digest(ptrs, None, 1, out.data_ptr(), s) != 0
    assert lib.ast_state_digest(ptrs, sizes, -1, out.data_ptr(), s) != 0
    assert lib.ast_state_digest(ptrs, neg, 1, out.data_ptr(), s) != 0
    assert lib.ast_state_digest(null, sizes, 1, out.data_ptr(), s) != 0
    assert lib.ast_state_digest(ptrs, sizes, 1, None, s) != 0
    assert b"ast_state_digest" in lib.ast_last_error()
    torch.cuda.synchronize()
    assert int(out) == 1234567
    assert lib.ast_state_digest(ptrs, sizes, 1, out.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert (int(out) & ref.MASK) == ref.digest_tensors([t])
