"""The shared host glue of ast_amd/ops.py, without a GPU or the library: the one dropout draw (_DropState.draw / counter_on), the
facts that are written down once in the package, the one backward of the scalar losses and of the two attention Functions, and the
messages of the whole-number-of-clips check."""
import glob
import os
import re

import pytest
import torch

import ast_amd
from ast_amd import ops

PKG = os.path.dirname(os.path.abspath(ast_amd.__file__))
LOSSES = ("InfoNCEFn", "MarginFn", "HSICFn", "CrossCovFn", "CrossEntropyFn", "SoftmaxEntropyFn")


@pytest.fixture
def drop_state():
    ds = ops._DropState
    saved = (ds.seed, ds.counter, ds.calls)
    yield ds
    ds.seed, ds.counter, ds.calls = saved


def test_draw_seeds_and_calls(drop_state):
    ds, cpu, n = drop_state, torch.device("cpu"), 5
    for seed, calls in ((0x5EED, 0), (0x5EED + 1000003 * 3, 3000)):
        ds.seed, ds.calls = seed, calls
        got = [ds.draw(cpu)[0] for _ in range(n)]
        assert got == [seed + 7919 * (calls + i) for i in range(1, n + 1)]
        assert ds.calls == calls + n


def test_draw_counter(drop_state):
    ds, cpu, meta = drop_state, torch.device("cpu"), torch.device("meta")
    ds.counter, ds.calls = None, 40
    c = ds.counter_on(cpu)
    assert c is ds.counter and c.dtype == torch.int64 and tuple(c.shape) == (1,) and c.device == cpu and int(c) == 0
    assert ds.calls == 40                                            # the accessor consumes no call
    assert ds.counter_on(cpu) is c and ds.draw(cpu)[1] is c and ds.draw(cpu)[1] is c and ds.counter is c   # created once, reused
    assert ds.calls == 42
    m = ds.counter_on(meta)                                          # another device: replaced
    assert m is not c and m is ds.counter and m.device == meta and ds.calls == 42
    assert ds.draw(meta)[1] is m
    back = ds.draw(cpu)[1]
    assert back is ds.counter and back is not c and back.device == cpu and ds.calls == 44
    given = torch.full((1,), 37, dtype=torch.int64)                  # one assigned from outside (Trainer._drop_scope, the tests) is kept
    ds.counter = given
    assert ds.counter_on(cpu) is given and ds.draw(cpu)[1] is given and int(given) == 37


def _package_lines():
    out = []
    for path in sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True)):
        with open(path) as f:
            out += [(os.path.relpath(path, PKG), line) for line in f]
    assert len({p for p, _ in out}) > 10
    return out


def test_written_once_in_the_package():
    lines = _package_lines()

    def where(pattern):
        return [(p, l.strip()) for p, l in lines if re.search(pattern, l)]

    assert len(where(r"7919")) == 1 and where(r"7919")[0][0] == "ops.py", where(r"7919")
    assert len(where(r"not a whole number of clips")) == 1, where(r"not a whole number of clips")
    # calls (an attribute of the library object followed by its arguments), not the names in the signature table or in docstrings
    for entry in ("ast_linear_wgrad_len", "ast_bign_gemm_len"):
        calls = where(r"\." + entry + r"\(")
        assert len(calls) == 1 and calls[0][0] == "ops.py", calls
    # the dropout counter is created in _DropState.counter_on alone; the other int64[1] tensors of the package are the optimiser's
    # step count, the Trainer's own counter that _drop_scope assigns to _DropState.counter, and the checkpoint digest's output
    made = sorted((p, re.match(r"\s*([\w.]+) = ", l).group(1)) for p, l in where(r"torch\.zeros\(1, dtype=torch\.int64"))
    assert made == [("checkpoint.py", "out"), ("ops.py", "cls.counter"), ("train.py", "self._drop_counter"), ("train.py", "self.step")]
    assert not where(r"_DropState\.counter = torch") and not where(r"_DropState\.calls \+= ")
    assert len(where(r"\.calls \+= 1")) == 1


def test_one_backward():
    """The six losses are declarations of ops._scalar_loss and ReconTotalFn / ReconLenGradFn keep their forwards: the backward of
    all eight is the one function ops._scaled_grads.  AttnCoreFn.backward and MaskedAttnFn.backward are the one function
    ops._attn_train_bwd, and both forwards that have a backward go through ops._attn_train_fwd."""
    for name in LOSSES + ("ReconTotalFn", "ReconLenGradFn"):
        fn = getattr(ops, name)
        assert issubclass(fn, torch.autograd.Function) and fn.__name__ == name and fn.__module__ == "ast_amd.ops"
        assert fn.backward is ops._scaled_grads, name
    forwards = [getattr(ops, name).forward for name in LOSSES]
    assert len({f.__code__ for f in forwards}) == 1 and len(set(forwards)) == 6       # one body, six closures
    assert ops.AttnCoreFn.backward is ops.MaskedAttnFn.backward is ops._attn_train_bwd
    for fn in (ops.AttnCoreFn, ops.MaskedAttnFn):
        assert "_attn_train_fwd" in fn.forward.__code__.co_names
    assert "ast_attn_fwd_len" not in ops._attn_train_fwd.__code__.co_consts           # the inference entry stays AttnCoreFn's own


def test_scaled_grads_counts():
    """One gradient per saved tensor, then ctx.n_rest times None (no library: _scaled is stubbed for the length of the test)."""
    class Ctx:
        saved_tensors, n_rest = (torch.ones(2), torch.ones(3)), 4
    real = ops._scaled
    ops._scaled = lambda d, g: d * g
    try:
        out = ops._scaled_grads(Ctx, torch.tensor(2.0), None, None)
    finally:
        ops._scaled = real
    assert len(out) == 6 and out[2:] == (None,) * 4
    assert torch.equal(out[0], torch.full((2,), 2.0)) and torch.equal(out[1], torch.full((3,), 2.0))


@pytest.mark.parametrize("who", ["BigLinearFn", "BigOutLinearLenFn", "big_out_linear"])
def test_clip_count_messages_rows(who):
    assert ops._whole_clips(who, 6, 3) == 2 and ops._whole_clips(who, 6, 1) == 6
    with pytest.raises(ValueError) as e:
        ops._whole_clips(who, 10, 3)
    assert str(e.value) == f"{who}: 10 rows are not a whole number of clips of 3 sections"
    with pytest.raises(ValueError) as e:
        ops._whole_clips(who, 6, 0)
    assert str(e.value) == f"{who}: 6 rows are not a whole number of clips of 0 sections"


@pytest.mark.parametrize("who", ["BatchNormActLenFn", "BilinearToNCHWLenFn", "nchw_to_nhwc_len"])
def test_clip_count_messages_images(who):
    """_check_image_lengths, the fourth site: the helper's message for images, reached through it."""
    n = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError) as e:
        ops._check_image_lengths(who, 10, n, 3)
    assert str(e.value) == f"{who}: 10 images are not a whole number of clips of S = 3 sections"
    with pytest.raises(ValueError) as e:
        ops._check_image_lengths(who, 6, n, 0)
    assert str(e.value) == f"{who}: 6 images are not a whole number of clips of S = 0 sections"
    with pytest.raises(ValueError) as e:
        ops._check_image_lengths(who, 6, None, 3)
    assert str(e.value) == f"{who}: n_sections must be an int32 device tensor of shape (2,), got None"


def test_clip_count_through_the_callers():
    """The three row sites raise the helper's message under their own names (no GPU: the check comes before any pointer is taken)."""
    x, w = torch.zeros(10, 8), torch.zeros(4, 8)
    n = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="^BigLinearFn: 10 rows are not a whole number of clips of 3 sections$"):
        ops.BigLinearFn.apply(x, w, None, 3, n)
    with pytest.raises(ValueError, match="^BigLinearFn: 10 rows are not a whole number of clips of None sections$"):
        ops.BigLinearFn.apply(x, w, None, None, n)
    with pytest.raises(ValueError, match="^BigOutLinearLenFn: 10 rows are not a whole number of clips of 3 sections$"):
        ops.BigOutLinearLenFn.apply(torch.zeros(10, 4), torch.zeros(8, 4), None, 3, None)
    with torch.no_grad(), pytest.raises(ValueError, match="^big_out_linear: 10 rows are not a whole number of clips of 3 sections$"):
        ops.big_out_linear(torch.zeros(10, 4), torch.zeros(8, 4), None, 3)
    with pytest.raises(RuntimeError) as e:
        ops.BigOutLinearLenFn.apply(torch.zeros(1025, 4), torch.zeros(8, 4), None, 1, None)
    assert str(e.value) == "BigOutLinearLenFn: 1025 token rows > 1024 (the cap of the wide token path, AST_WIDE_MAX_ROWS)"
    with torch.no_grad(), pytest.raises(RuntimeError) as e:
        ops.big_out_linear(torch.zeros(4097, 4), torch.zeros(8, 4), None, 1)
    assert str(e.value) == "big_out_linear: 4097 rows > 4096 (AST_BIGN_MAX_ROWS)"
    with pytest.raises(RuntimeError) as e:
        ops.big_out_linear(torch.zeros(4, 4, requires_grad=True), torch.zeros(8, 4), None, 2)
    assert str(e.value) == ("the length-masked output linear (big_out_linear) is inference only: it has no backward; "
                            "run it under torch.no_grad()")
