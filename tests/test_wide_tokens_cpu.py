"""Wide token path (65 .. AST_WIDE_MAX_ROWS token rows) without a GPU: the exports, the scratch sizes and the argument checks of
the ast_*_wide entry points.  Every call here is refused before any launch."""
import re
import os

from ast_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDE = ("ast_skinny_gemm_wide", "ast_skinny_gemm_wide_ex", "ast_linear_wgrad_wide", "ast_bigk_gemm_wide", "ast_bigk_gemm_wide_det",
        "ast_bigk_gemm_wide_det_ws_floats", "ast_bign_dgrad_wide", "ast_bign_dgrad_wide_det", "ast_bign_dgrad_wide_det_ws_floats")
FAKE = 0x10000                                            # a 16-byte aligned non-null pointer; nothing dereferences it


def test_wide_symbols_are_declared_and_exported():
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "ast_hip.h")).read()
    for name in WIDE:
        assert name in _lib.EXPORTS and name in _lib._SIGS
        getattr(lib, name)
        assert re.search(r"\b%s\(" % name, header), name
    assert re.search(r"#define\s+AST_WIDE_MAX_ROWS\s+1024\b", header)
    assert ops.WIDE_MAX_ROWS == 1024 and ops.SKINNY_MAX_ROWS == 64


def test_wide_ws_floats():
    lib = _lib.lib()
    bk, bn = lib.ast_bigk_gemm_wide_det_ws_floats, lib.ast_bign_dgrad_wide_det_ws_floats
    for M in (65, 1024):
        assert int(bk(M, 256, 4096)) == 4 * M * 256                  # one [M][N] slab per 1024-k chunk
        assert int(bk(M, 256, 294462)) == 288 * M * 256
        assert int(bn(M, 1000, 256)) == 2 * M * 256                  # one [M][K] slab per 512-n chunk
        assert int(bn(M, 294462, 256)) == 576 * M * 256
        assert int(bn(M, 2050, 100)) == 5 * M * 100
    for M in (64, 1025, 0, -3):
        assert int(bk(M, 256, 4096)) == -1 and int(bn(M, 1000, 256)) == -1
    assert int(bk(65, 256, 4095)) == -1 and int(bk(65, 256, 0)) == -1 and int(bk(65, 0, 4096)) == -1     # K odd / empty
    assert int(bn(65, 1000, 257)) == -1 and int(bn(65, 1000, 0)) == -1 and int(bn(65, 0, 256)) == -1     # K > 256 / empty


def _refused(rc, name):
    assert rc != 0, name
    assert name.encode() in _lib.lib().ast_last_error(), (name, _lib.lib().ast_last_error())


def test_wide_entries_refuse_bad_arguments():
    lib = _lib.lib()
    f = FAKE
    sk = lambda x=f, w=f, y=f, M=65, N=256, K=256, ldw=256, ldy=256: lib.ast_skinny_gemm_wide(x, w, None, y, M, N, K, ldw, ldy, 0, None)
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(M=64), dict(M=1025), dict(N=0), dict(K=254), dict(K=2048, ldw=2048),
               dict(ldw=258), dict(ldw=128), dict(ldy=128), dict(x=f + 4), dict(w=f + 8)):
        _refused(sk(**kw), "ast_skinny_gemm_wide")
    ex = lambda p, M=65, x=f: lib.ast_skinny_gemm_wide_ex(x, f, None, f, M, 256, 256, 256, 256, 1, None, f, p, 1, None, None)
    for a in ((0.0,), (1.0,), (0.5, 64), (0.5, 1025), (0.5, 65, None)):
        _refused(ex(*a), "ast_skinny_gemm_wide")
    wg = lambda dy=f, x=f, dW=f, M=65, N=40, K=100, lddy=40, ldw=100: lib.ast_linear_wgrad_wide(dy, x, dW, None, M, N, K, lddy, ldw, None)
    for kw in (dict(dy=None), dict(x=None), dict(dW=None), dict(M=64), dict(M=1025), dict(N=0), dict(K=0), dict(lddy=39), dict(ldw=99)):
        _refused(wg(**kw), "ast_linear_wgrad_wide")
    bk = lambda x=f, w=f, y=f, M=65, N=256, K=2050, ldy=256: lib.ast_bigk_gemm_wide(x, w, None, y, M, N, K, ldy, None)
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(M=64), dict(M=1025), dict(N=0), dict(K=2049), dict(K=0), dict(ldy=255),
               dict(x=f + 4)):
        _refused(bk(**kw), "ast_bigk_gemm_wide")
    need = int(lib.ast_bigk_gemm_wide_det_ws_floats(65, 256, 2050))
    assert need == 3 * 65 * 256
    bkd = lambda x=f, w=f, y=f, ws=f, n=need, M=65, K=2050: lib.ast_bigk_gemm_wide_det(x, w, None, y, M, 256, K, ws, n, None)
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(ws=None), dict(n=need - 1), dict(M=64), dict(M=1025), dict(K=2049),
               dict(w=f + 4)):
        _refused(bkd(**kw), "ast_bigk_gemm_wide_det")
    bn = lambda dy=f, w=f, dx=f, M=65, N=2050, K=256, lddy=2050: lib.ast_bign_dgrad_wide(dy, w, dx, M, N, K, lddy, None)
    for kw in (dict(dy=None), dict(w=None), dict(dx=None), dict(M=64), dict(M=1025), dict(N=0), dict(K=257), dict(K=0), dict(lddy=2049)):
        _refused(bn(**kw), "ast_bign_dgrad_wide")
    need = int(lib.ast_bign_dgrad_wide_det_ws_floats(65, 2050, 256))
    assert need == 5 * 65 * 256
    bnd = lambda dy=f, w=f, dx=f, ws=f, n=need, M=65, K=256: lib.ast_bign_dgrad_wide_det(dy, w, dx, M, 2050, K, 2050, ws, n, None)
    for kw in (dict(dy=None), dict(w=None), dict(dx=None), dict(ws=None), dict(n=need - 1), dict(M=64), dict(M=1025), dict(K=257)):
        _refused(bnd(**kw), "ast_bign_dgrad_wide_det")


def test_existing_entries_still_stop_at_64_rows():
    lib = _lib.lib()
    f = FAKE
    assert lib.ast_skinny_gemm(f, f, None, f, 65, 256, 256, 256, 256, 0, None) != 0
    assert lib.ast_linear_wgrad(f, f, f, None, 65, 40, 100, 40, 100, None) != 0
    assert lib.ast_bigk_gemm(f, f, None, f, 65, 256, 2050, 256, None) != 0
    assert lib.ast_bign_dgrad(f, f, f, 65, 2050, 256, 2050, None) != 0
    assert int(lib.ast_bigk_gemm_det_ws_floats(65, 256, 4096)) < 0 and int(lib.ast_bign_dgrad_det_ws_floats(65, 1000, 256)) < 0
