"""Deterministic mode without a GPU: the switch, its refusals, the graph key, and argument checks of the deterministic entry points."""
import ctypes
import os
import subprocess
import sys

import pytest

import ast_amd
from ast_amd import _lib, config, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_switch_env_setter_and_context_manager():
    assert config.deterministic is False                      # default off
    env = dict(os.environ, AST_DETERMINISTIC="1", PYTHONPATH=os.path.join(ROOT, "audio-style-transfer_amd"))
    out = subprocess.run([sys.executable, "-c", "from ast_amd import config; print(config.deterministic)"], env=env,
                         capture_output=True, text=True, check=True).stdout.strip()
    assert out == "True"
    ast_amd.set_deterministic(True)
    try:
        assert config.deterministic is True
        with ast_amd.deterministic(False):
            assert config.deterministic is False
        assert config.deterministic is True
    finally:
        ast_amd.set_deterministic(False)
    with ast_amd.deterministic():
        assert config.deterministic is True
    assert config.deterministic is False


def test_refused_combinations(monkeypatch):
    monkeypatch.setattr(config, "tok_programs", 1)
    with pytest.raises(ValueError):
        ast_amd.set_deterministic(True)
    assert config.deterministic is False
    with pytest.raises(ValueError):
        config.check_deterministic_supported(True)
    monkeypatch.setattr(config, "tok_programs", 0)
    with pytest.raises(ValueError):
        config.check_deterministic_supported(True, world=2)
    config.check_deterministic_supported(True, world=1)
    config.check_deterministic_supported(False, world=2)


def test_graph_key_holds_the_flag():
    import torch

    class _T:                                                 # the attributes _graph_key reads, without building models
        _frontend = _frontend_cqt = None
        _deterministic = train.Trainer._deterministic
    t = _T()
    x = torch.empty(4, 1, 2, 287, 597, device="meta")
    labels = torch.tensor([0, 0, 1, 1])
    keys = set()
    for flag in (None, True, False):
        t.cfg = train.TrainConfig(deterministic=flag)
        keys.add(train.Trainer._graph_key(t, x, labels, False))
    assert len(keys) == 2                                     # None follows the (off) global switch: the same key as False
    t.cfg = train.TrainConfig(deterministic=None)
    with ast_amd.deterministic():
        k_on = train.Trainer._graph_key(t, x, labels, False)
    t.cfg = train.TrainConfig(deterministic=True)
    assert k_on == train.Trainer._graph_key(t, x, labels, False)


def test_deterministic_entry_points_refuse_bad_arguments():
    lib = _lib.lib()
    fake = 0x10000
    big = 65537                                               # AST_DET_MAX_SLOTS + 1
    assert lib.ast_ordered_sum(None, 4, 2, 1, fake, 0, None) != 0 and b"ast_ordered_sum" in lib.ast_last_error()
    assert lib.ast_ordered_sum(fake, 4, 2, 1, None, 0, None) != 0
    assert lib.ast_ordered_sum(fake, -1, 2, 1, fake, 0, None) != 0 and lib.ast_ordered_sum(fake, 4, 0, 1, fake, 0, None) != 0
    assert lib.ast_ordered_sum(fake, 4, big, 1, fake, 0, None) != 0 and lib.ast_ordered_sum(fake, 4, 2, 0, fake, 0, None) != 0
    assert lib.ast_sumsq_det(fake, 64, fake, None, 16, None) != 0 and lib.ast_sumsq_det(fake, -1, fake, fake, 16, None) != 0
    assert lib.ast_sumsq_det(fake, 64, fake, fake, big, None) != 0 and lib.ast_sumsq_det(None, 64, fake, fake, 16, None) != 0
    assert lib.ast_colsum_acc_det(fake, 10, 16, 17, fake, 0, fake, 4, None) != 0          # Creal > C
    assert lib.ast_colsum_acc_det(fake, -1, 16, 16, fake, 0, fake, 4, None) != 0
    assert lib.ast_colsum_acc_det(fake, 10, 16, 16, fake, 0, None, 4, None) != 0
    assert lib.ast_colsum_acc_det(fake, 10, 16, 16, fake, 0, fake, big, None) != 0
    assert lib.ast_chan_stats_det(fake, fake, 2, 100, 12, 0, fake, 4, None) != 0            # C not a multiple of 8
    assert lib.ast_chan_stats_det(fake, fake, -2, 100, 16, 0, fake, 4, None) != 0
    assert lib.ast_chan_stats_det(fake, fake, 2, 100, 16, 0, None, 4, None) != 0
    assert lib.ast_chan_stats_det(fake, fake, 2, 100, 16, 0, fake, 0, None) != 0
    nb = lambda **k: lib.ast_norm_bwd_sums_det(k.get("dy", fake), None, fake, None, fake, 2, 100, k.get("C", 16), 0, 0, None, None, None, None,
                                               k.get("ws", fake), k.get("ns", 4), None)
    assert nb(dy=None) != 0 and nb(C=12) != 0 and nb(ws=None) != 0 and nb(ns=big) != 0
    assert lib.ast_layernorm_bwd_det(fake, fake, fake, fake, fake, fake, fake, fake, 4, 256, 0, None, None) != 0
    assert lib.ast_layernorm_bwd_det(fake, fake, fake, fake, fake, fake, fake, fake, -4, 256, 0, fake, None) != 0
    assert lib.ast_layernorm_bwd_det(fake, fake, fake, fake, fake, fake, fake, fake, 4, 256, 1, fake, None) != 0   # f32 only
    assert lib.ast_add_drop_ln_bwd_det(fake, None, fake, fake, fake, fake, None, None, fake, fake, fake, 4, 256, None, None) != 0
    assert lib.ast_add_drop_ln_bwd_det(fake, None, fake, fake, fake, fake, None, None, fake, fake, fake, big, 256, fake, None) != 0
    f5 = (ctypes.c_float * 5)(1, 1, 1, 1, 1)
    rl = lambda ws=fake, n=10 ** 6, out=fake: lib.ast_recon_loss_total_det(out, fake, 513, 2, 2, 287, 513, f5, f5, ws, n, fake, None, None)
    assert rl(ws=None) != 0 and rl(n=10) != 0 and rl(out=None) != 0                     # scratch smaller than one slot per workgroup
    assert lib.ast_weight_grads_flush_det(fake, fake, 8, fake, 7, None) != 0              # fewer partials than tiles
    assert lib.ast_weight_grads_flush_det(None, fake, 8, fake, 8, None) != 0
    assert lib.ast_weight_grads_flush_det(fake, fake, 8, None, 8, None) != 0
    # the simple decoder's huge linears: slabs must fit the scratch, M <= 64, K <= 256 for the data gradient
    assert int(lib.ast_bigk_gemm_det_ws_floats(65, 256, 4096)) < 0 and int(lib.ast_bign_dgrad_det_ws_floats(8, 1000, 257)) < 0
    need = int(lib.ast_bigk_gemm_det_ws_floats(8, 256, 4096))
    assert need == 4 * 8 * 256
    assert lib.ast_bigk_gemm_det(fake, fake, None, fake, 8, 256, 4096, fake, need - 1, None) != 0
    assert lib.ast_bigk_gemm_det(fake, fake, None, fake, 8, 256, 4095, fake, need, None) != 0          # odd K
    assert lib.ast_bigk_gemm_det(fake, fake, None, fake, 8, 256, 4096, None, need, None) != 0
    need = int(lib.ast_bign_dgrad_det_ws_floats(8, 1000, 256))
    assert lib.ast_bign_dgrad_det(fake, fake, fake, 8, 1000, 256, 1000, fake, need - 1, None) != 0
    assert lib.ast_bign_dgrad_det(fake, fake, None, 8, 1000, 256, 1000, fake, need, None) != 0
    # ast_igemm: the deterministic form refuses the fused statistics (epilogue atomics)
    from ast_amd import ops
    g, _ = ops.gather_direct(2, 8, 8, 16, 16, 3, 1, 1)
    assert lib.ast_igemm(fake, fake, None, fake, g, 0, 4096 | 8, fake, 1 << 20, None) != 0
    assert int(lib.ast_igemm_ws_floats_det(None, 0)) < 0
