"""Host side of resumable training: the Python statement of the state digest on known vectors, the sampler's state, the layout of
a full-state checkpoint and its refusals, and save_state / load_state over a world of two gloo ranks.  The Trainers here are
stand-ins with a few small CPU modules whose digest is the Python one; the device digest is tested in test_gpu_resume.py."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import state_digest_ref as ref
from ast_amd import checkpoint, config, ops, train
from ast_amd.dataloader import LengthBucketSampler


# ---- the digest's Python statement ------------------------------------------------------------------------------------------
def test_mix64_is_the_splitmix64_finaliser():
    assert ref.mix64(0) == 0xE220A8397B1DCDAF and ref.mix64(1) == 0x910A2DEC89025CC1      # splitmix64's first outputs for seeds 0, 1


@pytest.mark.parametrize("entries, want", [
    ([], 0x5E7CE1322180D00D),
    ([b""], 0x3B7D06304F1822A1),
    ([b"a"], 0x95073C00F84247D5),
    ([b"abc"], 0x41F486E967C77DF2),
    ([b"abcd"], 0x712D1D40199974F2),
    ([b"abcde"], 0x93B77CA7E5F3DFED),
    ([b"abcd", b"", b"efgh"], 0x349D1F9126E347A4),
    ([bytes(range(256)) * 5 + b"\x01"], 0xE6A534E35709BFCE),
])
def test_digest_reference_known_vectors(entries, want):
    assert ref.digest_bytes(entries) == want
    assert ref.digest_bytes_slow(entries) == want


def test_digest_reference_properties():
    g = torch.Generator().manual_seed(0)
    raw = torch.randint(0, 256, (70001,), dtype=torch.uint8, generator=g).numpy().tobytes()
    d = ref.digest_bytes([raw[:999], raw[999:]])
    assert d == ref.digest_bytes_slow([raw[:999], raw[999:]])
    assert d != ref.digest_bytes([raw]) and d != ref.digest_bytes([raw[999:], raw[:999]])
    swapped = raw[4:8] + raw[:4] + raw[8:]
    assert swapped != raw and ref.digest_bytes([swapped]) != ref.digest_bytes([raw])
    flipped = raw[:5000] + bytes([raw[5000] ^ 0x80]) + raw[5001:]
    assert ref.digest_bytes([flipped]) != ref.digest_bytes([raw])
    assert ref.digest_bytes([b"ab"]) != ref.digest_bytes([b"ab\0"])                  # the padding is not part of the bytes
    t = torch.arange(6, dtype=torch.bfloat16)
    assert ref.digest_tensors([t, torch.zeros(0)]) == ref.digest_bytes([ref.tensor_bytes(t), b""])


# ---- sampler ----------------------------------------------------------------------------------------------------------------
def test_sampler_state_continues_the_batch_order():
    lengths = [1000] * 10 + [2000] * 7 + [3000] * 4
    a = LengthBucketSampler(lengths, batch_size=2, seed=5)
    a.set_epoch(3)
    state = a.state_dict()
    assert state == {"epoch": 3, "seed": 5}
    b = LengthBucketSampler(lengths, batch_size=2, seed=0)
    assert list(b) != list(a)
    b.load_state_dict(state)
    for epoch in (3, 4):
        a.set_epoch(epoch)
        b.set_epoch(epoch)
        assert list(a) == list(b)


# ---- stand-in Trainer -------------------------------------------------------------------------------------------------------
def _net():
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.BatchNorm1d(7))


class _CpuTrainer(train.Trainer):
    """A Trainer's state and its save / load code over four small CPU modules (no model, no step)."""

    def __init__(self, rank=0, world=1, seed=0, decoder="new"):
        torch.manual_seed(seed)
        self.cfg = train.TrainConfig(use_graph=False, decoder=decoder)
        self.device, self.rank, self.world = torch.device("cpu"), rank, world
        self._drop_seed, self._drop_counter, self._drop_calls, self.steps, self.progress = -1, None, None, 0, None
        self.style, self.content, self.decoder, self.disc = _net(), _net(), _net(), _net()
        self.G = train.FlatGroup([self.style, self.content, self.decoder], self.device)
        self.D = train.FlatGroup([self.disc], self.device)
        self._graphs, self._hyper_sent = {"key": "graph"}, (1.0,)

    def state_digest(self):
        self._own_counter()
        return ref.digest_tensors(self._mutable_state())

    def train_a_little(self, k):
        """Stand-in for k steps: every kind of state moves, the BatchNorm statistics differently on every rank."""
        g = torch.Generator().manual_seed(100 + k)
        with torch.no_grad():
            for grp in (self.G, self.D):
                for p in grp.params:                     # (the padding between the views stays zero, as Adam leaves it)
                    p.add_(torch.randn(p.shape, generator=g))
                grp.m.copy_(torch.randn(grp.n, generator=g))
                grp.v.copy_(torch.rand(grp.n, generator=g))
                grp.step.fill_(k)
            for m in (self.style, self.content, self.decoder, self.disc):
                m[1].running_mean.fill_(float(k + self.rank))
                m[1].num_batches_tracked.fill_(k)
            self._own_counter().fill_(k)
        self._drop_calls, self.steps = 24, k
        self.set_progress(0.5)
        self.cfg.lr_g = 3e-5


def _good_entry():
    return dict(version=checkpoint.STATE_VERSION, decoder="new", dtype="torch.float32", deterministic=False, world=1,
                n_params={"G": 8, "D": 4}, optim={}, dropout={}, step=0, progress=None, cfg={}, sampler=None, digest=0)


_MINE = dict(decoder="new", dtype="torch.float32", deterministic=False, world=1, n_params={"G": 8, "D": 4})


def test_refusals_name_the_field_on_a_hand_made_entry():
    checkpoint.check_trainer_entry(_good_entry(), **_MINE)
    for field, bad in (("version", 2), ("decoder", "simple"), ("dtype", "torch.bfloat16"), ("deterministic", True), ("world", 2),
                       ("n_params", {"G": 12, "D": 4})):
        with pytest.raises(ValueError, match=f"^{field}:"):
            checkpoint.check_trainer_entry(dict(_good_entry(), **{field: bad}), **_MINE)
    for field in ("decoder", "digest", "optim", "dropout"):
        entry = _good_entry()
        del entry[field]
        with pytest.raises(ValueError, match=f"^{field}:"):
            checkpoint.check_trainer_entry(entry, **_MINE)
    with pytest.raises(ValueError, match="^trainer:"):
        checkpoint.trainer_entry({k: {} for k in checkpoint.KEYS})           # what save_checkpoint writes


def test_full_state_file_layout(tmp_path):
    tr = _CpuTrainer(seed=1)
    tr.train_a_little(3)
    sampler = LengthBucketSampler([100] * 8, batch_size=2, seed=9)
    sampler.set_epoch(6)
    path = str(tmp_path / "full.pth")
    tr.save_state(path, sampler=sampler, note="hello")
    ckpt = torch.load(path, map_location="cpu")
    assert tuple(ckpt) == checkpoint.KEYS + ("trainer", "note")
    for key, mod in zip(checkpoint.KEYS, (tr.content, tr.style, tr.decoder, tr.disc)):
        assert ckpt[key].keys() == mod.state_dict().keys()
    e = ckpt["trainer"]
    assert e["version"] == checkpoint.STATE_VERSION and e["decoder"] == "new" and e["dtype"] == str(config.compute_dtype)
    assert e["deterministic"] is False and e["world"] == 1 and e["n_params"] == {"G": tr.G.n, "D": tr.D.n}
    assert e["step"] == 3 and e["progress"] == 0.5 and e["sampler"] == {"epoch": 6, "seed": 9}
    assert e["dropout"]["calls"] == 24 and int(e["dropout"]["counter"]) == 3 and e["dropout"]["seed"] == 0x5EED
    assert set(e["cfg"]) == set(train.Trainer._STATE_CFG) and e["cfg"]["lr_g"] == 3e-5 and e["cfg"]["use_nce"] is True
    assert e["cfg"]["use_adv"] is False
    assert torch.equal(e["optim"]["G"]["m"], tr.G.m) and int(e["optim"]["D"]["step"]) == 3
    assert e["digest"] == tr.state_digest()
    with pytest.raises(ValueError, match="decoder"):
        tr.save_state(path, decoder="mine")                                  # an extra may not replace a checkpoint key
    # ... and save_checkpoint writes what it always wrote
    tr.save_checkpoint(str(tmp_path / "ref.pth"), note="x")
    assert tuple(torch.load(str(tmp_path / "ref.pth"), map_location="cpu")) == checkpoint.KEYS + ("note",)


def test_load_state_restores_in_place_and_rederives(tmp_path):
    a = _CpuTrainer(seed=1)
    a.train_a_little(3)
    path = str(tmp_path / "full.pth")
    sampler = LengthBucketSampler([100] * 8, batch_size=2, seed=9)
    sampler.set_epoch(6)
    a.save_state(path, sampler=sampler)
    b = _CpuTrainer(seed=2)
    assert b.state_digest() != a.state_digest()
    addrs = [t.data_ptr() for t in b._mutable_state()]
    s2 = LengthBucketSampler([100] * 8, batch_size=2)
    b.load_state(path, sampler=s2)
    assert [t.data_ptr() for t in b._mutable_state()] == addrs               # copied into, never rebound
    assert all(torch.equal(p, q) for p, q in zip(a._mutable_state(), b._mutable_state()))
    assert b.state_digest() == a.state_digest()
    assert all(p.data_ptr() == b.G.flat_p.data_ptr() + 4 * off for p, off in zip(b.style.parameters(), (0, 36)))   # still views
    assert b.steps == 3 and b.progress == 0.5 and b._drop_calls == 24 and b.cfg.lr_g == 3e-5 and b.cfg.use_adv is False
    assert b._hyper_sent is None                                             # the step scalars are pushed again
    assert b._graphs == {}                                                   # these graphs had baked other dropout seeds
    assert b._drop_seed == 0x5EED and ops._DropState.seed == 0x5EED
    assert s2.state_dict() == {"epoch": 6, "seed": 9}
    c = _CpuTrainer(seed=3)
    c._drop_calls = 24
    c.load_state(path)
    assert c._graphs == {"key": "graph"}                                     # same dropout seeds: the graphs stay


def test_load_state_refusals_leave_the_trainer_untouched(tmp_path):
    a = _CpuTrainer(seed=1)
    a.train_a_little(3)
    path = str(tmp_path / "full.pth")
    a.save_state(path)

    def refused(tr, p, field):
        d0, cfg0 = tr.state_digest(), tr.cfg
        with pytest.raises(ValueError, match=f"^{field}:"):
            tr.load_state(p)
        assert tr.state_digest() == d0 and tr.cfg is cfg0 and tr.steps == 0 and tr._graphs == {"key": "graph"}

    refused(_CpuTrainer(seed=2, decoder="simple"), path, "decoder")
    refused(_CpuTrainer(seed=2, world=2), path, "world")
    det = _CpuTrainer(seed=2)
    det.cfg.deterministic = True
    refused(det, path, "deterministic")
    prev = config.compute_dtype
    config.compute_dtype = torch.bfloat16
    try:
        refused(_CpuTrainer(seed=2), path, "dtype")
    finally:
        config.compute_dtype = prev
    ckpt = torch.load(path, map_location="cpu")
    ckpt["trainer"]["optim"]["G"]["m"].view(torch.uint8)[11] ^= 1           # one flipped bit of Adam's first moment
    bad = str(tmp_path / "flipped.pth")
    torch.save(ckpt, bad)
    refused(_CpuTrainer(seed=2), bad, "digest")
    ckpt = torch.load(path, map_location="cpu")
    ckpt["trainer"]["version"] = 99
    torch.save(ckpt, bad)
    refused(_CpuTrainer(seed=2), bad, "version")
    a.save_checkpoint(bad)
    refused(_CpuTrainer(seed=2), bad, "trainer")


# ---- data parallel: rank 0 writes, every rank loads ---------------------------------------------------------------------------
def _dp_worker(rank, world, port, path, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    a = _CpuTrainer(rank, world, seed=1)                 # identical replicas ...
    a.train_a_little(3)                                  # ... whose BatchNorm statistics followed their own shards
    a.save_state(path, writer=rank)
    dist.barrier()
    b = _CpuTrainer(rank, world, seed=50 + rank)
    b.load_state(path)
    ckpt = torch.load(path, map_location="cpu")
    q.put((rank, ckpt["writer"], ckpt["trainer"]["world"], b.state_digest(), a.state_digest(), b.style[1].running_mean.tolist(),
           b._drop_seed, ops._DropState.seed, ckpt["trainer"]["dropout"]["seed"], b.steps))
    dist.barrier()
    dist.destroy_process_group()


def test_save_and_load_state_gloo_world2(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    path = str(tmp_path / "dp.pth")
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, path, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r[0]: r[1:] for r in (q.get(timeout=180) for _ in range(2))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank in (0, 1):
        writer, world, d_loaded, d_saver, mean, seed, global_seed, file_seed, steps = res[rank]
        assert writer == 0 and world == 2 and steps == 3
        assert mean == [3.5] * 7                          # sync_buffers: the mean of rank 0's 3.0 and rank 1's 4.0
        assert d_loaded == d_saver                        # after sync_buffers every rank holds what rank 0 wrote
        assert seed == global_seed == 0x5EED + 1000003 * rank and file_seed == 0x5EED      # per rank, not from the file
    assert res[0][2] == res[1][2]
