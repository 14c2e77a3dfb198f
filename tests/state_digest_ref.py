"""The state digest (ast_state_digest, include/ast_hip.h) restated in Python: this file defines the expected value.

    digest = mix64(SEED + sum_e mix64((mix64(e) ^ LEN_KEY) + nbytes_e) + sum_i mix64(mix64(i) ^ w_i))     mod 2^64

over a list of byte strings: w_i is the i-th little-endian 32-bit word of the list, every entry starts a new word, the last word
of an entry is padded with zero bytes, and i runs on over the entries.  mix64 is the splitmix64 finaliser."""
import numpy as np

MASK = (1 << 64) - 1
SEED, LEN_KEY = 0x4153545F44494753, 0xA5A5A5A5A5A5A5A5


def mix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def _mix64_np(z):
    """mix64 on a uint64 array (numpy's uint64 arithmetic wraps around)."""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def digest_bytes(entries) -> int:
    """entries: an iterable of bytes-like objects (the tensors' bytes in list order)."""
    total, word0 = SEED, 0
    for e, raw in enumerate(entries):
        raw = bytes(raw)
        total = (total + mix64(((mix64(e) ^ LEN_KEY) + len(raw)) & MASK)) & MASK
        if not raw:
            continue
        words = np.frombuffer(raw + b"\0" * (-len(raw) % 4), dtype="<u4").astype(np.uint64)
        idx = np.arange(word0, word0 + len(words), dtype=np.uint64)
        with np.errstate(over="ignore"):
            terms = _mix64_np(_mix64_np(idx) ^ words)
            total = (total + int(terms.sum(dtype=np.uint64))) & MASK
        word0 += len(words)
    return mix64(total)


def digest_bytes_slow(entries) -> int:
    """The same, one word at a time in Python integers (what the numpy form is checked against)."""
    total, i = SEED, 0
    for e, raw in enumerate(entries):
        raw = bytes(raw)
        total = (total + mix64(((mix64(e) ^ LEN_KEY) + len(raw)) & MASK)) & MASK
        for k in range(0, len(raw), 4):
            total = (total + mix64(mix64(i) ^ int.from_bytes(raw[k:k + 4], "little"))) & MASK
            i += 1
    return mix64(total)


def tensor_bytes(t) -> bytes:
    """The exact bytes of a contiguous torch tensor (any dtype, bfloat16 included)."""
    import torch
    t = t.detach().cpu().contiguous()
    return t.reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b""


def digest_tensors(tensors) -> int:
    return digest_bytes(tensor_bytes(t) for t in tensors)
