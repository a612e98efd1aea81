"""dsgan_fingerprint (csrc/fingerprint.hip) / dsgan_hip.functional.fingerprint: the 64-bit fingerprint of a
flat buffer's bit patterns, fp = sum_i mix((i << 32) | word_i) mod 2^64 with the splitmix64 finaliser.

The reference is numpy uint64 array arithmetic (which wraps), itself checked against python big integers on
the CPU first.  The device result must equal it exactly: at every size where the kernel takes another path
(empty, below / at / past one float4, around one block of 256 lanes, several blocks, a 2^20 + 3 buffer that
makes every lane loop) and at a 16-byte aligned pointer as well as one offset by a word (the scalar form)."""
import functools

import numpy as np
import pytest
import torch

SIZES = [0, 1, 3, 4, 5, 255, 256, 257, 4097, 2 ** 20 + 3]
M64 = (1 << 64) - 1


def _mix_int(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def ref_int(words):
    return sum(_mix_int((i << 32) | int(w)) for i, w in enumerate(words)) & M64


def ref_np(words):
    words = np.asarray(words, dtype=np.uint32)
    with np.errstate(over="ignore"):
        z = (np.arange(words.size, dtype=np.uint64) << np.uint64(32)) | words.astype(np.uint64)
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return int(np.add.reduce(z, dtype=np.uint64)) if words.size else 0


@functools.lru_cache(maxsize=None)
def _words(n):
    """random uint32 bit patterns (as float32: NaN payloads, infinities, denormals), with the special
    values planted where the buffer is long enough"""
    w = np.random.default_rng(1000 + n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    special = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFFFFFFF, 0x00000001, 0x807FFFFF]
    if n >= 2 * len(special):
        w[:len(special)] = special
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _ref(n):
    return ref_np(_words(n))


def _device(words, offset):
    """the words as a float32 device tensor whose pointer is 16-byte aligned plus ``offset`` words"""
    host = np.zeros(words.size + 4, dtype=np.uint32)
    host[offset:offset + words.size] = words
    t = torch.from_numpy(host.view(np.int32)).cuda().view(torch.float32)[offset:offset + words.size]
    assert t.is_contiguous() and (t.numel() == 0 or t.data_ptr() % 16 == 4 * offset)
    return t


def test_reference_against_big_integers():
    for n in (0, 1, 3, 4, 5, 255, 256, 257, 4097):
        assert ref_np(_words(n)) == ref_int(_words(n)), n
    assert ref_np([0]) == _mix_int(0) and ref_np([]) == 0
    assert ref_np([0, 0]) == (_mix_int(0) + _mix_int(1 << 32)) & M64
    w = _words(2 ** 20 + 3)
    sample = slice(2 ** 20 - 5, 2 ** 20 + 3)   # large indices: the index term reaches bit 52
    tail = sum(_mix_int((i << 32) | int(w[i])) for i in range(sample.start, sample.stop)) & M64
    assert (ref_np(w) - ref_np(w[:sample.start])) & M64 == tail
    assert {0x80000000, 0x7FC00001, 0x00000001} <= set(int(x) for x in _words(255)[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_fingerprint_equals_reference(n, offset):
    from dsgan_hip import functional as HF
    t = _device(_words(n), offset)
    got = HF.fingerprint(t)
    print("n=%d offset=%d: %016x (reference %016x)" % (n, offset, got, _ref(n)))
    assert got == _ref(n)
    assert HF.fingerprint(t) == got   # two calls agree
    assert torch.equal(t.view(torch.int32).cpu(), torch.from_numpy(_words(n).view(np.int32).copy()))   # read-only


@pytest.mark.gpu
def test_fingerprint_sees_order_sign_of_zero_and_dtype():
    from dsgan_hip import functional as HF
    w = _words(4097).copy()
    base = HF.fingerprint(_device(w, 0))
    i, j = 100, 4096   # one in the float4 body, one in the tail
    assert w[i] != w[j]
    w[i], w[j] = w[j], w[i]
    swapped = HF.fingerprint(_device(w, 0))
    assert swapped != base and swapped == ref_np(w)
    z = torch.zeros(257, device="cuda")
    f0 = HF.fingerprint(z)
    z[200] = -0.0
    assert z[200] == 0 and HF.fingerprint(z) != f0
    z[200] = 0.0
    assert HF.fingerprint(z) == f0 == ref_np(np.zeros(257, dtype=np.uint32))
    # any 4-byte element type, any shape: the same bits, the same value
    t = _device(_words(4096), 0)
    assert HF.fingerprint(t.view(torch.int32).view(64, 64)) == HF.fingerprint(t) == _ref(4096)


@pytest.mark.gpu
def test_bad_arguments_raise_before_any_launch():
    from dsgan_hip import _lib
    from dsgan_hip import functional as HF
    parts = int(_lib.load().dsgan_fingerprint_parts())
    assert parts >= 1
    buf = torch.zeros(64, device="cuda")
    part = torch.zeros(parts + 1, device="cuda", dtype=torch.int64)
    p, s, o = buf.data_ptr(), part.data_ptr(), part[-1:].data_ptr()
    for args, msg in (((None, 64, s, parts, o, None), "buf is null"),
                      ((p, 64, None, parts, o, None), "part or out is null"),
                      ((p, 64, s, parts, None, None), "part or out is null"),
                      ((p, -1, s, parts, o, None), "outside"),
                      ((p, 1 << 32, s, parts, o, None), "outside"),
                      ((p + 2, 16, s, parts, o, None), "aligned"),
                      ((p, 64, s, parts - 1, o, None), "scratch")):
        with pytest.raises(RuntimeError, match=msg):
            _lib.call("dsgan_fingerprint", *args)
    torch.cuda.synchronize()
    assert int(part.abs().sum()) == 0   # nothing was written
    with pytest.raises(RuntimeError, match="device tensor"):
        HF.fingerprint(torch.zeros(8))
    with pytest.raises(ValueError, match="4-byte"):
        HF.fingerprint(torch.zeros(8, device="cuda", dtype=torch.float16))
    with pytest.raises(ValueError, match="contiguous"):
        HF.fingerprint(torch.zeros(8, 8, device="cuda")[:, ::2])
