"""numpy statement of the device-side noise of the training crop (csrc/patches.hip: Philox-4x32-10 + Box-Muller, keyed by
(seed, global element index before the flip)), for tests/test_philox_ref.py (known answers) and tests/test_gpu_device_noise.py.

Everything is integer arithmetic on uint64 arrays masked to 32 bits, then fp64; numpy only."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
SIGMA = 0.01                                   # isprs:305: normal(0, 0.01)
TWO_PI = 6.283185307179586


def _u64(a):
    return np.asarray(a, dtype=np.uint64) & M32


def philox4x32_10(key0, key1, c0, c1, c2, c3):
    """Philox-4x32 with 10 rounds (Salmon et al., SC'11): key (key0, key1), counter (c0, c1, c2, c3), each a uint64 array (or a
    Python integer) holding a 32-bit word; returns the four output words as uint64 arrays."""
    k0, k1 = _u64(key0), _u64(key1)
    c0, c1, c2, c3 = _u64(c0), _u64(c1), _u64(c2), _u64(c3)
    for _ in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2                       # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & M32, (p0 >> _S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + _W0) & M32, (k1 + _W1) & M32
    return c0, c1, c2, c3


def _counter_key(seed, index):
    index = np.asarray(index, dtype=np.uint64)
    seed = int(seed)
    assert 0 <= seed < 1 << 64
    return (seed & 0xFFFFFFFF, seed >> 32), (index & M32, index >> _S32, 0x1234567, 0x89ABCDEF)


def box_muller(a, b):
    """one N(0, 1) deviate from two 32-bit words: u1 = (a + 1) / 2^32 in (0, 1], u2 = b / 2^32 in [0, 1); fp64"""
    u1 = (np.asarray(a, dtype=np.float64) + 1.0) * (1.0 / 4294967296.0)
    u2 = np.asarray(b, dtype=np.float64) * (1.0 / 4294967296.0)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)


def device_noise(seed, index, words=(0, 1)):
    """the N(0, 1) deviate of element `index` (uint64 array) under `seed` (an integer below 2^64), as the kernel keys it: counter
    (index low, index high, 0x1234567, 0x89abcdef), key (seed low, seed high), Box-Muller on output words 0 and 1.  `words` picks other
    output words: only for negative controls."""
    key, ctr = _counter_key(seed, index)
    r = philox4x32_10(key[0], key[1], *ctr)
    return box_muller(r[words[0]], r[words[1]])


def expected(values, seed, index, mean3, std3, words=(0, 1)):
    """what the crop stores for the noiseless fp64 `values` [..., C] at the element indices `index` (same shape): ((v + 0.01 n) - mean)
    / std for the channels below 3, v + 0.01 n above, every operation rounded on its own in fp64 (the kernel file is compiled with
    contraction off), one rounding to float32 on the store."""
    v = np.asarray(values, dtype=np.float64)
    e = v + SIGMA * device_noise(seed, index, words)
    C = v.shape[-1]
    m = np.zeros(C)
    s = np.ones(C)
    n = min(3, C)
    m[:n], s[:n] = np.asarray(mean3, dtype=np.float64)[:n], np.asarray(std3, dtype=np.float64)[:n]
    out = e.copy()
    out[..., :n] = (e[..., :n] - m[:n]) / s[:n]
    return out.astype(np.float32)
