"""The numpy restatement of the crop's device-side noise (tests/philox_ref.py) against the published known answers of
Philox4x32-10 (Random123's kat_vectors: counter words, key words -> output words), and the moments of its Box-Muller deviates.
CPU only: this is what tests/test_gpu_device_noise.py then holds the kernel to."""
import numpy as np

import philox_ref as R

# (counter, key, output)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox4x32_10_known_answers():
    for ctr, key, want in KNOWN_ANSWERS:
        got = R.philox4x32_10(key[0], key[1], *ctr)
        assert tuple(int(g) for g in got) == want, (ctr, key)
    # ... and elementwise on arrays: the three vectors in one call
    c = [np.array([kat[0][i] for kat in KNOWN_ANSWERS], dtype=np.uint64) for i in range(4)]
    k = [np.array([kat[1][i] for kat in KNOWN_ANSWERS], dtype=np.uint64) for i in range(2)]
    got = R.philox4x32_10(k[0], k[1], *c)
    for i in range(4):
        assert [int(v) for v in got[i]] == [kat[2][i] for kat in KNOWN_ANSWERS]


def test_device_noise_keying_and_moments():
    idx = np.arange(3072, dtype=np.uint64)
    n = R.device_noise(12345, idx)
    assert n.dtype == np.float64 and np.isfinite(n).all()
    assert abs(n.mean()) < 0.05 and abs(n.std() - 1.0) < 0.03
    # the keying: seed low / high word are the key, index low / high word the first two counter words
    seed, index = (7 << 32) | 12345, np.array([5, (3 << 32) | 9], dtype=np.uint64)
    r = R.philox4x32_10(12345, 7, np.array([5, 9], dtype=np.uint64), np.array([0, 3], dtype=np.uint64), 0x1234567, 0x89abcdef)
    np.testing.assert_array_equal(R.device_noise(seed, index), R.box_muller(r[0], r[1]))
    assert not np.array_equal(R.device_noise(seed, idx), R.device_noise(12345, idx))      # the upper seed word matters
    # u1 = (r0 + 1) / 2^32 never reaches 0 (no log(0)), u2 = r1 / 2^32 stays below 1
    assert R.box_muller(0xffffffff, 0) == 0.0 and np.isfinite(R.box_muller(0, 0xffffffff))


def test_expected_rounds_every_operation_on_its_own():
    v = np.array([[0.25, 0.5, 0.75, 0.125, 1.0]])
    idx = np.arange(5, dtype=np.uint64).reshape(1, 5)
    mean, std = np.array([0.5, 0.4, 0.3]), np.array([0.25, 0.2, 0.1])
    n = R.device_noise(99, idx)
    got = R.expected(v, 99, idx, mean, std)
    assert got.dtype == np.float32 and got.shape == v.shape
    for c in range(5):
        e = v[0, c] + 0.01 * n[0, c]
        if c < 3:
            e = (e - mean[c]) / std[c]
        assert got[0, c] == np.float32(e)
