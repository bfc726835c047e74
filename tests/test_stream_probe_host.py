"""The comparators of tests/stream_probe.py on the CPU: what the stream tests call 'the same' must reject a NaN, one flipped mantissa
bit and a shape mismatch, or a GPU test built on them passes vacuously."""
import numpy as np

import stream_probe as SP


def _flip_lowest_mantissa_bit(a, index):
    out = a.copy()
    out.reshape(-1).view(np.uint32)[index] ^= 1
    return out


def test_import_makes_no_gpu_call():
    import sys
    assert "torch" not in vars(SP) and SP._cycles_per_ms is None
    assert "stream_probe" in sys.modules


def test_same_bits_accepts_equal_arrays_and_signed_zero():
    a = np.array([[1.5, -0.0, 0.0], [np.inf, -2.0, 3e-39]], np.float32)
    assert SP.same_bits(a, a.copy())
    assert SP.same_bits(np.array([-0.0], np.float32), np.array([-0.0], np.float32))
    assert SP.same_bits(np.arange(7, dtype=np.int32), np.arange(7, dtype=np.int32))
    assert SP.same_bits(np.array([True, False]), np.array([True, False]))
    assert SP.same_bits(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    nan = np.array([np.nan, 1.0], np.float32)
    assert SP.same_bits(nan, nan.copy())                   # the same NaN bit pattern is the same bits ...


def test_same_bits_rejects_a_nan_a_flipped_bit_a_sign_and_a_shape():
    a = np.linspace(-1.0, 1.0, 12, dtype=np.float32).reshape(3, 4)
    bad = a.copy()
    bad[1, 2] = np.nan
    assert not SP.same_bits(bad, a) and not SP.same_bits(a, bad)      # ... but a NaN against a number never is
    for index in (0, 5, 11):
        assert not SP.same_bits(_flip_lowest_mantissa_bit(a, index), a)
    assert not SP.same_bits(np.array([0.0], np.float32), np.array([-0.0], np.float32))
    assert not SP.same_bits(a, a.reshape(4, 3))
    assert not SP.same_bits(a, a[:2])
    assert not SP.same_bits(a, a.astype(np.float64))
    assert not SP.same_bits(np.zeros(4, np.int32), np.zeros(4, np.float32))


def test_close_to_serial_accepts_within_the_fraction_of_the_maximum():
    b = np.array([100.0, 1.0, -0.0, 0.0], np.float32)
    assert SP.close_to_serial(b.copy(), b, 0.0)
    assert SP.close_to_serial(np.array([-0.0], np.float32), np.array([-0.0], np.float32), 0.0)
    a = b.copy()
    a[1] += 4e-3                                            # 4e-5 of max|b| = 100: small against the tensor, not against the element
    assert SP.close_to_serial(a, b, 5e-5)
    assert not SP.close_to_serial(a, b, 3e-5)
    assert SP.close_to_serial(np.zeros(3, np.float32), np.zeros(3, np.float32), 1e-5)
    assert not SP.close_to_serial(np.full(3, 1e-3, np.float32), np.zeros(3, np.float32), 1e-5)


def test_close_to_serial_rejects_a_nan_a_flipped_exponent_and_a_shape():
    b = np.linspace(0.5, 2.0, 10, dtype=np.float32)
    a = b.copy()
    a[3] = np.nan
    assert not SP.close_to_serial(a, b, 1.0)
    both = b.copy()
    both[3] = np.nan
    assert not SP.close_to_serial(a, both, 1.0)             # a NaN in `a` fails even where `b` has one in the same place
    assert not SP.close_to_serial(b, both, 1.0)             # and a NaN in the reference compares with nothing
    inf = b.copy()
    inf[0] = np.inf
    assert not SP.close_to_serial(inf, b, 1.0)
    assert not SP.close_to_serial(b, b.reshape(2, 5), 1.0)
    assert not SP.close_to_serial(b[:9], b, 1.0)
    # one flipped mantissa bit is a relative 1.2e-7 of that element: inside the atomic-order bar, outside a bar of zero
    f = _flip_lowest_mantissa_bit(b, 9)
    assert SP.close_to_serial(f, b, 5e-5) and not SP.close_to_serial(f, b, 0.0) and not SP.same_bits(f, b)


def test_deviation_is_relative_to_the_reference_maximum():
    b = np.array([0.0, -8.0], np.float32)
    assert SP.deviation(np.array([0.5, -8.0], np.float32), b) == 0.0625
    assert SP.deviation(b, b) == 0.0
    assert SP.deviation(np.zeros(0, np.float32), np.zeros(0, np.float32)) == 0.0
