"""The library's prefix-sum primitives (csrc/sbam_scan.hip on csrc/sbam_device.h's workgroup scan) against
numpy.cumsum in int64, at the sizes where the code takes another path: below, at and above one wave (64), one
workgroup (1024), and 1024 per-workgroup sums (where a thread's run of the sums grows to 2 and to 4 elements, with
clamped threads and an uneven tail)."""
import numpy as np
import pytest

SCAN_NS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 1024 * 1023, 1024 * 1024, 1024 * 1024 + 1, 3 * 1024 * 1024 + 17]
SCAN_CASES = [(n, cols) for n in SCAN_NS for cols in (1, 4, 32) if cols < 32 or n <= 1025]
SUMS_NS = [0, 1, 1023, 1024, 1025, 2049, 206_000]


def exclusive(v):
    """[cols, n] -> [cols, n + 1]: exclusive prefix sums, the total last."""
    out = np.zeros((v.shape[0], v.shape[1] + 1), dtype=np.int64)
    np.cumsum(v, axis=1, dtype=np.int64, out=out[:, 1:])
    return out


def gpu_exclusive_scan(v):
    import sbam
    cols, n = v.shape
    v = np.ascontiguousarray(v, dtype=np.int64)
    out = np.full((cols, n + 1), -2, dtype=np.int64)
    rc = sbam.load_library().sbam_test_exclusive_scan(0, v.ctypes.data, n, cols, out.ctypes.data)
    assert rc == 0, rc
    return out


def test_scan_exports_are_declared_and_bound():
    """Host only: the two test-support entry points are part of the declared, bound ABI (test_abi.py compares the
    whole of sbam.EXPORTS with the header)."""
    import sbam
    assert {"sbam_test_exclusive_scan", "sbam_test_scan_sums_int"} <= set(sbam.EXPORTS)
    L = sbam.load_library()
    assert hasattr(L, "sbam_test_exclusive_scan") and hasattr(L, "sbam_test_scan_sums_int")


@pytest.mark.gpu
@pytest.mark.parametrize("n,cols", SCAN_CASES)
def test_exclusive_scan(n, cols):
    rng = np.random.default_rng(1000 * cols + n % 997)
    # totals pass 2^32 after a handful of elements: a 32-bit intermediate anywhere shows
    v = rng.integers(0, 1 << 40, size=(cols, n), dtype=np.int64)
    assert np.array_equal(gpu_exclusive_scan(v), exclusive(v)), "random"
    zero = np.zeros((cols, n), dtype=np.int64)
    assert np.array_equal(gpu_exclusive_scan(zero), exclusive(zero)), "zeros"
    if n:
        last = zero.copy()
        last[:, n - 1] = 1
        assert np.array_equal(gpu_exclusive_scan(last), exclusive(last)), "a single 1 at n - 1"


@pytest.mark.gpu
@pytest.mark.parametrize("n", SUMS_NS)
def test_scan_sums_i32(n):
    import sbam
    rng = np.random.default_rng(n)
    v = rng.integers(0, (1 << 31) - 1, size=n, dtype=np.int32, endpoint=True)  # the sum leaves int32 after two
    out = np.full(n + 1, -2, dtype=np.int64)
    rc = sbam.load_library().sbam_test_scan_sums_int(0, v.ctypes.data, n, out.ctypes.data)
    assert rc == 0, rc
    assert np.array_equal(out, exclusive(v[None, :])[0])
