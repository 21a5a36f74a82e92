"""The checker's general record-0 kernel (k_check) on the launches only it serves: reads_to_check == 0 in every mode
(no interior kernel runs: every tile goes to k_check), and by-key counts over unaligned sub-ranges.  The ranges of
2.bam hold interior tiles (inside the range, a tile plus kInteriorTail before the stream's end) and boundary tiles
(the first tile of an unaligned range, the tiles near the stream's end), and k_check decides which is which per tile."""
import numpy as np
import pytest

from test_gpu_parity import pair_hist

pytestmark = pytest.mark.gpu

NAME = "2.bam"
L = 1606522  # 2.bam's uncompressed stream
K_TILE, K_INTERIOR_TAIL = 8192, 262144 + 512  # sbam_check.hip: kTile, kInteriorTail
RANGES = [(0, L), (1, L), (3 * 8192 + 5, L - 7), (0, 8192), (L - 300, L)]
SUCC = 0x80000000


def tiles(x0, x1):
    """(interior, boundary) tile counts of [x0, x1): interior_tiles() of sbam_check.hip."""
    x0a = x0 & ~63
    nt = (x1 - x0a + K_TILE - 1) // K_TILE
    lim = min(x1, L - K_INTERIOR_TAIL)
    tlo = 0 if x0 == x0a else 1
    thi = max((lim - x0a) // K_TILE if lim - x0a >= K_TILE else 0, tlo)
    return thi - tlo, nt - (thi - tlo)


def test_ranges_hold_interior_and_boundary_tiles():
    assert tiles(0, L) == (164, (L + K_TILE - 1) // K_TILE - 164)
    got = [tiles(*r) for r in RANGES]
    assert all(i >= 1 and b >= 1 for i, b in got[:3]), got  # both kinds in one launch
    assert got[3] == (1, 0) and got[4] == (0, 1), got       # a lone interior tile, a lone boundary tile


@pytest.fixture(scope="module")
def oracle_words(oracle_files):
    """Oracle words of a range at reads_to_check R, computed once per (range, R) and left unchanged."""
    cache = {}

    def get(x0, x1, R):
        if (x0, x1, R) not in cache:
            w = oracle_files(NAME).check_full_range(x0, x1, R)
            w.setflags(write=False)
            cache[x0, x1, R] = w
        return cache[x0, x1, R]
    return get


def check_counts(g, o, want, x0, x1, R, by_key):
    counts, npos, rbe, nsucc = o.counts_range(x0, x1, R)
    c, bits = g.check_full_counts(x0, x1, R, want_bitmap=True, by_key=by_key)
    assert np.array_equal(c.totals, counts.sum(0))
    assert np.array_equal(c.positions, npos)
    # (without by_key the per-flag table holds keys 0-2 only)
    assert np.array_equal(c.by_key, counts) if by_key else np.array_equal(c.by_key[:3], counts[:3])
    assert np.array_equal(c.reads_before_error, rbe)
    assert c.n_success == nsucc
    assert np.array_equal(bits, (want & SUCC) != 0)
    return c


@pytest.mark.parametrize("r", RANGES)
def test_reads_to_check_zero_every_mode(r, gpu_files, oracle_files, oracle_words):
    g, o = gpu_files(NAME), oracle_files(NAME)
    assert o.L == L
    x0, x1 = r
    want = oracle_words(x0, x1, 0)
    assert np.array_equal(g.check_eager(x0, x1, 0), (want & SUCC) != 0)
    assert np.array_equal(g.check_full_words(x0, x1, 0), want)
    for by_key in (False, True):
        c = check_counts(g, o, want, x0, x1, 0, by_key)
        assert c.n_success == x1 - x0  # Success(0) at every position


@pytest.mark.parametrize("r", RANGES)
def test_by_key_unaligned_ranges(r, gpu_files, oracle_files, oracle_words):
    g, o = gpu_files(NAME), oracle_files(NAME)
    x0, x1 = r
    want = oracle_words(x0, x1, 10)
    c = check_counts(g, o, want, x0, x1, 10, True)
    assert np.array_equal(c.pair_hist, pair_hist(want))
