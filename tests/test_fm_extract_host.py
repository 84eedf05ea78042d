"""CPU: dk_fm_extract_bytes (host arithmetic) and the null-context answer of every extract entry point."""
import ctypes as C

from dark_amd import _lib
from dark_amd.context import fm_extract_bytes, fm_index_bytes, fm_locate_bytes

STEPS = [1, 2, 4, 32, 1024, 4096]


def bound(total, count, step):
    return 4 * total // step + 4 * count + 256


def test_size_is_monotone_aligned_and_bounded():
    totals = [1, 2, 31, 32, 33, 1023, 1024, 1025, 4096, 65535, 65536, 10 ** 6, 10 ** 8, 2 ** 31 - 2]
    for step in STEPS:
        for count in (1, 2, 500):
            prev = 0
            for total in totals:
                if count > total:
                    continue
                b = fm_extract_bytes(total, count, step)
                assert b > 0 and b % 4 == 0 and prev <= b <= bound(total, count, step), (total, count, step, b)
                # room for every block's anchors: sum of ceil(n_b / step) <= total // step + count
                assert b >= 4 * (64 + total // step + count)
                prev = b
    for total in (1000, 10 ** 6):
        for step in STEPS:
            sizes = [fm_extract_bytes(total, count, step) for count in (1, 2, 3, 100, 1000)]
            assert sizes == sorted(sizes)
        for count in (1, 100):
            sizes = [fm_extract_bytes(total, count, step) for step in STEPS]
            assert sizes == sorted(sizes, reverse=True)
    n = 10 ** 8
    assert fm_extract_bytes(n, 1, 32) <= 0.125 * n + 260
    assert n + fm_index_bytes(n, 1) + fm_extract_bytes(n, 1, 32) <= 2.13 * n
    assert n + fm_index_bytes(n, 1) + fm_locate_bytes(n, 1, 32) + fm_extract_bytes(n, 1, 32) <= 2.39 * n


def test_anchors_of_unequal_blocks_fit():
    """the worst pack for the anchors: every block one byte over a multiple of the step"""
    for step in STEPS:
        for count in (1, 7, 500):
            sizes = [step * (1 + b % 3) + 1 for b in range(count)]
            need = sum((n + step - 1) // step for n in sizes)
            assert fm_extract_bytes(sum(sizes), count, step) >= 4 * (64 + need), (step, count)


def test_size_of_refused_arguments_is_zero():
    for step in (0, 3, 8192, 48, 2 ** 31, -1, 2 ** 32):
        assert fm_extract_bytes(1000, 1, step) == 0, step
    for total, count in ((0, 1), (2 ** 31 - 1, 1), (10, 0), (10, 11), (-1, 1), (10, -1), (10 ** 6, _lib.DK_PACKED_MAX_BLOCKS + 1)):
        assert fm_index_bytes(total, count) == 0 and fm_extract_bytes(total, count, 32) == 0, (total, count)


def test_null_context():
    lib = _lib.load()
    p = C.c_void_p(256)  # (never looked at: the context is checked first)
    ns = (C.c_size_t * 1)(10)
    assert lib.dk_dev_fm_extract_build(None, p, 10, 0, 32, p) == _lib.DK_E_ARG
    assert lib.dk_dev_fm_extract_build_packed(None, p, 1, ns, p, 32, p) == _lib.DK_E_ARG
    assert lib.dk_dev_fm_extract(None, p, 10, p, p, 32, p, p, 1, 1, p) == _lib.DK_E_ARG
    assert lib.dk_dev_fm_extract_packed(None, p, 1, ns, p, p, 32, p, p, 1, p, 1, p) == _lib.DK_E_ARG
    assert lib.dk_fm_extract(None, p, 10, 0, 32, p, p, 1, 1, p) == _lib.DK_E_ARG
