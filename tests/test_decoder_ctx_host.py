"""Decoder contexts, the part that needs no GPU: dk_workspace_bytes (the accounting both dk_ctx_create and dk_ctx_create_decoder allocate by),
its Python twin, and dk_ctx_create_decoder's refusal to run without a device."""
import ctypes as C

import pytest

import dark_amd
from dark_amd import _lib
from dark_amd.context import workspace_bytes

FULL, DECODER = _lib.PURPOSES["full"], _lib.PURPOSES["decoder"]
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537, 70000, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 20) + 4097,
         768771, 10**8, 1 << 30, 0x7FFFFFFE]


@pytest.fixture(scope="module")
def lib():
    return dark_amd.load_library()


def test_non_decreasing_in_max_n(lib):
    # the listed sizes, and every size around the places where the formula changes form: the S = 8 / S = 64 switch at 2^16, the tile size
    # 4096, and 256 tiles x 4096 = 2^20, where the chunk count of the histogram scan folds back
    dense = sorted(set(SIZES) | set(range(1, 600)) | set(range(65536 - 300, 65536 + 300)) | set(range((1 << 20) - 5000, (1 << 20) + 5000, 7)))
    for max_blocks in (1, 2, 1024, _lib.DK_PACKED_MAX_BLOCKS):
        last = 0
        for n in dense:
            w = lib.dk_workspace_bytes(DECODER, n, max_blocks)
            assert w > 0 and w >= last, (n, max_blocks, w, last)
            last = w
    last = 0
    for n in dense:
        w = lib.dk_workspace_bytes(FULL, n, 1)
        assert w >= last and w > 0
        last = w


def test_non_decreasing_in_max_blocks(lib):
    for n in SIZES:
        last = 0
        for mb in (1, 2, 3, 63, 64, 65, 1000, 4096, 65535, 65536):
            w = lib.dk_workspace_bytes(DECODER, n, mb)
            assert w >= last and w > 0, (n, mb)
            last = w
        # a full context does not look at max_blocks at all
        assert len({lib.dk_workspace_bytes(FULL, n, mb) for mb in (0, 1, 77, 1 << 20)}) == 1


def test_bad_arguments_give_zero(lib):
    assert lib.dk_workspace_bytes(2, 1000, 1) == 0 and lib.dk_workspace_bytes(-1, 1000, 1) == 0  # unknown purpose
    assert lib.dk_workspace_bytes(DECODER, 0, 1) == 0 and lib.dk_workspace_bytes(FULL, 0, 1) == 0
    assert lib.dk_workspace_bytes(DECODER, 1000, 0) == 0
    assert lib.dk_workspace_bytes(DECODER, 1000, _lib.DK_PACKED_MAX_BLOCKS + 1) == 0
    assert lib.dk_workspace_bytes(DECODER, 1000, _lib.DK_PACKED_MAX_BLOCKS) > 0
    assert lib.dk_workspace_bytes(DECODER, 0x7FFFFFFF, 1) == 0  # past the largest block a context can be made for (dk_ctx_create: DK_E_ARG)


def test_full_formula_is_the_one_contexts_have_always_had(lib):
    # workspace_bytes(n) of csrc/abi.cpp, written out: 62 n + n/8 (sort) + 6 n (text, L, SA) + n/4 + n (on top) + n/4 (headroom) + 64 MiB
    for n in SIZES:
        assert lib.dk_workspace_bytes(FULL, n, 1) == 62 * n + n // 8 + 6 * n + n // 4 + n + n // 4 + (64 << 20)


@pytest.mark.parametrize("n", [1 << 24, 1 << 30])
def test_decoder_takes_a_quarter_or_less(lib, n):
    # the condition the term counts give: 2 n (L, output) + 8 n (successors) + n/4 (histograms) + 3 n/8 (splitters) + 4 n (records) = 14.625 n
    # against 69.625 n + 64 MiB
    dec, full = lib.dk_workspace_bytes(DECODER, n, 1), lib.dk_workspace_bytes(FULL, n, 1)
    print("n = %d: decoder %d, full %d, ratio %.3f" % (n, dec, full, full / dec))
    assert 4 * dec <= full


def test_no_cpu_backend_for_decoder_contexts(lib):
    import torch
    h = C.c_void_p()
    assert lib.dk_ctx_create_decoder(0, 0, 1, C.byref(h)) == _lib.DK_E_ARG
    assert lib.dk_ctx_create_decoder(0, 1000, 0, C.byref(h)) == _lib.DK_E_ARG
    assert lib.dk_ctx_create_decoder(0, 1000, _lib.DK_PACKED_MAX_BLOCKS + 1, C.byref(h)) == _lib.DK_E_ARG
    assert lib.dk_ctx_create_decoder(-1, 1000, 1, C.byref(h)) == _lib.DK_E_NODEVICE  # -1 ("CPU") is not a backend
    assert lib.dk_ctx_purpose(None) == _lib.DK_E_ARG
    if torch.cuda.is_available():
        return  # (with a GPU the rest is tests/test_gpu_decoder_ctx.py's)
    assert lib.dk_ctx_create_decoder(0, 1000, 1, C.byref(h)) == _lib.DK_E_NODEVICE
    with pytest.raises(dark_amd.DarkError) as e:
        dark_amd.Context(1000, purpose="decoder")
    assert e.value.code == _lib.DK_E_NODEVICE


def test_python_workspace_bytes_agrees(lib):
    for n in SIZES:
        assert workspace_bytes("full", n) == lib.dk_workspace_bytes(FULL, n, 1)
        for mb in (1, 7, 65536):
            assert workspace_bytes("decoder", n, mb) == lib.dk_workspace_bytes(DECODER, n, mb)
        assert workspace_bytes("decoder", n) == lib.dk_workspace_bytes(DECODER, n, 1)  # max_blocks defaults to 1
    assert workspace_bytes("decoder", 0) == 0 and workspace_bytes("nothing", 1000) == 0 and workspace_bytes("decoder", 1000, 0) == 0
    with pytest.raises(dark_amd.DarkError) as e:
        dark_amd.Context(1000, purpose="nothing")
    assert e.value.code == _lib.DK_E_ARG
