"""nrldpc_encode_kernel at offset device pointers, path by path (tests/tx_cases.py names the paths and holds the lists to reaching
all of them): the ballot ring build at Z % 32 == 0, the byte-wise extension store at 4 | Z and the 4-byte / byte systematic copies at
the large sizes run only when info / out are not 16-byte aligned -- a sub-allocated buffer, a packed layout, a slice.  Through
Codec.encode_dev against the oracle's encoder; every comparison is exact."""
import numpy as np
import pytest

import tx_cases as T
from conftest import ALL_Z, BG_DIMS

pytestmark = pytest.mark.gpu


def _encode_at(codec, info, io, oo):
    """info [B][K] placed io bytes, the codewords oo bytes above a 256-byte boundary; returns (codewords, checks passed)."""
    import torch
    B = info.shape[0]
    src = T.Slot(info.size, io, info)
    before = src.whole()
    dst = T.Slot(B * codec.N_cw, oo)
    codec.encode_dev(src.ptr, B, dst.ptr)
    torch.cuda.synchronize()
    return dst.data().reshape(B, codec.N_cw), dst.guards_intact() and bool((src.whole() == before).all())


@pytest.mark.parametrize("bg,Z", [(bg, Z) for bg in (1, 2) for Z in T.ENC_SIZES[bg]])
def test_encoder_paths_at_offset_pointers(pkg, orc, bg, Z):
    rng = np.random.default_rng(1000 * bg + Z)
    kb = BG_DIMS[bg][2]
    batches = T.enc_batches(bg, Z)
    info = rng.integers(0, 2, (max(batches), kb * Z), dtype=np.uint8)
    want = orc.encode(bg, Z, info)
    assert orc.syndrome_weight(bg, Z, want[0]) == 0
    codec = pkg.Codec(bg, Z, max_iter=1)
    try:
        for io, oo in T.ENC_OFFSETS:
            for B in batches:
                tag = (bg, Z, io, oo, B, [T.enc_class(bg, Z, io, oo, c)[3:] for c in range(B)])
                cw, clean = _encode_at(codec, info[:B], io, oo)
                assert (cw == want[:B]).all(), tag
                assert orc.syndrome_weight(bg, Z, cw[0]) == 0 and orc.syndrome_weight(bg, Z, cw[B - 1]) == 0, tag
                assert clean, tag  # the bytes either side of the output and the whole info buffer are as they were
    finally:
        codec.close()


@pytest.mark.parametrize("bg", [1, 2])
def test_encoder_all_lifting_sizes_at_offset_pointers(pkg, orc, bg):
    """Every size through the byte paths (1, 1) and the 4-byte paths (4, 4), which an aligned base never takes at 16 | K."""
    rng = np.random.default_rng(310 + bg)
    kb = BG_DIMS[bg][2]
    for Z in ALL_Z:
        info = rng.integers(0, 2, (5, kb * Z), dtype=np.uint8)
        want = orc.encode(bg, Z, info)
        codec = pkg.Codec(bg, Z, max_iter=1)
        try:
            for off in (1, 4):
                cw, clean = _encode_at(codec, info, off, off)
                assert (cw == want).all() and clean, (bg, Z, off)
        finally:
            codec.close()


@pytest.mark.parametrize("bg,Z", T.ENC_RING_SIZES)
def test_encoder_reads_bit_0_only(pkg, orc, bg, Z):
    """include/nrldpc.h: a byte b encodes as b & 1 and every output byte is 0 or 1 -- on the 16-byte, 4-byte and byte copies and on
    the word and ballot ring builds alike."""
    rng = np.random.default_rng(2000 * bg + Z)
    kb = BG_DIMS[bg][2]
    info = rng.integers(0, 256, (5, kb * Z), dtype=np.uint8)
    want = orc.encode(bg, Z, info & 1)
    codec = pkg.Codec(bg, Z, max_iter=1)
    try:
        for io, oo in T.ENC_OFFSETS:
            cw, clean = _encode_at(codec, info, io, oo)
            assert cw.max() <= 1 and (cw == want).all() and clean, (bg, Z, io, oo)
    finally:
        codec.close()


@pytest.mark.parametrize("bg,Z", [(1, 96), (1, 384)])
def test_host_entry_equals_device_entry(pkg, bg, Z):
    """Codec.encode (host arrays, the library's own staging buffers) and encode_dev at an offset pointer: the same codewords, one
    size per number of waves per codeword."""
    assert {T.enc_nwc(1, 96), T.enc_nwc(1, 384)} == {1, 4}
    rng = np.random.default_rng(Z)
    info = rng.integers(0, 2, (5, BG_DIMS[bg][2] * Z), dtype=np.uint8)
    codec = pkg.Codec(bg, Z, max_iter=1)
    try:
        host = codec.encode(info)
        for io, oo in ((0, 0), (3, 5)):
            cw, clean = _encode_at(codec, info, io, oo)
            assert (cw == host).all() and clean, (bg, Z, io, oo)
    finally:
        codec.close()
