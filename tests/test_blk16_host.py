"""Host: the BLK16 layout (include/ucod_dpl.h; ucod_dpl_amd/blk16.py) -- the address formula element by element, the round trip, pi as a permutation of every
group of 32 hidden units, and the identity fc2 rests on: W[:, pi] against the packed hidden equals W against the hidden, exactly on integer operands."""
import pytest
import torch

from ucod_dpl_amd import blk16


def _chunk_offset(m, s, g, F):
    """Byte offset of chunk (m, s, g) as the header states it."""
    return (((m // 16) * (F // 32) + s) * 64 + g * 16 + (m % 16)) * 16


@pytest.mark.parametrize("M,F", [(16, 64), (1, 64), (37, 128), (300, 320)])
def test_pack_places_every_element_where_the_header_says(M, F):
    x = torch.arange(M * F, dtype=torch.int32).view(M, F) + 1
    buf = blk16.pack(x, fill=-7)
    Mp = blk16.padded_rows(M)
    assert buf.numel() == Mp * F and Mp % 16 == 0 and 0 <= Mp - M < 16
    seen = torch.zeros(Mp * F, dtype=torch.bool)
    for m in range(M):
        for s in range(F // 32):
            for g in range(4):
                o = _chunk_offset(m, s, g, F) // 2                  # 16-bit elements
                for e in range(8):
                    unit = 32 * s + 16 * (e >> 2) + 4 * g + (e & 3)
                    assert int(buf[o + e]) == int(x[m, unit]), (m, s, g, e)
                    seen[o + e] = True
    assert int(seen.sum()) == M * F
    assert bool((buf[~seen] == -7).all())                           # the padding rows and nothing else


@pytest.mark.parametrize("M,F", [(16, 64), (45, 192), (513, 384)])
def test_round_trip(M, F):
    g = torch.Generator().manual_seed(M + F)
    x = torch.randn(M, F, generator=g).half()
    assert torch.equal(blk16.unpack(blk16.pack(x, fill=float("nan")), M, F), x)


@pytest.mark.parametrize("F", [32, 64, 3072])
def test_pi_permutes_each_group_of_32(F):
    p = blk16.pi(F)
    assert p.shape == (F,)
    for s in range(F // 32):
        assert sorted(p[32 * s:32 * s + 32].tolist()) == list(range(32 * s, 32 * s + 32))
    assert not torch.equal(p, torch.arange(F))


def test_pi_is_the_order_of_a_packed_block():
    """Lane (g, m) of a 1 KB block holds positions 8 g .. 8 g + 7 of the MFMA's 32-deep K slice: reading a packed row in (s, g, e) order gives x[m, pi]."""
    M, F = 16, 128
    x = torch.arange(M * F, dtype=torch.int32).view(M, F)
    blocks = blk16.pack(x).view(M // 16, F // 32, 4, 16, 8)          # [mb, s, g, ml, e]
    rows = blocks.permute(0, 3, 1, 2, 4).reshape(M, F)               # row m in K order (s, g, e)
    assert torch.equal(rows, x[:, blk16.pi(F)])


@pytest.mark.parametrize("M,N,F", [(37, 24, 128), (16, 8, 64)])
def test_permuted_weight_against_packed_hidden_is_the_same_product(M, N, F):
    g = torch.Generator().manual_seed(M * N + F)
    h = torch.randint(-8, 9, (M, F), generator=g, dtype=torch.int64)
    w = torch.randint(-8, 9, (N, F), generator=g, dtype=torch.int64)
    wp = blk16.permute_weight(w)
    blocks = blk16.pack(h).view(blk16.padded_rows(M) // 16, F // 32, 4, 16, 8)
    a_in_k_order = blocks.permute(0, 3, 1, 2, 4).reshape(-1, F)[:M]  # what the MFMA sees as A, k = 32 s + 8 g + e
    assert torch.equal(a_in_k_order @ wp.t(), h @ w.t())
