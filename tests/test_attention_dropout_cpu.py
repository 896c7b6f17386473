"""The host mirror of K8's attention-dropout mask (``reference.attention_dropout_mask``): a pure
function of (seed, offset, b, h, q, k, threshold), checked here without a GPU."""
import math

import pytest
import torch

from madnn.ops import reference

M32 = 0xFFFFFFFF


def _philox4x32_10(ctr, key):
    """Scalar Philox4x32-10 in Python ints (Salmon et al., 'Parallel random numbers: as easy as 1, 2, 3')."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def test_scalar_philox_known_answers():
    # the known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10)
    assert _philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert _philox4x32_10((M32,) * 4, (M32, M32)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert _philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_mask_is_the_documented_function_of_its_inputs():
    """Element (b, h, q, k) = byte k & 3 of word q & 3 of Philox(counter (offset lo, b*H + h, q >> 2,
    k >> 2), key (seed lo, seed hi ^ offset hi)) < threshold, with 64-bit seed and offset."""
    B, H, S, p = 2, 3, 13, 0.3
    seed, offset = 0xFEDCBA9876543210, (5 << 32) | 12
    thr = reference.attention_dropout_threshold(p)
    assert thr == 179
    m = reference.attention_dropout_mask(B, H, S, p, seed, offset)
    assert m.dtype == torch.bool and m.shape == (B, H, S, S)
    key = (seed & M32, ((seed >> 32) ^ (offset >> 32)) & M32)
    for b in range(B):
        for h in range(H):
            for q in range(S):
                for k in range(S):
                    w = _philox4x32_10((offset & M32, b * H + h, q >> 2, k >> 2), key)
                    assert bool(m[b, h, q, k]) == (((w[q & 3] >> (8 * (k & 3))) & 0xFF) < thr), (b, h, q, k)


def test_mask_deterministic_and_sensitive_to_each_input():
    a = reference.attention_dropout_mask(2, 2, 64, 0.5, 11, 4)
    assert torch.equal(a, reference.attention_dropout_mask(2, 2, 64, 0.5, 11, 4))
    assert not torch.equal(a, reference.attention_dropout_mask(2, 2, 64, 0.5, 12, 4))       # seed
    assert not torch.equal(a, reference.attention_dropout_mask(2, 2, 64, 0.5, 11, 8))       # offset
    assert not torch.equal(a, reference.attention_dropout_mask(2, 2, 64, 0.5, 11 + (1 << 32), 4))  # seed, high word
    assert not torch.equal(a[0], a[1])                                                        # b
    assert not torch.equal(a[0, 0], a[0, 1])                                                  # h
    assert not torch.equal(a[0, 1], a[1, 0])                                                  # (b, h), not b + h


def test_mask_does_not_depend_on_sequence_length():
    small = reference.attention_dropout_mask(1, 2, 77, 0.1, 3, 0)
    for S in (78, 80, 200):
        big = reference.attention_dropout_mask(1, 2, S, 0.1, 3, 0)
        assert torch.equal(small, big[:, :, :77, :77]), S


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_fraction_matches_the_quantised_probability(p):
    B, H, S = 2, 4, 360   # 1 036 800 elements
    m = reference.attention_dropout_mask(B, H, S, p, 2024, 16)
    n = m.numel()
    assert n >= 10 ** 6
    keep = reference.attention_dropout_threshold(p) / 2 ** reference.DROPOUT_BITS
    sd = math.sqrt(keep * (1 - keep) / n)
    frac = float(m.double().mean())
    print(f"p={p}: keep fraction {frac:.6f}, expected {keep:.6f}, {abs(frac - keep) / sd:.2f} sd")
    assert abs(frac - keep) < 5 * sd


def test_threshold_quantisation_and_rejection():
    assert reference.attention_dropout_threshold(0.0) == 256
    assert reference.attention_dropout_threshold(0.1) == 230
    assert reference.attention_dropout_threshold(0.5) == 128
    assert reference.attention_dropout_threshold(0.997) == 1
    for bad in (0.999, 1.0 - 1e-9, 1.0, 1.5, -0.1):
        with pytest.raises(ValueError):
            reference.attention_dropout_threshold(bad)
        with pytest.raises(ValueError):
            reference.attention_dropout_mask(1, 1, 8, bad, 0, 0)


def test_cpu_tensors_take_the_eager_reference():
    from madnn import ops

    torch.manual_seed(0)
    q, k, v = (torch.randn(1, 16, 2, 8) for _ in range(3))
    assert torch.equal(ops.attention(q, k, v, causal=True, dropout_p=0.0), ops.attention(q, k, v, causal=True))
    o = ops.attention(q, k, v, causal=True, dropout_p=0.5)
    assert o.shape == q.shape and not torch.equal(o, ops.attention(q, k, v, causal=True))
    assert not ops.attention_supported(q, 64, 0.1)
