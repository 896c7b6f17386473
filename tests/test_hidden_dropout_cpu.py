"""The host mirror of the hidden-dropout mask of K3 / K16 (``reference.hidden_dropout_mask``): a pure
function of (seed, offset, row, col, threshold), and the CPU tier of the ops that take ``dropout_p``,
checked here without a GPU."""
import pytest
import torch

from madnn import ops
from madnn.ops import reference

M32 = 0xFFFFFFFF
K = 230 / 256   # keep probability of p = 0.1 at the mask's 1/256 resolution


def _philox4x32_10(ctr, key):
    """Scalar Philox4x32-10 in Python ints (Salmon et al., 'Parallel random numbers: as easy as 1, 2, 3')."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def _scalar_keep(row, col, thr, seed, offset):
    key = (seed & M32, ((seed >> 32) ^ (offset >> 32)) & M32)
    w = _philox4x32_10((offset & M32, row & M32, (row >> 32) & M32, col >> 4), key)
    return ((w[(col >> 2) & 3] >> (8 * (col & 3))) & 0xFF) < thr


@pytest.mark.parametrize("row0", [0, 2 ** 32 - 2, (3 << 32) + 5])
def test_mask_is_the_documented_function_of_its_inputs(row0):
    """Element (row, col) = byte col & 3 of word (col >> 2) & 3 of Philox(counter (offset lo, row lo,
    row hi, col >> 4), key (seed lo, seed hi ^ offset hi)) < threshold; rows past 2**32 through row0."""
    rows, H, p = 4, 40, 0.3
    seed, offset = 0xFEDCBA9876543210, (0x80000005 << 32) | 12   # offset with high bits set
    thr = reference.attention_dropout_threshold(p)
    m = reference.hidden_dropout_mask(rows, H, p, seed, offset, row0=row0)
    assert m.dtype == torch.bool and m.shape == (rows, H)
    for r in range(rows):
        for c in (0, 3, 4, 15, 16, 17, 31, 32, 39):
            assert bool(m[r, c]) == _scalar_keep(row0 + r, c, thr, seed, offset), (r, c)
    # the high row word is part of the counter: the same low word with another high word is another mask
    assert not torch.equal(m, reference.hidden_dropout_mask(rows, H, p, seed, offset, row0=row0 + (1 << 32)))


def test_mask_does_not_depend_on_the_hidden_size():
    small = reference.hidden_dropout_mask(40, 64, 0.1, 7, 4)
    big = reference.hidden_dropout_mask(40, 1024, 0.1, 7, 4)
    assert torch.equal(small, big[:, :64])
    assert torch.equal(reference.hidden_dropout_mask(40, 72, 0.1, 7, 4), big[:, :72])   # H % 16 == 8
    assert torch.equal(reference.hidden_dropout_mask(9, 1024, 0.1, 7, 4, row0=31), big[31:40])


def test_keep_fraction_matches_the_quantised_probability():
    m = reference.hidden_dropout_mask(256, 1024, 0.1, 2024, 16)
    frac = float(m.double().mean())
    print(f"keep fraction {frac:.6f}, expected {K:.6f}")
    assert abs(frac - K) < 0.003   # 5 sigma of a binomial over 262144 elements (sigma ~ 0.0006)


def test_consecutive_rows_are_independent():
    m = reference.hidden_dropout_mask(256, 1024, 0.1, 2024, 16)
    differ = float((m[1:] != m[:-1]).double().mean())
    print(f"consecutive rows differ in {differ:.6f}, expected {2 * K * (1 - K):.6f}")
    assert abs(differ - 2 * K * (1 - K)) < 0.02


def test_mask_deterministic_and_sensitive_to_seed_and_offset():
    a = reference.hidden_dropout_mask(32, 128, 0.5, 11, 4)
    assert torch.equal(a, reference.hidden_dropout_mask(32, 128, 0.5, 11, 4))
    assert not torch.equal(a, reference.hidden_dropout_mask(32, 128, 0.5, 11, 8))               # offset
    assert not torch.equal(a, reference.hidden_dropout_mask(32, 128, 0.5, 11, 4 + (1 << 32)))   # offset, high word
    assert not torch.equal(a, reference.hidden_dropout_mask(32, 128, 0.5, 12, 4))               # seed
    for bad in (0.999, 1.0, -0.1):
        with pytest.raises(ValueError):
            reference.hidden_dropout_mask(1, 16, bad, 0, 0)


class _FakeGen:
    def __init__(self, seed, offset):
        self.seed, self.offset = seed, offset

    def initial_seed(self):
        return self.seed

    def get_offset(self):
        return self.offset

    def set_offset(self, v):
        self.offset = v


def test_default_rng_advances_the_generator_by_four_per_call():
    gen = _FakeGen(2 ** 63 + 5, 40)
    t = torch.zeros(1)
    p, seed, off = ops._dropout_args(t, 0.1, None, gen=gen)
    assert (p, seed, off) == (0.1, 5 - 2 ** 63, 40) and gen.offset == 44    # seed as a signed 64-bit value
    assert ops._dropout_args(t, 0.1, None, gen=gen)[2] == 44 and gen.offset == 48
    assert ops._dropout_args(t, 0.1, (9, 12), gen=gen) == (0.1, 9, 12) and gen.offset == 48   # pinned: no draw
    assert ops._dropout_args(t, 0.0, None, gen=gen) == (0.0, 0, 0) and gen.offset == 48       # no dropout: no draw
    with pytest.raises(ValueError):
        ops._dropout_args(t, 0.999, None, gen=gen)


@pytest.mark.parametrize("rms", [False, True])
def test_cpu_norm_with_dropout_composes_f_dropout(rms):
    torch.manual_seed(0)
    x, r = torch.randn(6, 64), torch.randn(6, 64)
    w, b = torch.rand(64) + 0.5, torch.randn(64)
    assert not ops.hidden_dropout_supported(x, 64, 0.1)

    def norm(**kw):
        return ops.rms_norm(x, w, residual=r, **kw) if rms else ops.layer_norm(x, w, b, residual=r, **kw)

    y0, s0 = norm()
    y1, s1 = norm(dropout_p=0.0)
    assert torch.equal(y0, y1) and torch.equal(s0, s1)
    y, s = norm(dropout_p=0.5)
    assert y.shape == x.shape and not torch.equal(s, s0)
    dropped = s == r
    assert 0 < int(dropped.sum()) < x.numel()
    torch.testing.assert_close(s[~dropped], (r + 2 * x)[~dropped])
    with pytest.raises(ValueError):
        ops.layer_norm(x, w, b, dropout_p=0.1)                       # no residual
    with pytest.raises(ValueError):
        ops.layer_norm(x, w, b, fork=True, dropout_p=0.1)


def test_cpu_dropout_add_composes_f_dropout():
    torch.manual_seed(0)
    x, r = torch.randn(6, 64), torch.randn(6, 64)
    assert torch.equal(ops.dropout_add(x, r, 0.0), x + r) and torch.equal(ops.dropout_add(x, None, 0.0), x)
    o = ops.dropout_add(x, r, 0.5)
    dropped = o == r
    assert 0 < int(dropped.sum()) < x.numel()
    torch.testing.assert_close(o[~dropped], (r + 2 * x)[~dropped])
    o = ops.dropout_add(x, None, 0.5)
    assert 0 < int((o == 0).sum()) < x.numel()


def test_modules_take_dropout_p_in_training_mode_only():
    from madnn.nn.norm import FusedLayerNorm, FusedRMSNorm

    torch.manual_seed(0)
    x, r = torch.randn(4, 32), torch.randn(4, 32)
    for m in (FusedLayerNorm(32), FusedRMSNorm(32)):
        m.eval()
        y0, s0 = m(x, residual=r)
        y1, s1 = m(x, residual=r, dropout_p=0.5)
        assert torch.equal(y0, y1) and torch.equal(s0, s1)
        m.train()
        assert not torch.equal(m(x, residual=r, dropout_p=0.5)[1], s0)


@pytest.mark.parametrize("name", ["gpt2", "bert"])
def test_cpu_models_with_hidden_dropout_train_and_eval(name):
    from madnn.models import bert, gpt2

    torch.manual_seed(0)
    if name == "gpt2":
        model = gpt2.GPT2(gpt2.gpt2_config("gpt2-tiny", n_layer=2, dropout=0.1))
    else:
        model = bert.BertForPreTraining(bert.bert_config("bert-tiny", layers=2, dropout=0.1))
    ids = torch.randint(0, 512, (2, 16))
    model.train()
    torch.manual_seed(1)
    a = model(ids)
    torch.manual_seed(1)
    assert torch.equal(a, model(ids))
    a.float().sum().backward()
    model.eval()
    assert torch.equal(model(ids), model(ids)) and not torch.equal(model(ids), a)
