"""--diffaug without a GPU: the Philox generator, the parameter draws, the torch reference of the transform and
its closed-form transpose (dsgan_hip/diffaug.py), the policy parser and the flag."""
import numpy as np
import pytest
import torch

from dsgan_hip import diffaug as DA

FULL = "color,translation,cutout"


def test_philox_known_answers():
    # Random123's kat_vectors for philox4x32-10: counter, key -> output
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(w) for w in DA.philox4x32_10(ctr, key)) == want
    # vectorised over the first counter word: row i is the scalar call with c0 = i
    rows = DA.philox4x32_10((np.arange(5), 1, 7, 9), (20, 0))
    assert rows.shape == (5, 4) and rows.dtype == np.uint32
    for i in range(5):
        assert np.array_equal(rows[i], DA.philox4x32_10((i, 1, 7, 9), (20, 0)))


def _table(*a):
    """The packed [n, 8] table of a draw as int32 bit patterns (a negative integer's pattern is a NaN as a float)."""
    return DA.pack_params(DA.draw_params(*a)).view(np.int32)


def test_draw_is_keyed_by_seed_stream_call_and_sample():
    base = _table(20, 0xFFFF, 3, 8, 16, 24)
    assert np.array_equal(base, _table(20, 0xFFFF, 3, 8, 16, 24))
    for other in ((21, 0xFFFF, 3), (20, 0x1FFFF, 3), (20, 0xFFFF, 4), (20 + (1 << 32), 0xFFFF, 3)):
        assert not np.array_equal(base, _table(*other, 8, 16, 24))
    # the call enters with its low 32 bits; a longer draw extends a shorter one
    assert np.array_equal(base, _table(20, 0xFFFF, 3 + (1 << 32), 8, 16, 24))
    assert np.array_equal(base[:5], _table(20, 0xFFFF, 3, 5, 16, 24))
    want = DA.draw_params(20, 0xFFFF, 3, 8, 16, 24)
    back = DA.unpack_params(base.view(np.float32))
    assert all(np.array_equal(back[f], want[f]) and back[f].dtype == want[f].dtype for f in DA.PARAM_FIELDS)
    assert (want["tx"] < 0).any()   # the bit patterns carry signs


@pytest.mark.parametrize("H,W", [(16, 24), (10, 13)])
def test_draw_ranges(H, W):
    p = DA.draw_params(20, 0xFFFF, 0, 4096, H, W)
    assert p["b"].dtype == p["s"].dtype == p["c"].dtype == np.float32 and p["tx"].dtype == np.int32
    assert p["b"].min() >= -0.5 and p["b"].max() < 0.5
    assert p["s"].min() >= 0.0 and p["s"].max() < 2.0
    assert p["c"].min() >= 0.5 and p["c"].max() < 1.5
    Sx, Sy, ch, cw = DA.geometry(H, W)
    assert (Sx, Sy, ch, cw) == (int(np.floor(W / 8 + 0.5)), int(np.floor(H / 8 + 0.5)),
                                int(np.floor(H / 2 + 0.5)), int(np.floor(W / 2 + 0.5)))
    assert sorted(set(p["tx"].tolist())) == list(range(-Sx, Sx + 1))
    assert sorted(set(p["ty"].tolist())) == list(range(-Sy, Sy + 1))
    assert sorted(set(p["oy"].tolist())) == list(range(0, H + 1 - ch % 2))   # [0, H] for an even cutout, [0, H) odd
    assert sorted(set(p["ox"].tolist())) == list(range(0, W + 1 - cw % 2))
    # the three colour draws are spread over their ranges, not stuck in a corner
    for f, lo in (("b", -0.5), ("s", 0.0), ("c", 0.5)):
        width = 2.0 if f == "s" else 1.0
        hist = np.histogram(p[f], bins=8, range=(lo, lo + width))[0]
        assert hist.min() > 4096 / 8 * 0.8, (f, hist)


def _x(n, C, H, W, dtype=torch.float64, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, C, H, W), generator=g, dtype=torch.float64).to(dtype)


def test_each_op_off_is_the_identity():
    H, W = 10, 13
    p = DA.draw_params(20, 3, 5, 4, H, W)
    x = _x(4, 4, H, W)
    assert torch.equal(DA.augment_reference(x, 1, "", p), x)
    ident = {"b": np.zeros(4, np.float32), "s": np.ones(4, np.float32), "c": np.ones(4, np.float32),
             "tx": np.zeros(4, np.int32), "ty": np.zeros(4, np.int32)}
    full = DA.augment_reference(x, 1, FULL, p)
    for op, fields in (("color", ("b", "s", "c")), ("translation", ("tx", "ty")), ("cutout", ())):
        rest = ",".join(o for o in DA.OPS if o != op)
        off = DA.augment_reference(x, 1, rest, p)
        assert not torch.equal(off, full), op
        if fields:   # leaving an op out of the policy == running it with its identity parameters
            q = dict(p, **{f: ident[f] for f in fields})
            assert torch.allclose(DA.augment_reference(x, 1, FULL, q), off, rtol=0, atol=1e-14), op
    # the condition channels: never recoloured, moved and cut with the image
    col = DA.augment_reference(x, 1, "color", p)
    assert torch.equal(col[:, :1], x[:, :1]) and not torch.equal(col[:, 1:], x[:, 1:])
    assert torch.equal(DA.augment_reference(x, 1, "translation,cutout", p)[:, 1:],
                       DA.augment_reference(x[:, 1:], 0, "translation,cutout", p))


def test_translation_and_cutout_by_hand():
    H, W = 4, 6   # Sx = 1, Sy = 1, ch = 2, cw = 3
    x = torch.arange(1, H * W + 1, dtype=torch.float64).reshape(1, 1, H, W)
    p = {"b": [0.0], "s": [1.0], "c": [1.0], "tx": [1], "ty": [-1], "oy": [0], "ox": [6]}
    y = DA.augment_reference(x, 0, "translation", p)[0, 0]
    assert y[0].tolist() == [0, 7, 8, 9, 10, 11] and y[3].tolist() == [0] * 6    # y[r, q] = x[r + 1, q - 1]
    z = DA.augment_reference(x, 0, "cutout", p)[0, 0]
    assert DA.cutout_box(0, 6, H, W) == (0, 1, 5, 6)   # rows [-1, 1), columns [5, 8), clipped
    want = x[0, 0].clone()
    want[0, 5] = 0
    assert torch.equal(z, want)


@pytest.mark.parametrize("H,W", [(16, 24), (10, 13)])
@pytest.mark.parametrize("Ca,Cb", [(0, 3), (1, 3), (3, 1)])
def test_autograd_equals_the_closed_form_transpose(H, W, Ca, Cb):
    n = 6
    p = DA.draw_params(20, 0xFFFF, 9, n, H, W)
    for policy in (FULL, "color", "translation,cutout"):
        x = _x(n, Ca + Cb, H, W, seed=1).requires_grad_(True)
        y = DA.augment_reference(x, Ca, policy, p)
        dy = _x(n, Ca + Cb, H, W, seed=2)
        (g,) = torch.autograd.grad(y, x, dy)
        cf = DA.backward_closed_form(dy, Ca, policy, p)
        assert (g[:, Ca:] - cf).abs().max().item() <= 1e-13 * max(1.0, cf.abs().max().item()), policy


def test_mean_is_the_input_mean_plus_brightness():
    """Saturation keeps every pixel's channel mean, so contrast's M needs one reduction over the input only."""
    H, W = 10, 13
    p = DA.draw_params(20, 0, 0, 3, H, W)
    x = _x(3, 3, H, W)
    y = DA.augment_reference(x, 0, "color", p)
    for j in range(3):
        b, c = float(p["b"][j]), float(p["c"][j])
        M = x[j].mean().item() + b
        assert abs(y[j].mean().item() - M) < 1e-13        # contrast keeps the sample mean, too
        u = x[j] + b
        m = u.mean(0, keepdim=True)
        want = ((u - m) * float(p["s"][j]) + m - M) * c + M
        assert torch.allclose(y[j], want, rtol=0, atol=1e-13)


def test_parse_policy():
    assert DA.parse_policy("") == () and DA.parse_policy(None) == ()
    assert DA.parse_policy(FULL) == DA.OPS
    assert DA.parse_policy("cutout, color") == ("color", "cutout")   # applied in the fixed order
    assert DA.policy_bits("translation,cutout") == 6 and DA.policy_bits("") == 0 and DA.policy_bits(FULL) == 7
    assert DA.policy_string(("cutout", "color")) == "color,cutout"
    with pytest.raises(ValueError, match="rotation"):
        DA.parse_policy("color,rotation")
    with pytest.raises(ValueError, match="'cutout'.*more than once"):
        DA.parse_policy("cutout,color,cutout")


def test_the_flag():
    from options.train_options import default_train_opt
    assert default_train_opt().diffaug == ""
    assert default_train_opt(diffaug="cutout,color").diffaug == "color,cutout"
    assert default_train_opt(["--diffaug", FULL]).diffaug == FULL
    with pytest.raises(ValueError, match="bogus"):
        default_train_opt(diffaug="bogus")
    with pytest.raises(SystemExit):
        default_train_opt(["--diffaug", "bogus"])
