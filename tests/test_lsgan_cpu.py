"""The LSGAN objective and the pixel / multi-scale discriminators, the parts that need no GPU: the
state_dict surface against the reference's (tests/golden/golden_v5.npz, written by
tests/golden/gen_golden_v5.py from DSGAN/models/networks.py:115-131, 533-699), construction of the
two least-squares losses, and the pairing the reference itself cannot train."""
import json
import os

import numpy as np
import pytest

G5 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v5.npz"))


@pytest.mark.parametrize("kind", ["basic", "pixel", "multi"])
def test_discriminator_keys_and_shapes(kind):
    from models.networks import define_D
    d = define_D(6, 32, kind, 3, "instance", True, "normal", [])
    sd = d.state_dict()
    assert list(sd.keys()) == list(G5["D5_%s_keys" % kind])
    assert [json.dumps(list(v.shape)) for v in sd.values()] == list(G5["D5_%s_shapes" % kind])


def test_default_basic_keys_unchanged():
    """use_sigmoid appends a parameter-free nn.Sigmoid as model.12: the keys are the default D's."""
    from models.networks import define_D
    plain = define_D(6, 32, "basic", 3, "instance", False, "normal", [])
    assert list(plain.state_dict().keys()) == list(G5["D5_basic_keys"])
    assert len(plain.model) == 12
    assert len(define_D(6, 32, "basic", 3, "instance", True, "normal", []).model) == 13


def test_multi_honours_n_layers_and_caps_channels():
    from models.networks import define_D
    d = define_D(6, 64, "multi", 5, "instance", True, "normal", [])
    sd = d.state_dict()
    idx = [0, 2, 5, 8, 11, 14, 17]
    assert list(sd.keys()) == ["layer%d.%d.%s" % (s, i, p) for s in range(3) for i in idx for p in ("weight", "bias")]
    assert [sd["layer0.%d.weight" % i].shape[0] for i in idx] == [64, 128, 256, 512, 512, 512, 1]
    assert all(m.padding == (2, 2) for m in d.layer1 if hasattr(m, "padding"))


def test_least_squares_losses_construct():
    from models.networks import GANLoss, GANLoss_multi
    assert GANLoss(True).use_lsgan and not GANLoss(False).use_lsgan
    assert GANLoss_multi(True).real_label == 1.0 and GANLoss_multi(True).fake_label == 0.0


def test_multi_without_sigmoid_raises():
    from models.networks import define_D, GANLoss_multi
    with pytest.raises(NotImplementedError, match="BCELoss"):
        define_D(6, 32, "multi", 3, "instance", False, "normal", [])
    with pytest.raises(NotImplementedError, match="BCELoss"):
        GANLoss_multi(False)
    for kind in ("multi", "pixel"):
        with pytest.raises(NotImplementedError, match="norm"):
            define_D(6, 32, kind, 3, "batch", True, "normal", [])
