"""Pinned output bits of the entry points whose host dispatch lives in instnorm.hip (one plane-size
ladder per direction) and of the two dsgan_mlp_bwd kernels that issue LDS-DMA through lds_dma.h.
tests/golden/csrc_bits_v1.json holds sha1 digests of their output bytes, recorded by
tests/golden/gen_csrc_bits.py from the library as it was before that code moved; the same cases are
recomputed here with the in-tree library.  There is no tolerance: every digest matches or the test fails."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_csrc_bits", os.path.join(GOLDEN, "gen_csrc_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def pinned():
    with open(gen.FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_group(pinned):
    assert sorted(pinned) == sorted(gen.GROUPS)
    assert all(pinned[g] for g in gen.GROUPS)


@pytest.mark.parametrize("group", gen.GROUPS)
def test_output_bits_are_pinned(pinned, group):
    from dsgan_hip import functional as HF
    from dsgan_hip import _lib
    prec = HF.get_precision()
    try:
        got = gen.compute(group)
    finally:
        HF.set_precision(prec)
        _lib.load().dsgan_mlp_tune(0, 2)
    want = pinned[group]
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, "%d of %d digests differ: %s" % (len(differ), len(want), differ)
