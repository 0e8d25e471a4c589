"""The op tables of the default plans and of every surviving plan switch are pinned (CPU, Engine(plan_only=True)): each
configuration of tests/golden/make_plan_fingerprints.py is rebuilt and its fingerprint -- kind, flags with lane and wait bits,
tag, i[], f[], descriptor bytes, resolved kernel name and symbolic pointers of every op of all 13 programs -- compared with
tests/golden/plan_fingerprints.json.  A refactor of the plan builder or of the library's planning helpers must leave them equal.

The eval conv + folded BatchNorm + ReLU + max-pool fusion (OP_CONV_FWD_AFFINE_MAXPOOL) is planned here as on a device (its one
library call is a host function); tests/test_gpu_plan_fingerprint.py holds a device engine's plans to the same golden."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_plan_fingerprints as mpf  # noqa: E402


def test_golden_covers_every_configuration():
    with open(mpf.GOLDEN) as fh:
        assert sorted(json.load(fh)) == sorted(mpf.CONFIGS)


@pytest.mark.parametrize('cfg', sorted(mpf.CONFIGS))
def test_plan_fingerprint_matches_golden(cfg):
    with open(mpf.GOLDEN) as fh:
        want = json.load(fh)[cfg]
    assert mpf.fingerprint(cfg) == want, '%s: the op tables changed (tests/golden/make_plan_fingerprints.py regenerates)' % cfg
