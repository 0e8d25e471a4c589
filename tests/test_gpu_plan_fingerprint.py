"""An engine with a device plans what Engine(plan_only=True) plans: for three configurations of tests/golden/make_plan_fingerprints.py
the op tables a device engine builds -- same cleaned environment, train_batch at its default -- have the fingerprint that
tests/golden/plan_fingerprints.json pins for the CPU.  Every pointer of the text is symbolic (owner, byte offset), so nothing of the
device's addresses enters it; the batch-64 configuration is the one whose grouped weight gradients grow the workspace while the plan
is built, which a plan_only engine skips.  Nothing is launched."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_plan_fingerprints as mpf  # noqa: E402


@pytest.mark.parametrize('cfg', ['inception_v3-bf16-b2', 'resnet50-bf16-b4', 'inception_v3-bf16-b64'])
def test_a_device_engine_plans_what_the_cpu_golden_pins(cfg):
    import hashlib
    from ifcb_classifier_amd import _lib
    with open(mpf.GOLDEN) as fh:
        want = json.load(fh)[cfg]
    eng, pl = mpf.build_plan(cfg, plan_only=False)
    try:
        assert not eng.plan_only and eng.train_batch == mpf.CONFIGS[cfg][2]
        if cfg.endswith('-b64'):
            assert pl.bwd.find(_lib.OP_CONV_WGRAD_GROUP), 'no grouped weight gradient in the batch-64 plan'
        got = hashlib.sha256(mpf.plan_text(eng, pl).encode()).hexdigest()
    finally:
        eng.close()
    assert got == want, '%s: a device engine plans other op tables than Engine(plan_only=True)' % cfg
