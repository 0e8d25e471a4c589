"""Per-seed spread of the end-to-end trained-weights measure: one fused fp32 step of resnet18, update distance to the
fp64 trajectory, HIP against the fp32 oracle, SGD and Adam, seeds 0..4.  Measures only; asserts nothing.  Needs a GPU.

    python scripts/e2e_seed_spread.py [BATCH ...]        (default: 8 16)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_gpu_trained_weights as T  # noqa: E402

for B in [int(a) for a in sys.argv[1:]] or [8, 16]:
    for opt in ('sgd', 'adam'):
        for seed in range(5):
            t = T._trajectories('resnet18', 2, B, 224, 'fp32', opt, steps=1, seed=seed, arbiter=True)[0]
            mh, mo = T._med(t['arb_h']), T._med(t['arb_o'])
            wh, wo = max(t['arb_h'].values()), max(t['arb_o'].values())
            print('batch %d %s seed %d: median HIP %.3e oracle %.3e ratio %.2f | worst tensor HIP %.3e oracle %.3e ratio %.2f | '
                  'arbitrated(ARB = %.1f) %s' % (B, opt, seed, mh, mo, mh / mo, wh, wo, wh / wo, T.ARB, T._arbitrated(t)), flush=True)
