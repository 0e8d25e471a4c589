"""Both feeds of TRAIN's per-item draws against tests/golden/roi_draws.json, recorded before the draw, the collate of draws and the
resident feed shared one code path: ``draw_items`` (TRAIN --resident) and ``NeustonDataset.__getitem__`` + ``collate_rois`` (the loaders)
consume the random streams they consumed then and build the entries they built then."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_roi_draws as mrd          # noqa: E402

with open(mrd.GOLDEN) as fh:
    GOLDEN = json.load(fh)


@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('roi_draws'))
    mrd.write_images(tmp)
    return tmp


def test_the_fixture_covers_every_setting():
    assert sorted(GOLDEN) == sorted(mrd.SETTINGS)
    for rec in GOLDEN.values():
        assert [len(b['flips']) for b in rec['draw_items']] == list(mrd.BATCHES) == [len(b['flips']) for b in rec['collate']]
    full = GOLDEN['flip xy rot90 jitter 0.4,0.3 blur 2.0 prob 0.5']['draw_items'][0]
    assert sorted(full) == ['blur', 'brightness', 'contrast', 'flips', 'turn'] and set(GOLDEN['none']['collate'][0]) == {'flips'}


@pytest.mark.parametrize('name', sorted(mrd.SETTINGS))
def test_both_feeds_reproduce_the_recorded_draws(folder, name):
    got = mrd.record(name, folder)
    assert got['draw_items'] == GOLDEN[name]['draw_items']
    assert got['collate'] == GOLDEN[name]['collate']
    assert got['collate'] == got['draw_items']                       # one stream, two feeds
