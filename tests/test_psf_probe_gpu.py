"""tools/psf_probe.py end to end at a reduced size: every step runs in its child and the document carries every key
DESIGN.md quotes from profiles/psf_probe.json."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_probe_runs_every_step_and_writes_every_key(tmp_path):
    spec = importlib.util.spec_from_file_location('psf_probe', os.path.join(ROOT, 'tools', 'psf_probe.py'))
    probe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    out = str(tmp_path / 'probe.json')
    assert probe.main(['--out', out, '--naxis', '256', '--nstars', '40', '--nimg', '2', '--nsrc', '2000', '--nref', '5',
                       '--reps', '2', '--step-timeout', '120']) == 0
    doc = json.load(open(out))
    assert set(probe.STEPS) <= set(doc) and 'not_measured' in doc and doc['psf_over_aperture'] > 0
    b = doc['build']
    assert b['wall_median_ms'] > 0 and abs(b['model_sum'] - 1.0) < 1e-12 and b['nstars'] == 40 and b['n_used_median'] > 3
    for k, ev in (('psf', 'psf_batch'), ('aperture', 'lc_batch')):
        assert doc[k]['wall_median_ms'] > 0 and doc[k]['event_ms'][ev] > 0 and doc[k]['npairs'] == doc['psf']['npairs'] > 0
    assert doc['psf']['check']['finite'] > 0
    assert doc['numpy']['npos'] == 5 == doc['numpy']['finite'] and doc['numpy']['ms_per_position'] > 0
