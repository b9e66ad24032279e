"""tools/photcal_probe.py end to end at a small size: the child runs both routes on the GPU and the document carries
every figure DESIGN.md quotes from profiles/photcal_probe.json."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_probe_measures_both_routes(tmp_path):
    spec = importlib.util.spec_from_file_location('photcal_probe', os.path.join(ROOT, 'tools', 'photcal_probe.py'))
    probe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    out = str(tmp_path / 'probe.json')
    assert probe.main(['--out', out, '--naxis', '256', '--nstars', '40', '--warmup', '1', '--repeat', '2', '--limit', '120']) == 0
    doc = json.load(open(out))
    m = doc['measured']
    for k in ('new_growth', 'new_clipped_medians', 'old_seven_aperture_launches', 'old_host_annulus_medians'):
        assert m[k]['median_ms'] > 0
    assert m['new_total_ms'] > 0 and m['old_total_ms'] > 0
    # the two routes find the same sky where nothing is bad: the host medians take every annulus pixel, the kernel leaves
    # out the masked ones, so only a loose agreement is asked here
    assert m['check']['stars_with_flags_0'] > 0 and m['check']['largest_sky_difference_from_the_host_medians'] < 2.0
    assert doc['naxis'] == 256 and doc['nstars'] == 40
