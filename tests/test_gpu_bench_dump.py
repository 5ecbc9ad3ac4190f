"""GPU: `bench.py --dump-outputs` writes what the timed path returned in its
last step.  A plain (lean) run at a small batch, in a child process; the
dumped arrays equal the same frame ids run through the same plan here, so two
builds of the library can be compared output for output."""
import importlib.util
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(ROOT, 'bench.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


@pytest.mark.gpu
def test_plain_bench_dumps_the_last_timed_step(tmp_path):
    F, steps = 192, 2          # three 64-frame decoder groups, every SNR point 12 times
    e = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps),
                        '--warmup', '1', '--frames', str(F), '--dump-outputs', str(tmp_path)],
                       env=e, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(line) == 1, r.stdout
    out = json.loads(line[0])
    # lean: the legs with runs of their own stay behind --full
    assert out['full'] is False and out['cpu_baseline'] is None and out['ber_match'] is None
    assert out['steps'] == steps and out['ms_per_step'] > 0 and out['dtype'] == 'f64'
    assert abs(out['value'] - F / (out['ms_per_step'] * 1e-3)) <= 1e-3 * out['value'] + 0.1
    assert out['roofline']['hbm_row_stream']['store_cost']['measured_in_this_run'] is False
    assert sorted(os.listdir(tmp_path)) == ['counts.npy', 'crc_ok.npy', 'frame_errors.npy']

    b = _bench()
    from lte_phy import dist as D
    plan = b.make_plan(2, types.SimpleNamespace(frames=F, precision='f64', velocity=0.0, iters=8, channel=None))
    ids = D.frame_ids(steps - 1, 0, 1, F)
    si = D.snr_index(ids, len(b.SNRS))
    ref = plan.run(b.SNRS[si], snr_index=si, n_snr=len(b.SNRS), seed=b.SEED, frame_ids=ids)
    for name in ('counts', 'frame_errors', 'crc_ok'):
        got = np.load(tmp_path / (name + '.npy'))
        assert got.dtype == np.float64 and got.shape == ref[name].shape
        assert np.array_equal(got, ref[name].astype(np.float64)), name
    assert ref['frame_errors'].sum() > 0 and ref['crc_ok'].sum() > 0      # both sides of the cliff
