"""GPU: the kernel path every chain's run takes (Plan.path, lte_run_path: nothing
is launched) equals the one recorded in tests/golden/run_paths.json before the
chains' traits moved into one table.  Every chain in its smallest legal antenna
set, crossed with precision, channel, modulation and three numerologies; the
coded chains also with an LLR capture (the switch from the (z, nv) hand-off to
LLRs); one HARQ plan at round 0."""
import itertools
import json
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

RUN_PATHS = os.path.join(ROOT, 'tests', 'golden', 'run_paths.json')

# chain value -> the antenna keywords of its smallest legal set
ANTENNAS = {
    0: dict(),                                                    # LTE_CHAIN_UNCODED 1x1
    1: dict(),                                                    # LTE_CHAIN_CODED 1x1
    2: dict(num_rx=2),                                            # LTE_CHAIN_SIMO 1x2
    3: dict(num_tx=2, num_rx=2),                                  # LTE_CHAIN_SFBC 2x2
    4: dict(num_tx=2, num_rx=2),                                  # LTE_CHAIN_SFBC_CODED 2x2
    5: dict(num_tx=2, num_rx=2, rank=2, precoder=np.eye(2)),      # LTE_CHAIN_SPATIAL 2x2 rank 2, MMSE
    6: dict(num_tx=2, num_rx=1),                                  # LTE_CHAIN_BEAMFORMING 2x1
    7: dict(num_rx=2),                                            # LTE_CHAIN_SIMO_CODED 1x2
    8: dict(num_tx=2, num_rx=2, rank=2, precoder=np.eye(2)),      # LTE_CHAIN_SPATIAL_CODED 2x2 rank 2, MMSE
    9: dict(num_rx=2),                                            # LTE_CHAIN_SCFDM_CODED 1x2
}
CODED = (1, 4, 7, 8, 9)
NUMEROLOGIES = ((128, 72, 9), (1024, 600, 72), (2048, 1200, 144))
SNR_DB = 10.0


def collect():
    """case id -> Plan.path(...) dictionary, over the whole cross product."""
    from lte_phy import _capi as C, engine
    C.device_init()
    out = {}

    def record(key, **kw):
        plan = engine.Plan(max_frames=1, fs=15000.0 * kw['N'], **kw)
        coded = kw['chain'] in CODED
        out[key] = plan.path(SNR_DB)
        if coded:
            out[key + '/llr'] = plan.path(SNR_DB, capture=('llr',))
        del plan

    for chain, prec, ray, bps, (N, Nc, cp) in itertools.product(sorted(ANTENNAS), ('f64', 'f32'), (0, 1), (2, 6),
                                                                 NUMEROLOGIES):
        kw = dict(N=N, Nc=Nc, cp_len=cp, bps=bps, chain=chain, precision=prec, detector=C.DET_MMSE,
                  channel=C.CH_RAYLEIGH if ray else C.CH_AWGN, **ANTENNAS[chain])
        if ray:   # two-tap static Rayleigh
            kw.update(delays=(0, 2), gains=(0.8, 0.6), fD=0.0)
        kw.update(dict(n_sym=0, n_bits=435) if chain in CODED else dict(n_sym=2, n_bits=100))
        record(f'chain{chain}/{prec}/{"rayleigh" if ray else "awgn"}/bps{bps}/N{N}', **kw)
    plan = engine.Plan(N=128, Nc=72, cp_len=9, bps=2, n_sym=0, n_bits=435, chain=C.CHAIN_CODED, channel=C.CH_AWGN,
                       fs=15000.0 * 128, max_frames=1, precision='f64', harq=dict(max_tx=2, rv_seq=(0, 2)))
    plan.harq_round(0)
    out['chain1/harq/round0'] = plan.path(SNR_DB)
    del plan
    return out


def test_every_chain_takes_its_recorded_path():
    want = json.load(open(RUN_PATHS))
    got = collect()
    assert sorted(got) == sorted(want) and len(got) == 240 + 120 + 1
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, (len(diff), dict(itertools.islice(diff.items(), 5)))
