"""CPU: the float64 oracle against the round-7 reference goldens
(tests/golden/make_golden_r7.py): the 8-tap ITU profiles, Pedestrian_B, the
extended CP, delta_f = 7.5 kHz, 15 / 2.5 / 1.25 MHz with max_delay == cp, and a
moving UE on 8 taps, each through the reference's own simulate_siso /
simulate_simo / simulate_siso_coded on its own global RNG.  All exact: bit
errors, received bits, PAPR, the stored slices of the received stream and of
the equalised symbols to the last bit, and the global RNG state afterwards."""
import os

import numpy as np
import pytest

from conftest import ROOT, unpack

GOLDEN_R7 = os.path.join(ROOT, 'tests', 'golden', 'golden_r7.npz')
HEAD, TAIL = 320, 64      # make_golden_r7.py's stream slices

# name, call, Numerology kwargs, profile, velocity (km/h at 2 GHz), SNRs, num_rx -- make_golden_r7.py's POINTS
POINTS = [
    ('siso_vb20', 'siso', dict(bandwidth=20.0, modulation='64-QAM'), 'Vehicular_B', 0, [17.4], 1),
    ('siso_bu20', 'siso', dict(bandwidth=20.0, modulation='64-QAM'), 'Bad_Urban', 0, [11.8], 1),
    ('siso_pb15x', 'siso', dict(bandwidth=15.0, modulation='16-QAM', cp_type='extended'), 'Pedestrian_B', 0,
     [14.2], 1),
    ('siso_vb125', 'siso', dict(bandwidth=1.25, modulation='QPSK'), 'Vehicular_B', 0, [6.5], 1),
    ('siso_pb25h', 'siso', dict(bandwidth=2.5, delta_f=7.5, modulation='QPSK'), 'Pedestrian_B', 0, [4.1], 1),
    ('simo4_pb10', 'simo', dict(bandwidth=10.0, modulation='16-QAM'), 'Pedestrian_B', 0, [9.3], 4),
    ('simo4_vb10', 'simo', dict(bandwidth=10.0, modulation='16-QAM'), 'Vehicular_B', 0, [9.3], 4),
    ('simo4_vb10x', 'simo', dict(bandwidth=10.0, modulation='16-QAM', cp_type='extended'), 'Vehicular_B', 0,
     [9.3], 4),
    ('simo4_pb10x', 'simo', dict(bandwidth=10.0, modulation='16-QAM', cp_type='extended'), 'Pedestrian_B', 0,
     [9.3], 4),
    ('simo2_q10hx', 'simo', dict(bandwidth=10.0, delta_f=7.5, modulation='QPSK', cp_type='extended'),
     'Pedestrian_A', 0, [2.7], 2),
    ('cod_vb20', 'coded', dict(bandwidth=20.0, modulation='64-QAM'), 'Vehicular_B', 0, [9.7, 22.3], 1),
    ('cod_bu5x', 'coded', dict(bandwidth=5.0, modulation='16-QAM', cp_type='extended'), 'Bad_Urban', 0,
     [4.4, 15.1], 1),
    ('siso_vb20_v3', 'siso', dict(bandwidth=20.0, modulation='64-QAM'), 'Vehicular_B', 3, [21.6], 1),
]
CASES = [(p, snr) for p in POINTS for snr in p[5]]


@pytest.fixture(scope='module')
def golden_r7():
    return np.load(GOLDEN_R7, allow_pickle=False)


def _state_head():
    return np.array(np.random.get_state()[1][:8], dtype=np.uint32)


def _ends(a):
    a = np.asarray(a).reshape(-1)
    return np.concatenate([a[:HEAD], a[-TAIL:]])


def test_points_cover_the_new_corners(oracle):
    """The numerology the goldens were taken at (the issue's table): odd and
    long CPs, max_delay == cp with two taps on one sample, 8 taps."""
    n = {p[0]: oracle.Numerology(**p[2]) for p in POINTS}
    assert (n['siso_pb15x'].N, n['siso_pb15x'].Nc, n['siso_pb15x'].cp) == (2048, 900, 509)
    assert (n['simo4_vb10x'].cp, n['simo2_q10hx'].cp, n['cod_bu5x'].cp) == (254, 253, 127)
    assert (n['siso_pb25h'].N, n['siso_pb25h'].fs, n['siso_pb25h'].cp) == (256, 1.92e6, 9)
    dl, g = oracle.itu_paths(n['siso_vb125'], 'Vehicular_B')
    assert len(dl) == 8 and max(dl) == n['siso_vb125'].cp == 9 and len(set(dl)) == 7
    dl, _ = oracle.itu_paths(n['simo4_vb10'], 'Vehicular_B')
    assert max(dl) == 70
    assert len(oracle.itu_paths(n['siso_bu20'], 'Bad_Urban')[0]) == 8


@pytest.mark.parametrize('point,snr', CASES, ids=[f'{p[0]}-{s}' for p, s in CASES])
def test_oracle_equals_reference(golden_r7, oracle, point, snr):
    name, call, nkw, prof, vel, _, nrx = point
    g = golden_r7
    num = oracle.Numerology(**nkw)
    nb = int(g[name + '_nbits'][0])
    bits = unpack(g[name + '_bits'], nb).astype(np.int64)
    assert np.array_equal(bits, np.random.RandomState(7).randint(0, 2, nb))
    fD = oracle.doppler_hz(2.0, vel) if vel else 0.0
    k = f'{name}_snr{snr}'
    if call == 'siso':
        r = oracle.simulate_siso(num, bits, snr, 'rayleigh_mp', profile=prof, fD=fD)
        sig, sym = _ends(r['signal_rx']), _ends(r['symbols_rx'])
    elif call == 'simo':
        r = oracle.simulate_simo(num, bits, snr, num_rx=nrx, channel='rayleigh_mp', profile=prof, fD=fD)
        sig, sym = np.stack([_ends(y) for y in r['signal_rx_list']]), _ends(r['symbols_rx_combined'])
    else:
        r = oracle.simulate_siso_coded(num, bits, snr, 'rayleigh_mp', profile=prof, fD=fD)
        sig, sym = _ends(r['signal_rx']), _ends(r['symbols_rx'])
        assert int(r['crc_pass']) == int(g[k + '_crc'][0])
        assert r['channel_snr_db'] == g[k + '_chsnr'][0]
        assert r['noise_var_mean'] == g[k + '_nvmean'][0]
    assert r['bit_errors'] == int(g[k + '_errors'][0])
    assert np.array_equal(r['bits_received_array'], unpack(g[k + '_rx'], nb))
    assert r['papr_db'] == g[k + '_papr'][0]
    assert np.array_equal(sig, g[k + '_sigrx'])
    assert np.array_equal(sym, g[k + '_symrx'])
    assert np.array_equal(_state_head(), g[k + '_state']), 'global RNG side effects differ'


def test_coded_points_decode_and_fail(golden_r7):
    """The coded goldens hold a frame the reference decodes and one it does not."""
    crc = {k: int(golden_r7[k][0]) for k in golden_r7.files if k.endswith('_crc')}
    assert 0 in crc.values() and 1 in crc.values(), crc
