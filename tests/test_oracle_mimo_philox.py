"""CPU: the oracle's Philox restatements for the multi-antenna chains
(oracle/philox.py bf_draws; the draws= / pmi= / paths= arguments of
oracle/bf_oracle.py, oracle/tm4_oracle.py and oracle/mimo_oracle.py) and the
preconditions of tests/test_gpu_mimo_philox.py, evaluated from the oracle alone.

(a) each new argument against code the reference goldens already pin
    (tests/test_oracle_bf.py, test_oracle_tm4.py, test_oracle_mimo.py): from the
    same seed, the draws= route on draws built from the global RNG in the
    reference's order returns bit-identical results to the draws=None route;
    paths= with the profile's own taps returns what the profile lookup returns;
    pmi=0 what the default route returns.
(b) bf_draws: the counters and outputs lte_bf.hip uses, from hand-made rng4 calls.
(c) for every case of tests/mimo_philox_cases.py: every slicer input at least
    the margin from every decision boundary (1e-9 of the spacing; spatial cases
    max(1e-9, r eps kappa / mu), SIC at every stage) with no RE exempted; the
    PMI choice of the beamforming cases not a near tie; uncoded cases reach
    from frames with errors to a nearly clean one, coded ones from a failed to a
    decoded one; r (mimo_philox_cases.R_SPATIAL) is the measurement; and the
    SFBC cases take both values of every dispatch predicate they exist for.
"""
import math

import numpy as np
import pytest

import mimo_philox_cases as K
from oracle import bf_oracle as BF
from oracle import lte_oracle as O
from oracle import mimo_oracle as MO
from oracle import philox as P
from oracle import tm4_oracle as T


def _state():
    return np.random.get_state()[1].copy(), np.random.get_state()[2]


def _same(a, b, keys):
    for k in keys:
        x, y = a[k], b[k]
        if isinstance(x, list):
            assert len(x) == len(y) and all(np.array_equal(u, v) for u, v in zip(x, y)), k
        else:
            assert np.array_equal(x, y), k


# ---------------------------------------------------------------------------
# (a) the new arguments against the pinned routes
@pytest.mark.parametrize('bw,mod,ntx,nrx,mode', [(1.25, 'QPSK', 2, 1, 'adaptive'), (5.0, '16-QAM', 4, 3, 'static'),
                                                 (5.0, '64-QAM', 8, 5, 'adaptive'), (1.25, '16-QAM', 8, 8, 'static')])
def test_beamforming_draws_route(bw, mod, ntx, nrx, mode):
    num = O.Numerology(bandwidth=bw, modulation=mod)
    bits = np.random.RandomState(3).randint(0, 2, 3 * num.Nd * num.bps - 5)
    np.random.seed(11)
    a = BF.simulate_beamforming(num, bits, 0.0, ntx, nrx, 'TM6', mode)
    st_a = _state()
    np.random.seed(11)
    d = BF.beamforming_draws(ntx, nrx, 3, num.Nd)
    st_d = _state()
    b = BF.simulate_beamforming(num, bits, 0.0, ntx, nrx, 'TM6', mode, draws=d)
    st_b = _state()
    _same(a, b, ('bits_received_array', 'bit_errors', 'channel_matrix', 'pmi_history', 'beamforming_gain_db',
                 'symbols_rx'))
    # the builder consumes what the driver consumes; the draws= route consumes nothing
    assert np.array_equal(st_a[0], st_d[0]) and st_a[1] == st_d[1]
    assert np.array_equal(st_d[0], st_b[0]) and st_d[1] == st_b[1]
    assert a['bit_errors'] > 0


SFBC_KEYS = ('bits_received_array', 'bit_errors', 'channel_matrix', 'signals_rx', 'symbols_rx', 'noise_power')


def _sfbc_built_draws(num, nrx, chan, L, n_paths):
    """The draws of the draws=None route: the global RNG as the transmitter's
    last pilot reseed (cell 1, TX1's pilots) leaves it."""
    O.pilots(1, len(num.pilot_idx[1::2]))
    return MO.transmit_mimo_draws(2, nrx, chan, L, n_paths=n_paths)


@pytest.mark.parametrize('coded', [False, True])
@pytest.mark.parametrize('chan,nrx,paths', [('rayleigh_mp', 2, None), ('awgn', 1, None),
                                            ('rayleigh_mp', 3, ((0, 5, 33), (1.0, 0.5, 0.25)))])
def test_sfbc_draws_and_paths_routes(chan, nrx, paths, coded):
    O.lib()
    num = O.Numerology(bandwidth=1.25, modulation='QPSK')
    sim = MO.simulate_sfbc_coded if coded else MO.simulate_sfbc
    keys = SFBC_KEYS + (('crc_pass', 'llrs', 'symbols_rx_grid') if coded else ())
    bits = np.random.RandomState(5).randint(0, 2, 200 if coded else 3 * (num.Nd & ~1) * 2 - 5)
    np.random.seed(21)
    a = sim(num, bits, 9.0, nrx, chan, 'Pedestrian_A', paths=paths)
    L = len(a['signals_rx'][0])
    dl, g = MO._paths(num, 'Pedestrian_A', paths)
    d = _sfbc_built_draws(num, nrx, chan, L, len(dl))
    b = sim(num, bits, 9.0, nrx, chan, 'Pedestrian_A', draws=d, paths=paths)
    _same(a, b, keys)
    # paths= with the profile's own taps is the profile lookup
    if paths is None:
        c = sim(num, bits, 9.0, nrx, chan, 'Pedestrian_A', draws=d, paths=O.itu_paths(num, 'Pedestrian_A'))
        _same(a, c, keys)
    else:       # and a custom tap set is not the profile
        c = sim(num, bits, 9.0, nrx, chan, 'Pedestrian_A',
                draws=_sfbc_built_draws(num, nrx, chan, L, 4))
        assert not np.array_equal(a['signals_rx'][0], c['signals_rx'][0])
    # the combined symbols are the slicer's input
    if not coded:
        assert np.array_equal(MO.hard_bits(a['symbols_rx'], 'QPSK')[:len(bits)], a['bits_received_array'])


def test_transmit_paths_routes():
    """transmit_mimo / transmit_sm / simulate_spatial: paths= with the profile's
    taps (the spatial chain's thrice-converted ones) is the profile route."""
    num = O.Numerology(bandwidth=1.25, modulation='QPSK')
    rs = np.random.RandomState(2)
    L = 2 * (num.N + num.cp)
    xs = [rs.randn(L) + 1j * rs.randn(L) for _ in range(2)]
    np.random.seed(4)
    ya, Ha = MO.transmit_mimo(num, xs, 2, 'rayleigh_mp', 12.0, 'Vehicular_A')
    np.random.seed(4)
    info = {}
    yb, Hb = MO.transmit_mimo(num, xs, 2, 'rayleigh_mp', 12.0, 'Vehicular_A', paths=O.itu_paths(num, 'Vehicular_A'),
                              info=info)
    assert all(np.array_equal(u, v) for u, v in zip(ya, yb)) and np.array_equal(Ha, Hb)
    assert info['noise_power'].shape == (2,)
    np.random.seed(4)
    ya, Ha = MO.transmit_sm(num, xs, 3, 'rayleigh_mp', 12.0, 'Vehicular_A', fD=5.0)
    np.random.seed(4)
    yb, Hb = MO.transmit_sm(num, xs, 3, 'rayleigh_mp', 12.0, 'Vehicular_A', fD=5.0,
                            paths=O.itu_paths(num, 'Vehicular_A', spatial=True), info=info)
    assert all(np.array_equal(u, v) for u, v in zip(ya, yb)) and np.array_equal(Ha, Hb)
    assert info['noise_power'].shape == (3,)
    bits = np.random.RandomState(7).randint(0, 2, 2 * num.Nd * 2)
    np.random.seed(9)
    a = MO.simulate_spatial(num, bits, 20.0, channel='rayleigh_mp')
    np.random.seed(9)
    b = MO.simulate_spatial(num, bits, 20.0, channel='rayleigh_mp',
                            paths=O.itu_paths(num, 'Pedestrian_A', spatial=True))
    _same(a, b, ('bits_received_array', 'bit_errors', 'signals_rx'))


TM4_ROUTES = [(4, 4, 4, 'MMSE', 'rayleigh_mp', 0), (4, 4, 2, 'SIC', 'awgn', 0), (4, 4, 2, 'SIC', 'awgn', 5),
              (4, 3, 3, 'ZF', 'rayleigh_mp', 0), (2, 2, 2, 'ZF', 'awgn', 1), (4, 2, 1, 'MRC', 'awgn', 3),
              (4, 4, 4, 'MMSE', 'awgn', 2)]
TM4_KEYS = ('bits_received_array', 'bit_errors', 'channel_matrix', 'precoder_matrix', 'rank', 'pmi_used', 'signals_rx',
            'symbols_rx', 'kappa', 'layers_rx', 'H_est', 'noise_power')


@pytest.mark.parametrize('ntx,nrx,rank,det,chan,pmi', TM4_ROUTES)
def test_tm4_draws_and_pmi_routes(ntx, nrx, rank, det, chan, pmi):
    num = O.Numerology(bandwidth=1.25, modulation='16-QAM')
    bits = np.random.RandomState(8).randint(0, 2, 2 * num.Nd * 4 - 5)
    kw = dict(num_tx=ntx, num_rx=nrx, rank=rank, detector=det, channel=chan, velocity_kmh=3, csi=False)
    np.random.seed(31)
    # pmi 0 is what the reference's fixed-rank route uses: the route the goldens pin
    a = T.simulate_tm4(num, bits, 8.0, **kw) if pmi == 0 else T.simulate_tm4(num, bits, 8.0, pmi=pmi, **kw)
    assert a['pmi_used'] == pmi and np.array_equal(a['precoder_matrix'], T.codebook(ntx, 'TM4', rank)[pmi])
    if pmi == 0:
        np.random.seed(31)
        _same(a, T.simulate_tm4(num, bits, 8.0, pmi=0, **kw), TM4_KEYS)     # H_initial is consumed all the same
    # the draws of that route: the global RNG as the transmitter's last pilot reseed leaves it
    pidx = MO.mimo_pilot_indices(num, ntx)
    O.pilots((ntx - 1) % 4, len(pidx[ntx - 1]))
    L = len(a['signals_rx'][0])
    d = MO.transmit_sm_draws(ntx, nrx, chan, L)
    np.random.seed(77)
    b = T.simulate_tm4(num, bits, 8.0, draws=d, pmi=pmi, **kw)
    _same(a, b, TM4_KEYS + (('sic_stages', 'sic_order') if det == 'SIC' else ()))
    # no H_initial: up to the transmitter's first pilot reseed the global RNG is untouched, so the
    # route's results cannot depend on it (the same results from another state)
    np.random.seed(78)
    _same(b, T.simulate_tm4(num, bits, 8.0, draws=d, pmi=pmi, **kw), TM4_KEYS)
    # the per-RE returns are the detector's: the layers demapped are the symbols, kappa is cond(A)
    n_sym, Nd = 2, num.Nd
    n_dsc = -(-Nd // rank)
    lay = b['layers_rx'].reshape(n_sym, n_dsc, rank)
    assert np.array_equal(lay.reshape(n_sym, n_dsc * rank)[:, :Nd].reshape(-1), b['symbols_rx'])
    He = b['H_eff']
    s2 = 10 ** (-8.0 / 10)
    if det != 'MRC':
        A = np.conj(np.swapaxes(He, 1, 2)) @ He + (0 if det == 'ZF' else s2) * np.eye(rank)
        assert np.array_equal(np.repeat(np.linalg.cond(A), rank).reshape(n_sym, -1)[:, :Nd].reshape(-1), b['kappa'])
    if det == 'SIC':     # every stage's slicer input slices to the decision the detector returns
        const = O.constellation('16-QAM')
        dec = const[np.argmin(np.abs(b['sic_stages'][:, :, None] - const[None, None, :]), axis=2)]
        got = np.take_along_axis(b['layers_rx'], b['sic_order'], axis=1)
        assert np.array_equal(dec, got)
    assert b['bit_errors'] > 0


# ---------------------------------------------------------------------------
# (b) bf_draws by hand
def _bm(a, b):
    u, v = (int(a) + 0.5) * 2.0 ** -32, (int(b) + 0.5) * 2.0 ** -32
    r, t = np.sqrt(-2.0 * np.log(u)), 6.283185307179586 * v
    return r * np.cos(t), r * np.sin(t)


@pytest.mark.parametrize('frame', [0, 2 ** 32 + 3, 65535])
def test_bf_draws_counters(frame):
    seed, ntx, nrx, n_sym, Nd = 0x5EED0123456789, 4, 3, 3, 62
    d = P.bf_draws(seed, frame, ntx, nrx, n_sym, Nd)
    assert d['H'].shape == (nrx, ntx) and d['z_re'].shape == d['z_im'].shape == (nrx, n_sym * Nd)
    # link (r = 2, t = 1): counter 0 of stream 0x40000 + 2 * 4 + 1, outputs (x, y), times 0.7071067811865475
    w = P.philox4x32_10(0, 0x40000 + 9, frame & 0xFFFFFFFF, frame >> 32, seed & 0xFFFFFFFF, seed >> 32)
    re, im = _bm(w[0], w[1])
    assert d['H'][2, 1] == complex(re * 0.7071067811865475, im * 0.7071067811865475)
    assert P.STREAM_BF == 0x40000 and P.STREAM_NOISE == 0x10000
    # noise sample n = l * Nd + j of RX r = 1: counter n // 2 of stream 0x10000 + 1; even n (x, y), odd n (z, w)
    for l, j in ((0, 0), (1, 7), (2, 61), (2, 60)):
        n = l * Nd + j
        w = P.philox4x32_10(n // 2, 0x10000 + 1, frame & 0xFFFFFFFF, frame >> 32, seed & 0xFFFFFFFF, seed >> 32)
        re, im = _bm(w[2], w[3]) if n & 1 else _bm(w[0], w[1])
        assert (d['z_re'][1, n], d['z_im'][1, n]) == (re, im), (l, j)
    assert math.isfinite(abs(d['H']).max())
    # one frame, one seed, one link differ from the next
    assert d['H'][0, 0] != P.bf_draws(seed, frame + 1, ntx, nrx, n_sym, Nd)['H'][0, 0]
    assert d['H'][0, 0] != P.bf_draws(seed + 1, frame, ntx, nrx, n_sym, Nd)['H'][0, 0]
    assert len(set(d['H'].reshape(-1).tolist())) == ntx * nrx


# ---------------------------------------------------------------------------
# (c) the preconditions of tests/test_gpu_mimo_philox.py, from the oracle alone
def _uncoded_mix(frames, floor, name):
    ok, ber, fl = K.frame_mix_ok(frames, floor)
    print(f'{name}: BER {np.round(ber, 4).tolist()}' +
          ('' if fl is None else f', without noise {np.round(fl, 4).tolist()}'))
    assert ok, (name, ber, fl)


@pytest.mark.parametrize('name', list(K.BF_CASES))
def test_beamforming_case_preconditions(name):
    frames = K.bf_frames(name)
    assert min(fr['margin'] for fr in frames) >= K.BOUNDARY_MARGIN, name
    assert min(fr['pmi_gap'] for fr in frames) >= K.PMI_MARGIN, name
    _uncoded_mix(frames, lambda: K.bf_frames(name, snrs=K.NOISE_FREE), name)


def test_beamforming_cases_cover_the_issue():
    cs = K.BF_CASES.values()
    assert {(c['ntx'], c['nrx']) for c in cs} == {(2, 1), (4, 1), (8, 1), (2, 4), (4, 3), (8, 5), (8, 8)}
    assert {(c['ntx'], c['nrx'], c['mode']) for c in cs} == {(t, r, m) for t, r in [(2, 1), (4, 1), (8, 1), (2, 4),
                                                                                    (4, 3), (8, 5), (8, 8)]
                                                             for m in ('adaptive', 'static')}
    assert {c['mod'] for c in cs} == {'QPSK', '16-QAM', '64-QAM'}
    assert {c['bw'] for c in cs} >= {1.25, 20.0}
    tail = [c for c in cs if c['bw'] == 1.25 and c['n_sym'] == 3]
    assert tail and (K.B * 3 * 62) % 256 != 0


@pytest.mark.parametrize('name', list(K.SC_CASES))
def test_scfdm_case_preconditions(name):
    frames = K.sc_frames(name)
    assert min(fr['margin'] for fr in frames) >= K.BOUNDARY_MARGIN, name
    if K.SC_CASES[name]['nrx'] == 1:
        _uncoded_mix(frames, lambda: K.sc_frames(name, snrs=K.NOISE_FREE), name)
    else:   # the SIMO combiner never de-precodes (the reference's behaviour): every frame near BER 0.5
        assert all(0.4 < fr['errs'] / fr['n_bits'] < 0.6 for fr in frames)


@pytest.mark.parametrize('name', [n for n, c in K.SFBC_CASES.items() if not c['coded']])
def test_sfbc_uncoded_case_preconditions(name):
    pr = K.sfbc_predicates(K.SFBC_CASES[name])
    for merged in ((False, True) if pr['merge'] else (False,)):
        frames = K.sfbc_frames(name, merged)
        assert min(fr['margin'] for fr in frames) >= K.BOUNDARY_MARGIN, (name, merged)
        _uncoded_mix(frames, lambda: K.sfbc_frames(name, merged, snrs=K.NOISE_FREE), f'{name} merged={merged}')


@pytest.mark.parametrize('name', [n for n, c in K.SFBC_CASES.items() if c['coded']])
def test_sfbc_coded_case_preconditions(name):
    """MIN_PASS = MIN_FAIL = 1 of the 5 frames."""
    O.lib()
    pr = K.sfbc_predicates(K.SFBC_CASES[name])
    for merged in ((False, True) if pr['merge'] else (False,)):
        crc = [fr['crc'] for fr in K.sfbc_frames(name, merged)]
        assert sum(crc) >= 1 and len(crc) - sum(crc) >= 1, (name, merged, crc)


def test_sfbc_cases_cross_every_predicate():
    """Both values of every predicate select_mimo evaluates for the SFBC chains
    occur among the Rayleigh cases, and each case sits where its name says."""
    pr = {n: K.sfbc_predicates(c) for n, c in K.SFBC_CASES.items()}
    ray = {n: p for n, p in pr.items() if K.SFBC_CASES[n]['chan'] == 'rayleigh_mp'}
    for k in ('txch', 'rx_fuse', 'merge', 'lp_fuse'):
        assert {p[k] for p in ray.values()} == {True, False}, k
    assert {p['n_est'] for p in pr.values()} == {1, 2}
    assert pr['sfbc_awgn5_u']['flat_fuse'] and not pr['sfbc_awgn5_u']['txch']
    assert pr['sfbc_pa20_u']['merge'] and pr['sfbc_pa20_c']['merge'] and pr['sfbc_pa15_c']['merge']
    assert (pr['sfbc_pb20_u']['maxd'], pr['sfbc_vb20x_u']['maxd'], pr['sfbc_vb5_u']['maxd']) == (114, 139, 35)
    assert not pr['sfbc_pb20_u']['txch'] and pr['sfbc_pb20_u']['lp_fuse']
    assert pr['sfbc_vb20x_u']['n_paths'] == 8 and K.numerology(K.SFBC_CASES['sfbc_vb20x_u']).cp == 512 - 3
    assert pr['sfbc_taps32_u']['txch'] and not pr['sfbc_taps33_u']['txch']          # SFX_TL
    assert pr['sfbc_taps8_u']['txch'] and not pr['sfbc_taps9_u']['txch']            # TXCH_MAXP
    assert pr['sfbc_taps33_u']['lp_fuse'] and not pr['sfbc_taps9_u']['lp_fuse']
    cp10 = K.numerology(K.SFBC_CASES['sfbc_taps_cp_u']).cp
    assert (pr['sfbc_taps_cp_u']['maxd'], pr['sfbc_taps_cp1_u']['maxd']) == (cp10, cp10 + 1)
    assert pr['sfbc_taps_cp_u']['lp_fuse'] and not pr['sfbc_taps_cp1_u']['lp_fuse']
    assert K.numerology(K.SFBC_CASES['sfbc_vb5_u']).cp == 36 and pr['sfbc_vb5_u']['lp_fuse']
    assert K.numerology(K.SFBC_CASES['sfbc_pa125_rx1_u']).N == 128 and not pr['sfbc_pa125_rx1_u']['lp_fuse']
    assert K.numerology(K.SFBC_CASES['sfbc_pa15_c']).Nd == 749
    assert [pr[f'sfbc_rx{r}_u']['rx_fuse'] for r in (3, 4, 5, 8)] == [True, True, False, False]
    assert not any(pr[f'sfbc_rx{r}_u']['txch'] for r in (3, 4, 5, 8))


@pytest.fixture(scope='module')
def sm_all():
    return {name: K.sm_frames(name) for name in K.SM_CASES}


def test_spatial_r_measurement(sm_all):
    """r: tm4_oracle's detectors (np.linalg.inv / pinv, the reference's calls)
    against the kernel's Cholesky order on the same inputs, over every subcarrier
    of every case, in units of 2^-52 kappa / mu_min ||s||.
    mimo_philox_cases.R_SPATIAL holds it."""
    per = {name: max(fr['r'] for fr in frames) for name, frames in sm_all.items()}
    r = max(per.values())
    print('spatial r per case: ' + ', '.join(f'{k} {v:.4g}' for k, v in per.items()) +
          f'; r = {r:.6g} (R_SPATIAL = {K.R_SPATIAL})')
    assert r <= K.R_SPATIAL, (r, K.R_SPATIAL)
    assert r >= 0.5 * K.R_SPATIAL, (r, K.R_SPATIAL)      # the constant is the measurement, not a cushion


@pytest.mark.parametrize('name', list(K.SM_CASES))
def test_spatial_case_preconditions(sm_all, name):
    frames = sm_all[name]
    ok, worst = K.sm_margin_ok(frames, K.R_SPATIAL)
    print(f'{name}: smallest distance / margin = {worst:.4g}, largest kappa = '
          f'{max(fr["kappa"].max() for fr in frames):.4g}')
    assert ok, (name, worst)
    _uncoded_mix(frames, lambda: K.sm_frames(name, snrs=K.NOISE_FREE), name)


def test_spatial_cases_cover_the_issue():
    cs = K.SM_CASES
    num = {n: K.numerology(c) for n, c in cs.items()}
    assert num['sm_pb5_static'].Nd % 4 == 1 and num['sm_pb5_static'].N == 512 and cs['sm_pb5_static']['vel'] == 0.0
    assert num['sm_vb20x_v3'].cp % 2 == 1 and num['sm_vb20x_v3'].N + num['sm_vb20x_v3'].cp == 2557
    assert num['sm_r3_zf'].N == 1024 and num['sm_22_pmi1_zf'].N == 128 and num['sm_15'].Nd == 749
    assert {c['det'] for c in cs.values()} == {'MMSE', 'ZF', 'SIC', 'MRC'}
    assert {c['pmi'] for c in cs.values()} >= {0, 1, 3, 5} and {c['rank'] for c in cs.values()} == {1, 2, 3, 4}
    # exact Jakes against the Taylor sets (channel_mimo_select: |w_max| * half-span > 2.7e-3)
    def w_half(name):
        n = num[name]
        return 2 * np.pi * O.doppler_hz(2.0, cs[name]['vel']) / n.fs * (n.N + n.cp) / 2
    assert w_half('sm_va20_v30') > 2.7e-3 > w_half('sm_pb20_v3') > 0
