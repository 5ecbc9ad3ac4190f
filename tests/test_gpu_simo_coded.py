"""GPU: the coded SIMO chain (LTE_CHAIN_SIMO_CODED, 1 x N MRC with turbo coding)
against the NumPy model of tests/simo_coded_model.py, which composes the
oracle's primitives (never against another GPU run, except where a test is
about two paths agreeing).

  (1) the ladder of simo_coded_model.CASES (1 to 5 RX), 67 frames over the
      turbo cliff at 2 iterations (tests/test_simo_coded_host.py asserts from
      the model alone that each case passes and fails at least 8 frames),
      injected bits / phases / noise, LLR capture, f64 and f32
  (2) the symbol hand-off (k_dematch_zn) against the LLR round trip
  (3) every switch select_siso consults for this chain, and an H capture, each
      against the model, f64 and f32
  (4) Philox draws (the fused TX + channel), frame ids from both ends of a
      4096-trial grid, at fD = 0 and at 3 km/h
  (5) run_grid(coded=True, num_rx=2), early_stop, simulate_simo_coded

Bars: tx_syms exact (f32 1e-6); noise_power 1e-12 (f32
2e-6); the combined symbols z within 1e-12 (f32 1e-4) of sqrt(sum_r
max|Y_r|^2) / sqrt(D) of the model's per RE; LLRs |got - ref| / (1 + |ref|) <
1e-12 against the model's own LLRs (f32: 1e-4 against the model's demapper and
sigma^2_eff on the run's own z, which the bar before ties to the model's, as
the suite forms its float32 LLR references); bits, error
counts, CRC verdicts and counters identical to the oracle's decode of the run's
own LLRs (f32: turbo_decode_f32_model)."""
import numpy as np
import pytest

import simo_coded_model as M

pytestmark = pytest.mark.gpu

FRAMES, ITERS = M.FRAMES, M.ITERS
SWITCHES = ('LTE_TXCH_FUSE', 'LTE_RX_FUSE', 'LTE_SIMO_TX_WAVE', 'LTE_SIMO_RX_WAVE', 'LTE_TX_FRAME', 'LTE_RX_WAVE',
            'LTE_TX_WAVE', 'LTE_RXS_PAIRS', 'LTE_SIMO_XHAND', 'LTE_DEMAP_IN_DEMATCH', 'LTE_TXW_STAGE', 'LTE_TX_STAGE')
TOL = {'f64': dict(npow=1e-12, llr=1e-12, sym=1e-12, tx=0.0), 'f32': dict(npow=2e-6, llr=1e-4, sym=1e-4, tx=1e-6)}
VERDICTS = ('bits_rx', 'crc_ok', 'frame_errors', 'counts')


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    _capi.device_init()
    return _capi


def clear_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def simulator(cs, prec, velocity_kmh=0.0):
    import lte_phy
    return lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=cs['bw'], modulation=cs['mod']), channel_type=cs['chan'],
                                 itu_profile=cs['prof'], frequency_ghz=2.0, velocity_kmh=velocity_kmh, precision=prec)


def case_plan(C, O, name, prec, max_frames=FRAMES, velocity_kmh=0.0, early_stop=False):
    cs = M.CASES[name]
    num = M.numerology(O, cs)
    plan = simulator(cs, prec, velocity_kmh)._plan(C.CHAIN_SIMO_CODED, 0, cs['n_bits'], num_rx=cs['nrx'],
                                                   max_frames=max_frames, iters=ITERS, early_stop=early_stop)
    assert plan.coded and not plan.mimo and plan.chain == 7 and plan.num_rx == cs['nrx']
    dl, g = M.taps(O, num, cs)
    d = plan.desc
    assert [d.delays[i] for i in range(d.n_paths)] == [int(v) for v in dl]
    assert np.array_equal(np.array([d.gains[i] for i in range(d.n_paths)]), np.asarray(g, dtype=np.float64))
    assert plan.Nd == num.Nd and plan.precision == prec
    return plan, num, cs


def inject(inp):
    return dict(bits=inp['bits'], phases=inp['ph'] if inp['ph'].size else None, noise=inp['z'])


def same_verdicts(a, b, tag):
    for k in VERDICTS:
        assert np.array_equal(a[k], b[k]), (tag, k)


def no_wave_kernel(path):
    return not any(v.endswith('_w') for v in path.values())


# ---------------------------------------------------------------------------
# (1) the ladder
_SEP = 'k_rx_chest+k_rx_data'
CAP = ('tx_syms', 'llr', 'bits_rx', 'noise_power', 'data_syms')


def fused_rx(num, nrx):
    """The receiver select_siso takes by default: fused for 2..4 RX (in pairs at
    N = 1024 with an even count), else the separate kernels."""
    if not 2 <= nrx <= 4:
        return _SEP
    return 'k_rx_frame_simo2' if num.N == 1024 and nrx % 2 == 0 else 'k_rx_frame_simo'


def check_against_model(O, plan, num, cs, inp, frames, r, prec, tag):
    """One run with the captures CAP against the model, frame by frame:
    tx_syms; the combiner's output z per RE within tol['sym'] * sqrt(sum_r
    max|Y_r|^2) / sqrt(D) of the model's (the suite's bar for MRC symbols,
    tests/test_gpu_profiles.py); LLRs (f64: the model's own; f32: the model's
    demapper and sigma^2_eff on the run's z, which the line before ties to the
    model's z); noise_power per RX; bits, CRC verdicts, error counts and
    counters equal to the oracle's decode of the run's own LLRs (f32:
    turbo_decode_f32_model), and in f64 to the model's own decisions.
    Returns the worst (z / bound, LLR error, noise_power error)."""
    tol, f32 = TOL[prec], prec == 'f32'
    coded = plan.coded_bits
    seg = frames[0]['tx']['plan']
    pos = M.deinterleave_index(len(frames[0]['tx']['qam']), num.Nd)
    src = M.deinterleave_index(coded // num.bps, num.Nd)
    worst_z = worst_llr = worst_np = 0.0
    errs, oks = [], []
    for b, fr in enumerate(frames):
        where = tag + (b,)
        assert coded == len(fr['tx']['coded'])
        ts = r['tx_syms'][b].astype(np.complex128)[pos]
        assert np.max(np.abs(ts - fr['tx']['qam'])) <= tol['tx'], where
        snr = float(inp['snrs'][b])
        zg = r['data_syms'][b].astype(np.complex128)
        worst_z = max(worst_z, float(np.max(np.abs(zg - fr['z']) / (tol['sym'] * fr['z_scale']))))
        got = r['llr'][b].astype(np.float64).reshape(-1, num.bps)[src].reshape(-1)[:coded]
        ref = M.soft_output(O, num, zg, fr['Dg'], coded, snr)[0] if f32 else fr['llr']
        worst_llr = max(worst_llr, float(np.max(np.abs(got - ref) / (1 + np.abs(ref)))))
        npw = M.noise_powers(O, num, cs, fr['tx']['signal'], snr, M.draws_of(inp['ph'][b], inp['z'][b]))
        worst_np = max(worst_np, float(np.max(np.abs(r['noise_power'][b].astype(np.float64) / npw - 1))))
        dec, ok = M.decode_llrs(O, num, seg, coded, r['llr'][b], f32=f32)
        assert np.array_equal(dec, r['bits_rx'][b]), where + (int(np.sum(dec != r['bits_rx'][b])),)
        assert bool(ok) == bool(r['crc_ok'][b]), where
        assert int(r['frame_errors'][b]) == int(np.sum(inp['bits'][b] != dec)), where
        errs.append(int(np.sum(inp['bits'][b] != dec)))
        oks.append(bool(ok))
        if not f32:      # and the model's own decisions (its LLRs differ from the run's by round-off only)
            assert np.array_equal(fr['bits_rx'], r['bits_rx'][b]) and fr['crc'] == bool(ok), where
    print(f'simo coded {tag}: worst z err / bound {worst_z:.3g}, LLR err {worst_llr:.3g}, noise_power rel err '
          f'{worst_np:.3g}, {sum(oks)} pass / {FRAMES - sum(oks)} fail, path {r.path}')
    assert worst_z <= 1.0, tag + (worst_z,)
    assert worst_llr < tol['llr'], tag + (worst_llr,)
    assert worst_np <= tol['npow'], tag + (worst_np,)
    assert sum(oks) >= M.MIN_PASS and FRAMES - sum(oks) >= M.MIN_FAIL
    want = np.array([[sum(errs), FRAMES * cs['n_bits'], FRAMES - sum(oks), FRAMES]], dtype=np.uint64)
    assert np.array_equal(r['counts'], want), (r['counts'], want)
    return worst_z, worst_llr, worst_np


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('name', list(M.CASES))
def test_ladder(C, oracle, monkeypatch, name, prec):
    """k_payload / k_encode / k_ofdm_txf with one channel per RX / k_chan_fix /
    k_npow / k_rx_frame_simo* writing LLRs / k_dematch / k_turbo* / k_crc_count /
    k_accumulate; with 1 and with 5 RX (B1, B5) the receiver is k_rx_chest +
    k_rx_data<SIMO_CODED> writing LLRs."""
    clear_switches(monkeypatch)
    plan, num, cs = case_plan(C, oracle, name, prec)
    inp, frames = M.case_frames(oracle, name)
    assert plan.L == inp['L']
    r = plan.run(inp['snrs'], **inject(inp), capture=CAP)
    assert r.path['dematch'] == 'llr' and no_wave_kernel(r.path), r.path
    assert r.path['rx'] == fused_rx(num, cs['nrx']), r.path
    check_against_model(oracle, plan, num, cs, inp, frames, r, prec, (name, prec))


# ---------------------------------------------------------------------------
# (2) symbol hand-off
@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('name', ['B2', 'C2', 'D4'])
def test_symbol_handoff_equals_llr_round_trip(C, oracle, monkeypatch, name, prec):
    """16 / 64-QAM without an LLR capture: the receiver writes z per RE and
    sigma^2_eff per (frame, group, data subcarrier) and k_dematch_zn demaps;
    LTE_DEMAP_IN_DEMATCH=0 and an LLR capture take k_dematch.  Same decisions."""
    clear_switches(monkeypatch)
    plan, num, cs = case_plan(C, oracle, name, prec)
    inp, _ = M.case_frames(oracle, name)
    kw = inject(inp)
    zn = plan.run(inp['snrs'], **kw, capture=('bits_rx',))
    assert zn.path['dematch'] == 'zn' and no_wave_kernel(zn.path), zn.path
    cap = plan.run(inp['snrs'], **kw, capture=('bits_rx', 'llr'))
    assert cap.path['dematch'] == 'llr'
    monkeypatch.setenv('LTE_DEMAP_IN_DEMATCH', '0')
    llr = plan.run(inp['snrs'], **kw, capture=('bits_rx',))
    assert llr.path['dematch'] == 'llr'
    from lte_phy.engine import path_diff
    assert path_diff(zn.path, llr.path) == {'dematch'}, (zn.path, llr.path)
    same_verdicts(zn, llr, (name, prec, 'zn / llr'))
    same_verdicts(zn, cap, (name, prec, 'zn / capture'))
    n_ok = int(np.sum(zn['crc_ok'] != 0))
    assert n_ok >= M.MIN_PASS and FRAMES - n_ok >= M.MIN_FAIL


# ---------------------------------------------------------------------------
# (3) dispatch edges
# label -> (environment, extra captures)
EDGES = {
    'rx_fuse0': ({'LTE_RX_FUSE': '0'}, ()),
    'rxs_pairs0': ({'LTE_RXS_PAIRS': '0'}, ()),
    'txch_fuse0': ({'LTE_TXCH_FUSE': '0'}, ()),
    'tx_frame0': ({'LTE_TX_FRAME': '0'}, ()),
    'tx_stage0': ({'LTE_TX_FRAME': '0', 'LTE_TX_STAGE': '0'}, ()),
    'cap_H': ({}, ('H',)),
    'wave_knobs_on': ({'LTE_SIMO_RX_WAVE': '1', 'LTE_SIMO_TX_WAVE': '1', 'LTE_SIMO_XHAND': '1'}, ()),
}


def default_path(num, cs):
    """The path of a run with injected draws and no stream capture.  N < 512 has
    no fused TX + channel (txch_supported)."""
    fused_tx = num.N >= 512 and cs['chan'] == 'rayleigh_mp'
    return {'tx': 'k_ofdm_txf' if fused_tx else 'k_ofdm_tx', 'tx_stage': '1', 'ch_fix': '1' if fused_tx else '0',
            'xhand': '0', 'rx': fused_rx(num, cs['nrx'])}


def moved(label, num, cs):
    """The path fields an edge moves away from default_path."""
    fused_tx = num.N >= 512 and cs['chan'] == 'rayleigh_mp'
    pairs = fused_rx(num, cs['nrx']) == 'k_rx_frame_simo2'
    unpair = {'rx': 'k_rx_frame_simo'} if pairs else {}
    per_sym = {'tx': 'k_ofdm_tx_ch'} if fused_tx else {}
    return {'rx_fuse0': {'rx': _SEP}, 'rxs_pairs0': unpair, 'cap_H': unpair, 'wave_knobs_on': {},
            'txch_fuse0': {'tx': 'k_ofdm_tx', 'ch_fix': '0'} if fused_tx else {},
            'tx_frame0': per_sym, 'tx_stage0': dict(per_sym, tx_stage='0')}[label]


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('name', ['A2', 'B3', 'D4'])
def test_dispatch_edges(C, oracle, monkeypatch, name, prec):
    """Each switch of select_siso that this chain reaches, on N = 128 QPSK (A2:
    no fused transmitter, LLRs on every path, so LTE_RX_FUSE=0 is k_rx_data<
    SIMO_CODED>'s LLR branch), N = 512 with an odd RX count (B3) and N = 1024 with
    the paired receiver (D4), in both precisions.  Every edge runs twice: with
    the LLR capture, checked against the model like a ladder run (symbols, LLRs,
    noise powers, the oracle's decode of the run's own LLRs), and without it
    (the symbol hand-off where the modulation has one), with the same
    decisions.  The path is the one lte_run_path claims and never names a wave
    kernel (k_rx_frame_simo_w / k_ofdm_tx_simo_w are uncoded, and so is the
    symbol hand-over LTE_SIMO_XHAND).  In f64 every path gives the default
    path's decisions bit for bit."""
    clear_switches(monkeypatch)
    plan, num, cs = case_plan(C, oracle, name, prec)
    inp, frames = M.case_frames(oracle, name)
    kw = inject(inp)
    zn = 'zn' if num.bps > 2 else 'llr'
    want = default_path(num, cs)
    base = plan.run(inp['snrs'], **kw, capture=('bits_rx',))
    assert base.path == dict(want, dematch=zn), base.path
    for label, (env, cap) in EDGES.items():
        clear_switches(monkeypatch)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        path = dict(want, **moved(label, num, cs))
        r = plan.run(inp['snrs'], **kw, capture=CAP + cap)
        assert r.path == dict(path, dematch='llr') and no_wave_kernel(r.path), (name, label, r.path)
        check_against_model(oracle, plan, num, cs, inp, frames, r, prec, (name, prec, label))
        q = plan.run(inp['snrs'], **kw, capture=('bits_rx',) + cap)
        assert q.path == dict(path, dematch=zn) and no_wave_kernel(q.path), (name, label, q.path)
        same_verdicts(r, q, (name, prec, label, 'llr / ' + zn))
        if prec == 'f64':
            same_verdicts(base, q, (name, label, 'default / edge'))


# ---------------------------------------------------------------------------
# (4) Philox draws
GRID_T, SEED = 4096, 77


def philox_ids(S):
    return np.concatenate([np.arange(8), S * GRID_T - 8 + np.arange(8)]).astype(np.uint64)


@pytest.mark.parametrize('name,velocity', [(n, 0.0) for n in M.CASES] + [('B2', 3.0)])
def test_philox_frames(C, oracle, name, velocity):
    """No injection: the fused TX + channel draws LTE_CHAIN_SIMO's streams
    (philox.siso_draws) and k_payload the payload.  The first and last 8 frame
    ids of a 2-point x 4096-trial grid whose points sit a quarter into the
    case's window from either end; per-frame bit errors and CRC verdicts equal
    the model's.  3 km/h: the per-symbol Taylor sets of every RX."""
    from oracle import philox as P
    O = oracle
    plan, num, cs = case_plan(C, O, name, 'f64', max_frames=16, velocity_kmh=velocity)
    lo, hi = cs['snr']
    snrs = np.array([lo + 0.25 * (hi - lo), lo + 0.75 * (hi - lo)])
    ids = philox_ids(len(snrs))
    si = (ids // GRID_T).astype(np.int32)
    r = plan.run(snrs[si], snr_index=si, n_snr=len(snrs), seed=SEED, frame_ids=ids)
    if cs['chan'] == 'rayleigh_mp':
        assert (r.path['tx'], r.path['ch_fix']) == ('k_ofdm_txf', '1'), r.path
    assert no_wave_kernel(r.path)
    fD = O.doppler_hz(2.0, velocity) if velocity else 0.0
    fr = [M.philox_frame(O, P, num, cs, SEED, int(i), float(snrs[s]), fD=fD) for i, s in zip(ids, si)]
    assert [int(e) for e in r['frame_errors']] == [f['errs'] for f in fr], (name, velocity)
    assert [bool(c) for c in r['crc_ok']] == [f['crc'] for f in fr], (name, velocity)
    want = np.zeros((2, 4), dtype=np.uint64)
    for s, f in zip(si, fr):
        want[s] += np.array([f['errs'], cs['n_bits'], 0 if f['crc'] else 1, 1], dtype=np.uint64)
    assert np.array_equal(r['counts'], want)


def test_philox_frames_f32(C, oracle):
    """float32 on Philox draws, 3 dB outside the window on either side (the
    float32 decoder may turn a frame on the cliff the other way): the verdicts
    equal the model's and the frames the model decodes come out clean."""
    from oracle import philox as P
    plan, num, cs = case_plan(C, oracle, 'B2', 'f32', max_frames=16)
    snrs = np.array([cs['snr'][0] - 3.0, cs['snr'][1] + 3.0])
    ids = philox_ids(2)
    si = (ids // GRID_T).astype(np.int32)
    r = plan.run(snrs[si], snr_index=si, n_snr=2, seed=SEED, frame_ids=ids)
    fr = [M.philox_frame(oracle, P, num, cs, SEED, int(i), float(snrs[s])) for i, s in zip(ids, si)]
    assert [f['crc'] for f in fr] == [False] * 8 + [True] * 8
    assert [bool(c) for c in r['crc_ok']] == [f['crc'] for f in fr]
    assert not r['frame_errors'][8:].any() and r['frame_errors'][:8].all()


# ---------------------------------------------------------------------------
# (5) public API
API_SNRS = [-2.0, 1.0, 4.0]
API_T, API_SEED = 6, 5


def test_run_grid_coded_simo(C, oracle):
    """run_grid(coded=True, num_rx=2): the new chain (not the SISO plan it used
    to build), sharding-invariant, equal to a plan-level run and to the model
    frame by frame; with num_rx=1 the same frames give other counts, as the
    models of the two chains say they must."""
    from oracle import philox as P
    O = oracle
    cs = M.CASES['A2']
    num = M.numerology(O, cs)
    sim = simulator(cs, 'f64')
    kw = dict(seed=API_SEED, coded=True, n_bits=cs['n_bits'], frames_per_call=8, turbo_iters=ITERS)
    full = sim.run_grid(API_SNRS, API_T, num_rx=2, **kw)
    assert full['plan'].chain == C.CHAIN_SIMO_CODED and full['plan'].num_rx == 2 and full['plan'].coded
    parts = [sim.run_grid(API_SNRS, API_T, num_rx=2, rank=k, world_size=2, **kw) for k in range(2)]
    assert np.array_equal(parts[0]['counts'] + parts[1]['counts'], full['counts'])
    ids = np.arange(len(API_SNRS) * API_T, dtype=np.uint64)
    si = (ids // API_T).astype(np.int32)
    plan = sim._plan(C.CHAIN_SIMO_CODED, 0, cs['n_bits'], num_rx=2, max_frames=len(ids), iters=ITERS)
    r = plan.run(np.asarray(API_SNRS)[si], snr_index=si, n_snr=len(API_SNRS), seed=API_SEED, frame_ids=ids)
    assert np.array_equal(r['counts'], full['counts'])
    want2 = np.zeros((len(API_SNRS), 4), dtype=np.uint64)
    want1 = np.zeros_like(want2)
    for i, s in zip(ids, si):
        f = M.philox_frame(O, P, num, cs, API_SEED, int(i), API_SNRS[s])
        want2[s] += np.array([f['errs'], cs['n_bits'], 0 if f['crc'] else 1, 1], dtype=np.uint64)
        bits = P.payload_bits(API_SEED, int(i), cs['n_bits'])
        L = len(f['tx']['signal'])
        o = O.simulate_siso_coded(num, bits, API_SNRS[s], 'awgn', draws=P.siso_draws(API_SEED, int(i), L, 0),
                                  iters=ITERS)
        want1[s] += np.array([o['bit_errors'], cs['n_bits'], 0 if o['crc_pass'] else 1, 1], dtype=np.uint64)
    assert np.array_equal(full['counts'], want2), (full['counts'], want2)
    assert not np.array_equal(want1[:, 2], want2[:, 2])         # the models: another BLER with one RX
    one = sim.run_grid(API_SNRS, API_T, num_rx=1, **kw)
    assert one['plan'].chain == C.CHAIN_CODED
    assert np.array_equal(one['counts'], want1), (one['counts'], want1)
    assert 0 < int(full['counts'][:, 2].sum()) < len(ids)       # and the window straddles the 2-RX cliff


def test_run_grid_early_stop(C, oracle):
    """early_stop=True on the new chain: 'turbo_iters_hist' is the histogram of
    the rule evaluated by the oracle on the model's LLRs of the same frames."""
    from oracle import philox as P
    O = oracle
    cs = M.CASES['A2']
    num = M.numerology(O, cs)
    sim = simulator(cs, 'f64')
    iters = 4
    kw = dict(seed=API_SEED, coded=True, n_bits=cs['n_bits'], frames_per_call=8, turbo_iters=iters, num_rx=2)
    g = sim.run_grid(API_SNRS, API_T, early_stop=True, **kw)
    hist = g['turbo_iters_hist']
    assert hist.dtype == np.uint64 and hist.shape == (len(API_SNRS), iters + 1)
    want = np.zeros_like(hist)
    for s in range(len(API_SNRS)):
        for t in range(API_T):
            f = M.philox_frame(O, P, num, cs, API_SEED, s * API_T + t, API_SNRS[s], iters=iters)
            for n in M.early_stop_n_star(O, f['llr'], f['tx']['plan'], iters):
                want[s, n] += 1
    assert np.array_equal(hist, want), (hist, want)
    assert len(set(np.flatnonzero(want.sum(axis=0)).tolist())) >= 2     # more than one stopping iteration occurs
    assert np.allclose(g['turbo_iters_mean'], (hist * np.arange(iters + 1)).sum(axis=1) / API_T)
    assert 'turbo_iters_hist' not in sim.run_grid(API_SNRS[-1:], 2, **kw)


SISO_CODED_KEYS = {'transmitted_bits', 'received_bits', 'bits_received_array', 'bit_errors', 'ber', 'crc_pass',
                   'snr_db', 'papr_db', 'papr_linear', 'coded_bits_length', 'signal_tx', 'signal_rx', 'symbols_tx',
                   'symbols_rx', 'H_estimate', 'channel_snr_db', 'noise_var_mean'}


@pytest.mark.parametrize('name,snr', [('B3', 5.0), ('B3', 9.0), ('A2', 3.0)])
def test_simulate_simo_coded_ref_compat(C, oracle, name, snr):
    """One call on the seeded global RNG equals the model on ref_compat_draws
    (simulate_simo's order: TX pilot reseed, per RX 16 phases per path and
    normal(L) twice, RX pilot reseed), 8 iterations, and leaves the RNG where
    simulate_simo leaves it on a frame of the same length."""
    O = oracle
    cs = M.CASES[name]
    num = M.numerology(O, cs)
    sim = simulator(cs, 'f64')
    bits = np.random.RandomState(3).randint(0, 2, cs['n_bits'])
    np.random.seed(11)
    r = sim.simulate_simo_coded(bits, snr, num_rx=cs['nrx'])
    state = np.random.get_state()
    assert set(r) == (SISO_CODED_KEYS - {'signal_rx', 'H_estimate', 'channel_snr_db'}) | \
        {'signal_rx_list', 'channel_gain', 'num_rx', 'combining_method'}
    assert (r['num_rx'], r['combining_method']) == (cs['nrx'], 'mrc')
    L = len(r['signal_tx'])
    np.random.seed(11)
    draws = O.ref_compat_draws(num, cs['chan'], L, cs['nrx'], cs['prof'])
    assert all(np.array_equal(a, b) for a, b in zip(state[1:3], np.random.get_state()[1:3]))
    fr = M.frame(O, num, cs, bits, snr, draws, iters=8)
    assert np.array_equal(r['bits_received_array'], fr['bits_rx']) and r['crc_pass'] == fr['crc']
    assert r['bit_errors'] == fr['errs'] and r['coded_bits_length'] == len(fr['tx']['coded'])
    assert np.array_equal(r['symbols_tx'], fr['tx']['qam'])
    assert np.linalg.norm(r['signal_tx'] - fr['tx']['signal']) <= 1e-13 * np.linalg.norm(fr['tx']['signal'])
    for a in range(cs['nrx']):
        assert np.linalg.norm(r['signal_rx_list'][a] - fr['rxs'][a]) <= 1e-13 * np.linalg.norm(fr['rxs'][a])
    assert np.max(np.abs(r['channel_gain'] / fr['channel_gain'] - 1)) < 1e-12
    nv = M.sigma2_eff(fr['channel_gain'], snr)
    assert abs(r['noise_var_mean'] / float(np.mean(nv)) - 1) < 1e-12
    # simulate_simo on a frame of the same length consumes the same numbers
    np.random.seed(11)
    sim.simulate_simo(np.zeros(L // (num.N + num.cp) * num.Nd * num.bps, dtype=int), snr, num_rx=cs['nrx'])
    after = np.random.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(state[1:], after[1:]))
