"""GPU: the coded TM4 chain (LTE_CHAIN_SPATIAL_CODED, spatial multiplexing with
the soft MMSE / ZF / MRC detector and turbo coding) against the NumPy model of
tests/spatial_coded_model.py, which composes the oracle's primitives (never
against another GPU run, except where a test is about two paths agreeing).

  (1) the ladder of spatial_coded_model.CASES, 67 frames over the turbo cliff at
      2 iterations (tests/test_spatial_coded_host.py asserts from the model alone
      that each case passes and fails at least 8 frames), injected bits / phases
      or link_h / noise, LLR, symbol and bit captures, f64 and f32
  (2) every switch select_mimo reads for this chain (lte_knobs.h), and an H
      capture, each against the model, f64 and f32
  (3) Philox draws, frame ids from both ends of a 4096-trial grid, and R44 at
      3 km/h
  (4) run_grid(coded=True, mimo='spatial'), early_stop,
      simulate_spatial_multiplexing_coded, and LTE_CHAIN_SPATIAL unchanged

Bars, per RE, with kappa = cond(A) and mu_min of the RE's subcarrier from the
model and r_cpu = spatial_coded_model.R_CPU (the disagreement of two float64
evaluations of the rule on the CPU, tests/test_spatial_coded_host.py): the
detector output z within 4 r_cpu eps kappa / mu_min ||z|| and the LLRs within
4 r_cpu eps kappa / mu_min (1 + |ref|) of the model's, eps = 2^-52 (f32 plans:
2^-23 -- the detector is float64 there too, Y, H and the stores are float32);
the 4 is for a third evaluation order with FMA contraction.  Bits, error counts,
CRC verdicts and counters identical to the oracle's decode of the run's own
LLRs (f32: turbo_decode_f32_model), and in f64 to the model's own decisions."""
import numpy as np
import pytest

import spatial_coded_model as M

pytestmark = pytest.mark.gpu

FRAMES, ITERS = M.FRAMES, M.ITERS
SWITCHES = ('LTE_MIMO_FLAT_FUSE', 'LTE_TXCH_PR', 'LTE_MIMO_TX_WAVE', 'LTE_TXM_FRAME', 'LTE_CHM_TAY', 'LTE_CHT_ECON',
            'LTE_CHT_J', 'LTE_CHT_G', 'LTE_MIMO_RX_WAVE', 'LTE_SPATIAL_HP', 'LTE_DSP_STAGE', 'LTE_MIMO_LP_FUSE',
            'LTE_DEMAP_IN_DEMATCH')
EPS = {'f64': 2.0 ** -52, 'f32': 2.0 ** -23}
VERDICTS = ('bits_rx', 'crc_ok', 'frame_errors', 'counts')
CAP = ('llr', 'data_syms', 'bits_rx')


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    _capi.device_init()
    return _capi


@pytest.fixture(scope='module')
def orc(oracle, mimo_oracle, tm4_oracle):
    return oracle, mimo_oracle, tm4_oracle


def clear_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def case_plan(C, orc, cs, prec, max_frames=FRAMES, velocity_kmh=0.0, iters=ITERS, early_stop=False):
    import lte_phy
    from lte_phy import ofdm_core
    from lte_phy.tm4 import DETECTORS
    O, MO, T = orc
    num = M.numerology(O, cs)
    cfg = lte_phy.LTEConfig(bandwidth=cs['bw'], modulation=cs['mod'])
    W = M.precoder(T, cs)
    plan = ofdm_core._spatial_plan(cfg, cs['chan'], cs['prof'], velocity_kmh, 2.0, 0, cs['n_bits'], max_frames,
                                   num_tx=cs['ntx'], num_rx=cs['nrx'], rank=cs['rank'], detector=DETECTORS[cs['det']],
                                   W=W, precision=prec, coded=True, turbo_iters=iters, early_stop=early_stop)[0]
    assert plan.coded and plan.mimo and plan.chain == 8 and plan.precision == prec
    assert plan.Nd == num.Nd and plan.res == num.Nd and plan.n_dsc == -(-num.Nd // cs['rank'])
    return plan, num


def inject(inp):
    return dict(bits=inp['bits'], phases=inp['ph'] if inp['P'] else None, link_h=None if inp['P'] else inp['lh'],
                noise=inp['z'])


def same_verdicts(a, b, tag):
    for k in VERDICTS:
        assert np.array_equal(a[k], b[k]), (tag, k)


def check_against_model(O, plan, num, cs, inp, frames, r, prec, tag, iters=ITERS):
    """One run with the captures CAP against the model, frame by frame: z and the
    LLRs per RE within the bars of the module docstring; bits, CRC verdicts,
    error counts and counters equal to the oracle's decode of the run's own LLRs
    (f32: turbo_decode_f32_model) and, in f64, to the model's own decisions.
    Returns the worst z and LLR errors in units of eps kappa / mu_min ||z|| and
    eps kappa / mu_min (1 + |ref|): the bar is 4 r_cpu."""
    f32 = prec == 'f32'
    eps = EPS[prec]
    bar = 4.0 * M.R_CPU
    seg = frames[0]['tx']['plan']
    coded = plan.coded_bits
    worst_z = worst_llr = 0.0
    errs, oks = [], []
    for b, fr in enumerate(frames):
        where = tag + (b,)
        assert coded == len(fr['tx']['coded']) and plan.n_sym == fr['tx']['n_sym']
        rx = fr['rx']
        unit = eps * rx['kappa'] / rx['mu_min']
        zg = r['data_syms'][b].astype(np.complex128)
        worst_z = max(worst_z, float(np.max(np.abs(zg - fr['z']) / (unit * rx['z_norm']))))
        got = r['llr'][b].astype(np.float64)
        ref = fr['llr']
        worst_llr = max(worst_llr, float(np.max(np.abs(got - ref) / (np.repeat(unit, num.bps) * (1 + np.abs(ref))))))
        dec, ok = M.decode_llrs(O, num, seg, coded, r['llr'][b], iters=iters, f32=f32)
        dec = np.asarray(dec)[:cs['n_bits']]
        assert np.array_equal(dec, r['bits_rx'][b]), where + (int(np.sum(dec != r['bits_rx'][b])),)
        assert bool(ok) == bool(r['crc_ok'][b]), where
        assert int(r['frame_errors'][b]) == int(np.sum(inp['bits'][b] != dec)), where
        errs.append(int(np.sum(inp['bits'][b] != dec)))
        oks.append(bool(ok))
        if not f32:      # and the model's own decisions (its LLRs differ from the run's by round-off only)
            assert np.array_equal(fr['bits_rx'], r['bits_rx'][b]) and fr['crc'] == bool(ok), where
    n = len(frames)
    print(f'spatial coded {tag}: worst z err {worst_z:.4g}, LLR err {worst_llr:.4g} (units of eps kappa / mu_min; '
          f'bar 4 r_cpu = {bar:.0f}), {sum(oks)} pass / {n - sum(oks)} fail, path {r.path}')
    assert worst_z <= bar, tag + (worst_z,)
    assert worst_llr <= bar, tag + (worst_llr,)
    want = np.array([[sum(errs), n * cs['n_bits'], n - sum(oks), n]], dtype=np.uint64)
    assert np.array_equal(r['counts'], want), (r['counts'], want)
    return worst_z, worst_llr, sum(oks)


# ---------------------------------------------------------------------------
# (1) the ladder
@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('name', list(M.CASES))
def test_ladder(C, orc, monkeypatch, name, prec):
    """k_payload / k_encode / the spatial transmitter with the coded streams /
    the link / k_rx_fft_mimo* / k_det_spatial<.., SOFT> writing LLRs / k_dematch /
    k_turbo* / k_crc_count / k_accumulate."""
    clear_switches(monkeypatch)
    cs = M.CASES[name]
    plan, num = case_plan(C, orc, cs, prec)
    inp, frames = M.case_frames(*orc, name)
    assert plan.L == inp['L'] and plan.n_paths == inp['P']
    r = plan.run(inp['snrs'], **inject(inp), capture=CAP)
    assert r.path['dematch'] == 'llr' and r.path['h_pilots'] == '1' and r.path['det_stage'] == '1', r.path
    _, _, n_ok = check_against_model(orc[0], plan, num, cs, inp, frames, r, prec, (name, prec))
    assert n_ok >= M.MIN_PASS and FRAMES - n_ok >= M.MIN_FAIL


# ---------------------------------------------------------------------------
# (2) dispatch edges: label -> (environment, extra captures, path fields it must set where it applies)
EDGES = {
    'dsp_stage0': ({'LTE_DSP_STAGE': '0'}, (), {'det_stage': '0', 'h_pilots': '1'}),
    'spatial_hp0': ({'LTE_SPATIAL_HP': '0'}, (), {'det_stage': '0', 'h_pilots': '0'}),
    'cap_H': ({}, ('H',), {'det_stage': '0', 'h_pilots': '0'}),
    'flat_fuse0': ({'LTE_MIMO_FLAT_FUSE': '0'}, (), {}),
    'chm_tay0': ({'LTE_CHM_TAY': '0', 'LTE_MIMO_FLAT_FUSE': '0'}, (), {'ch': 'k_channel_mimo'}),
    'cht_j1_g1': ({'LTE_CHT_J': '1', 'LTE_CHT_G': '1', 'LTE_CHT_ECON': '0'}, (), {}),
    'rx_wave0': ({'LTE_MIMO_RX_WAVE': '0'}, (), {'rx': 'k_rx_fft_mimo'}),
    'txm_frame0': ({'LTE_TXM_FRAME': '0'}, (), {}),
    'txch_pr1': ({'LTE_TXCH_PR': '1'}, (), {}),
    'tx_wave1': ({'LTE_MIMO_TX_WAVE': '1'}, (), {}),
}
EDGE_STRIDE = 3      # the edges run every third frame of the ladder: the whole window, a third of the decodes


def every(inp, frames, k):
    sub = dict(inp, **{key: inp[key][::k] for key in ('bits', 'ph', 'lh', 'z', 'snrs')})
    return sub, frames[::k]


def run_edges(C, orc, monkeypatch, cs, inp, frames, prec, tag):
    plan, num = case_plan(C, orc, cs, prec, max_frames=len(frames))
    kw = inject(inp)
    clear_switches(monkeypatch)
    base = plan.run(inp['snrs'][:len(frames)], **kw, capture=CAP)
    assert base.path['dematch'] == 'llr'
    seen = {tuple(sorted(base.path.items()))}
    for label, (env, cap, fields) in EDGES.items():
        clear_switches(monkeypatch)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        r = plan.run(inp['snrs'][:len(frames)], **kw, capture=CAP + cap)
        assert r.path == plan.path(inp['snrs'][:len(frames)], **kw, capture=CAP + cap)
        assert r.path['dematch'] == 'llr', (tag, label, r.path)     # the symbol hand-off is not this chain's
        for k, v in fields.items():
            assert r.path[k] == v, (tag, label, r.path)
        if label == 'flat_fuse0' or label == 'chm_tay0':
            assert r.path['tx'] in ('k_ofdm_tx_mimo', 'k_ofdm_tx_mimo_frame') and r.path['ch'] != 'fused', r.path
        seen.add(tuple(sorted(r.path.items())))
        check_against_model(orc[0], plan, num, cs, inp, frames, r, prec, tag + (label,))
        if prec == 'f64':
            same_verdicts(base, r, tag + (label, 'default / edge'))
    clear_switches(monkeypatch)
    return seen


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('name', ['P22', 'R43', 'D22', 'C44'])
def test_dispatch_edges(C, orc, monkeypatch, name, prec):
    """Each switch select_mimo reads for the spatial chains -- LTE_DSP_STAGE=0
    (estimates gathered per RE), LTE_SPATIAL_HP=0 and an H capture (interpolated
    H through HBM), the separate transmitter and channel kernels (k_channel_tay
    and its forms, k_channel_mimo), the block FFT receiver for the wave one, the
    per-pair transmitter -- on flat links at N = 128 (P22), Rayleigh links at
    N = 512 (R43), 1024 (D22) and 2048 (C44: the sizes the wave receiver and the
    per-frame transmitter exist for).  Every run is checked like a ladder run and
    takes the path lte_run_path names; in f64 every path gives the default
    path's decisions bit for bit.  At least three distinct paths occur."""
    cs = M.CASES[name]
    inp, frames = every(*M.case_frames(*orc, name), EDGE_STRIDE)
    assert 0 < sum(f['crc'] for f in frames) < len(frames)
    seen = run_edges(C, orc, monkeypatch, cs, inp, frames, prec, (name, prec))
    assert len(seen) >= 3, seen


FLAT20 = dict(bw=20.0, mod='64-QAM', chan='awgn', prof='Pedestrian_A', n_bits=6121, ntx=4, nrx=4, rank=4, det='MMSE',
              snr=(24.0, 40.0))


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_flat_links_at_2048(C, orc, monkeypatch, prec):
    """Flat links at N = 2048 (config 5's shape with the coded streams): the
    fused transmitters k_ofdm_txch_flat / _pr / _w read the coded bits through
    tx_map -- forms no ladder case reaches.  8 frames against the model."""
    O, MO, T = orc
    inp = M.case_inputs(O, MO, T, FLAT20, frames=8)
    num = M.numerology(O, FLAT20)
    frames = [M.frame(O, MO, T, num, FLAT20, inp['bits'][f], float(inp['snrs'][f]), inp['draws'][f]) for f in range(8)]
    seen = run_edges(C, orc, monkeypatch, FLAT20, inp, frames, prec, ('flat20', prec))
    txs = {dict(p)['tx'] for p in seen}
    assert {'k_ofdm_txch_flat', 'k_ofdm_txch_flat_pr', 'k_ofdm_tx_mimo_frame'} <= txs, txs
    assert ('k_ofdm_txch_flat_w' in txs) == (prec == 'f64'), txs          # the wave transmitter is float64's
    assert 0 < sum(f['crc'] for f in frames) < 8


# ---------------------------------------------------------------------------
# (3) Philox draws
GRID_T, SEED = 4096, 77


def philox_ids(S):
    return np.concatenate([np.arange(8), S * GRID_T - 8 + np.arange(8)]).astype(np.uint64)


@pytest.mark.parametrize('name,velocity', [(n, 0.0) for n in M.CASES] + [('R44', 3.0)])
def test_philox_frames(C, orc, monkeypatch, name, velocity):
    """No injection: LTE_CHAIN_SPATIAL's streams (philox.sm_draws) and k_payload's
    payload.  The first and last 8 frame ids of a 2-point x 4096-trial grid whose
    points sit a quarter into the case's window from either end; per-frame bit
    errors and CRC verdicts equal the model's.  3 km/h: the per-symbol Taylor
    sets of every link."""
    from oracle import philox as P
    O, MO, T = orc
    clear_switches(monkeypatch)
    cs = M.CASES[name]
    plan, num = case_plan(C, orc, cs, 'f64', max_frames=16, velocity_kmh=velocity)
    lo, hi = cs['snr']
    snrs = np.array([lo + 0.25 * (hi - lo), lo + 0.75 * (hi - lo)])
    ids = philox_ids(len(snrs))
    si = (ids // GRID_T).astype(np.int32)
    r = plan.run(snrs[si], snr_index=si, n_snr=len(snrs), seed=SEED, frame_ids=ids)
    fD = O.doppler_hz(2.0, velocity) if velocity else 0.0
    fr = [M.philox_frame(O, MO, T, P, num, cs, SEED, int(i), float(snrs[s]), fD=fD) for i, s in zip(ids, si)]
    assert [int(e) for e in r['frame_errors']] == [f['errs'] for f in fr], (name, velocity, r.path)
    assert [bool(c) for c in r['crc_ok']] == [f['crc'] for f in fr], (name, velocity)
    want = np.zeros((2, 4), dtype=np.uint64)
    for s, f in zip(si, fr):
        want[s] += np.array([f['errs'], cs['n_bits'], 0 if f['crc'] else 1, 1], dtype=np.uint64)
    assert np.array_equal(r['counts'], want)


# ---------------------------------------------------------------------------
# (4) public API
API_SNRS = [4.0, 12.0, 20.0]
API_T, API_SEED = 6, 5
API_SP = {'num_tx': 2, 'num_rx': 2, 'rank': 2, 'detector': 'MMSE', 'pmi': 0}


def simulator(cs, prec='f64'):
    import lte_phy
    return lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=cs['bw'], modulation=cs['mod']), channel_type=cs['chan'],
                                 itu_profile=cs['prof'], precision=prec)


def test_run_grid_coded_spatial(C, orc):
    """run_grid(coded=True, mimo='spatial'): the new chain, sharding-invariant,
    equal to a plan-level run and to the model frame by frame."""
    from oracle import philox as P
    O, MO, T = orc
    cs = M.CASES['P22']
    num = M.numerology(O, cs)
    sim = simulator(cs)
    kw = dict(seed=API_SEED, coded=True, mimo='spatial', spatial=API_SP, n_bits=cs['n_bits'], frames_per_call=8,
              turbo_iters=ITERS)
    full = sim.run_grid(API_SNRS, API_T, **kw)
    assert full['plan'].chain == C.CHAIN_SPATIAL_CODED and full['plan'].coded and full['plan'].mimo
    parts = [sim.run_grid(API_SNRS, API_T, rank=k, world_size=2, **kw) for k in range(2)]
    assert np.array_equal(parts[0]['counts'] + parts[1]['counts'], full['counts'])
    ids = np.arange(len(API_SNRS) * API_T, dtype=np.uint64)
    si = (ids // API_T).astype(np.int32)
    plan, _ = case_plan(C, orc, cs, 'f64', max_frames=len(ids))
    r = plan.run(np.asarray(API_SNRS)[si], snr_index=si, n_snr=len(API_SNRS), seed=API_SEED, frame_ids=ids)
    assert np.array_equal(r['counts'], full['counts'])
    want = np.zeros((len(API_SNRS), 4), dtype=np.uint64)
    for i, s in zip(ids, si):
        f = M.philox_frame(O, MO, T, P, num, cs, API_SEED, int(i), API_SNRS[s])
        want[s] += np.array([f['errs'], cs['n_bits'], 0 if f['crc'] else 1, 1], dtype=np.uint64)
    assert np.array_equal(full['counts'], want), (full['counts'], want)
    assert 0 < int(full['counts'][:, 2].sum()) < len(ids)       # the window straddles the cliff
    assert sim.run_grid(API_SNRS[:1], 1, seed=1, coded=True, mimo='spatial', spatial=API_SP,
                        frames_per_call=1)['plan'].n_bits == 27760                      # the default TB size


def test_run_grid_early_stop(C, orc):
    """early_stop=True on the new chain: 'turbo_iters_hist' is the histogram of
    the rule evaluated by the oracle on the model's LLRs of the same frames."""
    from oracle import philox as P
    O, MO, T = orc
    cs = M.CASES['P22']
    num = M.numerology(O, cs)
    sim = simulator(cs)
    iters = 4
    kw = dict(seed=API_SEED, coded=True, mimo='spatial', spatial=API_SP, n_bits=cs['n_bits'], frames_per_call=8,
              turbo_iters=iters)
    g = sim.run_grid(API_SNRS, API_T, early_stop=True, **kw)
    hist = g['turbo_iters_hist']
    assert hist.dtype == np.uint64 and hist.shape == (len(API_SNRS), iters + 1)
    want = np.zeros_like(hist)
    for s in range(len(API_SNRS)):
        for t in range(API_T):
            f = M.philox_frame(O, MO, T, P, num, cs, API_SEED, s * API_T + t, API_SNRS[s], iters=iters)
            coded = len(f['tx']['coded'])
            src = M.deinterleave_index(coded // num.bps, num.Nd)
            L = f['llr'].reshape(-1, num.bps)[src].reshape(-1)[:coded]
            for n in M.early_stop_n_star(O, L, f['tx']['plan'], iters):
                want[s, n] += 1
    assert np.array_equal(hist, want), (hist, want)
    assert len(set(np.flatnonzero(want.sum(axis=0)).tolist())) >= 2     # more than one stopping iteration occurs
    assert g['plan'].path([0.0])['turbo'] == 'es'
    assert 'turbo_iters_hist' not in sim.run_grid(API_SNRS[-1:], 2, **kw)


CODING_KEYS = {'transmitted_bits', 'received_bits', 'bits_received_array', 'bit_errors', 'ber', 'crc_pass', 'snr_db',
               'coded_bits_length', 'symbols_rx', 'noise_var_mean'}


@pytest.mark.parametrize('name,snr', [('R43', 12.0), ('R43', 20.0), ('P22', 14.0), ('M21', 4.0), ('Z42', 14.0)])
def test_simulate_spatial_multiplexing_coded_ref_compat(C, orc, name, snr):
    """One call on the seeded global RNG equals the model on the draws
    simulate_spatial_multiplexing's order gives (H_initial, TX pilot reseeds,
    transmit_sm_draws, RX pilot reseeds), 8 iterations, and leaves the RNG where
    simulate_spatial_multiplexing leaves it on a frame of the same length."""
    import lte_phy
    O, MO, T = orc
    cs = M.CASES[name]
    num = M.numerology(O, cs)
    cfg = lte_phy.LTEConfig(bandwidth=cs['bw'], modulation=cs['mod'])
    bits = np.random.RandomState(3).randint(0, 2, cs['n_bits'])
    args = (cs['ntx'], cs['nrx'], cs['rank'], cs['det'], snr, cfg, cs['chan'], cs['prof'], 0, 2.0, True)
    np.random.seed(11)
    r = lte_phy.simulate_spatial_multiplexing_coded(bits, *args)
    state = np.random.get_state()
    assert set(r) == CODING_KEYS | {'rank', 'pmi_used', 'precoder_matrix', 'channel_matrix', 'num_tx', 'num_rx',
                                    'detector_type'}
    assert (r['rank'], r['pmi_used']) == (cs['rank'], 0) and np.array_equal(r['precoder_matrix'], M.precoder(T, cs))
    L = M.frame_len(O, MO, T, num, cs)
    np.random.seed(11)
    np.random.randn(cs['nrx'], cs['ntx'])
    np.random.randn(cs['nrx'], cs['ntx'])                       # H_initial
    for t, pi in enumerate(MO.mimo_pilot_indices(num, cs['ntx'])):
        O.pilots(t % 4, len(pi))                                # the TX pilot reseeds: the draws follow the last one
    draws = MO.transmit_sm_draws(cs['ntx'], cs['nrx'], cs['chan'], L, cs['prof'])
    fr = M.frame(O, MO, T, num, cs, bits, snr, draws, iters=8)
    assert np.array_equal(r['bits_received_array'], fr['bits_rx']) and r['crc_pass'] == fr['crc']
    assert r['bit_errors'] == fr['errs'] and r['coded_bits_length'] == len(fr['tx']['coded'])
    assert np.allclose(r['channel_matrix'], fr['channel_matrix'], rtol=1e-12, atol=0)
    src = M.deinterleave_index(len(fr['tx']['coded']) // num.bps, num.Nd)
    unit = 4 * M.R_CPU * EPS['f64'] * (fr['rx']['kappa'] / fr['rx']['mu_min'])[src]
    assert np.all(np.abs(r['symbols_rx'] - fr['z'][src]) <= unit * fr['rx']['z_norm'][src])
    assert abs(r['noise_var_mean'] / float(np.mean(fr['nv'][src])) - 1) < 1e-9
    # simulate_spatial_multiplexing on a frame of the same length consumes the same numbers
    np.random.seed(11)
    n_sym = L // (num.N + num.cp)
    lte_phy.simulate_spatial_multiplexing(np.zeros(n_sym * num.Nd * num.bps, dtype=int), *args[:4],
                                          modulation=cs['mod'], snr_db=snr, config=cfg, channel_type=cs['chan'],
                                          itu_profile=cs['prof'], velocity_kmh=0, frequency_ghz=2.0)
    after = np.random.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(state[1:], after[1:]))


def test_uncoded_spatial_chain_is_unchanged(C, orc):
    """LTE_CHAIN_SPATIAL runs of the same plan shape before and after a coded
    run in the same session: the same bits, errors and symbols, and the oracle's
    config-5 frame."""
    from oracle import philox as P
    from lte_phy import ofdm_core
    import lte_phy
    O, MO, T = orc
    cs = M.CASES['R44']
    cfg = lte_phy.LTEConfig(bandwidth=cs['bw'], modulation=cs['mod'])
    num = M.numerology(O, cs)
    nb = 2 * num.Nd * num.bps
    hard = ofdm_core._spatial_plan(cfg, cs['chan'], cs['prof'], 0.0, 2.0, 2, nb, 8, precision='f64')[0]
    assert hard.chain == C.CHAIN_SPATIAL and not hard.coded
    ids = np.arange(8, dtype=np.uint64)
    snrs = np.full(8, 20.0)
    before = hard.run(snrs, seed=SEED, frame_ids=ids, capture=('bits_rx', 'data_syms'))
    soft, _ = case_plan(C, orc, cs, 'f64', max_frames=8)
    soft.run(snrs, seed=SEED, frame_ids=ids)
    after = hard.run(snrs, seed=SEED, frame_ids=ids, capture=('bits_rx', 'data_syms'))
    assert before.path == after.path and before.path['dematch'] == 'none'
    for k in ('bits_rx', 'data_syms', 'frame_errors', 'counts'):
        assert np.array_equal(before[k], after[k]), k
    L = hard.L
    o = MO.simulate_spatial(num, P.payload_bits(SEED, 0, nb), 20.0, 4, 4, 4, cs['chan'], cs['prof'], velocity_kmh=0,
                            draws=P.sm_draws(SEED, 0, L, 4, 4, cs['chan'], M.n_paths(O, num, cs)))
    assert int(before['frame_errors'][0]) == o['bit_errors']
    assert np.array_equal(before['bits_rx'][0], o['bits_received_array'])
