"""GPU: the coded SC-FDM chain (LTE_CHAIN_SCFDM_CODED: DFT precoder, soft MMSE /
ZF frequency-domain equaliser, turbo coding) against the NumPy model of
tests/scfdm_coded_model.py, which composes the oracle's primitives (never
against another GPU run, except where a test is about two paths agreeing).

  (1) the ladder of scfdm_coded_model.CASES (N = 128 .. 2048: a slot of 16 .. 256
      threads; both rules; 1, 2 and 5 RX), 67 frames over the turbo cliff at 2
      iterations (tests/test_scfdm_coded_host.py asserts from the model alone
      that each case passes and fails at least 8 frames), injected bits / phases
      / noise, f64 and f32
  (2) the zero-padded last symbol; every switch select_siso reads; determinism
  (3) Philox draws, frame ids from both ends of a 4096-trial grid, fD = 0 and 3 km/h
  (4) run_scfdm_grid, early_stop, simulate_scfdm_coded, HARQ's refusal, and
      simulate_siso_coded's indifference to enable_sc_fdm

Bars: tx_syms exact (f32 1e-6); noise_power 1e-12 (f32 2e-6); z within 4 x
R_CPU_Z x eps x ||z_sym||_2 / mu_sym and LLRs within 4 x R_CPU_LLR x eps x (1 +
|LLR|) / mu_sym of the model's (scfdm_coded_model.R_CPU_*: the spread of two
NumPy evaluations of the rule; eps = 2^-52, f32 2^-23 with the LLRs against the
model's demapper on the run's own z, as the suite forms its float32 LLR
references); bits, error counts, CRC verdicts and counters identical to the
oracle's decode of the run's own LLRs (f32: turbo_decode_f32_model), in f64
also to the model's own decisions."""
import ctypes

import numpy as np
import pytest

import scfdm_coded_model as M
from test_gpu_simo_coded import SWITCHES

pytestmark = pytest.mark.gpu

FRAMES, ITERS = M.FRAMES, M.ITERS
TOL = {'f64': dict(npow=1e-12, eps=2.0 ** -52, tx=0.0), 'f32': dict(npow=2e-6, eps=2.0 ** -23, tx=1e-6)}
VERDICTS = ('bits_rx', 'crc_ok', 'frame_errors', 'counts')
CAP = ('tx_syms', 'llr', 'bits_rx', 'noise_power', 'data_syms')
MARGIN = 4.0
_SEP = 'k_rx_chest+k_rx_data'


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    _capi.device_init()
    return _capi


def clear_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def simulator(cs, prec, velocity_kmh=0.0, **kw):
    import lte_phy
    return lte_phy.OFDMSimulator(lte_phy.LTEConfig(bandwidth=cs['bw'], modulation=cs['mod']), channel_type=cs['chan'],
                                 itu_profile=cs['prof'], frequency_ghz=2.0, velocity_kmh=velocity_kmh, precision=prec,
                                 **kw)


def case_plan(C, O, name, prec, max_frames=FRAMES, velocity_kmh=0.0, early_stop=False, iters=ITERS):
    cs = M.CASES[name]
    num = M.numerology(O, cs)
    det = C.DET_MMSE if cs['eq'] == 'mmse' else C.DET_ZF
    plan = simulator(cs, prec, velocity_kmh)._plan(C.CHAIN_SCFDM_CODED, 0, cs['n_bits'], num_rx=cs['nrx'],
                                                   max_frames=max_frames, iters=iters, early_stop=early_stop,
                                                   detector=det)
    assert plan.coded and not plan.mimo and plan.chain == 9 and plan.num_rx == cs['nrx']
    assert plan.desc.sc_fdm == 0 and plan.desc.detector == det
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


def chain_path(num, cs, captured_stream=False, tx_stage=None):
    """The path of section 2 of the design: the per-symbol transmitter (with the
    channel fused in from N = 512 on Rayleigh, unless a stream is captured) and
    the separate receiver kernels writing LLRs.  The coded stream is staged in
    LDS except in float64, where the two symbol buffers fill the 64 KB."""
    fused = num.N >= 512 and cs['chan'] == 'rayleigh_mp' and not captured_stream
    return {'tx': 'k_ofdm_tx_ch' if fused else 'k_ofdm_tx', 'tx_stage': tx_stage, 'ch_fix': '1' if fused else '0',
            'rx': _SEP, 'xhand': '0', 'dematch': 'llr'}


def expect_path(r, num, cs, prec, **kw):
    want = chain_path(num, cs, **kw)
    want['tx_stage'] = r.path['tx_stage'] if want['tx_stage'] is None else want['tx_stage']
    assert r.path == want, (r.path, want)
    if prec == 'f64':
        assert r.path['tx_stage'] == '0', r.path
    assert not any(v.endswith('_w') for v in r.path.values())


def check_against_model(O, plan, num, cs, inp, frames, r, prec, tag):
    """One run with the captures CAP against the model, frame by frame; no frame
    is left out of any comparison.  Returns the worst (z, LLR) ratios in units
    of eps ||z_sym|| / mu_sym and eps (1 + |LLR|) / mu_sym, and the noise_power error."""
    tol, f32 = TOL[prec], prec == 'f32'
    coded = plan.coded_bits
    seg = frames[0]['tx']['plan']
    pos = M.deinterleave_index(len(frames[0]['tx']['qam']), num.Nd)
    worst_z = worst_llr = worst_np = 0.0
    errs, oks = [], []
    assert len(frames) == len(r['llr']) == FRAMES
    for b, fr in enumerate(frames):
        where = tag + (b,)
        assert coded == len(fr['tx']['coded']) and plan.n_sym == fr['tx']['n_ofdm']
        ts = r['tx_syms'][b].astype(np.complex128)
        assert np.max(np.abs(ts[pos] - fr['tx']['qam'])) <= tol['tx'], where
        assert np.max(np.abs(ts - fr['tx']['grid'].reshape(-1))) <= tol['tx'], where      # padding zeros included
        snr = float(inp['snrs'][b])
        zg = r['data_syms'][b].astype(np.complex128)
        dz, dl = M.deviation(O, num, fr['z'], fr['nv'], fr['mu'], zg, fr['nv'], eps=tol['eps'], llr2=r['llr'][b])
        if f32:          # LLRs: the model's demapper and nv on the run's own z (which dz ties to the model's)
            dl = M.deviation(O, num, zg, fr['nv'], fr['mu'], zg, fr['nv'], eps=tol['eps'], llr2=r['llr'][b])[1]
        worst_z, worst_llr = max(worst_z, dz), max(worst_llr, dl)
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
    print(f'scfdm coded {tag}: worst z ratio {worst_z:.4g} (bar {MARGIN * M.R_CPU_Z:.4g}), LLR ratio {worst_llr:.4g} '
          f'(bar {MARGIN * M.R_CPU_LLR:.4g}), noise_power rel err {worst_np:.3g}, {sum(oks)} pass / '
          f'{FRAMES - sum(oks)} fail, path {r.path}')
    assert worst_z <= MARGIN * M.R_CPU_Z, tag + (worst_z,)
    assert worst_llr <= MARGIN * M.R_CPU_LLR, tag + (worst_llr,)
    assert worst_np <= tol['npow'], tag + (worst_np,)
    assert sum(oks) >= M.MIN_PASS and FRAMES - sum(oks) >= M.MIN_FAIL
    want = np.array([[sum(errs), FRAMES * cs['n_bits'], FRAMES - sum(oks), FRAMES]], dtype=np.uint64)
    assert np.array_equal(r['counts'], want), (r['counts'], want)
    return worst_z, worst_llr, worst_np


# ---------------------------------------------------------------------------
# (1) the ladder
@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('name', list(M.CASES))
def test_ladder(C, oracle, monkeypatch, name, prec):
    """k_payload / k_encode / k_ofdm_tx<CODED, SCF> (with the channel from N = 512
    on) / k_rx_chest / k_rx_data<SCFDM_CODED> (slot_sum, weights, IDFT, 1 / mu,
    LLRs) / k_dematch / k_turbo* / k_crc_count / k_accumulate."""
    clear_switches(monkeypatch)
    plan, num, cs = case_plan(C, oracle, name, prec)
    inp, frames = M.case_frames(oracle, name)
    assert plan.L == inp['L']
    r = plan.run(inp['snrs'], **inject(inp), capture=CAP)
    expect_path(r, num, cs, prec)
    check_against_model(oracle, plan, num, cs, inp, frames, r, prec, (name, prec))


# ---------------------------------------------------------------------------
# (2) padding, switches, determinism
def test_zero_padded_last_symbol(C, oracle, monkeypatch):
    """B1L: the grid holds zeros past the coded symbols (the last row of the T/F
    interleaver, so the last RE of the later subcarriers' columns: spread over
    the OFDM symbols).  They are precoded and equalised like any symbol: z and
    the LLRs of all n_sym * Nd REs equal the model's, and the decode reads none
    of the dropped positions (the oracle's decode of the first coded_bits
    de-interleaved LLRs gives the run's bits)."""
    clear_switches(monkeypatch)
    plan, num, cs = case_plan(C, oracle, 'B1L', 'f64')
    inp, frames = M.case_frames(oracle, 'B1L')
    r = plan.run(inp['snrs'], **inject(inp), capture=CAP)
    n_re = plan.n_sym * num.Nd
    pad = n_re - plan.coded_bits // num.bps
    assert pad >= 1 and plan.n_re_bits == n_re * num.bps and r['llr'].shape == (FRAMES, n_re * num.bps)
    eps = TOL['f64']['eps']
    for b, fr in enumerate(frames):
        grid = fr['tx']['grid'].reshape(-1)
        assert np.count_nonzero(grid == 0) == pad and np.array_equal(r['tx_syms'][b] == 0, grid == 0)
        zg = r['data_syms'][b].astype(np.complex128).reshape(plan.n_sym, num.Nd)
        holed = np.flatnonzero(np.any(fr['tx']['grid'] == 0, axis=1))  # the symbols that carry zeros
        assert len(holed) >= 1
        for l in holed:
            zm = fr['z'].reshape(plan.n_sym, num.Nd)[l]
            assert np.max(np.abs(zg[l] - zm)) <= MARGIN * M.R_CPU_Z * eps * np.linalg.norm(zm) / fr['mu'][l], (b, l)
        Lm = M.llrs_re_order(oracle, num, fr['z'], fr['nv'])
        Lg = r['llr'][b].astype(np.float64)
        lim = MARGIN * M.R_CPU_LLR * eps * (1 + np.abs(Lm)) / np.repeat(fr['mu'], num.Nd * num.bps)
        assert np.all(np.abs(Lg - Lm) <= lim), b                       # every RE, the padded ones too
        dec, ok = M.decode_llrs(oracle, num, fr['tx']['plan'], plan.coded_bits, Lg)
        assert np.array_equal(dec, r['bits_rx'][b]) and bool(ok) == bool(r['crc_ok'][b]) == fr['crc']


def test_switches_leave_the_path_and_the_outputs(C, oracle, monkeypatch):
    """Every switch select_siso consults, at 0 and at 1, on B1M in float64: the
    path is the chain's own and all captures are those of the run without
    switches -- except LTE_TXCH_FUSE=0, which takes the separate channel kernel
    (the chain's path for N < 512), and LTE_TX_STAGE, which has nothing to stage
    in float64.  Each run is also held to the model."""
    clear_switches(monkeypatch)
    plan, num, cs = case_plan(C, oracle, 'B1M', 'f64')
    inp, frames = M.case_frames(oracle, 'B1M')
    kw = inject(inp)
    base = plan.run(inp['snrs'], **kw, capture=CAP)
    expect_path(base, num, cs, 'f64')
    check_against_model(oracle, plan, num, cs, inp, frames, base, 'f64', ('B1M', 'base'))
    for name in SWITCHES:
        for v in ('0', '1'):
            clear_switches(monkeypatch)
            monkeypatch.setenv(name, v)
            r = plan.run(inp['snrs'], **kw, capture=CAP)
            unfused = (name, v) == ('LTE_TXCH_FUSE', '0')
            expect_path(r, num, cs, 'f64', captured_stream=unfused)
            assert r.path['tx_stage'] == '0'
            same_verdicts(base, r, (name, v))
            assert np.array_equal(r['tx_syms'], base['tx_syms']), (name, v)
            if unfused:      # another channel kernel: the model's bars, not bit equality
                check_against_model(oracle, plan, num, cs, inp, frames, r, 'f64', ('B1M', name, v))
            else:
                for k in ('llr', 'data_syms', 'noise_power'):
                    assert np.array_equal(r[k], base[k]), (name, v, k)
    q = plan.run(inp['snrs'], **kw, capture=('bits_rx',))             # no LLR capture: still the LLR path
    clear_switches(monkeypatch)
    assert q.path['dematch'] == 'llr'
    same_verdicts(base, q, 'no llr capture')


def test_tx_stage_switch_f32(C, oracle, monkeypatch):
    """float32 stages the coded stream behind the two symbol buffers;
    LTE_TX_STAGE=0 gathers from global memory.  The same symbols either way."""
    clear_switches(monkeypatch)
    plan, num, cs = case_plan(C, oracle, 'B1M', 'f32')
    inp, frames = M.case_frames(oracle, 'B1M')
    a = plan.run(inp['snrs'], **inject(inp), capture=CAP)
    assert a.path['tx_stage'] == '1', a.path
    monkeypatch.setenv('LTE_TX_STAGE', '0')
    b = plan.run(inp['snrs'], **inject(inp), capture=CAP)
    assert b.path['tx_stage'] == '0' and b.path['tx'] == a.path['tx'], b.path
    for k in CAP:
        assert np.array_equal(a[k], b[k]), k
    check_against_model(oracle, plan, num, cs, inp, frames, b, 'f32', ('B1M', 'f32', 'tx_stage0'))


@pytest.mark.parametrize('name', ['A2Z', 'D2M', 'C1M'])
def test_two_runs_give_the_same_bits(C, oracle, monkeypatch, name):
    """The reduction has a fixed order: two identical runs, bit-identical LLRs
    (slots of a quarter wave, of 2 waves and of 4 waves)."""
    clear_switches(monkeypatch)
    plan, num, cs = case_plan(C, oracle, name, 'f64')
    inp, _ = M.case_frames(oracle, name)
    a = plan.run(inp['snrs'], **inject(inp), capture=('llr', 'data_syms'))
    b = plan.run(inp['snrs'], **inject(inp), capture=('llr', 'data_syms'))
    assert np.array_equal(a['llr'].view(np.uint64), b['llr'].view(np.uint64))
    assert np.array_equal(a['data_syms'].view(np.uint64), b['data_syms'].view(np.uint64))


# ---------------------------------------------------------------------------
# (3) Philox draws
GRID_T, SEED = 4096, 77


def philox_ids(S):
    return np.concatenate([np.arange(8), S * GRID_T - 8 + np.arange(8)]).astype(np.uint64)


@pytest.mark.parametrize('name,velocity', [('A1M', 0.0), ('A2Z', 0.0), ('E1M', 0.0), ('B1M', 0.0), ('B5M', 0.0),
                                           ('D2M', 0.0), ('C1Z', 0.0), ('B1M', 3.0), ('D2M', 3.0)])
def test_philox_frames(C, oracle, name, velocity):
    """No injection: the transmitter and channel draw LTE_CHAIN_SIMO's streams
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
    expect_path(r, num, cs, 'f64')
    fD = O.doppler_hz(2.0, velocity) if velocity else 0.0
    fr = [M.philox_frame(O, P, num, cs, SEED, int(i), float(snrs[s]), fD=fD) for i, s in zip(ids, si)]
    assert [int(e) for e in r['frame_errors']] == [f['errs'] for f in fr], (name, velocity)
    assert [bool(c) for c in r['crc_ok']] == [f['crc'] for f in fr], (name, velocity)
    want = np.zeros((2, 4), dtype=np.uint64)
    for s, f in zip(si, fr):
        want[s] += np.array([f['errs'], cs['n_bits'], 0 if f['crc'] else 1, 1], dtype=np.uint64)
    assert np.array_equal(r['counts'], want)


# ---------------------------------------------------------------------------
# (4) public API
API_T, API_SEED = 8, 5


def test_run_scfdm_grid(C, oracle):
    """run_scfdm_grid on a 2-SNR x 8-trial grid: counts equal the sum of the
    model's per-frame verdicts, for either rule, and are sharding-invariant."""
    from oracle import philox as P
    O = oracle
    for name in ('A1M', 'A2Z'):
        cs = M.CASES[name]
        num = M.numerology(O, cs)
        lo, hi = cs['snr']
        snrs = [lo + 0.35 * (hi - lo), lo + 0.65 * (hi - lo)]
        sim = simulator(cs, 'f64')
        kw = dict(seed=API_SEED, num_rx=cs['nrx'], equalizer=cs['eq'], n_bits=cs['n_bits'], frames_per_call=8,
                  turbo_iters=ITERS)
        full = sim.run_scfdm_grid(snrs, API_T, **kw)
        assert full['plan'].chain == C.CHAIN_SCFDM_CODED and full['plan'].num_rx == cs['nrx'] and full['plan'].coded
        parts = [sim.run_scfdm_grid(snrs, API_T, rank=k, world_size=2, **kw) for k in range(2)]
        assert np.array_equal(parts[0]['counts'] + parts[1]['counts'], full['counts'])
        want = np.zeros((2, 4), dtype=np.uint64)
        for s in range(2):
            for t in range(API_T):
                f = M.philox_frame(O, P, num, cs, API_SEED, s * API_T + t, snrs[s])
                want[s] += np.array([f['errs'], cs['n_bits'], 0 if f['crc'] else 1, 1], dtype=np.uint64)
        assert np.array_equal(full['counts'], want), (name, full['counts'], want)
        assert 0 < int(full['counts'][:, 2].sum()) < 2 * API_T, name    # the grid straddles the cliff
        assert np.array_equal(full['bler'], want[:, 2] / want[:, 3])


def test_run_scfdm_grid_early_stop(C, oracle):
    """early_stop=True: per code block the iteration count and the bits of the
    early-stop rule evaluated with the oracle's decoders on the model's LLRs."""
    from oracle import philox as P
    O = oracle
    cs = M.CASES['A1M']
    num = M.numerology(O, cs)
    iters = 4
    snrs = [2.0, 4.5]
    sim = simulator(cs, 'f64')
    kw = dict(seed=API_SEED, num_rx=1, equalizer='mmse', n_bits=cs['n_bits'], frames_per_call=16, turbo_iters=iters)
    g = sim.run_scfdm_grid(snrs, API_T, early_stop=True, **kw)
    hist = g['turbo_iters_hist']
    assert hist.dtype == np.uint64 and hist.shape == (2, iters + 1)
    ids = np.arange(2 * API_T, dtype=np.uint64)
    si = (ids // API_T).astype(np.int32)
    plan = sim._plan(C.CHAIN_SCFDM_CODED, 0, cs['n_bits'], max_frames=16, iters=iters, early_stop=True)
    r = plan.run(np.asarray(snrs)[si], snr_index=si, n_snr=2, seed=API_SEED, frame_ids=ids, capture=('bits_rx',))
    assert r.path['turbo'] == 'es'
    want = np.zeros_like(hist)
    for i, s in zip(ids, si):
        f = M.philox_frame(O, P, num, cs, API_SEED, int(i), snrs[s], iters=iters)
        seg = f['tx']['plan']
        n_star = M.early_stop_n_star(O, f['llr'], seg, iters)
        assert [int(v) for v in r['turbo_iters_used'][i]] == n_star, int(i)
        dec, ok = O.coded_rx_decode(f['llr'], seg, f['tx']['rm_lens'], n_star[0])      # (one code block)
        assert len(seg) == 1 and np.array_equal(dec, r['bits_rx'][i]) and bool(ok) == bool(r['crc_ok'][i]), int(i)
        for n in n_star:
            want[s, n] += 1
    assert np.array_equal(hist, want), (hist, want)
    assert len(np.flatnonzero(want.sum(axis=0))) >= 2                   # more than one stopping iteration occurs
    assert 'turbo_iters_hist' not in sim.run_scfdm_grid(snrs[-1:], 2, **kw)


SIMO_CODED_KEYS = {'transmitted_bits', 'received_bits', 'bits_received_array', 'bit_errors', 'ber', 'crc_pass',
                   'snr_db', 'papr_db', 'papr_linear', 'coded_bits_length', 'signal_tx', 'signal_rx_list',
                   'symbols_tx', 'symbols_rx', 'channel_gain', 'noise_var_mean', 'num_rx', 'combining_method'}


@pytest.mark.parametrize('name,snr', [('B1M', 12.0), ('B1Z', 16.0), ('A2Z', 1.0)])
def test_simulate_scfdm_coded_ref_compat(C, oracle, name, snr):
    """One call on the seeded global RNG equals the model on ref_compat_draws
    (simulate_simo's order), 8 iterations; enable_sc_fdm does not matter."""
    O = oracle
    cs = M.CASES[name]
    num = M.numerology(O, cs)
    bits = np.random.RandomState(3).randint(0, 2, cs['n_bits'])
    out = []
    for flag in (False, True):
        sim = simulator(cs, 'f64', enable_sc_fdm=flag)
        np.random.seed(11)
        out.append(sim.simulate_scfdm_coded(bits, snr, num_rx=cs['nrx'], equalizer=cs['eq']))
    r = out[0]
    assert set(r) == SIMO_CODED_KEYS | {'equalizer'} and r['equalizer'] == cs['eq']
    for k in r:
        assert np.array_equal(np.asarray(r[k]), np.asarray(out[1][k])), k
    L = len(r['signal_tx'])
    np.random.seed(11)
    draws = O.ref_compat_draws(num, cs['chan'], L, cs['nrx'], cs['prof'])
    fr = M.frame(O, num, cs, bits, snr, draws, iters=8)
    assert np.array_equal(r['bits_received_array'], fr['bits_rx']) and r['crc_pass'] == fr['crc']
    assert r['bit_errors'] == fr['errs'] and r['coded_bits_length'] == len(fr['tx']['coded'])
    assert np.array_equal(r['symbols_tx'], fr['tx']['qam'])
    assert np.linalg.norm(r['signal_tx'] - fr['tx']['signal']) <= 1e-13 * np.linalg.norm(fr['tx']['signal'])
    for a in range(cs['nrx']):
        assert np.linalg.norm(r['signal_rx_list'][a] - fr['rxs'][a]) <= 1e-13 * np.linalg.norm(fr['rxs'][a])
    pa = O.papr(fr['tx']['signal'])
    assert abs(r['papr_db'] - pa['papr_db']) < 1e-9                    # of the DFT-spread stream
    src = M.deinterleave_index(len(fr['tx']['coded']) // num.bps, num.Nd)
    assert abs(r['noise_var_mean'] / float(np.mean(np.repeat(fr['nv'], num.Nd)[src])) - 1) < 1e-10
    zs = fr['z'][src]
    assert np.max(np.abs(r['symbols_rx'] - zs)) <= MARGIN * M.R_CPU_Z * 2.0 ** -52 * np.linalg.norm(fr['z']) / fr['mu'].min()


def test_harq_refuses_the_chain(C):
    lib = C.load()
    d, hd, h = C.PlanDesc(), C.HarqDesc(), ctypes.c_void_p()
    d.N, d.Nc, d.cp_len, d.bps, d.n_bits, d.max_frames = 128, 72, 9, 2, 435, 1
    d.chain, d.num_rx, hd.max_tx = C.CHAIN_SCFDM_CODED, 1, 4
    assert lib.lte_plan_create_harq(ctypes.byref(d), ctypes.byref(hd), ctypes.byref(h)) == C.LTE_EUNSUP
    assert b'HARQ' in lib.lte_last_error()


def test_simulate_siso_coded_keeps_ignoring_enable_sc_fdm(C, oracle):
    """The old behaviour, pinned: the reference's coded driver builds its grids
    without the precoder, so the flag changes nothing there -- and the result is
    the oracle's simulate_siso_coded."""
    cs = M.CASES['B1M']
    num = M.numerology(oracle, cs)
    bits = np.random.RandomState(4).randint(0, 2, cs['n_bits'])
    out = []
    for flag in (False, True):
        sim = simulator(cs, 'f64', enable_sc_fdm=flag)
        np.random.seed(21)
        out.append(sim.simulate_siso_coded(bits, 14.0))
    for k in out[0]:
        assert np.array_equal(np.asarray(out[0][k]), np.asarray(out[1][k])), k
    np.random.seed(21)
    o = oracle.simulate_siso_coded(num, bits, 14.0, 'rayleigh_mp', profile=cs['prof'])
    assert out[1]['bit_errors'] == o['bit_errors'] and out[1]['crc_pass'] == o['crc_pass']
    assert np.array_equal(out[1]['symbols_tx'], o['symbols_tx'])
