"""GPU: the multi-antenna chains (SFBC, spatial multiplexing, beamforming) and
uncoded SC-FDM on the device's own Philox draws -- the path run_grid and
bench.py take -- against the float64 oracle on the oracle's restatement of the
same draws (oracle/philox.py), off the bench shapes: never against another GPU
run.

Every case (tests/mimo_philox_cases.py) is B = 5 frames (odd: the last block is
partial) with the frame ids [0, 1, 2, 2^32 + 3, 65535] (the counter's frame_hi
word) and SNRs over the chain's useful range, through the plan the drop-in
builds (OFDMSimulator._sfbc_plan / _plan, ofdm_core._spatial_plan,
beamforming.bf_plan, or get_plan with a custom tap set), with no injection:
  run 1  plan.run(snrs, seed=, frame_ids=) alone -- the hot path; its
         Plan.run(...).path is asserted in full (PATHS[case][0]);
  run 2  with the captures (they change the path: PATHS[case][1] is asserted);
  flips  run 1 again with each switch of SWITCHES set to 0 that changes the
         case's path (Plan.path says so without running), each against the same
         oracle numbers.
The seeds are those of tests/mimo_philox_cases.py, chosen on the CPU;
tests/test_oracle_mimo_philox.py asserts from the oracle alone that every slicer
input of every case keeps its margin from every decision boundary, so in float64
the decisions are not at the mercy of round-off and the comparisons are exact.

float64 bars: frame_errors (and crc_ok) of every run identical to the oracle's;
bits_rx identical; and, the suite's own figures for the same quantities,
  signal_rx  relative L2 1e-13 (test_simulate_siso_signals_vs_oracle, TOL of
             tests/test_gpu_profiles.py)
  noise_power 1e-12 relative (test_wave_simo_tx_matches_block_tx, the same TOL)
  H          1e-12 of max|H| (the same TOL; beamforming: of the frame's max|H|)
  symbols    1e-12 times the RE's amplification of an input error: SFBC the
             Alamouti pair's mean_r 2 max|Y_r| max|h| / norm_r
             (mimo_philox_cases.sfbc_sym_scale, the MRC form of
             tests/test_gpu_profiles.py per pair); spatial kappa / mu_min ||s||
             of the RE's subcarrier (tests/test_gpu_spatial_coded.py's unit);
             SC-FDM SISO max|Y| / |H| per RE as the ZF form of
             tests/test_gpu_profiles.py, taken per OFDM symbol in L2 (the
             de-precoder is unitary), SIMO the MRC form; beamforming relative
             L2 1e-12 and gain 1e-9 dB (tests/test_gpu_bf.py)
  coded LLRs as test_sfbc_coded_llrs_and_decoding (tests/test_gpu_mimo.py)
             forms them: the oracle's max-log LLRs of the run's own combined
             symbols and estimates, 1e-12 of 1 + |LLR|, and the oracle's decode
             of the run's own LLRs equal to the run's bits and CRC verdict.
float32 (one case per family): |dBER| < 1e-3 over the case's 5 frames, captures
within TOL['f32'] of tests/test_gpu_profiles.py.

The cases and what each exists for (seed 1, the first seed that meets the
preconditions, for every case but sfbc_vb5_u: 403 and sfbc_pb20_c: 549; the
path fields each asserts are its PATHS entry below, all of them):
  SFBC, Rayleigh links unless stated (_u uncoded 3 symbols, _c TB 2041, 2 iterations)
    sfbc_pa20_u/_c      20 MHz 64-QAM PedA 2x2: sfbc_txch_supported and rx_sfbc_supported
                        hold, sfbc_merge: the baseline (fused TX, merged link noise)
    sfbc_pb20_u/_c      PedB, max_delay 114 > SFX_TL: MTX_PAIR (coded MTX_FRAME) +
                        k_channel_tay + lp_fuse, unmerged k_link_noise_pairs
    sfbc_vb20x_u        16-QAM VehB extended CP: 8 paths, max_delay 139, sym_len 2557 (J)
    sfbc_taps32/33_u    custom taps (0, 1, 31, 32) / (0, 33): both sides of SFX_TL
    sfbc_taps8/9_u      8 / 9 taps within 32 samples: both sides of TXCH_MAXP (9: lp_fuse off too)
    sfbc_taps_cp/cp1_u  10 MHz, max_delay = cp = 72 / 73: lp_fuse (k_link_power_fix) / k_link_power
    sfbc_vb5_u/_c       5 MHz QPSK VehB: N = 512, max_delay 35 against cp 36
    sfbc_pa125_rx1_u    1.25 MHz QPSK 2x1: N = 128 (below lp_fuse's N >= 512), MISO
    sfbc_pa15_c         15 MHz 64-QAM: N = 2048 with Nd = 749 (n_dsc, res against the LDS bounds)
    sfbc_rx3/4/5/8_u    2x3 / 2x4 / 2x5 / 2x8: no fused TX; k_rx_sfbc up to 4 RX; G = 3, 4, 1, 4
    sfbc_sym15_u        15 symbols: n_est = 2
    sfbc_awgn5_u        5 MHz 16-QAM flat links: MTX_FLAT in SFBC mode
  Spatial multiplexing, uncoded, 3 symbols
    sm_pb20_v3          20 MHz 64-QAM PedB 4x4 r4 MMSE 3 km/h: 6 paths, Taylor sets with econ
    sm_va20_v30         16-QAM VehA 30 km/h: exact_jakes, k_channel_mimo on Philox phases
    sm_vb20x_v3         16-QAM VehB extended CP: odd cp (block receiver), 8 paths, J for 2557
    sm_pb5_static       5 MHz 16-QAM PedB velocity 0: n_cs = 1, N = 512, Nd = 249 (last SC partly filled)
    sm_r2_pmi5_sic      5 MHz 16-QAM 4x4 rank 2 PMI 5 SIC flat: a non-identity precoder, SIC
    sm_r3_zf            10 MHz 16-QAM 4x3 rank 3 ZF PedA 3 km/h: N = 1024, num_rx < num_tx
    sm_22_pmi1_zf       1.25 MHz QPSK 2x2 r2 PMI 1 ZF flat: 2 TX, N = 128 (no flat_fuse)
    sm_42_r1_mrc        5 MHz 16-QAM 4x2 r1 PMI 3 MRC flat
    sm_15               15 MHz 64-QAM 4x4 r4 MMSE flat: Nd = 749 on the wave receiver and the staged detector
  Beamforming: (2,1) (4,1) (8,1) (2,4) (4,3) (8,5) (8,8) x adaptive / static, all three
    modulations; bf_21*: 1.25 MHz, 930 REs (k_bf_data's tail lanes); bf_88*: 20 MHz.  One
    path (tx=none rx=k_bf): k_bf_setup / k_bf_data have no switch.
  SC-FDM: sc_siso_pa5 (5 MHz 16-QAM PedA), sc_simo_flat125 (2 RX 1.25 MHz QPSK flat)

Predicates the public plan builders cannot cross:
  * tx_mimo_frame_supported's LDS bound and det_spatial_stage_supported's bound
    on num_rx * num_tx * maxP: no LTE numerology or antenna count the plans
    accept exceeds them (LTE_TXM_FRAME=0 / LTE_DSP_STAGE=0 take the other side).
  * sfbc_txch_supported's n_dsc <= 8 * (N >> 3): res <= Nd < N always.
  * rx_sfbc_supported's n_est == (n_sym + 13) / 14 and even res: the SFBC plans
    are built that way (res = Nd & ~1).
  * flat_fuse's num_tx <= 4: the spatial plans take 2 or 4 TX only.
  * lp_fuse's static-taps term (n_cs == 1, no exact Jakes) for SFBC: the oracle's
    transmit_mimo restates the reference's static links only, so an SFBC plan
    with fD != 0 has nothing to be compared with (the spatial cases cross n_cs
    and exact_jakes in channel_mimo_select).
"""
import numpy as np
import pytest

import mimo_philox_cases as K
from oracle import lte_oracle as O
from oracle import tm4_oracle as T

pytestmark = pytest.mark.gpu

B, IDS = K.B, K.IDS
SWITCHES = ('LTE_SFBC_TXCH_FUSE', 'LTE_SFBC_RX_FUSE', 'LTE_SFBC_LINK_MERGE', 'LTE_MIMO_LP_FUSE', 'LTE_CHM_TAY',
            'LTE_MIMO_RX_WAVE', 'LTE_SPATIAL_HP', 'LTE_DSP_STAGE', 'LTE_MIMO_FLAT_FUSE', 'LTE_TXM_FRAME')
TOL = {'f64': dict(npow=1e-12, sig=1e-13, H=1e-12, sym=1e-12, llr=1e-12),       # tests/test_gpu_profiles.py
       'f32': dict(npow=2e-6, sig=1e-5, H=1e-4, sym=1e-4, llr=1e-4)}
MIMO_CAP = ('bits_rx', 'data_syms', 'H', 'signal_rx', 'noise_power')


def _p(s):
    return dict(kv.split('=', 1) for kv in s.split())


def _mimo(tx, lp, ch, merge, rx, hp=0, det=0, dematch='none'):
    return _p(f'tx={tx} lp_fuse={lp} ch={ch} link_merge={merge} rx={rx} h_pilots={hp} det_stage={det} '
              f'dematch={dematch}')


_TAY = 'k_channel_tay,J={},G={},econ={}'.format
_PAIR, _FRAME, _SFBC, _FLAT = 'k_ofdm_tx_mimo', 'k_ofdm_tx_mimo_frame', 'k_ofdm_txch_sfbc', 'k_ofdm_txch_flat'
_RXS, _RXB, _RXW = 'k_rx_sfbc', 'k_rx_fft_mimo', 'k_rx_fft_mimo_w'


def _sf(tx, lp, ch, merge, rx, dematch='none', dematch2=None):
    """SFBC: run 1, and run 2 -- the captures drop the merged noise and the fused receiver."""
    return (_mimo(tx, lp, ch, merge, rx, dematch=dematch),
            _mimo(tx, lp, ch, 0, _RXB, dematch=dematch2 or dematch))


def _sp(tx, ch, rx):
    """Spatial: run 1 (pilot estimates handed over, staged detector), and run 2 --
    the H capture takes the interpolated H through HBM and the block receiver."""
    return _mimo(tx, 0, ch, 0, rx, 1, 1), _mimo(tx, 0, ch, 0, _RXB, 0, 0)


_SC_SISO = _p('tx=k_ofdm_tx_ch tx_stage=0 ch_fix=1 rx=k_rx_chest+k_rx_data xhand=0 dematch=none')
_SC_SIMO = _p('tx=k_ofdm_tx tx_stage=0 ch_fix=0 rx=k_rx_frame_simo xhand=0 dematch=none')
# case -> (the path of run 1, the path of run 2 with the captures); float32 where it differs: (case, 'f32')
PATHS = {
    'sc_siso_pa5': (_SC_SISO, _SC_SISO),
    'sc_simo_flat125': (_SC_SIMO, _SC_SIMO),
    'sfbc_pa20_u': _sf(_SFBC, 0, 'fused', 1, _RXS),
    'sfbc_pa20_c': _sf(_SFBC, 0, 'fused', 1, _RXS, 'zn', 'llr'),
    'sfbc_pb20_u': _sf(_PAIR, 1, _TAY(3, 2, 0), 0, _RXS),
    'sfbc_pb20_c': _sf(_FRAME, 1, _TAY(3, 2, 0), 0, _RXS, 'zn', 'llr'),
    'sfbc_vb20x_u': _sf(_PAIR, 1, _TAY(2, 2, 0), 0, _RXS),
    'sfbc_taps32_u': _sf(_SFBC, 0, 'fused', 1, _RXS),
    'sfbc_taps33_u': _sf(_PAIR, 1, _TAY(3, 2, 0), 0, _RXS),
    'sfbc_taps8_u': _sf(_SFBC, 0, 'fused', 1, _RXS),
    'sfbc_taps9_u': _sf(_PAIR, 0, _TAY(3, 2, 0), 0, _RXS),
    'sfbc_taps_cp_u': _sf(_PAIR, 1, _TAY(1, 2, 0), 0, _RXB),
    'sfbc_taps_cp1_u': _sf(_PAIR, 0, _TAY(1, 2, 0), 0, _RXB),
    'sfbc_vb5_u': _sf(_PAIR, 1, _TAY(3, 2, 0), 0, _RXB),
    'sfbc_vb5_c': _sf(_PAIR, 1, _TAY(3, 2, 0), 0, _RXB, 'llr'),
    'sfbc_pa125_rx1_u': _sf(_PAIR, 0, _TAY(1, 1, 0), 0, _RXB),
    'sfbc_pa15_c': _sf(_SFBC, 0, 'fused', 1, _RXS, 'zn', 'llr'),
    'sfbc_rx3_u': _sf(_PAIR, 1, _TAY(3, 3, 0), 0, _RXS),
    'sfbc_rx4_u': _sf(_PAIR, 1, _TAY(3, 4, 0), 0, _RXS),
    'sfbc_rx5_u': _sf(_PAIR, 1, _TAY(3, 1, 0), 0, _RXB),
    'sfbc_rx8_u': _sf(_PAIR, 1, _TAY(3, 4, 0), 0, _RXB),
    'sfbc_sym15_u': _sf(_SFBC, 0, 'fused', 1, _RXS),
    'sfbc_awgn5_u': _sf(_FLAT, 0, 'fused', 0, _RXB),
    'sm_pb20_v3': _sp(_PAIR, _TAY(3, 4, 1), _RXW),
    'sm_va20_v30': _sp(_PAIR, 'k_channel_mimo', _RXW),
    'sm_vb20x_v3': _sp(_PAIR, _TAY(2, 4, 0), _RXB),
    'sm_pb5_static': _sp(_PAIR, _TAY(3, 4, 0), _RXB),
    'sm_r2_pmi5_sic': _sp(_FLAT, 'fused', _RXB),
    'sm_r3_zf': _sp(_PAIR, _TAY(1, 3, 0), _RXB),
    'sm_22_pmi1_zf': _sp(_PAIR, _TAY(1, 2, 0), _RXB),
    'sm_42_r1_mrc': _sp(_FLAT, 'fused', _RXB),
    'sm_15': _sp(_FLAT, 'fused', _RXW),
    ('sm_15', 'f32'): _sp(_FLAT, 'fused', _RXB),        # the wave receiver is float64 only
}


def paths_of(name, prec):
    return PATHS.get((name, prec), PATHS[name])


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    _capi.device_init()
    return _capi


def set_env(monkeypatch, env):
    from lte_phy import engine
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    engine.clear_cache()


def config(cs):
    import lte_phy
    num = K.numerology(cs)
    cfg = lte_phy.LTEConfig(bandwidth=cs['bw'], modulation=cs['mod'], cp_type=cs.get('cp', 'normal'))
    assert (cfg.N, cfg.Nc, cfg.cp_length, cfg.fs) == (num.N, num.Nc, num.cp, num.fs)
    return cfg, num


def run(plan, cs, capture=()):
    return plan.run(np.array(cs['snrs'], dtype=np.float64), seed=cs['seed'], frame_ids=IDS, capture=capture)


def same_counts(r, frames, tag, coded=False):
    assert r['frame_errors'].tolist() == [fr['errs'] for fr in frames], (tag, r['frame_errors'].tolist())
    if coded:
        assert r['crc_ok'].astype(bool).tolist() == [fr['crc'] for fr in frames], tag


def ber_close(r, frames, tag):
    n = sum(fr['n_bits'] for fr in frames)
    d = abs(int(r['frame_errors'].astype(np.int64).sum()) - sum(fr['errs'] for fr in frames)) / n
    print(f'{tag}: |dBER| = {d:.3g}')
    assert d < 1e-3, (tag, d)


def check_path(got, want, tag):
    assert got == want, (tag, got, want)


def flips(monkeypatch, make_plan, cs, base_path, check, tag):
    """Run 1 once per switch whose flip changes the case's path."""
    from lte_phy import engine
    ran = []
    for sw in SWITCHES:
        set_env(monkeypatch, {sw: '0'})
        plan = make_plan()
        p = plan.path(np.array(cs['snrs'], dtype=np.float64), seed=cs['seed'], frame_ids=IDS)
        diff = engine.path_diff(p, base_path)
        if not diff:
            continue
        r = run(plan, cs)
        assert r.path == p
        check(r, tag + (sw,))
        ran.append((sw, sorted(diff)))
    set_env(monkeypatch, {})
    print(f'{tag}: flips run: {ran}')
    return ran


# ---------------------------------------------------------------------------
# beamforming
BF_PATH = _p('tx=none rx=k_bf')


def bf_case(C, name, prec):
    from lte_phy.beamforming import bf_plan
    cs = K.BF_CASES[name]
    cfg, num = config(cs)
    frames = K.bf_frames(name)
    plan = bf_plan(cfg, cs['n_sym'], frames[0]['n_bits'], cs['ntx'], cs['nrx'], cs['mode'] == 'adaptive', max_frames=B,
                   precision=prec)
    assert (plan.L, plan.Nd, plan.precision) == (cs['n_sym'] * num.Nd, num.Nd, prec)
    f64, tol = prec == 'f64', TOL[prec]
    r0 = run(plan, cs)
    check_path(r0.path, BF_PATH, name)
    r = run(plan, cs, ('bits_rx', 'data_syms', 'H', 'pmi', 'bf_gain'))
    check_path(r.path, BF_PATH, name)
    if f64:
        same_counts(r0, frames, name)
        same_counts(r, frames, name)
    else:
        ber_close(r0, frames, name)
    for b, fr in enumerate(frames):
        H = r['H'][b].astype(np.complex128)
        assert np.max(np.abs(H - fr['H'])) <= tol['H'] * np.max(np.abs(fr['H'])), (name, b)
        assert int(r['pmi'][b]) == fr['pmi'], (name, b)
        assert abs(float(r['bf_gain'][b]) - fr['gain']) < (1e-9 if f64 else 1e-4), (name, b)   # tests/test_gpu_bf.py
        sy = r['data_syms'][b].astype(np.complex128)
        assert np.linalg.norm(sy - fr['syms']) / np.linalg.norm(fr['syms']) < (1e-12 if f64 else 1e-5), (name, b)
        if f64:
            assert np.array_equal(r['bits_rx'][b], fr['bits_rx']), (name, b)
        else:
            assert np.mean(r['bits_rx'][b] != fr['bits_rx']) < 1e-3, (name, b)


@pytest.mark.parametrize('name', list(K.BF_CASES))
def test_beamforming(C, name):
    bf_case(C, name, 'f64')


def test_beamforming_f32(C):
    bf_case(C, 'bf_43a', 'f32')


# ---------------------------------------------------------------------------
# uncoded SC-FDM
def sc_case(C, name, prec):
    import lte_phy
    cs = K.SC_CASES[name]
    cfg, num = config(cs)
    frames = K.sc_frames(name)
    sim = lte_phy.OFDMSimulator(cfg, channel_type=cs['chan'], itu_profile=cs['prof'], enable_sc_fdm=True,
                                precision=prec)
    chain = C.CHAIN_UNCODED if cs['nrx'] == 1 else C.CHAIN_SIMO
    plan = sim._plan(chain, cs['n_sym'], frames[0]['n_bits'], num_rx=cs['nrx'], max_frames=B)
    assert plan.desc.sc_fdm == 1 and plan.L == cs['n_sym'] * (num.N + num.cp)
    f64, tol = prec == 'f64', TOL[prec]
    r0 = run(plan, cs)
    check_path(r0.path, paths_of(name, prec)[0], name)
    r = run(plan, cs, ('bits_rx', 'data_syms'))
    check_path(r.path, paths_of(name, prec)[1], name)
    if f64:
        same_counts(r0, frames, name)
        same_counts(r, frames, name)
    else:
        ber_close(r0, frames, name)
    Nd = num.Nd
    for b, fr in enumerate(frames):
        d = r['data_syms'][b].astype(np.complex128) - fr['syms']
        if cs['nrx'] == 1:
            err = np.linalg.norm(d.reshape(-1, Nd), axis=1)
        else:
            err = np.abs(d)
        ratio = float(np.max(err / (tol['sym'] * fr['scale'])))
        print(f'{name}[{prec}] frame {b}: data_syms |d| / bound = {ratio:.3g}')
        assert ratio <= 1.0, (name, b, ratio)
        if f64:
            assert np.array_equal(r['bits_rx'][b], fr['bits_rx']), (name, b)
        else:
            assert np.mean(r['bits_rx'][b] != fr['bits_rx']) < 1e-3, (name, b)


@pytest.mark.parametrize('name', list(K.SC_CASES))
def test_scfdm_uncoded(C, name):
    sc_case(C, name, 'f64')


def test_scfdm_uncoded_f32(C):
    sc_case(C, 'sc_siso_pa5', 'f32')


# ---------------------------------------------------------------------------
# SFBC
_SFBC_ORACLE = {}


def sfbc_oracle(name, merged):
    if (name, merged) not in _SFBC_ORACLE:
        _SFBC_ORACLE[name, merged] = K.sfbc_frames(name, merged)
    return _SFBC_ORACLE[name, merged]


def sfbc_plan(C, cs, prec):
    import lte_phy
    from lte_phy.engine import get_plan
    cfg, num = config(cs)
    n_sym, n_bits, L = K.sfbc_geometry(cs, num)
    dl, g = K.sfbc_taps(cs, num)
    if cs['paths'] is None:
        sim = lte_phy.OFDMSimulator(cfg, channel_type=cs['chan'], itu_profile=cs['prof'], precision=prec)
        plan = sim._sfbc_plan(0 if cs['coded'] else n_sym, n_bits, cs['nrx'], coded=cs['coded'], max_frames=B,
                              iters=K.ITERS)
    else:       # _sfbc_plan's keywords with the custom tap set
        plan = get_plan(N=cfg.N, Nc=cfg.Nc, cp_len=cfg.cp_length, bps=cfg.bits_per_symbol, n_sym=n_sym,
                        chain=C.CHAIN_SFBC, channel=C.CH_RAYLEIGH, num_rx=cs['nrx'], num_tx=2,
                        delays=tuple(int(v) for v in dl), gains=tuple(float(v) for v in g), fD=0.0, fs=cfg.fs,
                        n_bits=n_bits, turbo_iters=K.ITERS, max_frames=B, precision=prec, early_stop=False,
                        repack=None, turbo_scale=None)
    d = plan.desc
    assert [d.delays[i] for i in range(d.n_paths)] == [int(v) for v in dl]
    assert np.array_equal(np.array([d.gains[i] for i in range(d.n_paths)]), g)
    assert (plan.L, plan.n_sym, plan.res, plan.n_est) == (L, n_sym, num.Nd & ~1, (n_sym + 13) // 14)
    return plan, num


def sfbc_captures(name, cs, num, plan, r, frames, prec):
    tol, f64 = TOL[prec], prec == 'f64'
    res = plan.res
    worst = 0.0
    for b, fr in enumerate(frames):
        where = (name, prec, b)
        for a in range(cs['nrx']):
            y = r['signal_rx'][b, a].astype(np.complex128)
            assert np.linalg.norm(y - fr['rx'][a]) / np.linalg.norm(fr['rx'][a]) <= tol['sig'], where + (a,)
        npw = r['noise_power'][b].astype(np.float64)
        assert np.max(np.abs(npw / fr['npow'] - 1)) <= tol['npow'], where
        H = r['H'][b].astype(np.complex128)
        assert np.max(np.abs(H - fr['H'])) <= tol['H'] * np.max(np.abs(fr['H'])), where
        sy = r['data_syms'][b].astype(np.complex128)
        ratio = float(np.max(np.abs(sy - fr['syms']) / (tol['sym'] * K.sfbc_sym_scale(fr))))
        worst = max(worst, ratio)
        assert ratio <= 1.0, where + (ratio,)
        if cs['coded']:
            # as test_sfbc_coded_llrs_and_decoding: the oracle's max-log LLRs of the run's own symbols and estimates
            s2 = 1.0 / 10 ** (fr['snr'] / 10)
            nv = np.zeros(len(sy))
            for l in range(plan.n_sym):
                inv_g = np.zeros(res // 2)
                for a in range(cs['nrx']):
                    h0, h1 = H[a, l // 14, 0], H[a, l // 14, 1]
                    a0, a1 = (h0[0::2] + h0[1::2]) / 2, (h1[0::2] + h1[1::2]) / 2
                    nrm = (np.hypot(a0.real, a0.imag) ** 2 + np.hypot(a1.real, a1.imag) ** 2) + 1e-10
                    inv_g += 1.0 / np.clip(nrm, 1e-6, 1e6)
                nv[l * res:(l + 1) * res] = np.repeat(np.maximum(s2 / cs['nrx'] ** 2 * inv_g, s2 / 4.0), 2)
            ref = O.llrs(sy, nv, cs['mod'])
            got = r['llr'][b].astype(np.float64)[:len(ref)]
            assert np.max(np.abs(got - ref) / (1 + np.abs(ref))) < tol['llr'], where
            _, seg = O.segment(O.attach_crc24a(np.zeros(K.TB, dtype=np.int64)))
            coded = plan.coded_bits
            ncs = coded // num.bps
            rows = -(-ncs // res)
            q = np.arange(ncs)
            Lc = got.reshape(-1, num.bps)[(q % res) * rows + q // res].reshape(-1)[:coded]
            dec, ok = O.coded_rx_decode(Lc, seg, [3 * p[0] + 12 for p in seg], K.ITERS, f32_model=not f64)
            assert np.array_equal(np.asarray(dec)[:K.TB], r['bits_rx'][b]) and bool(ok) == bool(r['crc_ok'][b]), where
        if f64:
            assert np.array_equal(r['bits_rx'][b], fr['bits_rx']), where
        elif not cs['coded']:
            assert np.mean(r['bits_rx'][b] != fr['bits_rx']) < 1e-3, where
    print(f'{name}[{prec}]: worst data_syms |d| / bound = {worst:.3g}')


def sfbc_case(C, monkeypatch, name, prec='f64'):
    O.lib()
    cs = K.SFBC_CASES[name]
    f64 = prec == 'f64'
    set_env(monkeypatch, {})
    plan, num = sfbc_plan(C, cs, prec)
    want = paths_of(name, prec)

    def check(r, tag):
        frames = sfbc_oracle(name, r.path['link_merge'] == '1')
        if f64:
            same_counts(r, frames, tag, cs['coded'])
        elif not cs['coded']:
            ber_close(r, frames, tag)

    r0 = run(plan, cs)
    check_path(r0.path, want[0], name)
    assert (r0.path['link_merge'] == '1') == K.sfbc_predicates(cs)['merge'], (name, r0.path)
    check(r0, (name, prec, 'run 1'))
    cap = MIMO_CAP + (('llr',) if cs['coded'] else ())
    r = run(plan, cs, cap)
    check_path(r.path, want[1], name)
    check(r, (name, prec, 'run 2'))
    sfbc_captures(name, cs, num, plan, r, sfbc_oracle(name, False), prec)
    if f64 and cs['chan'] == 'rayleigh_mp':
        flips(monkeypatch, lambda: sfbc_plan(C, cs, prec)[0], cs, r0.path, check, (name, prec))


@pytest.mark.parametrize('name', list(K.SFBC_CASES))
def test_sfbc(C, monkeypatch, name):
    sfbc_case(C, monkeypatch, name)


def test_sfbc_f32(C, monkeypatch):
    sfbc_case(C, monkeypatch, 'sfbc_pa20_u', 'f32')


# ---------------------------------------------------------------------------
# uncoded spatial multiplexing
def sm_plan(C, cs, prec, n_bits):
    from lte_phy import ofdm_core
    from lte_phy.tm4 import DETECTORS, LTECodebook
    cfg, num = config(cs)
    W = LTECodebook(cs['ntx'], transmission_mode='TM4', rank=cs['rank']).get_precoder(cs['pmi'])
    assert np.array_equal(np.asarray(W), T.codebook(cs['ntx'], 'TM4', cs['rank'])[cs['pmi']])
    plan, gains, fD = ofdm_core._spatial_plan(cfg, cs['chan'], cs['prof'], cs['vel'], 2.0, cs['n_sym'], n_bits, B,
                                              num_tx=cs['ntx'], num_rx=cs['nrx'], rank=cs['rank'],
                                              detector=DETECTORS[cs['det']], W=W, precision=prec)
    if cs['chan'] == 'rayleigh_mp':
        dl, g = O.itu_paths(num, cs['prof'], spatial=True)
        d = plan.desc
        assert [d.delays[i] for i in range(d.n_paths)] == [int(v) for v in dl]
        assert np.array_equal(np.array([d.gains[i] for i in range(d.n_paths)]), g)
        assert abs(fD - O.doppler_hz(2.0, cs['vel'])) <= 1e-12 * max(1.0, fD)
    assert (plan.L, plan.Nd, plan.n_dsc) == (cs['n_sym'] * (num.N + num.cp), num.Nd, -(-num.Nd // cs['rank']))
    return plan, num


_SM_ORACLE = {}


def sm_case(C, monkeypatch, name, prec='f64'):
    cs = K.SM_CASES[name]
    f64, tol = prec == 'f64', TOL[prec]
    if name not in _SM_ORACLE:
        _SM_ORACLE[name] = K.sm_frames(name)
    frames = _SM_ORACLE[name]
    set_env(monkeypatch, {})
    plan, num = sm_plan(C, cs, prec, frames[0]['n_bits'])
    want = paths_of(name, prec)

    def check(r, tag):
        if f64:
            same_counts(r, frames, tag)
        else:
            ber_close(r, frames, tag)

    r0 = run(plan, cs)
    check_path(r0.path, want[0], name)
    check(r0, (name, prec, 'run 1'))
    r = run(plan, cs, MIMO_CAP)
    check_path(r.path, want[1], name)
    check(r, (name, prec, 'run 2'))
    worst = 0.0
    for b, fr in enumerate(frames):
        where = (name, prec, b)
        for a in range(cs['nrx']):
            y = r['signal_rx'][b, a].astype(np.complex128)
            assert np.linalg.norm(y - fr['rx'][a]) / np.linalg.norm(fr['rx'][a]) <= tol['sig'], where + (a,)
        npw = r['noise_power'][b].astype(np.float64)
        assert np.max(np.abs(npw / fr['npow'] - 1)) <= tol['npow'], where
        H = r['H'][b].astype(np.complex128)
        Ho = fr['H'].transpose(1, 0, 2, 3)                       # [rx][sym][tx][n_dsc]
        assert np.max(np.abs(H - Ho)) <= tol['H'] * np.max(np.abs(Ho)), where
        sy = r['data_syms'][b].astype(np.complex128)
        ratio = float(np.max(np.abs(sy - fr['syms']) / (tol['sym'] * fr['kappa'] / fr['mu'] * fr['s_norm'])))
        worst = max(worst, ratio)
        assert ratio <= 1.0, where + (ratio,)
        if f64:
            assert np.array_equal(r['bits_rx'][b], fr['bits_rx']), where
        else:
            assert np.mean(r['bits_rx'][b] != fr['bits_rx']) < 1e-3, where
    print(f'{name}[{prec}]: worst data_syms |d| / bound = {worst:.3g}')
    if f64:
        flips(monkeypatch, lambda: sm_plan(C, cs, prec, frames[0]['n_bits'])[0], cs, r0.path, check, (name, prec))


@pytest.mark.parametrize('name', list(K.SM_CASES))
def test_spatial(C, monkeypatch, name):
    sm_case(C, monkeypatch, name)


def test_spatial_f32(C, monkeypatch):
    sm_case(C, monkeypatch, 'sm_15', 'f32')
