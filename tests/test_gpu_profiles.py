"""GPU: every ITU profile, CP type, subcarrier spacing and tap-delay edge the
public API produces, on the kernels that `run_grid` and `bench.py` use by
default, against the float64 oracle (never against another GPU run).

Each case builds the plan the drop-in builds (`OFDMSimulator._plan`, or
`get_plan` with a custom tap set), injects bits, Jakes phases and unit normals
from a seeded RandomState in `OFDMChannel.draw`'s layout, and runs `Plan.run`
several times:
  (a) only the captures the fused TX + channel and the wave kernels accept
      (noise_power, tx_syms, data_syms, bits_rx; llr for the coded chain --
      and once more without llr, which is the demap-in-dematch path);
  (b) with H (drops the wave receivers) and signal_rx (drops the fused TX);
  (c) once per environment switch, flipped.
The oracle runs `simulate_siso` / `simulate_simo` / `simulate_siso_coded` with
`draws=` built from the same numbers, once per case (module cache).

Tolerances are the suite's own for the same quantities:
  tx_syms exact; noise_power 1e-12 (f64, test_wave_simo_tx_matches_block_tx) /
  2e-6 (f32, test_fused_tx_channel_matches_separate_kernels); signal_rx
  relative L2 1e-13 / 1e-5 (test_simulate_siso_signals_vs_oracle); H
  1e-12 / 1e-4 of max|H| (fused-vs-separate); data_syms per RE
  tol * max|Y| / |H| (ZF) or tol * sqrt(sum_r max|Y_r|^2) / sqrt(sum_r |H_r|^2)
  (MRC) with the same tol; LLRs 1e-12 / 1e-4 as test_coded_chain_llrs_vs_oracle
  forms them; f64 bits, error counts and CRC verdicts identical (after
  asserting from the oracle alone that no equalised symbol lies within 1e-9 of
  the constellation spacing of a decision boundary); f32 |dBER| < 1e-3.
B = 5 frames (odd: the wave TX's two-wave block is left half full), SNRs
spread over 0..30 dB, 14 OFDM symbols unless stated, TB 2000 when coded.

The multi-antenna chains (SFBC, spatial multiplexing, beamforming), whose fused
kernels draw from Philox only, are compared with the oracle on its Philox
restatement in tests/test_gpu_mimo_philox.py.
"""
import os

import numpy as np
import pytest

from conftest import ROOT, unpack

pytestmark = pytest.mark.gpu

B = 5
SNRS = np.array([0.0, 7.5, 15.0, 22.5, 30.0])
SWITCHES = ('LTE_TXCH_FUSE', 'LTE_RX_FUSE', 'LTE_SIMO_TX_WAVE', 'LTE_SIMO_RX_WAVE', 'LTE_TX_FRAME', 'LTE_RX_WAVE',
            'LTE_TX_WAVE', 'LTE_RXS_PAIRS', 'LTE_SIMO_XHAND', 'LTE_DEMAP_IN_DEMATCH', 'LTE_TXW_STAGE', 'LTE_TX_STAGE')
TOL = {'f64': dict(npow=1e-12, sig=1e-13, H=1e-12, sym=1e-12, llr=1e-12),
       'f32': dict(npow=2e-6, sig=1e-5, H=1e-4, sym=1e-4, llr=1e-4)}
BOUNDARY_MARGIN = 1e-9     # of the constellation spacing


@pytest.fixture(scope='module')
def C():
    from lte_phy import _capi
    _capi.device_init()
    return _capi


# ---------------------------------------------------------------------------
# cases: numerology, profile or custom taps, chain.  seed: the RandomState of
# the injected bits / phases / normals (chosen on the CPU so that the decision-
# boundary precondition holds, and, coded, that decoded and failed frames occur:
# on Vehicular_B at 20 MHz the reference's linear interpolation between pilots
# leaves an error floor, and of seeds 1..40 only 17 and 30 give a frame that decodes)
def _case(bw, mod, prof='Pedestrian_A', chain='uncoded', nrx=1, n_sym=14, df=15.0, cp='normal', vel=0.0,
          paths=None, seed=1, snrs=SNRS):
    return dict(bw=bw, mod=mod, prof=prof, chain=chain, nrx=nrx, n_sym=n_sym, df=df, cp=cp, vel=vel, paths=paths,
                seed=seed, snrs=np.asarray(snrs, dtype=np.float64))


_G9 = (1.0, 0.95, 0.9, 0.85, 0.8, 0.75, 0.7, 0.65, 0.6)
CASES = {
    # 2.1 SISO, N = 2048
    'siso_pb20': _case(20.0, '64-QAM', 'Pedestrian_B'),
    'siso_pb20_cod': _case(20.0, '64-QAM', 'Pedestrian_B', 'coded'),
    'siso_vb20': _case(20.0, '64-QAM', 'Vehicular_B'),
    'siso_vb20_cod': _case(20.0, '64-QAM', 'Vehicular_B', 'coded', seed=17),
    'siso_bu20x': _case(20.0, '64-QAM', 'Bad_Urban', cp='extended'),
    'siso_bu20x_cod': _case(20.0, '64-QAM', 'Bad_Urban', 'coded', cp='extended'),
    'siso_pa15': _case(15.0, '64-QAM', 'Pedestrian_A'),
    'siso_pa15_cod': _case(15.0, '64-QAM', 'Pedestrian_A', 'coded'),
    'siso_vb20_v3': _case(20.0, '64-QAM', 'Vehicular_B', vel=3.0),
    'siso_vb20_v3_cod': _case(20.0, '64-QAM', 'Vehicular_B', 'coded', vel=3.0, seed=17),
    'siso_vb20_v120': _case(20.0, '64-QAM', 'Vehicular_B', vel=120.0),
    'siso_vb20_v120_cod': _case(20.0, '64-QAM', 'Vehicular_B', 'coded', vel=120.0, seed=17),
    # 2.2 SIMO, N = 1024
    'simo_pb10': _case(10.0, '16-QAM', 'Pedestrian_B', 'simo', 4),
    'simo_bu10': _case(10.0, '16-QAM', 'Bad_Urban', 'simo', 4),
    'simo_vb10': _case(10.0, '16-QAM', 'Vehicular_B', 'simo', 4),
    'simo_pb10x': _case(10.0, '16-QAM', 'Pedestrian_B', 'simo', 4, cp='extended'),
    'simo_pb10hx': _case(10.0, '16-QAM', 'Pedestrian_B', 'simo', 4, df=7.5, cp='extended'),
    'simo_pb10_rx5': _case(10.0, '16-QAM', 'Pedestrian_B', 'simo', 5),
    'simo_pb10_rx3_15': _case(10.0, '16-QAM', 'Pedestrian_B', 'simo', 3, n_sym=15),
    # 2.3 custom tap sets (10 MHz, normal CP = 72, 2 RX; 20 MHz extended CP = 509, SISO)
    'taps_0_1_63_64': _case(10.0, '16-QAM', None, 'simo', 2, paths=((0, 1, 63, 64), (1.0, 0.9, 0.8, 0.7))),
    'taps_0_65': _case(10.0, '16-QAM', None, 'simo', 2, paths=((0, 65), (1.0, 0.8))),
    'taps_0_30_72': _case(10.0, '16-QAM', None, 'simo', 2, paths=((0, 30, 72), (1.0, 0.8, 0.6))),
    'taps_0_73': _case(10.0, '16-QAM', None, 'simo', 2, paths=((0, 73), (1.0, 0.8))),
    'taps_nine': _case(10.0, '16-QAM', None, 'simo', 2, paths=((0, 2, 5, 9, 14, 20, 27, 35, 40), _G9)),
    'taps_single': _case(10.0, '16-QAM', None, 'simo', 2, paths=((0,), (1.0,))),
    'taps_0_256': _case(20.0, '64-QAM', None, cp='extended', paths=((0, 256), (1.0, 0.8))),
    'taps_0_257': _case(20.0, '64-QAM', None, cp='extended', paths=((0, 257), (1.0, 0.8))),
    # 2.4 N < 512 and the smallest fused N
    'siso_vb125': _case(1.25, 'QPSK', 'Vehicular_B'),
    'siso_pa125h': _case(1.25, 'QPSK', 'Pedestrian_A', df=7.5),
    'siso_vb125h': _case(1.25, 'QPSK', 'Vehicular_B', df=7.5),
    'siso_vb5': _case(5.0, '16-QAM', 'Vehicular_B'),
}

A_CAP = ('noise_power', 'tx_syms', 'data_syms', 'bits_rx')
WAVE = {'LTE_RX_WAVE': '1', 'LTE_TX_WAVE': '1'}      # the opt-in 2048-point wave kernels (coded chain only)
V_SISO = [('a', {}, A_CAP), ('b', {}, A_CAP + ('H', 'signal_rx')),
          ('txch_fuse0', {'LTE_TXCH_FUSE': '0'}, A_CAP), ('rx_fuse0', {'LTE_RX_FUSE': '0'}, A_CAP)]
V_CODED = [('a', {}, A_CAP + ('llr',)), ('a_nollr', {}, A_CAP), ('b', {}, A_CAP + ('llr', 'H', 'signal_rx')),
           ('tx_frame0', {'LTE_TX_FRAME': '0'}, A_CAP + ('llr',)),
           ('txch_fuse0', {'LTE_TXCH_FUSE': '0'}, A_CAP + ('llr',)),
           ('rx_fuse0', {'LTE_RX_FUSE': '0'}, A_CAP + ('llr',)),
           ('wave1_llr', WAVE, A_CAP + ('llr',)), ('wave1_nollr', WAVE, A_CAP)]
V_SIMO = [('a', {}, A_CAP), ('b_H', {}, A_CAP + ('H',)), ('b_H_sig', {}, A_CAP + ('H', 'signal_rx')),
          ('tx_wave0', {'LTE_SIMO_TX_WAVE': '0'}, A_CAP), ('rx_wave0', {'LTE_SIMO_RX_WAVE': '0'}, A_CAP),
          ('txch_fuse0', {'LTE_TXCH_FUSE': '0'}, A_CAP), ('rx_fuse0', {'LTE_RX_FUSE': '0'}, A_CAP)]


# ---------------------------------------------------------------------------
# The kernel path each test's docstring claims, per variant: (transmitter,
# k_chan_fix runs, receiver) as lte_run_path names them (`Plan.run(...).path`),
# asserted for every run of check_case.  'k_ofdm_tx' is the separate TX (then
# k_channel), 'k_ofdm_tx_ch' the per-symbol k_ofdm_tx<.., CH>.
_TX, _TXC, _TXF, _TXFW, _TXSW = 'k_ofdm_tx', 'k_ofdm_tx_ch', 'k_ofdm_txf', 'k_ofdm_txf_w', 'k_ofdm_tx_simo_w'
_RXF, _RXFW, _RXSEP = 'k_rx_frame', 'k_rx_frame_w', 'k_rx_chest+k_rx_data'
_RXS, _RXS2, _RXSW = 'k_rx_frame_simo', 'k_rx_frame_simo2', 'k_rx_frame_simo_w'


def _siso(fused=True):
    """Uncoded SISO: fused -> k_ofdm_tx<.., CH> + k_chan_fix unless a stream capture
    / LTE_TXCH_FUSE=0 asks for k_ofdm_tx + k_channel; k_rx_frame unless LTE_RX_FUSE=0;
    the 2048-point wave kernels are coded-only."""
    on, off = ((_TXC, 1) if fused else (_TX, 0)), (_TX, 0)
    return {'a': on + (_RXF,), 'b': off + (_RXF,), 'txch_fuse0': off + (_RXF,), 'rx_fuse0': on + (_RXSEP,),
            'wave1': on + (_RXF,)}


def _coded(fused=True, wave_tx=False, wave_rx=True):
    """Coded SISO: k_ofdm_txf (LTE_TX_FRAME=0: k_ofdm_tx<.., CH>); wave_tx /
    wave_rx: txf_w_supported / rx_frame_w_supported hold (the wave receiver also
    needs the zn hand-off, that is no llr capture)."""
    on, sym, off = ((_TXF, 1), (_TXC, 1), (_TX, 0)) if fused else ((_TX, 0),) * 3
    w = (_TXFW, 1) if fused and wave_tx else on
    return {'a': on + (_RXF,), 'a_nollr': on + (_RXF,), 'b': off + (_RXF,), 'tx_frame0': sym + (_RXF,),
            'txch_fuse0': off + (_RXF,), 'rx_fuse0': on + (_RXSEP,), 'wave1_llr': w + (_RXF,),
            'wave1_nollr': w + (_RXFW if wave_rx else _RXF,)}


def _simo(tx=_TXSW, rx=_RXSW, rx_H=_RXS, rx_block=_RXS2):
    """SIMO: tx the default transmitter (_TXSW: head power in-kernel, no
    k_chan_fix; _TXC + k_chan_fix where tx_simo_w_supported refuses; _TX where
    txch_supported does); rx the default receiver, rx_H with an H capture,
    rx_block with LTE_SIMO_RX_WAVE=0."""
    fix = {_TXSW: 0, _TXC: 1, _TX: 0}
    on, blk, off = (tx, fix[tx]), ((_TXC, 1) if tx == _TXSW else (tx, fix[tx])), (_TX, 0)
    return {'a': on + (rx,), 'b_H': on + (rx_H,), 'b_H_sig': off + (rx_H,), 'tx_wave0': blk + (rx,),
            'rx_wave0': on + (rx_block,), 'txch_fuse0': off + (rx,), 'rx_fuse0': on + (_RXSEP,)}


PATHS = {
    'siso_pb20': _siso(), 'siso_vb20': _siso(), 'siso_bu20x': _siso(), 'siso_pa15': _siso(), 'siso_vb20_v3': _siso(),
    'siso_vb20_v120': _siso(fused=False),                      # fD fails mimo_taylor_ok
    'siso_pb20_cod': _coded(), 'siso_vb20_cod': _coded(), 'siso_vb20_v3_cod': _coded(),
    'siso_bu20x_cod': _coded(wave_rx=False),                   # odd CP
    'siso_pa15_cod': _coded(wave_tx=True),                     # 4 taps, max 13 <= 64
    'siso_vb20_v120_cod': _coded(fused=False),
    'simo_pb10': _simo(), 'simo_bu10': _simo(), 'simo_pb10x': _simo(),
    'simo_vb10': _simo(tx=_TXC),                               # max delay 70 > 64
    'simo_pb10hx': _simo(rx=_RXS2),                            # odd CP: no wave receiver
    'simo_pb10_rx5': _simo(tx=_TXC, rx=_RXSEP, rx_H=_RXSEP, rx_block=_RXSEP),   # 5 RX > 4
    'simo_pb10_rx3_15': _simo(rx_block=_RXS),                  # odd RX count: no pairs
    'taps_0_1_63_64': _simo(), 'taps_single': _simo(),
    'taps_0_65': _simo(tx=_TXC), 'taps_0_30_72': _simo(tx=_TXC),
    'taps_0_73': _simo(tx=_TX), 'taps_nine': _simo(tx=_TX),   # txch_supported refuses
    'taps_0_256': _siso(), 'taps_0_257': _siso(),
    'siso_vb125': _siso(fused=False), 'siso_pa125h': _siso(fused=False), 'siso_vb125h': _siso(fused=False),   # N < 512
    'siso_vb5': _siso(),
}
# float32: no wave kernel
PATHS_F32 = {'siso_vb20': _siso(), 'siso_vb5': _siso(), 'siso_vb20_cod': _coded(wave_rx=False),
             'simo_bu10': _simo(tx=_TXC, rx=_RXS2), 'simo_vb10': _simo(tx=_TXC, rx=_RXS2)}
assert set(PATHS) == set(CASES)


# ---------------------------------------------------------------------------
# the oracle side (no GPU needed): computed once per case
_ORACLE = {}
_QS = {'QPSK': np.sqrt(2.0), '16-QAM': np.sqrt(10.0), '64-QAM': np.sqrt(42.0)}
_NL = {'QPSK': 2, '16-QAM': 4, '64-QAM': 8}


def boundary_distance(syms, mod):
    """Smallest distance of any symbol's real or imaginary part to a decision
    boundary of the square constellation, in units of its spacing."""
    nl, sc = _NL[mod], _QS[mod]
    bnd = (np.arange(1, nl) * 2 - nl) / sc
    sp = 2.0 / sc
    d = np.inf
    for v in (syms.real, syms.imag):
        d = min(d, float(np.min(np.abs(v[:, None] - bnd[None, :]))))
    return d / sp


def case_draws(cs, num, O):
    """bits [B][n_bits], phases [B][rx][P][16], unit normals [B][rx][2][L] from
    the case's RandomState, in OFDMChannel.draw's layout."""
    coded = cs['chain'] == 'coded'
    if cs['paths'] is None:
        dl, g = O.itu_paths(num, cs['prof'])
    else:
        dl, g = np.array(cs['paths'][0]), np.array(cs['paths'][1], dtype=np.float64)
    rs = np.random.RandomState(cs['seed'])
    if coded:
        n_bits = 2000
        n_sym = O.coded_tx(num, np.zeros(n_bits, dtype=np.int64))['n_ofdm']
    else:
        n_sym = cs['n_sym']
        n_bits = n_sym * num.Nd * num.bps - 5
    L = n_sym * (num.N + num.cp)
    bits = rs.randint(0, 2, (B, n_bits)).astype(np.uint8)
    ph = 2 * np.pi * rs.rand(B, cs['nrx'], len(dl), 16)
    z = rs.standard_normal((B, cs['nrx'], 2, L))
    return dict(dl=dl, g=g, n_bits=n_bits, n_sym=n_sym, L=L, bits=bits, ph=ph, z=z)


def oracle_case(O, name):
    if name in _ORACLE:
        return _ORACLE[name]
    cs = CASES[name]
    num = O.Numerology(bandwidth=cs['bw'], delta_f=cs['df'], modulation=cs['mod'], cp_type=cs['cp'])
    dr = case_draws(cs, num, O)
    fD = O.doppler_hz(2.0, cs['vel']) if cs['vel'] else 0.0
    nrx, coded, simo = cs['nrx'], cs['chain'] == 'coded', cs['chain'] == 'simo'
    n_sym, Nd = dr['n_sym'], num.Nd
    frames = []
    for b in range(B):
        snr = float(cs['snrs'][b])
        bits = dr['bits'][b].astype(np.int64)
        d = [{'phases': [dr['ph'][b, r, p] for p in range(len(dr['dl']))], 'z_re': dr['z'][b, r, 0],
              'z_im': dr['z'][b, r, 1]} for r in range(nrx)]
        if simo:
            o = O.simulate_simo(num, bits, snr, num_rx=nrx, channel='rayleigh_mp', profile=cs['prof'], fD=fD,
                                draws=d, paths=cs['paths'])
            rxs = o['signal_rx_list']
        elif coded:
            assert cs['paths'] is None
            o = O.simulate_siso_coded(num, bits, snr, 'rayleigh_mp', profile=cs['prof'], fD=fD, draws=d)
            rxs = [o['signal_rx']]
        else:
            o = O.simulate_siso(num, bits, snr, 'rayleigh_mp', profile=cs['prof'], fD=fD, draws=d,
                                paths=cs['paths'])
            rxs = [o['signal_rx']]
        assert len(o['signal_tx']) == dr['L']
        # noise power (Q5): mean |y|^2 of the faded, noiseless stream / SNR, per RX
        npow = np.array([np.mean(np.abs(O.multipath(o['signal_tx'], dr['dl'], dr['g'], d[r]['phases'], fD,
                                                    num.fs)) ** 2) / 10 ** (snr / 10) for r in range(nrx)])
        Yf = [O.demod_stream(num, rxs[r]) for r in range(nrx)]
        Hg = np.stack([np.stack([O.estimate_channel(num, Yf[r][s0])[0] for s0 in range(0, n_sym, 14)])
                       for r in range(nrx)])                                   # [rx][grp][N]
        Hs = [Hg[r][np.arange(n_sym) // 14] for r in range(nrx)]               # [rx][sym][N]
        if simo:
            eq = o['symbols_rx_combined']
            den = sum(np.abs(Hs[r][:, num.data_idx]) ** 2 for r in range(nrx)).reshape(-1)
            ymax2 = sum(np.max(np.abs(Yf[r][:, num.data_idx])) ** 2 for r in range(nrx))
            scale = np.sqrt(ymax2) / np.sqrt(den)
        else:
            eq = (Yf[0] / (Hs[0] + 1e-6))[:, num.data_idx].reshape(-1)          # Q8, grid order
            if not coded:
                assert np.array_equal(eq, o['symbols_rx'])
            scale = np.max(np.abs(Yf[0][:, num.data_idx])) / np.abs(Hs[0][:, num.data_idx]).reshape(-1)
        fr = dict(o=o, npow=npow, rx=np.stack(rxs), H=Hg, eq=eq, scale=scale,
                  bits_rx=np.asarray(o['bits_received_array']).astype(np.uint8), errs=int(o['bit_errors']),
                  margin=boundary_distance(eq, cs['mod']))
        if coded:
            fr['crc'] = bool(o['crc_pass'])
            fr['Hd'] = Hs[0][:, num.data_idx].reshape(-1)
            # the transmitted REs in grid order: T/F interleaver (core/ofdm_core.py:1040-1060)
            qam = o['symbols_tx']
            q = np.arange(len(qam))
            rows = -(-len(qam) // Nd)
            fr['tx_pos'], fr['tx'] = (q % Nd) * rows + q // Nd, qam
        else:
            fr['tx_pos'], fr['tx'] = np.arange(n_sym * Nd), np.concatenate(o['symbols_tx'])
        frames.append(fr)
    _ORACLE[name] = dict(cs=cs, num=num, dr=dr, fD=fD, frames=frames)
    return _ORACLE[name]


# ---------------------------------------------------------------------------
# the GPU side
def _plan(C, oc, prec):
    import lte_phy
    from lte_phy.engine import get_plan
    cs, num, dr = oc['cs'], oc['num'], oc['dr']
    cfg = lte_phy.LTEConfig(bandwidth=cs['bw'], delta_f=cs['df'], modulation=cs['mod'], cp_type=cs['cp'])
    assert (cfg.N, cfg.Nc, cfg.cp_length, cfg.fs) == (num.N, num.Nc, num.cp, num.fs)
    chain = {'uncoded': C.CHAIN_UNCODED, 'coded': C.CHAIN_CODED, 'simo': C.CHAIN_SIMO}[cs['chain']]
    n_sym = 0 if cs['chain'] == 'coded' else dr['n_sym']
    if cs['paths'] is None:
        sim = lte_phy.OFDMSimulator(cfg, channel_type='rayleigh_mp', itu_profile=cs['prof'],
                                    frequency_ghz=2.0, velocity_kmh=cs['vel'], precision=prec)
        plan = sim._plan(chain, n_sym, dr['n_bits'], num_rx=cs['nrx'], max_frames=B)
        assert abs(sim.channels[0].fD - oc['fD']) <= 1e-12 * max(1.0, oc['fD'])
    else:
        plan = get_plan(N=cfg.N, Nc=cfg.Nc, cp_len=cfg.cp_length, bps=cfg.bits_per_symbol, n_sym=n_sym, chain=chain,
                        channel=C.CH_RAYLEIGH, num_rx=cs['nrx'], delays=tuple(int(v) for v in dr['dl']),
                        gains=tuple(float(v) for v in dr['g']), fD=0.0, fs=cfg.fs, n_bits=dr['n_bits'],
                        turbo_iters=8, max_frames=B, sc_fdm=0, no_equalization=0, precision=prec)
    d = plan.desc
    assert [d.delays[i] for i in range(d.n_paths)] == [int(v) for v in dr['dl']]
    assert np.array_equal(np.array([d.gains[i] for i in range(d.n_paths)]), dr['g'])
    assert (plan.L, plan.n_sym, plan.Nd) == (dr['L'], dr['n_sym'], num.Nd)
    return plan


def _compare(O, oc, r, cap, prec, tag):
    cs, num = oc['cs'], oc['num']
    tol, f64, coded = TOL[prec], prec == 'f64', cs['chain'] == 'coded'
    nrx, n_bits = cs['nrx'], oc['dr']['n_bits']
    worst, worst_np = 0.0, 0.0
    for b, fr in enumerate(oc['frames']):
        where = (tag, b)
        ts = r['tx_syms'][b].astype(np.complex128)
        if f64:
            assert np.array_equal(ts[fr['tx_pos']], fr['tx']), where
        else:
            assert np.max(np.abs(ts[fr['tx_pos']] - fr['tx'])) < 1e-6, where
        npw = r['noise_power'][b].astype(np.float64)
        e_np = float(np.max(np.abs(npw / fr['npow'] - 1)))
        worst_np = max(worst_np, e_np)
        assert e_np <= tol['npow'], where + (e_np,)
        if 'signal_rx' in cap:
            for a in range(nrx):
                y = r['signal_rx'][b, a].astype(np.complex128)
                assert np.linalg.norm(y - fr['rx'][a]) / np.linalg.norm(fr['rx'][a]) <= tol['sig'], where + (a,)
        if 'H' in cap:
            Hgpu = r['H'][b].astype(np.complex128)
            assert np.max(np.abs(Hgpu - fr['H'])) <= tol['H'] * np.max(np.abs(fr['H'])), where
        sy = r['data_syms'][b].astype(np.complex128)
        ratio = float(np.max(np.abs(sy - fr['eq']) / (tol['sym'] * fr['scale'])))
        worst = max(worst, ratio)
        assert ratio <= 1.0, where + (ratio,)
        if 'llr' in cap:
            # as test_coded_chain_llrs_vs_oracle forms it: the oracle's max-log LLRs of the
            # kernel's own equalised symbols, sigma^2_eff from its estimate when captured
            Hd = fr['Hd']
            if 'H' in cap:
                Hs = r['H'][b, 0].astype(np.complex128)
                Hd = np.concatenate([Hs[l // 14][num.data_idx] for l in range(oc['dr']['n_sym'])])
            ref = O.llrs(sy, O.noise_var_per_symbol(Hd, float(cs['snrs'][b]), 'rayleigh_mp'), cs['mod'])
            got = r['llr'][b].astype(np.float64)[:len(ref)]
            assert np.max(np.abs(got - ref) / (1 + np.abs(ref))) < tol['llr'], where
        brx = r['bits_rx'][b]
        if f64:
            assert np.array_equal(brx, fr['bits_rx']), where + (int(np.sum(brx != fr['bits_rx'])),)
            assert int(r['frame_errors'][b]) == fr['errs'], where
            if coded:
                assert bool(r['crc_ok'][b]) == fr['crc'], where
        elif coded:
            # float32 past the turbo cliff changes which wrong bits come out (as
            # test_simulate_siso_coded_ref_compat_f32): the verdict, and clean frames, agree
            assert bool(r['crc_ok'][b]) == fr['crc'], where
            if fr['errs'] == 0:
                assert int(r['frame_errors'][b]) == 0, where
        else:
            assert abs(int(r['frame_errors'][b]) - fr['errs']) / n_bits < 1e-3, where
            assert np.mean(brx != fr['bits_rx']) < 1e-3, where
    return worst, worst_np


def check_case(C, O, monkeypatch, name, variants, prec='f64'):
    oc = oracle_case(O, name)
    cs = oc['cs']
    for fr in oc['frames']:      # the decisions are not at the mercy of round-off (oracle alone)
        assert fr['margin'] >= BOUNDARY_MARGIN, (name, fr['margin'])
    if cs['chain'] == 'coded':
        crcs = [fr['crc'] for fr in oc['frames']]
        assert any(crcs) and not all(crcs), (name, crcs)
    plan = _plan(C, oc, prec)
    dr = oc['dr']
    for label, env, cap in variants:
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        r = plan.run(cs['snrs'], bits=dr['bits'], phases=dr['ph'], noise=dr['z'], capture=cap)
        got, want = r.path, (PATHS if prec == 'f64' else PATHS_F32)[name][label]
        assert (got['tx'], int(got['ch_fix']), got['rx']) == want, (name, prec, label, got)
        assert got['dematch'] == ('none' if cs['chain'] != 'coded' else 'llr' if 'llr' in cap else 'zn'), (label, got)
        worst, worst_np = _compare(O, oc, r, cap, prec, f'{name}[{prec}]/{label}')
        print(f'profiles {name}[{prec}]/{label}: worst data_syms |d| / bound = {worst:.3g}, '
              f'noise_power rel err = {worst_np:.3g}')


# ---------------------------------------------------------------------------
# 2.1 SISO, N = 2048
def test_siso_pedestrian_b_20mhz(C, oracle, monkeypatch):
    """6 taps, max delay 114 <= cp 144, fD = 0: txch_fusable -> launch_ofdm_tx_ch
    -> k_ofdm_tx<double, 0, 6, false, CH = 1, 2048, NP = 6> + k_chan_fix, then
    k_rx_frame.  (b) / LTE_TXCH_FUSE=0: k_ofdm_tx + staged k_channel (114 <=
    CH_HALO); LTE_RX_FUSE=0: k_rx_chest + k_rx_data."""
    check_case(C, oracle, monkeypatch, 'siso_pb20', V_SISO)


def test_siso_pedestrian_b_20mhz_coded(C, oracle, monkeypatch):
    """TB 2000, 6 taps: tx_per_frame -> k_ofdm_txf<double, 6, 2048> (runtime tap
    count, n_paths != 4) + k_chan_fix; k_rx_frame writing LLRs, or (no llr
    capture) handing (z, nv) to k_dematch_zn.  LTE_TX_FRAME=0: k_ofdm_tx<double, 1,
    6, false, 1, 2048, NP = 6>.  LTE_RX_WAVE=1 LTE_TX_WAVE=1: txf_w_supported
    refuses 6 taps; without an llr capture k_rx_frame_w receives (cp 144 even)."""
    check_case(C, oracle, monkeypatch, 'siso_pb20_cod', V_CODED)


def test_siso_vehicular_b_20mhz(C, oracle, monkeypatch):
    """8 taps, max delay 139 <= cp 144: k_ofdm_tx<double, 0, 6, false, CH = 1, 2048,
    NP = 0> (the generic body, TXCH_MAXP = 8 slots all live) + k_chan_fix."""
    check_case(C, oracle, monkeypatch, 'siso_vb20', V_SISO)


def test_siso_vehicular_b_20mhz_coded(C, oracle, monkeypatch):
    """8 taps coded: k_ofdm_txf<double, 6, 2048> with NP = 0; LTE_TX_FRAME=0:
    k_ofdm_tx<double, 1, 6, false, 1, 2048, NP = 0>.  The wave TX is refused (8
    taps); LTE_RX_WAVE=1 without an llr capture: k_rx_frame_w."""
    check_case(C, oracle, monkeypatch, 'siso_vb20_cod', V_CODED)


def test_siso_bad_urban_extended_cp(C, oracle, monkeypatch):
    """cp 509 (odd), 8 taps, max delay 80: k_ofdm_tx<.., CH = 1, 2048, NP = 0> with
    S = 2557 samples per symbol (tx_channel's 10 samples per thread: S <= 1.25 N
    holds, 509 < 512) + k_chan_fix; k_rx_frame.  With LTE_RX_WAVE=1 LTE_TX_WAVE=1
    rx_frame_w_supported (uncoded chain) and txf_w_supported refuse."""
    check_case(C, oracle, monkeypatch, 'siso_bu20x', V_SISO + [('wave1', WAVE, A_CAP)])


def test_siso_bad_urban_extended_cp_coded(C, oracle, monkeypatch):
    """cp 509 coded: k_ofdm_txf<double, 6, 2048> NP = 0.  LTE_RX_WAVE=1 without an
    llr capture reaches rx_frame_w_supported, which refuses the odd CP (cp % 2),
    and txf_w_supported refuses 8 taps: the block kernels run."""
    check_case(C, oracle, monkeypatch, 'siso_bu20x_cod', V_CODED)


def test_siso_pedestrian_a_15mhz(C, oracle, monkeypatch):
    """Nc = 900 on N = 2048 (Nd = 749), 4 taps, max delay 13: k_ofdm_tx<double, 0,
    6, false, CH = 1, 2048, NP = 4> + k_chan_fix, k_rx_frame.  The 2048-point wave
    kernels are coded-only (rx_frame_w_supported, launch_ofdm_txf): with
    LTE_RX_WAVE=1 LTE_TX_WAVE=1 the same block kernels run."""
    check_case(C, oracle, monkeypatch, 'siso_pa15', V_SISO + [('wave1', WAVE, A_CAP)])


def test_siso_pedestrian_a_15mhz_coded(C, oracle, monkeypatch):
    """Nd = 749, 4 taps, coded: k_ofdm_txf<double, 6, 2048, false, NP = 4, SP = 2>
    (txf_peda_launch) by default.  LTE_TX_WAVE=1: txf_w_supported holds (N 2048, 4
    taps, max 13 <= 64) -> k_ofdm_txf_w; LTE_RX_WAVE=1 without an llr capture:
    rx_frame_w_supported holds (cp 144 even, Np = 150) -> k_rx_frame_w; with the
    llr capture SoftOut::z is null and k_rx_frame runs after the wave TX."""
    check_case(C, oracle, monkeypatch, 'siso_pa15_cod', V_CODED)


def test_siso_vehicular_b_3kmh(C, oracle, monkeypatch):
    """fD = 5.6 Hz passes mimo_taylor_ok: per-symbol Taylor sets (k_jakes_sets) on
    8 taps, k_ofdm_tx<double, 0, 6, false, CH = 2, 2048> + k_chan_fix's tcoef
    branch.  (b) / LTE_TXCH_FUSE=0: k_channel's Taylor sub-intervals."""
    check_case(C, oracle, monkeypatch, 'siso_vb20_v3', V_SISO)


def test_siso_vehicular_b_3kmh_coded(C, oracle, monkeypatch):
    """Coded, time-varying 8 taps: k_ofdm_txf<double, 6, 2048, TV = true>;
    LTE_TX_FRAME=0: k_ofdm_tx<double, 1, 6, false, CH = 2, 2048>."""
    check_case(C, oracle, monkeypatch, 'siso_vb20_v3_cod', V_CODED)


def test_siso_vehicular_b_120kmh(C, oracle, monkeypatch):
    """fD = 222 Hz fails mimo_taylor_ok: txch_fusable refuses, k_ofdm_tx +
    k_channel with SL = 64 Taylor sub-intervals on 8 = CH_MAXP taps (staged, 139 <=
    CH_HALO) in every run."""
    check_case(C, oracle, monkeypatch, 'siso_vb20_v120', V_SISO)


def test_siso_vehicular_b_120kmh_coded(C, oracle, monkeypatch):
    """As above, coded: k_ofdm_tx<double, 1, 6> + k_channel whatever LTE_TX_FRAME /
    LTE_TXCH_FUSE say."""
    check_case(C, oracle, monkeypatch, 'siso_vb20_v120_cod', V_CODED)


# 2.2 SIMO, N = 1024: the config-3 wave kernels
def test_simo_pedestrian_b(C, oracle, monkeypatch):
    """6 taps, max 57 <= 64, cp 72 even, 4 RX: k_ofdm_tx_simo_w<4, NP = 6> (head
    power in-kernel, no k_chan_fix) + k_rx_frame_simo_w.  H capture:
    k_rx_frame_simo; LTE_SIMO_TX_WAVE=0: k_ofdm_tx<double, 0, 4, false, 1, 1024,
    6> + k_chan_fix; LTE_SIMO_RX_WAVE=0: k_rx_frame_simo2; LTE_RX_FUSE=0:
    k_rx_chest + k_rx_data."""
    check_case(C, oracle, monkeypatch, 'simo_pb10', V_SIMO)


def test_simo_bad_urban(C, oracle, monkeypatch):
    """8 taps, max 40: k_ofdm_tx_simo_w<4, NP = 0> (runtime count, 8 slots) +
    k_rx_frame_simo_w."""
    check_case(C, oracle, monkeypatch, 'simo_bu10', V_SIMO)


def test_simo_vehicular_b(C, oracle, monkeypatch):
    """max delay 70 > 64: tx_simo_w_supported refuses (TXSW_HALF window), so
    k_ofdm_tx<double, 0, 4, false, 1, 1024, NP = 0> + k_chan_fix run, then
    k_rx_frame_simo_w."""
    check_case(C, oracle, monkeypatch, 'simo_vb10', V_SIMO)


def test_simo_pedestrian_b_extended_cp(C, oracle, monkeypatch):
    """cp 254: k_ofdm_tx_simo_w<4, 6> with its head window at xs[576 - 254 + k] and
    tail = N - cp + D; k_rx_frame_simo_w (cp even)."""
    check_case(C, oracle, monkeypatch, 'simo_pb10x', V_SIMO)


def test_simo_7p5khz_extended_cp(C, oracle, monkeypatch):
    """delta_f 7.5 kHz, cp 253 (odd), delays (0, 2, 6, 9, 18, 28): the wave TX is
    kept (k_ofdm_tx_simo_w<4, 6>), rx_simo_w_supported refuses (cp % 2), so
    k_rx_frame_simo2 (4 RX, no H) receives; with H k_rx_frame_simo."""
    check_case(C, oracle, monkeypatch, 'simo_pb10hx', V_SIMO)


def test_simo_five_rx(C, oracle, monkeypatch):
    """num_rx 5 > 4: tx_simo_w_supported, rx_simo_w_supported and
    rx_frame_simo_supported (RXS_MAXRX) all refuse: k_ofdm_tx<double, 0, 4, false,
    1, 1024, 6> + k_chan_fix, k_rx_chest + k_rx_data<SIMO>."""
    check_case(C, oracle, monkeypatch, 'simo_pb10_rx5', V_SIMO)


def test_simo_three_rx_15_symbols(C, oracle, monkeypatch):
    """3 RX, 15 symbols: k_ofdm_tx_simo_w's tailp carries symbol 13's tail into
    symbol 14, the one-symbol second estimation group of k_rx_frame_simo_w (odd RX
    count: LTE_SIMO_RX_WAVE=0 falls to k_rx_frame_simo, not simo2)."""
    check_case(C, oracle, monkeypatch, 'simo_pb10_rx3_15', V_SIMO)


# 2.3 custom tap sets
def test_taps_max_delay_64(C, oracle, monkeypatch):
    """Delays {0, 1, 63, 64}: max_delay == 64, the wave TX's limit; every lane of
    k_ofdm_tx_simo_w<4, NP = 4> takes the head-power branch and symbol 0 reads the
    zero previous tail.  2 RX: k_rx_frame_simo_w."""
    check_case(C, oracle, monkeypatch, 'taps_0_1_63_64', V_SIMO)


def test_taps_max_delay_65(C, oracle, monkeypatch):
    """{0, 65}: one past the wave TX's limit: k_ofdm_tx<double, 0, 4, false, 1,
    1024, NP = 0> (2 taps) + k_chan_fix."""
    check_case(C, oracle, monkeypatch, 'taps_0_65', V_SIMO)


def test_taps_max_delay_equals_cp(C, oracle, monkeypatch):
    """{0, 30, 72}: max_delay == cp == 72, txch_supported's edge: k_ofdm_tx<..,
    CH = 1, 1024, NP = 0> writes no CP sample's power itself (m starts at D = cp);
    k_chan_fix forms all 72 head samples."""
    check_case(C, oracle, monkeypatch, 'taps_0_30_72', V_SIMO)


def test_taps_past_cp(C, oracle, monkeypatch):
    """{0, 73}: max_delay > cp: txch_supported refuses; k_ofdm_tx + staged
    k_channel in every run (inter-symbol interference the receiver cannot undo:
    an error floor, identical to the oracle's)."""
    check_case(C, oracle, monkeypatch, 'taps_0_73', V_SIMO)


def test_taps_nine(C, oracle, monkeypatch):
    """Nine taps (<= LTE_MAX_PATHS 16, > TXCH_MAXP 8): txch_supported refuses;
    k_channel's generic tap loop (n_paths > CH_MAXP: no register taps)."""
    check_case(C, oracle, monkeypatch, 'taps_nine', V_SIMO)


def test_taps_single(C, oracle, monkeypatch):
    """One tap at delay 0: max_delay 0, k_ofdm_tx_simo_w<4, NP = 0> with no head
    samples, launch_chan_fix a no-op on the block path."""
    check_case(C, oracle, monkeypatch, 'taps_single', V_SIMO)


def test_taps_halo_256(C, oracle, monkeypatch):
    """20 MHz extended CP (509), {0, 256}: fused by default (k_ofdm_tx<.., CH = 1,
    2048, NP = 0>); LTE_TXCH_FUSE=0 / (b): k_channel staged, max_delay == CH_HALO."""
    check_case(C, oracle, monkeypatch, 'taps_0_256', V_SISO)


def test_taps_halo_257(C, oracle, monkeypatch):
    """{0, 257}: LTE_TXCH_FUSE=0 / (b): k_channel unstaged (taps from global
    memory, src < 0 skipped)."""
    check_case(C, oracle, monkeypatch, 'taps_0_257', V_SISO)


# 2.4 N < 512: the fused TX is refused (txch_supported: N >= 512)
def test_siso_vehicular_b_1p25mhz(C, oracle, monkeypatch):
    """N 128, cp 9, 8 taps on 7 distinct delays, max_delay == cp: k_ofdm_tx<double,
    0, 2> (16 symbols per 256-thread block) + staged k_channel with 8 = CH_MAXP
    register taps, k_rx_frame; LTE_RX_FUSE=0: k_rx_chest + k_rx_data."""
    check_case(C, oracle, monkeypatch, 'siso_vb125', V_SISO)


def test_siso_pedestrian_a_1p25mhz_7p5khz(C, oracle, monkeypatch):
    """delta_f 7.5 kHz: fs 0.96 MHz, cp 4, all four taps at delay 0 (max_delay 0):
    k_ofdm_tx + k_channel summing four coefficients on one sample."""
    check_case(C, oracle, monkeypatch, 'siso_pa125h', V_SISO)


def test_siso_vehicular_b_1p25mhz_7p5khz(C, oracle, monkeypatch):
    """Same numerology, 8 taps on delays (0, 0, 1, 1, 2, 2, 4, 4): max_delay == cp
    == 4."""
    check_case(C, oracle, monkeypatch, 'siso_vb125h', V_SISO)


def test_siso_vehicular_b_5mhz(C, oracle, monkeypatch):
    """N 512, the smallest fused N; 8 taps, max 35 against cp 36: k_ofdm_tx<double,
    0, 4, false, CH = 1, NC = 0, NP = 0> (4 symbols per block) + k_chan_fix."""
    check_case(C, oracle, monkeypatch, 'siso_vb5', V_SISO)


# 2.5 float32
@pytest.mark.parametrize('name,variants', [('siso_vb20', V_SISO), ('siso_vb20_cod', V_CODED), ('simo_bu10', V_SIMO),
                                           ('simo_vb10', V_SIMO), ('siso_vb5', V_SISO)],
                         ids=['siso_vb20', 'siso_vb20_cod', 'simo_bu10', 'simo_vb10', 'siso_vb5'])
def test_float32(C, oracle, monkeypatch, name, variants):
    """precision='f32' on the 8-tap cases.  The wave kernels and the compile-time
    tap counts are float64 only: k_ofdm_tx<float, .., CH = 1, NP = 0> + k_chan_fix
    (k_ofdm_txf<float, ..> coded), k_rx_frame / k_rx_frame_simo2 (f32 tolerances)."""
    check_case(C, oracle, monkeypatch, name, variants, prec='f32')


# 2.6 a refusal that stays loud
def test_3mhz_is_refused_loudly(C):
    """LTEConfig(bandwidth=3.0): Nc 200 on N 256 gives Nd = 166 >= N / 2, which
    k_rx_data's four REs per thread cannot hold; lte_plan_create refuses
    (LTE_EUNSUP -> NotImplementedError, a RuntimeError).  The reference runs it."""
    import lte_phy
    cfg = lte_phy.LTEConfig(bandwidth=3.0)
    assert (cfg.Nc, cfg.N) == (200, 256)
    sim = lte_phy.OFDMSimulator(cfg, channel_type='rayleigh_mp')
    with pytest.raises(RuntimeError, match='Nd >= N/2 not supported'):
        sim.simulate_siso(np.random.RandomState(0).randint(0, 2, 500), 10.0)


# ---------------------------------------------------------------------------
# 1. the drop-in calls on the round-7 reference goldens (tests/golden/make_golden_r7.py)
GOLDEN_R7 = os.path.join(ROOT, 'tests', 'golden', 'golden_r7.npz')


@pytest.fixture(scope='module')
def golden_r7():
    return np.load(GOLDEN_R7, allow_pickle=False)


def _state_head():
    return np.array(np.random.get_state()[1][:8], dtype=np.uint32)


def _dropin(ckw, prec, **skw):
    import lte_phy
    return lte_phy.OFDMSimulator(lte_phy.LTEConfig(**ckw), channel_type='rayleigh_mp', precision=prec, **skw)


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('name,ckw,skw,snr', [
    ('siso_vb20', dict(bandwidth=20.0, modulation='64-QAM'), dict(itu_profile='Vehicular_B'), 17.4),
    ('siso_bu20', dict(bandwidth=20.0, modulation='64-QAM'), dict(itu_profile='Bad_Urban'), 11.8),
    ('siso_pb15x', dict(bandwidth=15.0, modulation='16-QAM', cp_type='extended'), dict(itu_profile='Pedestrian_B'),
     14.2),
    ('siso_vb125', dict(bandwidth=1.25, modulation='QPSK'), dict(itu_profile='Vehicular_B'), 6.5),
    ('siso_pb25h', dict(bandwidth=2.5, delta_f=7.5, modulation='QPSK'), dict(itu_profile='Pedestrian_B'), 4.1),
    ('siso_vb20_v3', dict(bandwidth=20.0, modulation='64-QAM'),
     dict(itu_profile='Vehicular_B', frequency_ghz=2.0, velocity_kmh=3), 21.6)],
    ids=['siso_vb20', 'siso_bu20', 'siso_pb15x', 'siso_vb125', 'siso_pb25h', 'siso_vb20_v3'])
def test_simulate_siso_ref_compat_r7(C, golden_r7, name, ckw, skw, snr, prec):
    """Drop-in simulate_siso == the reference's own output at the new points
    (signal_tx / signal_rx are captured, so k_ofdm_tx + k_channel + k_rx_frame
    run).  f64: identical received bits; f32: within 1e-3."""
    g = golden_r7
    sim = _dropin(ckw, prec, **skw)
    nb = int(g[name + '_nbits'][0])
    bits = unpack(g[name + '_bits'], nb).astype(np.int64)
    k = f'{name}_snr{snr}'
    r = sim.simulate_siso(bits, snr)
    ref_err = int(g[k + '_errors'][0])
    diff = np.mean(r['bits_received_array'] != unpack(g[k + '_rx'], nb))
    if prec == 'f64':
        assert r['bit_errors'] == ref_err and diff == 0, (k, r['bit_errors'], ref_err, diff)
    else:
        assert abs(r['bit_errors'] - ref_err) / nb < 1e-3, (k, r['bit_errors'], ref_err)
        assert diff < 1e-3, (k, diff)
    assert abs(r['papr_db'] - g[k + '_papr'][0]) < (1e-9 if prec == 'f64' else 1e-3)
    assert np.array_equal(_state_head(), g[k + '_state']), 'global RNG side effects differ'


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('name,ckw,prof,snr,nrx', [
    ('simo4_pb10', dict(bandwidth=10.0, modulation='16-QAM'), 'Pedestrian_B', 9.3, 4),
    ('simo4_vb10', dict(bandwidth=10.0, modulation='16-QAM'), 'Vehicular_B', 9.3, 4),
    ('simo4_vb10x', dict(bandwidth=10.0, modulation='16-QAM', cp_type='extended'), 'Vehicular_B', 9.3, 4),
    ('simo4_pb10x', dict(bandwidth=10.0, modulation='16-QAM', cp_type='extended'), 'Pedestrian_B', 9.3, 4),
    ('simo2_q10hx', dict(bandwidth=10.0, delta_f=7.5, modulation='QPSK', cp_type='extended'), 'Pedestrian_A', 2.7,
     2)], ids=['simo4_pb10', 'simo4_vb10', 'simo4_vb10x', 'simo4_pb10x', 'simo2_q10hx'])
def test_simulate_simo_ref_compat_r7(C, golden_r7, name, ckw, prof, snr, nrx, prec):
    """Drop-in simulate_simo == the reference (k_ofdm_tx + k_channel +
    k_rx_frame_simo: the call captures the streams and H)."""
    g = golden_r7
    sim = _dropin(ckw, prec, itu_profile=prof)
    nb = int(g[name + '_nbits'][0])
    bits = unpack(g[name + '_bits'], nb).astype(np.int64)
    k = f'{name}_snr{snr}'
    r = sim.simulate_simo(bits, snr, num_rx=nrx, parallel=False)
    ref_err = int(g[k + '_errors'][0])
    diff = np.mean(r['bits_received_array'] != unpack(g[k + '_rx'], nb))
    if prec == 'f64':
        assert r['bit_errors'] == ref_err and diff == 0, (k, r['bit_errors'], ref_err, diff)
    else:
        assert abs(r['bit_errors'] - ref_err) / nb < 1e-3, (k, r['bit_errors'], ref_err)
        assert diff < 1e-3, (k, diff)
    assert np.array_equal(_state_head(), g[k + '_state'])


CODED_R7 = [('cod_vb20', dict(bandwidth=20.0, modulation='64-QAM'), 'Vehicular_B', [9.7, 22.3]),
            ('cod_bu5x', dict(bandwidth=5.0, modulation='16-QAM', cp_type='extended'), 'Bad_Urban', [4.4, 15.1])]


@pytest.mark.parametrize('name,ckw,prof,snrs', CODED_R7, ids=['cod_vb20', 'cod_bu5x'])
def test_simulate_siso_coded_ref_compat_r7(C, golden_r7, name, ckw, prof, snrs):
    """Drop-in simulate_siso_coded in float64 == the reference: bit errors,
    received bits, CRC verdict, measured SNR, noise variance and RNG state, on
    frames it decodes and frames it does not."""
    g = golden_r7
    sim = _dropin(ckw, 'f64', itu_profile=prof)
    nb = int(g[name + '_nbits'][0])
    bits = unpack(g[name + '_bits'], nb).astype(np.int64)
    for snr in snrs:
        k = f'{name}_snr{snr}'
        r = sim.simulate_siso_coded(bits, snr)
        assert r['bit_errors'] == int(g[k + '_errors'][0]), (k, r['bit_errors'])
        assert np.array_equal(r['bits_received_array'], unpack(g[k + '_rx'], nb)), k
        assert bool(r['crc_pass']) == bool(int(g[k + '_crc'][0])), k
        assert abs(r['channel_snr_db'] - g[k + '_chsnr'][0]) < 1e-9
        assert abs(r['noise_var_mean'] / g[k + '_nvmean'][0] - 1) < 1e-12
        assert np.array_equal(_state_head(), g[k + '_state'])


@pytest.mark.parametrize('name,ckw,prof,snrs', CODED_R7, ids=['cod_vb20', 'cod_bu5x'])
def test_simulate_siso_coded_ref_compat_r7_f32(C, golden_r7, name, ckw, prof, snrs):
    """f32 fast mode on the same vectors, as test_simulate_siso_coded_ref_compat_f32:
    frames the reference decodes decode cleanly, the others fail the CRC."""
    g = golden_r7
    sim = _dropin(ckw, 'f32', itu_profile=prof)
    nb = int(g[name + '_nbits'][0])
    bits = unpack(g[name + '_bits'], nb).astype(np.int64)
    for snr in snrs:
        k = f'{name}_snr{snr}'
        r = sim.simulate_siso_coded(bits, snr)
        if int(g[k + '_errors'][0]) == 0:
            assert r['bit_errors'] == 0 and r['crc_pass'] and int(g[k + '_crc'][0]) == 1, k
        else:
            assert not r['crc_pass'] and int(g[k + '_crc'][0]) == 0, k
        assert np.array_equal(_state_head(), g[k + '_state'])


# ---------------------------------------------------------------------------
# 3. LTE_TX_STAGE is read per run, like every other switch
def test_tx_stage_switch_is_read_per_run(C, oracle, monkeypatch):
    """LTE_TX_STAGE=0, then unset, in one process on the coded per-symbol TX
    (LTE_TX_FRAME=0, k_ofdm_tx<double, 1, ..>): the path goes from the coded
    bits gathered through L1 / L2 to the stream staged in LDS, in that field
    only, and both runs give the oracle's outcome."""
    from lte_phy.engine import path_diff
    oc = oracle_case(oracle, 'siso_pb20_cod')
    plan, dr, cs = _plan(C, oc, 'f64'), oc['dr'], oc['cs']
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('LTE_TX_FRAME', '0')
    runs = []
    for stage in ('0', None):
        if stage is None:
            monkeypatch.delenv('LTE_TX_STAGE')
        else:
            monkeypatch.setenv('LTE_TX_STAGE', stage)
        r = plan.run(cs['snrs'], bits=dr['bits'], phases=dr['ph'], noise=dr['z'], capture=A_CAP)
        _compare(oracle, oc, r, A_CAP, 'f64', f'tx_stage={stage}')
        runs.append(r.path)
    assert runs[0]['tx'] == runs[1]['tx'] == _TXC
    assert (runs[0]['tx_stage'], runs[1]['tx_stage']) == ('0', '1')
    assert path_diff(*runs) == {'tx_stage'}
